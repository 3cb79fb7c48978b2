// wiring.hip -- what joins two gadgets on the device: single witness cells read into and written from the input formats of the gadget calls, and the
// generic rows between them (kimchi/src/circuits/polynomials/generic.rs; oracle/circuit.py::generic_spec has the coefficient order), for
// kh_witness_gather_dev, kh_witness_scatter_dev and kh_generic_witness_dev (csrc/witness_steps.cpp).  include/kimchi_hip.h has the formats.
//
// Every kernel is ONE LANE PER CELL (or generic instance) in blocks of one wave.  A cell is one 32-byte element at an arbitrary (row, column): two
// 16-byte accesses per lane that share a 32-byte sector and nothing else with their neighbours', whatever the launch shape -- the witness side moves
// a sector per cell, the cell list 8 bytes.  The dense side (out_dev, values_dev, l_dev, r_dev) is consecutive across the wave: 32, 16 or 8 bytes per
// lane.  Spreading a cell over several lanes would split the one Montgomery product its conversion costs; several cells per lane would leave a
// circuit's worth of wires (a few thousand cells) on a handful of CUs.
//
//   k_cell_gather     cell -> value: KH_CELL_FIELD copies; every other format is from_mont (the reduction half of a product), the low words out, the
//                     high words tested for the flag
//   k_cell_scatter    value -> cell: KH_CELL_FIELD copies; every other format is one product by R^2; a KH_CELL_INT256 value is compared with p, a
//                     KH_CELL_LIMB88 value with 2^88, for the flag
//   k_cell_moves      a witness schedule's group of consecutive gathers (or scatters) over its arena in ONE launch: a 16-byte record per lane carries
//                     the cell, the format, the step's flag bit and the value's place in the arena; the conversions are the two above
//   k_generic_half    l, r -> l, r, o = l (c_l' + c_m' r) + c_r' r + c_c' with the four coefficients already divided by -c_o on the host (all zero
//                     when c_o = 0: o = 0): three products, three additions, no inversion on the device
// In the direct kernels the format is a kernel argument: the branches on it are uniform, and a lane diverges from its wave only to raise the flag.
#include "common.hpp"
#include "field.cuh"
#include "cell_format.cuh"
#include "api_internal.hpp"

namespace kh {

// cell i of a list of (row, column) pairs in the 15 columns at `witness`
struct CellList {
    const u32* cells;
    size_t col_stride;
    __device__ __forceinline__ size_t offset(size_t i) const {
        const uint2 rc = ((const uint2*)cells)[i];
        return 4 * ((size_t)rc.y * col_stride + rc.x);
    }
};
__device__ __forceinline__ void raise_cell_flag(u32* flags, u32 bit, bool bad) {
    if (flags && __any(bad) && (threadIdx.x & 63u) == 0) atomicOr(flags, 1u << bit);
}
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_cell_gather(const u64* __restrict__ witness, CellList at, size_t n, int format, u64* __restrict__ out, u32* __restrict__ flags, u32 bit) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) bad = cell_to_value<F>(witness + at.offset(i), format, out + cell_words(format) * i);
    raise_cell_flag(flags, bit, bad);
}

template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_cell_scatter(const u64* __restrict__ values, int format, CellList at, size_t n, u64* __restrict__ witness, u32* __restrict__ flags, u32 bit) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) bad = value_to_cell<F>(values + cell_words(format) * i, format, witness + at.offset(i));
    raise_cell_flag(flags, bit, bad);
}

// A group of a witness schedule's wire steps in one launch: lane i carries move i, whatever step it came from.  One 16-byte record per lane, one
// load: row | column, format, flag bit | the dense side's word offset in the arena.  Format and flag bit are per lane: the lanes of a wave branch on
// the format where a group changes it, and their flag masks are ORed across the wave into at most one atomicOr.
template <class F, bool SCATTER>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_cell_moves(const CellMove* __restrict__ moves, size_t n, u64* witness, size_t col_stride, u64* arena, u32* __restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    u32 mask = 0;
    if (i < n) {
        const uint4 m = ((const uint4*)moves)[i];
        const int format = (int)((m.y >> 4) & 7u);
        const u32 flag = (m.y >> 8) & 63u;
        u64* const cell = witness + 4 * ((size_t)(m.y & 15u) * col_stride + m.x);
        u64* const dense = arena + ((u64)m.z | ((u64)m.w << 32));
        const bool bad = SCATTER ? value_to_cell<F>(dense, format, cell) : cell_to_value<F>(cell, format, dense);
        if (bad && flag < 32) mask = 1u << flag;
    }
    if (flags && __any(mask != 0)) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mask |= (u32)__shfl_xor((int)mask, off);
        if ((threadIdx.x & 63u) == 0) atomicOr(flags, mask);
    }
}

template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_generic_half(const u64* l_in, const u64* r_in, size_t n, GenericHalf co, unsigned col0, WitnessPlace at, u64* out) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const Fe<F> l = Fe<F>::load(l_in + 4 * i), r = r_in ? Fe<F>::load(r_in + 4 * i) : Fe<F>::zero();
    const Fe<F> cl = Fe<F>::load(co.l[0]), cr = Fe<F>::load(co.l[1]), cm = Fe<F>::load(co.l[2]), cc = Fe<F>::load(co.l[3]);
    const Fe<F> o = add<F>(add<F>(mul<F>(l, add<F>(cl, mul<F>(cm, r))), mul<F>(cr, r)), cc);
    const size_t row = at.start_row(i);
    l.store(at.cell(row, col0)); r.store(at.cell(row, col0 + 1)); o.store(at.cell(row, col0 + 2));
    if (out) o.store(out + 4 * i);
}

// (the callers in witness_steps.cpp have validated pointers, sizes and every cell; one phase of kh_last_timings per call)
int cell_gather(Context& C, int field, const uint64_t* witness_dev, size_t col_stride, const uint32_t* cells_dev, size_t n, int format, uint64_t* out_dev,
                uint32_t* flags_dev, unsigned bit) {
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_cell_gather<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)witness_dev, (CellList{cells_dev, col_stride}), n,
                    format, (u64*)out_dev, flags_dev, (u32)bit);
    C.timer.mark("cell_gather", C.stream);
    return KH_OK;
}
int cell_scatter(Context& C, int field, const uint64_t* values_dev, int format, const uint32_t* cells_dev, size_t n, uint64_t* witness_dev, size_t col_stride,
                 uint32_t* flags_dev, unsigned bit) {
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_cell_scatter<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)values_dev, format,
                    (CellList{cells_dev, col_stride}), n, (u64*)witness_dev, flags_dev, (u32)bit);
    C.timer.mark("cell_scatter", C.stream);
    return KH_OK;
}
int cell_moves(Context& C, int field, bool scatter, const CellMove* moves_dev, size_t n, uint64_t* witness_dev, size_t col_stride, uint64_t* arena_dev,
               uint32_t* flags_dev) {
    C.timer.begin(C.stream);
    if (scatter) KH_FIELD_LAUNCH(field, (k_cell_moves<F, true>), blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, moves_dev, n, (u64*)witness_dev, col_stride,
                                 (u64*)arena_dev, flags_dev);
    else KH_FIELD_LAUNCH(field, (k_cell_moves<F, false>), blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, moves_dev, n, (u64*)witness_dev, col_stride,
                         (u64*)arena_dev, flags_dev);
    C.timer.mark(scatter ? "cell_moves_scatter" : "cell_moves_gather", C.stream);
    return KH_OK;
}
GenericHalf generic_fold(int field, const uint64_t* coeffs) {
    const khost::Fld F(field);
    khost::fe c[5];
    memcpy(c, coeffs, sizeof(c));                                   // l r o m c
    GenericHalf co;
    memset(&co, 0, sizeof(co));
    if (!khost::is_zero(c[2])) {
        const khost::fe scale = F.neg(F.inv(c[2]));
        const khost::fe folded[4] = {F.mul(c[0], scale), F.mul(c[1], scale), F.mul(c[3], scale), F.mul(c[4], scale)};
        memcpy(co.l, folded, sizeof(co.l));
    }
    return co;
}
int generic_rows_prepared(Context& C, int field, const GenericHalf& co, int half, const uint64_t* l_dev, const uint64_t* r_dev, size_t n, const WitnessPlace& at,
                          uint64_t* out_dev) {
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_generic_half<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)l_dev, (const u64*)r_dev, n, co,
                    (unsigned)(3 * half), at, (u64*)out_dev);
    C.timer.mark("generic", C.stream);
    return KH_OK;
}

}  // namespace kh
