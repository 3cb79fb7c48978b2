// value_steps.hip -- the witness values no gate computes and the prover supplies as advice: the inverse of a cell, a square root, the bits of a value,
// for kh_field_inverse_dev, kh_field_sqrt_dev and kh_field_bits_dev (csrc/witness_steps.cpp).  A value step reads a dense device array and writes a
// dense device array: no witness cell, no placement.  Blocks of one wave, no LDS, no pool scratch, no per-lane scratch memory; none of the launchers
// waits for the device.
//
//   k_field_inverse   a lane holds a run of INV_RUN elements in registers: Montgomery's trick inside the run (prefix products, ONE Fermat chain
//                     -- inv_inlined of field.cuh, as k_complete_add pays per lane --, back-substitution).  Lane l of the launch takes the elements
//                     l, l + lanes, l + 2 lanes, ...: for each of them a wave's loads and stores are 64 consecutive elements.  A zero element is 1
//                     inside the run and 0 in the output.  The launch has ceil(n / (64 INV_RUN)) blocks, at most INV_MAX_BLOCKS; past
//                     INV_MAX_BLOCKS full blocks every lane works through further runs, one chain each.
//   k_field_sqrt      one lane per element: fe_sqrt of field_sqrt.cuh, every loop bounded by the 2-adicity.  The lanes of a wave take different
//                     numbers of Tonelli-Shanks rounds: the wave takes the longest of them.
//   k_field_bits      one lane per value: the canonical integer (cell_to_value of cell_format.cuh for a Montgomery element), shifted out bit by bit;
//                     bit k of every value is a store of 64 consecutive elements per wave (the output is bit-major)
#include "common.hpp"
#include "field.cuh"
#include "field_sqrt.cuh"
#include "cell_format.cuh"
#include "api_internal.hpp"

namespace kh {

__device__ __forceinline__ void raise_value_flag(u32* flags, u32 bit, bool bad) {
    if (flags && __any(bad) && (threadIdx.x & 63u) == 0) atomicOr(flags, 1u << bit);
}

// (in and out may be the same array: a lane has loaded its run before it stores it, and no other lane touches those elements)
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_field_inverse(const u64* in, size_t n, u64* out, u32* __restrict__ flags, u32 bit) {
    const size_t lanes = (size_t)gridDim.x * WAVE_BLOCK, lane = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    const Fe<F> one = Fe<F>::one();
    bool bad = false;
#pragma unroll 1
    for (size_t base = 0; base < n; base += lanes * INV_RUN) {      // (uniform across the launch)
        Fe<F> a[INV_RUN], pre[INV_RUN];
        bool zero[INV_RUN];
#pragma unroll
        for (int j = 0; j < INV_RUN; j++) {
            const size_t i = base + (size_t)j * lanes + lane;
            a[j] = one;
            if (i < n) a[j] = Fe<F>::load(in + 4 * i);
            zero[j] = a[j].is_zero();
            if (zero[j]) a[j] = one;
            pre[j] = j ? mul<F>(pre[j - 1], a[j]) : a[j];
        }
        Fe<F> t = inv_inlined<F>(pre[INV_RUN - 1]);
#pragma unroll
        for (int j = INV_RUN - 1; j >= 0; j--) {
            const size_t i = base + (size_t)j * lanes + lane;
            Fe<F> r = j ? mul<F>(t, pre[j - 1]) : t;
            if (j) t = mul<F>(t, a[j]);
            if (zero[j]) r = Fe<F>::zero();
            if (i < n) r.store(out + 4 * i);
            bad |= zero[j];
        }
    }
    raise_value_flag(flags, bit, bad);
}

template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_field_sqrt(const u64* in, size_t n, SqrtParams P, u64* out, u64* __restrict__ is_square, u32* __restrict__ flags, u32 bit) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) {
        Fe<F> r = Fe<F>::zero();
        const bool ok = fe_sqrt<F>(Fe<F>::load(in + 4 * i), P, r);
        r.store(out + 4 * i);
        if (is_square) (ok ? Fe<F>::one() : Fe<F>::zero()).store(is_square + 4 * i);
        bad = !ok;
    }
    raise_value_flag(flags, bit, bad);
}

template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_field_bits(const u64* __restrict__ in, int format, unsigned num_bits, size_t n, u64* __restrict__ out, u32* __restrict__ flags, u32 bit) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) {
        u64 w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        if (format == KH_CELL_FIELD || format == KH_CELL_INT256) {
            u64 __attribute__((aligned(16))) w[4];
            if (format == KH_CELL_FIELD) cell_to_value<F>(in + 4 * i, KH_CELL_INT256, w);
            else Fe<F>::load(in + 4 * i).store(w);
            w0 = w[0]; w1 = w[1]; w2 = w[2]; w3 = w[3];
        } else if (format == KH_CELL_U64) {
            w0 = in[i];
        } else {
            const ulonglong2 v = ((const ulonglong2*)in)[i];
            w0 = v.x; w1 = v.y;
        }
        const Fe<F> zero = Fe<F>::zero(), one = Fe<F>::one();
#pragma unroll 1
        for (unsigned k = 0; k < num_bits; k++) {
            ((w0 & 1) ? one : zero).store(out + 4 * ((size_t)k * n + i));
            w0 = (w0 >> 1) | (w1 << 63); w1 = (w1 >> 1) | (w2 << 63); w2 = (w2 >> 1) | (w3 << 63); w3 >>= 1;
        }
        bad = (w0 | w1 | w2 | w3) != 0;                             // what is left is the value over 2^num_bits
    }
    raise_value_flag(flags, bit, bad);
}

// (the callers in witness_steps.cpp have validated pointers and sizes: n >= 1; one phase of kh_last_timings per call)
int field_inverse(Context& C, int field, const uint64_t* in_dev, size_t n, uint64_t* out_dev, uint32_t* flags_dev, unsigned bit) {
    const size_t blocks = std::min((n + (size_t)WAVE_BLOCK * INV_RUN - 1) / ((size_t)WAVE_BLOCK * INV_RUN), INV_MAX_BLOCKS);
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_field_inverse<F>, dim3((unsigned)blocks), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)in_dev, n, (u64*)out_dev, flags_dev, (u32)bit);
    C.timer.mark("field_inverse", C.stream);
    return KH_OK;
}
int field_sqrt(Context& C, int field, const uint64_t* in_dev, size_t n, uint64_t* out_dev, uint64_t* out_is_square_dev, uint32_t* flags_dev, unsigned bit) {
    const SqrtParams P = sqrt_params(khost::Fld(field));
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_field_sqrt<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)in_dev, n, P, (u64*)out_dev, (u64*)out_is_square_dev,
                    flags_dev, (u32)bit);
    C.timer.mark("field_sqrt", C.stream);
    return KH_OK;
}
int field_bits(Context& C, int field, const uint64_t* in_dev, int format, unsigned num_bits, size_t n, uint64_t* out_dev, uint32_t* flags_dev, unsigned bit) {
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_field_bits<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)in_dev, format, num_bits, n, (u64*)out_dev, flags_dev,
                    (u32)bit);
    C.timer.mark("field_bits", C.stream);
    return KH_OK;
}

}  // namespace kh
