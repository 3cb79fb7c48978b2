// witness_check.hip -- ProverIndex::verify / ConstraintSystem::verify (kimchi/src/circuits/constraints.rs) on the device, for kh_witness_check
// (csrc/prover.cpp): which row of a witness is the first that does not satisfy the circuit, and why.
//
// Everything the check reads is resident already: the index's d1 columns (coefficients, one selector column per gate type), the device copy of the
// gate list's wires a created index keeps, and the witness.  Nothing here is probabilistic: every constraint of a row is evaluated on its own and
// compared with zero limb for limb (values of field.cuh are fully reduced, so "all eight limbs zero" is exact) -- no alpha, no selector product.
//
//   k_witness_gate_<Name>   one kernel per (gate type, field); thread per row, stride 1 over the d1 columns: witness 0..14, coefficients 15..29.  A wave
//                           none of whose rows has the gate's selector set leaves after that one 32-byte load per lane -- a Kimchi row has ONE gate
//                           type, so that is most waves of every kernel but one.  The live rows run gates_gen.inc's gate_constraints_<Name>, the
//                           same function the quotient kernels of csrc/gates.hip run, with a sink (CheckSink) that compares instead of summing:
//                           bit i of the result = constraint i is not zero.  `next` of row n - 1 is row 0.  Generic subtracts the row's public
//                           input, which is by definition the witness's own cell w[0][r] for r < public_inputs, from its first constraint.
//   k_witness_wires         thread per (row, column < 7) of the n_gates recorded rows: the cell's 32 bytes against those of the cell it is wired to
//                           (padding rows are wired to themselves and need no thread; nor does a recorded cell wired to itself).
//
// Reporting.  A violating lane forms key = row * 64 + sub, sub = 0..6 for a disconnected cell of that column, 7 for the row's gate: the lowest key is
// the reference's order (rows upwards, within a row the wires by column before the gate).  The status word is (key << 32) | detail -- detail = the row's
// constraint mask and gate id, or the cell the column is wired to -- so that the minimum carries its own description and nothing is read twice
// (n <= 2^26 rows: the key fits 32 bits).  A wave reduces its words with shuffles and issues ONE 64-bit atomicMin, and one atomicAdd of its popcount
// into the counter of violated rows resp. disconnected cells; a wave without a violation issues no atomic, so a satisfied witness issues none at all.
// Bound: the live gate's VALU issue (products of 254 instructions); the other kernels are one strided 32-byte load per row.
#include "common.hpp"
#include "field.cuh"
#include "msm.hpp"

namespace kh {

namespace {
struct WitnessCheckArgs {
    const u64* w;                                        // 15 witness columns of n elements
    const u64* coeffs;                                   // the index's 15 coefficient columns (d1)
    const u64* sel;                                      // the gate's selector column (d1)
    const u64* consts;                                   // the gate's constants table (as kh_gate_constants lays it out; literals and endo filled in), Montgomery limbs
    u64* status;                                         // [0] the lowest (key << 32 | detail), [1] rows with a violated gate, [2] disconnected cells
    u32 n, pub, gate;
};
template <class F>
struct GateCtx {
    const WitnessCheckArgs& a;
    u32 r0, r1;                                          // this row / the next one
    __device__ __forceinline__ Fe<F> cell(int c, int nxt) const {
        const u64* col = c < 15 ? a.w + 4 * (size_t)c * a.n : a.coeffs + 4 * (size_t)(c - 15) * a.n;
        return Fe<F>::load(col + 4 * (size_t)(nxt ? r1 : r0));
    }
    __device__ __forceinline__ Fe<F> cst(int k) const { return Fe<F>::load(a.consts + 4 * k); }
    __device__ __forceinline__ Fe<F> public_input() const { return r0 < a.pub ? Fe<F>::load(a.w + 4 * (size_t)r0) : Fe<F>::zero(); }
};

#include "gates_gen.inc"

// bit i of m = constraint i is not zero.  GENERIC: the public input of the row (zero past the public rows) belongs to the first constraint
template <class F, bool GENERIC>
struct CheckSink {
    const GateCtx<F>& g;
    u32 m;
    template <int I>
    __device__ __forceinline__ void constraint(const Fe<F>& v) {
        if constexpr (GENERIC && I == 0) m |= (sub<F>(v, g.public_input()).is_zero() ? 0u : 1u) << I;
        else m |= (v.is_zero() ? 0u : 1u) << I;
    }
};

constexpr u32 SUB_GATE = 7;
constexpr int ST_WORD = 0, ST_GATE_ROWS = 1, ST_CELLS = 2;

// Called by every lane of the wave.  bad lanes hold `word`; the wave's lowest goes to the status word, its number of bad lanes to status[counter].
__device__ __forceinline__ void report(u64* status, bool bad, u64 word, int counter) {
    const u64 m = __ballot(bad);
    if (!m) return;
    u64 v = bad ? word : ~0ull;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const u32 lo = __shfl_xor((u32)v, o), hi = __shfl_xor((u32)(v >> 32), o);
        const u64 t = ((u64)hi << 32) | lo;
        v = t < v ? t : v;
    }
    if ((int)__lane_id() == __ffsll((long long)m) - 1) {
        atomicMin((unsigned long long*)&status[ST_WORD], (unsigned long long)v);
        atomicAdd((unsigned long long*)&status[counter], (unsigned long long)__popcll(m));
    }
}

#define KH_WITNESS_GATE_KERNEL(ID, NAME)                                                                        \
    template <class F>                                                                                          \
    __global__ void __launch_bounds__(128) k_witness_gate_##NAME(WitnessCheckArgs a) {                          \
        const u32 i = blockIdx.x * 128 + threadIdx.x;                                                           \
        const bool live = i < a.n && !Fe<F>::load(a.sel + 4 * (size_t)i).is_zero();                             \
        if (!__ballot(live)) return;                                                                            \
        const GateCtx<F> g{a, i, i + 1 < a.n ? i + 1 : 0};                                                      \
        CheckSink<F, ID == GATE_ID_GENERIC> s{g, 0};                                                            \
        if (live) gate_constraints_##NAME<F>(g, s);                                                             \
        report(a.status, s.m != 0, ((((u64)i << 6) | SUB_GATE) << 32) | ((u64)a.gate << 24) | s.m, ST_GATE_ROWS); \
    }
KH_FOR_EACH_CHECKED_GATE(KH_WITNESS_GATE_KERNEL)

// wires: per recorded row 7 (row, column) pairs.  total = 7 * n_gates threads.
__global__ void __launch_bounds__(128)
k_witness_wires(const u64* __restrict__ w, const u32* __restrict__ wires, u32 n, u32 total, u64* __restrict__ status) {
    const u32 t = blockIdx.x * 128 + threadIdx.x;
    bool bad = false;
    u64 word = ~0ull;
    if (t < total) {
        const u32 r = t / 7, c = t - 7 * r;
        const u32 r2 = wires[2 * (size_t)t], c2 = wires[2 * (size_t)t + 1];
        if (r2 != r || c2 != c) {                        // (kh_prover_index_create refused a wire with r2 >= n or c2 >= 7)
            const uint4* p = (const uint4*)(w + 4 * ((size_t)c * n + r));
            const uint4* q = (const uint4*)(w + 4 * ((size_t)c2 * n + r2));
            const uint4 a0 = p[0], a1 = p[1], b0 = q[0], b1 = q[1];
            bad = ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w)) != 0;
            word = ((((u64)r << 6) | c) << 32) | ((u64)c2 << 28) | r2;
        }
    }
    report(status, bad, word, ST_CELLS);
}
}  // namespace

// scratch: the status block (4 words of 64 bits; the caller reads the first three back) followed by the checked gates' constants tables, one after
// the other: wc_const_words(gate) = the 64-bit words before that gate's table
static constexpr size_t WC_STATUS_WORDS = 4;
static constexpr size_t wc_const_words(int gate) { size_t n = WC_STATUS_WORDS; for (int k = 0; k < gate; k++) n += 4 * (size_t)GATE_NCONST[k]; return n; }
size_t witness_check_scratch_bytes() { return 8 * wc_const_words(GATE_CHECKED_COUNT); }

int witness_check_num_constraints(int gate) { return gate >= 0 && gate < GATE_CHECKED_COUNT ? GATE_NCONSTRAINTS[gate] : 0; }

// sel_col[gate id] = the d1 column of that gate's selector, or -1: no launch (a gate type the circuit has no rows of).  wires_dev may be NULL (no
// wiring check).  Queues everything on C.stream; the status block is then [lowest word or ~0 | rows with a violated gate | disconnected cells].
int witness_check_run(Context& C, int field, const uint64_t* witness_dev, const uint64_t* d1_dev, size_t n, const int* sel_col, size_t ngate_ids,
                      size_t public_inputs, const uint64_t endo[4], const uint32_t* wires_dev, size_t n_gates, void* scratch_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field %d", field);
    KH_REQUIRE(witness_dev && d1_dev && sel_col && endo && scratch_dev && n >= 2 && n <= ((size_t)1 << 26) && n_gates <= n, "witness_check_run: bad argument");
    static_assert(GATE_CHECKED_COUNT <= 16, "the gate id takes four bits of the status word");
    // one upload: the cleared status block and every gate's constants (the multiplier slots, which the sink here never reads, stay zero)
    std::vector<uint64_t> host(witness_check_scratch_bytes() / 8, 0);
    host[ST_WORD] = ~0ull;
    int rc;
    for (int k = 0; k < GATE_CHECKED_COUNT; k++)
        if ((rc = gate_fixed_constants(field, k, endo, &host[wc_const_words(k)]))) return rc;
    if ((rc = C.stage_upload(scratch_dev, {{host.data(), host.size() * 8}}))) return rc;
    u64* const status = (u64*)scratch_dev;
    WitnessCheckArgs a{};
    a.w = witness_dev; a.coeffs = d1_dev; a.status = status; a.n = (u32)n; a.pub = (u32)(public_inputs < n ? public_inputs : n);
    hipStream_t s = C.stream;
    const dim3 grid((unsigned)((n + 127) / 128));
    C.timer.begin(s);
#define KH_WITNESS_GATE_LAUNCH(ID, NAME)                                                                                          \
    if ((size_t)ID < ngate_ids && sel_col[ID] >= 0) {                                                                             \
        a.sel = d1_dev + 4 * (size_t)sel_col[ID] * n; a.consts = status + wc_const_words(ID); a.gate = ID;                      \
        if (field == KH_FIELD_FP) hipLaunchKernelGGL((k_witness_gate_##NAME<FpParams>), grid, dim3(128), 0, s, a);                \
        else hipLaunchKernelGGL((k_witness_gate_##NAME<FqParams>), grid, dim3(128), 0, s, a);                                     \
        C.timer.mark("check_" #NAME, s);                                                                                          \
    }
    KH_FOR_EACH_CHECKED_GATE(KH_WITNESS_GATE_LAUNCH)
#undef KH_WITNESS_GATE_LAUNCH
    if (wires_dev && n_gates) {
        const size_t total = 7 * n_gates;                // < 2^32: n_gates <= 2^26
        hipLaunchKernelGGL(k_witness_wires, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, s, witness_dev, wires_dev, (u32)n, (u32)total, status);
        C.timer.mark("check_wires", s);
    }
    KH_HIP(hipGetLastError());
    return KH_OK;
}

}  // namespace kh
