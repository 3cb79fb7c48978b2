// gates.hip -- the gate library's combined constraints as compiled kernels (kh_gate_evaluations_dev).
//
// prover.rs:824-868 evaluates, for every gate type, index(gate) * sum_i alpha^i constraint_i over the d8 columns.  csrc/expr.hip can run any
// such expression as a token program, but its operand stack and Store / Load slots live in LDS, which caps the Poseidon / VarBaseMul / EndoMulScalar
// programs at one wave per SIMD (16-30 G products/s).  The gate library is protocol data fixed at build time, so tools/gen_gate_kernels.py lowers
// the SAME expression DAGs (proof_systems_amd/polish.py) to straight-line functions (gates_gen.inc: gate_constraints_<Name>): every intermediate
// value a register-resident field element, common sub-expressions once, no interpreter.  Those functions hand each finished constraint to a sink;
// the one here (QuotientSink) sums multiplier_i * constraint_i, and the kernel multiplies by the selector -- csrc/witness_check.hip runs the same
// functions with a sink that compares.  One kernel per (gate, field); thread per row; columns 0..14 = witness, 15..29 = coefficients, 30 = the
// gate's selector; the constants table is the one polish.gate_program returns (literals, MDS, endo, powers of alpha).
// Bound: VALU issue (products of 254 instructions), as everywhere in this library.
#include "common.hpp"
#include "field.cuh"
#include "msm.hpp"
#include "host_ec.hpp"

namespace kh {

struct GateArgs {
    const u64* cols[31];
    const u64* consts;
    size_t rows, len;
    u32 stride, next_shift;
    int accumulate;
    u64* out;
};
template <class F>
struct GateCtx {
    const GateArgs& a;
    size_t i0, i1;                                       // element index of this row / of the next row in every column
    __device__ __forceinline__ Fe<F> cell(int c, int nxt) const { return Fe<F>::load(a.cols[c] + 4 * (nxt ? i1 : i0)); }
    __device__ __forceinline__ Fe<F> cst(int k) const { return Fe<F>::load(a.consts + 4 * k); }
};

#include "gates_gen.inc"

// acc = sum_i cst(SLOT[i]) * constraint_i: SLOT = the gate's GATE_MULT_SLOT, the table slots of alpha^i (of the two per-proof values for Generic)
template <class F, class G, const int* SLOT>
struct QuotientSink {
    const G& g;
    Fe<F> acc;
    template <int I>
    __device__ __forceinline__ void constraint(const Fe<F>& v) {
        const Fe<F> t = mul<F>(g.cst(SLOT[I]), v);
        if constexpr (I == 0) acc = t; else acc = add<F>(acc, t);
    }
};
#define KH_GATE_VALUE(ID, NAME)                                                                               \
    template <class F, class G>                                                                               \
    __device__ __forceinline__ Fe<F> gate_##NAME(const G& g) {                                                \
        QuotientSink<F, G, GATE_MULT_SLOT_##NAME> s{g, {}};                                                   \
        gate_constraints_##NAME<F>(g, s);                                                                     \
        return mul<F>(g.cell(30, 0), s.acc);                                                                  \
    }
KH_FOR_EACH_CHECKED_GATE(KH_GATE_VALUE)

#define KH_GATE_KERNEL(ID, NAME)                                                                              \
    template <class F>                                                                                        \
    __global__ void __launch_bounds__(128) k_gate_##NAME(GateArgs a) {                                        \
        const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;                                              \
        const size_t row = i < a.rows ? i : a.rows - 1;                                                       \
        size_t i0 = (size_t)a.stride * row, i1 = i0 + a.next_shift;                                           \
        if (i1 >= a.len) i1 -= a.len;                                                                         \
        const GateCtx<F> g{a, i0, i1};                                                                        \
        Fe<F> v = gate_##NAME<F>(g);                                                                          \
        if (i < a.rows) {                                                                                     \
            if (a.accumulate) v = add<F>(Fe<F>::load(a.out + 4 * i), v);                                      \
            v.store(a.out + 4 * i);                                                                           \
        }                                                                                                     \
    }
KH_FOR_EACH_GATE(KH_GATE_KERNEL)

// The same bodies with one constants table PER ROW: the verifier's constant term of the linearisation (kimchi/src/verifier.rs:412-490) for a batch of
// proofs.  Item i of the batch is rows 2i (the proof's evaluations at zeta) and 2i + 1 (at zeta omega) of every column, its table -- alpha differs
// from proof to proof -- the i-th of `consts`; thread per item, one launch per gate type present in the batch, all accumulating into one k-element
// output.  No LDS, no atomics.
struct GateBatchArgs {
    const u64* cols[31];
    const u64* consts;                                   // items x nconst x 4 limbs
    size_t items;
    int nconst, accumulate;
    u64* out;
};
template <class F>
struct GateBatchCtx {
    const GateBatchArgs& a;
    const u64* tab;                                      // this item's constants table
    size_t i0, i1;
    __device__ __forceinline__ Fe<F> cell(int c, int nxt) const { return Fe<F>::load(a.cols[c] + 4 * (nxt ? i1 : i0)); }
    __device__ __forceinline__ Fe<F> cst(int k) const { return Fe<F>::load(tab + 4 * k); }
};
#define KH_GATE_BATCH_KERNEL(ID, NAME)                                                                        \
    template <class F>                                                                                        \
    __global__ void __launch_bounds__(128) k_gate_batch_##NAME(GateBatchArgs a) {                             \
        const size_t t = (size_t)blockIdx.x * 128 + threadIdx.x;                                              \
        const size_t i = t < a.items ? t : a.items - 1;                                                       \
        const GateBatchCtx<F> g{a, a.consts + 4 * i * (size_t)a.nconst, 2 * i, 2 * i + 1};                    \
        Fe<F> v = gate_##NAME<F>(g);                                                                          \
        if (t < a.items) {                                                                                    \
            if (a.accumulate) v = add<F>(Fe<F>::load(a.out + 4 * i), v);                                      \
            v.store(a.out + 4 * i);                                                                           \
        }                                                                                                     \
    }
KH_FOR_EACH_CHECKED_GATE(KH_GATE_BATCH_KERNEL)

int gate_count() { return GATE_COUNT; }
const char* gate_name(int gate) { return gate >= 0 && gate < GATE_COUNT ? GATE_NAMES[gate] : nullptr; }
int gate_num_constants(int gate) { return gate >= 0 && gate < GATE_COUNT ? GATE_NCONST[gate] : -1; }

// the constants table of one gate for one proof, on the host (gates_gen.inc: GATE_CONST_TABLE): literals of the protocol, powers of alpha, the endo
// coefficient, the caller's per-proof values -- so that a caller needs no copy of the expression builder to drive kh_gate_evaluations_dev.
// fixed_only: the literals and the endo coefficient alone, the other slots of `out` left as they are (all that the constraints themselves read)
static int fill_constants(int field, int gate, bool fixed_only, const uint64_t* alpha, const uint64_t* endo, const uint64_t* params, size_t nparams, uint64_t* out) {
    KH_REQUIRE(gate >= 0 && gate < GATE_COUNT, "unknown gate id %d", gate);
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field %d", field);
    const khost::Fld F(field == KH_FIELD_FP ? 0 : 1);
    const GateConst* rc = GATE_CONST_TABLE[gate];
    khost::fe apow[64]; int have = 0;                     // alpha^1 .. alpha^have
    for (int k = 0; k < GATE_NCONST[gate]; k++) {
        khost::fe v;
        if (fixed_only && rc[k].kind != 0 && rc[k].kind != 2) continue;
        switch (rc[k].kind) {
            case 0: { khost::fe c; for (int i = 0; i < 4; i++) c.l[i] = rc[k].lit[field == KH_FIELD_FP ? 0 : 1][i]; v = F.to_mont(c); break; }
            case 1: {
                KH_REQUIRE(alpha, "gate %s needs alpha", GATE_NAMES[gate]);
                KH_REQUIRE(rc[k].arg >= 1 && rc[k].arg < 64, "bad power in the constants recipe");
                if (!have) { memcpy(&apow[1], alpha, 32); have = 1; }
                while (have < rc[k].arg) { apow[have + 1] = F.mul(apow[have], apow[1]); have++; }
                v = apow[rc[k].arg]; break;
            }
            case 2: KH_REQUIRE(endo, "gate %s needs the endo coefficient", GATE_NAMES[gate]); memcpy(&v, endo, 32); break;
            default:
                KH_REQUIRE(params && (size_t)rc[k].arg < nparams, "gate %s takes %d per-proof values, got %zu", GATE_NAMES[gate], rc[k].arg + 1, nparams);
                memcpy(&v, params + 4 * (size_t)rc[k].arg, 32); break;
        }
        memcpy(out + 4 * (size_t)k, &v, 32);
    }
    return KH_OK;
}
int gate_constants(int field, int gate, const uint64_t* alpha, const uint64_t* endo, const uint64_t* params, size_t nparams, uint64_t* out) {
    return fill_constants(field, gate, false, alpha, endo, params, nparams, out);
}
int gate_fixed_constants(int field, int gate, const uint64_t* endo, uint64_t* out) { return fill_constants(field, gate, true, nullptr, endo, nullptr, 0, out); }

#define g_gate_consts (kh::ctx().scratch("gate_consts"))

int gate_run(Context& C, int field, int gate, const uint64_t* const* cols_dev, size_t len, const uint64_t* consts, size_t nconsts, size_t rows,
             unsigned stride, unsigned next_shift, int accumulate, uint64_t* out_dev) {
    KH_REQUIRE(gate >= 0 && gate < GATE_COUNT, "unknown gate id %d", gate);
    KH_REQUIRE((int)nconsts == GATE_NCONST[gate], "gate %s takes %d constants (polish.gate_program), got %zu", GATE_NAMES[gate], GATE_NCONST[gate], nconsts);
    KH_REQUIRE(len > 0 && (size_t)stride * (rows ? rows - 1 : 0) < len && next_shift < len, "rows * stride must not exceed the column length (%zu rows, stride %u, length %zu)", rows, stride, len);
    if (rows == 0) return KH_OK;
    int rc;
    if ((rc = g_gate_consts.reserve(GATE_COUNT * 64 * 32))) return rc;
    // a slot of the constants scratch per gate: consecutive gate launches of one proof do not overwrite each other's table while queued
    u64* d_consts = g_gate_consts.as<u64>() + (size_t)gate * 64 * 4;
    if ((rc = C.stage_upload(d_consts, {{consts, nconsts * 32}}))) return rc;
    GateArgs a{};
    for (int c = 0; c < 31; c++) { KH_REQUIRE(cols_dev[c], "column %d is null", c); a.cols[c] = cols_dev[c]; }
    a.consts = d_consts; a.rows = rows; a.len = len; a.stride = stride; a.next_shift = next_shift; a.accumulate = accumulate; a.out = out_dev;
    hipStream_t s = C.stream;
    dim3 grid((unsigned)((rows + 127) / 128));
    C.timer.begin(s);
    switch (gate) {
#define KH_GATE_CASE(ID, NAME) case ID: KH_FIELD_LAUNCH(field, k_gate_##NAME<F>, grid, dim3(128), 0, s, a); break;
        KH_FOR_EACH_GATE(KH_GATE_CASE)
#undef KH_GATE_CASE
        default: break;
    }
    C.timer.mark("gate", s);
    return KH_OK;
}

#define g_gate_batch (kh::ctx().scratch("gate_batch"))

// cols_host: ncols columns of 2 * items elements (witness 0..14, coefficients 15..29, then the selector columns the launches name); launches: per gate type its
// selector column and the items' constants tables (items x kh_gate_num_constants x 4 limbs, host).  ONE staged upload of columns + tables, one launch per
// gate type, all accumulating into out_dev (items elements, on the main stream); the caller downloads it.  *cols_dev: where the columns are on the device
// (column c at + 8 c items limbs), valid until the context's next gate_batch_run -- the lookup programs of kh_batch_verify read them there.
int gate_batch_run(Context& C, int field, const uint64_t* cols_host, size_t ncols, size_t items, const GateBatchLaunch* launches, size_t nl, uint64_t* out_dev,
                   const uint64_t** cols_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field %d", field);
    KH_REQUIRE(cols_host && launches && out_dev && items > 0 && nl > 0 && ncols > 30, "gate_batch_run: bad argument");
    const size_t col_bytes = ncols * 2 * items * 32;
    size_t total = col_bytes;
    for (size_t l = 0; l < nl; l++) {
        KH_REQUIRE(launches[l].gate >= 0 && launches[l].gate < GATE_CHECKED_COUNT && launches[l].consts, "gate_batch_run: unknown gate id %d", launches[l].gate);
        KH_REQUIRE(launches[l].selector_col >= 30 && (size_t)launches[l].selector_col < ncols, "gate_batch_run: selector column %d of %zu", launches[l].selector_col, ncols);
        total += items * (size_t)GATE_NCONST[launches[l].gate] * 32;
    }
    int rc;
    if ((rc = g_gate_batch.reserve(total))) return rc;
    u64* base = g_gate_batch.as<u64>();
    std::vector<u64> blob(total / 8);
    memcpy(blob.data(), cols_host, col_bytes);
    size_t off = col_bytes / 8;
    std::vector<size_t> tab_off(nl);
    for (size_t l = 0; l < nl; l++) {
        const size_t words = items * (size_t)GATE_NCONST[launches[l].gate] * 4;
        memcpy(blob.data() + off, launches[l].consts, words * 8);
        tab_off[l] = off; off += words;
    }
    if ((rc = C.stage_upload(base, {{blob.data(), total}}))) return rc;
    hipStream_t s = C.stream;
    dim3 grid((unsigned)((items + 127) / 128));
    C.timer.begin(s);
    for (size_t l = 0; l < nl; l++) {
        GateBatchArgs a{};
        for (int c = 0; c < 30; c++) a.cols[c] = base + (size_t)c * 2 * items * 4;
        a.cols[30] = base + (size_t)launches[l].selector_col * 2 * items * 4;
        a.consts = base + tab_off[l]; a.items = items; a.nconst = GATE_NCONST[launches[l].gate]; a.accumulate = l > 0; a.out = out_dev;
        switch (launches[l].gate) {
#define KH_GATE_BATCH_CASE(ID, NAME) case ID: KH_FIELD_LAUNCH(field, k_gate_batch_##NAME<F>, grid, dim3(128), 0, s, a); break;
            KH_FOR_EACH_CHECKED_GATE(KH_GATE_BATCH_CASE)
#undef KH_GATE_BATCH_CASE
            default: break;
        }
    }
    C.timer.mark("gate_batch", s);
    if (cols_dev) *cols_dev = base;
    return KH_OK;
}

}  // namespace kh
