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
//
// Lookups (kh_witness_check_full with KH_WITNESS_LOOKUPS): is every looked-up tuple of rows r < L = n - zk_rows - 1 a row of the combined table?  Exact as
// well -- no joint combiner: a tuple is (table id, up to three cells), a table row is (id, column 0, 1, 2) with every further column zero, and the two are
// compared as 4 x 32 bytes (canonical Montgomery limbs are unique).  A hash join in the style of lookup_sorted.hip, 256-thread blocks, no field arithmetic:
//   k_witness_lookup_build  thread per table row t < L.  A lookup has at most 3 cells, so a row with a non-zero value in a column >= 3 can never match and
//                           is not inserted; nor is a row equal to its predecessor in every column (the padding of the combined table is thousands of
//                           all-zero rows that would fight for one slot).  The rest: linear probing, atomicCAS(slot, EMPTY, t); a slot whose row has the
//                           same 128 bytes already stands for the key.  On the runtime rows column 1 is the proof's runtime value.
//   k_witness_lookup_probe  thread per (row r < L, joint lookup s < the most a pattern present has), one s per block row (blockIdx.y), so a wave is 64 consecutive rows: a wave none
//                           of whose rows has a pattern selector set leaves after the selector loads.  A live lane forms the tuple of joint lookup s of
//                           its pattern (WitnessLookupPattern, from PATTERNS in csrc/prover.cpp) and walks the slots; an empty slot is a miss:
//                           key = row * 64 + 8 + s -- after the wires and the gate of the same row --, detail = the pattern id, reported like the others
//                           (one atomicMin and one atomicAdd per wave with a miss -- of the wave's number of misses, one per pattern set on a row --
//                           into status word 3; none for a satisfied witness).
#include "common.hpp"
#include "field.cuh"
#include "msm.hpp"
#include "lookup_key.cuh"

namespace kh {

namespace {
struct WitnessCheckArgs {
    const u64* w;                                        // 15 witness columns of n elements
    const u64* coeffs;                                   // the index's 15 coefficient columns (d1)
    const u64* sel;                                      // the gate's selector column (d1)
    const u64* consts;                                   // the gate's constants table (as kh_gate_constants lays it out; literals and endo filled in), Montgomery limbs
    u64* status;                                         // [0] the lowest (key << 32 | detail), [1] rows with a violated gate, [2] disconnected cells, [3] lookups that miss
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
constexpr int ST_WORD = 0, ST_GATE_ROWS = 1, ST_CELLS = 2, ST_LOOKUPS = 3;

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

// ---- lookups: the hash join.  Keys are compared as bytes, hashed as in lookup_sorted.hip / host_lookup.cpp (lookup_hash.hpp)
constexpr u32 LOOKUP_EMPTY = 0xffffffffu;
constexpr u32 SUB_LOOKUP0 = 8;

// (Key, Tuple = (table id, entry 0..2), same, hash: lookup_hash.hpp; load_key: lookup_key.cuh)
__device__ __forceinline__ Key zero_key() { Key k; k.l[0] = k.l[1] = k.l[2] = k.l[3] = 0; return k; }
__device__ __forceinline__ bool is_zero(const Key& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }

// the combined table as a set of tuples: columns 0..2 (absent columns are zero), the id column (absent: every id is 0), the runtime rows' column 1
struct LookupTable {
    const u64* col[3];
    const u64* tids;
    const u64* runtime;
    u32 rt_offset, rt_len;
    __device__ __forceinline__ Tuple row(u32 t) const {
        Tuple r;
        r.k[0] = tids ? load_key(tids + 4 * (size_t)t) : zero_key();
        r.k[1] = load_key(col[0] + 4 * (size_t)t);
        if (t - rt_offset < rt_len) r.k[2] = load_key(runtime + 4 * (size_t)(t - rt_offset));
        else r.k[2] = col[1] ? load_key(col[1] + 4 * (size_t)t) : zero_key();
        r.k[3] = col[2] ? load_key(col[2] + 4 * (size_t)t) : zero_key();
        return r;
    }
};

// cols: all W columns of the table (the tail 3.. is read here only)
__global__ void __launch_bounds__(256)
k_witness_lookup_build(LookupTable T, const u64* const* __restrict__ cols, u32 W, u32 L, u32* __restrict__ slots, u32 mask) {
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (t >= L) return;
    for (u32 k = 3; k < W; k++) if (!is_zero(load_key(cols[k] + 4 * (size_t)t))) return;
    const Tuple me = T.row(t);
    if (t > 0 && same(T.row(t - 1), me)) {               // equal to its predecessor in every column (its tail must be zero too): that row inserts the key
        bool tail_zero = true;
        for (u32 k = 3; k < W; k++) tail_zero = tail_zero && is_zero(load_key(cols[k] + 4 * (size_t)(t - 1)));
        if (tail_zero) return;
    }
    u32 h = hash(me) & mask;
    for (;;) {
        u32 cur = __hip_atomic_load(&slots[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == LOOKUP_EMPTY) {
            cur = atomicCAS(&slots[h], LOOKUP_EMPTY, t);
            if (cur == LOOKUP_EMPTY) return;             // claimed
        }
        if (same(T.row(cur), me)) return;                // (a slot never changes the key it stands for: equal keys meet in one slot)
        h = (h + 1) & mask;                              // (at most L of >= 2 L slots are ever occupied: the walk ends)
    }
}

struct LookupProbeArgs {
    const u64* w;                                        // 15 witness columns of n elements
    u32 n, L, npat;
    WitnessLookupPattern pat[4];
    LookupTable T;
    const u32* slots;
    u32 mask;
    u64* status;
};
// grid: (L / 256 rounded up, the joint lookups of the largest pattern present)
__global__ void __launch_bounds__(256) k_witness_lookup_probe(LookupProbeArgs a) {
    const u32 r = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    u32 live = 0;                                        // bit k: pattern k has a joint lookup s and its selector is set on this row
    if (r < a.L) {
#pragma unroll
        for (u32 k = 0; k < 4; k++)
            if (k < a.npat && s < (u32)a.pat[k].n && !is_zero(load_key(a.pat[k].sel + 4 * (size_t)r))) live |= 1u << k;
    }
    if (!__ballot(live != 0)) return;
    u32 misses = 0;                                      // of this (row, joint lookup): one per pattern whose selector is set (a row of a sound circuit has one)
    u64 word = ~0ull;
#pragma unroll
    for (u32 k = 0; k < 4; k++) {
        if (!(live >> k & 1)) continue;
        const WitnessJointLookup& j = a.pat[k].l[s];
        Tuple v;
        if (j.tid_is_column) v.k[0] = load_key(a.w + 4 * ((size_t)j.tid_column * a.n + r));
        else { v.k[0].l[0] = j.id[0]; v.k[0].l[1] = j.id[1]; v.k[0].l[2] = j.id[2]; v.k[0].l[3] = j.id[3]; }
#pragma unroll
        for (int c = 0; c < 3; c++) v.k[1 + c] = c < j.ncell ? load_key(a.w + 4 * ((size_t)j.cells[c] * a.n + r)) : zero_key();
        u32 h = hash(v) & a.mask;
        for (;;) {
            const u32 e = a.slots[h];
            if (e == LOOKUP_EMPTY) {                     // (patterns in increasing id: the first miss is the lowest word of this lane)
                if (!misses) word = ((((u64)r << 6) | (SUB_LOOKUP0 + s)) << 32) | (u32)a.pat[k].pattern;
                misses++;
                break;
            }
            if (same(a.T.row(e), v)) break;
            h = (h + 1) & a.mask;
        }
    }
    // as report(), with the wave's sum of misses in place of the popcount of its bad lanes
    const u64 m = __ballot(misses != 0);
    if (!m) return;
    u32 total = misses;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const u32 lo = __shfl_xor((u32)word, o), hi = __shfl_xor((u32)(word >> 32), o);
        const u64 t = ((u64)hi << 32) | lo;
        word = t < word ? t : word;
        total += __shfl_xor(total, o);
    }
    if ((int)__lane_id() == __ffsll((long long)m) - 1) {
        atomicMin((unsigned long long*)&a.status[ST_WORD], (unsigned long long)word);
        atomicAdd((unsigned long long*)&a.status[ST_LOOKUPS], (unsigned long long)total);
    }
}
}  // namespace

// scratch: the status block (4 words of 64 bits, which the caller reads back) followed by the checked gates' constants tables, one after the other:
// wc_const_words(gate) = the 64-bit words before that gate's table.  With lookups, behind them: the W column addresses of the table (padded to an
// even count: the runtime values are read 16 bytes at a time), the proof's runtime values, the slots (a power of two >= 2 L of u32).
static constexpr size_t WC_STATUS_WORDS = 4;
static constexpr size_t wc_const_words(int gate) { size_t n = WC_STATUS_WORDS; for (int k = 0; k < gate; k++) n += 4 * (size_t)GATE_NCONST[k]; return n; }
size_t witness_check_scratch_bytes() { return 8 * wc_const_words(GATE_CHECKED_COUNT); }
static size_t wc_lookup_col_words(size_t W) { return (W + 1) & ~(size_t)1; }
size_t witness_check_lookup_scratch_bytes(size_t L, size_t W, size_t rt_len) { return 8 * (wc_lookup_col_words(W) + 4 * rt_len) + 4 * lookup_slots(L); }

int witness_check_num_constraints(int gate) { return gate >= 0 && gate < GATE_CHECKED_COUNT ? GATE_NCONSTRAINTS[gate] : 0; }

// sel_col[gate id] = the d1 column of that gate's selector, or -1: no launch (a gate type the circuit has no rows of).  wires_dev may be NULL (no
// wiring check), lk may be NULL (no lookup check; else scratch_dev holds witness_check_lookup_scratch_bytes more).  Queues everything on C.stream;
// the status block is then [lowest word or ~0 | rows with a violated gate | disconnected cells | lookups that miss].
int witness_check_run(Context& C, int field, const uint64_t* witness_dev, const uint64_t* d1_dev, size_t n, const int* sel_col, size_t ngate_ids,
                      size_t public_inputs, const uint64_t endo[4], const uint32_t* wires_dev, size_t n_gates, const WitnessLookups* lk, void* scratch_dev) {
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
#define KH_WITNESS_GATE_STEP(ID, NAME)                                                                                            \
    if ((size_t)ID < ngate_ids && sel_col[ID] >= 0) {                                                                             \
        a.sel = d1_dev + 4 * (size_t)sel_col[ID] * n; a.consts = status + wc_const_words(ID); a.gate = ID;                      \
        KH_FIELD_LAUNCH(field, k_witness_gate_##NAME<F>, grid, dim3(128), 0, s, a);                                               \
        C.timer.mark("check_" #NAME, s);                                                                                          \
    }
    KH_FOR_EACH_CHECKED_GATE(KH_WITNESS_GATE_STEP)
#undef KH_WITNESS_GATE_STEP
    if (wires_dev && n_gates) {
        const size_t total = 7 * n_gates;                // < 2^32: n_gates <= 2^26
        hipLaunchKernelGGL(k_witness_wires, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, s, witness_dev, wires_dev, (u32)n, (u32)total, status);
        C.timer.mark("check_wires", s);
    }
    if (lk) {
        const size_t L = lk->L, W = lk->W;
        KH_REQUIRE(L >= 1 && L < n && W >= 1 && lk->tcols && lk->npat >= 1 && lk->npat <= 4 && lk->rt_offset + lk->rt_len <= L &&
                   (!lk->rt_len || ((!lk->runtime != !lk->runtime_dev) && W >= 2)) && (((uintptr_t)lk->runtime_dev) & 15) == 0,
                   "witness_check_run: bad lookup shape");
        for (size_t k = 0; k < lk->npat; k++) {
            const WitnessLookupPattern& P = lk->pat[k];
            KH_REQUIRE(P.sel && P.n >= 0 && P.n <= 4, "witness_check_run: bad lookup pattern");
            for (int i = 0; i < P.n; i++) {
                const WitnessJointLookup& j = P.l[i];
                KH_REQUIRE(j.ncell >= 0 && j.ncell <= 3 && (!j.tid_is_column || (j.tid_column >= 0 && j.tid_column < 15)), "witness_check_run: bad joint lookup");
                for (int c = 0; c < j.ncell; c++) KH_REQUIRE(j.cells[c] >= 0 && j.cells[c] < 15, "witness_check_run: bad lookup cell");
            }
        }
        u64* const cols_dev = status + wc_const_words(GATE_CHECKED_COUNT);
        u64* const runtime_dev = cols_dev + wc_lookup_col_words(W);
        u32* const slots = (u32*)(runtime_dev + 4 * lk->rt_len);
        const size_t cap = lookup_slots(L);
        static const u64 pad = 0;
        // (runtime values that are on the device already are read where they are: their room in the scratch block stays unused)
        if ((rc = C.stage_upload(cols_dev, {{lk->tcols, W * 8}, {&pad, (wc_lookup_col_words(W) - W) * 8}, {lk->runtime, lk->runtime ? lk->rt_len * 32 : 0}}))) return rc;
        KH_HIP(hipMemsetAsync(slots, 0xff, cap * sizeof(u32), s));
        LookupTable T{};
        for (size_t k = 0; k < 3 && k < W; k++) { KH_REQUIRE(lk->tcols[k], "witness_check_run: null table column"); T.col[k] = lk->tcols[k]; }
        T.tids = lk->tids; T.runtime = lk->runtime_dev ? lk->runtime_dev : runtime_dev; T.rt_offset = (u32)lk->rt_offset; T.rt_len = (u32)lk->rt_len;
        hipLaunchKernelGGL(k_witness_lookup_build, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, s, T, (const u64* const*)cols_dev, (u32)W, (u32)L, slots, (u32)(cap - 1));
        C.timer.mark("check_lookup_build", s);
        LookupProbeArgs p{};
        p.w = witness_dev; p.n = (u32)n; p.L = (u32)L; p.npat = (u32)lk->npat;
        for (size_t k = 0; k < lk->npat; k++) p.pat[k] = lk->pat[k];
        p.T = T; p.slots = slots; p.mask = (u32)(cap - 1); p.status = status;
        int slots_y = 1;
        for (size_t k = 0; k < lk->npat; k++) slots_y = lk->pat[k].n > slots_y ? lk->pat[k].n : slots_y;
        hipLaunchKernelGGL(k_witness_lookup_probe, dim3((unsigned)((L + 255) / 256), (unsigned)slots_y), dim3(256), 0, s, p);
        C.timer.mark("check_lookup_probe", s);
    }
    KH_HIP(hipGetLastError());
    return KH_OK;
}

}  // namespace kh
