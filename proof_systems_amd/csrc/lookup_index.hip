// lookup_index.hip -- the columns of LookupConstraintSystem::create (kimchi/src/circuits/lookup/index.rs:188-430, lookups.rs:222-264) and the
// row-set atoms of the lookup constraints (expr.rs:883-893), produced on the device for kh_prover_index_create_lookup (csrc/prover.cpp).
//
//   k_lookup_selectors   one thread per row of the domain: the pattern selectors from the lookup codes of rows r (CURR) and r - 1 (NEXT)
//   k_lookup_tables      one thread per row: its segment of the concatenated table from prefix offsets in the kernel arguments, then every table column,
//                        the table-id column and the runtime-table selector (gate tables generated, the caller's data copied, padding zero)
//   k_lookup_atom_den /  the three atoms over the 8n rows of d8: VanishesOnZeroKnowledgeAndPreviousRows as a product, the two unnormalised
//   k_lookup_atom_fin    Lagrange bases as (x^n - 1) / (x - a) -- denominators first (one batched inversion between the kernels), then the
//                        product with x^n - 1, which takes eight values on d8, and the limit n a^-1 where x = a
// All four are memory-bound: 256-thread blocks, consecutive rows in consecutive lanes, 32-byte element stores as in poly.hip.
#include "common.hpp"
#include "field.cuh"
#include "msm.hpp"

namespace kh {

struct Fe4q { u64 l[4]; };

// code[r]: low nibble = 1 + the pattern id row r's gate has on CURR, high nibble = 1 + the one it has on NEXT (0: none).  Pattern ids as in
// kh_prover_index_attach_lookup: 0 Xor, 1 Lookup, 2 RangeCheck, 3 ForeignFieldMul.  Rows from n_gates on are Zero rows.
struct LookupPats { u32 npat; u32 id[4]; };
template <class F>
__global__ void __launch_bounds__(256)
k_lookup_selectors(const uint8_t* __restrict__ code, size_t n_gates, size_t n, LookupPats pats, u64* __restrict__ out) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u32 cur = r < n_gates ? (u32)(code[r] & 15) : 0u;
    const u32 prv = (r > 0 && r - 1 < n_gates) ? (u32)(code[r - 1] >> 4) : 0u;
    for (u32 k = 0; k < pats.npat; k++) {
        const u32 want = pats.id[k] + 1;
        ((cur == want || prv == want) ? Fe<F>::one() : Fe<F>::zero()).store(out + 4 * (k * n + r));
    }
}

// A segment of the concatenated table, 8 words: first row | rows | element offset of its data in `data` | kind + (width << 32) | its id (4 Montgomery
// limbs).  Kinds: 0 = the caller's data, `width` columns of `rows` entries, column-major (a runtime table is such a segment of width 1: its
// second column arrives with each proof); 1 = the 12-bit range-check table (tables/range_check.rs:10-22); 2 = the 4-bit XOR table, reversed so
// that its last row is (0, 0, 0) (tables/xor.rs:9-30).  Segments are sorted by first row and contiguous from row 0.
static constexpr int SEG_WORDS = 8;
template <class F>
__device__ __forceinline__ Fe<F> small_to_mont(u32 v) {
    Fe<F> a = Fe<F>::zero(); a.v[0] = v;
    return to_mont<F>(a);
}
// The prefix offsets travel in the kernel's arguments: start[k] = the first row of segment k * stride, stride = ceil(nseg / SEG_STARTS) (1 for up to
// SEG_STARTS tables, the usual case: the segment is then found from scalar registers alone; more tables finish the search in the records).
static constexpr int SEG_STARTS = 32;
struct SegStarts { u64 start[SEG_STARTS]; u32 count, stride; };
template <class F>
__global__ void __launch_bounds__(256)
k_lookup_tables(const u64* __restrict__ segs, u32 nseg, SegStarts st, const u64* __restrict__ data, size_t n, u32 width, u64* __restrict__ tcols,
                u64* __restrict__ ids, u64* __restrict__ rtsel, size_t rt_lo, size_t rt_hi, size_t zk_lo) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    // the last segment that starts at or before r (nseg >= 1, segment 0 starts at row 0)
    u32 g = 0;
#pragma unroll
    for (u32 k = 1; k < SEG_STARTS; k++) if (k < st.count && st.start[k] <= r) g = k;
    u32 lo = g * st.stride;
    const u32 hi = lo + st.stride < nseg ? lo + st.stride : nseg;
    while (lo + 1 < hi && segs[SEG_WORDS * (lo + 1)] <= r) lo++;
    const u64* sg = segs + SEG_WORDS * lo;
    const size_t local = r - sg[0], len = sg[1];
    const bool inside = nseg > 0 && local < len;          // rows behind the last entry: zero padding, id 0
    const u32 kind = (u32)sg[3], w = (u32)(sg[3] >> 32);
    for (u32 c = 0; c < width; c++) {
        Fe<F> v = Fe<F>::zero();
        if (inside) {
            if (kind == 0) { if (c < w) v = Fe<F>::load(data + 4 * (sg[2] + (size_t)c * len + local)); }
            else if (kind == 1) { if (c == 0) v = small_to_mont<F>((u32)local); }
            else if (c < 3) { const u32 e = 255u - (u32)local, i = e >> 4, j = e & 15u; v = small_to_mont<F>(c == 0 ? i : c == 1 ? j : (i ^ j)); }
        }
        v.store(tcols + 4 * ((size_t)c * n + r));
    }
    if (ids) (inside ? Fe<F>::load(sg + 4) : Fe<F>::zero()).store(ids + 4 * r);
    if (rtsel) (((r >= rt_lo && r < rt_hi) || r >= zk_lo) ? Fe<F>::zero() : Fe<F>::one()).store(rtsel + 4 * r);
}

// x8: the evaluations of x over d8 (x8[k] = g^k, g the generator of the 8n-th roots of unity).  a = w^(n - zk_rows - 1), w = g^8.
// vanish[k] = prod_{j < nfac} (x - a w^j) (nfac = zk_rows + 1: the rows n - zk_rows - 1 .. n - 1); den0[k] = x - 1, denf[k] = x - a, each with 1
// written where it would be zero (k = 0 resp. k = kf = 8 (n - zk_rows - 1)): the quotient there is the limit k_lookup_atom_fin writes.
template <class F>
__global__ void __launch_bounds__(256)
k_lookup_atom_den(const u64* __restrict__ x8, size_t m, Fe4q a, Fe4q omega, u32 nfac, size_t kf, u64* __restrict__ vanish, u64* __restrict__ den0,
                  u64* __restrict__ denf) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const Fe<F> x = Fe<F>::load(x8 + 4 * k), fa = Fe<F>::load(a.l), w = Fe<F>::load(omega.l);
    Fe<F> t = fa, v = sub<F>(x, t);
    for (u32 j = 1; j < nfac; j++) { t = mul<F>(t, w); v = mul<F>(v, sub<F>(x, t)); }
    v.store(vanish + 4 * k);
    (k == 0 ? Fe<F>::one() : sub<F>(x, Fe<F>::one())).store(den0 + 4 * k);
    (k == kf ? Fe<F>::one() : sub<F>(x, fa)).store(denf + 4 * k);
}
// l0 / lf hold the inverted denominators; x^n - 1 on d8 is zh[k mod 8] (x^n = (g^n)^k, g^n a primitive 8th root of unity)
struct AtomZh { Fe4q zh[8]; };
template <class F>
__global__ void __launch_bounds__(256)
k_lookup_atom_fin(size_t m, AtomZh z, Fe4q lim0, Fe4q limf, size_t kf, u64* __restrict__ l0, u64* __restrict__ lf) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    Fe<F> zh = Fe<F>::load(z.zh[0].l);
#pragma unroll
    for (u32 j = 1; j < 8; j++) if ((k & 7) == j) zh = Fe<F>::load(z.zh[j].l);
    (k == 0 ? Fe<F>::load(lim0.l) : mul<F>(zh, Fe<F>::load(l0 + 4 * k))).store(l0 + 4 * k);
    (k == kf ? Fe<F>::load(limf.l) : mul<F>(zh, Fe<F>::load(lf + 4 * k))).store(lf + 4 * k);
}

int lookup_selector_columns(Context& C, int field, const uint8_t* code_dev, size_t n_gates, size_t n, const int* patterns, size_t npat, uint64_t* out_dev) {
    KH_REQUIRE(n_gates <= n && npat >= 1 && npat <= 4, "lookup_selector_columns: bad shape");
    LookupPats p; p.npat = (u32)npat;
    for (size_t k = 0; k < 4; k++) p.id[k] = k < npat ? (u32)patterns[k] : 0u;
    KH_FIELD_LAUNCH(field, k_lookup_selectors<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, C.stream, code_dev, n_gates, n, p, out_dev);
    return KH_OK;
}
int lookup_table_columns(Context& C, int field, const uint64_t* segs_dev, const uint64_t* seg_starts, size_t nseg, const uint64_t* data_dev, size_t n, size_t width,
                         uint64_t* tcols_dev, uint64_t* ids_dev, uint64_t* rtsel_dev, size_t rt_offset, size_t rt_len, size_t zk_rows) {
    KH_REQUIRE(seg_starts && nseg >= 1 && nseg < ((size_t)1 << 31) && width >= 1 && width < 256 && zk_rows < n && rt_offset + rt_len <= n, "lookup_table_columns: bad shape");
    SegStarts st; memset(&st, 0, sizeof(st));
    st.stride = (u32)((nseg + SEG_STARTS - 1) / SEG_STARTS);
    st.count = (u32)((nseg + st.stride - 1) / st.stride);
    for (u32 k = 0; k < st.count; k++) st.start[k] = seg_starts[(size_t)k * st.stride];
    KH_FIELD_LAUNCH(field, k_lookup_tables<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, C.stream, segs_dev, (u32)nseg, st, data_dev, n, (u32)width, tcols_dev, ids_dev, rtsel_dev, rt_offset,
                   rt_offset + rt_len, n - zk_rows);
    return KH_OK;
}
int lookup_atom_denominators(Context& C, int field, const uint64_t* x8_dev, size_t n, size_t zk_rows, const uint64_t a[4], const uint64_t omega[4],
                             uint64_t* atoms_dev) {
    KH_REQUIRE(zk_rows + 1 < n, "lookup_atom_denominators: bad shape");
    const size_t m = 8 * n;
    Fe4q fa, fw; memcpy(fa.l, a, 32); memcpy(fw.l, omega, 32);
    KH_FIELD_LAUNCH(field, k_lookup_atom_den<F>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, C.stream, x8_dev, m, fa, fw, (u32)(zk_rows + 1), 8 * (n - zk_rows - 1), atoms_dev, atoms_dev + 4 * m,
                   atoms_dev + 8 * m);
    return KH_OK;
}
int lookup_atom_finish(Context& C, int field, size_t n, size_t zk_rows, const uint64_t zh8[32], const uint64_t lim0[4], const uint64_t limf[4],
                       uint64_t* atoms_dev) {
    KH_REQUIRE(zk_rows + 1 < n, "lookup_atom_finish: bad shape");
    const size_t m = 8 * n;
    AtomZh z; memcpy(z.zh, zh8, sizeof(z.zh));
    Fe4q l0, lf; memcpy(l0.l, lim0, 32); memcpy(lf.l, limf, 32);
    KH_FIELD_LAUNCH(field, k_lookup_atom_fin<F>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, C.stream, m, z, l0, lf, 8 * (n - zk_rows - 1), atoms_dev + 4 * m, atoms_dev + 8 * m);
    return KH_OK;
}

}  // namespace kh
