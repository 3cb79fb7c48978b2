// curve_gadgets.hip -- the witness rows of the curve gates on the device: CompleteAdd, VarBaseMul, EndoMul, EndoMulScalar
// (kimchi/src/circuits/polynomials/{complete_add,varbasemul,endosclmul,endomul_scalar}.rs; oracle/gates.py restates their generators), for
// kh_complete_add_witness_dev, kh_varbasemul_witness_dev, kh_endomul_witness_dev and kh_endomul_scalar_witness_dev (csrc/witness_steps.cpp).
//
//   k_complete_add        one lane per instance, ONE Fermat inversion: the two denominators a row may need are inverted as their product
//   k_endomul_scalar      one lane per instance, additions only
//   k_chain               VarBaseMul / EndoMul, one lane per instance: the accumulator's walk acc -> acc + Q -> (acc + Q) + acc in XYZZ, no inversion;
//                         every acc_j goes to scratch with D_j = zzz_j (x_Q zz_j - x_j), the one value per step whose inverse yields 1 / zzz_j
//                         (the affine acc_j) AND 1 / (x_j - x_Q) (the slope s1)
//   k_endo_inv_denoms     EndoMul, one lane per (row, instance): E = (X_p ZZ_r - X_r ZZ_p)(X_r ZZ_s - X_s ZZ_r), the denominator of the row's `inv`
//   (poly_batch_inversion over all D and E of the slice: two scans and one inversion on the host; zeros stay zero)
//   k_varbasemul_cells,
//   k_endomul_cells       one lane per (step, instance): the affine accumulator, the slope and the bits into their cells
// The four kernels that write witness cells take where the instances land as one WitnessPlace (api_internal.hpp): at.start_row(i), at.cell(row, column).
//
// The reference inverts twice per bit (s1, s2); s2 is never written, and acc' = (acc + Q) + acc does not need it.  No lane of these kernels has a
// Fermat inversion on its chain but k_complete_add's one: the chain of a 255-bit VarBaseMul is 255 x (madd + add + 2) = 6630 products instead of
// 510 x 380.  A zero denominator (the reference panics) leaves a zero among the D / E: the batch inversion skips it, the lane that meets the zero
// sets the caller's flag, and every other instance is exact.
#include "common.hpp"
#include "curve.cuh"
#include "api_internal.hpp"

namespace kh {

struct GadgetConst { u64 l[4]; };
static constexpr int CELLS_BLOCK = 256;

template <class F>
__device__ __forceinline__ Fe<F> sel(bool c, const Fe<F>& a, const Fe<F>& b) {
    Fe<F> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}
// bit `pos` of a little-endian scalar of u64 words
__device__ __forceinline__ bool scalar_bit(const u64* s, unsigned pos) { return (s[pos >> 6] >> (pos & 63)) & 1; }
// ((s mod 2^num_bits) >> sh) mod p as a Montgomery element: the running n of the gates (NW words, num_bits <= 64 NW, sh <= num_bits <= 255, value < 2^255 < 2 p)
template <class F, int NW>
__device__ __forceinline__ Fe<F> scalar_prefix(const u64* s, unsigned num_bits, unsigned sh) {
    const unsigned ws = sh >> 6, bs = sh & 63;
    u32 t[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u64 w[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const unsigned idx = k + ws + h;
            u64 v = 0;
            if (idx < NW && 64 * idx < num_bits) {
                v = s[idx];
                if (num_bits - 64 * idx < 64) v &= ((u64)1 << (num_bits - 64 * idx)) - 1;
            }
            w[h] = v;
        }
        const u64 o = bs ? (w[0] >> bs) | (w[1] << (64 - bs)) : w[0];
        t[2 * k] = (u32)o; t[2 * k + 1] = (u32)(o >> 32);
    }
    return to_mont<F>(cond_sub_p<F>(t));
}

// ---------------------------------------------------------------------------------------------------------- CompleteAdd
// complete_add_witness: cells 0..10 = x1 y1 x2 y2 x3 y3 inf same_x s inf_z x21_inv.  The denominators: x2 - x1 (generic), 2 y1 (same x), and
// y2 - y1 as well for P + (-P) -- inverted together, 1 / (d1 d2) times the other one.
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_complete_add(const u64* __restrict__ p1, const u64* __restrict__ p2, size_t n, WitnessPlace at, u64* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const Aff<F> a = Aff<F>::load(p1 + 8 * i), b = Aff<F>::load(p2 + 8 * i);
    const Fe<F> dx = sub<F>(b.x, a.x), dy = sub<F>(b.y, a.y);
    const bool same_x = dx.is_zero(), opposite = same_x && !dy.is_zero();
    const Fe<F> d1 = sel<F>(same_x, dbl<F>(a.y), dx), d2 = sel<F>(opposite, dy, Fe<F>::one());
    const Fe<F> t = inv_inlined<F>(mul<F>(d1, d2));
    const Fe<F> i1 = mul<F>(t, d2), i2 = mul<F>(t, d1);
    const Fe<F> xx = sqr<F>(a.x);
    const Fe<F> s = mul<F>(sel<F>(same_x, add<F>(dbl<F>(xx), xx), dy), i1);
    const Fe<F> x3 = sub<F>(sub<F>(sqr<F>(s), a.x), b.x);
    const Fe<F> y3 = sub<F>(mul<F>(s, sub<F>(a.x, x3)), a.y);
    const size_t r = at.start_row(i);
    const Fe<F> zero = Fe<F>::zero(), one = Fe<F>::one();
    a.x.store(at.cell(r, 0)); a.y.store(at.cell(r, 1));
    b.x.store(at.cell(r, 2)); b.y.store(at.cell(r, 3));
    x3.store(at.cell(r, 4)); y3.store(at.cell(r, 5));
    sel<F>(opposite, one, zero).store(at.cell(r, 6));
    sel<F>(same_x, one, zero).store(at.cell(r, 7));
    s.store(at.cell(r, 8));
    sel<F>(opposite, i2, zero).store(at.cell(r, 9));
    sel<F>(same_x, zero, i1).store(at.cell(r, 10));
    if (out) { x3.store(out + 8 * i); y3.store(out + 8 * i + 4); }
}

// -------------------------------------------------------------------------------------------------------- EndoMulScalar
// endomul_scalar gen_witness: 8 crumbs per row, most significant first; cells 0..13 = n0 n8 a0 b0 a8 b8 x0..x7
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_endomul_scalar(const u64* __restrict__ chals, unsigned num_bits, size_t n, WitnessPlace at, GadgetConst endo_scalar, u64* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64* const sc = chals + 2 * i;
    const Fe<F> zero = Fe<F>::zero(), one = Fe<F>::one(), minus_one = neg<F>(one), two = dbl<F>(one), three = add<F>(two, one);
    Fe<F> a = two, b = two, nacc = zero;
    size_t r = at.start_row(i);
    unsigned pos = num_bits;                          // the next bit is pos - 1
#pragma unroll 1
    for (unsigned row = 0; row < num_bits / 16; row++, r++) {
        nacc.store(at.cell(r, 0)); a.store(at.cell(r, 2)); b.store(at.cell(r, 3));
#pragma unroll 1
        for (unsigned j = 0; j < 8; j++) {
            const bool b1 = scalar_bit(sc, pos - 1), b0 = scalar_bit(sc, pos - 2);
            pos -= 2;
            const Fe<F> crumb = sel<F>(b1, sel<F>(b0, three, two), sel<F>(b0, one, zero));
            const Fe<F> sgn = sel<F>(b0, one, minus_one);
            a = dbl<F>(a); b = dbl<F>(b);
            const Fe<F> a1 = add<F>(a, sgn), b1v = add<F>(b, sgn);
            a = sel<F>(b1, a1, a); b = sel<F>(b1, b, b1v);
            nacc = add<F>(dbl<F>(dbl<F>(nacc)), crumb);
            crumb.store(at.cell(r, 6 + j));
        }
        nacc.store(at.cell(r, 1)); a.store(at.cell(r, 4)); b.store(at.cell(r, 5));
    }
    if (out) add<F>(mul<F>(a, Fe<F>::load(endo_scalar.l)), b).store(out + 4 * i);
}

// ------------------------------------------------------------------------------------------------ VarBaseMul and EndoMul
// Scratch of a slice of m instances with E accumulators each (num_bits + 1, or num_bits / 2 + 1 for EndoMul): the planes X, Y, ZZ, ZZZ of E x m
// elements (entry j of instance i at j m + i: a wave stores 2 KiB in a row), then the inversion vector: D (E x m) and, for EndoMul, the num_bits / 4 x m
// denominators of `inv`.
struct ChainScratch { u64 *x, *y, *zz, *zzz, *den; };

// Step j adds Q_j twice-and-once: acc <- (acc + Q_j) + acc.  VarBaseMul: Q = base if the bit is 1, -base otherwise (varbasemul.rs:356-395); EndoMul: two
// bits per step, Q = (b ? endo x_T : x_T, (2 b' - 1) y_T) (endosclmul.rs:606-690).  The bits leave a 256-bit shift register by its top end; Q is built
// with per-lane selects, and madd always adds (negate = false): no call is divergent.  The exceptional branches of madd / add are taken by degenerate
// instances only.
template <class F, bool ENDO>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_chain(const u64* __restrict__ base, const u64* __restrict__ acc0, const u64* __restrict__ scalars, unsigned num_bits, size_t m, GadgetConst endo,
        ChainScratch S) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (i >= m) return;
    constexpr int NW = ENDO ? 4 : 8;                  // 32-bit words of a scalar
    u32 w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = 0;
    {
        const u32* const sc = (const u32*)scalars + NW * i;
#pragma unroll
        for (int k = 0; k < NW; k++) w[8 - NW + k] = sc[k];
    }
    auto next_bit = [&]() -> bool {
        const bool bit = w[7] >> 31;
#pragma unroll
        for (int k = 7; k > 0; k--) w[k] = (w[k] << 1) | (w[k - 1] >> 31);
        w[0] <<= 1;
        return bit;
    };
#pragma unroll 1
    for (unsigned k = 32 * NW; k > num_bits; k--) (void)next_bit();       // bit num_bits - 1 to the top
    const Aff<F> T = Aff<F>::load(base + 8 * i);
    const Fe<F> neg_y = neg<F>(T.y);
    const Fe<F> endo_x = ENDO ? mul<F>(Fe<F>::load(endo.l), T.x) : T.x;
    Xyzz<F> acc = Xyzz<F>::from_affine(Aff<F>::load(acc0 + 8 * i));
    const unsigned steps = ENDO ? num_bits / 2 : num_bits;
    size_t at = 4 * i;
#pragma unroll 1
    for (unsigned j = 0; j < steps; j++, at += 4 * m) {
        Aff<F> Q;
        Q.x = T.x;
        if (ENDO) Q.x = sel<F>(next_bit(), endo_x, T.x);
        Q.y = sel<F>(next_bit(), T.y, neg_y);
        acc.x.store(S.x + at); acc.y.store(S.y + at); acc.zz.store(S.zz + at); acc.zzz.store(S.zzz + at);
        mul<F>(acc.zzz, sub<F>(mul<F>(Q.x, acc.zz), acc.x)).store(S.den + at);
        const Xyzz<F> r = madd<F>(acc, Q, false);
        acc = add<F>(r, acc);
    }
    acc.x.store(S.x + at); acc.y.store(S.y + at); acc.zz.store(S.zz + at); acc.zzz.store(S.zzz + at);
    acc.zzz.store(S.den + at);
}

// x_p - x_r = (X_p ZZ_r - X_r ZZ_p) / (ZZ_p ZZ_r): the row's inv = 1 / ((x_p - x_r)(x_r - x_s)) = ZZ_p ZZ_r^2 ZZ_s / E
template <class F>
__global__ void __launch_bounds__(CELLS_BLOCK)
k_endo_inv_denoms(ChainScratch S, size_t m, size_t nrows, size_t entries) {
    const size_t t = (size_t)blockIdx.x * CELLS_BLOCK + threadIdx.x;
    if (t >= nrows * m) return;
    const size_t r = t / m, i = t - r * m, p = 4 * (2 * r * m + i), q = p + 4 * m, s = q + 4 * m;
    const Fe<F> xp = Fe<F>::load(S.x + p), zp = Fe<F>::load(S.zz + p), xr = Fe<F>::load(S.x + q), zr = Fe<F>::load(S.zz + q);
    const Fe<F> xs = Fe<F>::load(S.x + s), zs = Fe<F>::load(S.zz + s);
    const Fe<F> c1 = sub<F>(mul<F>(xp, zr), mul<F>(xr, zp)), c2 = sub<F>(mul<F>(xr, zs), mul<F>(xs, zr));
    mul<F>(c1, c2).store(S.den + 4 * (entries * m + t));
}

// What both cell kernels do with entry j of instance i once D_j is inverted: the affine accumulator and, before the last entry, the slope
// s1 = (y - y_Q) / (x - x_Q) = (y_Q zzz - Y) zz / D.  A D that was zero is still zero: `degenerate`.
template <class F>
struct Entry { Fe<F> x, y, s; bool degenerate; };
template <class F>
__device__ __forceinline__ Entry<F> entry_values(const ChainScratch& S, size_t at, bool last, const Fe<F>& qx, const Fe<F>& qy) {
    const Fe<F> X = Fe<F>::load(S.x + at), Y = Fe<F>::load(S.y + at), ZZ = Fe<F>::load(S.zz + at), ZZZ = Fe<F>::load(S.zzz + at);
    const Fe<F> dinv = Fe<F>::load(S.den + at);
    Entry<F> e;
    e.degenerate = dinv.is_zero();
    const Fe<F> izzz = last ? dinv : mul<F>(dinv, sub<F>(mul<F>(qx, ZZ), X));
    e.x = mul<F>(X, sqr<F>(mul<F>(izzz, ZZ)));                                  // 1 / zz = (zz / zzz)^2
    e.y = mul<F>(Y, izzz);
    e.s = mul<F>(mul<F>(sub<F>(mul<F>(qy, ZZZ), Y), ZZ), dinv);
    return e;
}

// varbasemul_witness: chunk c of 5 bits is rows r0 = start + 2 c and r0 + 1.  Entry j = 5 c + k: acc_j into r0 (columns 2 3 | 7 8 | 9 10 | 11 12 | 13 14 by k),
// bit and s1 into r0 + 1 (2 + k, 7 + k); k == 0 also writes base (0, 1) and n before / after the chunk (4, 5) of r0, and, from the second chunk on and
// for the last entry, acc_j into cells 0, 1 of the row before: the previous chunk's output.
template <class F>
__global__ void __launch_bounds__(CELLS_BLOCK)
k_varbasemul_cells(ChainScratch S, const u64* __restrict__ base, const u64* __restrict__ scalars, unsigned num_bits, size_t m,
                   WitnessPlace at, size_t first, u64* __restrict__ out_acc, u64* __restrict__ out_n, u32* __restrict__ flags, u32 bit) {
    const size_t t = (size_t)blockIdx.x * CELLS_BLOCK + threadIdx.x;
    bool degenerate = false;
    if (t < ((size_t)num_bits + 1) * m) {
        const size_t j = t / m, i = t - j * m;
        const bool last = j == num_bits;
        const u64* const sc = scalars + 4 * i;
        const bool b = !last && scalar_bit(sc, num_bits - 1 - (unsigned)j);
        const Aff<F> T = Aff<F>::load(base + 8 * i);
        const Entry<F> e = entry_values<F>(S, 4 * t, last, T.x, sel<F>(b, T.y, neg<F>(T.y)));
        degenerate = e.degenerate;
        const size_t c = j / 5, k = j - 5 * c, r0 = at.start_row(first + i) + 2 * c;
        if (!last) {
            const size_t xc = k == 0 ? 2 : 5 + 2 * k;
            e.x.store(at.cell(r0, xc)); e.y.store(at.cell(r0, xc + 1));
            sel<F>(b, Fe<F>::one(), Fe<F>::zero()).store(at.cell(r0 + 1, 2 + k));
            e.s.store(at.cell(r0 + 1, 7 + k));
            if (k == 0) {
                T.x.store(at.cell(r0, 0)); T.y.store(at.cell(r0, 1));
                scalar_prefix<F, 4>(sc, num_bits, num_bits - (unsigned)j).store(at.cell(r0, 4));
                scalar_prefix<F, 4>(sc, num_bits, num_bits - (unsigned)j - 5).store(at.cell(r0, 5));
            }
        }
        if (k == 0 && j > 0) { e.x.store(at.cell(r0 - 1, 0)); e.y.store(at.cell(r0 - 1, 1)); }
        if (last) {
            if (out_acc) { e.x.store(out_acc + 8 * (first + i)); e.y.store(out_acc + 8 * (first + i) + 4); }
            if (out_n) scalar_prefix<F, 4>(sc, num_bits, 0).store(out_n + 4 * (first + i));
        }
    }
    if (flags && __any(degenerate) && (threadIdx.x & 63u) == 0) atomicOr(flags, 1u << bit);
}

// endomul_witness: row r = start + h / 2 holds entries h = 2 r (x_p y_p in 4, 5; s1 in 9; with it x_T y_T in 0, 1, n in 6 and the four bits in 11..14)
// and 2 r + 1 (x_r y_r in 7, 8; s3 in 10; with it inv in 2); the last entry is the closing row: 0, 1, 4, 5, 6.
template <class F>
__global__ void __launch_bounds__(CELLS_BLOCK)
k_endomul_cells(ChainScratch S, const u64* __restrict__ base, const u64* __restrict__ chals, unsigned num_bits, size_t m, GadgetConst endo,
                WitnessPlace at, size_t first, u64* __restrict__ out_acc, u64* __restrict__ out_n, u32* __restrict__ flags, u32 bit) {
    const size_t t = (size_t)blockIdx.x * CELLS_BLOCK + threadIdx.x;
    const size_t entries = num_bits / 2 + 1;
    bool degenerate = false;
    if (t < entries * m) {
        const size_t h = t / m, i = t - h * m;
        const bool last = h + 1 == entries;
        const u64* const sc = chals + 2 * i;
        const unsigned top = num_bits - 1 - 2 * (unsigned)h;                     // the step's first bit (the x choice); the sign is the one below
        const bool bx = !last && scalar_bit(sc, top), by = !last && scalar_bit(sc, top - 1);
        const Aff<F> T = Aff<F>::load(base + 8 * i);
        const Fe<F> qx = bx ? mul<F>(Fe<F>::load(endo.l), T.x) : T.x;
        const Entry<F> e = entry_values<F>(S, 4 * t, last, qx, sel<F>(by, T.y, neg<F>(T.y)));
        degenerate = e.degenerate;
        const size_t r = at.start_row(first + i) + h / 2;
        const Fe<F> zero = Fe<F>::zero(), one = Fe<F>::one();
        if (h & 1) {
            e.x.store(at.cell(r, 7)); e.y.store(at.cell(r, 8)); e.s.store(at.cell(r, 10));
            const Fe<F> einv = Fe<F>::load(S.den + 4 * (entries * m + (h / 2) * m + i));
            degenerate |= einv.is_zero();
            const Fe<F> zp = Fe<F>::load(S.zz + 4 * (t - m)), zr = Fe<F>::load(S.zz + 4 * t), zs = Fe<F>::load(S.zz + 4 * (t + m));
            mul<F>(mul<F>(einv, sqr<F>(zr)), mul<F>(zp, zs)).store(at.cell(r, 2));
        } else {
            T.x.store(at.cell(r, 0)); T.y.store(at.cell(r, 1));
            e.x.store(at.cell(r, 4)); e.y.store(at.cell(r, 5));
            const Fe<F> nacc = scalar_prefix<F, 2>(sc, num_bits, num_bits - 2 * (unsigned)h);
            nacc.store(at.cell(r, 6));
            if (!last) {
                e.s.store(at.cell(r, 9));
                sel<F>(bx, one, zero).store(at.cell(r, 11)); sel<F>(by, one, zero).store(at.cell(r, 12));
                sel<F>(scalar_bit(sc, top - 2), one, zero).store(at.cell(r, 13));
                sel<F>(scalar_bit(sc, top - 3), one, zero).store(at.cell(r, 14));
            } else {
                if (out_acc) { e.x.store(out_acc + 8 * (first + i)); e.y.store(out_acc + 8 * (first + i) + 4); }
                if (out_n) nacc.store(out_n + 4 * (first + i));
            }
        }
    }
    if (flags && __any(degenerate) && (threadIdx.x & 63u) == 0) atomicOr(flags, 1u << bit);
}

// (the callers in witness_steps.cpp have validated pointers and sizes: n <= WAVE_BLOCK_MAX_N keeps the grids inside 31 bits; the phases of kh_last_timings
// are complete_add, endomul_scalar and, per slice, chain, denominators, cells)
int complete_add_rows(Context& C, int field, const uint64_t* p1_dev, const uint64_t* p2_dev, size_t n, const WitnessPlace& at, uint64_t* out_dev) {
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_complete_add<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, p1_dev, p2_dev, n, at, out_dev);
    C.timer.mark("complete_add", C.stream);
    return KH_OK;
}
int endomul_scalar_rows(Context& C, int field, const uint64_t* chals_dev, unsigned num_bits, size_t n, const WitnessPlace& at, const uint64_t* endo_scalar,
                        uint64_t* out_dev) {
    GadgetConst es; memset(&es, 0, sizeof(es));
    if (endo_scalar) memcpy(es.l, endo_scalar, 32);
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_endomul_scalar<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, chals_dev, num_bits, n, at, es, out_dev);
    C.timer.mark("endomul_scalar", C.stream);
    return KH_OK;
}

// The scratch of kh_varbasemul_witness_dev / kh_endomul_witness_dev: a slice of instances at a time, as many as keep the slice's inversion vector within
// CHAIN_SLICE_ELEMS elements (what one scan takes); 160 bytes per accumulator (+ 32 per EndoMul row).
static constexpr size_t CHAIN_SLICE_ELEMS = (size_t)1 << 22;
static std::atomic<size_t> g_slice_elems{CHAIN_SLICE_ELEMS};          // kh_curve_witness_set_slice_elements
void chain_set_slice_elements(size_t elems) { g_slice_elems.store(elems == 0 || elems > CHAIN_SLICE_ELEMS ? CHAIN_SLICE_ELEMS : elems, std::memory_order_relaxed); }
static size_t chain_entries(bool endo, unsigned num_bits) { return endo ? num_bits / 2 + 1 : (size_t)num_bits + 1; }
static size_t chain_inversions(bool endo, unsigned num_bits) { return chain_entries(endo, num_bits) + (endo ? num_bits / 4 : 0); }
size_t chain_slice(bool endo, unsigned num_bits, size_t n) {
    size_t m = g_slice_elems.load(std::memory_order_relaxed) / chain_inversions(endo, num_bits);
    if (m > WAVE_BLOCK) m -= m % WAVE_BLOCK;
    return std::min(n, std::max<size_t>(m, 1));
}
size_t chain_scratch_bytes(bool endo, unsigned num_bits, size_t n) {
    return 32 * chain_slice(endo, num_bits, n) * (4 * chain_entries(endo, num_bits) + chain_inversions(endo, num_bits));
}
int chain_rows(Context& C, int field, bool is_endo, const uint64_t* endo, const uint64_t* base_dev, const uint64_t* acc0_dev, const uint64_t* scalars_dev,
               unsigned num_bits, size_t n, const WitnessPlace& at, uint64_t* out_acc_dev, uint64_t* out_n_dev, uint32_t* flags_dev, unsigned bit,
               uint64_t* scratch_dev, size_t scratch_bytes) {
    GadgetConst en; memset(&en, 0, sizeof(en));
    if (endo) memcpy(en.l, endo, 32);
    const size_t slice = std::min(chain_slice(is_endo, num_bits, n), scratch_bytes / (32 * (4 * chain_entries(is_endo, num_bits) + chain_inversions(is_endo, num_bits))));
    const size_t entries = chain_entries(is_endo, num_bits), words = is_endo ? 2 : 4;
    C.timer.begin(C.stream);
    for (size_t first = 0; first < n; first += slice) {
        const size_t m = std::min(slice, n - first), plane = 4 * entries * m;
        ChainScratch S;
        S.x = (u64*)scratch_dev; S.y = S.x + plane; S.zz = S.y + plane; S.zzz = S.zz + plane; S.den = S.zzz + plane;
        const u64 *b = (const u64*)base_dev + 8 * first, *a = (const u64*)acc0_dev + 8 * first, *s = (const u64*)scalars_dev + words * first;
        if (is_endo) {
            KH_FIELD_LAUNCH(field, (k_chain<F, true>), blocks_of(m, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, b, a, s, num_bits, m, en, S);
            KH_FIELD_LAUNCH(field, k_endo_inv_denoms<F>, blocks_of((num_bits / 4) * m, CELLS_BLOCK), dim3(CELLS_BLOCK), 0, C.stream, S, m, (size_t)(num_bits / 4), entries);
        } else KH_FIELD_LAUNCH(field, (k_chain<F, false>), blocks_of(m, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, b, a, s, num_bits, m, en, S);
        C.timer.mark("chain", C.stream);
        int rc = poly_batch_inversion(C, field, (uint64_t*)S.den, chain_inversions(is_endo, num_bits) * m);
        if (rc) return rc;
        C.timer.mark("denominators", C.stream);
        if (is_endo)
            KH_FIELD_LAUNCH(field, k_endomul_cells<F>, blocks_of(entries * m, CELLS_BLOCK), dim3(CELLS_BLOCK), 0, C.stream, S, b, s, num_bits, m, en, at, first,
                            out_acc_dev, out_n_dev, flags_dev, (u32)bit);
        else
            KH_FIELD_LAUNCH(field, k_varbasemul_cells<F>, blocks_of(entries * m, CELLS_BLOCK), dim3(CELLS_BLOCK), 0, C.stream, S, b, s, num_bits, m, at, first,
                            out_acc_dev, out_n_dev, flags_dev, (u32)bit);
        C.timer.mark("cells", C.stream);
    }
    return KH_OK;
}

}  // namespace kh
