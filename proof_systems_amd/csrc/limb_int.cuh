// limb_int.cuh -- fixed-width unsigned integers of 32-bit words for the limb gadgets (csrc/limb_gadgets.hip): the 88-bit limbs of a foreign-field element,
// their 176-bit products, the 528-bit product of two elements and its division by the foreign modulus.  Plain C++ with compile-time word counts and
// compile-time indices only (every loop unrolls, every array lives in registers); no field arithmetic, so the same code runs on the host, where
// kh_foreign_field_mul_witness_dev computes the Barrett constant and tests/cpp/test_limb_int.cpp checks the division against big integers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KH_LIMB_FN __host__ __device__ __forceinline__
#else
#define KH_LIMB_FN inline
#endif

namespace kh {
namespace limb {

typedef uint32_t u32;
typedef uint64_t u64;

static constexpr int LIMB_BITS = 88;

template <int N>
struct Wide { u32 w[N]; };

template <int N>
KH_LIMB_FN Wide<N> zero() {
    Wide<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.w[i] = 0;
    return r;
}
// zero-extended or truncated to N words
template <int N, int M>
KH_LIMB_FN Wide<N> resize(const Wide<M>& a) {
    Wide<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.w[i] = i < M ? a.w[i < M ? i : 0] : 0u;
    return r;
}
template <int N>
KH_LIMB_FN Wide<N> from_u64(u64 lo, u64 hi = 0) {
    Wide<N> r = zero<N>();
    r.w[0] = (u32)lo;
    if (N > 1) r.w[N > 1 ? 1 : 0] = (u32)(lo >> 32);
    if (N > 2) r.w[N > 2 ? 2 : 0] = (u32)hi;
    if (N > 3) r.w[N > 3 ? 3 : 0] = (u32)(hi >> 32);
    return r;
}
template <int N>
KH_LIMB_FN Wide<N> add(const Wide<N>& a, const Wide<N>& b) {                 // mod 2^(32 N)
    Wide<N> r; u64 c = 0;
#pragma unroll
    for (int i = 0; i < N; i++) { c += (u64)a.w[i] + b.w[i]; r.w[i] = (u32)c; c >>= 32; }
    return r;
}
template <int N>
KH_LIMB_FN Wide<N> sub(const Wide<N>& a, const Wide<N>& b, u32* borrow = nullptr) {     // mod 2^(32 N); *borrow = (a < b)
    Wide<N> r; u32 br = 0;
#pragma unroll
    for (int i = 0; i < N; i++) { const u64 d = (u64)a.w[i] - b.w[i] - br; r.w[i] = (u32)d; br = (u32)(d >> 63); }
    if (borrow) *borrow = br;
    return r;
}
template <int N>
KH_LIMB_FN bool ge(const Wide<N>& a, const Wide<N>& b) { u32 br; (void)sub<N>(a, b, &br); return br == 0; }
template <int N>
KH_LIMB_FN bool is_zero(const Wide<N>& a) {
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < N; i++) o |= a.w[i];
    return o == 0;
}
template <int N>
KH_LIMB_FN Wide<N> select(bool c, const Wide<N>& a, const Wide<N>& b) {
    Wide<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.w[i] = c ? a.w[i] : b.w[i];
    return r;
}
// a >> S and a << S for a compile-time S (words that leave the N are lost)
template <int S, int N>
KH_LIMB_FN Wide<N> shr(const Wide<N>& a) {
    constexpr int ws = S / 32, bs = S % 32;
    Wide<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const u32 lo = i + ws < N ? a.w[i + ws < N ? i + ws : 0] : 0u, hi = i + ws + 1 < N ? a.w[i + ws + 1 < N ? i + ws + 1 : 0] : 0u;
        r.w[i] = bs ? (lo >> bs) | (hi << ((32 - bs) & 31)) : lo;
    }
    return r;
}
template <int S, int N>
KH_LIMB_FN Wide<N> shl(const Wide<N>& a) {
    constexpr int ws = S / 32, bs = S % 32;
    Wide<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const u32 hi = i >= ws ? a.w[i >= ws ? i - ws : 0] : 0u, lo = i >= ws + 1 ? a.w[i >= ws + 1 ? i - ws - 1 : 0] : 0u;
        r.w[i] = bs ? (hi << bs) | (lo >> ((32 - bs) & 31)) : hi;
    }
    return r;
}
// the low BITS bits of a
template <int BITS, int N>
KH_LIMB_FN Wide<N> low_bits(const Wide<N>& a) {
    Wide<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.w[i] = 32 * (i + 1) <= BITS ? a.w[i] : 32 * i >= BITS ? 0u : a.w[i] & ((1u << (BITS % 32)) - 1u);
    return r;
}
// words SKIP .. SKIP + NO - 1 of a * b, exact (product scanning from column 0: one 64 x 32-bit accumulator with a carry word per column)
template <int NO, int SKIP, int NA, int NB>
KH_LIMB_FN Wide<NO> mul_words(const Wide<NA>& a, const Wide<NB>& b) {
    Wide<NO> r;
    u64 lo = 0; u32 hi = 0;
#pragma unroll
    for (int k = 0; k < SKIP + NO; k++) {
#pragma unroll
        for (int i = 0; i < NA; i++) {
            const int j = k - i;
            if (j >= 0 && j < NB) {
                const u64 t = (u64)a.w[i] * b.w[j >= 0 && j < NB ? j : 0];
                lo += t; hi += lo < t ? 1u : 0u;
            }
        }
        if (k >= SKIP) r.w[k >= SKIP ? k - SKIP : 0] = (u32)lo;
        lo = (lo >> 32) | ((u64)hi << 32); hi = 0;
    }
    return r;
}
template <int NO, int NA, int NB>
KH_LIMB_FN Wide<NO> mul(const Wide<NA>& a, const Wide<NB>& b) { return mul_words<NO, 0, NA, NB>(a, b); }

// ---- foreign-field elements: three 88-bit limbs, 264 bits in 9 words ----
typedef Wide<3> Limb;        // < 2^88 where it is one
typedef Wide<6> Prod;        // sums of a few limb products: < 2^192
typedef Wide<9> Elem;        // a foreign element, a quotient, a remainder
struct Limbs { Limb l[3]; };

KH_LIMB_FN Elem pack(const Limbs& x) {
    return add<9>(resize<9>(x.l[0]), add<9>(shl<LIMB_BITS>(resize<9>(x.l[1])), shl<2 * LIMB_BITS>(resize<9>(x.l[2]))));
}
KH_LIMB_FN Limbs unpack(const Elem& x) {                 // x < 2^264
    Limbs r;
    r.l[0] = low_bits<LIMB_BITS>(resize<3>(x));
    r.l[1] = low_bits<LIMB_BITS>(resize<3>(shr<LIMB_BITS>(x)));
    r.l[2] = low_bits<LIMB_BITS>(resize<3>(shr<2 * LIMB_BITS>(x)));
    return r;
}

// What the division of kh_foreign_field_mul_witness_dev needs of the modulus, computed once on the host: f, mu = floor(2^528 / f) (529 bits for f = 1)
// and the limbs of 2^264 - f.
struct FfModulus { Elem f; Wide<17> mu; Limbs nf; Limb f2; };

// (q, r) = divmod(a b, f) for a, b < 2^264 by Barrett's estimate with the FULL product: qe = floor(a b mu / 2^528) > a b / f - 1 - a b / 2^528, so
// q - 1 <= qe <= q and one conditional correction, a select, makes it exact: no lane diverges.  The columns 0..15 of a b mu are computed for their
// carries only.  q_overflow: q >= 2^264, i.e. (a b >> 264) >= f; then q
// and r are not meaningful (the caller flags the instance).
struct DivMod { Elem q, r; bool q_overflow; };
KH_LIMB_FN DivMod ff_divmod(const Elem& a, const Elem& b, const FfModulus& m) {
    const Wide<17> p = mul<17>(a, b);
    DivMod d;
    d.q_overflow = ge<9>(resize<9>(shr<3 * LIMB_BITS>(p)), m.f);
    const Wide<10> top = mul_words<10, 16>(p, m.mu);                       // bits 512 .. 831 of p mu
    Elem q = resize<9>(shr<16>(top));                                     // bits 528 .. 815: the estimate (< 2^264 unless q_overflow)
    Elem r = sub<9>(resize<9>(p), mul<9>(q, m.f));                        // < 2 f < 2^265
    Elem one = zero<9>(); one.w[0] = 1;
    const bool over = ge<9>(r, m.f);
    d.q = select<9>(over, add<9>(q, one), q);
    d.r = select<9>(over, sub<9>(r, m.f), r);
    return d;
}

// The cells of a ForeignFieldMul gate and its next row that are not copies of the inputs (foreign_field_mul/witness.rs: compute_witness_variables), from
// a, b, q, r and the negated modulus nf = 2^264 - f in limbs:
//   p0 = a0 b0 + q0 nf0, p1 = a0 b1 + a1 b0 + q0 nf1 + q1 nf0, p2 = a0 b2 + a2 b0 + a1 b1 + q0 nf2 + q2 nf0 + q1 nf1          (< 2^179)
//   p1 = p1_lo + 2^88 (p1_hi0 + 2^88 p1_hi1), carry0 = (p0 + 2^88 p1_lo - r0 - 2^88 r1) >> 176, carry1 = (p2 + p1_hi + carry0 - r2) >> 88
// a b + q nf = r + 2^264 q makes both differences non-negative multiples of the power they are shifted by.
struct FfMulCells { Limb p1_lo, p1_hi0, carry1, bound; u32 p1_hi1, carry0; Prod r01; bool overflow; };
KH_LIMB_FN Prod limb_mul(const Limb& x, const Limb& y) { return mul<6>(x, y); }
KH_LIMB_FN FfMulCells ff_mul_cells(const Limbs& a, const Limbs& b, const Limbs& q, const Limbs& r, const FfModulus& m) {
    const Limbs& nf = m.nf;
    const Prod p0 = add<6>(limb_mul(a.l[0], b.l[0]), limb_mul(q.l[0], nf.l[0]));
    const Prod p1 = add<6>(add<6>(limb_mul(a.l[0], b.l[1]), limb_mul(a.l[1], b.l[0])), add<6>(limb_mul(q.l[0], nf.l[1]), limb_mul(q.l[1], nf.l[0])));
    const Prod p2 = add<6>(add<6>(add<6>(limb_mul(a.l[0], b.l[2]), limb_mul(a.l[2], b.l[0])), add<6>(limb_mul(a.l[1], b.l[1]), limb_mul(q.l[0], nf.l[2]))),
                           add<6>(limb_mul(q.l[2], nf.l[0]), limb_mul(q.l[1], nf.l[1])));
    FfMulCells c;
    const Prod p1_hi = shr<LIMB_BITS>(p1);
    c.p1_lo = resize<3>(low_bits<LIMB_BITS>(p1));
    c.p1_hi0 = resize<3>(low_bits<LIMB_BITS>(p1_hi));
    const Prod hi1 = shr<LIMB_BITS>(p1_hi);
    c.p1_hi1 = hi1.w[0];
    c.r01 = add<6>(resize<6>(r.l[0]), shl<LIMB_BITS>(resize<6>(r.l[1])));
    const Prod c0 = shr<2 * LIMB_BITS>(sub<6>(add<6>(p0, shl<LIMB_BITS>(resize<6>(c.p1_lo))), c.r01));
    c.carry0 = c0.w[0];
    Prod c0w = zero<6>(); c0w.w[0] = c.carry0;
    const Prod c1 = shr<LIMB_BITS>(sub<6>(add<6>(add<6>(p2, p1_hi), c0w), resize<6>(r.l[2])));
    c.carry1 = resize<3>(c1);
    Limb L = zero<3>(); L.w[2] = 1u << 24;                                  // 2^88
    Limb one = zero<3>(); one.w[0] = 1;
    c.bound = sub<3>(sub<3>(add<3>(q.l[2], L), m.f2), one);                 // q2 + 2^88 - f2 - 1 (< 2^89)
    c.overflow = c.carry0 >= 4 || c.p1_hi1 >= 4 || (hi1.w[1] | hi1.w[2]) != 0 || (c.carry1.w[2] >> 27) != 0 || (c1.w[3] | c1.w[4] | c1.w[5]) != 0;
    return c;
}

// ---- ForeignFieldAdd ----
// r = left + sign right - overflow f with overflow in {0, sign} such that 0 <= r < f, and carry = r2 - left2 - sign right2 + overflow f2 in {-1, 0, 1}
// (the top-limb equation of the gate; the bottom one has the same carry).  bad: no such r (an operand >= f).
struct FfAdd { Limbs r; int overflow, carry; bool bad; };
KH_LIMB_FN FfAdd ff_add(const Limbs& left, const Limbs& right, int sign, const Elem& f, const Limb& f2) {
    const Elem l = pack(left), rt = pack(right);
    FfAdd o;
    o.bad = ge<9>(l, f) || ge<9>(rt, f);
    Elem r;
    if (sign > 0) {
        const Elem s = add<9>(l, rt);                                       // < 2^265
        const bool over = ge<9>(s, f);
        r = select<9>(over, sub<9>(s, f), s);
        o.overflow = over ? 1 : 0;
    } else {
        u32 borrow;
        const Elem d = sub<9>(l, rt, &borrow);
        r = select<9>(borrow != 0, add<9>(d, f), d);
        o.overflow = borrow ? -1 : 0;
    }
    o.r = unpack(r);
    // the carry is tiny: the low word of each top limb decides it
    const u32 fterm = o.overflow == 0 ? 0u : o.overflow > 0 ? f2.w[0] : 0u - f2.w[0];
    const u32 rterm = sign > 0 ? right.l[2].w[0] : 0u - right.l[2].w[0];
    o.carry = (int)(o.r.l[2].w[0] - left.l[2].w[0] - rterm + fterm);
    return o;
}

// ---- the modulus on the host ----
// f != 0, limbs < 2^88: mu = floor(2^528 / f) by shift-and-subtract, 529 steps
inline FfModulus ff_modulus(const Limbs& fl) {
    FfModulus m;
    m.f = pack(fl);
    m.f2 = fl.l[2];
    Wide<10> rem = zero<10>();
    const Wide<10> f10 = resize<10>(m.f);
    m.mu = zero<17>();
    for (int bit = 528; bit >= 0; bit--) {                                 // numerator 2^528: one set bit
        rem = shl<1>(rem);
        if (bit == 528) rem.w[0] |= 1u;
        if (ge<10>(rem, f10)) { rem = sub<10>(rem, f10); m.mu.w[bit / 32] |= 1u << (bit % 32); }
    }
    Elem two264 = zero<9>(); two264.w[8] = 1u << 8;                        // 2^264 = bit 8 of word 8
    m.nf = unpack(low_bits<264>(sub<9>(two264, m.f)));                     // f = 2^264 is excluded by the limb bound; nf < 2^264
    return m;
}

}  // namespace limb
}  // namespace kh
