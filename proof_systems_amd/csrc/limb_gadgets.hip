// limb_gadgets.hip -- the witness rows of the optional gates on the device: RangeCheck0 / RangeCheck1 (the multi-range-check), Xor16, Rot64,
// ForeignFieldAdd and ForeignFieldMul (kimchi/src/circuits/polynomials/{range_check,xor,rot,foreign_field_add,foreign_field_mul}; oracle/gates.py restates
// their constraints), for kh_range_check_witness_dev, kh_xor_witness_dev, kh_rot64_witness_dev, kh_foreign_field_add_witness_dev and
// kh_foreign_field_mul_witness_dev (csrc/witness_steps.cpp).  include/kimchi_hip.h has the cell tables.
//
// Every kernel is ONE LANE PER (instance, row) in blocks of one wave: the witness is column-major, so with instances packed densely the 64 lanes of a
// wave store 64 consecutive rows of a column, 2 KiB in a row, fifteen times.  (One lane per instance would store four rows of each column 128 bytes
// apart.)  The lanes of an instance all read its 48..96 bytes of input and each derives its own row: the integer work is a few dozen shifts and masks,
// the cost is the 15 conversions to Montgomery form (one product by R^2 each) and the 480 bytes of stores.  The rows of an instance differ in WHICH
// bits go to which cell, not in what is done with them: each lane selects its row's fifteen integers first, then one common tail converts and stores
// them, so a wave does fifteen products, not fifteen per kind of row.
//
//   k_range_check     4 lanes per instance: RangeCheck0, RangeCheck0, RangeCheck1, Zero
//   k_xor             ceil(bits / 16) + 1 lanes per instance; each reads its operands already shifted (a word offset into the 4 words)
//   k_rot64           3 lanes per instance: Rot64, the RangeCheck0 rows of shifted and excess
//   k_ff_add          2 lanes per instance: a 264-bit add or subtract and one comparison with the modulus each
//   k_ff_mul          2 lanes per instance, and BOTH divide: (q, r) = divmod(a b, f) by Barrett's estimate with the full 528 x 529-bit product
//                     (limb_int.cuh: fixed trip count, q - 1 <= estimate <= q, one correction by select), 261 + 81 + 45 32-bit products -- four
//                     conversions' worth.  Handing q, r and the carries from one lane to the other through memory would take a second launch
//                     and 100 bytes per instance each way to save that.
// Integer arithmetic is limb_int.cuh's (plain C++, compile-time indices: nothing in scratch memory); the field arithmetic is one mul<F> per cell.
#include "common.hpp"
#include "field.cuh"
#include "limb_int.cuh"
#include "api_internal.hpp"

namespace kh {

using limb::Wide;
using limb::Limb;
using limb::Limbs;

// an integer < p of up to 8 words as its Montgomery element
template <class F, int N>
__device__ __forceinline__ Fe<F> fe_of(const Wide<N>& x) {
    static_assert(N <= 8, "a cell is one field element");
    Fe<F> e = Fe<F>::zero();
#pragma unroll
    for (int i = 0; i < N; i++) e.v[i] = x.w[i];
    return to_mont<F>(e);
}
template <class F>
__device__ __forceinline__ Fe<F> fe_of(u64 v) { return fe_of<F>(limb::from_u64<2>(v)); }
// 0, 1 or -1
template <class F>
__device__ __forceinline__ Fe<F> fe_of_sign(int s) {
    const Fe<F> one = Fe<F>::one(), minus_one = neg<F>(one);
    Fe<F> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = s == 0 ? 0u : s > 0 ? one.v[i] : minus_one.v[i];
    return r;
}
// bits pos .. pos + n - 1 of lo + 2^64 hi (n <= 32)
__device__ __forceinline__ u64 bits128(u64 lo, u64 hi, unsigned pos, unsigned n) {
    const u64 s = pos >= 64 ? hi >> (pos - 64) : pos == 0 ? lo : (lo >> pos) | (hi << (64 - pos));
    return s & (((u64)1 << n) - 1);
}
// An 88-bit limb as the calls take it: two u64, little-endian.  `bad` collects a limb >= 2^88; the value goes on masked.
struct Limb128 { u64 lo, hi; };
__device__ __forceinline__ Limb128 load_limb(const u64* p, bool& bad) {
    const ulonglong2 v = *(const ulonglong2*)p;
    bad |= (v.y >> 24) != 0;
    return Limb128{v.x, v.y & 0xffffffu};
}
__device__ __forceinline__ Limb as_limb(const Limb128& x) { return limb::from_u64<3>(x.lo, x.hi); }
__device__ __forceinline__ Limb128 as_limb128(const Limb& x) { return Limb128{(u64)x.w[0] | ((u64)x.w[1] << 32), (u64)x.w[2]}; }
__device__ __forceinline__ Limbs load_limbs(const u64* p, bool& bad) {
    Limbs r;
#pragma unroll
    for (int k = 0; k < 3; k++) r.l[k] = as_limb(load_limb(p + 2 * k, bad));
    return r;
}
__device__ __forceinline__ void store_limb(u64* p, const Limb& x) {
    const Limb128 v = as_limb128(x);
    *(ulonglong2*)p = make_ulonglong2(v.lo, v.hi);
}
__device__ __forceinline__ void raise_flag(u32* flags, u32 bit, bool bad) {
    if (flags && __any(bad) && (threadIdx.x & 63u) == 0) atomicOr(flags, 1u << bit);
}

// The fifteen integers of one row of the range-check family: column 0 up to 88 bits, column 1 up to 176 (the compact row's v0 + 2^88 v1), the rest up
// to 64 (Rot64's excess; 12 bits or 2 everywhere else).
struct SmallRow { u64 c0lo, c0hi, c1[3], s[15]; };                  // s[0], s[1] are not used
// the RangeCheck0 row of x = lo + 2^64 hi < 2^88: x, six 12-bit limbs from the top, eight crumbs down to bit 0
__device__ __forceinline__ void rc0_cells(SmallRow& R, u64 lo, u64 hi) {
    R.c0lo = lo; R.c0hi = hi;
    R.c1[0] = bits128(lo, hi, 76, 12); R.c1[1] = R.c1[2] = 0;
#pragma unroll
    for (int k = 1; k < 6; k++) R.s[1 + k] = bits128(lo, hi, 76 - 12 * k, 12);
#pragma unroll
    for (int k = 0; k < 8; k++) R.s[7 + k] = (lo >> (14 - 2 * k)) & 3;
}
template <class F>
__device__ __forceinline__ void store_small_row(const WitnessPlace& at, size_t r, const SmallRow& R) {
    fe_of<F>(limb::from_u64<4>(R.c0lo, R.c0hi)).store(at.cell(r, 0));
    Wide<6> c1;
#pragma unroll
    for (int k = 0; k < 3; k++) { c1.w[2 * k] = (u32)R.c1[k]; c1.w[2 * k + 1] = (u32)(R.c1[k] >> 32); }
    fe_of<F>(c1).store(at.cell(r, 1));
#pragma unroll
    for (int c = 2; c < 15; c++) fe_of<F>(R.s[c]).store(at.cell(r, c));
}

// ------------------------------------------------------------------------------------------------------ multi-range-check
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_range_check(const u64* __restrict__ limbs, size_t n, int compact, WitnessPlace at, u32* __restrict__ flags, u32 bit) {
    const size_t t = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (t < 4 * n) {
        const size_t i = t >> 2;
        const unsigned rr = (unsigned)t & 3u;
        const Limb128 v0 = load_limb(limbs + 6 * i, bad), v1 = load_limb(limbs + 6 * i + 2, bad), v2 = load_limb(limbs + 6 * i + 4, bad);
        const Limb128 x0 = compact ? v2 : v0, x1 = compact ? v0 : v1, x2 = compact ? v1 : v2;
        SmallRow R;
        if (rr < 2) {
            const Limb128 x = rr ? x1 : x0;
            rc0_cells(R, x.lo, x.hi);
        } else if (rr == 2) {                                       // RangeCheck1: x2, the compact sum, the top crumb, four limbs, crumbs 36 .. 22
            R.c0lo = x2.lo; R.c0hi = x2.hi;
            R.c1[0] = compact ? v0.lo : 0;                          // v0 + 2^88 v1 in three words
            R.c1[1] = compact ? v0.hi | (v1.lo << 24) : 0;
            R.c1[2] = compact ? (v1.lo >> 40) | (v1.hi << 24) : 0;
            R.s[2] = bits128(x2.lo, x2.hi, 86, 2);
#pragma unroll
            for (int k = 0; k < 4; k++) R.s[3 + k] = bits128(x2.lo, x2.hi, 74 - 12 * k, 12);
#pragma unroll
            for (int k = 0; k < 8; k++) R.s[7 + k] = (x2.lo >> (36 - 2 * k)) & 3;
        } else {                                                    // Zero: crumbs 20 .. 16 of x2, the top two limbs of x0 and x1, crumbs 14 .. 0 of x2
            R.c0lo = (x2.lo >> 20) & 3; R.c0hi = 0;
            R.c1[0] = (x2.lo >> 18) & 3; R.c1[1] = R.c1[2] = 0;
            R.s[2] = (x2.lo >> 16) & 3;
            R.s[3] = bits128(x0.lo, x0.hi, 76, 12); R.s[4] = bits128(x0.lo, x0.hi, 64, 12);
            R.s[5] = bits128(x1.lo, x1.hi, 76, 12); R.s[6] = bits128(x1.lo, x1.hi, 64, 12);
#pragma unroll
            for (int k = 0; k < 8; k++) R.s[7 + k] = (x2.lo >> (14 - 2 * k)) & 3;
        }
        store_small_row<F>(at, at.start_row(i) + rr, R);
    }
    raise_flag(flags, bit, bad);
}

// ------------------------------------------------------------------------------------------------------------------ Rot64
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_rot64(const u64* __restrict__ words, unsigned rot, size_t n, WitnessPlace at, u64* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (t >= 3 * n) return;
    const size_t i = t / 3;
    const unsigned rr = (unsigned)(t - 3 * i);
    const u64 w = words[i];
    const u64 excess = rot ? w >> (64 - rot) : 0, shifted = w << rot, rotated = shifted | excess;
    const u64 bound = excess - ((u64)1 << rot);                     // excess - 2^rot + 2^64: excess < 2^rot, so the u64 wraps to it
    SmallRow R;
    if (rr == 0) {
        R.c0lo = w; R.c0hi = 0;
        R.c1[0] = rotated; R.c1[1] = R.c1[2] = 0;
        R.s[2] = excess;
#pragma unroll
        for (int k = 0; k < 4; k++) R.s[3 + k] = (bound >> (52 - 12 * k)) & 0xfff;
#pragma unroll
        for (int k = 0; k < 8; k++) R.s[7 + k] = (bound >> (14 - 2 * k)) & 3;
        if (out) out[i] = rotated;
    } else rc0_cells(R, rr == 1 ? shifted : excess, 0);
    store_small_row<F>(at, at.start_row(i) + rr, R);
}

// ------------------------------------------------------------------------------------------------------------------ Xor16
// Row rr of an instance holds in1 >> 16 rr, in2 >> 16 rr, their xor and the twelve low nybbles; the last row (rr == nrows - 1) is zero.
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_xor(const u64* __restrict__ in1, const u64* __restrict__ in2, unsigned nbits, unsigned nrows, size_t n, WitnessPlace at, u64* __restrict__ out,
      u32* __restrict__ flags, u32 bit) {
    const size_t t = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (t < (size_t)nrows * n) {
        const size_t i = t / nrows;
        const unsigned rr = (unsigned)(t - i * nrows);
        const bool closing = rr + 1 == nrows;
        const unsigned ws = closing ? 4u : rr >> 2, bs = (16 * rr) & 63;
        u64 v[2][4];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const u64* const p = (j ? in2 : in1) + 4 * i;
            u64 w[5];
#pragma unroll
            for (unsigned k = 0; k < 5; k++) w[k] = ws + k < 4 ? p[ws + k] : 0;
#pragma unroll
            for (int k = 0; k < 4; k++) v[j][k] = bs ? (w[k] >> bs) | (w[k + 1] << (64 - bs)) : w[k];
        }
        if (rr == 0) {                                              // the whole operands are here: their range, and the result
#pragma unroll
            for (unsigned k = 0; k < 4; k++) {
                const u64 both = v[0][k] | v[1][k];
                bad |= 64 * k >= nbits ? both != 0 : nbits < 64 * (k + 1) ? (both >> (nbits - 64 * k)) != 0 : false;
            }
            if (out) {
#pragma unroll
                for (int k = 0; k < 4; k++) out[4 * i + k] = v[0][k] ^ v[1][k];
            }
        }
        const size_t r = at.start_row(i) + rr;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Wide<8> x;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u64 word = j == 2 ? v[0][k] ^ v[1][k] : v[j][k];
                x.w[2 * k] = (u32)word; x.w[2 * k + 1] = (u32)(word >> 32);
            }
            fe_of<F>(x).store(at.cell(r, j));
#pragma unroll
            for (int k = 0; k < 4; k++) fe_of<F>((u64)((x.w[0] >> (4 * k)) & 15u)).store(at.cell(r, 3 + 4 * j + k));
        }
    }
    raise_flag(flags, bit, bad);
}

// -------------------------------------------------------------------------------------------------------- ForeignFieldAdd
struct FfAddConst { limb::Elem f; Limb f2; };
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_ff_add(const u64* __restrict__ left, const u64* __restrict__ right, int sign, size_t n, FfAddConst m, WitnessPlace at, u64* __restrict__ out,
         u32* __restrict__ flags, u32 bit) {
    const size_t t = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (t < 2 * n) {
        const size_t i = t >> 1;
        const bool result_row = t & 1;
        const Limbs l = load_limbs(left + 6 * i, bad), rt = load_limbs(right + 6 * i, bad);
        const limb::FfAdd s = limb::ff_add(l, rt, sign, m.f, m.f2);
        bad |= s.bad;
        const size_t r = at.start_row(i) + (result_row ? 1 : 0);
#pragma unroll
        for (int k = 0; k < 3; k++) fe_of<F>(limb::select<3>(result_row, s.r.l[k], l.l[k])).store(at.cell(r, k));
        if (!result_row) {
#pragma unroll
            for (int k = 0; k < 3; k++) fe_of<F>(rt.l[k]).store(at.cell(r, 3 + k));
            fe_of_sign<F>(s.overflow).store(at.cell(r, 6));
            fe_of_sign<F>(s.carry).store(at.cell(r, 7));
        } else if (out) {
#pragma unroll
            for (int k = 0; k < 3; k++) store_limb(out + 6 * i + 2 * k, s.r.l[k]);
        }
    }
    raise_flag(flags, bit, bad);
}

// -------------------------------------------------------------------------------------------------------- ForeignFieldMul
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_ff_mul(const u64* __restrict__ a_in, const u64* __restrict__ b_in, size_t n, limb::FfModulus m, WitnessPlace at, u64* __restrict__ out_checks,
         u32* __restrict__ flags, u32 bit) {
    const size_t t = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (t < 2 * n) {
        const size_t i = t >> 1;
        const bool next_row = t & 1;
        const Limbs a = load_limbs(a_in + 6 * i, bad), b = load_limbs(b_in + 6 * i, bad);
        const limb::DivMod d = limb::ff_divmod(limb::pack(a), limb::pack(b), m);
        const Limbs q = limb::unpack(d.q), rem = limb::unpack(d.r);
        const limb::FfMulCells c = limb::ff_mul_cells(a, b, q, rem, m);
        bad |= d.q_overflow || c.overflow;
        const size_t r = at.start_row(i) + (next_row ? 1 : 0);
        // gate row: a0 a1 a2 b0 b1 b2 p1_lo | carry1 bits 0..48 by 12, 84..90 by 2, 90;  next row: r01 r2 q0 q1 q2 bound p1_hi0 | p1_hi1, carry1 bits 48..84 by 12, carry0
        fe_of<F>(limb::select<6>(next_row, c.r01, limb::resize<6>(a.l[0]))).store(at.cell(r, 0));
        const Limb gate[6] = {a.l[1], a.l[2], b.l[0], b.l[1], b.l[2], c.p1_lo}, next[6] = {rem.l[2], q.l[0], q.l[1], q.l[2], c.bound, c.p1_hi0};
#pragma unroll
        for (int k = 0; k < 6; k++) fe_of<F>(limb::select<3>(next_row, next[k], gate[k])).store(at.cell(r, 1 + k));
        const Limb128 c1 = as_limb128(c.carry1);
        fe_of<F>(next_row ? (u64)c.p1_hi1 : bits128(c1.lo, c1.hi, 0, 12)).store(at.cell(r, 7));
#pragma unroll
        for (int k = 1; k < 4; k++) fe_of<F>(bits128(c1.lo, c1.hi, (next_row ? 36 : 0) + 12 * k, 12)).store(at.cell(r, 7 + k));
        fe_of<F>(next_row ? (u64)c.carry0 : bits128(c1.lo, c1.hi, 84, 2)).store(at.cell(r, 11));
        if (!next_row) {
            fe_of<F>(bits128(c1.lo, c1.hi, 86, 2)).store(at.cell(r, 12));
            fe_of<F>(bits128(c1.lo, c1.hi, 88, 2)).store(at.cell(r, 13));
            fe_of<F>(bits128(c1.lo, c1.hi, 90, 1)).store(at.cell(r, 14));
        } else if (out_checks) {
            u64* const o = out_checks + 18 * i;
            const Limb checks[9] = {q.l[0], q.l[1], q.l[2], rem.l[0], rem.l[1], rem.l[2], c.bound, c.p1_lo, c.p1_hi0};
#pragma unroll
            for (int k = 0; k < 9; k++) store_limb(o + 2 * k, checks[k]);
        }
    }
    raise_flag(flags, bit, bad);
}

// (the callers in witness_steps.cpp have validated pointers and sizes: at most WAVE_BLOCK_MAX_N lanes per call keeps the grids inside 31 bits; one phase
// of kh_last_timings per call, under the gate's name)
int range_check_rows(Context& C, int field, const uint64_t* limbs_dev, size_t n, int compact, const WitnessPlace& at, uint32_t* flags_dev, unsigned bit) {
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_range_check<F>, blocks_of(4 * n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)limbs_dev, n, compact, at, flags_dev, (u32)bit);
    C.timer.mark("range_check", C.stream);
    return KH_OK;
}
int xor_rows(Context& C, int field, const uint64_t* in1_dev, const uint64_t* in2_dev, unsigned bits, size_t n, const WitnessPlace& at, uint64_t* out_dev,
             uint32_t* flags_dev, unsigned bit) {
    const unsigned nrows = (bits + 15) / 16 + 1;
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_xor<F>, blocks_of(nrows * n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)in1_dev, (const u64*)in2_dev, bits, nrows, n, at,
                    (u64*)out_dev, flags_dev, (u32)bit);
    C.timer.mark("xor", C.stream);
    return KH_OK;
}
int rot64_rows(Context& C, int field, const uint64_t* words_dev, unsigned rot, size_t n, const WitnessPlace& at, uint64_t* out_dev) {
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_rot64<F>, blocks_of(3 * n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)words_dev, rot, n, at, (u64*)out_dev);
    C.timer.mark("rot64", C.stream);
    return KH_OK;
}
static Limbs host_limbs(const uint64_t* modulus) {
    Limbs f;
    for (int k = 0; k < 3; k++) f.l[k] = limb::from_u64<3>(modulus[2 * k], modulus[2 * k + 1]);
    return f;
}
int ff_add_rows(Context& C, int field, const uint64_t* modulus, const uint64_t* left_dev, const uint64_t* right_dev, int sign, size_t n, const WitnessPlace& at,
                uint64_t* out_dev, uint32_t* flags_dev, unsigned bit) {
    const Limbs f = host_limbs(modulus);
    const FfAddConst m{limb::pack(f), f.l[2]};
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_ff_add<F>, blocks_of(2 * n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)left_dev, (const u64*)right_dev, sign, n, m, at,
                    (u64*)out_dev, flags_dev, (u32)bit);
    C.timer.mark("foreign_field_add", C.stream);
    return KH_OK;
}
struct FfMulConst { limb::FfModulus m; };
std::shared_ptr<const FfMulConst> ff_mul_prepare(const uint64_t* modulus) {
    return std::make_shared<const FfMulConst>(FfMulConst{limb::ff_modulus(host_limbs(modulus))});
}
int ff_mul_rows_prepared(Context& C, int field, const FfMulConst& m, const uint64_t* a_dev, const uint64_t* b_dev, size_t n, const WitnessPlace& at,
                         uint64_t* out_checks_dev, uint32_t* flags_dev, unsigned bit) {
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_ff_mul<F>, blocks_of(2 * n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)a_dev, (const u64*)b_dev, n, m.m, at,
                    (u64*)out_checks_dev, flags_dev, (u32)bit);
    C.timer.mark("foreign_field_mul", C.stream);
    return KH_OK;
}
// the limbs of f and of 2^264 - f, two u64 each (kh_foreign_field_gate_coefficients reduces them into the field)
void ff_negated_modulus(const uint64_t* modulus, uint64_t* nf_out) {
    const limb::FfModulus m = limb::ff_modulus(host_limbs(modulus));
    for (int k = 0; k < 3; k++) {
        nf_out[2 * k] = (uint64_t)m.nf.l[k].w[0] | ((uint64_t)m.nf.l[k].w[1] << 32);
        nf_out[2 * k + 1] = m.nf.l[k].w[2];
    }
}

}  // namespace kh
