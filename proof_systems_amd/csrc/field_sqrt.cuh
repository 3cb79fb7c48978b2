// field_sqrt.cuh -- the square root ark-ff returns (SqrtPrecomputation::TonelliShanks, no sign normalisation; oracle/pasta.py::Field.sqrt restates
// it), for srs_gen.hip (the Shallue-van de Woestijne map: the SRS files are byte-identical because of it) and value_steps.hip (kh_field_sqrt_dev).
// The two constants it needs depend on the field alone and are computed on the host: SqrtParams travels as a kernel argument.
//
// EVERY loop has a constant trip bound from the 2-adicity of p - 1 (32 for both Pasta fields): at most 32 outer rounds, an order search of at most
// 32 squarings, a power of z of at most 32 squarings.  For a canonical input none of the bounds is reached -- the order of b strictly falls from
// round to round --, so the result is ark-ff's; for a non-canonical one (device data is not compared with p) the value is unspecified and the
// function still ends.
#pragma once
#include <string.h>

#include "field.cuh"
#include "host_ec.hpp"

namespace kh {

static constexpr int SQRT_TWO_ADICITY = 32;                 // p - 1 = 2^32 T, T odd, for Fp and Fq alike

struct SqrtParams {
    u32 root[8];               // 5^T: a generator of the 2-Sylow subgroup, Montgomery limbs
    u32 t_m1_d2[8];            // (T - 1) / 2, a plain integer
};

inline SqrtParams sqrt_params(const khost::Fld& F) {
    khost::fe five = {{5, 0, 0, 0}}; five = F.to_mont(five);
    khost::fe pm1 = F.f.p; pm1.l[0] -= 1;
    khost::fe T, Tm1, tm1d2;
    for (int i = 0; i < 4; i++) T.l[i] = (pm1.l[i] >> 32) | (i < 3 ? pm1.l[i + 1] << 32 : 0);
    Tm1 = T; Tm1.l[0] -= 1;
    for (int i = 0; i < 4; i++) tm1d2.l[i] = (Tm1.l[i] >> 1) | (i < 3 ? Tm1.l[i + 1] << 63 : 0);
    khost::fe root = F.f.one, b = five;
    for (int i = 0; i < 256; i++) { if ((T.l[i >> 6] >> (i & 63)) & 1) root = F.mul(root, b); b = F.sqr(b); }
    SqrtParams P;
    memcpy(P.root, &root, 32); memcpy(P.t_m1_d2, &tm1d2, 32);
    return P;
}

// Tonelli-Shanks exactly as ark-ff / the oracle.  Returns false for a non-residue and leaves `out` as it is.
template <class F>
__device__ bool fe_sqrt(const Fe<F>& a, const SqrtParams& P, Fe<F>& out) {
    if (a.is_zero()) { out = a; return true; }
    const Fe<F> one = Fe<F>::one();
    // w = a^((T-1)/2)
    Fe<F> w = one;
    int top = 255;
    while (top > 0 && !((P.t_m1_d2[top >> 5] >> (top & 31)) & 1u)) top--;
    for (int i = top; i >= 0; i--) {
        w = sqr<F>(w);
        if ((P.t_m1_d2[i >> 5] >> (i & 31)) & 1u) w = mul<F>(w, a);
    }
    Fe<F> x = mul<F>(a, w);
    Fe<F> b = mul<F>(x, w);              // a^T
    {                                    // residue test: b^(2^31) == 1
        Fe<F> t = b;
        for (int i = 0; i < SQRT_TWO_ADICITY - 1; i++) t = sqr<F>(t);
        if (!(t == one)) return false;
    }
    Fe<F> z;
#pragma unroll
    for (int i = 0; i < 8; i++) z.v[i] = P.root[i];
    int v = SQRT_TWO_ADICITY;
    for (int round = 0; round < SQRT_TWO_ADICITY && !(b == one); round++) {
        int k = 0; Fe<F> t = b;
        for (; k < SQRT_TWO_ADICITY && !(t == one); k++) t = sqr<F>(t);      // the order of b is 2^k, k < v
        w = z;
        for (int i = 0; i < SQRT_TWO_ADICITY && i < v - k - 1; i++) w = sqr<F>(w);
        z = sqr<F>(w);
        b = mul<F>(b, z);
        x = mul<F>(x, w);
        v = k;
    }
    out = x;
    return true;
}

}  // namespace kh
