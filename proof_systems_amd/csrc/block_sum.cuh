// block_sum.cuh -- sums of field elements and of whole XYZZ points over a wave and over a block, one value per thread.  (Points spread over four lanes
// have their folds in coop.cuh.)  Field addition is associative and the group law exact, so any order gives the same element.
#pragma once
#include "curve.cuh"

namespace kh {

// the sum over the 64 lanes of a wave, by shuffles (valid in lane 0)
template <class F>
__device__ __forceinline__ Fe<F> wave_sum(Fe<F> v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Fe<F> o;
#pragma unroll
        for (int k = 0; k < 8; k++) o.v[k] = __shfl_down(v.v[k], d, 64);
        v = add<F>(v, o);
    }
    return v;
}
// the sum over a block of T threads (a power of two) through LDS: sh holds 8 T words, word-major (no bank conflicts); a halving tree, valid in thread 0
template <class F, int T>
__device__ __forceinline__ Fe<F> block_tree_sum(Fe<F> acc, u32* sh) {
    const u32 t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; k++) sh[k * T + t] = acc.v[k];
    __syncthreads();
    for (int s = T / 2; s >= 1; s >>= 1) {
        if ((int)t < s) {
            Fe<F> o;
#pragma unroll
            for (int k = 0; k < 8; k++) o.v[k] = sh[k * T + t + s];
            acc = add<F>(acc, o);
#pragma unroll
            for (int k = 0; k < 8; k++) sh[k * T + t] = acc.v[k];
        }
        __syncthreads();
    }
    return acc;
}

template <class F>
__device__ __forceinline__ Xyzz<F> shfl_down(const Xyzz<F>& a, int delta) {
    Xyzz<F> r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r.x.v[i] = __shfl_down(a.x.v[i], delta, 64); r.y.v[i] = __shfl_down(a.y.v[i], delta, 64);
        r.zz.v[i] = __shfl_down(a.zz.v[i], delta, 64); r.zzz.v[i] = __shfl_down(a.zzz.v[i], delta, 64);
    }
    return r;
}
// the sum of one point per thread over a block of <= 4 waves: shuffle tree, then wave 0 folds the wave results parked in sh (32 words per wave); valid in thread 0
template <class BF>
__device__ __forceinline__ Xyzz<BF> block_sum(Xyzz<BF> acc, u32* sh) {
    for (int d = 32; d >= 1; d >>= 1) { Xyzz<BF> o = shfl_down<BF>(acc, d); acc = add<BF>(acc, o); }
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    u32* mine = sh + wave * 32;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; i++) { mine[i] = acc.x.v[i]; mine[8 + i] = acc.y.v[i]; mine[16 + i] = acc.zz.v[i]; mine[24 + i] = acc.zzz.v[i]; }
    }
    __syncthreads();
    int nw = blockDim.x >> 6;
    if (threadIdx.x < 64) {              // wave 0 folds the (<= 4) wave results
        Xyzz<BF> o = Xyzz<BF>::identity();
        if (lane < nw) {
            const u32* p = sh + lane * 32;
#pragma unroll
            for (int i = 0; i < 8; i++) { o.x.v[i] = p[i]; o.y.v[i] = p[8 + i]; o.zz.v[i] = p[16 + i]; o.zzz.v[i] = p[24 + i]; }
        }
        for (int d = 2; d >= 1; d >>= 1) { Xyzz<BF> q = shfl_down<BF>(o, d); o = add<BF>(o, q); }
        acc = o;
    }
    return acc;                          // valid in thread 0
}

}  // namespace kh
