// cell_format.cuh -- a witness cell in the five KH_CELL_* formats (include/kimchi_hip.h): the conversions of wiring.hip (kh_witness_gather_dev,
// kh_witness_scatter_dev, a schedule's fused moves) and of value_steps.hip (kh_field_bits_dev reads its input as a gather delivers it).
#pragma once
#include "common.hpp"
#include "field.cuh"

namespace kh {

__device__ __forceinline__ u64 word64(const u32* v, int k) { return (u64)v[2 * k] | ((u64)v[2 * k + 1] << 32); }

// The conversion of ONE cell, the same code for the direct kernels (format uniform across the launch) and for a schedule's fused moves (format per
// lane).  `dense` is the value's own place on the dense side: cell_words(format) words.  Both return whether the value does not fit its format.
__device__ __forceinline__ size_t cell_words(int format) { return format == KH_CELL_FIELD || format == KH_CELL_INT256 ? 4 : format == KH_CELL_U64 ? 1 : 2; }
template <class F>
__device__ __forceinline__ bool cell_to_value(const u64* __restrict__ cell, int format, u64* __restrict__ dense) {
    Fe<F> v = Fe<F>::load(cell);
    if (format != KH_CELL_FIELD) v = from_mont<F>(v);
    if (format == KH_CELL_FIELD || format == KH_CELL_INT256) { v.store(dense); return false; }
    if (format == KH_CELL_U64) {
        dense[0] = word64(v.v, 0);
        return (word64(v.v, 1) | word64(v.v, 2) | word64(v.v, 3)) != 0;
    }
    const bool limb = format == KH_CELL_LIMB88;                     // two words: 128 bits, or 88
    const u64 hi = word64(v.v, 1);
    *(ulonglong2*)dense = make_ulonglong2(word64(v.v, 0), limb ? hi & 0xffffffu : hi);
    return ((limb ? hi >> 24 : 0) | word64(v.v, 2) | word64(v.v, 3)) != 0;
}
template <class F>
__device__ __forceinline__ bool value_to_cell(const u64* __restrict__ dense, int format, u64* __restrict__ cell) {
    Fe<F> v = Fe<F>::zero();
    bool bad = false;
    if (format == KH_CELL_FIELD || format == KH_CELL_INT256) {
        v = Fe<F>::load(dense);
        if (format == KH_CELL_INT256) {                             // v >= p: v - p does not borrow
            u32 br = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) br = (u32)(((u64)v.v[k] - Fe<F>::pw(k) - br) >> 63);
            bad = br == 0;
        }
    } else if (format == KH_CELL_U64) {
        const u64 w = dense[0];
        v.v[0] = (u32)w; v.v[1] = (u32)(w >> 32);
    } else {
        const ulonglong2 w = *(const ulonglong2*)dense;
        bad = format == KH_CELL_LIMB88 && (w.y >> 24) != 0;
        v.v[0] = (u32)w.x; v.v[1] = (u32)(w.x >> 32); v.v[2] = (u32)w.y; v.v[3] = (u32)(w.y >> 32);
    }
    if (format != KH_CELL_FIELD) v = to_mont<F>(v);
    v.store(cell);
    return bad;
}

}  // namespace kh
