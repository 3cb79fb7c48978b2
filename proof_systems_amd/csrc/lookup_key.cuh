// lookup_key.cuh -- a field element as a hash key, for the device hash sets of lookup_sorted.hip and lookup_rows.hip: values are compared as 32-byte
// strings (canonical Montgomery limbs are unique) and hashed as host_lookup.cpp hashes them.  No field arithmetic; 16-byte loads.
#pragma once
#include <stdint.h>

namespace kh {
namespace {
struct Key { uint64_t l[4]; };
__device__ __forceinline__ Key load_key(const uint64_t* __restrict__ p) {
    const ulonglong2 a = ((const ulonglong2*)p)[0], b = ((const ulonglong2*)p)[1];
    Key k; k.l[0] = a.x; k.l[1] = a.y; k.l[2] = b.x; k.l[3] = b.y;
    return k;
}
__device__ __forceinline__ bool same(const Key& a, const Key& b) { return ((a.l[0] ^ b.l[0]) | (a.l[1] ^ b.l[1]) | (a.l[2] ^ b.l[2]) | (a.l[3] ^ b.l[3])) == 0; }
__device__ __forceinline__ uint64_t hash(const Key& k) {          // as host_lookup.cpp
    uint64_t h = k.l[0] * 0x9e3779b97f4a7c15ULL ^ k.l[1];
    h = (h ^ (h >> 29)) * 0xbf58476d1ce4e5b9ULL ^ k.l[2];
    h = (h ^ (h >> 32)) * 0x94d049bb133111ebULL ^ k.l[3];
    return h ^ (h >> 31);
}
}  // namespace
}  // namespace kh
