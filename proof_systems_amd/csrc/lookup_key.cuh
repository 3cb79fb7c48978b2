// lookup_key.cuh -- a field element as a hash key on the device, for the hash sets of lookup_sorted.hip, lookup_rows.hip and witness_check.hip: the key,
// its comparison and its hash are lookup_hash.hpp's (shared with host_lookup.cpp); here the 16-byte loads.  No field arithmetic.
#pragma once
#include <stdint.h>
#include "lookup_hash.hpp"                                   // Key, Tuple, same, hash, lookup_slots

namespace kh {
namespace {
__device__ __forceinline__ Key load_key(const uint64_t* __restrict__ p) {
    const ulonglong2 a = ((const ulonglong2*)p)[0], b = ((const ulonglong2*)p)[1];
    Key k; k.l[0] = a.x; k.l[1] = a.y; k.l[2] = b.x; k.l[3] = b.y;
    return k;
}
}  // namespace
}  // namespace kh
