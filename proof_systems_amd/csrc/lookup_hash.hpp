// lookup_hash.hpp -- the one definition of what the four lookup hash tables share: the key (a field element as 32 bytes), the tuple key of the witness
// check (table id, entry 0..2), their comparisons and hashes, and the number of slots of a table of L entries.  The tables are csrc/lookup_sorted.hip,
// csrc/lookup_rows.hip and csrc/witness_check.hip on the device and csrc/host_lookup.cpp on the host; all probe linearly, h = (h + 1) & (slots - 1), from
// hash & (slots - 1).  Plain C++, no device types and no field arithmetic (canonical Montgomery limbs are unique, so bytes compare as values): the same
// code runs on the host, where tests/cpp/test_lookup_hash.cpp prints it for tests/lookup_collisions.py -- the Python mirror the tests build colliding
// keys with -- to be held to it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)                                       // (spelled out: host_lookup.cpp includes no HIP header, which is where __forceinline__ comes from)
#define KH_LOOKUP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define KH_LOOKUP_FN inline
#endif

namespace kh {
namespace {
struct Key { uint64_t l[4]; };
struct Tuple { Key k[4]; };                              // table id, entry 0..2
KH_LOOKUP_FN bool same(const Key& a, const Key& b) { return ((a.l[0] ^ b.l[0]) | (a.l[1] ^ b.l[1]) | (a.l[2] ^ b.l[2]) | (a.l[3] ^ b.l[3])) == 0; }
KH_LOOKUP_FN bool same(const Tuple& a, const Tuple& b) { return same(a.k[0], b.k[0]) && same(a.k[1], b.k[1]) && same(a.k[2], b.k[2]) && same(a.k[3], b.k[3]); }
constexpr uint64_t LOOKUP_HASH_MUL = 0x9e3779b97f4a7c15ULL;   // 2^64 / the golden ratio: the first multiplier of both hashes
KH_LOOKUP_FN uint64_t hash(const Key& k) {
    uint64_t h = k.l[0] * LOOKUP_HASH_MUL ^ k.l[1];
    h = (h ^ (h >> 29)) * 0xbf58476d1ce4e5b9ULL ^ k.l[2];
    h = (h ^ (h >> 32)) * 0x94d049bb133111ebULL ^ k.l[3];
    return h ^ (h >> 31);
}
KH_LOOKUP_FN uint32_t hash(const Tuple& t) {
    uint64_t h = hash(t.k[0]);
#pragma unroll
    for (int i = 1; i < 4; i++) h = (h ^ (h >> 27)) * LOOKUP_HASH_MUL + hash(t.k[i]);
    return (uint32_t)(h ^ (h >> 32));
}
// the slots of a table of L entries: a power of two of at least 2 L (and at least 16), so that at most half of them are ever occupied -- what ends
// every probe walk
KH_LOOKUP_FN size_t lookup_slots(size_t L) { size_t cap = 16; while (cap < 2 * L) cap <<= 1; return cap; }
}  // namespace
}  // namespace kh
