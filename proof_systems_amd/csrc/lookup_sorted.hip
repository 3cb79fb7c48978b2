// lookup_sorted.hip -- the `sorted` step of the lookup argument (kimchi/src/circuits/lookup/constraints.rs:90-194) on the device, for
// kh_lookup_sorted_dev (csrc/vector_api.cpp): the hash join of host_lookup.cpp over device-resident columns, plus the expansion into the snake layout.
// No field arithmetic: values are compared as 32-byte strings (canonical Montgomery limbs are unique), with the hash of host_lookup.cpp.
//
//   k_sorted_clear    slots = EMPTY, cnt[i] = 1 (every table entry appears once), cnt[L] = 0 (the scan's total lands in off[L]), status = none
//   k_sorted_build    one thread per table entry i that differs from entry i - 1: linear probing, atomicCAS(slot, EMPTY, i); a slot whose entry has
//                     the same 32 bytes takes atomicMin(slot, i).  Slots only go from empty to occupied and an occupied slot never changes the key it stands for, so equal
//                     keys meet in one slot, and that slot ends up holding the FIRST occurrence -- the rule of host_lookup.cpp, whatever the arrival order
//   k_sorted_count    one thread per (lookup slot s, row r): probe, cnt[found] += 1.  Most values of a real circuit are the dummy value 0, so the adds
//                     are combined within the wave first (ballot + popcount, one atomic per distinct entry for the first rounds).  Counts are
//                     integers: the result does not depend on the arrival order.  A value that is not in the table records s * L + r with an atomicMin
//                     into the status word (the lowest = the first in slot-major order, what the host function reports); nothing traps
//   (scan)            off = exclusive prefix sum of cnt (exclusive_scan_u32, msm.hip).  Only first occurrences are ever counted, so a repeated table
//                     entry keeps its 1 and cnt[i] IS the run length of entry i; off[L] = L + (values found) = (max_per_row + 1) L when none is missing
//   k_sorted_expand   one thread per output element (column k, index e <= L): its position in the sorted multiset under the snake layout, the table
//                     entry by binary search over off, 32 bytes stored with two 16-byte stores (consecutive lanes, consecutive elements of a column).
//                     Does nothing when the status word names a missing value: the output is then left as it was
// All memory-bound, 256-thread blocks.  Every index is below 2^31 (the caller refuses (max_per_row + 1) L >= 2^31).
#include "common.hpp"
#include "msm.hpp"
#include "lookup_key.cuh"                                    // load_key; Key, same, hash, lookup_slots (lookup_hash.hpp)

namespace kh {

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
constexpr u32 SORTED_EMPTY = 0xffffffffu;
}  // namespace

__global__ void __launch_bounds__(256)
k_sorted_clear(u32* __restrict__ slots, u32 cap, u32* __restrict__ cnt, u32 L, u32* __restrict__ status) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) slots[i] = SORTED_EMPTY;
    if (i < L) cnt[i] = 1u;
    if (i == L) cnt[i] = 0u;                                 // (cap >= 2 L > L: some thread has i == L)
    if (i == 0) { status[0] = SORTED_EMPTY; status[1] = 0u; }
}

__global__ void __launch_bounds__(256)
k_sorted_build(const u64* __restrict__ table, u32 L, u32* __restrict__ slots, u32 mask) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const Key me = load_key(table + 4 * (size_t)i);
    // An entry equal to its predecessor is never a first occurrence, and the head of its run inserts the key: it has nothing to do.  (The combined table
    // of a real circuit ends in tens of thousands of equal padding rows -- left in, their atomics on ONE slot took 1.35 ms at 2^16 rows.)
    if (i > 0 && same(load_key(table + 4 * (size_t)(i - 1)), me)) return;
    u32 h = (u32)hash(me) & mask;
    for (;;) {
        u32 cur = __hip_atomic_load(&slots[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == SORTED_EMPTY) {
            cur = atomicCAS(&slots[h], SORTED_EMPTY, i);
            if (cur == SORTED_EMPTY) return;                 // claimed
        }
        if (same(load_key(table + 4 * (size_t)cur), me)) {   // (the slot's index only ever decreases: one that is already lower needs no atomic)
            if (i < cur) atomicMin(&slots[h], i);
            return;
        }
        h = (h + 1) & mask;                                  // (at most L of >= 2 L slots are ever occupied: the walk ends)
    }
}

// values: column s at values + 4 s stride.  total = max_per_row * L threads.
__global__ void __launch_bounds__(256)
k_sorted_count(const u64* __restrict__ table, const u64* __restrict__ values, size_t stride, u32 L, u32 total, const u32* __restrict__ slots, u32 mask,
               u32* __restrict__ cnt, u32* __restrict__ status) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    u32 found = SORTED_EMPTY;
    if (g < total) {
        const u32 s = g / L, r = g - s * L;
        const Key v = load_key(values + 4 * ((size_t)s * stride + r));
        u32 h = (u32)hash(v) & mask;
        for (;;) {
            const u32 e = slots[h];
            if (e == SORTED_EMPTY) { atomicMin(&status[0], g); break; }          // not in the table: g = s * L + r
            if (same(load_key(table + 4 * (size_t)e), v)) { found = e; break; }
            h = (h + 1) & mask;
        }
    }
    // one add per distinct entry of the wave for the first rounds (the dummy entry takes nearly all lanes of a real circuit), the rest one by one
    bool pending = found != SORTED_EMPTY;
    const u32 lane = __lane_id();
    for (int round = 0; round < 4; round++) {
        const u64 m = __ballot(pending);
        if (m == 0) break;
        const u32 leader = (u32)__ffsll((long long)m) - 1u;
        const u32 lf = __shfl(found, (int)leader);
        const bool match = pending && found == lf;
        const u64 mm = __ballot(match);
        if (lane == leader) atomicAdd(&cnt[lf], (u32)__popcll(mm));
        if (match) pending = false;
    }
    if (pending) atomicAdd(&cnt[found], 1u);
}

// out: column k at out + 4 k out_stride, L + 1 elements.  Column k holds the positions k L .. k L + L - 1 of the sorted multiset, its L-th element is
// position (k + 1) L (the next column's first), the last column's L-th repeats the last position; odd columns are reversed over all L + 1 elements.
__global__ void __launch_bounds__(256)
k_sorted_expand(const u64* __restrict__ table, const u32* __restrict__ off, u32 L, u32 ncols, u32 total, u64* __restrict__ out, size_t out_stride,
                u32* __restrict__ status) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0) status[1] = off[L];                          // the multiset's size, for the caller's check
    if (g >= total || status[0] != SORTED_EMPTY) return;
    const u32 W = L + 1, k = g / W, e = g - k * W;
    const u32 j = (k & 1u) ? L - e : e;
    const u32 last = ncols * L - 1u;
    u32 pos = k * L + j;
    if (pos > last) pos = last;
    u32 lo = 0, hi = L;                                      // the entry i with off[i] <= pos < off[i + 1] (runs are non-empty: off is strictly increasing)
    while (hi - lo > 1) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= pos) lo = mid; else hi = mid;
    }
    const ulonglong2* src = (const ulonglong2*)(table + 4 * (size_t)lo);
    ulonglong2* dst = (ulonglong2*)(out + 4 * ((size_t)k * out_stride + e));
    const ulonglong2 a = src[0], b = src[1];
    dst[0] = a; dst[1] = b;
}

// scratch: words for sorted_scratch_words(L) u32; status_dev = 2 words inside it (see sorted_status_offset).  Queues everything on C.stream.
size_t lookup_sorted_scratch_words(size_t L) { return lookup_slots(L) + 2 * (L + 1) + 2; }
size_t lookup_sorted_status_offset(size_t L) { return lookup_slots(L) + 2 * (L + 1); }

int lookup_sorted_run(Context& C, const uint64_t* table_dev, size_t L, const uint64_t* values_dev, size_t value_stride, size_t mpr, uint64_t* out_dev,
                      size_t out_stride, uint32_t* scratch_dev) {
    KH_REQUIRE(L >= 1 && mpr >= 1 && (mpr + 1) * L < ((size_t)1 << 31), "lookup_sorted_run: bad shape");
    const size_t cap = lookup_slots(L);
    u32* const slots = scratch_dev;
    u32* const cnt = slots + cap;
    u32* const off = cnt + (L + 1);
    u32* const status = off + (L + 1);
    const u32 mask = (u32)(cap - 1);
    const dim3 block(256);
    auto blocks = [](size_t threads) { return dim3((unsigned)((threads + 255) / 256)); };
    hipLaunchKernelGGL(k_sorted_clear, blocks(cap), block, 0, C.stream, slots, (u32)cap, cnt, (u32)L, status);
    hipLaunchKernelGGL(k_sorted_build, blocks(L), block, 0, C.stream, table_dev, (u32)L, slots, mask);
    hipLaunchKernelGGL(k_sorted_count, blocks(mpr * L), block, 0, C.stream, table_dev, values_dev, value_stride, (u32)L, (u32)(mpr * L), slots, mask, cnt, status);
    KH_HIP(hipGetLastError());
    int rc = exclusive_scan_u32(cnt, off, L + 1, C.scratch("lookup_sorted_scan"), C.stream);
    if (rc) return rc;
    const size_t total = (mpr + 1) * (L + 1);                // < 2^32: mpr + 1 <= (mpr + 1) L < 2^31
    hipLaunchKernelGGL(k_sorted_expand, blocks(total), block, 0, C.stream, table_dev, off, (u32)L, (u32)(mpr + 1), (u32)total, out_dev, out_stride, status);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

}  // namespace kh
