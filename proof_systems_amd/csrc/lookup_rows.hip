// lookup_rows.hip -- the rows of GateType::Lookup on the device, for kh_lookup_witness_dev and KH_STEP_LOOKUP (csrc/witness_steps.cpp): a row holds
// (table id, key, value, key, value, key, value); the circuit knows the keys, the values are what the table holds at them.  The table is two device
// columns of table_len elements -- keys and values --, the keys of the call n x 3 elements; a hash set over the table's keys is built per call in
// scratch and probed once per (slot, instance).  No field arithmetic: elements are compared as 32-byte strings (lookup_hash.hpp), with the scheme of
// lookup_sorted.hip.
//
//   (memset)          slots = EMPTY (0xff bytes)
//   k_lookup_build    one lane per table entry t that differs from entry t - 1: linear probing, atomicCAS(slot, EMPTY, t); a slot whose entry has the
//                     same 32 bytes takes atomicMin(slot, t).  A slot goes from empty to occupied once and never changes the key it stands for, so
//                     equal keys meet in one slot and that slot ends at the LOWEST index, whatever the arrival order
//   k_lookup_rows     one lane per (slot k, instance i), slot-major: g = k n + i.  Probe (at most capacity steps; a slot value >= table_len is a miss,
//                     whatever the slots hold), then cell 2k + 1 = the key, cell 2k + 2 = the value (zero on a miss, which raises the flag), the
//                     lanes of slot 0 also cell 0 = the table id; out_values[3 i + k] = the value.  A wave of one slot stores a column at 64 rows,
//                     consecutive ones when the instances are packed densely
// Elements move in 16-byte loads and stores; the slots are u32.  Blocks of one wave, no LDS, no scratch memory.  The launches follow each other on
// one stream: the kernel boundary is the only ordering between clearing, building and probing.
#include "common.hpp"
#include "api_internal.hpp"
#include "lookup_key.cuh"

namespace kh {

namespace {
typedef uint32_t u32;
typedef uint64_t u64;
constexpr u32 LOOKUP_EMPTY = 0xffffffffu;
struct TableId { u64 l[4]; };

__device__ __forceinline__ void store_key(u64* __restrict__ p, const Key& k) {
    ((ulonglong2*)p)[0] = make_ulonglong2(k.l[0], k.l[1]);
    ((ulonglong2*)p)[1] = make_ulonglong2(k.l[2], k.l[3]);
}
}  // namespace

__global__ void __launch_bounds__(WAVE_BLOCK)
k_lookup_build(const u64* __restrict__ table_keys, u32 L, u32* __restrict__ slots, u32 mask) {
    const u32 t = blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (t >= L) return;
    const Key me = load_key(table_keys + 4 * (size_t)t);
    // an entry equal to its predecessor is never a first occurrence, and the head of its run inserts the key (lookup_sorted.hip: a padded table ends
    // in thousands of equal rows, whose atomics would all land on one slot)
    if (t > 0 && same(load_key(table_keys + 4 * (size_t)(t - 1)), me)) return;
    u32 h = (u32)hash(me) & mask;
    for (u32 step = 0; step <= mask; step++) {                // (at most L of >= 2 L slots are ever occupied: the walk ends long before)
        u32 cur = __hip_atomic_load(&slots[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == LOOKUP_EMPTY) {
            cur = atomicCAS(&slots[h], LOOKUP_EMPTY, t);
            if (cur == LOOKUP_EMPTY) return;                  // claimed
        }
        if (cur >= L) return;                                 // (never: only indices below L are written after the clear)
        if (same(load_key(table_keys + 4 * (size_t)cur), me)) {   // (the slot's index only ever decreases: one that is already lower needs no atomic)
            if (t < cur) atomicMin(&slots[h], t);
            return;
        }
        h = (h + 1) & mask;
    }
}

__global__ void __launch_bounds__(WAVE_BLOCK)
k_lookup_rows(const u64* __restrict__ table_keys, const u64* __restrict__ table_values, u32 L, const u64* __restrict__ keys, size_t n,
              const u32* __restrict__ slots, u32 mask, TableId id, WitnessPlace at, u64* __restrict__ out_values, u32* __restrict__ flags, u32 bit) {
    const size_t g = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool miss = false;
    if (g < 3 * n) {
        const size_t k = (g >= n ? 1 : 0) + (g >= 2 * n ? 1 : 0), i = g - k * n;
        const Key key = load_key(keys + 4 * (3 * i + k));
        Key value{{0, 0, 0, 0}};
        miss = true;
        u32 h = (u32)hash(key) & mask;
        for (u32 step = 0; step <= mask; step++) {
            const u32 e = slots[h];
            if (e >= L) break;                                // empty, or not an index of this table: not in the table
            if (same(load_key(table_keys + 4 * (size_t)e), key)) { value = load_key(table_values + 4 * (size_t)e); miss = false; break; }
            h = (h + 1) & mask;
        }
        const size_t row = at.start_row(i);
        if (k == 0) { Key t; t.l[0] = id.l[0]; t.l[1] = id.l[1]; t.l[2] = id.l[2]; t.l[3] = id.l[3]; store_key(at.cell(row, 0), t); }
        store_key(at.cell(row, 2 * k + 1), key);
        store_key(at.cell(row, 2 * k + 2), value);
        if (out_values) store_key(out_values + 4 * (3 * i + k), value);
    }
    if (flags && __any(miss) && (threadIdx.x & 63u) == 0) atomicOr(flags, 1u << bit);
}

// the slots of a table of L entries: lookup_slots(L) u32 (lookup_hash.hpp)
size_t lookup_rows_slot_bytes(size_t table_len) { return lookup_slots(table_len) * sizeof(u32); }

// (the callers in witness_steps.cpp have validated pointers, sizes and the placement: 1 <= table_len < 2^31, n >= 1, 3 n lanes fit a grid; slots_dev
// holds scratch_bytes, which the caller asked lookup_rows_slot_bytes for)
int lookup_rows(Context& C, const uint64_t* table_id, const uint64_t* table_keys_dev, const uint64_t* table_values_dev, size_t table_len,
                const uint64_t* keys_dev, size_t n, const WitnessPlace& at, uint64_t* out_values_dev, uint32_t* flags_dev, unsigned bit, uint32_t* slots_dev,
                size_t scratch_bytes) {
    const size_t cap = lookup_slots(table_len);
    KH_REQUIRE(slots_dev && scratch_bytes >= cap * sizeof(u32) && table_len >= 1 && table_len < ((size_t)1 << 31) && n >= 1 && n <= WAVE_BLOCK_MAX_N / 3,
               "lookup_rows: bad shape");
    TableId id;
    memcpy(id.l, table_id, sizeof(id.l));
    const u32 mask = (u32)(cap - 1);
    C.timer.begin(C.stream);
    KH_HIP(hipMemsetAsync(slots_dev, 0xff, cap * sizeof(u32), C.stream));
    hipLaunchKernelGGL(k_lookup_build, blocks_of(table_len, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)table_keys_dev, (u32)table_len, slots_dev, mask);
    KH_HIP(hipGetLastError());
    C.timer.mark("lookup_build", C.stream);
    hipLaunchKernelGGL(k_lookup_rows, blocks_of(3 * n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)table_keys_dev, (const u64*)table_values_dev,
                       (u32)table_len, (const u64*)keys_dev, n, (const u32*)slots_dev, mask, id, at, (u64*)out_values_dev, flags_dev, (u32)bit);
    KH_HIP(hipGetLastError());
    C.timer.mark("lookup_rows", C.stream);
    return KH_OK;
}

}  // namespace kh
