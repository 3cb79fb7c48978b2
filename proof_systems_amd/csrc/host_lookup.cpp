// host_lookup.cpp -- the `sorted` step of the lookup argument (kimchi/src/circuits/lookup/constraints.rs:90-194) on the host.
//
// The reference counts, with a HashMap over field elements, how often every entry of the combined table is looked up, repeats each entry
// (count + 1) times in table order and lays the result out as max_per_row + 1 "snake" columns (consecutive columns share one element, every
// second column is reversed).  That is a hash join between two vectors.  This file is the host entry point, kh_lookup_sorted: host vectors in, host
// vectors out, one thread (the Python loop it replaced cost 0.36 s of a 0.38 s proof at 2^16 rows).  kh_prove and the Python prover no longer come
// through here: their values and table are device-resident and csrc/lookup_sorted.hip (kh_lookup_sorted_dev) runs the same join there, without the
// two transfers.  This function stays for callers with host-side columns and as the reference the device path is tested against, position for
// position (tests/test_gpu_lookup_sorted_dev.py); the hash (lookup_hash.hpp) and the first-occurrence rule below are the ones the kernels use.
// Nothing here does field arithmetic: values are compared as 32-byte strings (canonical Montgomery limbs are unique).
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/kimchi_hip.h"
#include "lookup_hash.hpp"

namespace kh { void set_error(const char* fmt, ...); }

using namespace kh;                                     // Key, same, hash, lookup_slots

extern "C" int kh_lookup_sorted(const uint64_t* table, size_t lookup_rows, const uint64_t* values, size_t value_stride, size_t max_per_row, uint64_t* out,
                                size_t* bad_row) {
    if (!table || !values || !out || lookup_rows == 0 || max_per_row == 0 || value_stride < lookup_rows) { kh::set_error("kh_lookup_sorted: bad argument"); return KH_E_INVALID; }
    if (bad_row) *bad_row = (size_t)-1;
    const Key* T = (const Key*)table;
    const size_t cap = lookup_slots(lookup_rows);
    const size_t mask = cap - 1;
    std::vector<uint32_t> slot(cap, 0xffffffffu);      // open addressing: table index of the FIRST occurrence of a value
    std::vector<uint32_t> cnt(lookup_rows, 1);         // counts live on first occurrences; a repeated table entry keeps its 1
    std::vector<uint8_t> first(lookup_rows, 0);
    for (size_t i = 0; i < lookup_rows; i++) {
        size_t h = hash(T[i]) & mask;
        while (slot[h] != 0xffffffffu && !same(T[slot[h]], T[i])) h = (h + 1) & mask;
        if (slot[h] == 0xffffffffu) { slot[h] = (uint32_t)i; first[i] = 1; }
    }
    for (size_t s = 0; s < max_per_row; s++) {
        const Key* V = (const Key*)(values + 4 * s * value_stride);
        for (size_t r = 0; r < lookup_rows; r++) {
            size_t h = hash(V[r]) & mask;
            while (slot[h] != 0xffffffffu && !same(T[slot[h]], V[r])) h = (h + 1) & mask;
            if (slot[h] == 0xffffffffu) {               // a looked-up value that is not in the table (constraints.rs:137-141)
                if (bad_row) *bad_row = r;
                kh::set_error("lookup in row %zu (slot %zu): the value is not in the table", r, s);
                return KH_E_INVALID;
            }
            cnt[slot[h]]++;
        }
    }
    // the sorted multiset, table order, cut into max_per_row + 1 columns of lookup_rows values + the snake's shared element
    const size_t L = lookup_rows, W = L + 1;
    Key* O = (Key*)out;
    size_t pos = 0;
    for (size_t i = 0; i < L; i++) {
        const size_t c = first[i] ? cnt[i] : 1;
        for (size_t j = 0; j < c; j++, pos++) O[(pos / L) * W + pos % L] = T[i];
    }
    if (pos != (max_per_row + 1) * L) { kh::set_error("kh_lookup_sorted: %zu values for %zu places", pos, (max_per_row + 1) * L); return KH_E_INVALID; }
    for (size_t k = 0; k < max_per_row; k++) O[k * W + L] = O[(k + 1) * W];
    O[max_per_row * W + L] = O[max_per_row * W + L - 1];
    for (size_t k = 1; k <= max_per_row; k += 2)
        for (size_t a = 0, b = L; a < b; a++, b--) { Key t = O[k * W + a]; O[k * W + a] = O[k * W + b]; O[k * W + b] = t; }
    return KH_OK;
}
