// witness_lookup.hpp -- what csrc/prover.cpp hands to witness_check.hip for the lookup part of kh_witness_check_full: plain data, no device types, so that
// prover.cpp (public header + host arithmetic only) and the kernel file read one definition.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace kh {

// one joint lookup of a pattern (PATTERNS in csrc/prover.cpp): the table id -- a witness column, or a constant given as Montgomery limbs -- and the
// witness columns of the entry
struct WitnessJointLookup { int tid_is_column, tid_column, ncell, cells[3]; uint64_t id[4]; };
struct WitnessLookupPattern { int pattern, n; const uint64_t* sel; WitnessJointLookup l[4]; };   // sel: the pattern's selector column (d1, device)
struct WitnessLookups {
    size_t npat;
    WitnessLookupPattern pat[4];
    size_t L, W;                                         // rows checked = table rows = n - zk_rows - 1; columns of the combined table
    const uint64_t* const* tcols;                        // host array of W device columns (d1)
    const uint64_t* tids;                                // the table-id column (d1, device), or NULL: every id is 0
    size_t rt_offset, rt_len;                            // the runtime rows of the table
    const uint64_t* runtime;                             // HOST: rt_len elements, column 1 of the runtime rows, or ...
    const uint64_t* runtime_dev;                         // ... the same in DEVICE memory (16-byte aligned), read in stream order; both NULL iff rt_len == 0
};

}  // namespace kh
