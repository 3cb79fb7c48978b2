// gate_batch.hpp -- what csrc/verifier.cpp hands to gates.hip for the constant term of a batch of proofs: plain data, no device types (as witness_lookup.hpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace kh {
// one launch of a gate type over the whole batch: the kh_gate_name id, the column its selector's evaluations are in, and every item's constants table
// (items x kh_gate_num_constants x 4 Montgomery limbs, host memory, filled by kh_gate_constants)
struct GateBatchLaunch { int gate; int selector_col; const uint64_t* consts; };
}  // namespace kh
