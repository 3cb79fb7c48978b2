// wire_handles.hpp -- what proof_msgpack.cpp needs from the translation units that own the handles: the shape and the previous challenges a kh_proof
// carries (prover.cpp), a view of a kh_verifier_index (verifier.cpp), and kh_proofs_from_wire's body with one more list of points per proof (point_codec.hip).
#pragma once
#include <vector>

#include "../../include/kimchi_hip.h"
#include "proof_wire.hpp"

namespace kh {

// RecursionChallenges in exactly the arrays kh_verify_item_t and kh_prove_recursive take
struct ProofPrev {
    std::vector<uint64_t> chals, comm_xy;
    std::vector<unsigned> rounds;
    std::vector<uint8_t> comm_inf;
    std::vector<size_t> comm_chunks;
};
const kh_proof_wire::Shape& proof_shape(const kh_proof_t* proof);
void proof_set_shape(kh_proof_t* proof, const kh_proof_wire::Shape& shape);
const ProofPrev& proof_prev(const kh_proof_t* proof);
void proof_set_prev(kh_proof_t* proof, ProofPrev&& prev);

struct VindexView {
    kh_srs_t* srs;
    int curve;
    unsigned log2_n;
    size_t zk_rows, public_inputs, prev_challenges, chunks, max_per_row, max_joint_size;
    bool any_prev;                   // kh_verifier_index_of: the index carries no number of previous challenges
    uint8_t optional, patterns;      // bit k: optional gate / lookup pattern k, as kh_proof_wire::Shape
    bool lookup, joint_lookup_used, runtime;
    const uint64_t* shifts;          // 7 elements, Montgomery limbs
    kh_section_t sec[KH_VINDEX_LOOKUP_INFO + 1];     // the commitment sections; shifts, digest and lookup_info are left empty
};
void vindex_view(const kh_verifier_index_t* vix, VindexView* out);
kh_proof_wire::Shape vindex_shape(const VindexView& v);

// kh_proofs_from_wire under another caller's name.  extra (nullable): k more lists of point records, one per proof, decoded in the SAME launch; their
// affine form comes back in extra_xy[p] / extra_inf[p] (k vectors each).
int proofs_from_wire(const char* call, int curve, const kh_wire_section_t* sections, size_t n_sections, size_t k, const kh_wire_section_t* extra,
                     std::vector<uint64_t>* extra_xy, std::vector<uint8_t>* extra_inf, kh_proof_t** out);

}  // namespace kh
