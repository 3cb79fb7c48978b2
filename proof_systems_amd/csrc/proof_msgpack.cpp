// proof_msgpack.cpp -- the reference's serialised ProverProof and VerifierIndex (rmp-serde msgpack) at the C ABI: kh_proofs_from_msgpack,
// kh_proof_to_wire, kh_proof_to_msgpack, kh_verifier_index_from_msgpack, kh_verifier_index_to_msgpack.
//
//   bytes -> handle   proof_wire.hpp walks the structure on the host and refuses what is malformed before any device work; the points of everything the call
//                     reads -- all k proofs with their previous-challenge commitments, or all commitments of an index -- are decoded in ONE launch of
//                     k_points_decompress (point_codec.hip); the elements become Montgomery limbs on the host.  The handles are then made by
//                     kh_proof_from_sections / kh_verifier_index_new, so they are the ones a caller's own sections would have given.
//   handle -> bytes   every point of the handle through ONE launch of k_points_compress, the elements out of Montgomery form on the host, then the walk
//                     backwards.  A size query writes the same structure over zero-filled records and launches nothing: the size depends on counts alone.
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/kimchi_hip.h"
#include "host_ec.hpp"
#include "protocol_host.hpp"
#include "wire_handles.hpp"

namespace kh {
const char* point_status_name(unsigned status);      // point_codec.hip
}

namespace {
namespace W = kh_proof_wire;
using khost::fe;

static_assert(W::P_W_COMM == KH_PROOF_W_COMM && W::P_EVALS == KH_PROOF_EVALS && W::P_PUBLIC_EVALS == KH_PROOF_PUBLIC_EVALS && W::P_LR == KH_PROOF_LR &&
              W::P_Z1_Z2 == KH_PROOF_Z1_Z2 && W::P_SG == KH_PROOF_SG && W::P_CHALLENGES == KH_PROOF_CHALLENGES && W::P_LOOKUP_SORTED_COMM == KH_PROOF_LOOKUP_SORTED_COMM &&
              W::P_SECTIONS == KH_PROOF_LOOKUP_RUNTIME_COMM + 1 && W::POINT == KH_POINT_BYTES, "proof_wire.hpp numbers the proof sections as kimchi_hip.h does");
static_assert(W::V_SIGMA_COMM == KH_VINDEX_SIGMA_COMM && W::V_OPTIONAL_COMM == KH_VINDEX_OPTIONAL_COMM && W::V_SHIFTS == KH_VINDEX_SHIFTS && W::V_DIGEST == KH_VINDEX_DIGEST &&
              W::V_LOOKUP_TABLE_COMM == KH_VINDEX_LOOKUP_TABLE_COMM && W::V_LOOKUP_RUNTIME_SELECTOR_COMM == KH_VINDEX_LOOKUP_RUNTIME_SELECTOR_COMM &&
              W::V_SECTIONS == KH_VINDEX_LOOKUP_INFO + 1, "proof_wire.hpp numbers the index sections as kimchi_hip.h does");

#define KM_INVALID(...) do { kh::set_error(__VA_ARGS__); return KH_E_INVALID; } while (0)
#define KM(expr) do { int rc_ = (expr); if (rc_ != KH_OK) return rc_; } while (0)

const char* const OPTIONAL_GATE_NAMES[6] = {"RangeCheck0", "RangeCheck1", "ForeignFieldAdd", "ForeignFieldMul", "Xor16", "Rot64"};
const char* const VINDEX_SECTION_NAMES[KH_VINDEX_LOOKUP_INFO + 1] = {"sigma_comm", "coefficients_comm", "generic_comm", "selector_comm", "optional_comm", "shifts", "digest",
                                                                     "lookup_table_comm", "lookup_table_ids_comm", "lookup_selector_comm", "lookup_runtime_selector_comm", "lookup_info"};
bool proof_point_section(int s) { return s <= KH_PROOF_PUBLIC_COMM || s == KH_PROOF_LR || s == KH_PROOF_DELTA || s == KH_PROOF_SG || s >= KH_PROOF_LOOKUP_SORTED_COMM; }
bool vindex_point_section(int s) { return s != KH_VINDEX_SHIFTS && s != KH_VINDEX_DIGEST && s != KH_VINDEX_LOOKUP_INFO; }

// count elements, Montgomery limbs -> 32 little-endian bytes of the canonical integer each
void elements_out(const khost::Fld& F, const uint64_t* limbs, size_t count, uint8_t* out) {
    for (size_t i = 0; i < count; i++) {
        const fe v = F.from_mont(kh_protocol::load(limbs + 4 * i));
        memcpy(out + 32 * i, v.l, 32);                                   // (little-endian hosts only, as everywhere in the library)
    }
}
// the lists of points a handle holds, gathered for one launch of the encoder and scattered back as records
struct PointBatch {
    std::vector<uint64_t> xy; std::vector<uint8_t> inf;
    struct Part { uint8_t* out; size_t first, count; };
    std::vector<Part> parts;
    void add(const uint64_t* limbs, const uint8_t* flags, size_t count, uint8_t* out) {
        if (!count) return;
        parts.push_back(Part{out, inf.size(), count});
        xy.insert(xy.end(), limbs, limbs + 8 * count);
        if (flags) inf.insert(inf.end(), flags, flags + count); else inf.insert(inf.end(), count, 0);
    }
    int run(int curve) {
        if (inf.empty()) return KH_OK;
        std::vector<uint8_t> rec(inf.size() * KH_POINT_BYTES);
        KM(kh_points_compress(curve, xy.data(), inf.data(), inf.size(), rec.data()));
        for (const Part& p : parts) memcpy(p.out, rec.data() + p.first * KH_POINT_BYTES, p.count * KH_POINT_BYTES);
        return KH_OK;
    }
};

// the sections and previous challenges of a handle in wire form; fill = false: the counts, zero-filled records, nothing launched
int proof_to_wire_form(int curve, const kh_proof_t* proof, bool fill, W::Proof* out) {
    const khost::Fld F(khost::scalar_field_id(curve));
    PointBatch batch;
    for (int s = 0; s <= KH_PROOF_LOOKUP_RUNTIME_COMM; s++) {
        const uint64_t* limbs = nullptr; const uint8_t* flags = nullptr; size_t count = 0;
        KM(kh_proof_section(proof, s, &limbs, &flags, &count));
        W::Section& o = out->sec[s];
        o.count = count;
        o.bytes.assign(count * (proof_point_section(s) ? W::POINT : W::ELEM), 0);
        if (!fill) continue;
        if (proof_point_section(s)) batch.add(limbs, flags, count, o.bytes.data());
        else elements_out(F, limbs, count, o.bytes.data());
    }
    const kh::ProofPrev& pv = kh::proof_prev(proof);
    out->prev.resize(pv.rounds.size());
    size_t cpos = 0, ppos = 0;
    for (size_t j = 0; j < pv.rounds.size(); j++) {
        W::PrevChallenge& pc = out->prev[j];
        pc.chals.count = pv.rounds[j]; pc.chals.bytes.assign(W::ELEM * pc.chals.count, 0);
        pc.comm.count = pv.comm_chunks[j]; pc.comm.bytes.assign(W::POINT * pc.comm.count, 0);
        if (fill) {
            elements_out(F, pv.chals.data() + 4 * cpos, pc.chals.count, pc.chals.bytes.data());
            batch.add(pv.comm_xy.data() + 8 * ppos, pv.comm_inf.data() + ppos, pc.comm.count, pc.comm.bytes.data());
        }
        cpos += pc.chals.count; ppos += pc.comm.count;
    }
    return fill ? batch.run(curve) : KH_OK;
}

// size query, capacity check, copy: what the three writers share.  make(fill, &bytes) builds the output
template <class Make>
int emit(const char* call, Make make, uint8_t* out, size_t cap, size_t* len) {
    std::vector<uint8_t> bytes;
    KM(make(false, &bytes));
    *len = bytes.size();
    if (!out) return KH_OK;
    if (cap < bytes.size()) KM_INVALID("%s: %zu bytes are needed, the buffer has %zu", call, bytes.size(), cap);
    KM(make(true, &bytes));
    memcpy(out, bytes.data(), bytes.size());
    return KH_OK;
}

// the seven elements of the domain record for 2^log2_n rows, as canonical little-endian bytes: n, 1/n, omega, 1/omega, 1, 1, 1
int domain_elements(int fid, unsigned log2_n, uint8_t out[32 * W::DOMAIN_ELEMS]) {
    const khost::Fld F(fid);
    uint64_t w[4];
    KM(kh_domain_generator(fid, log2_n, w));
    const fe n = F.to_mont(fe{{(uint64_t)1 << log2_n, 0, 0, 0}}), omega = kh_protocol::load(w);
    const fe e[W::DOMAIN_ELEMS] = {n, F.inv(n), omega, F.inv(omega), F.f.one, F.f.one, F.f.one};
    elements_out(F, e[0].l, W::DOMAIN_ELEMS, out);
    return KH_OK;
}
}  // namespace

extern "C" {

int kh_proofs_from_msgpack(int curve, const uint8_t* const* bytes, const size_t* lens, size_t k, kh_proof_t** out) {
    const char* const call = "kh_proofs_from_msgpack";
    if (out) for (size_t p = 0; p < k; p++) out[p] = nullptr;
    if (curve != KH_CURVE_VESTA && curve != KH_CURVE_PALLAS) KM_INVALID("%s: unknown curve id %d", call, curve);
    if (!bytes || !lens || !out || k == 0) KM_INVALID("%s: null argument or no proof", call);
    // ---- the host walk: everything malformed is refused here
    const khost::Fld F(khost::scalar_field_id(curve));
    std::vector<W::Proof> wp(k);
    std::vector<kh::ProofPrev> prev(k);
    std::vector<std::vector<uint8_t>> prev_records(k);
    char err[256];
    for (size_t p = 0; p < k; p++) {
        if (!bytes[p]) KM_INVALID("%s: proof %zu: null bytes", call, p);
        if (W::read_proof(bytes[p], lens[p], &wp[p], err, sizeof(err))) KM_INVALID("%s: proof %zu: %s", call, p, err);
        for (size_t j = 0; j < wp[p].prev.size(); j++) {
            const W::PrevChallenge& pc = wp[p].prev[j];
            for (size_t i = 0; i < pc.chals.count; i++) {
                fe v;
                memcpy(v.l, pc.chals.bytes.data() + 32 * i, 32);
                if (khost::geq(v, F.f.p)) KM_INVALID("%s: proof %zu previous challenge %zu element %zu is not a canonical field element (>= p)", call, p, j, i);
                v = F.to_mont(v);
                prev[p].chals.insert(prev[p].chals.end(), v.l, v.l + 4);
            }
            prev[p].rounds.push_back((unsigned)pc.chals.count);
            prev[p].comm_chunks.push_back(pc.comm.count);
            prev_records[p].insert(prev_records[p].end(), pc.comm.bytes.begin(), pc.comm.bytes.end());
        }
    }
    // ---- one decode launch for the points of all k, the handles as kh_proofs_from_wire makes them
    const size_t ns = KH_PROOF_LOOKUP_RUNTIME_COMM + 1;
    std::vector<kh_wire_section_t> secs(k * ns), extra(k);
    for (size_t p = 0; p < k; p++) {
        for (size_t s = 0; s < ns; s++) secs[p * ns + s] = kh_wire_section_t{wp[p].sec[s].bytes.data(), wp[p].sec[s].count};
        extra[p] = kh_wire_section_t{prev_records[p].data(), prev_records[p].size() / KH_POINT_BYTES};
    }
    std::vector<std::vector<uint64_t>> prev_xy(k);
    std::vector<std::vector<uint8_t>> prev_inf(k);
    std::vector<kh_proof_t*> made(k, nullptr);
    KM(kh::proofs_from_wire(call, curve, secs.data(), ns, k, extra.data(), prev_xy.data(), prev_inf.data(), made.data()));
    for (size_t p = 0; p < k; p++) {
        prev[p].comm_xy = std::move(prev_xy[p]); prev[p].comm_inf = std::move(prev_inf[p]);
        kh::proof_set_prev(made[p], std::move(prev[p]));
        kh::proof_set_shape(made[p], wp[p].shape);
        out[p] = made[p];
    }
    return KH_OK;
}

int kh_proof_to_wire(int curve, const kh_proof_t* proof, uint8_t* out, size_t cap, size_t* len, kh_wire_section_t* sections) {
    const char* const call = "kh_proof_to_wire";
    if (curve != KH_CURVE_VESTA && curve != KH_CURVE_PALLAS) KM_INVALID("%s: unknown curve id %d", call, curve);
    if (!proof || !len || (out && !sections)) KM_INVALID("%s: null argument", call);
    auto make = [&](bool fill, std::vector<uint8_t>* bytes) -> int {
        W::Proof wp;
        KM(proof_to_wire_form(curve, proof, fill, &wp));
        bytes->clear();
        for (int s = 0; s <= KH_PROOF_LOOKUP_RUNTIME_COMM; s++) {
            if (fill) sections[s] = kh_wire_section_t{wp.sec[s].count ? out + bytes->size() : nullptr, wp.sec[s].count};
            bytes->insert(bytes->end(), wp.sec[s].bytes.begin(), wp.sec[s].bytes.end());
        }
        return KH_OK;
    };
    return emit(call, make, out, cap, len);
}

int kh_proof_to_msgpack(int curve, const kh_proof_t* proof, const kh_verifier_index_t* shape, uint8_t* out, size_t cap, size_t* len) {
    const char* const call = "kh_proof_to_msgpack";
    if (curve != KH_CURVE_VESTA && curve != KH_CURVE_PALLAS) KM_INVALID("%s: unknown curve id %d", call, curve);
    if (!proof || !len) KM_INVALID("%s: null argument", call);
    W::Shape sh = kh::proof_shape(proof);
    if (shape) {
        kh::VindexView v;
        kh::vindex_view(shape, &v);
        if (v.curve != curve) KM_INVALID("%s: the shape index is over curve %d, the call names curve %d", call, v.curve, curve);
        const W::Shape of_index = kh::vindex_shape(v);
        if (sh.known && !sh.same(of_index))
            KM_INVALID("%s: the proof's own shape (optional gates 0x%02x, lookup %d, patterns 0x%x, %u lookups per row, runtime tables %d) is not the shape index's (0x%02x, %d, 0x%x, %u, %d)",
                       call, sh.optional, (int)sh.lookup, sh.patterns, sh.max_per_row, (int)sh.runtime, of_index.optional, (int)of_index.lookup, of_index.patterns,
                       of_index.max_per_row, (int)of_index.runtime);
        sh = of_index;
    }
    if (!sh.known)
        KM_INVALID("%s: the proof carries no shape (it comes from kh_proof_from_sections or kh_proofs_from_wire) and no shape index is given: which optional evaluations it has is not known", call);
    auto make = [&](bool fill, std::vector<uint8_t>* bytes) -> int {
        W::Proof wp;
        KM(proof_to_wire_form(curve, proof, fill, &wp));
        wp.sec[KH_PROOF_PUBLIC_COMM] = W::Section(); wp.sec[KH_PROOF_CHALLENGES] = W::Section();      // not part of the serialised proof
        wp.shape = sh;
        char err[256];
        if (W::write_proof(wp, bytes, err, sizeof(err))) KM_INVALID("%s: %s", call, err);
        return KH_OK;
    };
    return emit(call, make, out, cap, len);
}

int kh_verifier_index_from_msgpack(kh_srs_t* srs, const uint8_t* bytes, size_t len, kh_verifier_index_t** out) {
    const char* const call = "kh_verifier_index_from_msgpack";
    if (out) *out = nullptr;
    if (!srs || !bytes || !out) KM_INVALID("%s: null argument", call);
    const int curve = kh_srs_curve(srs), fid = khost::scalar_field_id(curve);
    const khost::Fld F(fid);
    // ---- the host walk, twice over two kilobytes: the first pass gives log_size, the second compares the domain record with the library's own
    W::Index wi;
    char err[256];
    if (W::read_index(bytes, len, nullptr, kh_srs_size(srs), &wi, err, sizeof(err))) KM_INVALID("%s: %s", call, err);
    if (wi.log_size == 0 || wi.log_size > 26) KM_INVALID("%s: VerifierIndex: a domain of 2^%u rows is not supported", call, wi.log_size);
    uint8_t domain[32 * W::DOMAIN_ELEMS];
    KM(domain_elements(fid, wi.log_size, domain));
    if (W::read_index(bytes, len, domain, kh_srs_size(srs), &wi, err, sizeof(err))) KM_INVALID("%s: %s", call, err);
    if (wi.zk_rows > 0xffffffffu || wi.public_inputs > 0xffffffffu || wi.prev_challenges > 0xffffffffu)
        KM_INVALID("%s: VerifierIndex: zk_rows %llu, public %llu, prev_challenges %llu", call, (unsigned long long)wi.zk_rows, (unsigned long long)wi.public_inputs,
                   (unsigned long long)wi.prev_challenges);
    fe shifts[W::PERMUTS];
    for (size_t i = 0; i < W::PERMUTS; i++) {
        memcpy(shifts[i].l, wi.sec[KH_VINDEX_SHIFTS].bytes.data() + 32 * i, 32);
        if (khost::geq(shifts[i], F.f.p)) KM_INVALID("%s: section shifts element %zu is not a canonical field element (>= p)", call, i);
        shifts[i] = F.to_mont(shifts[i]);
    }
    std::vector<int> optional;
    for (int slot = 0; slot < 6; slot++) {
        if (!(wi.optional >> slot & 1)) continue;
        int gid = -1;
        for (int g = 0; g < kh_gate_count(); g++) if (!strcmp(kh_gate_name(g), OPTIONAL_GATE_NAMES[slot])) gid = g;
        if (gid < 0) KM_INVALID("%s: the library has no gate %s", call, OPTIONAL_GATE_NAMES[slot]);
        optional.push_back(gid);
    }
    // ---- one decode launch for every commitment of the index
    std::vector<uint8_t> records;
    size_t first[KH_VINDEX_LOOKUP_INFO + 2] = {0};
    for (int s = 0; s <= KH_VINDEX_LOOKUP_INFO; s++) {
        first[s + 1] = first[s];
        if (!vindex_point_section(s)) continue;
        records.insert(records.end(), wi.sec[s].bytes.begin(), wi.sec[s].bytes.end());
        first[s + 1] += wi.sec[s].count;
    }
    const size_t n_points = first[KH_VINDEX_LOOKUP_INFO + 1];
    std::vector<uint64_t> xy(8 * n_points);
    std::vector<uint8_t> inf(n_points), status(n_points);
    size_t bad = 0;
    const int rc = kh_points_decompress(curve, records.data(), n_points, xy.data(), inf.data(), status.data(), &bad);
    if (rc == KH_E_INVALID && bad < n_points && status[bad] != KH_POINT_OK && status[bad] != KH_POINT_INFINITY) {
        int s = 0;
        while (bad >= first[s + 1]) s++;
        KM_INVALID("%s: section %s point %zu is %s", call, VINDEX_SECTION_NAMES[s], bad - first[s], kh::point_status_name(status[bad]));
    }
    KM(rc);
    kh_section_t secs[KH_VINDEX_LOOKUP_INFO + 1] = {};
    for (int s = 0; s <= KH_VINDEX_LOOKUP_INFO; s++)
        if (vindex_point_section(s) && wi.sec[s].count) secs[s] = kh_section_t{xy.data() + 8 * first[s], inf.data() + first[s], wi.sec[s].count};
    secs[KH_VINDEX_SHIFTS] = kh_section_t{shifts[0].l, nullptr, W::PERMUTS};
    const uint64_t info[8] = {wi.max_per_row, wi.max_joint_size, wi.joint_lookup_used ? 1u : 0u, wi.uses_runtime_tables ? 1u : 0u, wi.patterns,
                              wi.chunks ? wi.sec[KH_VINDEX_LOOKUP_TABLE_COMM].count / wi.chunks : 0, 0, 0};
    if (wi.lookup) secs[KH_VINDEX_LOOKUP_INFO] = kh_section_t{info, nullptr, 2};
    return kh_verifier_index_new(srs, wi.log_size, (unsigned)wi.zk_rows, (unsigned)wi.public_inputs, (unsigned)wi.prev_challenges, optional.data(), optional.size(), secs,
                                 KH_VINDEX_LOOKUP_INFO + 1, out);
}

int kh_verifier_index_to_msgpack(const kh_verifier_index_t* vix, unsigned prev_challenges, uint8_t* out, size_t cap, size_t* len) {
    const char* const call = "kh_verifier_index_to_msgpack";
    if (!vix || !len) KM_INVALID("%s: null argument", call);
    kh::VindexView v;
    kh::vindex_view(vix, &v);
    if (!v.any_prev && prev_challenges != v.prev_challenges) KM_INVALID("%s: prev_challenges %u, the index carries %zu", call, prev_challenges, v.prev_challenges);
    const int fid = khost::scalar_field_id(v.curve);
    const khost::Fld F(fid);
    auto make = [&](bool fill, std::vector<uint8_t>* bytes) -> int {
        W::Index wi;
        wi.domain_size = (uint64_t)1 << v.log2_n; wi.log_size = v.log2_n;
        wi.max_poly_size = kh_srs_size(v.srs); wi.zk_rows = v.zk_rows; wi.public_inputs = v.public_inputs; wi.prev_challenges = prev_challenges;
        wi.chunks = v.chunks; wi.optional = v.optional;
        wi.lookup = v.lookup; wi.joint_lookup_used = v.joint_lookup_used; wi.uses_runtime_tables = v.runtime; wi.patterns = v.patterns;
        wi.max_per_row = v.max_per_row; wi.max_joint_size = v.max_joint_size;
        PointBatch batch;
        for (int s = 0; s <= KH_VINDEX_LOOKUP_INFO; s++) {
            if (!vindex_point_section(s)) continue;
            wi.sec[s].count = v.sec[s].count;
            wi.sec[s].bytes.assign(W::POINT * v.sec[s].count, 0);
            if (fill) batch.add(v.sec[s].limbs, v.sec[s].flags, v.sec[s].count, wi.sec[s].bytes.data());
        }
        wi.sec[KH_VINDEX_SHIFTS].count = W::PERMUTS;
        wi.sec[KH_VINDEX_SHIFTS].bytes.assign(W::ELEM * W::PERMUTS, 0);
        if (fill) {
            elements_out(F, v.shifts, W::PERMUTS, wi.sec[KH_VINDEX_SHIFTS].bytes.data());
            KM(domain_elements(fid, v.log2_n, wi.domain));
            KM(batch.run(v.curve));
        }
        char err[256];
        if (W::write_index(wi, bytes, err, sizeof(err))) KM_INVALID("%s: %s", call, err);
        return KH_OK;
    };
    return emit(call, make, out, cap, len);
}

}  // extern "C"
