// verifier.cpp -- kimchi::verifier::verify / batch_verify (kimchi/src/verifier.rs:126-640, 781-1200, 1275-1373) and the scalar side of SRS::verify
// (poly-commitment/src/ipa.rs:301-470) as a native host loop over this library's own C ABI, the way prover.cpp is ProverProof::create.
//
//   per item   verifier.rs:160-420    Fiat-Shamir replay (kh_sponge_*); the public commitment: kh_msm over the registered Lagrange basis, negated, masked with 1
//              proof.rs:430-470       the evaluations chunk-combined with zeta^srs_len
//   per batch  linearization.rs       the constant term sum_g selector_g(zeta) sum_i alpha^i constraint_i on the proofs' evaluations: ON THE DEVICE, from the
//                                     bodies the quotient and the witness check use (gates.hip: k_gate_batch_*, one constants table per item, one launch per
//                                     gate type present); the lookup constraints as the prover's token program (protocol_host.hpp), one launch per item that has them
//   per item   verifier.rs:412-490    ft_eval0; :834-1175 the evaluation list in opening order, combined_inner_product (commitment.rs:622-657)
//              ipa.rs:330-470         the scalars of SRS::verify
//   per batch  ipa.rs:474-502         ONE MSM: kh_ipa_verify_msm (challenge polynomials expanded on the device over the resident tables + the proofs' points)
//
// f_comm = perm_scalar * sigma_6, ft_comm = f_comm - (zeta^n - 1) t and the combined lookup table (combine_table, lookup/tables/mod.rs:164-199) are linear
// combinations of commitments: instead of computing them as points (a 255-bit scalar multiplication each on the host) their scalars are multiplied out into
// the final MSM's, which takes sigma_6, the chunks of t and the table columns as points of their own.  Same group equation, no group operation on the host.
// The oracle's restatement (oracle/kimchi.py::verify, oracle/pasta.py::ipa_verify_terms) is the line-by-line blueprint and is pinned on the reference's bytes.
#include <stdint.h>
#include <string.h>
#include <chrono>
#include <new>
#include <vector>

#include "../../include/kimchi_hip.h"
#include "gate_batch.hpp"
#include "host_ec.hpp"
#include "protocol_host.hpp"
#include "wire_handles.hpp"

namespace kh {
void prover_index_facts(const kh_prover_index_t* ix, kh_srs_t** srs, unsigned* public_inputs, const int** optional_gates, size_t* n_optional);   // prover.cpp
int verifier_gate_terms_dev(int field, const uint64_t* cols_host, size_t ncols, size_t items, const GateBatchLaunch* launches, size_t nl, uint64_t* out_dev,
                            const uint64_t** cols_dev);                                                                                              // vector_api.cpp
}

namespace {
using namespace kh_protocol;
const char* const LIB_GATES[5] = {"Poseidon", "CompleteAdd", "VarBaseMul", "EndoMul", "EndoMulScalar"};
// the optional gates in column order (proof.rs:95-106) and their position in VerifierIndex::digest (verifier_index.rs:466-480)
const char* const OPTIONAL_GATE_NAMES[6] = {"RangeCheck0", "RangeCheck1", "ForeignFieldAdd", "ForeignFieldMul", "Xor16", "Rot64"};
const int OPTIONAL_DIGEST_ORDER[6] = {0, 1, 3, 2, 4, 5};
// the columns of the constant term's evaluation table (two rows per item): witness, coefficients, the selectors of Generic / the five library gates / the
// six optional gates, then what the lookup constraints read
constexpr size_t C_SEL_GENERIC = 30, C_SEL_LIB = 31, C_SEL_OPT = 36, C_SORTED = 42, C_AGG = 47, C_TABLE = 48, C_RT = 49, C_RTSEL = 50, C_PATSEL = 51,
                 C_VANISH = 55, C_L0 = 56, C_LFINAL = 57, NCOLS = 58;
// polynomial numbers of KH_PROOF_EVALS (the opening order): z, generic selector, five selectors, w x 15, coefficients x 15, sigma x 6, optional selectors, lookups
constexpr size_t P_Z = 0, P_GENERIC = 1, P_LIB = 2, P_W = 7, P_COEFF = 22, P_SIGMA = 37, P_OPT = 43;

bool canonical(const khost::Fld& F, const uint64_t* l) { return !khost::geq(load(l), F.f.p); }
// y^2 = x^3 + 5 (both Pasta curves), coordinates canonical: what a verifier checks before a point reaches the group law
bool on_curve(const khost::Fld& B, const uint64_t* xy) {
    if (!canonical(B, xy) || !canonical(B, xy + 4)) return false;
    const fe x = load(xy), y = load(xy + 4), five = B.to_mont(fe{{5, 0, 0, 0}});
    return khost::eq(B.sqr(y), B.add(B.mul(B.sqr(x), x), five));
}
struct Points {
    std::vector<uint64_t> xy; std::vector<uint8_t> inf; size_t count = 0;
    void set(const uint64_t* p, const uint8_t* f, size_t cnt) { xy.assign(p, p + 8 * cnt); if (f) inf.assign(f, f + cnt); else inf.assign(cnt, 0); count = cnt; }
};
thread_local double tl_phase[4] = {0, 0, 0, 0};
}  // namespace

struct kh_verifier_index {
    kh_srs_t* srs = nullptr;
    int curve = 0, fid = 0;
    unsigned logn = 0;
    size_t n = 0, size = 0, nch = 1, zk = 3, pub = 0, nprev = 0, rounds = 0;
    bool any_prev = false;                               // kh_verifier_index_of: a prover index carries no number of previous challenges
    fe omega, endo, shifts[7], digest;
    std::vector<int> optional, optional_slot;            // kh gate ids in column order; their position among the six optional gates
    int lib_gate[5] = {0, 0, 0, 0, 0}, gid_generic = -1;
    Points sec[KH_VINDEX_LOOKUP_INFO + 1];
    bool lookup = false, joint_used = false, has_rt = false, has_ids = false;
    size_t mpr = 0, mjs = 0, width = 0;
    std::vector<int> pats;
};

namespace kh {
// what kh_verifier_index_to_msgpack and kh_proof_to_msgpack's `shape` argument read of an index (wire_handles.hpp)
void vindex_view(const kh_verifier_index_t* vx, VindexView* out) {
    VindexView& v = *out;
    v = VindexView{};
    v.srs = vx->srs; v.curve = vx->curve; v.log2_n = vx->logn;
    v.zk_rows = vx->zk; v.public_inputs = vx->pub; v.prev_challenges = vx->nprev; v.chunks = vx->nch; v.any_prev = vx->any_prev;
    for (int slot : vx->optional_slot) v.optional |= (uint8_t)(1u << slot);
    for (int q : vx->pats) v.patterns |= (uint8_t)(1u << q);
    v.lookup = vx->lookup; v.joint_lookup_used = vx->joint_used; v.runtime = vx->has_rt; v.max_per_row = vx->mpr; v.max_joint_size = vx->mjs;
    v.shifts = vx->shifts[0].l;
    for (int s = 0; s <= KH_VINDEX_LOOKUP_INFO; s++)
        if (s != KH_VINDEX_SHIFTS && s != KH_VINDEX_DIGEST && s != KH_VINDEX_LOOKUP_INFO) v.sec[s] = kh_section_t{vx->sec[s].xy.data(), vx->sec[s].inf.data(), vx->sec[s].count};
}
kh_proof_wire::Shape vindex_shape(const VindexView& v) {
    kh_proof_wire::Shape sh;
    sh.known = true; sh.optional = v.optional; sh.patterns = v.patterns; sh.lookup = v.lookup; sh.runtime = v.runtime; sh.max_per_row = (unsigned)v.max_per_row;
    return sh;
}
}  // namespace kh

namespace {
int vindex_build(const char* who, kh_srs_t* srs, unsigned log2_n, unsigned zk_rows, unsigned public_inputs, unsigned prev_challenges, bool any_prev,
                 const int* optional_gates, size_t n_optional, const kh_section_t* sections, size_t n_sections, kh_verifier_index_t** out) {
    if (out) *out = nullptr;
    if (!srs || !out || !sections || (n_optional && !optional_gates)) { kh::set_error("%s: null argument", who); return KH_E_INVALID; }
    if (n_sections > KH_VINDEX_LOOKUP_INFO + 1 || log2_n > 26 || log2_n == 0) { kh::set_error("%s: %zu sections, a domain of 2^%u rows", who, n_sections, log2_n); return KH_E_INVALID; }
    for (size_t s = 0; s < n_sections; s++)
        if (sections[s].count && !sections[s].limbs) { kh::set_error("%s: section %zu has %zu entries and no limbs", who, s, sections[s].count); return KH_E_INVALID; }
    kh_verifier_index* vx = new (std::nothrow) kh_verifier_index();
    if (!vx) { kh::set_error("out of memory"); return KH_E_NOMEM; }
    struct Guard { kh_verifier_index* p; ~Guard() { delete p; } } guard{vx};
    vx->srs = srs; vx->curve = kh_srs_curve(srs); vx->fid = khost::scalar_field_id(vx->curve);
    vx->logn = log2_n; vx->n = (size_t)1 << log2_n; vx->size = kh_srs_size(srs);
    const size_t n = vx->n, size = vx->size;
    if (size < 2 || (size & (size - 1)) || (n >= size && n % size)) { kh::set_error("%s: a domain of 2^%u rows over an SRS of %zu points is not supported", who, log2_n, size); return KH_E_INVALID; }
    while (((size_t)1 << vx->rounds) < size) vx->rounds++;
    const size_t nch = vx->nch = n < size ? 1 : n / size;
    vx->zk = zk_rows; vx->pub = public_inputs; vx->nprev = prev_challenges; vx->any_prev = any_prev;
    if (zk_rows <= (2 * (PERMUTS + 1) * nch - 2) / PERMUTS || zk_rows >= n) { kh::set_error("%s: NotZeroKnowledge: zk_rows %u for %zu chunks", who, zk_rows, nch); return KH_E_INVALID; }
    if (public_inputs >= n - zk_rows) { kh::set_error("%s: %u public inputs, the domain has %zu rows before the zero-knowledge rows", who, public_inputs, n - zk_rows); return KH_E_INVALID; }
    const khost::Fld F(vx->fid), B(khost::base_field_id(vx->curve));
    const int ngates = kh_gate_count();
    for (int g = 0; g < ngates; g++) {
        const char* nm = kh_gate_name(g);
        for (int k = 0; k < 5; k++) if (!strcmp(nm, LIB_GATES[k])) vx->lib_gate[k] = g;
        if (!strcmp(nm, "Generic")) vx->gid_generic = g;
    }
    int last_slot = -1;
    for (size_t j = 0; j < n_optional; j++) {
        const int g = optional_gates[j];
        int slot = -1;
        if (g >= 0 && g < ngates) for (int k = 0; k < 6; k++) if (!strcmp(kh_gate_name(g), OPTIONAL_GATE_NAMES[k])) slot = k;
        if (slot < 0 || slot <= last_slot) { kh::set_error("%s: optional gate %zu (id %d) is not an optional gate type in column order (RangeCheck0, RangeCheck1, ForeignFieldAdd, ForeignFieldMul, Xor16, Rot64)", who, j, g); return KH_E_INVALID; }
        vx->optional.push_back(g); vx->optional_slot.push_back(slot); last_slot = slot;
    }
    auto sec = [&](int s) -> kh_section_t { return (size_t)s < n_sections ? sections[s] : kh_section_t{nullptr, nullptr, 0}; };
    static const char* const SEC_NAMES[KH_VINDEX_LOOKUP_INFO + 1] = {"sigma_comm", "coefficients_comm", "generic_comm", "selector_comm", "optional_comm", "shifts", "digest",
                                                                     "lookup_table_comm", "lookup_table_ids_comm", "lookup_selector_comm", "lookup_runtime_selector_comm", "lookup_info"};
    auto points = [&](int s, size_t want) -> int {
        const kh_section_t in = sec(s);
        if (in.count != want) { kh::set_error("%s: %s has %zu points, %zu expected (%zu chunks per commitment)", who, SEC_NAMES[s], in.count, want, nch); return KH_E_INVALID; }
        for (size_t i = 0; i < in.count; i++)
            if (!(in.flags && in.flags[i]) && !on_curve(B, in.limbs + 8 * i)) { kh::set_error("%s: %s: point %zu is not on the curve", who, SEC_NAMES[s], i); return KH_E_INVALID; }
        vx->sec[s].set(in.limbs, in.flags, in.count);
        return KH_OK;
    };
    int rc;
    if ((rc = points(KH_VINDEX_SIGMA_COMM, PERMUTS * nch)) || (rc = points(KH_VINDEX_COEFFICIENTS_COMM, COLUMNS * nch)) || (rc = points(KH_VINDEX_GENERIC_COMM, nch)) ||
        (rc = points(KH_VINDEX_SELECTOR_COMM, 5 * nch)) || (rc = points(KH_VINDEX_OPTIONAL_COMM, n_optional * nch))) return rc;
    // ---- the lookup index (LookupVerifierIndex, verifier_index.rs:35-56)
    const kh_section_t info = sec(KH_VINDEX_LOOKUP_INFO);
    vx->lookup = sec(KH_VINDEX_LOOKUP_TABLE_COMM).count != 0;
    if (vx->lookup) {
        if (info.count != 2) { kh::set_error("%s: a lookup index needs lookup_info (2 records of 4 words)", who); return KH_E_INVALID; }
        const uint64_t* w = info.limbs;
        vx->mpr = (size_t)w[0]; vx->mjs = (size_t)w[1]; vx->joint_used = w[2] != 0; vx->has_rt = w[3] != 0; vx->width = (size_t)w[5];
        for (int q = 0; q < 4; q++) if (w[4] >> q & 1) vx->pats.push_back(q);
        if (vx->mpr < 1 || vx->mpr > 4 || vx->mjs < 1 || vx->mjs > 3 || vx->pats.empty() || (w[4] >> 4) || vx->width < 1 || vx->width > 128) {
            kh::set_error("%s: lookup_info: %zu lookups per row, joint size %zu, pattern mask %llu, %zu table columns", who, vx->mpr, vx->mjs, (unsigned long long)w[4], vx->width); return KH_E_INVALID;
        }
        const size_t nids = sec(KH_VINDEX_LOOKUP_TABLE_IDS_COMM).count;
        if (nids != 0 && nids != nch) { kh::set_error("%s: lookup_table_ids_comm has %zu points, 0 or %zu expected", who, nids, nch); return KH_E_INVALID; }
        vx->has_ids = nids != 0;
        if ((rc = points(KH_VINDEX_LOOKUP_TABLE_COMM, vx->width * nch)) || (rc = points(KH_VINDEX_LOOKUP_TABLE_IDS_COMM, nids)) ||
            (rc = points(KH_VINDEX_LOOKUP_SELECTOR_COMM, vx->pats.size() * nch)) || (rc = points(KH_VINDEX_LOOKUP_RUNTIME_SELECTOR_COMM, vx->has_rt ? nch : 0))) return rc;
    } else {
        for (int s = KH_VINDEX_LOOKUP_TABLE_IDS_COMM; s <= KH_VINDEX_LOOKUP_INFO; s++)
            if (sec(s).count) { kh::set_error("%s: %s without lookup_table_comm: lookup sections without a lookup index", who, SEC_NAMES[s]); return KH_E_INVALID; }
    }
    // ---- domain generator, endo coefficient, shifts, digest
    uint64_t w[4], eq[4], er[4];
    if ((rc = kh_domain_generator(vx->fid, log2_n, w))) return rc;
    vx->omega = load(w);
    if ((rc = kh_endos(1 - vx->curve, eq, er))) return rc;                 // VerifierIndex::endo = endos::<OtherCurve>().0
    vx->endo = load(eq);
    const kh_section_t sh = sec(KH_VINDEX_SHIFTS), dg = sec(KH_VINDEX_DIGEST);
    if (sh.count) {
        if (sh.count != 7) { kh::set_error("%s: shifts has %zu elements, 7 expected", who, sh.count); return KH_E_INVALID; }
        for (int i = 0; i < 7; i++) {
            if (!canonical(F, sh.limbs + 4 * i)) { kh::set_error("%s: shift %d is not a canonical field element (>= p)", who, i); return KH_E_INVALID; }
            vx->shifts[i] = load(sh.limbs + 4 * i);
        }
    } else if ((rc = kh_permutation_shifts(vx->fid, log2_n, vx->shifts[0].l))) return rc;
    if (dg.count) {
        if (dg.count != 1 || !canonical(B, dg.limbs)) { kh::set_error("%s: digest: one canonical base-field element expected", who); return KH_E_INVALID; }
        vx->digest = load(dg.limbs);
    } else {                                                             // verifier_index.rs:405-540
        SpongeH sp;
        if ((rc = kh_sponge_new(KH_SPONGE_FQ, vx->curve, &sp.s))) return rc;
        auto absorb = [&](int s, size_t first, size_t cnt) { return cnt ? kh_sponge_absorb_g(sp.s, vx->sec[s].xy.data() + 8 * first, vx->sec[s].inf.data() + first, cnt) : KH_OK; };
        if ((rc = absorb(KH_VINDEX_SIGMA_COMM, 0, PERMUTS * nch)) || (rc = absorb(KH_VINDEX_COEFFICIENTS_COMM, 0, COLUMNS * nch)) || (rc = absorb(KH_VINDEX_GENERIC_COMM, 0, nch)) ||
            (rc = absorb(KH_VINDEX_SELECTOR_COMM, 0, 5 * nch))) return rc;
        for (int k : OPTIONAL_DIGEST_ORDER)
            for (size_t j = 0; j < vx->optional.size(); j++) if (vx->optional_slot[j] == k && (rc = absorb(KH_VINDEX_OPTIONAL_COMM, j * nch, nch))) return rc;
        if (vx->lookup && ((rc = absorb(KH_VINDEX_LOOKUP_TABLE_COMM, 0, vx->width * nch)) || (rc = absorb(KH_VINDEX_LOOKUP_TABLE_IDS_COMM, 0, vx->has_ids ? nch : 0)) ||
                           (rc = absorb(KH_VINDEX_LOOKUP_RUNTIME_SELECTOR_COMM, 0, vx->has_rt ? nch : 0)) || (rc = absorb(KH_VINDEX_LOOKUP_SELECTOR_COMM, 0, vx->pats.size() * nch)))) return rc;
        if ((rc = kh_sponge_squeeze_field(sp.s, vx->digest.l))) return rc;
    }
    guard.p = nullptr;
    *out = vx;
    return KH_OK;
}

// one item of a batch while it is being verified
struct Item {
    const kh_verifier_index* vx = nullptr;
    const kh_verify_item_t* in = nullptr;
    kh_section_t sec[KH_PROOF_LOOKUP_RUNTIME_COMM + 1];
    size_t L0 = 0, ns = 0, nl = 0, nrt = 0, npat = 0, npoly = 0, prev_chunks = 0;
    std::vector<fe> pub_eval;                            // nch at zeta, nch at zeta omega
    SpongeH fq;                                          // the Fq-sponge as SRS::verify receives it
    Points pub_comm;
    fe beta, gamma, alpha, zeta, v, u, jc, zetaw, zeta1, zeta_srs, zetaw_srs, constant_term, ft0, cip;
    const fe* E() const { return (const fe*)sec[KH_PROOF_EVALS].limbs; }
    fe comb(const khost::Fld& F, size_t j, int p) const { return horner(F, E() + (2 * j + p) * vx->nch, vx->nch, p ? zetaw_srs : zeta_srs); }
};
#define KV_INVALID(...) do { kh::set_error(__VA_ARGS__); return KH_E_INVALID; } while (0)

// everything that can be wrong with an item, checked on the host before any device work (verifier.rs:781-830, check_proof_evals_len)
int validate_item(size_t i, Item& it) {
    const kh_verify_item_t& in = *it.in;
    if (!in.index || !in.proof) KV_INVALID("kh_batch_verify: item %zu: null index or proof", i);
    const kh_verifier_index& vx = *in.index;
    it.vx = &vx;
    const size_t nch = vx.nch;
    const khost::Fld F(vx.fid), B(khost::base_field_id(vx.curve));
    for (int s = 0; s <= KH_PROOF_LOOKUP_RUNTIME_COMM; s++) {
        kh_section_t& o = it.sec[s];
        if (kh_proof_section(in.proof, s, &o.limbs, &o.flags, &o.count)) return KH_E_INVALID;
    }
    static const char* const SEC_NAMES[KH_PROOF_LOOKUP_RUNTIME_COMM + 1] = {"w_comm", "z_comm", "t_comm", "public_comm", "evals", "public_evals", "ft_eval1", "lr", "delta", "z1_z2", "sg",
                                                                            "challenges", "lookup_sorted_comm", "lookup_aggreg_comm", "lookup_runtime_comm"};
    auto points = [&](int s, size_t want, const char* what) -> int {
        const kh_section_t& p = it.sec[s];
        if (p.count != want) KV_INVALID("kh_batch_verify: item %zu: %s has %zu points, %zu expected (%s)", i, SEC_NAMES[s], p.count, want, what);
        for (size_t j = 0; j < p.count; j++)
            if (!(p.flags && p.flags[j]) && !on_curve(B, p.limbs + 8 * j)) KV_INVALID("kh_batch_verify: item %zu: %s: point %zu is not on the curve", i, SEC_NAMES[s], j);
        return KH_OK;
    };
    auto elems = [&](int s, size_t want, const char* what) -> int {
        const kh_section_t& p = it.sec[s];
        if (p.count != want) KV_INVALID("kh_batch_verify: item %zu: %s has %zu elements, %zu expected (%s)", i, SEC_NAMES[s], p.count, want, what);
        for (size_t j = 0; j < p.count; j++)
            if (!canonical(F, p.limbs + 4 * j)) KV_INVALID("kh_batch_verify: item %zu: %s: element %zu is not a canonical field element (>= p)", i, SEC_NAMES[s], j);
        return KH_OK;
    };
    int rc;
    if ((rc = points(KH_PROOF_W_COMM, COLUMNS * nch, "15 commitments of num_chunks chunks")) || (rc = points(KH_PROOF_Z_COMM, nch, "num_chunks chunks")) ||
        (rc = points(KH_PROOF_T_COMM, 7 * nch, "7 num_chunks chunks")) || (rc = points(KH_PROOF_LR, 2 * vx.rounds, "an L and an R per round, log2(SRS size) rounds")) ||
        (rc = points(KH_PROOF_DELTA, 1, "one point")) || (rc = points(KH_PROOF_SG, 1, "one point"))) return rc;
    // the lookup sections follow the index (verifier.rs:179-230, 800-830)
    const bool proof_has_lookup = it.sec[KH_PROOF_LOOKUP_SORTED_COMM].count || it.sec[KH_PROOF_LOOKUP_AGGREG_COMM].count || it.sec[KH_PROOF_LOOKUP_RUNTIME_COMM].count;
    if (proof_has_lookup && !vx.lookup) KV_INVALID("kh_batch_verify: item %zu: the proof has lookup commitments, the index has no lookup index", i);
    if (vx.lookup && !it.sec[KH_PROOF_LOOKUP_SORTED_COMM].count) KV_INVALID("kh_batch_verify: item %zu: the index has a lookup index, the proof has no lookup commitments", i);
    it.ns = vx.lookup ? vx.mpr + 1 : 0; it.nl = vx.lookup ? it.ns + 2 : 0; it.nrt = vx.has_rt ? 2 : 0; it.npat = vx.pats.size();
    if ((rc = points(KH_PROOF_LOOKUP_SORTED_COMM, it.ns * nch, "max lookups per row + 1 commitments")) || (rc = points(KH_PROOF_LOOKUP_AGGREG_COMM, vx.lookup ? nch : 0, "num_chunks chunks")) ||
        (rc = points(KH_PROOF_LOOKUP_RUNTIME_COMM, vx.has_rt ? nch : 0, "num_chunks chunks iff the index has runtime tables"))) return rc;
    it.L0 = P_OPT + vx.optional.size();
    it.npoly = it.L0 + it.nl + it.nrt + it.npat;
    {
        const size_t got = it.sec[KH_PROOF_EVALS].count, per = 2 * nch;
        if (got != it.npoly * per) {
            const size_t base = (P_OPT + it.nl + it.nrt + it.npat) * per;
            if (got > it.npoly * per && got <= base + 6 * per && (got - base) % per == 0)
                KV_INVALID("kh_batch_verify: item %zu: evals has %zu optional-gate selector evaluations, the index has %zu optional-gate commitments", i, (got - base) / per, vx.optional.size());
            KV_INVALID("kh_batch_verify: item %zu: evals has %zu elements, %zu polynomials x 2 points x %zu chunks expected", i, got, it.npoly, nch);
        }
    }
    if ((rc = elems(KH_PROOF_EVALS, it.npoly * 2 * nch, "polynomials x 2 points x num_chunks")) || (rc = elems(KH_PROOF_FT_EVAL1, 1, "one element")) || (rc = elems(KH_PROOF_Z1_Z2, 2, "z1, z2"))) return rc;
    if (it.sec[KH_PROOF_PUBLIC_EVALS].count) { if ((rc = elems(KH_PROOF_PUBLIC_EVALS, 2 * nch, "num_chunks at zeta, num_chunks at zeta omega"))) return rc; }
    else if (nch != 1) KV_INVALID("kh_batch_verify: item %zu: public_evals are absent and the proof has %zu chunks (they can be computed for one chunk only)", i, nch);
    // public inputs, previous challenges
    if (in.n_public != vx.pub) KV_INVALID("kh_batch_verify: item %zu: %zu public inputs, the index has %zu", i, in.n_public, vx.pub);
    if (in.n_public && !in.public_inputs) KV_INVALID("kh_batch_verify: item %zu: null public inputs", i);
    for (size_t j = 0; j < in.n_public; j++) if (!canonical(F, in.public_inputs + 4 * j)) KV_INVALID("kh_batch_verify: item %zu: public input %zu is not a canonical field element (>= p)", i, j);
    if (!vx.any_prev && in.n_prev != vx.nprev) KV_INVALID("kh_batch_verify: item %zu: %zu previous challenges, the index has %zu", i, in.n_prev, vx.nprev);
    if (in.n_prev && (!in.prev_chals || !in.prev_rounds || !in.prev_comm_xy || !in.prev_comm_chunks)) KV_INVALID("kh_batch_verify: item %zu: null previous-challenge argument", i);
    size_t cpos = 0, ppos = 0;
    for (size_t j = 0; j < in.n_prev; j++) {
        const unsigned r = in.prev_rounds[j];
        const size_t ln = r <= 27 ? (size_t)1 << r : 0, want = ln <= vx.size ? 1 : 2;
        if ((ln != vx.size && ln != 2 * vx.size) || in.prev_comm_chunks[j] != want)
            KV_INVALID("kh_batch_verify: item %zu: previous challenge %zu: %u rounds / %zu commitment chunks do not fit an SRS of %zu", i, j, r, in.prev_comm_chunks[j], vx.size);
        for (unsigned c = 0; c < r; c++) if (!canonical(F, in.prev_chals + 4 * (cpos + c))) KV_INVALID("kh_batch_verify: item %zu: previous challenge %zu: element %u is not a canonical field element (>= p)", i, j, c);
        for (size_t c = 0; c < want; c++)
            if (!(in.prev_comm_inf && in.prev_comm_inf[ppos + c]) && !on_curve(B, in.prev_comm_xy + 8 * (ppos + c))) KV_INVALID("kh_batch_verify: item %zu: previous challenge %zu: commitment chunk %zu is not on the curve", i, j, c);
        cpos += r; ppos += want;
    }
    it.prev_chunks = ppos;
    return KH_OK;
}
}  // namespace

extern "C" {

#define KV(expr) do { int rc_ = (expr); if (rc_ != KH_OK) return rc_; } while (0)

int kh_verifier_index_new(kh_srs_t* srs, unsigned log2_n, unsigned zk_rows, unsigned public_inputs, unsigned prev_challenges, const int* optional_gates, size_t n_optional,
                          const kh_section_t* sections, size_t n_sections, kh_verifier_index_t** out) {
    return vindex_build("kh_verifier_index_new", srs, log2_n, zk_rows, public_inputs, prev_challenges, false, optional_gates, n_optional, sections, n_sections, out);
}
int kh_verifier_index_of(const kh_prover_index_t* index, kh_verifier_index_t** out) {
    if (out) *out = nullptr;
    if (!index || !out) { kh::set_error("kh_verifier_index_of: null argument"); return KH_E_INVALID; }
    kh_section_t secs[KH_VINDEX_LOOKUP_INFO + 1];
    for (int s = 0; s <= KH_VINDEX_LOOKUP_INFO; s++) KV(kh_verifier_index_section(index, s, &secs[s].limbs, &secs[s].flags, &secs[s].count));
    kh_srs_t* srs = nullptr; unsigned pub = 0, logn = 0, zk = 0; const int* opt = nullptr; size_t nopt = 0;
    kh::prover_index_facts(index, &srs, &pub, &opt, &nopt);
    KV(kh_prover_index_shape(index, &logn, &zk, nullptr));
    return vindex_build("kh_verifier_index_of", srs, logn, zk, pub, 0, true, opt, nopt, secs, KH_VINDEX_LOOKUP_INFO + 1, out);
}
int kh_verifier_index_digest(const kh_verifier_index_t* vix, uint64_t out[4]) {
    if (!vix || !out) { kh::set_error("kh_verifier_index_digest: null argument"); return KH_E_INVALID; }
    memcpy(out, vix->digest.l, 32);
    return KH_OK;
}
void kh_verifier_index_free(kh_verifier_index_t* vix) { delete vix; }
int kh_verify_last_phase_seconds(double* seconds, size_t cap) {
    if (!seconds) { kh::set_error("kh_verify_last_phase_seconds: null argument"); return KH_E_INVALID; }
    for (size_t i = 0; i < cap && i < 4; i++) seconds[i] = tl_phase[i];
    return 4;
}
int kh_verify(const kh_verify_item_t* item, int* ok, kh_verify_trace_t* trace) { return kh_batch_verify(item, item ? 1 : 0, nullptr, ok, trace); }

int kh_batch_verify(const kh_verify_item_t* items, size_t k, const uint64_t* rand, int* ok, kh_verify_trace_t* trace) {
    if (!items || !ok) { kh::set_error("kh_batch_verify: null argument"); return KH_E_INVALID; }
    if (k == 0) { kh::set_error("kh_batch_verify: an empty batch"); return KH_E_INVALID; }
    auto t_prev = std::chrono::steady_clock::now();
    double phase[4] = {0, 0, 0, 0};
    auto mark = [&](int p) { auto t = std::chrono::steady_clock::now(); phase[p] += std::chrono::duration<double>(t - t_prev).count(); t_prev = t; };
    // ---- phase 0: everything malformed is refused here, on the host
    std::vector<Item> its(k);
    for (size_t i = 0; i < k; i++) { its[i].in = &items[i]; KV(validate_item(i, its[i])); }
    kh_srs_t* srs = its[0].vx->srs;
    for (size_t i = 1; i < k; i++) if (its[i].vx->srs != srs) { kh::set_error("kh_batch_verify: item %zu is over another SRS handle than item 0 (one batch, one SRS)", i); return KH_E_INVALID; }
    const int curve = kh_srs_curve(srs), fid = khost::scalar_field_id(curve);
    const khost::Fld F(fid);
    const fe one = F.f.one, zero = {{0, 0, 0, 0}};
    const size_t size = its[0].vx->size, rounds = its[0].vx->rounds;
    fe rnd[2];
    if (rand) {
        for (int j = 0; j < 2; j++) {
            if (!canonical(F, rand + 4 * j)) { kh::set_error("kh_batch_verify: rand[%d] is not a canonical field element (>= p)", j); return KH_E_INVALID; }
            rnd[j] = load(rand + 4 * j);
            if (khost::is_zero(rnd[j])) { kh::set_error("kh_batch_verify: rand[%d] is zero", j); return KH_E_INVALID; }
        }
    } else do { KV(os_random(fid, 2, rnd)); } while (khost::is_zero(rnd[0]) || khost::is_zero(rnd[1]));
    // ---- the call's device and context
    struct DeviceRestore { int prev; ~DeviceRestore() { if (prev >= 0) (void)kh_set_device(prev); } } device_restore{kh_get_device()};
    KV(kh_set_device(kh_srs_device(srs)));
    struct PrivateContext { bool mine = false; ~PrivateContext() { if (mine) (void)kh_private_context_end(); } } private_context;
    if (!kh_private_context_active()) { KV(kh_private_context_begin()); private_context.mine = true; KV(kh_set_phase_timers(0)); }
    auto scalar_challenge = [&](kh_sponge_t* sp, fe& o) -> int {
        uint64_t ch[2];
        int rc = kh_sponge_challenge(sp, ch); if (rc) return rc;
        return kh_scalar_challenge_to_field(curve, ch, o.l);
    };
    uint64_t h_xy[8];
    KV(kh_srs_get_blinding_base(srs, h_xy));
    // ---- phase 1, per item: the public commitment and the transcript (oracle/kimchi.py::fiat_shamir)
    for (size_t i = 0; i < k; i++) {
        Item& it = its[i];
        const kh_verifier_index& vx = *it.vx;
        const kh_verify_item_t& in = *it.in;
        const size_t nch = vx.nch;
        // verifier.rs:834-858: the commitment to -sum_i pub_i L_i, masked with the blinder 1; an empty public input gives h per chunk
        if (in.n_public) {
            if (kh_srs_lagrange_chunks(srs, vx.logn) == 0) KV(kh_srs_compute_lagrange(srs, vx.logn));
            std::vector<fe> neg(in.n_public), ones(nch, one);
            for (size_t j = 0; j < in.n_public; j++) neg[j] = F.neg(load(in.public_inputs + 4 * j));
            std::vector<uint64_t> cxy(8 * nch); std::vector<uint8_t> cinf(nch);
            for (size_t c = 0; c < nch; c++) KV(kh_msm(srs, (int)vx.logn, (unsigned)c, 0, neg[0].l, in.n_public, 1, &cxy[8 * c], &cinf[c]));
            it.pub_comm.xy.resize(8 * nch); it.pub_comm.inf.resize(nch); it.pub_comm.count = nch;
            KV(kh_mask_custom(srs, cxy.data(), cinf.data(), nch, ones[0].l, nch, it.pub_comm.xy.data(), it.pub_comm.inf.data()));
        } else {
            it.pub_comm.xy.resize(8 * nch); it.pub_comm.inf.assign(nch, 0); it.pub_comm.count = nch;
            for (size_t c = 0; c < nch; c++) memcpy(&it.pub_comm.xy[8 * c], h_xy, 64);
        }
        kh_sponge_t*& fq = it.fq.s;
        KV(kh_sponge_new(KH_SPONGE_FQ, curve, &fq));
        KV(kh_sponge_absorb(fq, vx.digest.l, 1));
        if (it.prev_chunks) KV(kh_sponge_absorb_g(fq, in.prev_comm_xy, in.prev_comm_inf, it.prev_chunks));
        KV(kh_sponge_absorb_g(fq, it.pub_comm.xy.data(), it.pub_comm.inf.data(), nch));
        auto absorb_sec = [&](int s) { return kh_sponge_absorb_g(fq, it.sec[s].limbs, it.sec[s].flags, it.sec[s].count); };
        KV(absorb_sec(KH_PROOF_W_COMM));
        it.jc = zero;
        if (vx.lookup) {                                                 // verifier.rs:179-230
            if (vx.has_rt) KV(absorb_sec(KH_PROOF_LOOKUP_RUNTIME_COMM));
            uint64_t chal[2] = {0, 0};
            if (vx.joint_used) KV(kh_sponge_challenge(fq, chal));
            KV(kh_scalar_challenge_to_field(curve, chal, it.jc.l));
            KV(absorb_sec(KH_PROOF_LOOKUP_SORTED_COMM));
        }
        KV(kh_sponge_challenge_field(fq, it.beta.l)); KV(kh_sponge_challenge_field(fq, it.gamma.l));
        if (vx.lookup) KV(absorb_sec(KH_PROOF_LOOKUP_AGGREG_COMM));
        KV(absorb_sec(KH_PROOF_Z_COMM));
        KV(scalar_challenge(fq, it.alpha));
        KV(absorb_sec(KH_PROOF_T_COMM));
        KV(scalar_challenge(fq, it.zeta));
        it.zetaw = F.mul(it.zeta, vx.omega);
        it.zeta1 = fpow(F, it.zeta, vx.n); it.zeta_srs = fpow(F, it.zeta, size); it.zetaw_srs = fpow(F, it.zetaw, size);
        // the evaluations of the public polynomial: the proof's, or from the inputs (verifier.rs:336-386)
        it.pub_eval.assign(2 * nch, zero);
        if (it.sec[KH_PROOF_PUBLIC_EVALS].count) memcpy(it.pub_eval.data(), it.sec[KH_PROOF_PUBLIC_EVALS].limbs, 64 * nch);
        else if (in.n_public) {
            const fe ninv = F.inv(F.to_mont(fe{{(uint64_t)vx.n, 0, 0, 0}}));
            const fe pts[2] = {it.zeta, it.zetaw};
            for (int p = 0; p < 2; p++) {
                fe acc = zero, wi = one;
                for (size_t j = 0; j < in.n_public; j++) {
                    acc = F.sub(acc, F.mul(F.mul(load(in.public_inputs + 4 * j), wi), F.inv(F.sub(pts[p], wi))));
                    wi = F.mul(wi, vx.omega);
                }
                it.pub_eval[p] = F.mul(F.mul(acc, F.sub(fpow(F, pts[p], vx.n), one)), ninv);
            }
        }
        // the Fr-sponge: v, u (verifier.rs:300-420, plonk_sponge.rs:92-155)
        {
            SpongeH fqc, fr, pd;
            KV(kh_sponge_clone(fq, &fqc.s)); KV(kh_sponge_new(KH_SPONGE_FR, curve, &fr.s)); KV(kh_sponge_new(KH_SPONGE_FR, curve, &pd.s));
            fe d; KV(kh_sponge_digest(fqc.s, d.l)); KV(kh_sponge_absorb(fr.s, d.l, 1));
            size_t pos = 0;
            for (size_t j = 0; j < in.n_prev; j++) { KV(kh_sponge_absorb(pd.s, in.prev_chals + 4 * pos, in.prev_rounds[j])); pos += in.prev_rounds[j]; }
            KV(kh_sponge_digest(pd.s, d.l)); KV(kh_sponge_absorb(fr.s, d.l, 1));
            const fe* E = it.E();
            std::vector<fe> flat; flat.reserve(1 + 2 * nch * (it.npoly + 1));
            flat.push_back(load(it.sec[KH_PROOF_FT_EVAL1].limbs));
            flat.insert(flat.end(), it.pub_eval.begin(), it.pub_eval.end());
            flat.insert(flat.end(), E, E + 2 * nch * it.L0);
            if (vx.lookup) {                                             // aggregation, table, sorted ..., runtime table + selector, pattern selectors
                auto both = [&](size_t j) { flat.insert(flat.end(), E + 2 * nch * j, E + 2 * nch * (j + 1)); };
                both(it.L0 + it.ns); both(it.L0 + it.ns + 1);
                for (size_t s = 0; s < it.ns; s++) both(it.L0 + s);
                for (size_t s = 0; s < it.nrt + it.npat; s++) both(it.L0 + it.nl + s);
            }
            KV(kh_sponge_absorb(fr.s, (const uint64_t*)flat.data(), flat.size()));
            KV(scalar_challenge(fr.s, it.v)); KV(scalar_challenge(fr.s, it.u));
        }
    }
    mark(0);
    // ---- phase 2, the batch: the constant terms of the linearisation on the device.  One table of two-row columns (row 2i: item i at zeta, row 2i + 1: at zeta
    //      omega), one constants table per item and gate type, one launch per gate type present, the lookup program per item that has lookups, one download
    {
        std::vector<fe> cols(NCOLS * 2 * k, zero);
        auto put = [&](size_t col, size_t i, const fe& at_zeta, const fe& at_zetaw) { cols[col * 2 * k + 2 * i] = at_zeta; cols[col * 2 * k + 2 * i + 1] = at_zetaw; };
        bool lib_live[5] = {false, false, false, false, false}, opt_live[6] = {false, false, false, false, false, false};
        for (size_t i = 0; i < k; i++) {
            const Item& it = its[i];
            const kh_verifier_index& vx = *it.vx;
            auto both = [&](size_t col, size_t poly) { put(col, i, it.comb(F, poly, 0), it.comb(F, poly, 1)); };
            for (size_t c = 0; c < COLUMNS; c++) { both(c, P_W + c); both(COLUMNS + c, P_COEFF + c); }
            both(C_SEL_GENERIC, P_GENERIC);
            for (size_t g = 0; g < 5; g++) { both(C_SEL_LIB + g, P_LIB + g); lib_live[g] |= !khost::is_zero(it.comb(F, P_LIB + g, 0)); }
            for (size_t j = 0; j < vx.optional.size(); j++) { both(C_SEL_OPT + (size_t)vx.optional_slot[j], P_OPT + j); opt_live[vx.optional_slot[j]] = true; }
            if (vx.lookup) {
                for (size_t s = 0; s < it.ns; s++) both(C_SORTED + s, it.L0 + s);
                both(C_AGG, it.L0 + it.ns); both(C_TABLE, it.L0 + it.ns + 1);
                if (vx.has_rt) { both(C_RT, it.L0 + it.nl); both(C_RTSEL, it.L0 + it.nl + 1); }
                for (size_t q = 0; q < it.npat; q++) both(C_PATSEL + q, it.L0 + it.nl + it.nrt + q);
                // the row-set atoms at zeta (expr.rs:883-893): VanishesOnZeroKnowledgeAndPreviousRows, UnnormalizedLagrangeBasis(0), (-zk_rows - 1)
                const fe wf = fpow(F, vx.omega, vx.n - vx.zk - 1), zh = F.sub(it.zeta1, one);
                fe vanish = one, wj = wf;
                for (size_t j = 0; j <= vx.zk; j++) { vanish = F.mul(vanish, F.sub(it.zeta, wj)); wj = F.mul(wj, vx.omega); }
                const fe l0 = F.mul(zh, F.inv(F.sub(it.zeta, one))), lf = F.mul(zh, F.inv(F.sub(it.zeta, wf)));
                put(C_VANISH, i, vanish, vanish); put(C_L0, i, l0, l0); put(C_LFINAL, i, lf, lf);
            }
        }
        // the launches: Generic always, a library gate when some item's selector does not evaluate to zero, an optional gate when some item's index has it
        std::vector<int> gates; std::vector<size_t> selcol;
        gates.push_back(its[0].vx->gid_generic); selcol.push_back(C_SEL_GENERIC);
        for (size_t g = 0; g < 5; g++) if (lib_live[g]) { gates.push_back(its[0].vx->lib_gate[g]); selcol.push_back(C_SEL_LIB + g); }
        for (size_t o = 0; o < 6; o++) if (opt_live[o]) {
            int gid = -1;
            for (int g = 0; g < kh_gate_count(); g++) if (!strcmp(kh_gate_name(g), OPTIONAL_GATE_NAMES[o])) gid = g;
            gates.push_back(gid); selcol.push_back(C_SEL_OPT + o);
        }
        std::vector<std::vector<uint64_t>> tables(gates.size());
        std::vector<kh::GateBatchLaunch> launches(gates.size());
        for (size_t l = 0; l < gates.size(); l++) {
            const int nc = kh_gate_num_constants(gates[l]);
            if (nc <= 0) { kh::set_error("kh_batch_verify: gate id %d has no constants table", gates[l]); return KH_E_INVALID; }
            tables[l].resize((size_t)nc * 4 * k);
            for (size_t i = 0; i < k; i++) {
                const fe gp[2] = {one, its[i].alpha};
                if (l == 0) KV(kh_gate_constants(fid, gates[l], nullptr, nullptr, gp[0].l, 2, &tables[l][(size_t)nc * 4 * i]));
                else KV(kh_gate_constants(fid, gates[l], its[i].alpha.l, its[i].vx->endo.l, nullptr, 0, &tables[l][(size_t)nc * 4 * i]));
            }
            launches[l] = kh::GateBatchLaunch{gates[l], (int)selcol[l], tables[l].data()};
        }
        Dev out; KV(out.alloc(k));
        const uint64_t* cols_dev = nullptr;
        KV(kh::verifier_gate_terms_dev(fid, (const uint64_t*)cols.data(), NCOLS, k, launches.data(), launches.size(), out.p, &cols_dev));
        for (size_t i = 0; i < k; i++) {                                 // lookup_constant_term: the prover's constraint program on this item's two rows
            const Item& it = its[i];
            const kh_verifier_index& vx = *it.vx;
            if (!vx.lookup) continue;
            LookupChallenges ch{};
            ch.jc = it.jc; ch.tic = fpow(F, it.jc, vx.mjs); ch.beta = it.beta; ch.gamma = it.gamma; ch.gb1 = F.mul(it.gamma, F.add(one, it.beta));
            const fe b1m = fpow(F, F.add(one, it.beta), vx.mpr);
            fe gp = one;
            for (size_t j = 0; j <= vx.mpr; j++) { ch.prefactor[j] = F.mul(gp, b1m); gp = F.mul(gp, it.gamma); }
            Prog p;
            const LookupColumns lc{(uint32_t)C_SORTED, (uint32_t)C_AGG, (uint32_t)C_TABLE, (uint32_t)C_PATSEL, (uint32_t)C_VANISH, (uint32_t)C_L0, (uint32_t)C_LFINAL, (uint32_t)C_RT, (uint32_t)C_RTSEL};
            emit_lookup_constraints(p, F, vx.pats, vx.mpr, ch, it.alpha, lc, vx.has_rt);
            std::vector<const uint64_t*> cp(NCOLS); std::vector<size_t> lens(NCOLS, 2);
            for (size_t c = 0; c < NCOLS; c++) cp[c] = cols_dev + 4 * (c * 2 * k + 2 * i);
            KV(p.run(fid, cp, lens, 1, 1, 1, 1, out.at(i)));
        }
        std::vector<fe> ct(k);
        KV(kh_dev_download(ct.data(), out.p, 32 * k));
        for (size_t i = 0; i < k; i++) its[i].constant_term = ct[i];
    }
    mark(1);
    // ---- phase 3, per item: ft_eval0, the evaluation list with its combined inner product, the terms of SRS::verify (oracle/pasta.py::ipa_verify_terms)
    std::vector<uint64_t> pts; std::vector<uint8_t> pinf; std::vector<fe> sc;       // H first
    std::vector<fe> g_chals(k * rounds), g_weights(k);
    auto term = [&](const uint64_t* xy, uint8_t inf, const fe& s) { pts.insert(pts.end(), xy, xy + 8); pinf.push_back(inf); sc.push_back(s); };
    term(h_xy, 0, zero);
    fe rb_i = one, sg_i = one;
    uint64_t eq[4], er[4];
    KV(kh_endos(curve, eq, er));
    for (size_t i = 0; i < k; i++) {
        Item& it = its[i];
        const kh_verifier_index& vx = *it.vx;
        const kh_verify_item_t& in = *it.in;
        const size_t nch = vx.nch;
        const fe* E = it.E();
        const fe zeta = it.zeta, beta = it.beta, gamma = it.gamma;
        fe alphas[3]; alphas[0] = fpow(F, it.alpha, ALPHA_PERM0); alphas[1] = F.mul(alphas[0], it.alpha); alphas[2] = F.mul(alphas[1], it.alpha);
        const fe w_zk = fpow(F, vx.omega, vx.n - vx.zk);
        const fe zkp = F.mul(F.mul(F.sub(zeta, w_zk), F.sub(zeta, F.mul(w_zk, vx.omega))), F.sub(zeta, fpow(F, vx.omega, vx.n - 1)));
        const fe z0 = it.comb(F, P_Z, 0), z1e = it.comb(F, P_Z, 1);
        fe w0[COLUMNS]; for (size_t c = 0; c < COLUMNS; c++) w0[c] = it.comb(F, P_W + c, 0);
        // ---- ft_eval0 (verifier.rs:412-490)
        fe ft0 = F.mul(F.mul(F.mul(F.add(w0[PERMUTS - 1], gamma), z1e), alphas[0]), zkp);
        fe perm = F.mul(F.mul(F.mul(z1e, beta), alphas[0]), zkp);       // perm_scalars (permutation.rs:340-370)
        for (size_t c = 0; c + 1 < PERMUTS; c++) {
            const fe f = F.add(F.add(F.mul(beta, it.comb(F, P_SIGMA + c, 0)), w0[c]), gamma);
            ft0 = F.mul(ft0, f); perm = F.mul(perm, f);
        }
        perm = F.neg(perm);
        ft0 = F.sub(ft0, horner(F, it.pub_eval.data(), nch, it.zeta_srs));
        fe t = F.mul(F.mul(alphas[0], zkp), z0);
        for (size_t c = 0; c < PERMUTS; c++) t = F.mul(t, F.add(F.add(gamma, F.mul(F.mul(beta, zeta), vx.shifts[c])), w0[c]));
        ft0 = F.sub(ft0, t);
        const fe zeta1m1 = F.sub(it.zeta1, one);
        const fe num = F.mul(F.add(F.mul(F.mul(zeta1m1, alphas[1]), F.sub(zeta, w_zk)), F.mul(F.mul(zeta1m1, alphas[2]), F.sub(zeta, one))), F.sub(one, z0));
        const fe den = F.mul(F.sub(zeta, w_zk), F.sub(zeta, one));
        ft0 = F.add(ft0, F.mul(num, F.inv(den)));
        ft0 = F.sub(ft0, it.constant_term);
        it.ft0 = ft0;
        const fe ft1 = load(it.sec[KH_PROOF_FT_EVAL1].limbs);
        // ---- the sponge of SRS::verify needs the combined inner product first: the evaluation list in opening order (verifier.rs:834-1175), chunk by chunk.
        //      Each chunk's commitment goes into the MSM with rc * polyscale^t; those scalars need c, which the sponge gives after cip: two passes over one list
        struct Chunk { const uint64_t* xy; uint8_t inf; fe e0, e1, mult; };                      // a point whose scalar is rc * ps * mult
        std::vector<Chunk> list;                                         // advance[e] = 0: the next entry shares this one's ps (the points of ft_comm, of a combined-table chunk);
        std::vector<uint8_t> advance;                                    // the last entry of such a group carries its evaluation pair
        auto chunk = [&](const uint64_t* xy, uint8_t inf, const fe& e0, const fe& e1, const fe& mult, bool adv) { list.push_back(Chunk{xy, inf, e0, e1, mult}); advance.push_back(adv ? 1 : 0); };
        // previous challenges: b_poly at both points, in one chunk or two (RecursionChallenge::evals, proof.rs:455-494)
        {
            size_t cpos = 0, ppos = 0;
            const fe ptsz[2] = {zeta, it.zetaw}, pws[2] = {it.zeta_srs, it.zetaw_srs};
            for (size_t j = 0; j < in.n_prev; j++) {
                const unsigned r = in.prev_rounds[j];
                const size_t ln = (size_t)1 << r;
                fe full[2], diff[2] = {zero, zero};
                for (int p = 0; p < 2; p++) {
                    std::vector<fe> pw(r ? r : 1); pw[0] = ptsz[p];
                    for (unsigned q = 1; q < r; q++) pw[q] = F.sqr(pw[q - 1]);
                    fe acc = one;
                    for (unsigned q = 0; q < r; q++) acc = F.mul(acc, F.add(one, F.mul(load(in.prev_chals + 4 * (cpos + q)), pw[r - 1 - q])));
                    full[p] = acc;
                }
                auto pinf_at = [&](size_t c) -> uint8_t { return in.prev_comm_inf ? in.prev_comm_inf[ppos + c] : 0; };
                if (ln <= size) chunk(in.prev_comm_xy + 8 * ppos, pinf_at(0), full[0], full[1], one, true);
                else {
                    std::vector<fe> bc(ln);
                    KV(kh_b_poly_coefficients(fid, in.prev_chals + 4 * cpos, r, 1, (uint64_t*)bc.data()));
                    for (int p = 0; p < 2; p++) diff[p] = horner(F, bc.data() + size, ln - size, ptsz[p]);
                    chunk(in.prev_comm_xy + 8 * ppos, pinf_at(0), F.sub(full[0], F.mul(diff[0], pws[0])), F.sub(full[1], F.mul(diff[1], pws[1])), one, true);
                    chunk(in.prev_comm_xy + 8 * (ppos + 1), pinf_at(1), diff[0], diff[1], one, true);
                }
                cpos += r; ppos += in.prev_comm_chunks[j];
            }
        }
        for (size_t c = 0; c < nch; c++) chunk(&it.pub_comm.xy[8 * c], it.pub_comm.inf[c], it.pub_eval[c], it.pub_eval[nch + c], one, true);
        // ft_comm = perm_scalar * chunk_commitment(sigma_6) - (zeta^n - 1) chunk_commitment(t) (commitment.rs:188-205), multiplied out: one ps for all its points
        {
            const Points& sg = vx.sec[KH_VINDEX_SIGMA_COMM];
            const kh_section_t& tc = it.sec[KH_PROOF_T_COMM];
            fe pw = one;
            for (size_t c = 0; c < nch; c++) { chunk(&sg.xy[8 * ((PERMUTS - 1) * nch + c)], sg.inf[(PERMUTS - 1) * nch + c], zero, zero, F.mul(perm, pw), false); pw = F.mul(pw, it.zeta_srs); }
            pw = one;
            const fe m1 = F.neg(zeta1m1);
            for (size_t c = 0; c < tc.count; c++) { chunk(tc.limbs + 8 * c, tc.flags ? tc.flags[c] : 0, zero, zero, F.mul(m1, pw), false); pw = F.mul(pw, it.zeta_srs); }
            list.back().e0 = ft0; list.back().e1 = ft1; advance.back() = 1;            // the one evaluation pair of ft closes the group
        }
        auto poly_sec = [&](const uint64_t* xy, const uint8_t* inf, size_t first, size_t j) {     // polynomial j of KH_PROOF_EVALS against nch points from `first`
            for (size_t c = 0; c < nch; c++) chunk(xy + 8 * (first + c), inf ? inf[first + c] : 0, E[(2 * j) * nch + c], E[(2 * j + 1) * nch + c], one, true);
        };
        auto vsec = [&](int s, size_t first, size_t j) { poly_sec(vx.sec[s].xy.data(), vx.sec[s].inf.data(), first, j); };
        auto psec = [&](int s, size_t first, size_t j) { poly_sec(it.sec[s].limbs, it.sec[s].flags, first, j); };
        psec(KH_PROOF_Z_COMM, 0, P_Z);
        vsec(KH_VINDEX_GENERIC_COMM, 0, P_GENERIC);
        for (size_t g = 0; g < 5; g++) vsec(KH_VINDEX_SELECTOR_COMM, g * nch, P_LIB + g);
        for (size_t c = 0; c < COLUMNS; c++) psec(KH_PROOF_W_COMM, c * nch, P_W + c);
        for (size_t c = 0; c < COLUMNS; c++) vsec(KH_VINDEX_COEFFICIENTS_COMM, c * nch, P_COEFF + c);
        for (size_t c = 0; c + 1 < PERMUTS; c++) vsec(KH_VINDEX_SIGMA_COMM, c * nch, P_SIGMA + c);
        for (size_t j = 0; j < vx.optional.size(); j++) vsec(KH_VINDEX_OPTIONAL_COMM, j * nch, P_OPT + j);
        if (vx.lookup) {                                                 // verifier.rs:1034-1175: sorted ..., aggregation, the combined table, runtime, the pattern selectors
            for (size_t s = 0; s < it.ns; s++) psec(KH_PROOF_LOOKUP_SORTED_COMM, s * nch, it.L0 + s);
            psec(KH_PROOF_LOOKUP_AGGREG_COMM, 0, it.L0 + it.ns);
            const size_t jt = it.L0 + it.ns + 1;
            const Points& tb = vx.sec[KH_VINDEX_LOOKUP_TABLE_COMM]; const Points& ids = vx.sec[KH_VINDEX_LOOKUP_TABLE_IDS_COMM];
            const kh_section_t& rt = it.sec[KH_PROOF_LOOKUP_RUNTIME_COMM];
            const fe tic = fpow(F, it.jc, vx.mjs);
            for (size_t c = 0; c < nch; c++) {                           // combine_table (lookup/tables/mod.rs:164-199), chunk c: sum_i jc^i column_i + jc^max_joint_size ids + jc runtime
                fe pw = one;
                for (size_t col = 0; col < vx.width; col++) { chunk(&tb.xy[8 * (col * nch + c)], tb.inf[col * nch + c], zero, zero, pw, false); pw = F.mul(pw, it.jc); }
                if (vx.has_ids) chunk(&ids.xy[8 * c], ids.inf[c], zero, zero, tic, false);
                if (vx.has_rt) chunk(rt.limbs + 8 * c, rt.flags ? rt.flags[c] : 0, zero, zero, it.jc, false);
                list.back().e0 = E[(2 * jt) * nch + c]; list.back().e1 = E[(2 * jt + 1) * nch + c]; advance.back() = 1;
            }
            if (vx.has_rt) { psec(KH_PROOF_LOOKUP_RUNTIME_COMM, 0, it.L0 + it.nl); vsec(KH_VINDEX_LOOKUP_RUNTIME_SELECTOR_COMM, 0, it.L0 + it.nl + 1); }
            for (size_t q = 0; q < it.npat; q++) vsec(KH_VINDEX_LOOKUP_SELECTOR_COMM, q * nch, it.L0 + it.nl + it.nrt + q);
        }
        // combined_inner_product (commitment.rs:622-657): sum_t polyscale^t (e_t(zeta) + evalscale e_t(zeta omega)) over the chunks of the list
        fe cip = zero, ps = one;
        for (size_t e = 0; e < list.size(); e++) if (advance[e]) { cip = F.add(cip, F.mul(ps, F.add(list[e].e0, F.mul(it.u, list[e].e1)))); ps = F.mul(ps, it.v); }
        it.cip = cip;
        // ---- SRS::verify's sponge and scalars (ipa.rs:340-470)
        kh_sponge_t* fq = it.fq.s;
        {
            const khost::Fld BF(khost::base_field_id(curve));
            fe acc = one;
            for (int b = 0; b < 255; b++) acc = F.add(acc, acc);          // 2^255 = 2^(modulus bits): shift_scalar (commitment.rs:273-288)
            const fe sh = !khost::geq(F.f.p, BF.f.p) ? F.mul(F.sub(cip, F.add(acc, one)), F.inv(F.add(one, one))) : F.sub(cip, acc);
            KV(kh_sponge_absorb_fr(fq, sh.l, 1));
        }
        uint64_t tq[4], u_base[8];
        KV(kh_sponge_squeeze_field(fq, tq));
        KV(kh_group_map_to_group(curve, tq, u_base));
        const kh_section_t& lr = it.sec[KH_PROOF_LR];
        std::vector<fe> chal(rounds), chal_inv(rounds);
        for (size_t r = 0; r < rounds; r++) {
            KV(kh_sponge_absorb_g(fq, lr.limbs + 16 * r, lr.flags ? lr.flags + 2 * r : nullptr, 2));
            KV(scalar_challenge(fq, chal[r]));
            chal_inv[r] = F.inv(chal[r]);
            g_chals[i * rounds + r] = chal[r];
        }
        const kh_section_t& dl = it.sec[KH_PROOF_DELTA]; const kh_section_t& sgp = it.sec[KH_PROOF_SG];
        KV(kh_sponge_absorb_g(fq, dl.limbs, dl.flags, 1));
        fe c; KV(scalar_challenge(fq, c));
        const fe z1 = load(it.sec[KH_PROOF_Z1_Z2].limbs), z2 = load(it.sec[KH_PROOF_Z1_Z2].limbs + 4);
        fe b0 = zero, scale = one;
        const fe ptsz[2] = {zeta, it.zetaw};
        for (int p = 0; p < 2; p++) {                                    // b_poly(chal, e) (commitment.rs:426-436)
            std::vector<fe> pw(rounds); pw[0] = ptsz[p];
            for (size_t q = 1; q < rounds; q++) pw[q] = F.sqr(pw[q - 1]);
            fe acc = one;
            for (size_t q = 0; q < rounds; q++) acc = F.mul(acc, F.add(one, F.mul(chal[q], pw[rounds - 1 - q])));
            b0 = F.add(b0, F.mul(scale, acc)); scale = F.mul(scale, it.u);
        }
        term(sgp.limbs, sgp.flags ? sgp.flags[0] : 0, F.sub(F.neg(F.mul(rb_i, z1)), sg_i));
        g_weights[i] = sg_i;
        sc[0] = F.sub(sc[0], F.mul(rb_i, z2));
        term(u_base, 0, F.neg(F.mul(rb_i, F.mul(z1, b0))));
        const fe rc = F.mul(c, rb_i);
        for (size_t r = 0; r < rounds; r++) {
            term(lr.limbs + 16 * r, lr.flags ? lr.flags[2 * r] : 0, F.mul(rc, chal_inv[r]));
            term(lr.limbs + 16 * r + 8, lr.flags ? lr.flags[2 * r + 1] : 0, F.mul(rc, chal[r]));
        }
        ps = one;                                                        // combine_commitments (commitment.rs:724-744)
        for (size_t e = 0; e < list.size(); e++) {
            term(list[e].xy, list[e].inf, F.mul(F.mul(rc, ps), list[e].mult));
            if (advance[e]) ps = F.mul(ps, it.v);
        }
        term(u_base, 0, F.mul(rc, cip));
        term(dl.limbs, dl.flags ? dl.flags[0] : 0, rb_i);
        rb_i = F.mul(rb_i, rnd[0]); sg_i = F.mul(sg_i, rnd[1]);
    }
    mark(2);
    // ---- phase 4: the one MSM of the batch (ipa.rs:474-502)
    int is_zero = 0;
    KV(kh_ipa_verify_msm(srs, (const uint64_t*)g_chals.data(), k * rounds, (const uint64_t*)g_weights.data(), k, pts.data(), pinf.data(), (const uint64_t*)sc.data(), sc.size(), &is_zero));
    KV(kh_sync());
    mark(3);
    memcpy(tl_phase, phase, sizeof(phase));
    if (trace)
        for (size_t i = 0; i < k; i++) {
            const Item& it = its[i];
            const fe ch[7] = {it.beta, it.gamma, it.alpha, it.zeta, it.v, it.u, it.vx->lookup ? it.jc : zero};
            memcpy(trace[i].challenges, ch, sizeof(ch));
            memcpy(trace[i].constant_term, it.constant_term.l, 32); memcpy(trace[i].ft_eval0, it.ft0.l, 32); memcpy(trace[i].combined_inner_product, it.cip.l, 32);
        }
    *ok = is_zero ? 1 : 0;
    return KH_OK;
}

}  // extern "C"
