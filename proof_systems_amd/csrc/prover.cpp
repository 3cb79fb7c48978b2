// prover.cpp -- ProverProof::create (kimchi/src/prover.rs:187-1515) as a native host loop over this library's own C ABI.
//
// The same protocol proof_systems_amd/prover.py runs from Python, for everything create_recursive takes (previous challenges, lookups, runtime tables), written against the public
// entry points only (kh_ntt_dev, kh_gate_evaluations_dev, kh_msm_submit, kh_ipa_open, kh_sponge_*, ...): a Rust or C caller gets a whole proof
// with one call, no interpreter in the measured latency, and several prover threads do not share a GIL.  Every device step is the entry
// point the Python prover calls at the same place, with the same arguments, so the two give the same proof for the same randomness
// (tests/test_gpu_native_prover.py compares them field element for field element; the Python prover is pinned on the reference's whole-proof
// vector through the oracle prover).  Host arithmetic: khost::Fld on Montgomery limbs (the wire form).
//
//   round 1  prover.rs:254-327   zero-knowledge rows, public polynomial, 15 witness commitments (one batched MSM over the Lagrange basis)
//   round 2  prover.rs:676-707   beta, gamma; permutation aggregation z (permutation.rs:510-568), commitment
//   round 3  prover.rs:709-985   alpha; generic + permutation + gate constraints on d8, division by Z_H, boundary quotients, t commitment
//   round 4  prover.rs:987-1263  zeta; chunked evaluations, ft (Maller), Fr-sponge -> v, u
//   round 5  prover.rs:1265-1500 SRS::open over (public, ft, z, selectors, w, coefficients, sigma, optional selectors)
#include <stdint.h>
#include <string.h>
#include <chrono>
#include <new>
#include <vector>

#include "../../include/kimchi_hip.h"
#include "env.hpp"
#include "host_ec.hpp"
#include "protocol_host.hpp"
#include "wire_handles.hpp"
#include "witness_lookup.hpp"

namespace kh {
int index_columns_dev(int field, const uint8_t* selcol_dev, const uint32_t* wires_dev, const uint64_t* coeffs_dev, size_t n_gates, size_t n,
                      size_t zk_rows, const uint64_t* shifts, size_t ncol, uint64_t* d1_dev);     // vector_api.cpp / poly.hip: the column pass of kh_prover_index_create
// vector_api.cpp / lookup_index.hip: the lookup passes of kh_prover_index_create_lookup
int lookup_selectors_dev(int field, const uint8_t* code_dev, size_t n_gates, size_t n, const int* patterns, size_t npat, uint64_t* out_dev);
int lookup_tables_dev(int field, const uint64_t* segs_dev, const uint64_t* seg_starts, size_t nseg, const uint64_t* data_dev, size_t n, size_t width, uint64_t* tcols_dev,
                      uint64_t* ids_dev, uint64_t* rtsel_dev, size_t rt_offset, size_t rt_len, size_t zk_rows);
int lookup_atom_denominators_dev(int field, const uint64_t* x8_dev, size_t n, size_t zk_rows, const uint64_t a[4], const uint64_t omega[4], uint64_t* atoms_dev);
int lookup_atom_finish_dev(int field, size_t n, size_t zk_rows, const uint64_t zh8[32], const uint64_t lim0[4], const uint64_t limf[4], uint64_t* atoms_dev);
// vector_api.cpp / witness_check.hip: the kernels of kh_witness_check(_full) and the read-back of their status words
int witness_check_dev(int field, const uint64_t* witness_dev, const uint64_t* d1_dev, size_t n, const int* sel_col, size_t ngate_ids, size_t public_inputs,
                      const uint64_t endo[4], const uint32_t* wires_dev, size_t n_gates, const WitnessLookups* lk, uint64_t status[4]);
int witness_check_num_constraints(int gate);         // of a gate id the check evaluates, else 0
}

namespace {
using namespace kh_protocol;
constexpr size_t SEL0 = COLUMNS + 2 + PERMUTS, OPT0 = SEL0 + 5;
const char* const LIB_GATES[5] = {"Poseidon", "CompleteAdd", "VarBaseMul", "EndoMul", "EndoMulScalar"};

}  // namespace

struct kh_lookup_index {
    std::vector<int> pats;                           // pattern ids present, in the reference's order
    std::vector<const uint64_t*> sel1, selc, sel8, tcols;
    const uint64_t* tids = nullptr;
    const uint64_t* atoms8[3] = {nullptr, nullptr, nullptr};
    size_t mpr = 0, mjs = 0;
    // runtime tables (lookup/runtime_tables.rs): the rows of the combined table whose second column arrives with each proof
    const uint64_t *rtsel1 = nullptr, *rtselc = nullptr, *rtsel8 = nullptr;
    size_t rt_offset = 0, rt_len = 0;
    // kh_prover_index_create_lookup: where each table sits in the combined table (kh_prover_index_lookup_table); empty for an attached lookup index
    struct TableAt { int id; size_t first_row, len; bool runtime; size_t runtime_first; };
    std::vector<TableAt> tables;
};

struct kh_prover_index {
    kh_srs_t* srs = nullptr;
    int curve = 0, fid = 0;
    unsigned logn = 0, live = 0;
    size_t n = 0, size = 0, nch = 1, zk = 3, pub = 0, ncol = 0;
    const uint64_t *d1 = nullptr, *dc = nullptr, *d8 = nullptr;
    std::vector<int> optional;                       // kh gate ids of the optional selector columns
    int lib_gate[5] = {0, 0, 0, 0, 0}, gid_generic = -1, gid_perm = -1;
    fe shifts[7], digest, omega, endo;
    uint64_t* zero_poly = nullptr;                   // n zeros on the device: the public polynomial of a circuit without public inputs
    std::vector<uint64_t> zsel_xy; std::vector<uint8_t> zsel_inf;   // commitment to the zero polynomial masked with 1 (= h per chunk)
    kh_lookup_index* lk = nullptr;                   // kh_prover_index_attach_lookup, or built by kh_prover_index_create_lookup
    // kh_prover_index_create(_lookup): the index owns its columns and carries its verifier index (kh_verifier_index_section) and build phases
    bool created = false;
    uint64_t *own_d1 = nullptr, *own_dc = nullptr, *own_d8 = nullptr;
    uint64_t *own_l1 = nullptr, *own_lc = nullptr, *own_l8 = nullptr;      // the lookup columns: d1, coefficient forms of the selectors, their d8 + the atoms
    uint32_t* own_wires = nullptr; size_t n_gates = 0;                    // the gate list's wires, 7 (row, column) pairs per recorded row: kh_witness_check's copy constraints
    struct VSec { std::vector<uint64_t> limbs; std::vector<uint8_t> flags; size_t count = 0; };
    VSec vsec[KH_VINDEX_LOOKUP_INFO + 1];
    double phase[4] = {0, 0, 0, 0};
    const uint64_t* col1(size_t k) const { return d1 + 4 * k * n; }
    const uint64_t* colc(size_t k) const { return dc + 4 * k * n; }
    const uint64_t* col8(size_t k) const { return d8 + 4 * k * 8 * n; }
};

struct kh_proof {
    struct Sec { std::vector<uint64_t> limbs; std::vector<uint8_t> flags; size_t count = 0; bool points = false; };
    Sec sec[15];
    double phase[6] = {0, 0, 0, 0, 0, 0};
    // for kh_proof_to_msgpack: which Options the serialised proof has (known to kh_prove* and kh_proofs_from_msgpack) and the previous challenges it was made
    // with or read with.  Nothing of the proving or verifying path reads them.
    kh_proof_wire::Shape shape;
    kh::ProofPrev prev;
    void set_points(int s, const uint64_t* xy, const uint8_t* inf, size_t cnt) {
        sec[s].limbs.assign(xy, xy + 8 * cnt); sec[s].flags.assign(inf, inf + cnt); sec[s].count = cnt; sec[s].points = true;
    }
    void set_elems(int s, const fe* v, size_t cnt) {
        sec[s].limbs.resize(4 * cnt); if (cnt) memcpy(sec[s].limbs.data(), v, 32 * cnt); sec[s].flags.clear(); sec[s].count = cnt; sec[s].points = false;
    }
};

namespace kh {
const kh_proof_wire::Shape& proof_shape(const kh_proof_t* proof) { return proof->shape; }
void proof_set_shape(kh_proof_t* proof, const kh_proof_wire::Shape& shape) { proof->shape = shape; }
const ProofPrev& proof_prev(const kh_proof_t* proof) { return proof->prev; }
void proof_set_prev(kh_proof_t* proof, ProofPrev&& prev) { proof->prev = std::move(prev); }
}  // namespace kh

extern "C" {

#define KP(expr)                                   \
    do {                                           \
        int rc_ = (expr);                          \
        if (rc_ != KH_OK) { (void)kh_sync(); return rc_; }   \
    } while (0)
#define KP_REQUIRE(cond, ...)                                        \
    do {                                                             \
        if (!(cond)) { kh::set_error(__VA_ARGS__); (void)kh_sync(); return KH_E_INVALID; } \
    } while (0)

int kh_prover_index_new(kh_srs_t* srs, unsigned log2_n, unsigned zk_rows, unsigned public_inputs, const uint64_t* d1_dev, const uint64_t* dc_dev,
                        const uint64_t* d8_dev, const int* optional_gates, size_t n_optional, unsigned live_mask, const uint64_t* shifts,
                        const uint64_t digest[4], kh_prover_index_t** out) {
    if (!srs || !d1_dev || !dc_dev || !d8_dev || !shifts || !digest || !out || (n_optional && !optional_gates) || log2_n > 26) {
        kh::set_error("kh_prover_index_new: bad argument"); return KH_E_INVALID;
    }
    kh_prover_index* ix = new (std::nothrow) kh_prover_index();
    if (!ix) { kh::set_error("out of memory"); return KH_E_NOMEM; }
    ix->srs = srs; ix->curve = kh_srs_curve(srs); ix->fid = ix->curve == KH_CURVE_VESTA ? KH_FIELD_FP : KH_FIELD_FQ;
    ix->logn = log2_n; ix->n = (size_t)1 << log2_n; ix->size = kh_srs_size(srs);
    ix->nch = ix->n < ix->size ? 1 : ix->n / ix->size;
    ix->zk = zk_rows; ix->pub = public_inputs; ix->live = live_mask;
    ix->d1 = d1_dev; ix->dc = dc_dev; ix->d8 = d8_dev;
    ix->optional.assign(optional_gates, optional_gates + n_optional);
    ix->ncol = OPT0 + n_optional;
    int rc = KH_OK;
    auto fail = [&](int code) { kh_prover_index_free(ix); return code; };
    if (zk_rows <= (2 * (PERMUTS + 1) * ix->nch - 2) / PERMUTS || zk_rows >= ix->n) { kh::set_error("NotZeroKnowledge: zk_rows %u for %zu chunks", zk_rows, ix->nch); return fail(KH_E_INVALID); }
    if (kh_srs_lagrange_chunks(srs, log2_n) == 0) { kh::set_error("the Lagrange basis of 2^%u is not registered on this SRS (kh_srs_compute_lagrange)", log2_n); return fail(KH_E_NOTFOUND); }
    const int ngates = kh_gate_count();
    for (int g = 0; g < ngates; g++) {
        const char* nm = kh_gate_name(g);
        for (int k = 0; k < 5; k++) if (!strcmp(nm, LIB_GATES[k])) ix->lib_gate[k] = g;
        if (!strcmp(nm, "Generic")) ix->gid_generic = g;
        if (!strcmp(nm, "Permutation")) ix->gid_perm = g;
    }
    for (int g : ix->optional) if (g < 0 || g >= ngates) { kh::set_error("unknown optional gate id %d", g); return fail(KH_E_INVALID); }
    for (int i = 0; i < 7; i++) ix->shifts[i] = load(shifts + 4 * i);
    ix->digest = load(digest);
    uint64_t w[4], eq[4], er[4];
    if ((rc = kh_domain_generator(ix->fid, log2_n, w))) return fail(rc);
    ix->omega = load(w);
    if ((rc = kh_endos(1 - ix->curve, eq, er))) return fail(rc);          // VerifierIndex::endo = endos::<OtherCurve>().0: an element of this scalar field
    ix->endo = load(eq);
    if ((rc = kh_dev_alloc((void**)&ix->zero_poly, ix->n * 32))) return fail(rc);
    if ((rc = kh_dev_memset_zero(ix->zero_poly, ix->n * 32))) return fail(rc);
    // the commitment to the zero public polynomial: infinity per chunk (commit_non_hiding), masked with blinders 1 (prover.rs:296-309)
    const khost::Fld F(ix->fid);
    std::vector<uint64_t> zxy(8 * ix->nch, 0), ones(4 * ix->nch); std::vector<uint8_t> zinf(ix->nch, 1);
    for (size_t c = 0; c < ix->nch; c++) memcpy(&ones[4 * c], &F.f.one, 32);
    ix->zsel_xy.resize(8 * ix->nch); ix->zsel_inf.resize(ix->nch);
    if ((rc = kh_mask_custom(srs, zxy.data(), zinf.data(), ix->nch, ones.data(), ix->nch, ix->zsel_xy.data(), ix->zsel_inf.data()))) return fail(rc);
    if ((rc = kh_sync())) return fail(rc);
    *out = ix;
    return KH_OK;
}
void kh_prover_index_free(kh_prover_index_t* ix) {
    if (!ix) return;
    if (ix->zero_poly) (void)kh_dev_free(ix->zero_poly);
    for (uint64_t* p : {ix->own_d1, ix->own_dc, ix->own_d8, ix->own_l1, ix->own_lc, ix->own_l8}) if (p) (void)kh_dev_free(p);
    if (ix->own_wires) (void)kh_dev_free(ix->own_wires);
    delete ix->lk;
    delete ix;
}
int kh_prover_index_attach_lookup(kh_prover_index_t* ix, const int* patterns, size_t n_patterns, const uint64_t* const* selectors_d1,
                                  const uint64_t* const* selectors_c, const uint64_t* const* selectors_d8, const uint64_t* const* table_cols_d1, size_t n_table_cols,
                                  const uint64_t* table_ids_d1, const uint64_t* const* atoms_d8) {
    if (!ix || !patterns || !n_patterns || n_patterns > 4 || !selectors_d1 || !selectors_c || !selectors_d8 || !table_cols_d1 || !n_table_cols || !atoms_d8) {
        kh::set_error("kh_prover_index_attach_lookup: bad argument"); return KH_E_INVALID;
    }
    if (ix->created) {
        kh::set_error(ix->lk ? "kh_prover_index_attach_lookup: the index comes from kh_prover_index_create_lookup and carries its own lookup index"
                             : "kh_prover_index_attach_lookup: the index comes from kh_prover_index_create, whose digest covers no lookup index");
        return KH_E_INVALID;
    }
    kh_lookup_index* lk = new (std::nothrow) kh_lookup_index();
    if (!lk) { kh::set_error("out of memory"); return KH_E_NOMEM; }
    for (size_t k = 0; k < n_patterns; k++) {
        if (patterns[k] < 0 || patterns[k] > 3 || (k && patterns[k] <= patterns[k - 1]) || !selectors_d1[k] || !selectors_c[k] || !selectors_d8[k]) {
            kh::set_error("lookup patterns must be distinct ids 0..3 in increasing order, with their selector columns"); delete lk; return KH_E_INVALID;
        }
        lk->pats.push_back(patterns[k]);
        lk->sel1.push_back(selectors_d1[k]); lk->selc.push_back(selectors_c[k]); lk->sel8.push_back(selectors_d8[k]);
        const Pattern& P = PATTERNS[patterns[k]];
        if ((size_t)P.n > lk->mpr) lk->mpr = (size_t)P.n;
        for (int i = 0; i < P.n; i++) if ((size_t)P.l[i].ncell > lk->mjs) lk->mjs = (size_t)P.l[i].ncell;
    }
    for (size_t k = 0; k < n_table_cols; k++) { if (!table_cols_d1[k]) { kh::set_error("null table column"); delete lk; return KH_E_INVALID; } lk->tcols.push_back(table_cols_d1[k]); }
    lk->tids = table_ids_d1;
    for (int a = 0; a < 3; a++) { if (!atoms_d8[a]) { kh::set_error("null atom column"); delete lk; return KH_E_INVALID; } lk->atoms8[a] = atoms_d8[a]; }
    delete ix->lk;
    ix->lk = lk;
    return KH_OK;
}
int kh_prover_index_attach_runtime_tables(kh_prover_index_t* ix, const uint64_t* selector_d1, const uint64_t* selector_c, const uint64_t* selector_d8, size_t offset,
                                          size_t length) {
    if (ix && ix->created) {
        kh::set_error(ix->lk ? "kh_prover_index_attach_runtime_tables: the index comes from kh_prover_index_create_lookup, which configures its runtime tables itself"
                             : "kh_prover_index_attach_runtime_tables: the index comes from kh_prover_index_create (no lookup index)");
        return KH_E_INVALID;
    }
    if (!ix || !ix->lk || !selector_d1 ||!selector_c || !selector_d8 || !length || offset + length + ix->zk >= ix->n || ix->lk->tcols.size() < 2) {
        kh::set_error("kh_prover_index_attach_runtime_tables: attach the lookup index first; %zu runtime rows at %zu must fit the table (two columns at least)", length, offset);
        return KH_E_INVALID;
    }
    ix->lk->rtsel1 = selector_d1; ix->lk->rtselc = selector_c; ix->lk->rtsel8 = selector_d8;
    ix->lk->rt_offset = offset; ix->lk->rt_len = length;
    return KH_OK;
}

// ConstraintSystem::create(gates).public(k).build() + ProverIndex::verifier_index() (constraints.rs, prover_index.rs, verifier_index.rs:175-300,
// 405-540): the same columns, commitments and digest as proof_systems_amd/prover.py::ProverIndex + set_wiring (+ lookup.py::LookupIndex +
// attach_lookup), built from the gate records by one kernel pass (poly.hip: k_index_columns), the lookup passes of lookup_index.hip and the
// library's own transforms and MSMs.  One builder serves both entry points: kh_prover_index_create is the builder with lookups disallowed.
namespace {
struct LookupInput { const kh_lookup_table_t* tables; size_t n_tables; const kh_runtime_table_cfg_t* runtime; size_t n_runtime; };
constexpr int XOR_TABLE_ID = 0, RANGE_CHECK_TABLE_ID = 1;      // tables/mod.rs:13,16
constexpr size_t XOR_TABLE_LEN = 256, RANGE_CHECK_TABLE_LEN = 4096;
// the optional gates in the column order kh_prover_index_new documents (proof.rs:95-106) ...
const char* const OPTIONAL_GATE_NAMES[6] = {"RangeCheck0", "RangeCheck1", "ForeignFieldAdd", "ForeignFieldMul", "Xor16", "Rot64"};
// ... their position in VerifierIndex::digest (verifier_index.rs:405-540): range_check0, range_check1, foreign_field_mul, foreign_field_add, xor, rot
const int OPTIONAL_DIGEST_ORDER[6] = {0, 1, 3, 2, 4, 5};
// LookupPattern::from_gate (lookups.rs:500-513) per optional gate: 1 + pattern id on CURR | (1 + pattern id on NEXT) << 4
const uint8_t OPTIONAL_LOOKUP_CODE[6] = {3, 3 | (3 << 4), 0, 4 | (4 << 4), 1, 3};
constexpr uint8_t LOOKUP_GATE_CODE = 2;                         // GateType::Lookup: the Lookup pattern on CURR

int index_build(const char* who, kh_srs_t* srs, size_t n_gates, const int* gate_types, const uint32_t* wires, const uint64_t* coeffs, unsigned public_inputs,
                const LookupInput* lin, kh_prover_index_t** out) {
    if (out) *out = nullptr;
    if (!srs || !out || !gate_types || !wires || !coeffs) { kh::set_error("%s: null argument", who); return KH_E_INVALID; }
    if (lin && ((lin->n_tables && !lin->tables) || (lin->n_runtime && !lin->runtime))) { kh::set_error("%s: null table list", who); return KH_E_INVALID; }
    if (n_gates < 2) { kh::set_error("%s: %zu gates, a circuit has at least 2 (constraints.rs)", who, n_gates); return KH_E_INVALID; }
    const auto t0 = std::chrono::steady_clock::now();
    const int curve = kh_srs_curve(srs), fid = curve == KH_CURVE_VESTA ? KH_FIELD_FP : KH_FIELD_FQ;
    const size_t size = kh_srs_size(srs);
    const khost::Fld F(fid);
    // ---- the gate types: which optional gates and lookup patterns the circuit has; refusals with their reason
    const int ngates = kh_gate_count();
    std::vector<int> base_col(ngates, -1), opt_of(ngates, -1);       // base_col: the selector column of an always-present gate; opt_of: index into OPTIONAL_GATE_NAMES
    for (int g = 0; g < ngates; g++) {
        const char* nm = kh_gate_name(g);
        if (!strcmp(nm, "Generic")) base_col[g] = (int)COLUMNS;
        for (int k = 0; k < 5; k++) if (!strcmp(nm, LIB_GATES[k])) base_col[g] = (int)SEL0 + k;
        for (int k = 0; k < 6; k++) if (!strcmp(nm, OPTIONAL_GATE_NAMES[k])) opt_of[g] = k;
    }
    bool opt_present[6] = {false, false, false, false, false, false}, pat_used[4] = {false, false, false, false};
    unsigned live = 0;
    char gate_error[320] = "";                       // the first refused row: reported after the domain's own refusals, as kh_prover_index_create always has
    for (size_t i = 0; i < n_gates; i++) {
        const int t = gate_types[i];
        if (t == KH_GATE_ZERO) continue;
        if (lin && t == KH_GATE_LOOKUP) { pat_used[LOOKUP_GATE_CODE - 1] = true; continue; }
        if (t < 0 || t >= ngates) {
            if (!gate_error[0]) snprintf(gate_error, sizeof(gate_error), "%s: unknown gate type id %d at row %zu", who, t, i);
            continue;
        }
        if (base_col[t] >= 0) {
            if (base_col[t] >= (int)SEL0) live |= 1u << (base_col[t] - (int)SEL0);
            continue;
        }
        const int o = opt_of[t];
        const uint8_t code = o >= 0 ? OPTIONAL_LOOKUP_CODE[o] : 0;
        if (o < 0 || (code && !lin)) {
            const char* nm = kh_gate_name(t);
            if (gate_error[0]) continue;
            if (!strcmp(nm, "Permutation")) snprintf(gate_error, sizeof(gate_error), "%s: row %zu: Permutation is not a gate type of a circuit", who, i);
            else snprintf(gate_error, sizeof(gate_error), "%s: row %zu: %s has a lookup pattern; its index needs the lookup index (kh_prover_index_new + "
                          "kh_prover_index_attach_lookup)", who, i, nm);
            continue;
        }
        opt_present[o] = true;
        if (code & 15) pat_used[(code & 15) - 1] = true;
        if (code >> 4) pat_used[(code >> 4) - 1] = true;
    }
    std::vector<int> pats;                           // LookupPatterns::into_iter: xor, lookup, range_check, foreign_field_mul
    for (int q = 0; q < 4; q++) if (pat_used[q]) pats.push_back(q);
    const size_t npat = pats.size();
    // ---- the lookup tables: lengths for the domain; values, ids and the dummy entry checked on the host
    struct Table { int id; size_t width, len; int kind; const uint64_t* data; };      // kind as in lookup_index.hip: 0 data, 1 range check, 2 xor
    std::vector<Table> tabs;
    size_t rt_offset = 0, rt_len = 0, lookup_domain = 0;
    bool fixed_zero_id = false;
    if (lin) {
        for (size_t k = 0; k < lin->n_tables; k++) {
            const kh_lookup_table_t& t = lin->tables[k];
            if (!t.width || t.width > 128 || (t.len && !t.data)) { kh::set_error("%s: lookup table %zu: %zu columns of %zu entries, data %s", who, k, t.width, t.len, t.data ? "given" : "NULL"); return KH_E_INVALID; }
            tabs.push_back(Table{t.id, t.width, t.len, 0, t.data});
            lookup_domain += t.len;
            fixed_zero_id |= t.id == 0;
        }
        if (pat_used[2] || pat_used[3]) { tabs.push_back(Table{RANGE_CHECK_TABLE_ID, 1, RANGE_CHECK_TABLE_LEN, 1, nullptr}); lookup_domain += RANGE_CHECK_TABLE_LEN; }
        if (pat_used[0]) { tabs.push_back(Table{XOR_TABLE_ID, 3, XOR_TABLE_LEN, 2, nullptr}); lookup_domain += XOR_TABLE_LEN; }
        for (const Table& t : tabs) rt_offset += t.len;
        for (size_t k = 0; k < lin->n_runtime; k++) {
            const kh_runtime_table_cfg_t& t = lin->runtime[k];
            if (t.len && !t.first_column) { kh::set_error("%s: runtime table %zu: NULL first column", who, k); return KH_E_INVALID; }
            for (size_t j = 0; j < k; j++) if (lin->runtime[j].id == t.id) { kh::set_error("%s: runtime table id %d is configured twice", who, t.id); return KH_E_INVALID; }
            tabs.push_back(Table{t.id, 1, t.len, 0, t.first_column});
            rt_len += t.len; lookup_domain += t.len;
        }
    }
    const bool has_rt = lin && lin->n_runtime;
    if (!fixed_zero_id) lookup_domain += 1;          // the dummy entry (constraints.rs:883-945)
    // ---- the domain: zk_rows and the number of chunks follow each other, with the SRS size as max_poly_size (constraints.rs:769-771, 946-999)
    const size_t lower = n_gates > lookup_domain + 1 ? n_gates : lookup_domain + 1;
    size_t zk = 3, bound = lower + zk, nch = 1;
    for (;;) {
        size_t sz = 1; while (sz < bound) sz <<= 1;
        nch = sz < size ? 1 : sz / size;
        zk = (2 * (PERMUTS + 1) * nch - 2) / PERMUTS + 1;
        bound = lower + zk;
        if (sz >= bound) break;
    }
    unsigned logn = 0; while (((size_t)1 << logn) < bound) logn++;
    const size_t n = (size_t)1 << logn;
    if (logn > 26 || (n >= size && n % size)) { kh::set_error("%s: a domain of 2^%u rows over an SRS of %zu points is not supported", who, logn, size); return KH_E_INVALID; }
    if (public_inputs >= n - zk) { kh::set_error("%s: %u public inputs, the domain has %zu rows before the %zu zero-knowledge rows", who, public_inputs, n - zk, zk); return KH_E_INVALID; }
    if (gate_error[0]) { kh::set_error("%s", gate_error); return KH_E_INVALID; }
    if (lin && lin->n_runtime && !npat) { kh::set_error("%s: runtime tables are configured, but no gate of the circuit has a lookup pattern", who); return KH_E_INVALID; }
    // ---- the lookup constraint system (lookup/index.rs:188-430), when a gate has a pattern: the refusals of LookupConstraintSystem::create
    size_t mpr = 0, mjs = 0, width = 0, entries = 0, data_elems = 0;
    bool has_ids = false;
    if (npat) {
        for (int q : pats) {
            const Pattern& P = PATTERNS[q];
            if ((size_t)P.n > mpr) mpr = (size_t)P.n;
            for (int i = 0; i < P.n; i++) if ((size_t)P.l[i].ncell > mjs) mjs = (size_t)P.l[i].ncell;
        }
        width = mjs;
        for (size_t k = 0; k < tabs.size(); k++) {
            const Table& t = tabs[k];
            const bool runtime = k >= tabs.size() - (lin ? lin->n_runtime : 0);
            for (size_t j = 0; j < k; j++) if (tabs[j].id == t.id) { kh::set_error("%s: lookup table id collision: two tables have id %d", who, t.id); return KH_E_INVALID; }
            const size_t w = runtime ? 2 : t.width;  // a runtime table's second column comes with each proof (index.rs:241-311)
            if (w > width) width = w;
            has_ids |= t.id != 0;
            entries += t.len;
            if (t.kind == 0) {
                for (size_t e = 0; e < t.width * t.len; e++)
                    if (khost::geq(load(t.data + 4 * e), F.f.p)) { kh::set_error("%s: lookup table with id %d: value %zu is not a canonical field element (>= p)", who, t.id, e); return KH_E_INVALID; }
                if (t.id == 0) {                     // the dummy lookup (0, ..., 0) with table id 0 must be in the table (index.rs:330-346)
                    bool zero_row = false;
                    for (size_t r = 0; r < t.len && !zero_row; r++) {
                        zero_row = true;
                        for (size_t c = 0; c < t.width && zero_row; c++) { const fe v = load(t.data + 4 * (c * t.len + r)); zero_row = !(v.l[0] | v.l[1] | v.l[2] | v.l[3]); }
                    }
                    if (!zero_row) { kh::set_error("%s: the lookup table with id 0 has no all-zero entry (TableIDZeroMustHaveZeroEntry)", who); return KH_E_INVALID; }
                }
                data_elems += t.width * t.len;
            }
        }
        if (entries >= n - zk - 1) { kh::set_error("%s: %zu lookup table entries, the domain of %zu rows has room for fewer than %zu (LookupTableTooLong)", who, entries, n, n - zk - 1); return KH_E_INVALID; }
    } else if (lin) {                                // tables of a circuit without lookups only size the domain; their values are still the caller's claim
        for (const Table& t : tabs)
            for (size_t e = 0; t.kind == 0 && e < t.width * t.len; e++)
                if (khost::geq(load(t.data + 4 * e), F.f.p)) { kh::set_error("%s: lookup table with id %d: value %zu is not a canonical field element (>= p)", who, t.id, e); return KH_E_INVALID; }
    }
    // ---- the selector column of every row and its lookup code
    size_t nopt = 0;
    int opt_col[6];
    for (int k = 0; k < 6; k++) opt_col[k] = opt_present[k] ? (int)(OPT0 + nopt++) : -1;
    const size_t ncol = OPT0 + nopt;
    std::vector<uint8_t> selcol(n_gates), lkcode(npat ? n_gates : 0);
    for (size_t i = 0; i < n_gates; i++) {
        const int t = gate_types[i];
        uint8_t col = 0, code = 0;
        if (t == KH_GATE_LOOKUP) code = LOOKUP_GATE_CODE;
        else if (t != KH_GATE_ZERO) {
            if (base_col[t] >= 0) col = (uint8_t)base_col[t];
            else { col = (uint8_t)opt_col[opt_of[t]]; code = OPTIONAL_LOOKUP_CODE[opt_of[t]]; }
        }
        selcol[i] = col;
        if (npat) lkcode[i] = code;
    }
    for (size_t i = 0; i < 7 * n_gates; i++)         // the kernel gathers sid[row]: nothing outside the domain may reach it
        if (wires[2 * i] >= n || wires[2 * i + 1] >= PERMUTS) {
            kh::set_error("%s: row %zu, cell %zu is wired to (%u, %u), outside %zu rows x %zu columns", who, i / 7, i % 7, wires[2 * i], wires[2 * i + 1], n, PERMUTS);
            return KH_E_INVALID;
        }
    for (size_t i = 0; i < COLUMNS * n_gates; i++)
        if (khost::geq(load(coeffs + 4 * i), F.f.p)) {
            kh::set_error("%s: row %zu, coefficient %zu is not a canonical field element (>= p)", who, i / COLUMNS, i % COLUMNS);
            return KH_E_INVALID;
        }
    // ---- device work, on the SRS's device
    struct DeviceRestore { int prev; ~DeviceRestore() { if (prev >= 0) (void)kh_set_device(prev); } } device_restore{kh_get_device()};
    KP(kh_set_device(kh_srs_device(srs)));
    if (kh_srs_lagrange_chunks(srs, logn) == 0) KP(kh_srs_compute_lagrange(srs, logn));      // SRS::lagrange_basis (index time)
    fe shifts[7];
    KP(kh_permutation_shifts(fid, logn, shifts[0].l));
    Dev d1, dc, d8, g_sel, g_wires, g_coeffs;
    KP(d1.alloc(ncol * n)); KP(dc.alloc((ncol + 2) * n)); KP(d8.alloc((ncol + 2) * 8 * n));
    KP(kh_dev_alloc((void**)&g_sel.p, n_gates)); KP(kh_dev_alloc((void**)&g_wires.p, 56 * n_gates)); KP(g_coeffs.alloc(COLUMNS * n_gates));
    KP(kh_dev_upload(g_sel.p, selcol.data(), n_gates));
    KP(kh_dev_upload(g_wires.p, wires, 56 * n_gates));
    KP(kh_dev_upload(g_coeffs.p, coeffs, 32 * COLUMNS * n_gates));
    const fe one = F.f.one;
    uint64_t* sid = d1.at((COLUMNS + 1) * n);
    KP(kh_dev_memset_zero(sid, 32 * n));                               // the polynomial x: its evaluations are sid[j] = omega^j
    KP(kh_dev_upload(sid + 4, one.l, 32));
    KP(kh_ntt_dev(fid, sid, logn, 0, 1));
    KP(kh::index_columns_dev(fid, (const uint8_t*)g_sel.p, (const uint32_t*)g_wires.p, g_coeffs.p, n_gates, n, zk, shifts[0].l, ncol, d1.p));
    // the lookup columns, d1: [pattern selectors | runtime selector | table columns | table ids]; coefficient forms and d8 of the selectors; the atoms on d8
    const size_t nsel = npat + (has_rt ? 1 : 0), nlk = npat ? nsel + width + (has_ids ? 1 : 0) : 0;
    Dev l1, lc, l8, g_code, g_segs, g_data;
    std::vector<uint64_t> segs;
    if (npat) {
        KP(l1.alloc(nlk * n)); KP(lc.alloc(nsel * n)); KP(l8.alloc((nsel + 3) * 8 * n));
        KP(kh_dev_alloc((void**)&g_code.p, n_gates)); KP(g_data.alloc(data_elems ? data_elems : 1));
        KP(kh_dev_upload(g_code.p, lkcode.data(), n_gates));
        size_t row = 0, off = 0;
        for (const Table& t : tabs) {                // segment records of k_lookup_tables (lookup_index.hip)
            fe idv = {{(uint64_t)(t.id < 0 ? -(int64_t)t.id : (int64_t)t.id), 0, 0, 0}};
            idv = F.to_mont(idv);
            if (t.id < 0) idv = F.neg(idv);
            const uint64_t rec[8] = {row, t.len, off, (uint64_t)t.kind | ((uint64_t)t.width << 32), idv.l[0], idv.l[1], idv.l[2], idv.l[3]};
            segs.insert(segs.end(), rec, rec + 8);
            if (t.kind == 0 && t.len) { KP(kh_dev_upload(g_data.at(off), t.data, 32 * t.width * t.len)); off += t.width * t.len; }
            row += t.len;
        }
        if (segs.empty()) segs.assign(8, 0);         // no table at all: every row is padding
        KP(kh_dev_alloc((void**)&g_segs.p, 8 * segs.size()));
        KP(kh_dev_upload(g_segs.p, segs.data(), 8 * segs.size()));
        KP(kh::lookup_selectors_dev(fid, (const uint8_t*)g_code.p, n_gates, n, pats.data(), npat, l1.p));
        std::vector<uint64_t> seg_starts(segs.size() / 8);           // the prefix offsets, for the kernel's arguments
        for (size_t k = 0; k < seg_starts.size(); k++) seg_starts[k] = segs[8 * k];
        KP(kh::lookup_tables_dev(fid, g_segs.p, seg_starts.data(), segs.size() / 8, g_data.p, n, width, l1.at(nsel * n), has_ids ? l1.at((nsel + width) * n) : nullptr,
                                 has_rt ? l1.at(npat * n) : nullptr, rt_offset, has_rt ? rt_len : 0, zk));
    }
    KP(kh_sync());
    const auto t1 = std::chrono::steady_clock::now();
    // ---- coefficient forms, x and the permutation vanishing polynomial (x - w^(n-zk))(x - w^(n-zk+1))(x - w^(n-1)) (permutation.rs:107-118), d8
    KP(kh_dev_copy(dc.p, d1.p, 32 * ncol * n));
    KP(kh_ntt_dev(fid, dc.p, logn, 1, ncol));
    uint64_t w[4];
    KP(kh_domain_generator(fid, logn, w));
    const fe omega = load(w);
    const fe a = fpow(F, omega, n - zk), b = F.mul(a, omega), c = fpow(F, omega, n - 1);
    const fe ab = F.mul(a, b), zkpm[4] = {F.neg(F.mul(ab, c)), F.add(F.add(ab, F.mul(a, c)), F.mul(b, c)), F.neg(F.add(F.add(a, b), c)), one};
    KP(kh_dev_memset_zero(dc.at(ncol * n), 32 * 2 * n));
    KP(kh_dev_upload(dc.at(ncol * n + 1), one.l, 32));
    KP(kh_dev_upload(dc.at((ncol + 1) * n), zkpm, sizeof(zkpm)));
    KP(kh_lde_dev(fid, dc.p, logn, 3, d8.p, ncol + 2));
    if (npat) {
        KP(kh_dev_copy(lc.p, l1.p, 32 * nsel * n));
        KP(kh_ntt_dev(fid, lc.p, logn, 1, nsel));
        KP(kh_lde_dev(fid, lc.p, logn, 3, l8.p, nsel));
        // the row-set atoms (expr.rs:883-893) from x on d8: x^n - 1 takes the eight values w8^j - 1 there, w8 = g^n for the generator g of d8
        uint64_t g8[4];
        KP(kh_domain_generator(fid, logn + 3, g8));
        const fe w8 = fpow(F, load(g8), n), af = fpow(F, omega, n - zk - 1);
        fe zh8[8], pw = one;
        for (int j = 0; j < 8; j++) { zh8[j] = F.sub(pw, one); pw = F.mul(pw, w8); }
        const fe nf = F.to_mont(fe{{(uint64_t)n, 0, 0, 0}}), limf = F.mul(nf, F.inv(af));
        uint64_t* atoms = l8.at(nsel * 8 * n);
        KP(kh::lookup_atom_denominators_dev(fid, d8.at(ncol * 8 * n), n, zk, af.l, omega.l, atoms));
        KP(kh_batch_inversion_dev(fid, atoms + 4 * 8 * n, 2 * 8 * n));
        KP(kh::lookup_atom_finish_dev(fid, n, zk, zh8[0].l, nf.l, limf.l, atoms));
    }
    KP(kh_sync());
    const auto t2 = std::chrono::steady_clock::now();
    // ---- commitments over the Lagrange basis: [coefficients | generic], [sigma | five selectors | optional] and the lookup columns, batched MSMs per chunk
    const size_t k1 = COLUMNS + 1, k2 = PERMUTS + 5 + nopt;
    const size_t kmax = 16;
    std::vector<uint64_t> xy1(8 * k1 * nch), xy2(8 * k2 * nch), xyl(8 * nlk * nch), o(8 * (k2 > kmax ? k2 : kmax));
    std::vector<uint8_t> inf1(k1 * nch), inf2(k2 * nch), infl(nlk * nch), oi(k2 > kmax ? k2 : kmax);
    for (size_t ch = 0; ch < nch; ch++) {            // chunk lists flat, commitment after commitment
        KP(kh_msm_batch_dev(srs, (int)logn, (unsigned)ch, 0, d1.p, n, k1, 1, o.data(), oi.data()));
        for (size_t i = 0; i < k1; i++) { memcpy(&xy1[8 * (i * nch + ch)], &o[8 * i], 64); inf1[i * nch + ch] = oi[i]; }
        KP(kh_msm_batch_dev(srs, (int)logn, (unsigned)ch, 0, d1.at((COLUMNS + 2) * n), n, k2, 1, o.data(), oi.data()));
        for (size_t i = 0; i < k2; i++) { memcpy(&xy2[8 * (i * nch + ch)], &o[8 * i], 64); inf2[i * nch + ch] = oi[i]; }
        for (size_t i0 = 0; i0 < nlk; i0 += kmax) {
            const size_t k = nlk - i0 < kmax ? nlk - i0 : kmax;
            KP(kh_msm_batch_dev(srs, (int)logn, (unsigned)ch, 0, l1.at(i0 * n), n, k, 1, o.data(), oi.data()));
            for (size_t i = 0; i < k; i++) { memcpy(&xyl[8 * ((i0 + i) * nch + ch)], &o[8 * i], 64); infl[(i0 + i) * nch + ch] = oi[i]; }
        }
    }
    const auto t3 = std::chrono::steady_clock::now();
    // ---- the generic and the five library selectors, the table columns and the table ids masked with blinder 1 (verifier_index.rs:189-216, 255-300),
    //      the digest (verifier_index.rs:405-540)
    const size_t ntab = npat ? width + (has_ids ? 1 : 0) : 0, nm = 6 + ntab;
    std::vector<uint64_t> mxy(8 * nm * nch), mout(8 * nm * nch), ones(4 * nm * nch);
    std::vector<uint8_t> minf(nm * nch), moinf(nm * nch);
    memcpy(mxy.data(), &xy1[8 * COLUMNS * nch], 64 * nch); memcpy(minf.data(), &inf1[COLUMNS * nch], nch);
    memcpy(&mxy[8 * nch], &xy2[8 * PERMUTS * nch], 64 * 5 * nch); memcpy(&minf[nch], &inf2[PERMUTS * nch], 5 * nch);
    if (ntab) { memcpy(mxy.data() + 8 * 6 * nch, xyl.data() + 8 * nsel * nch, 64 * ntab * nch); memcpy(minf.data() + 6 * nch, infl.data() + nsel * nch, ntab * nch); }
    for (size_t i = 0; i < nm * nch; i++) memcpy(&ones[4 * i], one.l, 32);
    KP(kh_mask_custom(srs, mxy.data(), minf.data(), nm * nch, ones.data(), nm * nch, mout.data(), moinf.data()));
    SpongeH sp;
    KP(kh_sponge_new(KH_SPONGE_FQ, curve, &sp.s));
    KP(kh_sponge_absorb_g(sp.s, xy2.data(), inf2.data(), PERMUTS * nch));                          // sigma
    KP(kh_sponge_absorb_g(sp.s, xy1.data(), inf1.data(), COLUMNS * nch));                          // coefficients
    KP(kh_sponge_absorb_g(sp.s, mout.data(), moinf.data(), 6 * nch));                              // generic, psm, complete_add, mul, emul, endomul_scalar
    for (int k : OPTIONAL_DIGEST_ORDER)
        if (opt_present[k]) { const size_t j = PERMUTS + 5 + (size_t)(opt_col[k] - (int)OPT0); KP(kh_sponge_absorb_g(sp.s, xy2.data() + 8 * j * nch, inf2.data() + j * nch, nch)); }
    if (npat) {                                      // the lookup index (verifier_index.rs:482-530): tables, ids, runtime selector, pattern selectors
        KP(kh_sponge_absorb_g(sp.s, mout.data() + 8 * 6 * nch, moinf.data() + 6 * nch, ntab * nch));
        if (has_rt) KP(kh_sponge_absorb_g(sp.s, xyl.data() + 8 * npat * nch, infl.data() + npat * nch, nch));
        KP(kh_sponge_absorb_g(sp.s, xyl.data(), infl.data(), npat * nch));
    }
    fe digest;
    KP(kh_sponge_squeeze_field(sp.s, digest.l));
    // ---- the prover index over the columns (kh_prover_index_new's body), which now owns them
    std::vector<int> optional;
    for (int k = 0; k < 6; k++) if (opt_present[k]) for (int g = 0; g < ngates; g++) if (opt_of[g] == k) optional.push_back(g);
    kh_prover_index* ix = nullptr;
    KP(kh_prover_index_new(srs, logn, (unsigned)zk, public_inputs, d1.p, dc.p, d8.p, optional.data(), optional.size(), live, shifts[0].l, digest.l, &ix));
    ix->created = true;
    ix->own_d1 = d1.p; ix->own_dc = dc.p; ix->own_d8 = d8.p;
    d1.p = dc.p = d8.p = nullptr;
    ix->own_wires = (uint32_t*)g_wires.p; ix->n_gates = n_gates;
    g_wires.p = nullptr;
    auto points = [&](int s, const uint64_t* pxy, const uint8_t* pinf, size_t cnt) {
        ix->vsec[s].limbs.assign(pxy, pxy + 8 * cnt); ix->vsec[s].flags.assign(pinf, pinf + cnt); ix->vsec[s].count = cnt;
    };
    points(KH_VINDEX_SIGMA_COMM, xy2.data(), inf2.data(), PERMUTS * nch);
    points(KH_VINDEX_COEFFICIENTS_COMM, xy1.data(), inf1.data(), COLUMNS * nch);
    points(KH_VINDEX_GENERIC_COMM, mout.data(), moinf.data(), nch);
    points(KH_VINDEX_SELECTOR_COMM, &mout[8 * nch], &moinf[nch], 5 * nch);
    points(KH_VINDEX_OPTIONAL_COMM, xy2.data() + 8 * (PERMUTS + 5) * nch, inf2.data() + (PERMUTS + 5) * nch, nopt * nch);
    if (npat) {
        kh_lookup_index* lk = new (std::nothrow) kh_lookup_index();
        if (!lk) { kh_prover_index_free(ix); kh::set_error("out of memory"); return KH_E_NOMEM; }
        lk->pats = pats; lk->mpr = mpr; lk->mjs = mjs;
        for (size_t k = 0; k < npat; k++) { lk->sel1.push_back(l1.at(k * n)); lk->selc.push_back(lc.at(k * n)); lk->sel8.push_back(l8.at(k * 8 * n)); }
        for (size_t k = 0; k < width; k++) lk->tcols.push_back(l1.at((nsel + k) * n));
        if (has_ids) lk->tids = l1.at((nsel + width) * n);
        for (int k = 0; k < 3; k++) lk->atoms8[k] = l8.at((nsel + (size_t)k) * 8 * n);
        if (has_rt) { lk->rtsel1 = l1.at(npat * n); lk->rtselc = lc.at(npat * n); lk->rtsel8 = l8.at(npat * 8 * n); lk->rt_offset = rt_offset; lk->rt_len = rt_len; }
        size_t first_row = 0;
        for (size_t k = 0; k < tabs.size(); k++) {       // the combined table's order: fixed, gate, runtime tables
            const bool runtime = k >= tabs.size() - lin->n_runtime;
            lk->tables.push_back({tabs[k].id, first_row, tabs[k].len, runtime, runtime ? first_row - rt_offset : 0});
            first_row += tabs[k].len;
        }
        ix->lk = lk;
        ix->own_l1 = l1.p; ix->own_lc = lc.p; ix->own_l8 = l8.p;
        l1.p = lc.p = l8.p = nullptr;
        points(KH_VINDEX_LOOKUP_TABLE_COMM, mout.data() + 8 * 6 * nch, moinf.data() + 6 * nch, width * nch);
        points(KH_VINDEX_LOOKUP_TABLE_IDS_COMM, mout.data() + 8 * (6 + width) * nch, moinf.data() + (6 + width) * nch, has_ids ? nch : 0);
        points(KH_VINDEX_LOOKUP_SELECTOR_COMM, xyl.data(), infl.data(), npat * nch);
        points(KH_VINDEX_LOOKUP_RUNTIME_SELECTOR_COMM, xyl.data() + 8 * npat * nch, infl.data() + npat * nch, has_rt ? nch : 0);
        unsigned mask = 0;
        for (int q : pats) mask |= 1u << q;
        ix->vsec[KH_VINDEX_LOOKUP_INFO].limbs = {mpr, mjs, mjs > 1 ? 1u : 0u, has_rt ? 1u : 0u, mask, width, has_rt ? rt_offset : 0, has_rt ? rt_len : 0};
        ix->vsec[KH_VINDEX_LOOKUP_INFO].count = 2;
    }
    const auto t4 = std::chrono::steady_clock::now();
    const std::chrono::steady_clock::time_point ts[5] = {t0, t1, t2, t3, t4};
    for (int i = 0; i < 4; i++) ix->phase[i] = std::chrono::duration<double>(ts[i + 1] - ts[i]).count();
    *out = ix;
    return KH_OK;
}
}  // namespace

int kh_prover_index_create(kh_srs_t* srs, size_t n_gates, const int* gate_types, const uint32_t* wires, const uint64_t* coeffs, unsigned public_inputs,
                           kh_prover_index_t** out) {
    return index_build("kh_prover_index_create", srs, n_gates, gate_types, wires, coeffs, public_inputs, nullptr, out);
}
int kh_prover_index_create_lookup(kh_srs_t* srs, size_t n_gates, const int* gate_types, const uint32_t* wires, const uint64_t* coeffs, unsigned public_inputs,
                                  const kh_lookup_table_t* tables, size_t n_tables, const kh_runtime_table_cfg_t* runtime, size_t n_runtime,
                                  kh_prover_index_t** out) {
    const LookupInput lin{tables, n_tables, runtime, n_runtime};
    return index_build("kh_prover_index_create_lookup", srs, n_gates, gate_types, wires, coeffs, public_inputs, &lin, out);
}
int kh_prover_index_shape(const kh_prover_index_t* ix, unsigned* log2_n, unsigned* zk_rows, size_t* num_chunks) {
    if (!ix) { kh::set_error("kh_prover_index_shape: null index"); return KH_E_INVALID; }
    if (log2_n) *log2_n = ix->logn;
    if (zk_rows) *zk_rows = (unsigned)ix->zk;
    if (num_chunks) *num_chunks = ix->nch;
    return KH_OK;
}
int kh_verifier_index_section(const kh_prover_index_t* ix, int section, const uint64_t** limbs, const uint8_t** flags, size_t* count) {
    if (!ix || section < 0 || section > KH_VINDEX_LOOKUP_INFO || !limbs || !count) { kh::set_error("kh_verifier_index_section: bad argument"); return KH_E_INVALID; }
    if (section == KH_VINDEX_SHIFTS || section == KH_VINDEX_DIGEST) {
        *limbs = section == KH_VINDEX_SHIFTS ? ix->shifts[0].l : ix->digest.l;
        *count = section == KH_VINDEX_SHIFTS ? 7 : 1;
        if (flags) *flags = nullptr;
        return KH_OK;
    }
    if (!ix->created) { kh::set_error("kh_verifier_index_section: the index comes from kh_prover_index_new, whose commitments are the caller's"); return KH_E_NOTFOUND; }
    const kh_prover_index::VSec& s = ix->vsec[section];
    *limbs = s.limbs.data(); *count = s.count;
    if (flags) *flags = section == KH_VINDEX_LOOKUP_INFO ? nullptr : s.flags.data();
    return KH_OK;
}
}  // extern "C"
namespace kh {
// what kh_verifier_index_of (csrc/verifier.cpp) needs besides kh_verifier_index_section and kh_prover_index_shape
void prover_index_facts(const kh_prover_index_t* ix, kh_srs_t** srs, unsigned* public_inputs, const int** optional_gates, size_t* n_optional) {
    *srs = ix->srs; *public_inputs = (unsigned)ix->pub; *optional_gates = ix->optional.data(); *n_optional = ix->optional.size();
}
}  // namespace kh
extern "C" {
int kh_debug_lookup_column(const kh_prover_index_t* ix, int block, size_t k, const uint64_t** dev, size_t* elems) {
    if (!ix || !dev || !elems) { kh::set_error("kh_debug_lookup_column: null argument"); return KH_E_INVALID; }
    const kh_lookup_index* lk = ix->lk;
    if (!lk) { kh::set_error("kh_debug_lookup_column: the index has no lookup index"); return KH_E_NOTFOUND; }
    const uint64_t* p = nullptr;
    size_t len = ix->n;
    switch (block) {
        case KH_LOOKUP_COL_SELECTOR_D1: if (k < lk->sel1.size()) p = lk->sel1[k]; break;
        case KH_LOOKUP_COL_SELECTOR_C: if (k < lk->selc.size()) p = lk->selc[k]; break;
        case KH_LOOKUP_COL_SELECTOR_D8: if (k < lk->sel8.size()) p = lk->sel8[k]; len = 8 * ix->n; break;
        case KH_LOOKUP_COL_TABLE_D1: if (k < lk->tcols.size()) p = lk->tcols[k]; break;
        case KH_LOOKUP_COL_TABLE_IDS_D1: if (k == 0) p = lk->tids; break;
        case KH_LOOKUP_COL_ATOM_D8: if (k < 3) p = lk->atoms8[k]; len = 8 * ix->n; break;
        case KH_LOOKUP_COL_RUNTIME_SELECTOR: if (k < 3) p = k == 0 ? lk->rtsel1 : k == 1 ? lk->rtselc : lk->rtsel8; if (k == 2) len = 8 * ix->n; break;
        default: break;
    }
    if (!p) { kh::set_error("kh_debug_lookup_column: the index has no column %zu in block %d", k, block); return KH_E_NOTFOUND; }
    *dev = p; *elems = len;
    return KH_OK;
}
int kh_prover_index_lookup_table(const kh_prover_index_t* ix, int table_id, size_t* first_row, size_t* len, int* is_runtime, size_t* runtime_first,
                                 const uint64_t** keys_dev, const uint64_t** values_dev) {
    if (!ix) { kh::set_error("kh_prover_index_lookup_table: null index"); return KH_E_INVALID; }
    const kh_lookup_index* lk = ix->lk;
    if (!lk) { kh::set_error("kh_prover_index_lookup_table: the index has no lookup index"); return KH_E_NOTFOUND; }
    if (!ix->created) { kh::set_error("kh_prover_index_lookup_table: the index comes from kh_prover_index_new, whose tables are the caller's own"); return KH_E_NOTFOUND; }
    for (const kh_lookup_index::TableAt& t : lk->tables) {
        if (t.id != table_id) continue;
        if (first_row) *first_row = t.first_row;
        if (len) *len = t.len;
        if (is_runtime) *is_runtime = t.runtime ? 1 : 0;
        if (runtime_first) *runtime_first = t.runtime_first;
        if (keys_dev) *keys_dev = lk->tcols[0] + 4 * t.first_row;
        if (values_dev) *values_dev = lk->tcols.size() > 1 ? lk->tcols[1] + 4 * t.first_row : nullptr;
        return KH_OK;
    }
    kh::set_error("kh_prover_index_lookup_table: the index has no lookup table with id %d", table_id);
    return KH_E_NOTFOUND;
}
int kh_prover_index_phase_seconds(const kh_prover_index_t* ix, double* seconds, size_t cap) {
    if (!ix || !seconds) { kh::set_error("kh_prover_index_phase_seconds: null argument"); return KH_E_INVALID; }
    for (size_t i = 0; i < cap && i < 4; i++) seconds[i] = ix->phase[i];
    return 4;
}

// ProverIndex::verify (constraints.rs): the first row of the witness that violates its gate or a copy constraint -- or, kh_witness_check_full with
// KH_WITNESS_LOOKUPS, looks up a tuple that is in no table.  Kernels in witness_check.hip.  `allowed`: the flags the entry point `who` takes.
// runtime_on_device: runtime_values is device memory, read in stream order and not compared with p.
static int witness_check_impl(const char* who, unsigned allowed, kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev,
                              const uint64_t* runtime_values, bool runtime_on_device, size_t n_runtime, unsigned flags, kh_witness_report_t* out,
                              kh_witness_lookup_t* lookup_out) {
    if (!ix || !out) { kh::set_error("%s: null argument", who); return KH_E_INVALID; }
    if (!witness == !witness_dev) { kh::set_error("%s: give the witness either on the host or on the device", who); return KH_E_INVALID; }
    if (!flags || (flags & ~allowed)) {
        kh::set_error(allowed & KH_WITNESS_LOOKUPS ? "%s: flags %u: a combination of KH_WITNESS_GATES, KH_WITNESS_WIRES and KH_WITNESS_LOOKUPS" : "%s: flags %u: KH_WITNESS_GATES, KH_WITNESS_WIRES or both", who, flags);
        return KH_E_INVALID;
    }
    const size_t n = ix->n;
    if (witness && (rows > n || rows + ix->zk > n)) { kh::set_error("%s: %zu witness rows + %zu zero-knowledge rows do not fit the domain of %zu rows", who, rows, ix->zk, n); return KH_E_INVALID; }
    if ((flags & KH_WITNESS_WIRES) && !ix->own_wires) {
        kh::set_error("%s: KH_WITNESS_WIRES needs the gate list's wires, which only an index from kh_prover_index_create(_lookup) keeps; this one comes from "
                      "kh_prover_index_new (sigma columns only)", who);
        return KH_E_INVALID;
    }
    const khost::Fld F(ix->fid);
    const kh_lookup_index* lk = ix->lk;
    kh::WitnessLookups wl{};
    if (flags & KH_WITNESS_LOOKUPS) {
        if (!lk) { kh::set_error("%s: KH_WITNESS_LOOKUPS on an index without a lookup index (kh_prover_index_create_lookup, or kh_prover_index_attach_lookup)", who); return KH_E_INVALID; }
        if (!lookup_out) { kh::set_error("%s: KH_WITNESS_LOOKUPS needs lookup_out", who); return KH_E_INVALID; }
        const size_t rt_len = lk->rtsel1 ? lk->rt_len : 0;
        if (!rt_len && (runtime_values || n_runtime)) { kh::set_error("%s: runtime values for an index without runtime tables", who); return KH_E_INVALID; }
        if (n_runtime != rt_len || (rt_len && !runtime_values)) {
            kh::set_error("%s: RuntimeTablesInconsistent: the index has %zu runtime table rows, the call brings %zu", who, rt_len, runtime_values ? n_runtime : (size_t)0);
            return KH_E_INVALID;
        }
        if (runtime_on_device && (((uintptr_t)runtime_values) & 15)) { kh::set_error("%s: runtime_values_dev must be 16-byte aligned", who); return KH_E_INVALID; }
        for (size_t i = 0; !runtime_on_device && i < rt_len; i++)
            if (khost::geq(load(runtime_values + 4 * i), F.f.p)) { kh::set_error("%s: runtime value %zu is not below the field's modulus", who, i); return KH_E_INVALID; }
        if (n <= ix->zk + 1 || lk->tcols.empty() || lk->pats.empty()) { kh::set_error("%s: the lookup index is empty", who); return KH_E_INVALID; }
        wl.npat = lk->pats.size();
        for (size_t k = 0; k < wl.npat; k++) {
            const Pattern& P = PATTERNS[lk->pats[k]];
            kh::WitnessLookupPattern& q = wl.pat[k];
            q.pattern = lk->pats[k]; q.n = P.n; q.sel = lk->sel1[k];
            for (int i = 0; i < P.n; i++) {
                const JointLookup& J = P.l[i];
                q.l[i].tid_is_column = J.tid_is_column; q.l[i].tid_column = J.tid_is_column ? J.tid : 0; q.l[i].ncell = J.ncell;
                for (int c = 0; c < 3; c++) q.l[i].cells[c] = J.cells[c];
                const fe id = J.tid_is_column ? fe{{0, 0, 0, 0}} : F.to_mont(fe{{(uint64_t)J.tid, 0, 0, 0}});
                memcpy(q.l[i].id, id.l, 32);
            }
        }
        wl.L = n - ix->zk - 1; wl.W = lk->tcols.size(); wl.tcols = lk->tcols.data(); wl.tids = lk->tids;
        wl.rt_offset = rt_len ? lk->rt_offset : 0; wl.rt_len = rt_len;
        wl.runtime = rt_len && !runtime_on_device ? runtime_values : nullptr; wl.runtime_dev = rt_len && runtime_on_device ? runtime_values : nullptr;
    }
    struct DeviceRestore { int prev; ~DeviceRestore() { if (prev >= 0) (void)kh_set_device(prev); } } device_restore{kh_get_device()};
    KP(kh_set_device(kh_srs_device(ix->srs)));
    Dev wbuf;
    if (witness) {                                   // padded with zeros: no zero-knowledge rows, no randomness
        KP(wbuf.alloc(COLUMNS * n));
        if (rows < n) KP(kh_dev_memset_zero(wbuf.p, COLUMNS * n * 32));
        if (rows) KP(kh_dev_upload_2d(wbuf.p, n * 32, witness, rows * 32, rows * 32, COLUMNS));
    }
    // the selector column of every gate id: none = no launch.  Generic and the optional gates always, the library gates by live_mask
    std::vector<int> sel_col((size_t)kh_gate_count(), -1);
    if (flags & KH_WITNESS_GATES) {
        sel_col[(size_t)ix->gid_generic] = (int)COLUMNS;
        for (int k = 0; k < 5; k++) if (ix->live >> k & 1) sel_col[(size_t)ix->lib_gate[k]] = (int)SEL0 + k;
        for (size_t j = 0; j < ix->optional.size(); j++) sel_col[(size_t)ix->optional[j]] = (int)(OPT0 + j);
    }
    uint64_t st[4] = {0, 0, 0, 0};
    KP(kh::witness_check_dev(ix->fid, witness ? wbuf.p : witness_dev, ix->d1, n, sel_col.data(), sel_col.size(), ix->pub, ix->endo.l,
                             (flags & KH_WITNESS_WIRES) ? ix->own_wires : nullptr, ix->n_gates, (flags & KH_WITNESS_LOOKUPS) ? &wl : nullptr, st));
    kh_witness_report_t r;
    memset(&r, 0, sizeof(r));
    r.gate = -1;
    r.gate_rows_violated = (size_t)st[1]; r.cells_disconnected = (size_t)st[2];
    kh_witness_lookup_t l;
    memset(&l, 0, sizeof(l));
    l.pattern = -1; l.slot = -1;
    l.lookups_missing = (size_t)st[3];
    if (st[0] != ~(uint64_t)0) {                     // (key << 32) | detail, key = row * 64 + sub (witness_check.hip)
        const uint64_t key = st[0] >> 32; const uint32_t detail = (uint32_t)st[0];
        r.row = (size_t)(key >> 6);
        if ((key & 63) >= 8) {                       // the tuple the row looked up: read back from the witness, a few cells
            r.kind = KH_WITNESS_LOOKUP;
            l.pattern = (int)(detail & 3); l.slot = (int)(key & 63) - 8;
            KP_REQUIRE(l.slot < PATTERNS[l.pattern].n, "%s: status word names lookup %d of pattern %d", who, l.slot, l.pattern);
            const JointLookup& J = PATTERNS[l.pattern].l[l.slot];
            auto cell = [&](int c, uint64_t* dst) -> int {
                if (witness_dev) return kh_dev_download(dst, witness_dev + 4 * ((size_t)c * n + r.row), 32);
                if (r.row < rows) memcpy(dst, witness + 4 * ((size_t)c * rows + r.row), 32); else memset(dst, 0, 32);
                return KH_OK;
            };
            l.ncells = J.ncell;
            for (int c = 0; c < J.ncell; c++) { l.cols[c] = J.cells[c]; KP(cell(J.cells[c], l.entry[c])); }
            if (J.tid_is_column) KP(cell(J.tid, l.table_id));
            else { const fe id = F.to_mont(fe{{(uint64_t)J.tid, 0, 0, 0}}); memcpy(l.table_id, id.l, 32); }
        } else if ((key & 63) == 7) { r.kind = KH_WITNESS_GATE; r.gate = (int)(detail >> 24 & 15); r.constraints = detail & 0xffffffu; }
        else { r.kind = KH_WITNESS_DISCONNECTED; r.col = (int)(key & 63); r.wired_col = (int)(detail >> 28 & 7); r.wired_row = (size_t)(detail & 0x0fffffffu); }
    }
    *out = r;
    if (lookup_out) *lookup_out = l;
    return KH_OK;
}
int kh_witness_check(kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev, unsigned flags, kh_witness_report_t* out) {
    return witness_check_impl("kh_witness_check", KH_WITNESS_GATES | KH_WITNESS_WIRES, ix, witness, rows, witness_dev, nullptr, false, 0, flags, out, nullptr);
}
int kh_witness_check_full(kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev, const uint64_t* runtime_values, size_t n_runtime,
                          unsigned flags, kh_witness_report_t* out, kh_witness_lookup_t* lookup_out) {
    return witness_check_impl("kh_witness_check_full", KH_WITNESS_GATES | KH_WITNESS_WIRES | KH_WITNESS_LOOKUPS, ix, witness, rows, witness_dev, runtime_values, false,
                              n_runtime, flags, out, lookup_out);
}
int kh_witness_check_full_runtime_dev(kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev, const uint64_t* runtime_values_dev,
                                      size_t n_runtime, unsigned flags, kh_witness_report_t* out, kh_witness_lookup_t* lookup_out) {
    return witness_check_impl("kh_witness_check_full_runtime_dev", KH_WITNESS_GATES | KH_WITNESS_WIRES | KH_WITNESS_LOOKUPS, ix, witness, rows, witness_dev,
                              runtime_values_dev, true, n_runtime, flags, out, lookup_out);
}
int kh_witness_report_message(const kh_witness_report_t* r, char* buf, size_t cap) {
    if (!r || (!buf && cap)) { kh::set_error("kh_witness_report_message: null argument"); return KH_E_INVALID; }
    char line[512];
    int len = 0;
    if (r->kind == KH_WITNESS_OK) len = snprintf(line, sizeof(line), "the witness satisfies the circuit");
    else if (r->kind == KH_WITNESS_DISCONNECTED)
        len = snprintf(line, sizeof(line), "row %zu, column %d is wired to (%zu, %d) but holds a different value (%zu cells disconnected)", r->row, r->col, r->wired_row, r->wired_col,
                       r->cells_disconnected);
    else if (r->kind == KH_WITNESS_GATE) {
        const char* nm = kh_gate_name(r->gate);
        char list[160]; size_t pos = 0; int total;
        list[0] = 0;
        for (int i = 0; i < 32; i++)
            if (r->constraints >> i & 1) { const int k = snprintf(list + pos, sizeof(list) - pos, pos ? ", %d" : "%d", i); if (k > 0 && pos + (size_t)k < sizeof(list)) pos += (size_t)k; }
        total = kh::witness_check_num_constraints(r->gate);
        len = snprintf(line, sizeof(line), "row %zu: gate %s, constraint%s %s of %d %s not zero (%zu rows violated)", r->row, nm ? nm : "?", (r->constraints & (r->constraints - 1)) ? "s" : "",
                       list, total, (r->constraints & (r->constraints - 1)) ? "are" : "is", r->gate_rows_violated);
    } else if (r->kind == KH_WITNESS_LOOKUP) len = snprintf(line, sizeof(line), "row %zu: a looked-up value is in no table (kh_witness_lookup_message names it)", r->row);
    else { kh::set_error("kh_witness_report_message: unknown kind %d", r->kind); return KH_E_INVALID; }
    if (cap) { snprintf(buf, cap, "%s", line); }
    return len;
}
int kh_witness_lookup_message(const kh_witness_report_t* r, const kh_witness_lookup_t* l, char* buf, size_t cap) {
    if (!r || !l || (!buf && cap)) { kh::set_error("kh_witness_lookup_message: null argument"); return KH_E_INVALID; }
    if (r->kind != KH_WITNESS_LOOKUP) return kh_witness_report_message(r, buf, cap);
    if (l->pattern < 0 || l->pattern > 3 || l->slot < 0 || l->slot > 3 || l->ncells < 0 || l->ncells > 3) { kh::set_error("kh_witness_lookup_message: the lookup record names no lookup"); return KH_E_INVALID; }
    // the id as a number: the record does not say which field its limbs belong to, and a table id is small -- the field under which it is below 2^32
    char id[96];
    id[0] = 0;
    for (int fid = 0; fid < 2 && !id[0]; fid++) {
        const fe v = khost::Fld(fid).from_mont(load(l->table_id));
        if (!(v.l[1] | v.l[2] | v.l[3]) && v.l[0] < ((uint64_t)1 << 32)) snprintf(id, sizeof(id), "%llu", (unsigned long long)v.l[0]);
    }
    if (!id[0]) snprintf(id, sizeof(id), "0x%016llx%016llx%016llx%016llx (Montgomery limbs)", (unsigned long long)l->table_id[3], (unsigned long long)l->table_id[2],
                         (unsigned long long)l->table_id[1], (unsigned long long)l->table_id[0]);
    char cols[48]; size_t pos = 0;
    cols[0] = 0;
    for (int c = 0; c < l->ncells; c++) { const int k = snprintf(cols + pos, sizeof(cols) - pos, pos ? ", %d" : "%d", l->cols[c]); if (k > 0 && pos + (size_t)k < sizeof(cols)) pos += (size_t)k; }
    char line[512];
    const int len = snprintf(line, sizeof(line), "row %zu: lookup %d of pattern %s (column%s %s), table id %s: the value is not in the table (%zu lookup%s missing)", r->row, l->slot,
                             PATTERN_NAMES[l->pattern], l->ncells == 1 ? "" : "s", cols, id, l->lookups_missing, l->lookups_missing == 1 ? "" : "s");
    if (cap) { snprintf(buf, cap, "%s", line); }
    return len;
}

size_t kh_prove_randomness_count(const kh_prover_index_t* ix, int witness_on_host) {
    if (!ix) return 0;
    size_t logs = 0; while (((size_t)1 << logs) < ix->size) logs++;
    size_t lookups = ix->lk ? (ix->lk->mpr + 1) * (ix->zk + ix->nch) + ix->zk + ix->nch : 0;   // sorted columns: zk rows + blinders; aggregation: zk rows + blinders
    if (ix->lk && ix->lk->rtsel1) lookups += ix->zk + ix->nch;                               // the runtime table column: zk rows + blinders
    return (witness_on_host ? COLUMNS * ix->zk : 0) + COLUMNS * ix->nch + lookups + 2 + ix->nch + 7 * ix->nch + 2 * logs + 2;
}

int kh_prove(kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev, const uint64_t* randomness, size_t n_random,
             unsigned flags, kh_proof_t** out) {
    return kh_prove_full(ix, witness, rows, witness_dev, randomness, n_random, flags, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, out);
}
int kh_prove_recursive(kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev, const uint64_t* randomness, size_t n_random,
                       unsigned flags, const uint64_t* prev_chals, const unsigned* prev_rounds, const uint64_t* prev_comm_xy, const uint8_t* prev_comm_inf,
                       const size_t* prev_comm_chunks, size_t n_prev, kh_proof_t** out) {
    return kh_prove_full(ix, witness, rows, witness_dev, randomness, n_random, flags, prev_chals, prev_rounds, prev_comm_xy, prev_comm_inf, prev_comm_chunks, n_prev,
                         nullptr, 0, out);
}

// the body of kh_prove_full and kh_prove_full_runtime_dev: runtime_values is host memory, or (runtime_on_device) device memory read in stream order
static int prove_full_impl(kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev, const uint64_t* randomness, size_t n_random,
                           unsigned flags, const uint64_t* prev_chals, const unsigned* prev_rounds, const uint64_t* prev_comm_xy, const uint8_t* prev_comm_inf,
                           const size_t* prev_comm_chunks, size_t n_prev, const uint64_t* runtime_values, bool runtime_on_device, size_t n_runtime, kh_proof_t** out);
int kh_prove_full(kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev, const uint64_t* randomness, size_t n_random,
                  unsigned flags, const uint64_t* prev_chals, const unsigned* prev_rounds, const uint64_t* prev_comm_xy, const uint8_t* prev_comm_inf,
                  const size_t* prev_comm_chunks, size_t n_prev, const uint64_t* runtime_values, size_t n_runtime, kh_proof_t** out) {
    return prove_full_impl(ix, witness, rows, witness_dev, randomness, n_random, flags, prev_chals, prev_rounds, prev_comm_xy, prev_comm_inf, prev_comm_chunks, n_prev,
                           runtime_values, false, n_runtime, out);
}
int kh_prove_full_runtime_dev(kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev, const uint64_t* randomness, size_t n_random,
                              unsigned flags, const uint64_t* prev_chals, const unsigned* prev_rounds, const uint64_t* prev_comm_xy, const uint8_t* prev_comm_inf,
                              const size_t* prev_comm_chunks, size_t n_prev, const uint64_t* runtime_values_dev, size_t n_runtime, kh_proof_t** out) {
    if (((uintptr_t)runtime_values_dev) & 15) { kh::set_error("kh_prove_full_runtime_dev: runtime_values_dev must be 16-byte aligned"); return KH_E_INVALID; }
    return prove_full_impl(ix, witness, rows, witness_dev, randomness, n_random, flags, prev_chals, prev_rounds, prev_comm_xy, prev_comm_inf, prev_comm_chunks, n_prev,
                           runtime_values_dev, true, n_runtime, out);
}
static int prove_full_impl(kh_prover_index_t* ix, const uint64_t* witness, size_t rows, const uint64_t* witness_dev, const uint64_t* randomness, size_t n_random,
                           unsigned flags, const uint64_t* prev_chals, const unsigned* prev_rounds, const uint64_t* prev_comm_xy, const uint8_t* prev_comm_inf,
                           const size_t* prev_comm_chunks, size_t n_prev, const uint64_t* runtime_values, bool runtime_on_device, size_t n_runtime, kh_proof_t** out) {
    if (ix && ((ix->lk && ix->lk->rtsel1) ? (!runtime_values || n_runtime != ix->lk->rt_len) : n_runtime != 0)) {
        kh::set_error("RuntimeTablesInconsistent: the index has %zu runtime table rows, the proof brings %zu", (ix->lk && ix->lk->rtsel1) ? ix->lk->rt_len : (size_t)0, n_runtime);
        return KH_E_INVALID;
    }
    if (!ix || !out || (!witness == !witness_dev)) { kh::set_error("kh_prove: give the witness either on the host or on the device"); return KH_E_INVALID; }
    if (n_prev && (!prev_chals || !prev_rounds || !prev_comm_xy || !prev_comm_inf || !prev_comm_chunks)) { kh::set_error("kh_prove_recursive: null previous-challenge argument"); return KH_E_INVALID; }
    const bool check = flags & KH_PROVE_CHECK, all_gates = flags & KH_PROVE_ALL_GATES;
    static const bool eager_env = kh::env_flag("KH_PROVE_EAGER_CHECK", false);
    const bool eager = check && ((flags & KH_PROVE_EAGER_CHECK) || eager_env);       // fail at the phase the reference fails at (a stream stall per check)
    const int fid = ix->fid, curve = ix->curve;
    const unsigned logn = ix->logn;
    const size_t n = ix->n, size = ix->size, nch = ix->nch, zk = ix->zk, nopt = ix->optional.size();
    kh_srs_t* srs = ix->srs;
    const khost::Fld F(fid);
    const fe one = F.f.one, zero = {{0, 0, 0, 0}};
    struct DeviceRestore { int prev; ~DeviceRestore() { if (prev >= 0) (void)kh_set_device(prev); } } device_restore{kh_get_device()};
    KP(kh_set_device(kh_srs_device(srs)));           // the index lives on the SRS's device: this thread works there until the proof is made
    // a context of this thread's own for the proof (own main stream, pipeline slots, lock): provers on several threads do not queue behind each other
    struct PrivateContext {
        bool mine = false;
        ~PrivateContext() { if (mine) (void)kh_private_context_end(); }
    } private_context;
    if (!(flags & KH_PROVE_SHARED_CONTEXT) && !kh_private_context_active()) {
        KP(kh_private_context_begin()); private_context.mine = true;
        static const bool keep_timers = kh::env_flag("KH_PROVE_TIMERS", false);
        KP(kh_set_phase_timers(keep_timers ? 1 : 0));    // (this context is ours for the call: no per-phase events between the kernels of the proof; a pooled context may come with them on)
    }
    // ---- the randomness of the whole proof, in the reference's draw order
    const size_t need = kh_prove_randomness_count(ix, witness != nullptr);
    std::vector<fe> rnd(need + 64, fe{{0, 0, 0, 0}});   // (slack: a miscounted draw reads zeros, and the count check at the end reports it)
    if (randomness) {
        KP_REQUIRE(n_random == need, "kh_prove: %zu random elements given, %zu drawn (kh_prove_randomness_count)", n_random, need);
        memcpy(rnd.data(), randomness, 32 * need);
    } else KP(os_random(fid, need, rnd.data()));
    size_t rpos = 0;
    auto draw = [&](size_t k) { const fe* p = rnd.data() + rpos; rpos += k; return p; };
    kh_proof* pr = new (std::nothrow) kh_proof();
    if (!pr) { kh::set_error("out of memory"); return KH_E_NOMEM; }
    struct Guard { kh_proof* p; ~Guard() { delete p; } } guard{pr};
    auto t_prev = std::chrono::steady_clock::now();
    int phase_i = 0;
    auto mark = [&]() { auto t = std::chrono::steady_clock::now(); pr->phase[phase_i++] = std::chrono::duration<double>(t - t_prev).count(); t_prev = t; };
    const size_t NB = n, N8 = 8 * n;                 // elements per d1 / d8 column
    // commitments: chunk lists, flat (commitment after commitment)
    auto commit_evals = [&](const uint64_t* ptr, size_t k, std::vector<uint64_t>& xy, std::vector<uint8_t>& inf) -> int {
        // SRS::commit_evaluations_non_hiding of k columns: per chunk of the Lagrange basis one batched MSM over all n evaluations
        xy.assign(8 * k * nch, 0); inf.assign(k * nch, 0);
        std::vector<uint64_t> o(8 * k); std::vector<uint8_t> oi(k);
        for (size_t c = 0; c < nch; c++) {
            int rc = kh_msm_batch_dev(srs, (int)logn, (unsigned)c, 0, ptr, n, k, 1, o.data(), oi.data());
            if (rc) return rc;
            for (size_t i = 0; i < k; i++) { memcpy(&xy[8 * (i * nch + c)], &o[8 * i], 64); inf[i * nch + c] = oi[i]; }
        }
        return KH_OK;
    };
    auto commit_coeffs = [&](const uint64_t* ptr, size_t length, size_t chunks, std::vector<uint64_t>& xy, std::vector<uint8_t>& inf) -> int {
        // SRS::commit_non_hiding (ipa.rs:638-683): chunks of the SRS size, padded with the point at infinity
        size_t cnt = (length + size - 1) / size; if (cnt < chunks) cnt = chunks; if (cnt < 1) cnt = 1;
        xy.assign(8 * cnt, 0); inf.assign(cnt, 1);
        const size_t full = length / size, rem = length - full * size;
        if (full) { int rc = kh_msm_batch_dev(srs, KH_BASIS_G, 0, 0, ptr, size, full, 1, xy.data(), inf.data()); if (rc) return rc; }
        if (rem) { int rc = kh_msm_batch_dev(srs, KH_BASIS_G, 0, 0, ptr + 4 * full * size, rem, 1, 1, &xy[8 * full], &inf[full]); if (rc) return rc; }
        return KH_OK;
    };
    auto mask = [&](const std::vector<uint64_t>& xy, const std::vector<uint8_t>& inf, const fe* blinders, std::vector<uint64_t>& oxy, std::vector<uint8_t>& oinf) -> int {
        const size_t k = inf.size();
        oxy.resize(8 * k); oinf.resize(k);
        return kh_mask_custom(srs, xy.data(), inf.data(), k, (const uint64_t*)blinders, k, oxy.data(), oinf.data());
    };
    // SRS::mask_custom in two halves around a commitment still running on the device: the blinding points [r_j] H first (host, ~5 us each), ...
    auto blinding_points = [&](const fe* blinders, size_t k, std::vector<uint64_t>& bxy, std::vector<uint8_t>& binf) -> int {
        std::vector<uint64_t> none(8 * k, 0); std::vector<uint8_t> at_inf(k, 1);
        bxy.resize(8 * k); binf.resize(k);
        return kh_mask_custom(srs, none.data(), at_inf.data(), k, (const uint64_t*)blinders, k, bxy.data(), binf.data());
    };
    // ... then one addition per commitment once its result is there
    auto mask_with = [&](const std::vector<uint64_t>& xy, const std::vector<uint8_t>& inf, const std::vector<uint64_t>& bxy, const std::vector<uint8_t>& binf,
                         std::vector<uint64_t>& oxy, std::vector<uint8_t>& oinf) -> int {
        const size_t k = inf.size();
        oxy.resize(8 * k); oinf.resize(k);
        return kh_points_add(curve, xy.data(), inf.data(), bxy.data(), binf.data(), k, oxy.data(), oinf.data());
    };
    auto scalar_challenge = [&](kh_sponge_t* sp, fe& o) -> int {
        uint64_t ch[2];
        int rc = kh_sponge_challenge(sp, ch); if (rc) return rc;
        return kh_scalar_challenge_to_field(curve, ch, o.l);
    };
    // ---- witness on the device: [w 0..14 | z] in evaluation form
    Dev ev; KP(ev.alloc(16 * NB));
    struct Ticket {                                   // the un-waited MSM ticket (one at a time): an error on the way out must not leave its pipeline slot taken
        uint64_t t = 0; bool live = false;
        ~Ticket() { if (live) { uint64_t xy[8 * COLUMNS]; uint8_t inf[COLUMNS]; (void)kh_msm_wait(t, xy, inf); } }
        int wait(uint64_t* xy, uint8_t* inf) { live = false; return kh_msm_wait(t, xy, inf); }
    } ticket;
    // The witness arrives over PCIe in 0.6 ms at 2^16 rows (31 MB), and nothing of the proof can start without it -- except the columns' own interpolation and
    // extension, which need one column each.  So the columns travel in groups (KH_PROVE_UPLOAD_GROUPS, default 3; 1 = one transfer as before) and every group but
    // the last has its copy -> iNTT -> LDE queued behind its transfer: that work (2/3 of 0.37 ms) runs underneath the next group's transfer instead of underneath
    // the commitment, the permutation aggregation finds an idle stream ~0.25 ms earlier.  The commitment stays ONE batched MSM behind the last group (submitting
    // it per group was measured in round 4: three submits cost more than the overlap gave back).
    Dev cf; KP(cf.alloc(16 * NB));                    // coefficient forms [w | z]
    Dev e8; KP(e8.alloc(16 * N8));
    const bool any_lib = (ix->live != 0) || nopt > 0;
    const size_t w8 = (!any_lib && !all_gates) ? PERMUTS : COLUMNS;     // generic + permutation read w0..w6 only
    // The witness extension (0.35 ms of throughput work) goes right behind the interpolation: it then runs underneath the transfer / the witness commitment, and the
    // small kernels of the permutation aggregation queue behind it.
    auto interpolate_extend = [&](size_t c0, size_t c1) -> int {       // columns c0 .. c1-1: evaluations -> coefficients -> d8
        if (c1 <= c0) return KH_OK;
        int rc_ = kh_dev_copy(cf.at(c0 * NB), ev.at(c0 * NB), (c1 - c0) * NB * 32); if (rc_) return rc_;
        rc_ = kh_ntt_dev(fid, cf.at(c0 * NB), logn, 1, c1 - c0); if (rc_) return rc_;
        const size_t e1 = c1 < w8 ? c1 : w8;
        if (e1 > c0) rc_ = kh_lde_dev(fid, cf.at(c0 * NB), logn, 3, e8.at(c0 * N8), e1 - c0);
        return rc_;
    };
    size_t cols_pending = 0;                           // first column whose interpolation / extension is not queued yet
    if (witness) {
        KP_REQUIRE(rows + zk <= n, "NoRoomForZkInWitness: %zu rows + %zu zero-knowledge rows > %zu", rows, zk, n);
        if (rows + zk < n) KP(kh_dev_memset_zero(ev.p, 16 * NB * 32));
        const fe* z = draw(COLUMNS * zk);            // per column, from the LAST row backwards (prover.rs:254-266)
        std::vector<fe> zkr(COLUMNS * zk);
        for (size_t c = 0; c < COLUMNS; c++) for (size_t j = 0; j < zk; j++) zkr[c * zk + j] = z[c * zk + (zk - 1 - j)];
        KP(kh_dev_upload_2d(ev.at(n - zk), NB * 32, zkr.data(), zk * 32, zk * 32, COLUMNS));
        static const size_t groups_env = (size_t)kh::env_int("KH_PROVE_UPLOAD_GROUPS", 3);
        const size_t groups = (rows == 0 || groups_env < 1 || nch != 1 || n < 4096) ? 1 : (groups_env > COLUMNS ? COLUMNS : groups_env);
        for (size_t g = 0; g < groups && rows; g++) {
            const size_t c0 = COLUMNS * g / groups, c1 = COLUMNS * (g + 1) / groups;
            // (the destination rows are touched by nothing that is queued: no wait for the main stream, which holds the previous group's transforms)
            if (groups > 1) KP(kh_dev_upload_2d_unordered(ev.at(c0 * NB), NB * 32, witness + 4 * c0 * rows, rows * 32, rows * 32, c1 - c0));
            else KP(kh_dev_upload_2d(ev.p, NB * 32, witness, rows * 32, rows * 32, COLUMNS));
            if (g + 1 < groups) { KP(interpolate_extend(c0, c1)); cols_pending = c1; }
        }
    } else KP(kh_dev_copy(ev.p, witness_dev, COLUMNS * NB * 32));
    mark();
    SpongeH fq; KP(kh_sponge_new(KH_SPONGE_FQ, curve, &fq.s));
    KP(kh_sponge_absorb(fq.s, ix->digest.l, 1));
    {                                                 // prover.rs:276-279: the previous proofs' accumulator commitments
        size_t pos = 0;
        for (size_t j = 0; j < n_prev; j++) { KP(kh_sponge_absorb_g(fq.s, prev_comm_xy + 8 * pos, prev_comm_inf + pos, prev_comm_chunks[j])); pos += prev_comm_chunks[j]; }
    }
    Dev pub_c;
    std::vector<uint64_t> pub_xy; std::vector<uint8_t> pub_inf;
    if (ix->pub) {                                    // the negated public-input polynomial (prover.rs:281-309)
        KP_REQUIRE(ix->pub <= n, "more public inputs than rows");
        std::vector<fe> pe(n, zero);
        KP(kh_dev_download(pe.data(), ev.p, ix->pub * 32));
        for (size_t i = 0; i < ix->pub; i++) pe[i] = F.neg(pe[i]);
        KP(pub_c.alloc(NB)); KP(kh_dev_upload(pub_c.p, pe.data(), NB * 32));
        std::vector<uint64_t> cxy; std::vector<uint8_t> cinf;
        KP(commit_evals(pub_c.p, 1, cxy, cinf));
        std::vector<fe> ones(nch, one);
        KP(mask(cxy, cinf, ones.data(), pub_xy, pub_inf));
        KP(kh_ntt_dev(fid, pub_c.p, logn, 1, 1));
    } else { pub_xy = ix->zsel_xy; pub_inf = ix->zsel_inf; }
    KP(kh_sponge_absorb_g(fq.s, pub_xy.data(), pub_inf.data(), nch));
    pr->set_points(KH_PROOF_PUBLIC_COMM, pub_xy.data(), pub_inf.data(), nch);
    // ---- the proof's invariants (the accumulators end at 1, the divisions leave no remainder) are queued as device-side checks behind the steps that
    // produce them (kh_check_equal_dev: one bit each in a word on the device) and read ONCE, after the opening: a synchronous download per check
    // stalled the stream five times per proof, and the small host <-> device patches below (a one, two random rows, z_0 - 1) four times more.
    Dev chk; KP(chk.alloc(4));                         // [0]: the flags word; [1], [2]: the remainders of the two boundary divisions
    KP(kh_dev_memset_zero(chk.p, 4 * 32));
    uint32_t* const chk_flags = (uint32_t*)chk.p;
    enum { CHK_AGG = 0, CHK_Z = 1, CHK_REM = 2, CHK_BND = 3 };
    static const char* const chk_msg[4] = {"final value of the lookup aggregation is not 1 (lookup/constraints.rs:325-331)",
                                           "final value of the permutation accumulator is not 1 (permutation.rs:566-568)",
                                           "rest of division by vanishing polynomial (prover.rs:913-917): the witness does not satisfy the constraints",
                                           "permutation boundary division rest (permutation.rs:301-321)"};
    auto eager_check = [&](unsigned bit) -> int {      // KH_PROVE_EAGER_CHECK: the check queued just now, read back on the spot
        if (!eager) return KH_OK;
        uint32_t fl = 0;
        int rc_ = kh_dev_download(&fl, chk.p, 4); if (rc_) return rc_;
        if (fl & (1u << bit)) { kh::set_error("%s", chk_msg[bit]); return KH_E_INVALID; }
        return KH_OK;
    };
    auto set_const = [&](uint64_t* dst, const fe& val) { return kh_dev_fill_elements(dst, val.l, 1); };    // *dst = val, queued on the main stream
    // ---- witness commitments: one batched MSM per chunk of the Lagrange basis, queued before the columns are interpolated
    uint64_t& tk = ticket.t; bool& have_tk = ticket.live;
    if (nch == 1) { KP(kh_msm_submit(srs, (int)logn, 0, 0, ev.p, n, COLUMNS, 1, &tk)); have_tk = true; }
    KP(interpolate_extend(cols_pending, COLUMNS));
    std::vector<uint64_t> wxy, wbx; std::vector<uint8_t> winf, wbi;
    const fe* w_blind = draw(COLUMNS * nch);          // blinder(num_chunks) per column, column by column (prover.rs:316-327)
    KP(blinding_points(w_blind, COLUMNS * nch, wbx, wbi));              // (underneath the MSM)
    if (have_tk) { wxy.resize(8 * COLUMNS); winf.resize(COLUMNS); KP(ticket.wait(wxy.data(), winf.data())); }
    else KP(commit_evals(ev.p, COLUMNS, wxy, winf));
    std::vector<uint64_t> wcx; std::vector<uint8_t> wci;
    KP(mask_with(wxy, winf, wbx, wbi, wcx, wci));
    KP(kh_sponge_absorb_g(fq.s, wcx.data(), wci.data(), COLUMNS * nch));
    pr->set_points(KH_PROOF_W_COMM, wcx.data(), wci.data(), COLUMNS * nch);
    // ---- lookup argument, part 1 (prover.rs:383-633): joint combiner, combined table, sorted columns
    const kh_lookup_index* lk = ix->lk;
    const size_t ns = lk ? lk->mpr + 1 : 0, npat = lk ? lk->pats.size() : 0, lookup_rows = n - zk - 1;
    fe jc = zero, tic_t = zero, tic_c = zero;
    Dev d_table, d_sorted;
    const fe* s_blind = nullptr;
    Dev d_rt, d_rtc, rt8;                             // the proof's runtime contribution to the table's second column: d1, coefficients, d8
    const fe* rt_blind = nullptr;
    const bool has_rt = lk && lk->rtsel1;
    if (has_rt) {                                     // prover.rs:397-470: placed at the runtime rows, zero-knowledge rows drawn from the last row backwards, committed hiding
        const fe* z = draw(zk);
        KP(d_rt.alloc(NB)); KP(d_rtc.alloc(NB));
        if (runtime_on_device) {                      // the same column assembled on the device, in stream order: nothing waits for the values' producer
            KP(kh_dev_memset_zero(d_rt.p, NB * 32));
            KP(kh_dev_copy(d_rt.at(lk->rt_offset), runtime_values, n_runtime * 32));
            for (size_t j = 0; j < zk; j++) KP(set_const(d_rt.at(n - zk + j), z[zk - 1 - j]));
        } else {
            std::vector<fe> rte(n, zero);
            memcpy(&rte[lk->rt_offset], runtime_values, n_runtime * 32);
            for (size_t j = 0; j < zk; j++) rte[n - zk + j] = z[zk - 1 - j];
            KP(kh_dev_upload(d_rt.p, rte.data(), NB * 32));
        }
        KP(kh_dev_copy(d_rtc.p, d_rt.p, NB * 32));
        KP(kh_ntt_dev(fid, d_rtc.p, logn, 1, 1));
        std::vector<uint64_t> rxy, rcx; std::vector<uint8_t> rinf, rci;
        KP(commit_coeffs(d_rtc.p, n, nch, rxy, rinf));
        KP_REQUIRE(rinf.size() == nch, "unexpected chunk count of the runtime table");
        rt_blind = draw(nch);
        KP(mask(rxy, rinf, rt_blind, rcx, rci));
        KP(kh_sponge_absorb_g(fq.s, rcx.data(), rci.data(), nch));
        pr->set_points(KH_PROOF_LOOKUP_RUNTIME_COMM, rcx.data(), rci.data(), nch);
    }
    if (lk) {
        uint64_t chal[2] = {0, 0};
        if (lk->mjs > 1) KP(kh_sponge_challenge(fq.s, chal));       // joint_lookup_used (lookups.rs:90-110)
        KP(kh_scalar_challenge_to_field(curve, chal, jc.l));
        tic_c = fpow(F, jc, lk->mjs);                               // the constraints' table-id combiner (constraints.rs:424-440)
        tic_t = lk->tids ? tic_c : zero;                            // ... the table's, when the index has a table-id column (prover.rs:500-572)
        const size_t ntc = lk->tcols.size();
        {                                                           // the combined table: Horner over the table columns + tic * ids
            Prog p;
            const uint32_t c_rt = (uint32_t)(ntc + (lk->tids ? 1 : 0));               // the runtime column goes to the table's second column (prover.rs:455-464)
            auto col = [&](size_t k) { p.cell((uint32_t)k); if (k == 1 && has_rt) { p.cell(c_rt); p.add(); } };
            col(ntc - 1);
            for (size_t k = ntc - 1; k-- > 0;) { p.C(jc); p.mul(); col(k); p.add(); }
            std::vector<const uint64_t*> cols(lk->tcols);
            if (lk->tids) { p.C(tic_t); p.cell((uint32_t)ntc); p.mul(); p.add(); cols.push_back(lk->tids); }
            if (has_rt) cols.push_back(d_rt.p);
            std::vector<size_t> lens(cols.size(), n);
            KP(d_table.alloc(NB));
            KP(p.run(fid, cols, lens, n, 1, 1, 0, d_table.p));
        }
        KP(d_sorted.alloc(ns * NB));
        {                                                           // the looked-up joint values, one column per lookup slot (0 = the dummy entry's value)
            Dev d_vals; KP(d_vals.alloc(lk->mpr * NB));
            LookupChallenges ch{}; ch.jc = jc; ch.tic = tic_t;
            std::vector<const uint64_t*> cols;
            for (size_t i = 0; i < COLUMNS; i++) cols.push_back(ev.at(i * NB));
            for (size_t k = 0; k < npat; k++) cols.push_back(lk->sel1[k]);
            std::vector<size_t> lens(cols.size(), n);
            for (size_t sl = 0; sl < lk->mpr; sl++) {
                Prog p; bool first = true;
                for (size_t k = 0; k < npat; k++) {
                    const Pattern& P = PATTERNS[lk->pats[k]];
                    if (sl >= (size_t)P.n) continue;
                    emit_joint(p, F, P.l[sl], ch); p.cell((uint32_t)(COLUMNS + k)); p.mul();
                    if (!first) p.add();
                    first = false;
                }
                KP(p.run(fid, cols, lens, n, 1, 1, 0, d_vals.at(sl * NB)));
            }
            // the sorted columns (constraints.rs:90-194) on the device: hash join + snake layout straight into rows 0 .. n - zk - 1 of the padded columns;
            // values and table stay on the card, the one wait is the join's status word (a value that is not in the table fails here, with its row)
            size_t bad = 0;
            KP(kh_lookup_sorted_dev(d_table.p, lookup_rows, d_vals.p, n, lk->mpr, d_sorted.p, n, &bad));
        }
        {                                                           // zk_patch (constraints.rs:35-48): the last zk_rows random, column by column
            std::vector<fe> zkr(ns * zk);
            for (size_t k = 0; k < ns; k++) memcpy(&zkr[k * zk], draw(zk), zk * 32);
            KP(kh_dev_upload_2d(d_sorted.at(n - zk), NB * 32, zkr.data(), zk * 32, zk * 32, ns));
        }
        std::vector<uint64_t> sxy, scx; std::vector<uint8_t> sinf, sci;
        KP(commit_evals(d_sorted.p, ns, sxy, sinf));
        s_blind = draw(ns * nch);
        KP(mask(sxy, sinf, s_blind, scx, sci));
        KP(kh_sponge_absorb_g(fq.s, scx.data(), sci.data(), ns * nch));
        pr->set_points(KH_PROOF_LOOKUP_SORTED_COMM, scx.data(), sci.data(), ns * nch);
    }
    mark();
    fe beta, gamma;
    KP(kh_sponge_challenge_field(fq.s, beta.l)); KP(kh_sponge_challenge_field(fq.s, gamma.l));
    // ---- lookup argument, part 2 (prover.rs:635-673; constraints.rs:233-338): the aggregation, committed before z
    Dev d_agg;
    const fe* a_blind = nullptr;
    LookupChallenges lch{};
    if (lk) {
        const size_t mpr = lk->mpr;
        lch.jc = jc; lch.tic = tic_t; lch.beta = beta; lch.gamma = gamma; lch.gb1 = F.mul(gamma, F.add(one, beta));
        const fe b1m = fpow(F, F.add(one, beta), mpr);
        fe gp = one;
        for (size_t k = 0; k <= mpr; k++) { lch.prefactor[k] = F.mul(gp, b1m); gp = F.mul(gp, gamma); }     // the dummy entry's value is 0
        // columns: witness 0..14 | sorted 15..15+mpr | combined table | pattern selectors
        std::vector<const uint64_t*> cols;
        for (size_t i = 0; i < COLUMNS; i++) cols.push_back(ev.at(i * NB));
        for (size_t k = 0; k < ns; k++) cols.push_back(d_sorted.at(k * NB));
        const uint32_t c_table = (uint32_t)cols.size(); cols.push_back(d_table.p);
        const uint32_t c_sel0 = (uint32_t)cols.size();
        for (size_t k = 0; k < npat; k++) cols.push_back(lk->sel1[k]);
        std::vector<size_t> lens(cols.size(), n);
        Prog pn, pd;
        emit_numerator(pn, F, lk->pats, mpr, lch, c_sel0, c_table);
        emit_denominator(pd, mpr, lch, (uint32_t)COLUMNS);
        Dev num, den; KP(num.alloc(NB)); KP(den.alloc(NB)); KP(d_agg.alloc(NB));
        KP(kh_dev_memset_zero(num.p, NB * 32)); KP(kh_dev_memset_zero(den.p, NB * 32));
        KP(pn.run(fid, cols, lens, lookup_rows, 1, 1, 0, num.at(1)));
        KP(pd.run(fid, cols, lens, lookup_rows, 1, 1, 0, den.at(1)));
        KP(kh_batch_inversion_dev(fid, den.at(1), lookup_rows));
        KP(set_const(num.p, one)); KP(set_const(den.p, one));
        const uint32_t prod[6] = {KH_TOK_CELL, 0, KH_TOK_CELL, 2, KH_TOK_MUL, 0};
        const uint64_t* pc[2] = {num.p, den.p}; const size_t pl[2] = {n, n};
        KP(kh_expr_evaluations_dev(fid, prod, 3, pc, pl, 2, one.l, 1, n, 1, 1, 0, d_agg.p));
        KP(kh_field_scan_dev(fid, KH_SCAN_MUL, 0, d_agg.p, lookup_rows + 1));
        if (check) { KP(kh_check_equal_dev(d_agg.at(lookup_rows), 1, one.l, chk_flags, CHK_AGG)); KP(eager_check(CHK_AGG)); }      // before the random rows overwrite anything: row lookup_rows = n - zk - 1 is not one of them
        { const fe* rr = draw(zk); for (size_t j = 0; j < zk; j++) KP(set_const(d_agg.at(n - zk + j), rr[j])); }
        a_blind = draw(nch);
        std::vector<uint64_t> axy, acx; std::vector<uint8_t> ainf, aci;
        KP(commit_evals(d_agg.p, 1, axy, ainf));
        KP(mask(axy, ainf, a_blind, acx, aci));
        KP(kh_sponge_absorb_g(fq.s, acx.data(), aci.data(), nch));
        pr->set_points(KH_PROOF_LOOKUP_AGGREG_COMM, acx.data(), aci.data(), nch);
        KP(kh_sync());                                              // num / den are released at the end of this block
    }
    // ---- permutation aggregation z: numerators / denominators, batch inversion, running product (permutation.rs:510-568)
    fe bshift[7];
    for (int i = 0; i < 7; i++) bshift[i] = F.mul(beta, ix->shifts[i]);
    uint64_t* zcol = ev.at(COLUMNS * NB);
    Dev num, den; KP(num.alloc(NB)); KP(den.alloc(NB));
    {
        const uint64_t* cols[15]; size_t lens[15];
        for (size_t i = 0; i < PERMUTS; i++) { cols[i] = ev.at(i * NB); cols[PERMUTS + i] = ix->col1(COLUMNS + 2 + i); }
        cols[14] = ix->col1(COLUMNS + 1);
        for (int i = 0; i < 15; i++) lens[i] = n;
        fe consts[9]; consts[0] = gamma; consts[1] = beta; for (int i = 0; i < 7; i++) consts[2 + i] = bshift[i];
        std::vector<uint32_t> nt, dt;
        auto tok = [](std::vector<uint32_t>& v, uint32_t op, uint32_t a) { v.push_back(op); v.push_back(a); };
        for (uint32_t i = 0; i < 7; i++) {            // prod_i (w_i + sid beta shift_i + gamma), prod_i (w_i + sigma_i beta + gamma)
            tok(nt, KH_TOK_CELL, 2 * i); tok(nt, KH_TOK_CELL, 2 * 14); tok(nt, KH_TOK_CONST, 2 + i); tok(nt, KH_TOK_MUL, 0); tok(nt, KH_TOK_ADD, 0);
            tok(nt, KH_TOK_CONST, 0); tok(nt, KH_TOK_ADD, 0); if (i) tok(nt, KH_TOK_MUL, 0);
            tok(dt, KH_TOK_CELL, 2 * i); tok(dt, KH_TOK_CELL, 2 * (7 + i)); tok(dt, KH_TOK_CONST, 1); tok(dt, KH_TOK_MUL, 0); tok(dt, KH_TOK_ADD, 0);
            tok(dt, KH_TOK_CONST, 0); tok(dt, KH_TOK_ADD, 0); if (i) tok(dt, KH_TOK_MUL, 0);
        }
        // z_0 = 1, z_(i+1) = z_i num_i / den_i: the quotients of rows 0 .. n-2 go to z's rows 1 .. n-1 and the running product does the rest
        KP(kh_expr_evaluations_dev(fid, nt.data(), nt.size() / 2, cols, lens, 15, (const uint64_t*)consts, 9, n - 1, 1, 8, 0, num.p));
        KP(kh_expr_evaluations_dev(fid, dt.data(), dt.size() / 2, cols, lens, 15, (const uint64_t*)consts, 9, n - 1, 1, 8, 0, den.p));
        KP(kh_batch_inversion_dev(fid, den.p, n - 1));
        const uint32_t prod[6] = {KH_TOK_CELL, 0, KH_TOK_CELL, 2, KH_TOK_MUL, 0};
        const uint64_t* pc[2] = {num.p, den.p}; const size_t pl[2] = {n - 1, n - 1};
        KP(set_const(zcol, one));
        KP(kh_expr_evaluations_dev(fid, prod, 3, pc, pl, 2, one.l, 1, n - 1, 1, 8, 0, zcol + 4));
        KP(kh_field_scan_dev(fid, KH_SCAN_MUL, 0, zcol, n - zk + 1));
        if (check) { KP(kh_check_equal_dev(zcol + 4 * (n - zk), 1, one.l, chk_flags, CHK_Z)); KP(eager_check(CHK_Z)); }
        { const fe* rr = draw(2); KP(set_const(zcol + 4 * (n - zk + 1), rr[0])); KP(set_const(zcol + 4 * (n - zk + 2), rr[1])); }   // z's two random rows, in that order
        if (zk > 3) KP(kh_field_scan_dev(fid, KH_SCAN_MUL, 0, zcol + 4 * (n - zk + 2), zk - 2));
    }
    uint64_t* zc = cf.at(COLUMNS * NB);
    KP(kh_dev_copy(zc, zcol, NB * 32));
    KP(kh_ntt_dev(fid, zc, logn, 1, 1));
    if (nch == 1 && size == n) { KP(kh_msm_submit(srs, KH_BASIS_G, 0, 0, zc, n, 1, 1, &tk)); have_tk = true; }   // ... while z is extended to d8
    KP(kh_lde_dev(fid, zc, logn, 3, e8.at(COLUMNS * N8), 1));
    std::vector<uint64_t> zxy, zbx; std::vector<uint8_t> zinf, zbi;
    const fe* z_blind = draw(nch);
    KP(blinding_points(z_blind, nch, zbx, zbi));
    if (have_tk) { zxy.resize(8); zinf.resize(1); KP(ticket.wait(zxy.data(), zinf.data())); }
    else KP(commit_coeffs(zc, n, nch, zxy, zinf));
    const size_t nzb = zinf.size();
    KP_REQUIRE(nzb == nch, "unexpected chunk count of z");
    std::vector<uint64_t> zcx; std::vector<uint8_t> zci;
    KP(mask_with(zxy, zinf, zbx, zbi, zcx, zci));
    KP(kh_sponge_absorb_g(fq.s, zcx.data(), zci.data(), nzb));
    pr->set_points(KH_PROOF_Z_COMM, zcx.data(), zci.data(), nzb);
    mark();
    fe alpha; KP(scalar_challenge(fq.s, alpha));
    fe alphas[3]; alphas[0] = fpow(F, alpha, ALPHA_PERM0); alphas[1] = F.mul(alphas[0], alpha); alphas[2] = F.mul(alphas[1], alpha);
    // ---- constraint rows on d8, quotient (prover.rs:794-917)
    Dev t8; KP(t8.alloc(N8));                         // the constraint rows on d8 (the reference keeps the generic gate's on d4: same polynomial, see below)
    {
        const uint64_t* cols[31];
        std::vector<uint64_t> consts(4 * 64);
        for (size_t i = 0; i < COLUMNS; i++) { cols[i] = e8.at(i * N8); cols[COLUMNS + i] = ix->col8(i); }
        cols[30] = ix->col8(COLUMNS);
        fe gp[2] = {one, alpha};
        const uint64_t* pc[31];
        for (size_t i = 0; i < COLUMNS; i++) pc[i] = e8.at(i * N8);
        for (size_t i = 0; i < PERMUTS; i++) pc[COLUMNS + i] = ix->col8(COLUMNS + 2 + i);
        pc[22] = e8.at(COLUMNS * N8); pc[23] = ix->col8(ix->ncol); pc[24] = ix->col8(ix->ncol + 1);
        for (int i = 25; i < 31; i++) pc[i] = pc[0];
        fe pp[10]; pp[0] = gamma; pp[1] = beta; pp[2] = alphas[0]; for (int i = 0; i < 7; i++) pp[3 + i] = bshift[i];
        KP(kh_gate_constants(fid, ix->gid_perm, nullptr, nullptr, (const uint64_t*)pp, 10, consts.data()));
        KP(kh_gate_evaluations_dev(fid, ix->gid_perm, pc, N8, consts.data(), (size_t)kh_gate_num_constants(ix->gid_perm), N8, 1, 8, 0, t8.p));
        // the double generic gate on ALL of d8, accumulated onto the permutation rows: the reference evaluates it on d4 and interpolates separately
        // (prover.rs:794-822, t4); its degree is below 4n, so the 8n-point interpolation of the sum gives the same polynomial -- the 4n-point iNTT and
        // the t4 buffer go away, and the kernel, memory-bound on whole cache lines either way, reads the same lines it read with stride 2
        KP(kh_gate_constants(fid, ix->gid_generic, nullptr, nullptr, (const uint64_t*)gp, 2, consts.data()));
        KP(kh_gate_evaluations_dev(fid, ix->gid_generic, cols, N8, consts.data(), (size_t)kh_gate_num_constants(ix->gid_generic), N8, 1, 8, 1, t8.p));
        for (size_t k = 0; k < 5 + nopt; k++) {      // the gate library on d8 (prover.rs:824-868): index(gate) * sum_i alpha^i constraint_i
            const bool live = k < 5 ? (((ix->live >> k) & 1u) || all_gates) : true;
            if (!live) continue;
            const int gid = k < 5 ? ix->lib_gate[k] : ix->optional[k - 5];
            const int nc = kh_gate_num_constants(gid);
            KP_REQUIRE(nc >= 0 && nc <= 64, "constants table of gate %d too large", gid);
            KP(kh_gate_constants(fid, gid, alpha.l, ix->endo.l, nullptr, 0, consts.data()));
            cols[30] = ix->col8(SEL0 + k);
            KP(kh_gate_evaluations_dev(fid, gid, cols, N8, consts.data(), (size_t)nc, N8, 1, 8, 1, t8.p));
        }
    }
    Dev lkc, lk8;                                      // coefficient forms / d8 of [sorted ... | aggregation | combined table]
    const size_t nl = lk ? ns + 2 : 0;
    if (lk) {                                         // the lookup constraints on d8 (prover.rs:874-903), powers alpha^24 ...
        const size_t mpr = lk->mpr;
        KP(lkc.alloc(nl * NB)); KP(lk8.alloc(nl * N8));
        KP(kh_dev_copy(lkc.p, d_sorted.p, ns * NB * 32));
        KP(kh_dev_copy(lkc.at(ns * NB), d_agg.p, NB * 32));
        KP(kh_dev_copy(lkc.at((ns + 1) * NB), d_table.p, NB * 32));
        KP(kh_ntt_dev(fid, lkc.p, logn, 1, nl));
        KP(kh_lde_dev(fid, lkc.p, logn, 3, lk8.p, nl));
        LookupChallenges cch = lch; cch.tic = tic_c;
        // columns: witness 0..14 | sorted | aggregation | table | pattern selectors | vanish, l0, lfinal (expr.rs:883-893)
        std::vector<const uint64_t*> cols;
        for (size_t i = 0; i < COLUMNS; i++) cols.push_back(e8.at(i * N8));
        for (size_t k = 0; k < nl; k++) cols.push_back(lk8.at(k * N8));
        const uint32_t c_sorted = (uint32_t)COLUMNS, c_agg = (uint32_t)(COLUMNS + ns), c_table = c_agg + 1, c_sel0 = c_table + 1;
        for (size_t k = 0; k < npat; k++) cols.push_back(lk->sel8[k]);
        const uint32_t c_vanish = (uint32_t)cols.size(), c_l0 = c_vanish + 1, c_lfinal = c_vanish + 2;
        for (int a = 0; a < 3; a++) cols.push_back(lk->atoms8[a]);
        std::vector<size_t> lens(cols.size(), N8);
        LookupColumns lc{c_sorted, c_agg, c_table, c_sel0, c_vanish, c_l0, c_lfinal, 0, 0};
        if (has_rt) {
            KP(rt8.alloc(N8)); KP(kh_lde_dev(fid, d_rtc.p, logn, 3, rt8.p, 1));
            lc.rt = (uint32_t)cols.size(); lc.rtsel = lc.rt + 1; cols.push_back(rt8.p); cols.push_back(lk->rtsel8);
            lens.assign(cols.size(), N8);
        }
        Prog p;
        emit_lookup_constraints(p, F, lk->pats, mpr, cch, alpha, lc, has_rt);
        KP(p.run(fid, cols, lens, N8, 1, 8, 1, t8.p));
    }
    KP(kh_ntt_dev(fid, t8.p, logn + 3, 1, 1));
    if (pub_c.p) {                                    // f = t + public (prover.rs:906-908)
        const uint64_t* ps[2] = {t8.p, pub_c.p}; const size_t ls[2] = {8 * n, n};
        fe sc[2] = {one, one};
        KP(kh_poly_lincomb_dev(fid, ps, ls, (const uint64_t*)sc, 2, t8.p, 8 * n));
    }
    Dev quot, rem; KP(quot.alloc(7 * NB)); KP(rem.alloc(NB));
    KP(kh_divide_by_vanishing_poly_dev(fid, t8.p, 8 * n, logn, quot.p, rem.p));
    if (check) { KP(kh_check_equal_dev(rem.p, n, nullptr, chk_flags, CHK_REM)); KP(eager_check(CHK_REM)); }
    Dev zm1, b1, b2; KP(zm1.alloc(NB)); KP(b1.alloc(NB)); KP(b2.alloc(NB));
    {
        const uint64_t* ps[1] = {zc}; const size_t ls[1] = {n};
        KP(kh_poly_lincomb_dev(fid, ps, ls, one.l, 1, zm1.p, n));
        {   // z_0 - 1, in place, on the stream
            const uint32_t prog[6] = {KH_TOK_CELL, 0, KH_TOK_CONST, 0, KH_TOK_SUB, 0};
            const uint64_t* c0[1] = {zm1.p}; const size_t l0[1] = {n};
            KP(kh_expr_evaluations_dev(fid, prog, 3, c0, l0, 1, one.l, 1, 1, 1, 0, 0, zm1.p));
        }
        KP(kh_dev_memset_zero(b1.p, NB * 32)); KP(kh_dev_memset_zero(b2.p, NB * 32));
        const fe pts2[2] = {one, fpow(F, ix->omega, n - zk)};
        uint64_t* dst[2] = {b1.p, b2.p};
        for (int i = 0; i < 2; i++) {                 // (z - 1) / (x - 1), (z - 1) / (x - omega^(n - zk)) (permutation.rs:301-321)
            KP(kh_divide_by_linear_async_dev(fid, zm1.p, n, pts2[i].l, dst[i], chk.at(1 + i)));
            if (check) { KP(kh_check_equal_dev(chk.at(1 + i), 1, nullptr, chk_flags, CHK_BND)); KP(eager_check(CHK_BND)); }
        }
        const uint64_t* qs[3] = {quot.p, b1.p, b2.p}; const size_t ql[3] = {7 * n, n - 1, n - 1};
        fe sc[3] = {one, alphas[1], alphas[2]};
        KP(kh_poly_lincomb_dev(fid, qs, ql, (const uint64_t*)sc, 3, quot.p, 7 * n));
    }
    std::vector<uint64_t> txy, tbx; std::vector<uint8_t> tinf, tbi;
    if (nch == 1 && size == n) { KP(kh_msm_submit(srs, KH_BASIS_G, 0, 0, quot.p, n, 7, 1, &tk)); have_tk = true; }   // the seven chunks as one batch
    const size_t ntb = 7 * nch;
    const fe* t_blind = draw(ntb);
    KP(blinding_points(t_blind, ntb, tbx, tbi));
    if (have_tk) { txy.resize(8 * 7); tinf.resize(7); KP(ticket.wait(txy.data(), tinf.data())); }
    else KP(commit_coeffs(quot.p, 7 * n, 7 * nch, txy, tinf));
    KP_REQUIRE(tinf.size() == ntb, "unexpected chunk count of t");
    std::vector<uint64_t> tcx; std::vector<uint8_t> tci;
    KP(mask_with(txy, tinf, tbx, tbi, tcx, tci));
    KP(kh_sponge_absorb_g(fq.s, tcx.data(), tci.data(), ntb));
    pr->set_points(KH_PROOF_T_COMM, tcx.data(), tci.data(), ntb);
    mark();
    fe zeta; KP(scalar_challenge(fq.s, zeta));
    const fe zetaw = F.mul(zeta, ix->omega);
    SpongeH fq_before; KP(kh_sponge_clone(fq.s, &fq_before.s));
    // ---- chunked evaluations at zeta, zeta omega (prover.rs:989-1004)
    std::vector<const uint64_t*> polys;
    polys.push_back(zc); polys.push_back(ix->colc(COLUMNS));
    for (size_t k = 0; k < 5; k++) polys.push_back(ix->colc(SEL0 + k));
    for (size_t i = 0; i < COLUMNS; i++) polys.push_back(cf.at(i * NB));
    for (size_t i = 0; i < COLUMNS; i++) polys.push_back(ix->colc(i));
    for (size_t i = 0; i + 1 < PERMUTS; i++) polys.push_back(ix->colc(COLUMNS + 2 + i));
    for (size_t k = 0; k < nopt; k++) polys.push_back(ix->colc(OPT0 + k));
    const size_t L0 = polys.size();                   // opening order of the lookup polynomials (prover.rs:1368-1420): sorted ..., aggregation, table, selectors
    for (size_t k = 0; k < nl; k++) polys.push_back(lkc.at(k * NB));
    const size_t nrt = has_rt ? 2 : 0;                // ... combined table, runtime table, runtime selector, pattern selectors
    if (has_rt) { polys.push_back(d_rtc.p); polys.push_back(lk->rtselc); }
    for (size_t k = 0; k < npat; k++) polys.push_back(lk->selc[k]);
    const size_t npoly = polys.size();
    const fe pts[2] = {zeta, zetaw};
    std::vector<fe> E(npoly * 2 * nch);               // polynomial j: E[(2 j + p) nch + c]
    // The same launch evaluates the chunks of sigma_6 and of the quotient t at both points: ft = perm_scalar sigma_6 - (zeta^n - 1) t is linear in
    // them, so ft(zeta), ft(zeta omega) -- the Fr-sponge absorbs the latter FIRST -- are known without a second launch + download behind the host's
    // computation of perm_scalar (round 5: ~0.1 ms of idle GPU between the two evaluation launches).
    std::vector<fe> E_ft(2 * 8 * nch);               // sigma_6: [p][c], c < nch; then t: [p][c], c < 7 nch
    std::vector<fe> pub_eval(2 * nch, zero);
    const uint64_t* const sig6_c = ix->colc(COLUMNS + 2 + PERMUTS - 1);
    {
        std::vector<const uint64_t*> ev(polys); ev.push_back(sig6_c); ev.push_back(quot.at(0));
        std::vector<size_t> lens(npoly, n), chs(npoly, nch);
        lens.push_back(n); chs.push_back(nch);
        lens.push_back(7 * n); chs.push_back(7 * nch);
        if (pub_c.p) { ev.push_back(pub_c.p); lens.push_back(n); chs.push_back(nch); }      // ... and the public-input polynomial's, when there is one
        std::vector<fe> all(E.size() + E_ft.size() + (pub_c.p ? 2 * nch : 0));
        KP(kh_evaluate_chunks_batch_dev(fid, ev.data(), lens.data(), chs.data(), ev.size(), size, (const uint64_t*)pts, 2, (uint64_t*)all.data()));
        std::copy(all.begin(), all.begin() + E.size(), E.begin());
        std::copy(all.begin() + E.size(), all.begin() + E.size() + E_ft.size(), E_ft.begin());
        if (pub_c.p) std::copy(all.begin() + E.size() + E_ft.size(), all.end(), pub_eval.begin());
    }
    // ---- ft = perm_scalar sigma_6 - (zeta^n - 1) t, chunk-linearised with zeta^max_poly_size (Maller; prover.rs:1147-1200)
    const fe zeta1 = fpow(F, zeta, n), zeta_srs = fpow(F, zeta, size), zetaw_srs = fpow(F, zetaw, size);
    auto comb = [&](size_t j, int p) { return horner(F, &E[(2 * j + p) * nch], nch, p ? zetaw_srs : zeta_srs); };
    const fe wz = fpow(F, ix->omega, n - zk);
    fe zkp = F.mul(F.mul(F.sub(zeta, wz), F.sub(zeta, F.mul(wz, ix->omega))), F.sub(zeta, fpow(F, ix->omega, n - 1)));
    fe scal = F.mul(F.mul(F.mul(comb(0, 1), beta), alphas[0]), zkp);
    for (size_t i = 0; i + 1 < PERMUTS; i++)          // w_i: polynomial 7 + i; sigma_i: polynomial 37 + i
        scal = F.mul(scal, F.add(F.add(gamma, F.mul(beta, comb(37 + i, 0))), comb(7 + i, 0)));
    scal = F.neg(scal);
    const fe m1 = F.neg(F.sub(zeta1, one));
    const size_t ft_len = size < 7 * n ? size : 7 * n;
    Dev ft; KP(ft.alloc(ft_len));
    {
        std::vector<const uint64_t*> segs; std::vector<size_t> lens; std::vector<fe> scs;
        const uint64_t* sig6 = sig6_c;
        fe pw = one;
        for (size_t c = 0; c < nch; c++) {            // f_chunked.linearize(zeta^srs_len)
            if (c * size < n) { const size_t ln = n - c * size < size ? n - c * size : size; segs.push_back(sig6 + 4 * c * size); lens.push_back(ln); scs.push_back(F.mul(scal, pw)); }
            pw = F.mul(pw, zeta_srs);
        }
        pw = one;
        for (size_t c = 0; c < 7 * nch; c++) {        // t_chunked.linearize(zeta^srs_len) * -(zeta^n - 1)
            if (c * size < 7 * n) { const size_t ln = 7 * n - c * size < size ? 7 * n - c * size : size; segs.push_back(quot.at(c * size)); lens.push_back(ln); scs.push_back(F.mul(m1, pw)); }
            pw = F.mul(pw, zeta_srs);
        }
        KP(kh_poly_lincomb_dev(fid, segs.data(), lens.data(), (const uint64_t*)scs.data(), segs.size(), ft.p, ft_len));
    }
    fe fte[2];                                        // ft at zeta, zeta omega from the chunk evaluations (the polynomial itself is only needed by the opening)
    for (int p = 0; p < 2; p++)
        fte[p] = F.add(F.mul(scal, horner(F, &E_ft[p * nch], nch, zeta_srs)), F.mul(m1, horner(F, &E_ft[2 * nch + p * 7 * nch], 7 * nch, zeta_srs)));
    const fe blinding_ft = F.mul(m1, horner(F, t_blind, ntb, zeta_srs));
    // ---- Fr-sponge: v, u (prover.rs:1206-1250, plonk_sponge.rs:92-155)
    fe v, u;
    {
        SpongeH fr, pd; KP(kh_sponge_new(KH_SPONGE_FR, curve, &fr.s)); KP(kh_sponge_new(KH_SPONGE_FR, curve, &pd.s));
        fe d; KP(kh_sponge_digest(fq.s, d.l)); KP(kh_sponge_absorb(fr.s, d.l, 1));
        {                                             // the digest of the previous challenges (prover.rs:1212-1219)
            size_t pos = 0;
            for (size_t j = 0; j < n_prev; j++) { KP(kh_sponge_absorb(pd.s, prev_chals + 4 * pos, prev_rounds[j])); pos += prev_rounds[j]; }
        }
        KP(kh_sponge_digest(pd.s, d.l)); KP(kh_sponge_absorb(fr.s, d.l, 1));
        std::vector<fe> flat; flat.reserve(1 + 2 * nch * (npoly + 1));
        flat.push_back(fte[1]);
        flat.insert(flat.end(), pub_eval.begin(), pub_eval.end());
        flat.insert(flat.end(), E.begin(), E.begin() + 2 * nch * L0);
        if (lk) {                                     // plonk_sponge.rs:92-155: aggregation, table, sorted ..., pattern selectors
            auto both = [&](size_t j) { flat.insert(flat.end(), E.begin() + 2 * nch * j, E.begin() + 2 * nch * (j + 1)); };
            both(L0 + ns); both(L0 + ns + 1);
            for (size_t k = 0; k < ns; k++) both(L0 + k);
            for (size_t k = 0; k < nrt + npat; k++) both(L0 + nl + k);
        }
        KP(kh_sponge_absorb(fr.s, (const uint64_t*)flat.data(), flat.size()));
        KP(scalar_challenge(fr.s, v)); KP(scalar_challenge(fr.s, u));
    }
    pr->set_elems(KH_PROOF_EVALS, E.data(), E.size());
    pr->set_elems(KH_PROOF_PUBLIC_EVALS, pub_eval.data(), pub_eval.size());
    pr->set_elems(KH_PROOF_FT_EVAL1, &fte[1], 1);
    mark();
    // ---- SRS::open on (public, ft, z, 6 selectors, w x 15, coefficients x 15, sigma x 6, optional selectors)
    size_t logs = 0; while (((size_t)1 << logs) < size) logs++;
    std::vector<uint64_t> lr_xy(16 * logs); std::vector<uint8_t> lr_inf(2 * logs);
    uint64_t delta[8], sg[8], z1[4], z2[4]; uint8_t dinf = 0, sginf = 0;
    {
        std::vector<const uint64_t*> op; std::vector<size_t> ol, oc;
        // the previous challenges' polynomials b_poly_coefficients(chals), non-hiding, opened first (prover.rs:1220-1262); their evaluations are
        // closed-form (RecursionChallenge::evals, proof.rs:455-494): one chunk, or two when the polynomial is twice the SRS size
        std::vector<Dev> prev_bufs(n_prev);
        std::vector<fe> prev_e0, prev_e1;             // chunk evaluations at zeta / zeta omega, polynomial after polynomial
        {
            size_t cpos = 0;
            for (size_t j = 0; j < n_prev; j++) {
                const unsigned k = prev_rounds[j];
                KP_REQUIRE(k <= 26, "previous challenge %zu has %u rounds", j, k);
                const size_t ln = (size_t)1 << k;
                const size_t want_chunks = ln <= size ? 1 : 2;
                KP_REQUIRE((ln == size || ln == 2 * size) && prev_comm_chunks[j] == want_chunks, "previous challenge %zu: 2^%u coefficients / %zu commitment chunks do not fit an SRS of %zu", j, k, prev_comm_chunks[j], size);
                std::vector<fe> bc(ln);
                KP(kh_b_poly_coefficients(fid, prev_chals + 4 * cpos, k, 1, (uint64_t*)bc.data()));
                KP(prev_bufs[j].alloc(ln)); KP(kh_dev_upload(prev_bufs[j].p, bc.data(), ln * 32));
                op.push_back(prev_bufs[j].p); ol.push_back(ln); oc.push_back(want_chunks);
                fe full[2];
                for (int p = 0; p < 2; p++) {         // b_poly(chals, x) = prod_i (1 + chals[i] x^(2^(k-1-i))) (commitment.rs:426-436)
                    std::vector<fe> pw(k ? k : 1); pw[0] = pts[p];
                    for (unsigned i = 1; i < k; i++) pw[i] = F.sqr(pw[i - 1]);
                    fe r = one;
                    for (unsigned i = 0; i < k; i++) r = F.mul(r, F.add(one, F.mul(load(prev_chals + 4 * (cpos + i)), pw[k - 1 - i])));
                    full[p] = r;
                }
                if (want_chunks == 1) { prev_e0.push_back(full[0]); prev_e1.push_back(full[1]); }
                else {
                    const fe d0 = horner(F, bc.data() + size, ln - size, zeta), d1 = horner(F, bc.data() + size, ln - size, zetaw);
                    prev_e0.push_back(F.sub(full[0], F.mul(d0, zeta_srs))); prev_e0.push_back(d0);
                    prev_e1.push_back(F.sub(full[1], F.mul(d1, zetaw_srs))); prev_e1.push_back(d1);
                }
                cpos += k;
            }
        }
        op.push_back(pub_c.p ? pub_c.p : ix->zero_poly); ol.push_back(pub_c.p ? n : 0); oc.push_back(nch);
        op.push_back(ft.p); ol.push_back(ft_len); oc.push_back(1);
        for (size_t j = 0; j < npoly; j++) { op.push_back(polys[j]); ol.push_back(n); oc.push_back(nch); }
        std::vector<fe> bl;                            // one blinder per chunk of every opened polynomial
        bl.insert(bl.end(), prev_e0.size(), zero);
        bl.insert(bl.end(), nch, one); bl.push_back(blinding_ft);
        bl.insert(bl.end(), z_blind, z_blind + nch);
        bl.insert(bl.end(), 6 * nch, one);
        bl.insert(bl.end(), w_blind, w_blind + COLUMNS * nch);
        bl.insert(bl.end(), (COLUMNS + PERMUTS - 1 + nopt) * nch, zero);
        if (lk) {                                     // sorted, aggregation, the combined table -- sum_i jc^i over its masked columns + the table-id combiner
            bl.insert(bl.end(), s_blind, s_blind + ns * nch);                       // (prover.rs:1384-1400) --, the non-hiding pattern selectors
            bl.insert(bl.end(), a_blind, a_blind + nch);
            fe tb = tic_t, pw = one;
            for (size_t i = 0; i < lk->tcols.size(); i++) { tb = F.add(tb, pw); pw = F.mul(pw, jc); }
            if (has_rt) {                              // the runtime column's blinders enter the combined table's through the joint combiner (prover.rs:1402-1415)
                for (size_t c = 0; c < nch; c++) bl.push_back(F.add(F.mul(jc, rt_blind[c]), tb));
                bl.insert(bl.end(), rt_blind, rt_blind + nch);
                bl.insert(bl.end(), nch, zero);
            } else bl.insert(bl.end(), nch, tb);
            bl.insert(bl.end(), npat * nch, zero);
        }
        Dev a_dev, b_dev; KP(a_dev.alloc(size)); KP(b_dev.alloc(size));
        size_t out_len = 0;
        KP(kh_combine_polys_dev(fid, op.data(), ol.data(), oc.data(), op.size(), v.l, size, a_dev.p, &out_len));
        KP(kh_b_init_dev(fid, (const uint64_t*)pts, 2, u.l, size, b_dev.p));
        // per chunk: combined_inner_product (commitment.rs:622-657) and the combined blinder
        fe blinding_factor = zero, cip = zero, ps = one;
        size_t bi = 0;
        auto take = [&](const fe& c0, const fe& c1) {
            blinding_factor = F.add(blinding_factor, F.mul(bl[bi++], ps));
            cip = F.add(cip, F.mul(ps, F.add(c0, F.mul(u, c1))));
            ps = F.mul(ps, v);
        };
        for (size_t c = 0; c < prev_e0.size(); c++) take(prev_e0[c], prev_e1[c]);
        for (size_t c = 0; c < nch; c++) take(pub_eval[c], pub_eval[nch + c]);
        take(fte[0], fte[1]);
        for (size_t j = 0; j < npoly; j++) for (size_t c = 0; c < nch; c++) take(E[(2 * j) * nch + c], E[(2 * j + 1) * nch + c]);
        KP_REQUIRE(bi == bl.size(), "blinders / evaluation chunks mismatch");
        const fe* ob = draw(2 * logs + 2);            // (rand_l, rand_r) per round, then d, r_delta
        KP(kh_ipa_open(srs, a_dev.p, size, b_dev.p, size, cip.l, blinding_factor.l, fq_before.s, (const uint64_t*)ob, 2 * logs + 2, lr_xy.data(), lr_inf.data(),
                       delta, &dinf, z1, z2, sg, &sginf));
    }
    KP_REQUIRE(rpos == need, "randomness count mismatch");
    if (check) {                                     // the deferred invariants, earliest first (the reference returns the first it meets)
        uint32_t fl = 0;
        KP(kh_dev_download(&fl, chk.p, 4));
        for (unsigned bit = 0; bit < 4; bit++) KP_REQUIRE(!(fl & (1u << bit)), "%s", chk_msg[bit]);
    }
    pr->set_points(KH_PROOF_LR, lr_xy.data(), lr_inf.data(), 2 * logs);
    pr->set_points(KH_PROOF_DELTA, delta, &dinf, 1);
    pr->set_points(KH_PROOF_SG, sg, &sginf, 1);
    fe zz[2] = {load(z1), load(z2)};
    pr->set_elems(KH_PROOF_Z1_Z2, zz, 2);
    fe ch[7] = {beta, gamma, alpha, zeta, v, u, jc};
    pr->set_elems(KH_PROOF_CHALLENGES, ch, lk ? 7 : 6);
    KP(kh_sync());                                   // every queued user of the buffers released below has finished
    mark();
    {                                                // the shape of the serialised proof, and a copy of the previous challenges
        static const char* const OPTIONAL_GATE_NAMES[6] = {"RangeCheck0", "RangeCheck1", "ForeignFieldAdd", "ForeignFieldMul", "Xor16", "Rot64"};
        kh_proof_wire::Shape& sh = pr->shape;
        for (int g : ix->optional)
            for (int k = 0; k < 6; k++) if (!strcmp(kh_gate_name(g), OPTIONAL_GATE_NAMES[k])) sh.optional |= (uint8_t)(1u << k);
        if (lk) {
            sh.lookup = true; sh.runtime = has_rt; sh.max_per_row = (unsigned)lk->mpr;
            for (int q : lk->pats) sh.patterns |= (uint8_t)(1u << q);
        }
        sh.known = true;
        size_t nchal = 0, nchunk = 0;
        for (size_t j = 0; j < n_prev; j++) { nchal += prev_rounds[j]; nchunk += prev_comm_chunks[j]; }
        if (n_prev) {
            pr->prev.chals.assign(prev_chals, prev_chals + 4 * nchal); pr->prev.rounds.assign(prev_rounds, prev_rounds + n_prev);
            pr->prev.comm_xy.assign(prev_comm_xy, prev_comm_xy + 8 * nchunk); pr->prev.comm_inf.assign(prev_comm_inf, prev_comm_inf + nchunk);
            pr->prev.comm_chunks.assign(prev_comm_chunks, prev_comm_chunks + n_prev);
        }
    }
    guard.p = nullptr;
    *out = pr;
    return KH_OK;
}

int kh_proof_section(const kh_proof_t* proof, int section, const uint64_t** limbs, const uint8_t** flags, size_t* count) {
    if (!proof || section < 0 || section > KH_PROOF_LOOKUP_RUNTIME_COMM || !limbs || !count) { kh::set_error("kh_proof_section: bad argument"); return KH_E_INVALID; }
    const kh_proof::Sec& s = proof->sec[section];
    *limbs = s.limbs.data(); *count = s.count;
    if (flags) *flags = s.points ? s.flags.data() : nullptr;
    return KH_OK;
}
// a proof from a caller's own data (a deserialised ProverProof), for kh_verify: the sections are copied as given; what they must hold is checked where the
// curve is known, in kh_batch_verify
int kh_proof_from_sections(const kh_section_t* sections, size_t n_sections, kh_proof_t** out) {
    if (!sections || !out || n_sections > KH_PROOF_LOOKUP_RUNTIME_COMM + 1) { kh::set_error("kh_proof_from_sections: bad argument"); return KH_E_INVALID; }
    for (size_t s = 0; s < n_sections; s++)
        if (sections[s].count && !sections[s].limbs) { kh::set_error("kh_proof_from_sections: section %zu has %zu entries and no limbs", s, sections[s].count); return KH_E_INVALID; }
    kh_proof* pr = new (std::nothrow) kh_proof();
    if (!pr) { kh::set_error("out of memory"); return KH_E_NOMEM; }
    for (size_t s = 0; s < n_sections; s++) {
        const kh_section_t& in = sections[s];
        if (s == KH_PROOF_PUBLIC_COMM || s == KH_PROOF_CHALLENGES || !in.count) continue;      // the verifier derives both
        const bool points = s <= KH_PROOF_PUBLIC_COMM || s == KH_PROOF_LR || s == KH_PROOF_DELTA || s == KH_PROOF_SG || s >= KH_PROOF_LOOKUP_SORTED_COMM;
        if (points) {
            const std::vector<uint8_t> finite(in.count, 0);
            pr->set_points((int)s, in.limbs, in.flags ? in.flags : finite.data(), in.count);
        } else pr->set_elems((int)s, (const fe*)in.limbs, in.count);
    }
    *out = pr;
    return KH_OK;
}
int kh_proof_phase_seconds(const kh_proof_t* proof, double* seconds, size_t cap) {
    if (!proof || !seconds) { kh::set_error("kh_proof_phase_seconds: null argument"); return KH_E_INVALID; }
    for (size_t i = 0; i < cap && i < 6; i++) seconds[i] = proof->phase[i];
    return 6;
}
int kh_proof_prev_challenges(const kh_proof_t* proof, const uint64_t** chals, const unsigned** rounds, const uint64_t** comm_xy, const uint8_t** comm_inf,
                             const size_t** comm_chunks, size_t* n_prev) {
    if (!proof || !chals || !rounds || !comm_xy || !comm_inf || !comm_chunks || !n_prev) { kh::set_error("kh_proof_prev_challenges: null argument"); return KH_E_INVALID; }
    const kh::ProofPrev& p = proof->prev;
    *n_prev = p.rounds.size();
    *chals = p.chals.data(); *rounds = p.rounds.data(); *comm_xy = p.comm_xy.data(); *comm_inf = p.comm_inf.data(); *comm_chunks = p.comm_chunks.data();
    return KH_OK;
}
void kh_proof_free(kh_proof_t* proof) { delete proof; }

}  // extern "C"
