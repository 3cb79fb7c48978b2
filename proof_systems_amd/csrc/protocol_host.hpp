// protocol_host.hpp -- what the two host loops over the C ABI, csrc/prover.cpp (ProverProof::create) and csrc/verifier.cpp (verify / batch_verify), share:
// small helpers on Montgomery limbs and device allocations, and the lookup argument's protocol data with the token programs of its constraints, so
// that the prover's quotient and the verifier's constant term evaluate ONE statement of them.
#pragma once
#include <stdint.h>
#include <string.h>
#include <sys/random.h>
#include <vector>

#include "../../include/kimchi_hip.h"
#include "host_ec.hpp"

namespace kh {
void set_error(const char* fmt, ...);
}

namespace kh_protocol {
using khost::fe;
constexpr size_t COLUMNS = 15, PERMUTS = 7;
constexpr int ALPHA_PERM0 = 21;                      // the gates take the first 21 powers of alpha (linearization.rs:56-58), the permutation the next 3
struct Dev {                                         // a device allocation that lives as long as the proof is being made
    uint64_t* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) (void)kh_dev_free(p); }
    int alloc(size_t elems) { return kh_dev_alloc((void**)&p, elems * 32); }
    uint64_t* at(size_t elem) const { return p + 4 * elem; }
};
struct SpongeH {
    kh_sponge_t* s = nullptr;
    ~SpongeH() { if (s) kh_sponge_free(s); }
};
inline fe load(const uint64_t* l) { fe r; memcpy(&r, l, 32); return r; }
inline fe fpow(const khost::Fld& F, fe base, uint64_t e) {
    fe acc = F.f.one;
    while (e) { if (e & 1) acc = F.mul(acc, base); base = F.sqr(base); e >>= 1; }
    return acc;
}
// sum_k c[k] x^k over `cnt` consecutive elements (ProofEvaluations::combine: the chunks of one evaluation)
inline fe horner(const khost::Fld& F, const fe* c, size_t cnt, const fe& x) {
    fe acc = {{0, 0, 0, 0}};
    for (size_t k = cnt; k-- > 0;) acc = F.add(F.mul(acc, x), c[k]);
    return acc;
}
inline int os_random(int fid, size_t k, fe* out) {          // uniform elements of the field, used as Montgomery limbs
    const fe& p = khost::field(fid).p;
    for (size_t i = 0; i < k;) {
        fe buf[8];
        if (getrandom(buf, sizeof(buf), 0) != (ssize_t)sizeof(buf)) { kh::set_error("getrandom failed"); return KH_E_DEVICE; }
        for (int j = 0; j < 8 && i < k; j++) {
            buf[j].l[3] &= 0x7fffffffffffffffULL;
            if (!khost::geq(buf[j], p)) out[i++] = buf[j];
        }
    }
    return KH_OK;
}

// ---- the lookup argument (kimchi/src/circuits/lookup/): protocol data and the expressions of its constraints as token programs ----
// LookupPattern::lookups (lookups.rs:417-487): per pattern the joint lookups of a row -- table id (a constant, or a witness column) and the
// witness columns of the entry.  Pattern ids: 0 Xor, 1 Lookup, 2 RangeCheck, 3 ForeignFieldMul (the reference's order).
struct JointLookup { int tid_is_column, tid, ncell, cells[3]; };
struct Pattern { int n; JointLookup l[4]; };
static const char* const PATTERN_NAMES[4] = {"Xor", "Lookup", "RangeCheck", "ForeignFieldMul"};
static const Pattern PATTERNS[4] = {
    {4, {{0, 0, 3, {3, 7, 11}}, {0, 0, 3, {4, 8, 12}}, {0, 0, 3, {5, 9, 13}}, {0, 0, 3, {6, 10, 14}}}},
    {3, {{1, 0, 2, {1, 2, 0}}, {1, 0, 2, {3, 4, 0}}, {1, 0, 2, {5, 6, 0}}, {0, 0, 0, {0, 0, 0}}}},
    {4, {{0, 1, 1, {3, 0, 0}}, {0, 1, 1, {4, 0, 0}}, {0, 1, 1, {5, 0, 0}}, {0, 1, 1, {6, 0, 0}}}},
    {4, {{0, 1, 1, {7, 0, 0}}, {0, 1, 1, {8, 0, 0}}, {0, 1, 1, {9, 0, 0}}, {0, 1, 1, {10, 0, 0}}}},
};
// a postfix token program under construction (KH_TOK_*), constants interned by value
struct Prog {
    std::vector<uint32_t> t;
    std::vector<fe> consts;
    void push(uint32_t op, uint32_t a) { t.push_back(op); t.push_back(a); }
    void C(const fe& v) {
        for (size_t i = 0; i < consts.size(); i++) if (khost::eq(consts[i], v)) { push(KH_TOK_CONST, (uint32_t)i); return; }
        consts.push_back(v); push(KH_TOK_CONST, (uint32_t)(consts.size() - 1));
    }
    void cell(uint32_t col, int next = 0) { push(KH_TOK_CELL, 2 * col + (next ? 1u : 0u)); }
    void add() { push(KH_TOK_ADD, 0); }
    void sub() { push(KH_TOK_SUB, 0); }
    void mul() { push(KH_TOK_MUL, 0); }
    int run(int fid, const std::vector<const uint64_t*>& cols, const std::vector<size_t>& lens, size_t rows, unsigned stride, unsigned next_shift, int accumulate, uint64_t* out) const {
        return kh_expr_evaluations_dev(fid, t.data(), t.size() / 2, cols.data(), lens.data(), cols.size(), (const uint64_t*)consts.data(), consts.size(), rows, stride,
                                       next_shift, accumulate, out);
    }
};
struct LookupChallenges { fe jc, tic, beta, gamma, gb1; fe prefactor[5]; };   // prefactor[k] = (gamma + dummy)^k (1 + beta)^max_per_row, dummy = 0
// combine_table_entry (tables/mod.rs:147-162) of one joint lookup: Horner in the joint combiner from the last cell + table_id_combiner * id
inline void emit_joint(Prog& p, const khost::Fld& F, const JointLookup& L, const LookupChallenges& ch) {
    p.cell((uint32_t)L.cells[L.ncell - 1]);
    for (int i = L.ncell - 2; i >= 0; i--) { p.C(ch.jc); p.mul(); p.cell((uint32_t)L.cells[i]); p.add(); }
    if (L.tid_is_column) { p.cell((uint32_t)L.tid); p.C(ch.tic); p.mul(); p.add(); }
    else if (L.tid) { fe id = {{(uint64_t)L.tid, 0, 0, 0}}; p.C(F.mul(ch.tic, F.to_mont(id))); p.add(); }
}
// (1 + beta)^max_per_row (gamma + dummy)^padding prod (gamma + joint value)   (constraints.rs:497-523)
inline void emit_fterm(Prog& p, const khost::Fld& F, const Pattern* pat, size_t mpr, const LookupChallenges& ch) {
    const int n = pat ? pat->n : 0;
    p.C(ch.prefactor[mpr - (size_t)n]);
    for (int i = 0; i < n; i++) { p.C(ch.gamma); emit_joint(p, F, pat->l[i], ch); p.add(); p.mul(); }
}
// numerator of an aggregation row: f_chunk * t_chunk, with the pattern selectors at columns sel0.., the combined table at column `table`
inline void emit_numerator(Prog& p, const khost::Fld& F, const std::vector<int>& pats, size_t mpr, const LookupChallenges& ch, uint32_t sel0, uint32_t table) {
    p.C(F.f.one);
    for (size_t k = 0; k < pats.size(); k++) { p.cell(sel0 + (uint32_t)k); if (k) p.add(); }
    p.sub();                                                            // 1 - sum of the selectors: a row without lookups
    emit_fterm(p, F, nullptr, mpr, ch); p.mul();
    for (size_t k = 0; k < pats.size(); k++) { p.cell(sel0 + (uint32_t)k); emit_fterm(p, F, &PATTERNS[pats[k]], mpr, ch); p.mul(); p.add(); }
    p.C(ch.gb1); p.cell(table); p.add(); p.C(ch.beta); p.cell(table, 1); p.mul(); p.add();      // t_chunk = gamma (1 + beta) + t + beta t'
    p.mul();
}
// denominator: prod_i (gamma (1 + beta) + s_i + beta s_i') with the roles of s_i, s_i' swapped for odd i (the snake)
inline void emit_denominator(Prog& p, size_t mpr, const LookupChallenges& ch, uint32_t sorted0) {
    for (size_t i = 0; i <= mpr; i++) {
        const int odd = (int)(i & 1);
        p.C(ch.gb1); p.cell(sorted0 + (uint32_t)i, odd); p.add(); p.C(ch.beta); p.cell(sorted0 + (uint32_t)i, !odd); p.mul(); p.add();
        if (i) p.mul();
    }
}
// The lookup constraints (lookup/constraints.rs:378-673), combined with alpha^24 ...: appended to `p` as one expression.  Columns: witness 0..14, then
// where the caller put the rest.  On d8 columns (stride 1, next_shift 8) this is the lookup part of the quotient (prover.rs:874-903); on two-row
// columns of a proof's evaluations (row 0 at zeta, row 1 at zeta omega; the three row-set atoms evaluated at zeta) it is the lookup part of the
// linearisation's constant term (verifier.rs:412-490).
struct LookupColumns { uint32_t sorted0, agg, table, sel0, vanish, l0, lfinal, rt, rtsel; };
inline void emit_lookup_constraints(Prog& p, const khost::Fld& F, const std::vector<int>& pats, size_t mpr, const LookupChallenges& cch, const fe& alpha,
                                    const LookupColumns& c, bool has_rt) {
    const fe one = F.f.one;
    fe ap = fpow(F, alpha, ALPHA_PERM0 + 3);
    // alpha^24 vanish (aggreg' denominator - aggreg numerator)
    p.C(ap); p.cell(c.vanish);
    p.cell(c.agg, 1); emit_denominator(p, mpr, cch, c.sorted0); p.mul();
    p.cell(c.agg); emit_numerator(p, F, pats, mpr, cch, c.sel0, c.table); p.mul();
    p.sub(); p.mul(); p.mul();
    // alpha^25 l0 (aggreg - 1), alpha^26 lfinal (aggreg - 1)
    for (int i = 0; i < 2; i++) { ap = F.mul(ap, alpha); p.C(ap); p.cell(i ? c.lfinal : c.l0); p.cell(c.agg); p.C(one); p.sub(); p.mul(); p.mul(); p.add(); }
    // the snake's shared elements: lfinal (s_i - s_i+1) for even i, l0 (...) for odd i
    for (size_t i = 0; i < mpr; i++) {
        ap = F.mul(ap, alpha);
        p.C(ap); p.cell((i & 1) ? c.l0 : c.lfinal); p.cell(c.sorted0 + (uint32_t)i); p.cell(c.sorted0 + (uint32_t)i + 1); p.sub(); p.mul(); p.mul(); p.add();
    }
    // the constraints are padded to 3 + 4, then RT(x) selector_RT(x) (constraints.rs:658-680, runtime_tables.rs:59-66)
    if (has_rt) { p.C(fpow(F, alpha, ALPHA_PERM0 + 3 + 7)); p.cell(c.rt); p.cell(c.rtsel); p.mul(); p.mul(); p.add(); }
}
}  // namespace kh_protocol
