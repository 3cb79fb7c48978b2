// proof_wire.hpp -- the structure walk between the msgpack bytes of a ProverProof / VerifierIndex (rmp-serde: structs as arrays in declaration order,
// Option::None as nil, points as 33-byte bins, field elements as 32-byte little-endian bins) and the library's sections, for proof_msgpack.cpp.
//
//   ProverProof       kimchi/src/proof.rs:134-195   [commitments [w[15], z, t, lookup?[sorted[], aggreg, runtime?]], opening [lr[(L, R)], delta, z1, z2, sg],
//                                                    evals, ft_eval1, prev_challenges[[chals[], comm]]]
//   ProofEvaluations  kimchi/src/proof.rs:51-115    [public?, w[15], z, s[6], coefficients[15], generic, poseidon, complete_add, mul, emul, endomul_scalar,
//                                                    range_check0?, range_check1?, foreign_field_add?, foreign_field_mul?, xor?, rot?, lookup_aggregation?,
//                                                    lookup_table?, lookup_sorted[5 x ?], runtime_lookup_table?, runtime_lookup_table_selector?,
//                                                    xor / lookup / range_check / foreign_field_mul lookup selector ?]      an evaluation: [[zeta chunks], [zeta omega chunks]]
//   VerifierIndex     kimchi/src/verifier_index.rs:59-158   [domain (236 bytes), max_poly_size, zk_rows, public, prev_challenges, sigma_comm[7],
//                                                    coefficients_comm[15], generic, psm, complete_add, mul, emul, endomul_scalar, the six optional gates ?
//                                                    (order as in the evaluations), shift[7], lookup_index?]
//   LookupVerifierIndex  verifier_index.rs:35-56    [joint_lookup_used, lookup_table[], lookup_selectors[xor?, lookup?, range_check?, ffmul?], table_ids?,
//                                                    lookup_info [max_per_row, max_joint_size, features [patterns[4 bools], joint_lookup_used,
//                                                    uses_runtime_tables]], runtime_tables_selector?]
//   PolyComm          [[chunk, ...]]
//   the domain record size u64 LE | log_size u32 LE | 7 x 32-byte LE elements (n, 1/n, omega, 1/omega, 1, 1, 1)
//
// A proof comes out as the wire sections kh_proofs_from_wire takes (numbered as KH_PROOF_*), its previous challenges and its SHAPE: which Options were
// there.  Writing is the same walk backwards and needs the shape.  Host C++ over byte buffers with no device type and no library state: what must hold
// inside one file is refused here with the byte offset; what needs the other file (chunk counts against the index, rounds against the SRS) is kh_verify's.
#pragma once
#include <stdarg.h>

#include "msgpack_wire.hpp"

namespace kh_proof_wire {

using kh_msgpack::Reader;
using kh_msgpack::Writer;

constexpr size_t POINT = 33, ELEM = 32, DOMAIN_ELEMS = 7, DOMAIN_RECORD = 12 + 32 * DOMAIN_ELEMS, COLUMNS = 15, PERMUTS = 7;
// the section numbers of include/kimchi_hip.h (KH_PROOF_*, KH_VINDEX_*; proof_msgpack.cpp asserts they agree)
enum { P_W_COMM = 0, P_Z_COMM, P_T_COMM, P_PUBLIC_COMM, P_EVALS, P_PUBLIC_EVALS, P_FT_EVAL1, P_LR, P_DELTA, P_Z1_Z2, P_SG, P_CHALLENGES, P_LOOKUP_SORTED_COMM,
       P_LOOKUP_AGGREG_COMM, P_LOOKUP_RUNTIME_COMM, P_SECTIONS };
enum { V_SIGMA_COMM = 0, V_COEFFICIENTS_COMM, V_GENERIC_COMM, V_SELECTOR_COMM, V_OPTIONAL_COMM, V_SHIFTS, V_DIGEST, V_LOOKUP_TABLE_COMM, V_LOOKUP_TABLE_IDS_COMM,
       V_LOOKUP_SELECTOR_COMM, V_LOOKUP_RUNTIME_SELECTOR_COMM, V_LOOKUP_INFO, V_SECTIONS };
static const char* const OPTIONAL_NAMES[6] = {"range_check0", "range_check1", "foreign_field_add", "foreign_field_mul", "xor", "rot"};
static const char* const PATTERN_SELECTOR_NAMES[4] = {"xor_lookup_selector", "lookup_gate_lookup_selector", "range_check_lookup_selector", "foreign_field_mul_lookup_selector"};
static const char* const DOMAIN_NAMES[DOMAIN_ELEMS] = {"size_as_field_element", "size_inv", "group_gen", "group_gen_inv", "offset", "offset_inv", "offset_pow_size"};

// which Options of a proof are there
struct Shape {
    bool known = false;
    uint8_t optional = 0;            // bit k: the selector evaluation of optional gate k (OPTIONAL_NAMES' order)
    uint8_t patterns = 0;            // bit k: the selector evaluation of lookup pattern k
    bool lookup = false, runtime = false;
    unsigned max_per_row = 0;        // sorted polynomials - 1
    bool same(const Shape& o) const { return optional == o.optional && patterns == o.patterns && lookup == o.lookup && runtime == o.runtime && max_per_row == o.max_per_row; }
};
struct Section {
    std::vector<uint8_t> bytes;      // count records of 33 bytes, or count elements of 32
    size_t count = 0;
};
struct PrevChallenge {
    Section chals, comm;             // RecursionChallenge { chals, comm }
};
struct Proof {
    Section sec[P_SECTIONS];
    Shape shape;
    std::vector<PrevChallenge> prev;
};
struct Index {
    uint64_t domain_size = 0, max_poly_size = 0, zk_rows = 0, public_inputs = 0, prev_challenges = 0;
    uint32_t log_size = 0;
    uint8_t domain[32 * DOMAIN_ELEMS] = {0};
    Section sec[V_SECTIONS];         // V_DIGEST and V_LOOKUP_INFO stay empty
    size_t chunks = 0;               // per commitment
    uint8_t optional = 0;            // as Shape::optional
    bool lookup = false, joint_lookup_used = false, uses_runtime_tables = false;
    uint8_t patterns = 0;
    uint64_t max_per_row = 0, max_joint_size = 0;
};

inline int popcount8(unsigned v) { int c = 0; for (; v; v &= v - 1) c++; return c; }

// ------------------------------------------------------------------------------------------------------------------------ reading
struct Walk {
    Reader r;
    Walk(const uint8_t* b, size_t n) : r(b, n) {}
    bool fail(size_t at, const char* fmt, ...) {
        if (r.failed) return false;
        r.failed = true;
        const int k = snprintf(r.err, sizeof(r.err), "offset %zu: ", at);
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(r.err + k, sizeof(r.err) - (size_t)k, fmt, ap);
        va_end(ap);
        return false;
    }
    bool record(Section& s, size_t width) {
        const uint8_t* b = nullptr;
        if (!r.bin_of(width, &b)) return false;
        s.bytes.insert(s.bytes.end(), b, b + width);
        s.count++;
        return true;
    }
    bool point(Section& s) { return record(s, POINT); }
    bool elem(Section& s) { return record(s, ELEM); }
    // PolyComm { chunks }
    bool comm(Section& s, size_t* chunks, const char* what) {
        size_t c = 0;
        if (!r.enter_of(1, what) || !r.enter(&c)) return false;
        for (size_t i = 0; i < c; i++) if (!point(s)) return false;
        r.leave(); r.leave();
        *chunks = c;
        return !r.failed;
    }
    // a commitment that must have as many chunks as the first one read (`*want` = 0: this is the first)
    bool comm_of(Section& s, size_t* want, const char* what, size_t idx) {
        const size_t at = r.pos;
        size_t c = 0;
        if (!comm(s, &c, what)) return false;
        if (*want == 0) {
            if (c == 0) return fail(at, "%s[%zu] has no chunks", what, idx);
            *want = c;
        } else if (c != *want) return fail(at, "%s[%zu] has %zu chunks, the first commitment has %zu", what, idx, c, *want);
        return true;
    }
    // PointEvaluations { zeta, zeta_omega }: chunks at zeta, then as many at zeta omega; every evaluation of a proof has the first one's count
    bool evaluation(Section& s, size_t* want, const char* what, size_t idx) {
        const size_t at = r.pos;
        size_t a = 0, b = 0;
        if (!r.enter_of(2, what) || !r.enter(&a)) return false;
        for (size_t i = 0; i < a; i++) if (!elem(s)) return false;
        r.leave();
        if (!r.enter(&b)) return false;
        for (size_t i = 0; i < b; i++) if (!elem(s)) return false;
        r.leave(); r.leave();
        if (r.failed) return false;
        if (a != b) return fail(at, "%s[%zu] has %zu values at zeta and %zu at zeta omega", what, idx, a, b);
        if (*want == 0) {
            if (a == 0) return fail(at, "%s[%zu] has no values", what, idx);
            *want = a;
        } else if (a != *want) return fail(at, "%s[%zu] has %zu chunks, the first evaluation has %zu", what, idx, a, *want);
        return true;
    }
    bool optional_evaluation(Section& s, size_t* want, const char* what, size_t idx, bool* present) {
        *present = !r.at_nil();
        return *present ? evaluation(s, want, what, idx) : r.nil();
    }
};

inline int finish_read(Walk& w, bool ok, const char* who, char* err, size_t cap) {
    if (ok && w.r.finish()) return 0;
    snprintf(err, cap, "%s: %s", who, w.r.err);
    return -1;
}
inline void append(Section& to, const Section& from) {
    to.bytes.insert(to.bytes.end(), from.bytes.begin(), from.bytes.end());
    to.count += from.count;
}

// 0, or -1 with `err` filled in; *out is then to be dropped
inline int read_proof(const uint8_t* bytes, size_t len, Proof* out, char* err, size_t cap) {
    *out = Proof();
    Walk w(bytes, len);
    Reader& r = w.r;
    Proof& p = *out;
    Shape& sh = p.shape;
    auto walk = [&]() -> bool {
        size_t n = 0;
        if (!r.enter_of(5, "ProverProof")) return false;
        // ---- commitments
        if (!r.enter_of(4, "commitments") || !r.enter_of(COLUMNS, "w_comm")) return false;
        size_t nch = 0, any = 0, sorted_comms = 0;
        for (size_t i = 0; i < COLUMNS; i++) if (!w.comm_of(p.sec[P_W_COMM], &nch, "w_comm", i)) return false;
        r.leave();
        if (!w.comm(p.sec[P_Z_COMM], &any, "z_comm") || !w.comm(p.sec[P_T_COMM], &any, "t_comm")) return false;
        if (r.at_nil()) r.nil();
        else {
            const size_t at = r.pos;
            if (!r.enter_of(3, "lookup commitments") || !r.enter(&sorted_comms)) return false;
            if (sorted_comms < 2 || sorted_comms > 5) return w.fail(at, "lookup.sorted has %zu commitments, 2 to 5 expected", sorted_comms);
            size_t sch = 0;
            for (size_t i = 0; i < sorted_comms; i++) if (!w.comm_of(p.sec[P_LOOKUP_SORTED_COMM], &sch, "lookup.sorted", i)) return false;
            r.leave();
            if (!w.comm(p.sec[P_LOOKUP_AGGREG_COMM], &any, "lookup.aggreg")) return false;
            if (r.at_nil()) r.nil();
            else { sh.runtime = true; if (!w.comm(p.sec[P_LOOKUP_RUNTIME_COMM], &any, "lookup.runtime")) return false; }
            r.leave();
            sh.lookup = true; sh.max_per_row = (unsigned)sorted_comms - 1;
        }
        r.leave();
        // ---- opening
        if (!r.enter_of(5, "opening") || !r.enter(&n)) return false;
        for (size_t i = 0; i < n; i++) {
            if (!r.enter_of(2, "an (L, R) pair of opening.lr") || !w.point(p.sec[P_LR]) || !w.point(p.sec[P_LR])) return false;
            r.leave();
        }
        r.leave();
        if (!w.point(p.sec[P_DELTA]) || !w.elem(p.sec[P_Z1_Z2]) || !w.elem(p.sec[P_Z1_Z2]) || !w.point(p.sec[P_SG])) return false;
        r.leave();
        // ---- evaluations, into KH_PROOF_EVALS' order: z, generic, the five selectors, w, coefficients, s, optional gates, sorted, aggregation, table,
        //      runtime table and selector, pattern selectors
        Section z, fixed, wv, co, s, opt, sorted, agg, table, rt, rtsel, pat;
        size_t ech = 0, sorted_evals = 0;
        bool here = false, agg_here = false, table_here = false, rt_here = false, rtsel_here = false;
        const size_t evals_at = r.pos;
        if (!r.enter_of(26, "evals")) return false;
        if (!w.optional_evaluation(p.sec[P_PUBLIC_EVALS], &ech, "evals.public", 0, &here)) return false;
        if (!r.enter_of(COLUMNS, "evals.w")) return false;
        for (size_t i = 0; i < COLUMNS; i++) if (!w.evaluation(wv, &ech, "evals.w", i)) return false;
        r.leave();
        if (!w.evaluation(z, &ech, "evals.z", 0) || !r.enter_of(PERMUTS - 1, "evals.s")) return false;
        for (size_t i = 0; i + 1 < PERMUTS; i++) if (!w.evaluation(s, &ech, "evals.s", i)) return false;
        r.leave();
        if (!r.enter_of(COLUMNS, "evals.coefficients")) return false;
        for (size_t i = 0; i < COLUMNS; i++) if (!w.evaluation(co, &ech, "evals.coefficients", i)) return false;
        r.leave();
        for (size_t i = 0; i < 6; i++) if (!w.evaluation(fixed, &ech, "evals.selector", i)) return false;
        for (size_t i = 0; i < 6; i++) {
            if (!w.optional_evaluation(opt, &ech, "evals.optional_selector", i, &here)) return false;
            if (here) sh.optional |= (uint8_t)(1u << i);
        }
        if (!w.optional_evaluation(agg, &ech, "evals.lookup_aggregation", 0, &agg_here) || !w.optional_evaluation(table, &ech, "evals.lookup_table", 0, &table_here)) return false;
        const size_t sorted_at = r.pos;
        if (!r.enter_of(5, "evals.lookup_sorted")) return false;
        for (size_t i = 0; i < 5; i++) {
            if (!w.optional_evaluation(sorted, &ech, "evals.lookup_sorted", i, &here)) return false;
            if (here && sorted_evals != i) return w.fail(sorted_at, "evals.lookup_sorted[%zu] follows an absent entry", i);
            if (here) sorted_evals++;
        }
        r.leave();
        if (!w.optional_evaluation(rt, &ech, "evals.runtime_lookup_table", 0, &rt_here) ||
            !w.optional_evaluation(rtsel, &ech, "evals.runtime_lookup_table_selector", 0, &rtsel_here)) return false;
        for (size_t i = 0; i < 4; i++) {
            if (!w.optional_evaluation(pat, &ech, "evals.lookup_selector", i, &here)) return false;
            if (here) sh.patterns |= (uint8_t)(1u << i);
        }
        r.leave();
        // the Options of one proof agree with each other
        if (agg_here != sh.lookup || table_here != sh.lookup || sorted_evals != sorted_comms || (sh.patterns != 0) != sh.lookup)
            return w.fail(evals_at, "evals: the lookup evaluations (aggregation %d, table %d, %zu sorted, pattern mask %u) do not match the lookup commitments (%zu sorted)",
                          (int)agg_here, (int)table_here, sorted_evals, (unsigned)sh.patterns, sorted_comms);
        if (rt_here != sh.runtime || rtsel_here != sh.runtime)
            return w.fail(evals_at, "evals: the runtime table evaluations (table %d, selector %d) do not match the runtime commitment (%d)", (int)rt_here, (int)rtsel_here, (int)sh.runtime);
        Section& e = p.sec[P_EVALS];
        for (const Section* part : {&z, &fixed, &wv, &co, &s, &opt, &sorted, &agg, &table, &rt, &rtsel, &pat}) append(e, *part);
        // ---- ft_eval1, previous challenges
        if (!w.elem(p.sec[P_FT_EVAL1]) || !r.enter(&n)) return false;
        for (size_t i = 0; i < n; i++) {
            PrevChallenge pc;
            size_t rounds = 0, chunks = 0;
            if (!r.enter_of(2, "a RecursionChallenge") || !r.enter(&rounds)) return false;
            for (size_t k = 0; k < rounds; k++) if (!w.elem(pc.chals)) return false;
            r.leave();
            if (!w.comm(pc.comm, &chunks, "prev_challenges.comm")) return false;
            r.leave();
            p.prev.push_back(std::move(pc));
        }
        r.leave(); r.leave();
        sh.known = true;
        return !r.failed;
    };
    return finish_read(w, walk(), "ProverProof", err, cap);
}

// expected_domain: the 7 x 32 bytes the domain record must hold (nullable: not compared); expected_max_poly_size: 0 = not compared
inline int read_index(const uint8_t* bytes, size_t len, const uint8_t* expected_domain, uint64_t expected_max_poly_size, Index* out, char* err, size_t cap) {
    *out = Index();
    Walk w(bytes, len);
    Reader& r = w.r;
    Index& v = *out;
    auto walk = [&]() -> bool {
        if (!r.enter_of(21, "VerifierIndex")) return false;
        size_t at = r.pos;
        const uint8_t* d = nullptr;
        if (!r.bin_of(DOMAIN_RECORD, &d)) return false;
        for (int i = 0; i < 8; i++) v.domain_size |= (uint64_t)d[i] << (8 * i);
        for (int i = 0; i < 4; i++) v.log_size |= (uint32_t)d[8 + i] << (8 * i);
        memcpy(v.domain, d + 12, sizeof(v.domain));
        if (v.log_size >= 64 || v.domain_size != (uint64_t)1 << v.log_size)
            return w.fail(at, "domain: size %llu is not 2^log_size (log_size %u)", (unsigned long long)v.domain_size, v.log_size);
        if (expected_domain)
            for (size_t i = 0; i < DOMAIN_ELEMS; i++)
                if (memcmp(v.domain + 32 * i, expected_domain + 32 * i, 32)) return w.fail(at, "domain: %s is not the library's value for a domain of 2^%u", DOMAIN_NAMES[i], v.log_size);
        at = r.pos;
        if (!r.uint(&v.max_poly_size)) return false;
        if (expected_max_poly_size && v.max_poly_size != expected_max_poly_size)
            return w.fail(at, "max_poly_size %llu, the SRS has %llu points", (unsigned long long)v.max_poly_size, (unsigned long long)expected_max_poly_size);
        if (!r.uint(&v.zk_rows) || !r.uint(&v.public_inputs) || !r.uint(&v.prev_challenges)) return false;
        size_t nch = 0;
        if (!r.enter_of(PERMUTS, "sigma_comm")) return false;
        for (size_t i = 0; i < PERMUTS; i++) if (!w.comm_of(v.sec[V_SIGMA_COMM], &nch, "sigma_comm", i)) return false;
        r.leave();
        if (!r.enter_of(COLUMNS, "coefficients_comm")) return false;
        for (size_t i = 0; i < COLUMNS; i++) if (!w.comm_of(v.sec[V_COEFFICIENTS_COMM], &nch, "coefficients_comm", i)) return false;
        r.leave();
        if (!w.comm_of(v.sec[V_GENERIC_COMM], &nch, "generic_comm", 0)) return false;
        for (size_t i = 0; i < 5; i++) if (!w.comm_of(v.sec[V_SELECTOR_COMM], &nch, "selector_comm", i)) return false;
        for (size_t i = 0; i < 6; i++) {
            if (r.at_nil()) { r.nil(); continue; }
            if (!w.comm_of(v.sec[V_OPTIONAL_COMM], &nch, "optional_comm", i)) return false;
            v.optional |= (uint8_t)(1u << i);
        }
        v.chunks = nch;
        if (!r.enter_of(PERMUTS, "shift")) return false;
        for (size_t i = 0; i < PERMUTS; i++) if (!w.elem(v.sec[V_SHIFTS])) return false;
        r.leave();
        if (r.at_nil()) r.nil();
        else {                                                           // LookupVerifierIndex
            size_t width = 0;
            bool joint_again = false, runtime_selector = false;
            at = r.pos;
            if (!r.enter_of(6, "lookup_index") || !r.boolean(&v.joint_lookup_used) || !r.enter(&width)) return false;
            if (width == 0) return w.fail(at, "lookup_index: lookup_table has no commitment");
            for (size_t i = 0; i < width; i++) if (!w.comm_of(v.sec[V_LOOKUP_TABLE_COMM], &nch, "lookup_table", i)) return false;
            r.leave();
            uint8_t selectors = 0;
            if (!r.enter_of(4, "lookup_selectors")) return false;
            for (size_t i = 0; i < 4; i++) {
                if (r.at_nil()) { r.nil(); continue; }
                if (!w.comm_of(v.sec[V_LOOKUP_SELECTOR_COMM], &nch, "lookup_selectors", i)) return false;
                selectors |= (uint8_t)(1u << i);
            }
            r.leave();
            if (r.at_nil()) r.nil();
            else if (!w.comm_of(v.sec[V_LOOKUP_TABLE_IDS_COMM], &nch, "table_ids", 0)) return false;
            const size_t info_at = r.pos;
            if (!r.enter_of(3, "lookup_info") || !r.uint(&v.max_per_row) || !r.uint(&v.max_joint_size) || !r.enter_of(3, "lookup_info.features") ||
                !r.enter_of(4, "lookup_info.features.patterns")) return false;
            for (size_t i = 0; i < 4; i++) {
                bool on = false;
                if (!r.boolean(&on)) return false;
                if (on) v.patterns |= (uint8_t)(1u << i);
            }
            r.leave();
            if (!r.boolean(&joint_again) || !r.boolean(&v.uses_runtime_tables)) return false;
            r.leave(); r.leave();
            if (r.at_nil()) r.nil();
            else { runtime_selector = true; if (!w.comm_of(v.sec[V_LOOKUP_RUNTIME_SELECTOR_COMM], &nch, "runtime_tables_selector", 0)) return false; }
            r.leave();
            if (r.failed) return false;
            if (joint_again != v.joint_lookup_used)
                return w.fail(info_at, "lookup_index: joint_lookup_used is %d, lookup_info.features.joint_lookup_used is %d", (int)v.joint_lookup_used, (int)joint_again);
            for (size_t i = 0; i < 4; i++)
                if ((selectors >> i & 1) != (v.patterns >> i & 1))
                    return w.fail(info_at, "lookup_index: the selector commitment of pattern %zu is %s, its feature bit is %s", i, selectors >> i & 1 ? "present" : "absent",
                                  v.patterns >> i & 1 ? "true" : "false");
            if (runtime_selector != v.uses_runtime_tables)
                return w.fail(info_at, "lookup_index: runtime_tables_selector is %s, uses_runtime_tables is %s", runtime_selector ? "present" : "absent", v.uses_runtime_tables ? "true" : "false");
            v.lookup = true;
        }
        r.leave();
        return !r.failed;
    };
    return finish_read(w, walk(), "VerifierIndex", err, cap);
}

// ------------------------------------------------------------------------------------------------------------------------ writing
struct Emit {
    Writer w;
    void records(const Section& s, size_t first, size_t n, size_t width) { for (size_t i = 0; i < n; i++) w.bin(s.bytes.data() + width * (first + i), width); }
    void comm(const Section& s, size_t first, size_t chunks) { w.array(1); w.array(chunks); records(s, first, chunks, POINT); }
    // evaluation j of a section laid out as KH_PROOF_EVALS: chunks at zeta, chunks at zeta omega
    void evaluation(const Section& s, size_t j, size_t chunks) {
        w.array(2);
        w.array(chunks); records(s, 2 * j * chunks, chunks, ELEM);
        w.array(chunks); records(s, (2 * j + 1) * chunks, chunks, ELEM);
    }
};

// the bytes of a proof whose shape is known; 0, or -1 with `err` filled in when the sections do not fit the shape
inline int write_proof(const Proof& p, std::vector<uint8_t>* out, char* err, size_t cap) {
    const Shape& sh = p.shape;
    auto cnt = [&](int s) { return p.sec[s].count; };
    for (int s = 0; s < P_SECTIONS; s++) {
        const bool pts = s <= P_PUBLIC_COMM || s == P_LR || s == P_DELTA || s == P_SG || s >= P_LOOKUP_SORTED_COMM;
        if (p.sec[s].bytes.size() != cnt(s) * (pts ? POINT : ELEM)) { snprintf(err, cap, "ProverProof: section %d has %zu bytes for %zu entries", s, p.sec[s].bytes.size(), cnt(s)); return -1; }
    }
    if (!sh.known) { snprintf(err, cap, "ProverProof: the shape of the proof is not known"); return -1; }
    const size_t nopt = (size_t)popcount8(sh.optional), npat = (size_t)popcount8(sh.patterns), ns = sh.lookup ? sh.max_per_row + 1 : 0;
    const size_t npoly = 7 + 2 * COLUMNS + (PERMUTS - 1) + nopt + (sh.lookup ? ns + 2 + npat : 0) + (sh.runtime ? 2 : 0);
    const size_t nch = cnt(P_W_COMM) / COLUMNS, ech = cnt(P_EVALS) / (2 * npoly);
    if (nch == 0 || cnt(P_W_COMM) != COLUMNS * nch || cnt(P_Z_COMM) == 0 || cnt(P_T_COMM) == 0 || cnt(P_DELTA) != 1 || cnt(P_SG) != 1 || cnt(P_Z1_Z2) != 2 ||
        cnt(P_FT_EVAL1) != 1 || cnt(P_LR) % 2) {
        snprintf(err, cap, "ProverProof: w_comm %zu, z_comm %zu, t_comm %zu, lr %zu, delta %zu, z1_z2 %zu, sg %zu, ft_eval1 %zu entries are not those of a proof", cnt(P_W_COMM),
                 cnt(P_Z_COMM), cnt(P_T_COMM), cnt(P_LR), cnt(P_DELTA), cnt(P_Z1_Z2), cnt(P_SG), cnt(P_FT_EVAL1));
        return -1;
    }
    if (ech == 0 || cnt(P_EVALS) != 2 * npoly * ech || (cnt(P_PUBLIC_EVALS) != 0 && cnt(P_PUBLIC_EVALS) != 2 * ech)) {
        snprintf(err, cap, "ProverProof: evals has %zu elements and public_evals %zu, the shape has %zu polynomials x 2 points x chunks", cnt(P_EVALS), cnt(P_PUBLIC_EVALS), npoly);
        return -1;
    }
    if (sh.lookup ? (sh.max_per_row < 1 || sh.max_per_row > 4 || npat == 0 || cnt(P_LOOKUP_SORTED_COMM) == 0 || cnt(P_LOOKUP_SORTED_COMM) % ns || cnt(P_LOOKUP_AGGREG_COMM) == 0 ||
                     (cnt(P_LOOKUP_RUNTIME_COMM) != 0) != sh.runtime)
                  : (cnt(P_LOOKUP_SORTED_COMM) || cnt(P_LOOKUP_AGGREG_COMM) || cnt(P_LOOKUP_RUNTIME_COMM) || sh.runtime || npat)) {
        snprintf(err, cap, "ProverProof: lookup commitments (%zu sorted, %zu aggregation, %zu runtime) do not fit the shape (lookup %d, %u per row, runtime %d, %zu patterns)",
                 cnt(P_LOOKUP_SORTED_COMM), cnt(P_LOOKUP_AGGREG_COMM), cnt(P_LOOKUP_RUNTIME_COMM), (int)sh.lookup, sh.max_per_row, (int)sh.runtime, npat);
        return -1;
    }
    Emit e;
    Writer& w = e.w;
    const Section& E = p.sec[P_EVALS];
    w.array(5);
    w.array(4);
    w.array(COLUMNS);
    for (size_t i = 0; i < COLUMNS; i++) e.comm(p.sec[P_W_COMM], i * nch, nch);
    e.comm(p.sec[P_Z_COMM], 0, cnt(P_Z_COMM));
    e.comm(p.sec[P_T_COMM], 0, cnt(P_T_COMM));
    if (!sh.lookup) w.nil();
    else {
        const size_t sch = cnt(P_LOOKUP_SORTED_COMM) / ns;
        w.array(3);
        w.array(ns);
        for (size_t i = 0; i < ns; i++) e.comm(p.sec[P_LOOKUP_SORTED_COMM], i * sch, sch);
        e.comm(p.sec[P_LOOKUP_AGGREG_COMM], 0, cnt(P_LOOKUP_AGGREG_COMM));
        if (sh.runtime) e.comm(p.sec[P_LOOKUP_RUNTIME_COMM], 0, cnt(P_LOOKUP_RUNTIME_COMM)); else w.nil();
    }
    w.array(5);
    w.array(cnt(P_LR) / 2);
    for (size_t i = 0; i < cnt(P_LR) / 2; i++) { w.array(2); e.records(p.sec[P_LR], 2 * i, 2, POINT); }
    e.records(p.sec[P_DELTA], 0, 1, POINT);
    e.records(p.sec[P_Z1_Z2], 0, 2, ELEM);
    e.records(p.sec[P_SG], 0, 1, POINT);
    // polynomial numbers of KH_PROOF_EVALS
    const size_t J_Z = 0, J_FIXED = 1, J_W = 7, J_CO = J_W + COLUMNS, J_S = J_CO + COLUMNS, J_OPT = J_S + PERMUTS - 1, J_SORTED = J_OPT + nopt, J_AGG = J_SORTED + ns,
                 J_TABLE = J_AGG + 1, J_RT = J_TABLE + 1, J_PAT = J_RT + (sh.runtime ? 2 : 0);
    w.array(26);
    if (cnt(P_PUBLIC_EVALS)) e.evaluation(p.sec[P_PUBLIC_EVALS], 0, ech); else w.nil();
    w.array(COLUMNS);
    for (size_t i = 0; i < COLUMNS; i++) e.evaluation(E, J_W + i, ech);
    e.evaluation(E, J_Z, ech);
    w.array(PERMUTS - 1);
    for (size_t i = 0; i + 1 < PERMUTS; i++) e.evaluation(E, J_S + i, ech);
    w.array(COLUMNS);
    for (size_t i = 0; i < COLUMNS; i++) e.evaluation(E, J_CO + i, ech);
    for (size_t i = 0; i < 6; i++) e.evaluation(E, J_FIXED + i, ech);
    for (size_t i = 0, j = 0; i < 6; i++) { if (sh.optional >> i & 1) e.evaluation(E, J_OPT + j++, ech); else w.nil(); }
    if (sh.lookup) { e.evaluation(E, J_AGG, ech); e.evaluation(E, J_TABLE, ech); } else { w.nil(); w.nil(); }
    w.array(5);
    for (size_t i = 0; i < 5; i++) { if (i < ns) e.evaluation(E, J_SORTED + i, ech); else w.nil(); }
    if (sh.runtime) { e.evaluation(E, J_RT, ech); e.evaluation(E, J_RT + 1, ech); } else { w.nil(); w.nil(); }
    for (size_t i = 0, j = 0; i < 4; i++) { if (sh.patterns >> i & 1) e.evaluation(E, J_PAT + j++, ech); else w.nil(); }
    e.records(p.sec[P_FT_EVAL1], 0, 1, ELEM);
    w.array(p.prev.size());
    for (const PrevChallenge& pc : p.prev) {
        w.array(2);
        w.array(pc.chals.count);
        e.records(pc.chals, 0, pc.chals.count, ELEM);
        e.comm(pc.comm, 0, pc.comm.count);
    }
    *out = std::move(w.out);
    return 0;
}

inline int write_index(const Index& v, std::vector<uint8_t>* out, char* err, size_t cap) {
    auto cnt = [&](int s) { return v.sec[s].count; };
    const size_t nch = v.chunks, nopt = (size_t)popcount8(v.optional), npat = (size_t)popcount8(v.patterns);
    const size_t width = nch ? cnt(V_LOOKUP_TABLE_COMM) / nch : 0;
    if (nch == 0 || cnt(V_SIGMA_COMM) != PERMUTS * nch || cnt(V_COEFFICIENTS_COMM) != COLUMNS * nch || cnt(V_GENERIC_COMM) != nch || cnt(V_SELECTOR_COMM) != 5 * nch ||
        cnt(V_OPTIONAL_COMM) != nopt * nch || cnt(V_SHIFTS) != PERMUTS) {
        snprintf(err, cap, "VerifierIndex: the sections do not hold %zu chunks per commitment and 7 shifts", nch);
        return -1;
    }
    if (v.lookup ? (width == 0 || cnt(V_LOOKUP_TABLE_COMM) != width * nch || cnt(V_LOOKUP_SELECTOR_COMM) != npat * nch || (cnt(V_LOOKUP_TABLE_IDS_COMM) != 0 && cnt(V_LOOKUP_TABLE_IDS_COMM) != nch) ||
                    cnt(V_LOOKUP_RUNTIME_SELECTOR_COMM) != (v.uses_runtime_tables ? nch : 0))
                 : (cnt(V_LOOKUP_TABLE_COMM) || cnt(V_LOOKUP_SELECTOR_COMM) || cnt(V_LOOKUP_TABLE_IDS_COMM) || cnt(V_LOOKUP_RUNTIME_SELECTOR_COMM))) {
        snprintf(err, cap, "VerifierIndex: the lookup sections do not fit the lookup index (%zu patterns, runtime tables %d)", npat, (int)v.uses_runtime_tables);
        return -1;
    }
    Emit e;
    Writer& w = e.w;
    uint8_t d[DOMAIN_RECORD];
    for (int i = 0; i < 8; i++) d[i] = (uint8_t)(v.domain_size >> (8 * i));
    for (int i = 0; i < 4; i++) d[8 + i] = (uint8_t)(v.log_size >> (8 * i));
    memcpy(d + 12, v.domain, sizeof(v.domain));
    w.array(21);
    w.bin(d, DOMAIN_RECORD);
    w.uint(v.max_poly_size); w.uint(v.zk_rows); w.uint(v.public_inputs); w.uint(v.prev_challenges);
    w.array(PERMUTS);
    for (size_t i = 0; i < PERMUTS; i++) e.comm(v.sec[V_SIGMA_COMM], i * nch, nch);
    w.array(COLUMNS);
    for (size_t i = 0; i < COLUMNS; i++) e.comm(v.sec[V_COEFFICIENTS_COMM], i * nch, nch);
    e.comm(v.sec[V_GENERIC_COMM], 0, nch);
    for (size_t i = 0; i < 5; i++) e.comm(v.sec[V_SELECTOR_COMM], i * nch, nch);
    for (size_t i = 0, j = 0; i < 6; i++) { if (v.optional >> i & 1) e.comm(v.sec[V_OPTIONAL_COMM], nch * j++, nch); else w.nil(); }
    w.array(PERMUTS);
    e.records(v.sec[V_SHIFTS], 0, PERMUTS, ELEM);
    if (!v.lookup) w.nil();
    else {
        w.array(6);
        w.boolean(v.joint_lookup_used);
        w.array(width);
        for (size_t i = 0; i < width; i++) e.comm(v.sec[V_LOOKUP_TABLE_COMM], i * nch, nch);
        w.array(4);
        for (size_t i = 0, j = 0; i < 4; i++) { if (v.patterns >> i & 1) e.comm(v.sec[V_LOOKUP_SELECTOR_COMM], nch * j++, nch); else w.nil(); }
        if (cnt(V_LOOKUP_TABLE_IDS_COMM)) e.comm(v.sec[V_LOOKUP_TABLE_IDS_COMM], 0, nch); else w.nil();
        w.array(3);
        w.uint(v.max_per_row); w.uint(v.max_joint_size);
        w.array(3);
        w.array(4);
        for (size_t i = 0; i < 4; i++) w.boolean(v.patterns >> i & 1);
        w.boolean(v.joint_lookup_used); w.boolean(v.uses_runtime_tables);
        if (v.uses_runtime_tables) e.comm(v.sec[V_LOOKUP_RUNTIME_SELECTOR_COMM], 0, nch); else w.nil();
    }
    *out = std::move(w.out);
    return 0;
}

}  // namespace kh_proof_wire
