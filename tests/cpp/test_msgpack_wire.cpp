// test_msgpack_wire.cpp -- csrc/msgpack_wire.hpp and csrc/proof_wire.hpp on the host alone, over the inner ProverProof / VerifierIndex bytes of stored
// reference proofs (tests/test_msgpack_wire.py hands them over as files: proof, index, proof, index, ...).  Every buffer a reader sees is a heap block of
// exactly the length it is told, so a read past the end is an AddressSanitizer report; the program is built with -fsanitize=address,undefined.
//   round trip       parse, walk, write: the identical bytes
//   truncation       every length 0 .. len - 1 is refused; one trailing byte is refused
//   foreign bytes    every type byte replaced by a map, a str, the reserved byte, a float, a negative int, a bin32 and an array32 of 2^32 - 1: a refusal or a
//                    structurally valid parse, no length accepted beyond the bytes that remain
//   depth            8 nested arrays pass, 9 are refused
//   arity            each refusal of the structure walk, provoked by a minimal edit of a real file
#include <stdio.h>
#include <stdlib.h>
#include <string>

#include "../../proof_systems_amd/csrc/proof_wire.hpp"

using namespace kh_proof_wire;
typedef std::vector<uint8_t> Bytes;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// a heap block of exactly b.size() bytes
struct Exact {
    uint8_t* p; size_t n;
    explicit Exact(const Bytes& b) : p((uint8_t*)malloc(b.size() ? b.size() : 1)), n(b.size()) { if (n) memcpy(p, b.data(), n); }
    Exact(const Exact&) = delete;
    ~Exact() { free(p); }
};

static Bytes read_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); exit(2); }
    Bytes b; uint8_t buf[4096]; size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + k);
    fclose(f);
    return b;
}

static char err[256];
static int parse_proof(const Bytes& b, Proof* out) { Exact e(b); err[0] = 0; return read_proof(e.n ? e.p : e.p, e.n, out, err, sizeof(err)); }
static int parse_index(const Bytes& b, Index* out, const uint8_t* dom = nullptr, uint64_t mps = 0) { Exact e(b); err[0] = 0; return read_index(e.p, e.n, dom, mps, out, err, sizeof(err)); }
// the generic parse: one value of the subset and nothing behind it; every claimed length is checked against what remains
static bool generic_walk(Reader& r, std::vector<size_t>* type_bytes) {
    if (r.failed || r.pos >= r.len) return r.refuse("a value");
    if (type_bytes) type_bytes->push_back(r.pos);
    const uint8_t t = r.p[r.pos];
    if ((t & 0xf0) == 0x90 || t == 0xdc || t == 0xdd) {
        size_t n = 0;
        if (!r.enter(&n)) return false;
        CHECK(n <= r.left(), "an array of %zu entries accepted with %zu bytes left", n, r.left());
        for (size_t i = 0; i < n; i++) if (!generic_walk(r, type_bytes)) return false;
        r.leave();
        return true;
    }
    if (t >= 0xc4 && t <= 0xc6) {
        const uint8_t* b = nullptr; size_t n = 0;
        const size_t before = r.pos;
        if (!r.bin(&b, &n)) return false;
        CHECK(b + n <= r.p + r.len && r.pos > before, "a bin of %zu bytes accepted past the end", n);
        return true;
    }
    return r.skip();
}
static bool generic_parse(const Bytes& b, std::vector<size_t>* type_bytes = nullptr) {
    Exact e(b);
    Reader r(e.p, e.n);
    return generic_walk(r, type_bytes) && r.finish();
}
// the offset of the value at `path` (indexes into nested arrays)
static size_t locate(const Bytes& b, std::initializer_list<size_t> path) {
    Reader r(b.data(), b.size());
    for (size_t idx : path) {
        size_t n = 0;
        if (!r.enter(&n) || idx >= n) { printf("locate: bad path\n"); exit(2); }
        for (size_t i = 0; i < idx; i++) if (!r.skip()) { printf("locate: bad path\n"); exit(2); }
    }
    return r.pos;
}
static size_t value_len(const Bytes& b, size_t at) { Reader r(b.data(), b.size()); r.pos = at; r.skip(); return r.pos - at; }
static Bytes with_byte(Bytes b, size_t at, uint8_t v) { b[at] = v; return b; }
// the one-entry array at `at` given a second copy of its entry
static Bytes doubled(Bytes b, size_t at) {
    CHECK(b[at] == 0x91, "no one-entry array at %zu", at);
    const size_t n = value_len(b, at + 1);
    const Bytes item(b.begin() + at + 1, b.begin() + at + 1 + n);
    b[at] = 0x92;
    b.insert(b.begin() + at + 1, item.begin(), item.end());
    return b;
}

static void refused_proof(const char* what, const Bytes& b, const char* word) {
    Proof p;
    const int rc = parse_proof(b, &p);
    CHECK(rc == -1 && strstr(err, word) && strstr(err, "offset"), "%s: rc %d, message '%s' (wanted '%s')", what, rc, err, word);
}
static void refused_index(const char* what, const Bytes& b, const char* word, const uint8_t* dom = nullptr, uint64_t mps = 0) {
    Index v;
    const int rc = parse_index(b, &v, dom, mps);
    CHECK(rc == -1 && strstr(err, word) && strstr(err, "offset"), "%s: rc %d, message '%s' (wanted '%s')", what, rc, err, word);
}

static const struct { uint8_t b[5]; size_t n; } FOREIGN[] = {{{0x80}, 1}, {{0xa0}, 1}, {{0xc1}, 1}, {{0xca}, 1}, {{0xd0}, 1}, {{0xc6, 0xff, 0xff, 0xff, 0xff}, 5},
                                                              {{0xdd, 0xff, 0xff, 0xff, 0xff}, 5}};

template <class Parse>
static void hostile(const char* name, const Bytes& file, Parse parse) {
    // truncation, a trailing byte
    for (size_t len = 0; len < file.size(); len++) {
        const Bytes cut(file.begin(), file.begin() + len);
        CHECK(parse(cut) == -1, "%s: accepted when cut to %zu of %zu bytes", name, len, file.size());
        CHECK(!generic_parse(cut), "%s: the generic parse accepted %zu of %zu bytes", name, len, file.size());
    }
    Bytes more = file; more.push_back(0xc0);
    CHECK(parse(more) == -1 && strstr(err, "end of the buffer"), "%s: a trailing byte: '%s'", name, err);
    // foreign type bytes
    std::vector<size_t> at;
    CHECK(generic_parse(file, &at) && at.size() > 100, "%s: the generic parse of the file itself", name);
    size_t refused = 0, accepted = 0;
    for (size_t off : at)
        for (const auto& f : FOREIGN) {
            Bytes b = file;
            for (size_t i = 0; i < f.n && off + i < b.size(); i++) b[off + i] = f.b[i];
            const int rc = parse(b);
            CHECK(rc == 0 || (rc == -1 && err[0]), "%s: offset %zu byte 0x%02x: rc %d", name, off, f.b[0], rc);
            (rc == 0 ? accepted : refused)++;
            generic_parse(b);
        }
    CHECK(accepted == 0, "%s: %zu foreign type bytes gave a proof / an index", name, accepted);
    printf("%s: %zu bytes, %zu type bytes, %zu hostile edits refused\n", name, file.size(), at.size(), refused);
}

int main(int argc, char** argv) {
    if (argc < 3 || argc % 2 != 1) { printf("usage: test_msgpack_wire proof index [proof index ...]\n"); return 2; }
    // ---- the framing alone
    {
        const uint8_t big[10] = {0xdd, 0xff, 0xff, 0xff, 0xff, 0, 0, 0, 0, 0};
        CHECK(!generic_parse(Bytes(big, big + 10)), "an array32 of 2^32 - 1 entries in 10 bytes was accepted");
        Exact e(Bytes(big, big + 10));
        Reader r(e.p, e.n); size_t n = 0;
        CHECK(!r.enter(&n) && strstr(r.err, "offset 0") && strstr(r.err, "more entries"), "array32: '%s'", r.err);
        const uint8_t bigbin[6] = {0xc6, 0xff, 0xff, 0xff, 0xff, 0};
        CHECK(!generic_parse(Bytes(bigbin, bigbin + 6)), "a bin32 of 2^32 - 1 bytes in 6 bytes was accepted");
        Bytes d8(8, 0x91), d9(9, 0x91);
        d8.push_back(0xc0); d9.push_back(0xc0);
        CHECK(generic_parse(d8), "8 nested arrays were refused");
        CHECK(!generic_parse(d9), "9 nested arrays were accepted");
        for (int t : {0x80, 0xa0, 0xc1, 0xc7, 0xca, 0xcb, 0xd0, 0xd3, 0xd9, 0xde, 0xe0, 0xff}) {
            const Bytes one(1, (uint8_t)t);
            Exact x(one);
            Reader q(x.p, x.n);
            char want[40]; snprintf(want, sizeof(want), "found type byte 0x%02x", t);
            CHECK(!q.skip() && strstr(q.err, "offset 0: expected") && strstr(q.err, want), "type byte 0x%02x: '%s'", t, q.err);
        }
        // the shortest encoding of each length class, and a non-minimal integer parsing to the same value
        kh_msgpack::Writer w;
        for (uint64_t v : {0ull, 127ull, 128ull, 255ull, 256ull, 65535ull, 65536ull, 0xffffffffull, 0x100000000ull}) w.uint(v);
        const uint8_t want[] = {0x00, 0x7f, 0xcc, 0x80, 0xcc, 0xff, 0xcd, 0x01, 0x00, 0xcd, 0xff, 0xff, 0xce, 0x00, 0x01, 0x00, 0x00, 0xce, 0xff, 0xff, 0xff, 0xff,
                                0xcf, 0, 0, 0, 1, 0, 0, 0, 0};
        CHECK(w.out.size() == sizeof(want) && !memcmp(w.out.data(), want, sizeof(want)), "the writer's integers are not the shortest");
        const uint8_t fat[] = {0xcf, 0, 0, 0, 0, 0, 0, 0, 5};
        Reader q(fat, sizeof(fat)); uint64_t v = 0;
        CHECK(q.uint(&v) && v == 5 && q.finish(), "a uint64 holding 5");
        kh_msgpack::Writer a; a.array(15); a.array(16); a.array(65536);
        const uint8_t wa[] = {0x9f, 0xdc, 0x00, 0x10, 0xdd, 0x00, 0x01, 0x00, 0x00};
        CHECK(a.out.size() == sizeof(wa) && !memcmp(a.out.data(), wa, sizeof(wa)), "the writer's array headers are not the shortest");
    }
    bool saw_lookup = false, saw_prev = false;
    for (int i = 1; i + 1 < argc; i += 2) {
        const Bytes pb = read_file(argv[i]), vb = read_file(argv[i + 1]);
        // ---- round trips
        Proof p; Index v;
        CHECK(parse_proof(pb, &p) == 0, "%s: %s", argv[i], err);
        CHECK(parse_index(vb, &v) == 0, "%s: %s", argv[i + 1], err);
        Bytes again;
        CHECK(write_proof(p, &again, err, sizeof(err)) == 0 && again == pb, "%s: the proof does not round-trip (%zu -> %zu bytes) %s", argv[i], pb.size(), again.size(), err);
        CHECK(write_index(v, &again, err, sizeof(err)) == 0 && again == vb, "%s: the index does not round-trip (%zu -> %zu bytes) %s", argv[i + 1], vb.size(), again.size(), err);
        CHECK(p.shape.known && p.shape.lookup == v.lookup && p.shape.runtime == v.uses_runtime_tables && p.shape.patterns == v.patterns && p.shape.optional == v.optional,
              "%s: the proof's shape is not its index's", argv[i]);
        CHECK(p.prev.size() == v.prev_challenges && p.sec[P_W_COMM].count == 15 * v.chunks && p.sec[P_LR].count == 32 && v.max_poly_size == 65536, "%s: counts", argv[i]);
        CHECK(parse_index(vb, &v, v.domain, 65536) == 0, "%s: the index against its own domain record: %s", argv[i + 1], err);
        saw_lookup |= v.lookup; saw_prev |= !p.prev.empty();
        hostile(argv[i], pb, [](const Bytes& b) { Proof q; return parse_proof(b, &q); });
        hostile(argv[i + 1], vb, [](const Bytes& b) { Index q; return parse_index(b, &q); });
        // ---- arity and consistency: the proof
        refused_proof("4 top-level entries", with_byte(pb, 0, 0x94), "ProverProof");
        refused_proof("w_comm with 14", with_byte(pb, locate(pb, {0, 0}), 0x9e), "w_comm");
        refused_proof("evals.w with 14", with_byte(pb, locate(pb, {2, 1}), 0x9e), "evals.w");
        refused_proof("evals.s with 5", with_byte(pb, locate(pb, {2, 3}), 0x95), "evals.s");
        refused_proof("evals.coefficients with 14", with_byte(pb, locate(pb, {2, 4}), 0x9e), "evals.coefficients");
        refused_proof("evals.lookup_sorted with 4 slots", with_byte(pb, locate(pb, {2, 19}), 0x94), "lookup_sorted");
        refused_proof("evals with 25", with_byte(pb, locate(pb, {2}) + 2, 25), "evals");
        refused_proof("an (L, R) pair of one", with_byte(pb, locate(pb, {1, 0, 3}), 0x91), "(L, R)");
        refused_proof("an opening of 4", with_byte(pb, locate(pb, {1}), 0x94), "opening");
        refused_proof("a PolyComm of 2 fields", with_byte(pb, locate(pb, {0, 1}), 0x92), "z_comm");
        {
            Bytes b = pb;                                                   // evals.z: one value at zeta, none at zeta omega
            const size_t at = locate(b, {2, 2, 1});
            b[at] = 0x90; b.erase(b.begin() + at + 1, b.begin() + at + 35);
            refused_proof("evals.z 1 / 0", b, "1 values at zeta and 0 at zeta omega");
            b = doubled(pb, locate(pb, {2, 2, 0}));                         // two chunks at both points, every other evaluation has one
            b = doubled(b, locate(b, {2, 2, 1}));
            refused_proof("evals.z with two chunks", b, "the first evaluation has 1");
            refused_proof("w_comm[3] with two chunks", doubled(pb, locate(pb, {0, 0, 3, 0})), "w_comm[3] has 2 chunks");
            b = pb;                                                         // ft_eval1 as a bin of 31 bytes
            const size_t ft = locate(b, {3});
            b[ft + 1] = 31; b.erase(b.begin() + ft + 2);
            refused_proof("a 31-byte element", b, "a bin of 32 bytes, found one of 31");
            b = pb;                                                         // delta as a bin of 32 bytes
            const size_t dl = locate(b, {1, 1});
            b[dl + 1] = 32; b.erase(b.begin() + dl + 2);
            refused_proof("a 32-byte point", b, "a bin of 33 bytes, found one of 32");
        }
        if (p.shape.lookup) {                                               // the lookup commitments taken out, their evaluations left in
            Bytes b = pb;
            const size_t at = locate(b, {0, 3}), n = value_len(b, at);
            b.erase(b.begin() + at + 1, b.begin() + at + n); b[at] = 0xc0;
            refused_proof("lookup evaluations without commitments", b, "do not match the lookup commitments");
        }
        // ---- arity and consistency: the index
        const size_t dom = locate(vb, {0}) + 2;
        refused_index("sigma_comm with 6", with_byte(vb, locate(vb, {5}), 0x96), "sigma_comm");
        refused_index("coefficients_comm with 14", with_byte(vb, locate(vb, {6}), 0x9e), "coefficients_comm");
        refused_index("shift with 6", with_byte(vb, locate(vb, {19}), 0x96), "shift");
        refused_index("20 top-level entries", with_byte(vb, 2, 20), "VerifierIndex");
        refused_index("log_size + 1", with_byte(vb, dom + 8, (uint8_t)(vb[dom + 8] + 1)), "is not 2^log_size");
        refused_index("size + 1", with_byte(vb, dom, (uint8_t)(vb[dom] + 1)), "is not 2^log_size");
        for (size_t k = 0; k < DOMAIN_ELEMS; k++)
            refused_index("a domain element changed", with_byte(vb, dom + 12 + 32 * k, (uint8_t)(vb[dom + 12 + 32 * k] ^ 1)), DOMAIN_NAMES[k], v.domain, 65536);
        {
            Bytes b = vb;                                                   // max_poly_size 32768 (uint32 0x00010000 -> 0x00008000: same parse, other value)
            const size_t at = locate(b, {1});
            CHECK(b[at] == 0xce, "max_poly_size is not a uint32");
            b[at + 2] = 0x00; b[at + 3] = 0x80;
            refused_index("max_poly_size 32768", b, "max_poly_size 32768", v.domain, 65536);
        }
        if (v.lookup) {
            refused_index("joint_lookup_used twice", with_byte(vb, locate(vb, {20, 0}), (uint8_t)(vb[locate(vb, {20, 0})] ^ 1)), "joint_lookup_used");
            for (size_t q = 0; q < 4; q++) {                                // a pattern's feature bit flipped: its selector commitment is now surplus / missing
                const size_t at = locate(vb, {20, 4, 2, 0, q});
                refused_index("a pattern bit flipped", with_byte(vb, at, (uint8_t)(vb[at] ^ 1)), (v.patterns >> q & 1) ? "is present, its feature bit is false" : "is absent, its feature bit is true");
            }
            const size_t rt = locate(vb, {20, 4, 2, 2});
            refused_index("uses_runtime_tables flipped", with_byte(vb, rt, (uint8_t)(vb[rt] ^ 1)), "uses_runtime_tables");
            refused_index("lookup_selectors with 3", with_byte(vb, locate(vb, {20, 2}), 0x93), "lookup_selectors");
        }
    }
    CHECK(saw_lookup && saw_prev, "the files must include a lookup proof with runtime tables and a recursive one");
    if (failures) { printf("msgpack_wire: %d failures\n", failures); return 1; }
    printf("msgpack_wire OK\n");
    return 0;
}
