// A C caller with nothing but include/kimchi_hip.h: builds the index of a circuit WITH a lookup argument from its gate list and its lookup
// table with kh_prover_index_create_lookup, proves with the randomness it is given and writes the verifier-index digest, the lookup sections of
// the verifier index and the proof's sections.  tests/test_gpu_index_create_lookup.py compiles it and compares everything with the Python-built
// index (ProverIndex + LookupIndex + attach_lookup) of the same circuit proving from the same randomness.
//   circuit: `rows` GateType::Lookup rows wired to themselves; one fixed table with id 3, two columns, `entries` rows (3 j + 1, j^2 + 2);
//   witness: w0 = 3 (the table id), (w1, w2), (w3, w4), (w5, w6) = the entries (3 r + k) mod entries, k = 0..2, of row r.
// Usage: test_index_create_lookup <rows> <entries> <in: count, then count x 4 randomness limbs, binary u64> <out>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kimchi_hip.h"

#define CK(expr) do { int rc_ = (expr); if (rc_ != KH_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, kh_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: test_index_create_lookup rows entries in out\n"); return 2; }
    const size_t rows = (size_t)std::atoi(argv[1]), entries = (size_t)std::atoi(argv[2]);
    std::FILE* f = std::fopen(argv[3], "rb");
    if (!f) return 2;
    uint64_t count = 0;
    if (std::fread(&count, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> rnd(4 * count);
    if (std::fread(rnd.data(), 8, rnd.size(), f) != rnd.size()) return 2;
    std::fclose(f);
    CK(kh_init(0));
    // ---- the table, column-major, in Montgomery form through the library's field hook (this program has no bignum code)
    std::vector<uint64_t> plain(4 * 2 * entries, 0), table(4 * 2 * entries);
    for (size_t j = 0; j < entries; j++) { plain[4 * j] = 3 * j + 1; plain[4 * (entries + j)] = j * j + 2; }
    CK(kh_debug_field_op(KH_FIELD_FP, 3, plain.data(), plain.data(), table.data(), 2 * entries));
    const uint64_t plain_id[4] = {3, 0, 0, 0};
    uint64_t id[4];
    CK(kh_debug_field_op(KH_FIELD_FP, 3, plain_id, plain_id, id, 1));
    // ---- the gate list
    std::vector<int> types(rows, KH_GATE_LOOKUP);
    std::vector<uint32_t> wires(14 * rows);
    std::vector<uint64_t> coeffs(60 * rows, 0), wit(4 * 15 * rows, 0);
    for (size_t r = 0; r < rows; r++) {
        for (uint32_t c = 0; c < 7; c++) { wires[14 * r + 2 * c] = (uint32_t)r; wires[14 * r + 2 * c + 1] = c; }
        for (int k = 0; k < 4; k++) wit[4 * r + k] = id[k];
        for (size_t l = 0; l < 3; l++) {
            const size_t e = (3 * r + l) % entries;
            for (int k = 0; k < 4; k++) { wit[4 * ((1 + 2 * l) * rows + r) + k] = table[4 * e + k]; wit[4 * ((2 + 2 * l) * rows + r) + k] = table[4 * (entries + e) + k]; }
        }
    }
    size_t log_srs = 0;
    while (((size_t)1 << log_srs) < rows + entries + 8) log_srs++;
    kh_srs_t* srs = nullptr;
    CK(kh_srs_create_device(KH_CURVE_VESTA, (size_t)1 << log_srs, &srs));
    const kh_lookup_table_t tab = {3, 2, entries, table.data()};
    kh_prover_index_t* index = nullptr;
    CK(kh_prover_index_create_lookup(srs, rows, types.data(), wires.data(), coeffs.data(), 0, &tab, 1, nullptr, 0, &index));
    for (uint64_t& v : plain) v = ~0ull;           // the index keeps nothing of the caller's arrays ...
    std::vector<uint64_t> table_copy(table);
    for (uint64_t& v : table) v = ~0ull;           // ... the table included
    unsigned logn = 0, zk = 0; size_t nch = 0;
    CK(kh_prover_index_shape(index, &logn, &zk, &nch));
    if (logn != log_srs || zk != 3 || nch != 1) { std::fprintf(stderr, "shape %u %u %zu\n", logn, zk, nch); return 4; }
    if (kh_prove_randomness_count(index, 1) != count) { std::fprintf(stderr, "randomness count %zu, given %llu\n", kh_prove_randomness_count(index, 1), (unsigned long long)count); return 5; }
    if (kh_prover_index_attach_runtime_tables(index, table.data(), table.data(), table.data(), 0, 1) != KH_E_INVALID) { std::fprintf(stderr, "attach on a created index\n"); return 6; }
    kh_proof_t* proof = nullptr;
    CK(kh_prove(index, wit.data(), rows, nullptr, rnd.data(), count, KH_PROVE_CHECK, &proof));
    std::FILE* o = std::fopen(argv[4], "wb");
    if (!o) return 2;
    const uint64_t* limbs = nullptr; const uint8_t* flags = nullptr; size_t cnt = 0;
    CK(kh_verifier_index_section(index, KH_VINDEX_DIGEST, &limbs, &flags, &cnt));
    std::fwrite(limbs, 8, 4, o);
    auto put = [&](bool points) {
        const uint64_t head[2] = {(uint64_t)cnt, points ? 1u : 0u};
        std::fwrite(head, 8, 2, o);
        std::fwrite(limbs, 8, (points ? 8 : 4) * cnt, o);
        if (points) std::fwrite(flags, 1, cnt, o);
    };
    for (int s = KH_VINDEX_LOOKUP_TABLE_COMM; s <= KH_VINDEX_LOOKUP_INFO; s++) {
        CK(kh_verifier_index_section(index, s, &limbs, &flags, &cnt));
        put(s != KH_VINDEX_LOOKUP_INFO);
    }
    for (int s = 0; s <= KH_PROOF_LOOKUP_RUNTIME_COMM; s++) {
        CK(kh_proof_section(proof, s, &limbs, &flags, &cnt));
        put(flags != nullptr);
    }
    std::fclose(o);
    std::printf("INDEX_CREATE_LOOKUP_OK\n");
    kh_proof_free(proof); kh_prover_index_free(index); kh_srs_free(srs);
    return 0;
}
