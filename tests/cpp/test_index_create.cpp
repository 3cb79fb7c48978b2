// A C caller with nothing but include/kimchi_hip.h: builds the index of the reference's benchmark circuit (kimchi/src/bench.rs:59-96: 2^k - 10
// generic gates `w0 - 1 = 0`, every cell wired to itself) from its GATE LIST with kh_prover_index_create, proves with the randomness it is given
// and writes the verifier-index digest and the proof's sections.  tests/test_gpu_index_create.py compiles it, checks the digest against the
// committed fixture record and the sections against the Python-built index proving from the same randomness.
// Usage: test_index_create <log2_n> <in: count, then count x 4 randomness limbs, binary u64> <out>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "kimchi_hip.h"

#define CK(expr) do { int rc_ = (expr); if (rc_ != KH_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, kh_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: test_index_create log2_n in out\n"); return 2; }
    const unsigned logn = (unsigned)std::atoi(argv[1]);
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    uint64_t count = 0;
    if (std::fread(&count, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> rnd(4 * count);
    if (std::fread(rnd.data(), 8, rnd.size(), f) != rnd.size()) return 2;
    std::fclose(f);
    const size_t n = (size_t)1 << logn, gates = n - 10;
    CK(kh_init(0));
    kh_srs_t* srs = nullptr;
    CK(kh_srs_create_device(KH_CURVE_VESTA, n, &srs));
    // Montgomery 1 and -1 through the library's field hook (this program has no bignum code)
    uint64_t one[4], minus_one[4];
    const uint64_t plain_one[4] = {1, 0, 0, 0}, zero[4] = {0, 0, 0, 0};
    CK(kh_debug_field_op(KH_FIELD_FP, 3, plain_one, plain_one, one, 1));
    CK(kh_debug_field_op(KH_FIELD_FP, 2, zero, one, minus_one, 1));
    // ---- the gate list: CircuitGate { typ: Generic, wires: identity, coeffs: [1, 0, 0, 0, -1, 0 ...] }
    int generic = -1;
    for (int g = 0; g < kh_gate_count(); g++) if (std::string_view(kh_gate_name(g)) == "Generic") generic = g;
    if (generic < 0) return 3;
    std::vector<int> types(gates, generic);
    std::vector<uint32_t> wires(14 * gates);
    std::vector<uint64_t> coeffs(60 * gates, 0);
    for (size_t r = 0; r < gates; r++) {
        for (uint32_t c = 0; c < 7; c++) { wires[14 * r + 2 * c] = (uint32_t)r; wires[14 * r + 2 * c + 1] = c; }
        for (int k = 0; k < 4; k++) { coeffs[60 * r + k] = one[k]; coeffs[60 * r + 16 + k] = minus_one[k]; }
    }
    kh_prover_index_t* index = nullptr;
    CK(kh_prover_index_create(srs, gates, types.data(), wires.data(), coeffs.data(), 0, &index));
    unsigned got_logn = 0, zk = 0; size_t nch = 0;
    CK(kh_prover_index_shape(index, &got_logn, &zk, &nch));
    if (got_logn != logn || zk != 3 || nch != 1) { std::fprintf(stderr, "shape %u %u %zu\n", got_logn, zk, nch); return 4; }
    if (kh_prove_randomness_count(index, 1) != count) { std::fprintf(stderr, "randomness count\n"); return 5; }
    // ---- the witness of the fixture: 15 columns of ones
    std::vector<uint64_t> wit(4 * 15 * gates);
    for (size_t i = 0; i < 15 * gates; i++) for (int k = 0; k < 4; k++) wit[4 * i + k] = one[k];
    kh_proof_t* proof = nullptr;
    CK(kh_prove(index, wit.data(), gates, nullptr, rnd.data(), count, KH_PROVE_CHECK, &proof));
    std::FILE* o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    const uint64_t* limbs = nullptr; const uint8_t* flags = nullptr; size_t cnt = 0;
    CK(kh_verifier_index_section(index, KH_VINDEX_DIGEST, &limbs, &flags, &cnt));
    std::fwrite(limbs, 8, 4, o);
    for (int s = 0; s <= KH_PROOF_CHALLENGES; s++) {
        CK(kh_proof_section(proof, s, &limbs, &flags, &cnt));
        const uint64_t head[2] = {(uint64_t)cnt, flags ? 1u : 0u};
        std::fwrite(head, 8, 2, o);
        std::fwrite(limbs, 8, (flags ? 8 : 4) * cnt, o);
        if (flags) std::fwrite(flags, 1, cnt, o);
    }
    std::fclose(o);
    std::printf("INDEX_CREATE_OK\n");
    kh_proof_free(proof); kh_prover_index_free(index); kh_srs_free(srs);
    return 0;
}
