// A caller of kh_verify that is not Python: the reference's benchmark circuit (kimchi/src/bench.rs:59-96: 2^7 - 10 generic gates `w0 - 1 = 0`, identity
// wiring) through kh_prover_index_create, one proof with the library's own randomness (kh_prove), its verifier index (kh_verifier_index_of), then
// kh_verify: accepted; the same proof rebuilt from its sections with one limb of an evaluation changed (kh_proof_from_sections): rejected with KH_OK;
// an evaluation >= p: refused with KH_E_INVALID.  Prints "test_verify OK" and returns 0.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_verify.cpp -lkimchi_hip
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kimchi_hip.h"

#define CK(expr) do { int rc_ = (expr); if (rc_ != KH_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, kh_last_error()); return 1; } } while (0)
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s is false (%s)\n", __FILE__, __LINE__, #cond, kh_last_error()); return 1; } } while (0)

int main() {
    const unsigned logn = 7;
    const size_t n = (size_t)1 << logn, rows = n - 10;
    CK(kh_init(0));
    kh_srs_t* srs = nullptr;
    CK(kh_srs_create_device(KH_CURVE_VESTA, n, &srs));
    uint64_t one[4], minus_one[4]; const uint64_t plain_one[4] = {1, 0, 0, 0}, zero[4] = {0, 0, 0, 0};
    CK(kh_debug_field_op(KH_FIELD_FP, 3 /* to_mont */, plain_one, plain_one, one, 1));
    CK(kh_debug_field_op(KH_FIELD_FP, 2 /* sub */, zero, one, minus_one, 1));
    int generic = -1;
    for (int g = 0; g < kh_gate_count(); g++) if (!std::strcmp(kh_gate_name(g), "Generic")) generic = g;
    EXPECT(generic >= 0);
    std::vector<int> types(rows, generic);
    std::vector<uint32_t> wires(14 * rows);
    std::vector<uint64_t> coeffs(60 * rows, 0), witness(4 * 15 * rows, 0);
    for (size_t r = 0; r < rows; r++) {
        for (uint32_t c = 0; c < 7; c++) { wires[14 * r + 2 * c] = (uint32_t)r; wires[14 * r + 2 * c + 1] = c; }
        std::memcpy(&coeffs[60 * r], one, 32); std::memcpy(&coeffs[60 * r + 16], minus_one, 32);       // c0 = 1, c4 = -1
        std::memcpy(&witness[4 * r], one, 32);                                                        // w0 = 1
    }
    kh_prover_index_t* index = nullptr;
    CK(kh_prover_index_create(srs, rows, types.data(), wires.data(), coeffs.data(), 0, &index));
    kh_proof_t* proof = nullptr;
    CK(kh_prove(index, witness.data(), rows, nullptr, nullptr, 0, KH_PROVE_CHECK, &proof));
    kh_verifier_index_t* vix = nullptr;
    CK(kh_verifier_index_of(index, &vix));
    kh_verify_item_t item;
    std::memset(&item, 0, sizeof(item));
    item.index = vix; item.proof = proof;
    int ok = -1;
    kh_verify_trace_t trace;
    CK(kh_verify(&item, &ok, &trace));
    EXPECT(ok == 1);
    // the proof again from its sections, one limb of z(zeta) changed to another canonical value
    kh_section_t secs[KH_PROOF_LOOKUP_RUNTIME_COMM + 1];
    for (int s = 0; s <= KH_PROOF_LOOKUP_RUNTIME_COMM; s++) CK(kh_proof_section(proof, s, &secs[s].limbs, &secs[s].flags, &secs[s].count));
    std::vector<uint64_t> evals(secs[KH_PROOF_EVALS].limbs, secs[KH_PROOF_EVALS].limbs + 4 * secs[KH_PROOF_EVALS].count);
    evals[0] ^= 1;
    secs[KH_PROOF_EVALS].limbs = evals.data();
    kh_proof_t* bad = nullptr;
    CK(kh_proof_from_sections(secs, KH_PROOF_LOOKUP_RUNTIME_COMM + 1, &bad));
    item.proof = bad; ok = -1;
    CK(kh_verify(&item, &ok, nullptr));
    EXPECT(ok == 0);
    kh_proof_free(bad); bad = nullptr;
    // ... and to a value that is no field element: refused, *ok untouched
    evals[0] ^= 1; evals[3] = ~(uint64_t)0;
    CK(kh_proof_from_sections(secs, KH_PROOF_LOOKUP_RUNTIME_COMM + 1, &bad));
    item.proof = bad; ok = -1;
    EXPECT(kh_verify(&item, &ok, nullptr) == KH_E_INVALID && ok == -1);
    kh_proof_free(bad);
    kh_verifier_index_free(vix);
    kh_proof_free(proof);
    kh_prover_index_free(index);
    kh_srs_free(srs);
    std::printf("test_verify OK\n");
    return 0;
}
