// The lookup tables' hash, tuple hash and capacity rule (csrc/lookup_hash.hpp) on the host, printed for tests/test_lookup_hash.py to compare with the
// Python mirror of tests/lookup_collisions.py.  Stand-alone: lookup_hash.hpp alone, no library, no GPU (the test builds it under AddressSanitizer and UBSan).
// stdin, one request per line, numbers in hex:   K l0 l1 l2 l3  ->  hash(Key)      T + 16 limbs (id, entry 0..2)  ->  hash(Tuple)      L n  ->  lookup_slots(n)
// stdout: one hex number per request.  Exits non-zero at a line it cannot read.
#include "../../proof_systems_amd/csrc/lookup_hash.hpp"
#include <inttypes.h>
#include <stdio.h>

using namespace kh;

static bool read_key(Key& k) { return scanf("%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &k.l[0], &k.l[1], &k.l[2], &k.l[3]) == 4; }

int main() {
    char op[2];
    size_t line = 0;
    while (scanf("%1s", op) == 1) {
        line++;
        bool ok = true;
        if (op[0] == 'K') {
            Key k;
            ok = read_key(k);
            if (ok) printf("%" PRIx64 "\n", hash(k));
        } else if (op[0] == 'T') {
            Tuple t;
            for (int i = 0; i < 4 && ok; i++) ok = read_key(t.k[i]);
            if (ok) printf("%" PRIx32 "\n", hash(t));
        } else if (op[0] == 'L') {
            uint64_t n;
            ok = scanf("%" SCNx64, &n) == 1;
            if (ok) printf("%zx\n", lookup_slots((size_t)n));
        } else ok = false;
        if (!ok) { fprintf(stderr, "request %zu: cannot read it\n", line); return 1; }
    }
    return 0;
}
