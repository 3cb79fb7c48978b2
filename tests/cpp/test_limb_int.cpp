// csrc/limb_int.cuh on the host: the foreign modulus' constants (mu = floor(2^528 / f), 2^264 - f), the division of ForeignFieldMul, its carries, and
// ForeignFieldAdd -- the very functions the kernels of csrc/limb_gadgets.hip run per lane.  Reads one case per line (op, three limbs of f, a and b in
// hex, the sign) and prints what the functions return; tests/test_limb_int.py builds this with g++ and both sanitizers, writes the cases and compares
// with Python's integers (CPU, no GPU, no library).
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../../proof_systems_amd/csrc/limb_int.cuh"
using namespace kh::limb;
typedef unsigned __int128 u128;

static Limb parse(const std::string& s) {
    u128 v = 0;
    for (char c : s) v = v * 16 + (c <= '9' ? c - '0' : c - 'a' + 10);
    return from_u64<3>((u64)v, (u64)(v >> 64));
}
template <int N>
static std::string hex(const Wide<N>& x) {
    std::string s;
    char b[16];
    for (int i = N - 1; i >= 0; i--) { snprintf(b, sizeof b, "%08x", x.w[i]); s += b; }
    return s;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string op, t;
        is >> op;
        Limbs f, a, b;
        for (int k = 0; k < 3; k++) { is >> t; f.l[k] = parse(t); }
        for (int k = 0; k < 3; k++) { is >> t; a.l[k] = parse(t); }
        for (int k = 0; k < 3; k++) { is >> t; b.l[k] = parse(t); }
        int sign;
        is >> sign;
        if (op == "M") {        // q r mu | p1_lo p1_hi0 carry1 bound p1_hi1 carry0 r01 | q_overflow cell_overflow | nf0 nf1 nf2
            const FfModulus m = ff_modulus(f);
            const DivMod d = ff_divmod(pack(a), pack(b), m);
            const Limbs q = unpack(d.q), r = unpack(d.r);
            const FfMulCells c = ff_mul_cells(a, b, q, r, m);
            printf("%s %s %s %s %s %s %s %x %x %s %d %d %s %s %s\n", hex(d.q).c_str(), hex(d.r).c_str(), hex(m.mu).c_str(), hex(c.p1_lo).c_str(),
                   hex(c.p1_hi0).c_str(), hex(c.carry1).c_str(), hex(c.bound).c_str(), c.p1_hi1, c.carry0, hex(c.r01).c_str(), (int)d.q_overflow, (int)c.overflow,
                   hex(m.nf.l[0]).c_str(), hex(m.nf.l[1]).c_str(), hex(m.nf.l[2]).c_str());
        } else {                // r0 r1 r2 overflow carry bad
            const FfAdd s = ff_add(a, b, sign, pack(f), f.l[2]);
            printf("%s %s %s %d %d %d\n", hex(s.r.l[0]).c_str(), hex(s.r.l[1]).c_str(), hex(s.r.l[2]).c_str(), s.overflow, s.carry, (int)s.bad);
        }
    }
    return 0;
}
