"""csrc/limb_int.cuh on the host against Python's integers: the Barrett division of kh_foreign_field_mul_witness_dev (q and r exact for ANY modulus below
2^264 -- 1, 3, 2^88, 2^263, 2^264 - 1 and the three of the GPU tests --, a b = k f and k f - 1, the quotient-overflow test), the constants the host
computes per call (mu = floor(2^528 / f), 2^264 - f), the carries of the gate's cells, and ForeignFieldAdd's result, overflow and carry for both signs.
tests/cpp/test_limb_int.cpp is built with g++ under AddressSanitizer and UBSan here -- host code only, no GPU, no library."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 1 << 88
SECP = (1 << 256) - (1 << 32) - 977
PALLAS_BASE = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
MODULI = [SECP, PALLAS_BASE, (1 << 259) - 1, 3, 1, (1 << 264) - 1, 1 << 263, (1 << 263) + 1, 7, L, L * L + 5]


def limbs(x):
    return [x % L, (x >> 88) % L, x >> 176]


def make_cases():
    rng = random.Random(5)
    cases = []
    for f in MODULI:
        for _ in range(200):
            a = rng.randrange(f) if rng.random() < .7 else rng.randrange(1 << 264)
            b = rng.randrange(f) if rng.random() < .7 else rng.randrange(1 << 264)
            if f < 1 << 100 and rng.random() < .5:
                a, b = rng.randrange(1 << 60), rng.randrange(1 << 60)             # a small modulus with a quotient that fits
            cases.append(("M", f, a, b, 0))
        cases += [("M", f, f - 1, f - 1, 0), ("M", f, 0, 0, 0), ("M", f, 0, f - 1, 0), ("M", f, (1 << 264) - 1, (1 << 264) - 1, 0), ("M", f, f, (1 << 264) - 1, 0)]
        for _ in range(40):
            cases.append(("M", f, f, rng.randrange(1, 1 << 100), 0))                 # a b = k f
            if f > 3:
                a = rng.randrange(2, f)
                try:
                    cases.append(("M", f, a, (-pow(a, -1, f)) % f, 0))              # a b = k f - 1
                except ValueError:
                    pass
        for s in (1, -1):
            for _ in range(100):
                cases.append(("A", f, rng.randrange(f), rng.randrange(f), s))
            cases += [("A", f, f - 1, f - 1, s), ("A", f, 0, 0, s), ("A", f, 0, f - 1, s), ("A", f, f - 1, 0, s), ("A", f, f - 1, 1 % f, s),
                      ("A", f, (L * L - 1) % f, 1 % f, s), ("A", f, (L * L) % f, 1 % f, s), ("A", f, (L * L - 1) % f, (L * L) % f, s)]
    return cases


def test_division_carries_and_addition_equal_pythons_integers(tmp_path):
    exe = str(tmp_path / "test_limb_int")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_limb_int.cpp"), "-o", exe])
    cases = make_cases()
    text = "\n".join(" ".join([op] + ["%x" % v for x in (f, a, b) for v in limbs(x)] + [str(s)]) for op, f, a, b, s in cases) + "\n"
    run = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out = run.stdout.splitlines()
    assert len(out) == len(cases)
    exact = 0
    for (op, f, a, b, s), line in zip(cases, out):
        t = line.split()
        if op == "M":
            q, r = divmod(a * b, f)
            nf = limbs((1 << 264) - f)
            assert int(t[2], 16) == (1 << 528) // f and [int(x, 16) for x in t[12:15]] == nf, hex(f)
            assert int(t[10]) == (q >= 1 << 264), (hex(f), hex(a), hex(b))
            if q >= 1 << 264:
                continue
            assert (int(t[0], 16), int(t[1], 16)) == (q, r), (hex(f), hex(a), hex(b))
            A, B, Q, R = limbs(a), limbs(b), limbs(q), limbs(r)
            p0 = A[0] * B[0] + Q[0] * nf[0]
            p1 = A[0] * B[1] + A[1] * B[0] + Q[0] * nf[1] + Q[1] * nf[0]
            p2 = A[0] * B[2] + A[2] * B[0] + A[1] * B[1] + Q[0] * nf[2] + Q[2] * nf[0] + Q[1] * nf[1]
            p1_lo, p1_hi = p1 % L, p1 >> 88
            d0 = p0 + L * p1_lo - R[0] - L * R[1]
            assert d0 >= 0 and d0 % (L * L) == 0
            c0 = d0 >> 176
            d1 = p2 + p1_hi + c0 - R[2]
            assert d1 >= 0 and d1 % L == 0
            c1 = d1 >> 88
            assert c0 < 4 and p1_hi >> 88 < 4 and c1 < 1 << 91 and int(t[11]) == 0
            got = [int(x, 16) for x in t[3:10]]
            assert got == [p1_lo, p1_hi % L, c1, Q[2] + L - limbs(f)[2] - 1, p1_hi >> 88, c0, R[0] + L * R[1]], (hex(f), hex(a), hex(b))
            exact += 1
        else:
            v, ov = a + s * b, 0
            if v >= f:
                v, ov = v - f, 1
            elif v < 0:
                v, ov = v + f, -1
            num = a % (L * L) + s * (b % (L * L)) - ov * (f % (L * L)) - v % (L * L)
            assert num % (L * L) == 0 and num // (L * L) in (-1, 0, 1)
            assert ([int(x, 16) for x in t[:3]], int(t[3]), int(t[4]), int(t[5])) == (limbs(v), ov, num // (L * L), 0), (hex(f), hex(a), hex(b), s)
    assert exact > 1500
