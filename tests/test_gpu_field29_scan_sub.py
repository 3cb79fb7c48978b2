"""The product scans that subtract (csrc/field29.cuh: mulsub29 / sqrsub29) on the device.

1. The two scans by themselves, through khip.debug_field29_op on the caller's limbs: 4096 elements per field, under each of the three spread constants
   the additions subtract with -- the directed vectors of tools/gen_field29_asm.py (every column of the scan with m_k = 0 and m_k = 2^29 - 1), operands
   at the bounds of the accumulator, random ones, c at both ends of its range -- against Python big integers: the scan leaves (a b + m p) / 2^261 with
   m = -a b / p mod 2^261, the subtraction adds K p - c, and normalised limbs of an integer are unique.
2. The additions built on them, where they run: buckets of 1 / 2 / 3 / 40 entries through the wide path (k_acc_wide29: the opening aadd29, the loop's
   madd29; k_wide_a1 / k_wide_l2: add29) and through the narrow path (k_accumulate29), 2^12 scalars, both curves, bit-exact against the C oracle."""
import os
import random
import sys

import numpy as np
import pytest

from oracle import cref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_field29_asm as G  # noqa: E402

pytestmark = pytest.mark.gpu
THREADS = min(64, os.cpu_count() or 8)
MASK = G.MASK
N = 4096
SPREADS = [("s71", 7, 1), ("s51", 5, 1), ("s44", 4, 4)]


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    yield k
    k.set_wide_min_n(1 << 19)


def _operands(p, square):
    """N operand pairs as limb lists: directed, bounds, random.  square: a alone matters, limbs below 2^30 (the scan's column bound for a squaring)."""
    rnd = random.Random(f"scan_sub/{p & 0xffff}/{square}")
    M = G.Madd29Model(p)
    to29 = lambda x: M.mul(G.limbs29(x), M.c["KIN"])
    out = [(to29(x), to29(y)) for x, y, _k, _t in G.directed29(p, "sqrsub" if square else "mulsub")]
    top = {k: G.limbs29(k * p - 1) for k in (2, 4, 6)}
    full, wide = [MASK] * 9, [(3 << 29) - 1] * 9
    if square:
        out += [(a, a) for a in (top[2], top[4], top[6], full, [(1 << 30) - 1] * 9, G.limbs29(0), G.limbs29(1))]
    else:
        out += [(G.limbs29((p - 1) << 5), top[2]), (top[6], top[2]), (top[4], top[2]), (top[6], top[6]), (wide, full), (full, wide), (G.limbs29(0), top[2])]
    while len(out) < N:
        if square:
            a = [rnd.randrange(1 << 30) for _ in range(9)] if len(out) % 2 else G.limbs29(rnd.randrange(6 * p))
            out.append((a, a))
        else:
            a = [rnd.randrange(3 << 29) for _ in range(9)] if len(out) % 2 else G.limbs29(rnd.randrange(32 * p))
            out.append((a, G.limbs29(rnd.randrange(6 * p))))
    return out


@pytest.mark.parametrize("fname", ["FP", "FQ"])
@pytest.mark.parametrize("op", ["mulsub29", "sqrsub29"])
def test_scans_against_big_integers(khip, fname, op):
    p = G.P_FP if fname == "FP" else G.P_FQ
    fid = getattr(khip, fname)
    square = op == "sqrsub29"
    ab = _operands(p, square)
    a = np.array([x for x, _ in ab], dtype=np.uint32)
    b = None if square else np.array([y for _, y in ab], dtype=np.uint32)
    pinv = pow(p, -1, 1 << 261)
    prod = []
    for x, y in ab:
        v = G.val29(x) * G.val29(y)
        m = (-v * pinv) % (1 << 261)
        assert (v + m * p) % (1 << 261) == 0
        prod.append((v + m * p) >> 261)
    rnd = random.Random(f"scan_sub/c/{fname}/{op}")
    for key, K, J in SPREADS:
        C = G.spread(p, K, J)
        ends = [[0] * 9, [J * MASK] * 8 + [C[8]]]
        c = [ends[i % 2] if i < 64 else [rnd.randrange(J * MASK + 1) for _ in range(8)] + [rnd.randrange(C[8] + 1)] for i in range(N)]
        got = khip.debug_field29_op(fid, op, key, a, b, np.array(c, dtype=np.uint32))
        want = np.array([G.limbs29(t + K * p - G.val29(ci)) for t, ci in zip(prod, c)], dtype=np.uint64)
        assert want.max() < (1 << 32)
        bad = np.nonzero((got.astype(np.uint64) != want).any(axis=1))[0]
        assert bad.size == 0, f"{op} {key}: {bad.size} elements differ, first at {bad[0]}: got {got[bad[0]].tolist()} want {want[bad[0]].tolist()}"


# ---- the additions, where they run
def _digits(v, c):
    """signed c-bit window digits of the canonical scalar v, lowest window first (emit_digits of csrc/msm.hip)"""
    out, carry = [], 0
    for _ in range((255 + c - 1) // c):
        d = (v & ((1 << c) - 1)) + carry
        v >>= c
        carry = 1 if d > (1 << (c - 1)) else 0
        out.append(d - (carry << c))
    assert v == 0 and carry == 0
    return out


def _bucket_scalars(c, n, rng, reps):
    """scalars that fill buckets with exactly 1, 2, 3 and 40 entries (reps of each), signs at random: an entry of bucket b is a scalar whose one digit is b;
    a negative entry -b gets a positive companion digit one window up, in a bucket of its own"""
    top = 255 // c - 1
    vals, want, fresh, b = [], {}, 1 << 12, 0
    for _ in range(reps):
        for size in (1, 2, 3, 40):
            b += 1
            want[b] = size
            for _e in range(size):
                w = int(rng.integers(0, top))
                if rng.integers(0, 2):
                    fresh += 1
                    digs = {w: -b, w + 1: fresh}
                    want[fresh] = 1
                else:
                    digs = {w: b}
                v = sum(d << (c * k) for k, d in digs.items())
                got = _digits(v, c)
                assert 0 < v < (1 << 254) and all(got[k] == digs.get(k, 0) for k in range(len(got)))
                vals.append(v)
    assert b < (1 << 12) and fresh < (1 << (c - 1)) and len(vals) <= n
    sizes = {}
    for v in vals:
        for d in _digits(v, c):
            if d:
                sizes[abs(d)] = sizes.get(abs(d), 0) + 1
    assert sizes == want and {1, 2, 3, 40} == set(sizes.values())
    return vals + [0] * (n - len(vals))


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("wide", [True, False])
def test_buckets_of_1_2_3_40_entries(khip, cid, wide):
    n = 1 << 12
    khip.set_wide_min_n(n if wide else 1 << 19)
    vals = _bucket_scalars(20 if wide else 16, n, np.random.default_rng(110 + cid + 2 * wide), reps=40)
    g = khip.srs_generate(cid, 0, n)
    sc = cref.ints_to_limbs(vals)
    want, winf = cref.msm(cid, g, sc, scalars_mont=False, threads=THREADS)
    srs = khip.Srs(cid, g)
    got, ginf = srs.msm(sc, mont=False)
    ran_wide = any(name == "reduce_a1" for name, _ in khip.last_timings())
    srs.close()
    assert ran_wide == wide, "the MSM did not take the path this case is about"
    assert not winf and not ginf and np.array_equal(got, want)
