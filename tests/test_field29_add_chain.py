"""add29 (csrc/field29.cuh) chained the way the second level of the wide MSM's lazy reduction chains it (csrc/msm.hip, k_wide_l2): the SECOND operand is
itself an add29 result that went through a stored B29 record.  Level one (k_wide_a1) only ever feeds add29 results back in as the first operand.

Through the limb-exact model tools/gen_field29_asm.py (Madd29Model.add: every product runs the generated instruction stream, whose interpreter asserts
the 64-bit column bound at every v_mad_u64_u32, and every 32-bit operation asserts its range): sixteen leaves make a chunk record, F = 4 chunk
records make a run record.  The leaves, and then the chunk records themselves, are drawn at the bounds of Acc29 -- x < 6 p, y < 4 p, zz, zzz < 2 p,
limbs 0..7 normalised -- by adding the multiples of p the bounds leave room for, and at the limb bound by choosing zz with all low limbs 2^29 - 1.
After every addition: the value bounds, normalised limbs, and the point against affine big-integer arithmetic."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_field29_asm as G  # noqa: E402

MASK = G.MASK
R29 = 1 << 261
CHUNK, F = 16, 4                      # msm.hip: 2^rlog buckets per chunk, 2^flog chunks per run
BOUND = (6, 4, 2, 2)                  # Acc29: x, y, zz, zzz in units of p


def _sqrt(a, p):
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2; s += 1
    z = 5
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, tt = 0, t
        while tt != 1:
            tt = tt * tt % p; i += 1
        b = pow(c, 1 << (m - i - 1), p); m, c = i, b * b % p; t, r = t * c % p, r * b % p
    return r


def _aff_add(A, B, p):
    (x1, y1), (x2, y2) = A, B
    lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def _rand_point(rnd, p):
    while True:
        x = rnd.randrange(p); y2 = (x * x * x + 5) % p
        if pow(y2, (p - 1) // 2, p) == 1:
            return x, _sqrt(y2, p)


def _raise(vals, p, top):
    """the same residues with as many p added as the Acc29 bounds allow (top) or none"""
    out = []
    for v, k in zip(vals, BOUND):
        v %= p
        out.append(v + (k - 1) * p if top else v)
    return out


def _lazy(A, lam, p, top):
    """the affine point A as a lazy XYZZ point with zz = lam^2, zzz = lam^3 (R'-form), its values at the top or the bottom of the Acc29 ranges"""
    zz, zzz = lam * lam % p, lam * lam * lam % p
    vals = [A[0] * zz * R29 % p, A[1] * zzz * R29 % p, zz * R29 % p, zzz * R29 % p]
    return tuple(G.limbs29(v) for v in _raise(vals, p, top))


def _lam_for_zz(target, p):
    """lam with lam^2 R' = target (mod p), or None when target / R' is no square"""
    zz = target * pow(R29, -1, p) % p
    return _sqrt(zz, p) if zz and pow(zz, (p - 1) // 2, p) == 1 else None


def _extreme_lams(p):
    """zz (as stored) with limbs 0..7 all 2^29 - 1 and the largest top limb below 2 p; zz = 2 p - 1 - j; zz = 1 + j: the first square of each kind"""
    out = []
    top = (2 * p) >> 232
    for cands in (((t << 232) | ((1 << 232) - 1) for t in range(top, 0, -1)), (2 * p - 1 - j for j in range(64)), (1 + j for j in range(64))):
        for target in cands:
            lam = _lam_for_zz(target, p) if target < 2 * p else None
            if lam:
                out.append((lam, target)); break
    assert len(out) == 3
    return out


def _stored(acc):
    """through a B29 record: 36 words of 32 bits"""
    words = [w for v in acc for w in v]
    assert len(words) == 36 and all(0 <= w < (1 << 32) for w in words)
    return tuple(words[9 * i:9 * i + 9] for i in range(4))


def _check(acc, A, p):
    vals = [G.val29(v) for v in acc]
    assert all(v < k * p for v, k in zip(vals, BOUND)), [v / p for v in vals]
    assert all(0 <= l <= MASK for v in acc for l in v[:8]) and all(0 <= v[8] < (1 << 32) for v in acc)
    x, y, zz, zzz = [v * pow(R29, -1, p) % p for v in vals]
    assert zz and x * pow(zz, -1, p) % p == A[0] and y * pow(zzz, -1, p) % p == A[1]
    assert zz * zz * zz % p == zzz * zzz % p


def _at_bounds(acc, p, top):
    return tuple(G.limbs29(v) for v in _raise([G.val29(v) for v in acc], p, top))


@pytest.mark.parametrize("p,name", [(G.P_FP, "Fp"), (G.P_FQ, "Fq")])
def test_add29_second_operand_is_a_stored_sum(p, name):
    rnd = random.Random(2929)
    M = G.Madd29Model(p)
    ext = _extreme_lams(p)
    for lam, target in ext:                                  # the directed zz really is what the record holds
        assert lam * lam * R29 % p == target % p
    chunks = []
    for j in range(F):
        acc, A = None, None
        for i in range(CHUNK):
            B = _rand_point(rnd, p)
            kind = (i + j) % 5                               # leaves: random zz at the top / bottom of the ranges, and the three directed zz
            lam = ext[kind - 2][0] if kind >= 2 else rnd.randrange(1, p)
            b = _stored(_lazy(B, lam, p, top=(kind != 1)))
            if kind == 2:
                assert all(l == MASK for l in b[2][:8])      # all low limbs of zz at the limb bound
            _check(b, B, p)
            if acc is None:
                acc, A = b, B
                continue
            acc = M.add(acc, b); A = _aff_add(A, B, p)
            assert acc is not None, "filter fired on random points"
            _check(acc, A, p)
        chunks.append((_stored(acc), A))
    # level two, three ways: the chunk records as add29 left them, all raised to the top of the Acc29 ranges, and alternating top / bottom
    for mode in ("as stored", "top", "mixed"):
        acc, A = None, None
        for j, (c, Cp) in enumerate(chunks):
            b = c if mode == "as stored" else _stored(_at_bounds(c, p, top=(mode == "top" or j % 2 == 0)))
            _check(b, Cp, p)
            if acc is None:
                acc, A = b, Cp
                continue
            acc = M.add(acc, b); A = _aff_add(A, Cp, p)
            assert acc is not None, "filter fired on random points"
            _check(acc, A, p)
        run = _stored(acc)
        # one level further than the kernels go: a run record as the second operand (chunk 0 is part of the run, but not the same point)
        again = M.add(chunks[0][0], run)
        assert again is not None
        _check(again, _aff_add(chunks[0][1], A, p), p)
    # equal and opposite chunk sums are refused (the marker of k_wide_l2)
    c0 = chunks[0][0]
    neg = (c0[0], G.limbs29((4 * p - G.val29(c0[1])) % p), c0[2], c0[3])
    assert M.add(c0, _stored(_at_bounds(c0, p, True))) is None and M.add(c0, neg) is None
