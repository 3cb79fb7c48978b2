"""aadd29 (csrc/field29.cuh): the affine + affine addition that opens a bucket in the MSM accumulation kernels, and its helper fold29.

Through the limb-exact model tools/gen_field29_asm.py (Madd29Model.aadd / .fold: every product runs the generated instruction stream, whose
interpreter asserts the 64-bit column bound at every v_mad_u64_u32, and every 32-bit operation asserts its range).  Both points enter as the kernels
hand them over: 32 X, 32 Y of the canonical wire coordinates (X = x 2^256 mod p), nine normalised limbs.  The addition formulas hold for any
coordinates with x1 != x2 (the curve equation does not enter them), so the directed coordinates need not lie on the curve.  After every addition:
the Acc29 value bounds (x < 6 p, y < 4 p, zz, zzz < 2 p), normalised limbs, and the point against affine big-integer arithmetic."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_field29_asm as G  # noqa: E402

MASK = G.MASK
R29 = 1 << 261
BOUND = (6, 4, 2, 2)                  # Acc29: x, y, zz, zzz in units of p
FIELDS = [(G.P_FP, "Fp"), (G.P_FQ, "Fq")]


def _wire(X):
    """canonical wire value X < p -> the limbs of 32 X (pack29<F, 5>)"""
    l = G.limbs29(X << 5)
    assert all(v <= MASK for v in l)
    return l


def _val(X, p):
    """the field element that the wire value X stands for in the lazy R'-form: 32 X = x R'"""
    return (X << 5) * pow(R29, -1, p) % p


def _aff_add(A, B, p):
    (x1, y1), (x2, y2) = A, B
    lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def _check(acc, A, p):
    vals = [G.val29(v) for v in acc]
    assert all(v < k * p for v, k in zip(vals, BOUND)), [v / p for v in vals]
    assert all(0 <= l <= MASK for v in acc for l in v[:8]) and all(0 <= v[8] < (1 << 32) for v in acc)
    x, y, zz, zzz = [v * pow(R29, -1, p) % p for v in vals]
    assert zz and x * pow(zz, -1, p) % p == A[0] and y * pow(zzz, -1, p) % p == A[1]
    assert zz * zz * zz % p == zzz * zzz % p


def _at_top(acc, p):
    """the same residues with as many p added as the Acc29 bounds allow"""
    return tuple(G.limbs29(G.val29(v) % p + (k - 1) * p) for v, k in zip(acc, BOUND))


def _open(M, P1, P2, p):
    """aadd29 on two wire points, checked; returns (lazy sum, affine sum)"""
    acc = M.aadd(_wire(P1[0]), _wire(P1[1]), _wire(P2[0]), _wire(P2[1]))
    assert acc is not None, "refused although x1 != x2"
    A = _aff_add((_val(P1[0], p), _val(P1[1], p)), (_val(P2[0], p), _val(P2[1], p)), p)
    _check(acc, A, p)
    return acc, A


@pytest.mark.parametrize("p,name", FIELDS)
def test_fold29_range_and_multiples_of_p(p, name):
    """the fold over its whole input range (0, 65 p): same residue, in (0, 2 p), normalised; every k p it can meet comes out as p itself"""
    rnd = random.Random(2901)
    M = G.Madd29Model(p)
    for k in range(1, 66):
        assert M.fold(G.limbs29(k * p)) == G.limbs29(p)
    ends = [1, 2, p - 1, p + 1, (1 << 254) - 1, 1 << 254, (1 << 254) + 1, 2 * p - 1, 33 * p - 1, 33 * p + 1, 64 * p + 1, 65 * p - 1]
    ends += [(h << 254) + d for h in (1, 2, 32, 33, 64, 65) for d in (-1, 0, 1) if (h << 254) + d < 65 * p]      # borrows through the empty limbs 5..7
    for v in ends + [rnd.randrange(1, 65 * p) for _ in range(300)]:
        f = M.fold(G.limbs29(v))
        assert all(0 <= l <= MASK for l in f[:8])
        assert 0 < G.val29(f) < 2 * p and G.val29(f) % p == v % p


@pytest.mark.parametrize("p,name", FIELDS)
def test_aadd29_random_pairs(p, name):
    rnd = random.Random(2902)
    M = G.Madd29Model(p)
    for _ in range(40):
        P1 = (rnd.randrange(p), rnd.randrange(p)); P2 = (rnd.randrange(p), rnd.randrange(p))
        _open(M, P1, P2, p)


@pytest.mark.parametrize("p,name", FIELDS)
def test_aadd29_directed_coordinates(p, name):
    """X1, X2 (and Y1, Y2) at the ends of their range, in both orders: P = 32 (X2 - X1) + 33 p sits at either end of (p, 65 p) before the fold.
    2^254 .. p - 1 are the wire values whose 32 X has the top limb at its maximum, 2^27; 2^254 - 1 has every lower limb at the limb bound."""
    M = G.Madd29Model(p)
    D = [0, 1, p - 1, 1 << 254, (1 << 254) - 1]
    assert G.limbs29((p - 1) << 5)[8] == G.limbs29(32 * p)[8] == 1 << 27 and G.limbs29(((1 << 254) - 1) << 5)[1:8] == [MASK] * 7
    for X1 in D:
        for X2 in D:
            if X1 == X2:
                continue
            for Y1 in D:
                for Y2 in D:
                    _open(M, (X1, Y1), (X2, Y2), p)


@pytest.mark.parametrize("p,name", FIELDS)
def test_aadd29_then_madd_chain_at_the_upper_bounds(p, name):
    """an opening carried on through mixed additions, the accumulator raised to the top of the Acc29 ranges before every one of them"""
    rnd = random.Random(2903)
    M = G.Madd29Model(p)
    D = [0, 1, p - 1, 1 << 254, (1 << 254) - 1]
    for chain in range(6):
        P1 = (rnd.choice(D), rnd.choice(D)) if chain % 2 else (rnd.randrange(p), rnd.randrange(p))
        P2 = (rnd.randrange(p), rnd.randrange(p))
        acc, A = _open(M, P1, P2, p)
        for step in range(8):
            B = (rnd.choice(D), rnd.choice(D)) if step % 3 == 2 else (rnd.randrange(p), rnd.randrange(p))
            top = _at_top(acc, p)
            _check(top, A, p)
            acc = M.madd(top, _wire(B[0]), _wire(B[1]))
            assert acc is not None, "filter fired on random points"
            A = _aff_add(A, (_val(B[0], p), _val(B[1], p)), p)
            _check(acc, A, p)


@pytest.mark.parametrize("p,name", FIELDS)
def test_aadd29_refuses_equal_x(p, name):
    """P = 0 (mod p): the same point and the opposite point are refused.  Before the fold P is 33 p there, and whichever multiple of p reached the
    fold, it leaves p (test_fold29_range_and_multiples_of_p), the one value the filter looks for."""
    rnd = random.Random(2904)
    M = G.Madd29Model(p)
    for X in [0, 1, p - 1, 1 << 254, (1 << 254) - 1] + [rnd.randrange(p) for _ in range(8)]:
        for Y in (1, p - 1, rnd.randrange(1, p)):
            assert M.subn(_wire(X), _wire(X), M.c["S331"]) == G.limbs29(33 * p)
            assert M.aadd(_wire(X), _wire(Y), _wire(X), _wire(Y)) is None                   # equal points
            assert M.aadd(_wire(X), _wire(Y), _wire(X), _wire(p - Y)) is None               # opposite points
            assert M.aadd(_wire(X), _wire(Y), _wire(X), _wire(rnd.randrange(p))) is None    # (no curve point, the same x all the same)
