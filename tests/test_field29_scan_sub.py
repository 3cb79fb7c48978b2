"""mulsub29 / sqrsub29 (csrc/field29.cuh): the Montgomery product scans that take a subtraction along, a b / R' - c + K p from ONE scan.

Through the generator's interpreter and limb model (tools/gen_field29_asm.py): the streams KH29_MULSUB_ASM / KH29_SQRSUB_ASM add d_i = C_i - c_i
to column 9 + i of the scan, C the multiple K p that the additions spread over the limbs (S71, S51, S44).  What is checked is equality LIMB FOR
LIMB with the composition they replace, the product's stream followed by the normalising sweep subn (Madd29Model.mulsub / .sqrsub assert it on
every call; here it is asserted again from outside, and the integer against big-integer arithmetic), with the interpreter asserting the 64-bit
column bound at every v_mad_u64_u32 and the 32-bit range of the last limb."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_field29_asm as G  # noqa: E402

MASK = G.MASK
FIELDS = [(G.P_FP, "Fp"), (G.P_FQ, "Fq")]
SPREADS = [("S71", 7, 1), ("S51", 5, 1), ("S44", 4, 4)]           # P = U2 - X1, R = S2 - Y1, X3 = RR - (PPP + 2 Q)
Model = G.Madd29Model


def _c_ends(M, key, J):
    """the subtrahend at both ends of what the spread allows: all limbs 0; limbs 0..7 at J MASK and limb 8 at (K p)_8 - J (= the spread's own limb 8)"""
    return [[0] * 9, [J * MASK] * 8 + [M.c[key][8]]]


def _both(M, a, b, c, key, K):
    """the scan against the composition, from outside the model: limbs and integer.  b None: the squaring."""
    C = M.c[key]
    if b is None:
        got, prod = M.sqrsub(a, c, C), M.sqr(a)
    else:
        got, prod = M.mulsub(a, b, c, C), M.mul(a, b)
    assert got == M.subn(prod, c, C)
    assert all(0 <= l <= MASK for l in got[:8]) and 0 <= got[8] < (1 << 32)
    assert G.val29(got) == G.val29(prod) + K * M.p - G.val29(c)
    return got


@pytest.mark.parametrize("p,name", FIELDS)
def test_directed_vectors(p, name):
    """every column of the scan with m_k = 0 and with m_k = 2^29 - 1, found through the new streams themselves; under each spread, c at both ends"""
    M = Model(p)
    for kind in ("mulsub", "sqrsub"):
        vecs = G.directed29(p, kind)
        assert vecs == G.directed29(p, kind)                          # deterministic
        assert {(k, t) for _, _, k, t in vecs} == {(k, t) for k in range(9) for t in (0, MASK)}
        for x, y, k, t in vecs:
            a, b = M.mul(G.limbs29(x), M.c["KIN"]), M.mul(G.limbs29(y), M.c["KIN"])
            for key, K, J in SPREADS:
                for c in _c_ends(M, key, J):
                    _both(M, a, None if kind == "sqrsub" else b, c, key, K)
    for lines in (G.gen_mulsub(), G.gen_sqrsub()):
        assert not any(ln.split(",")[-1].strip() == "vcc" for ln in lines)          # no instruction reads VCC


@pytest.mark.parametrize("p,name", FIELDS)
def test_operands_at_the_acc29_bounds(p, name):
    """x < 6 p, y < 4 p, zz and zzz < 2 p against a table coordinate 32 X < 32 p, and one un-normalised operand with 1.5 * 2^30 in every limb
    against a normalised one with every limb full; the squaring on limbs below 2^30 (its operand R is normalised in the additions)."""
    M = Model(p)
    top = {k: G.limbs29(k * p - 1) for k in (2, 4, 6)}
    px = G.limbs29((p - 1) << 5)
    wide, full = [(3 << 29) - 1] * 9, [MASK] * 9
    pairs = [(px, top[2]), (top[6], top[2]), (top[4], top[2]), (top[6], top[6]), (wide, full), (full, wide)]
    for key, K, J in SPREADS:
        for c in _c_ends(M, key, J) + [top[6] if key == "S71" else top[4] if key == "S51" else [3 * MASK] * 8 + [M.c[key][8]]]:
            for a, b in pairs:
                _both(M, a, b, c, key, K)
            for a in (top[2], top[6], full, [(1 << 30) - 1] * 9):
                _both(M, a, None, c, key, K)


@pytest.mark.parametrize("p,name", FIELDS)
def test_random_operands(p, name):
    rnd = random.Random(2911)
    M = Model(p)
    for i in range(300):
        key, K, J = SPREADS[i % 3]
        a = G.limbs29(rnd.randrange(32 * p)) if i % 2 else [rnd.randrange(3 << 29) for _ in range(9)]
        b = G.limbs29(rnd.randrange(6 * p))
        c = [rnd.randrange(J * MASK + 1) for _ in range(8)] + [rnd.randrange(M.c[key][8] + 1)]
        _both(M, a, b, c, key, K)
        _both(M, [rnd.randrange(1 << 30) for _ in range(9)] if i % 2 else b, None, c, key, K)


def _replay(monkeypatch, scan_sub, fn, *args):
    """fn (one of the generator's check_* functions) over a model built on the scans (scan_sub) or on the composition; every addition's result"""
    log = []

    class Rec(Model):
        def __init__(self, p):
            super().__init__(p, scan_sub=scan_sub)

        def madd(self, *a):
            log.append(("madd", super().madd(*a))); return log[-1][1]

        def add(self, *a):
            log.append(("add", super().add(*a))); return log[-1][1]

        def aadd(self, *a):
            log.append(("aadd", super().aadd(*a))); return log[-1][1]

    monkeypatch.setattr(G, "Madd29Model", Rec)
    fn(*args)
    monkeypatch.setattr(G, "Madd29Model", Model)
    return log


@pytest.mark.parametrize("p,name", FIELDS)
def test_additions_on_the_scans_equal_the_composition(p, name, monkeypatch):
    """madd / add / aadd rebuilt on mulsub / sqrsub against the sweeps they had, over the chains and trees that check_madd / check_add / check_aadd
    draw (seeded: the same in both runs), refusals included: the same limbs after every addition"""
    for fn, args, kinds in ((G.check_madd, (p, name, 3, 20), {"madd"}), (G.check_add, (p, name, 2, 12), {"madd", "add"}), (G.check_aadd, (p, name, 20, 4), {"aadd", "madd"})):
        new, old = _replay(monkeypatch, True, fn, *args), _replay(monkeypatch, False, fn, *args)
        assert len(new) > 20 and {k for k, _ in new} == kinds
        assert new == old
    assert any(r is None for _, r in new)                                 # (check_aadd ends on its refusals)


def test_generated_file_holds_the_two_streams():
    text = open(G.INC_PATH).read()
    assert text == G.render()
    assert G.emit("KH29_MULSUB_ASM", G.gen_mulsub()) in text and G.emit("KH29_SQRSUB_ASM", G.gen_sqrsub()) in text
    # the streams that to29 / from29 and the narrow rebase use are what they were: the new ones are theirs plus nine additions, the last in place of the v_mov
    for plain, sub in ((G.gen_mul(), G.gen_mulsub()), (G.gen_sqr(), G.gen_sqrsub())):
        assert len(sub) == len(plain) + 8 and sum("v_mad_u64_u32" in l for l in sub) == sum("v_mad_u64_u32" in l for l in plain) + 8
        assert plain[-1].startswith("v_mov_b32") and sub[-1].startswith("v_add_u32")
