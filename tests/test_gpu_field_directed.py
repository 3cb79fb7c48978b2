"""The directed operand sets of tools/field_model.py (every reachable carry / borrow site of the eight-limb product, squaring,
add and sub at 0 and at 1, and the named edge cases) and of tools/gen_field29_asm.py (extreme reduction digits of the nine-limb
product and squaring) on the device, through khip.debug_field_op, bit for bit against Python big integers.  tests/
test_field_model.py holds the same vectors to the CPU model of the instruction streams; a disagreement between the two is a
finding about opcode semantics or register allocation."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fm = _load("field_model")
g29 = _load("gen_field29_asm")
R = 1 << 256
FIELDS = [(0, "Fp"), (1, "Fq")]
# one wavefront is 64 lanes, one block of the debug kernel 256: lengths that leave the last wavefront / block partial
RAGGED = (1, 63, 65, 255, 257)


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def to_limbs(vals):
    out = np.empty((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        assert 0 <= v < R
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & ((1 << 64) - 1)
    return out


def from_limbs(arr):
    return [sum(int(r[j]) << (64 * j) for j in range(4)) for r in arr]


def check(khip, fid, op, a, b, want, what):
    """the whole list at once and at every ragged length (a prefix, and the tail so that every vector meets a partial wavefront)"""
    n = len(a)
    cuts = [(0, n)] + [(0, m) for m in RAGGED if m < n] + [(n - m, n) for m in RAGGED if m < n]
    if n % 64 == 0:                                         # keep the full run ragged too
        cuts.append((0, n - 1))
    for lo, hi in cuts:
        got = from_limbs(khip.debug_field_op(fid, op, to_limbs(a[lo:hi]), None if b is None else to_limbs(b[lo:hi])))
        bad = [i for i in range(hi - lo) if got[i] != want[lo + i]]
        assert not bad, f"{what} {op} [{lo}:{hi}]: first wrong at {lo + bad[0]}: a = {a[lo + bad[0]]:#x}" + \
            ("" if b is None else f", b = {b[lo + bad[0]]:#x}") + f", got {got[bad[0]]:#x}, want {want[lo + bad[0]]:#x}"


def operands(field, streams, canonical_only):
    """the directed vectors of the given streams and the edge values pairwise, as two parallel lists"""
    p = fm.PRIMES[field]
    a, b = [], []
    for s in streams:
        for v in fm.directed(s, field):
            if v.canonical or not canonical_only:
                a.append(v.a); b.append(v.b)
    e = fm.edge_values(p)
    a += [x for x in e for _ in e]
    b += [y for _ in e for y in e]
    return a, b


@pytest.mark.parametrize("fid,field", FIELDS)
@pytest.mark.parametrize("op", ["mul", "sqr", "add", "sub"])
def test_directed_sets_on_the_device(khip, fid, field, op):
    """each stream on its own directed set -- operands >= p included where the set needs them to reach t = p, t = 2p - 1 or the
    squaring's top limb (the streams only need t < 2p; the definition holds for them as it stands) -- and on the canonical
    vectors of the other three streams"""
    p = fm.PRIMES[field]
    a, b = operands(field, [op], canonical_only=False)
    a2, b2 = operands(field, [s for s in fm.STREAMS if s != op], canonical_only=True)
    a, b = a + a2, b + b2
    want = [fm.reference(op, p, x, y) for x, y in zip(a, b)]
    check(khip, fid, op, a, None if op == "sqr" else b, want, field)


@pytest.mark.parametrize("fid,field", FIELDS)
def test_directed_sets_through_neg_and_the_montgomery_conversions(khip, fid, field):
    """neg (p - a, 0 for 0), to_mont (the product with R^2: a R mod p) and from_mont (the reduction half alone, on the column
    blocks of field_cols.inc: a R^-1 mod p) on every canonical operand of the directed sets.  from_mont also gets operands that
    put t = 0 .. and t just below and at p behind its reduction: a = t R mod p arrives at t or t - p."""
    p = fm.PRIMES[field]
    a, b = operands(field, fm.STREAMS, canonical_only=True)
    vals = a + b
    Rinv = pow(R, -1, p)
    check(khip, fid, "neg", vals, None, [(p - x) % p for x in vals], field)
    check(khip, fid, "to_mont", vals, None, [x * R % p for x in vals], field)
    plow = p % (1 << 128)
    ts = [0, 1, p - 1, p - 2, 1 << 254, (1 << 254) + plow - 1, (1 << 254) + 1, (1 << 254) - 1, plow, plow - 1, (1 << 224) - 1, 1 << 128, (1 << 128) - 1]
    fvals = vals + [t * R % p for t in ts]
    check(khip, fid, "from_mont", fvals, None, [x * Rinv % p for x in fvals], field)


@pytest.mark.parametrize("fid,field", FIELDS)
def test_directed_sets_through_the_29_bit_path(khip, fid, field):
    """mul29 / sqr29 / mul29_32x on the operands that put m_k = 0 and m_k = 2^29 - 1 into every column of their middle product
    (gen_field29_asm.directed29), and on the canonical vectors of the eight-limb directed sets"""
    p = fm.PRIMES[field]
    Rinv = pow(R, -1, p)
    a, b = operands(field, fm.STREAMS, canonical_only=True)
    for op, kind in (("mul29", "mul"), ("sqr29", "sqr"), ("mul29_32x", "mul32x")):
        d = g29.directed29(p, kind)
        x = [v[0] for v in d] + a
        y = [v[1] for v in d] + (a if kind == "sqr" else b)
        want = [u * v * Rinv % p for u, v in zip(x, y)]
        check(khip, fid, op, x, None if kind == "sqr" else y, want, field)
