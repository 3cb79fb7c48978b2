"""The curve gates' witness on the device (csrc/curve_gadgets.hip: kh_complete_add_witness_dev, kh_varbasemul_witness_dev, kh_endomul_witness_dev,
kh_endomul_scalar_witness_dev) against the oracle's restatement of the reference's generators (oracle/gates.py) and the product's own constraint check,
prover and verifier.  Everything is compared bit for bit on a sentinel-filled 15 x col_stride buffer: a cell holds the oracle's value where the
generator assigns one and the sentinel everywhere else."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import gates as G
from oracle import pasta as P

pytestmark = pytest.mark.gpu
FIELDS = (P.Fp, P.Fq)
CURVES = (P.PALLAS, P.VESTA)          # the curve whose coordinates live in field 0 / 1
SENTINEL = np.array([0x0123456789abcdef, 0xfedcba9876543210, 0x0f1e2d3c4b5a6978, 0x1badc0de1badc0de], dtype=np.uint64)     # a canonical element (< 2^253)
COL_LEN = 256

# the cells the generators assign, per row of an instance
CADD_COLS = tuple(range(11))
VBM_BASE_COLS = (0, 1, 2, 3, 4, 5) + tuple(range(7, 15))
VBM_BIT_COLS = tuple(range(12))
ENDO_COLS = (0, 1, 2) + tuple(range(4, 15))
ENDO_CLOSING_COLS = (0, 1, 4, 5, 6)
EMS_COLS = tuple(range(14))


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def limbs(F, vals):
    """(len(vals), 4) Montgomery limbs"""
    p, R = F.p, 1 << 256
    return np.frombuffer(b"".join((v % p * R % p).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def plain(vals, words):
    """(len(vals), words) canonical little-endian limbs of plain integers"""
    return np.frombuffer(b"".join(v.to_bytes(8 * words, "little") for v in vals), dtype=np.uint64).reshape(-1, words).copy()


def points(F, pts):
    return limbs(F, [c for pt in pts for c in pt])


def sentinel_buf(khip, elems):
    return khip.DevBuf(32 * elems).upload(np.tile(SENTINEL, (elems, 1)))


def msb_bits(k, num_bits):
    return [(k >> (num_bits - 1 - t)) & 1 for t in range(num_bits)]


def neg(F, pt):
    return (pt[0], (-pt[1]) % F.p)


@pytest.fixture(scope="module")
def pool():
    """per field: 140 points of the curve over it, computed once"""
    out = []
    for fid, crv in enumerate(CURVES):
        rnd = random.Random(500 + fid)
        out.append([crv.mul(crv.gen, rnd.randrange(1, 1 << 60)) for _ in range(140)])
    return out


def endo_of(khip, fid):
    """(the oracle's endo coefficient, the library's limbs of it): kh_endos of the curve whose base field is `fid`"""
    e = P.endos(CURVES[fid])[0]
    lib = khip.endos((khip.PALLAS, khip.VESTA)[fid])[0]
    assert np.array_equal(np.asarray(lib, dtype=np.uint64), limbs(FIELDS[fid], [e])[0])
    return e, lib


def expected(F, col_stride, placed):
    """the sentinel-filled witness with the cells of `placed` = [(start row, [(row offset, columns, oracle row)])] set"""
    want = np.tile(SENTINEL, (15, col_stride, 1))
    where, vals = [], []
    for start, rows in placed:
        for off, cols, row in rows:
            for c in cols:
                where.append((c, start + off)); vals.append(row[c])
    lm = limbs(F, vals)
    for (c, r), v in zip(where, lm):
        want[c, r] = v
    return want


def compare(wit, want, col_stride, ignore_rows=()):
    got = wit.download((15, col_stride, 4))
    diff = (got != want).any(axis=2)
    for r in ignore_rows:
        diff[:, r] = False
    bad = np.argwhere(diff)
    assert bad.size == 0, ("cells (column, row) that differ", bad[:8].tolist())


def starts_of(n, rows, row0, row_stride):
    return list(rows) if rows is not None else [row0 + i * row_stride for i in range(n)]


# ---- 1. CompleteAdd
def cadd_pairs(F, pts, n):
    """a doubling, a P + (-P), generic pairs"""
    pairs = [(pts[2 * i], pts[2 * i + 1]) for i in range(n)]
    if n > 1:
        pairs[1] = (pts[5], pts[5])
    if n > 2:
        pairs[2] = (pts[7], neg(F, pts[7]))
    if n > 64:
        pairs[64] = (pts[9], pts[9])
    return pairs


def run_complete_add(khip, fid, pairs, rows=None, row0=0, row_stride=1, col_stride=COL_LEN, col_len=COL_LEN):
    F, crv, n = FIELDS[fid], CURVES[fid], len(pairs)
    w = [G.complete_add_witness(F, a, b) for a, b in pairs]
    for (a, b), row in zip(pairs, w):                       # the oracle's row is the group sum
        s = crv.add(a, b)
        assert (row[6] == 1) if s is None else (row[6] == 0 and (row[4], row[5]) == s)
    want = expected(F, col_stride, [(st, [(0, CADD_COLS, row)]) for st, row in zip(starts_of(n, rows, row0, row_stride), w)])
    wit = sentinel_buf(khip, 15 * col_stride)
    p1 = khip.DevBuf(64 * n).upload(points(F, [a for a, _ in pairs])); p2 = khip.DevBuf(64 * n).upload(points(F, [b for _, b in pairs]))
    out = sentinel_buf(khip, 2 * n + 1)
    khip.complete_add_witness_dev(fid, p1, p2, n, wit, col_stride, col_len, rows=rows, row0=row0, row_stride=row_stride, out=out)
    compare(wit, want, col_stride)
    assert np.array_equal(out.download((2 * n + 1, 4)), np.vstack([limbs(F, [c for row in w for c in (row[4], row[5])]), SENTINEL[None]]))
    for b in (wit, p1, p2, out):
        b.free()


@pytest.mark.parametrize("fid", [0, 1])
def test_complete_add_rows(khip, pool, fid):
    F, pts = FIELDS[fid], pool[fid]
    run_complete_add(khip, fid, cadd_pairs(F, pts, 1), row0=17)
    run_complete_add(khip, fid, cadd_pairs(F, pts, 5), rows=[COL_LEN - 1, 0, 100, 101, 7])          # irregular, touching both ends
    run_complete_add(khip, fid, cadd_pairs(F, pts, 65), row0=3, row_stride=2, col_stride=COL_LEN + 5)  # one lane into a second wave
    run_complete_add(khip, fid, [(pts[0], pts[1])], rows=[COL_LEN - 1], col_stride=COL_LEN + 5)


# ---- 2. VarBaseMul
def vbm_oracle(fid, base, k, num_bits, acc0=None):
    F, crv = FIELDS[fid], CURVES[fid]
    bits = msb_bits(k, num_bits)
    w, acc, nacc = G.varbasemul_witness(F, base, bits, acc0 or crv.add(base, base))
    if acc0 is None:                                          # acc <- 2 acc + (2 b - 1) base per bit, from acc0 = 2 base (tests/test_gates.py)
        m = 2
        for b in bits:
            m = 2 * m + (2 * b - 1)
        assert acc == crv.mul(base, m)
    rows = [(j, VBM_BIT_COLS if j & 1 else VBM_BASE_COLS, w[j]) for j in range(len(w))]
    return rows, acc, nacc


def run_varbasemul(khip, fid, bases, scalars, num_bits, rows=None, row0=0, row_stride=None, col_stride=COL_LEN, col_len=COL_LEN):
    F, crv, n = FIELDS[fid], CURVES[fid], len(bases)
    inst = 2 * num_bits // 5
    row_stride = inst if row_stride is None else row_stride
    placed, accs, ns = [], [], []
    for st, base, k in zip(starts_of(n, rows, row0, row_stride), bases, scalars):
        r, acc, nacc = vbm_oracle(fid, base, k, num_bits)
        placed.append((st, r)); accs.append(acc); ns.append(nacc)
    want = expected(F, col_stride, placed)
    wit = sentinel_buf(khip, 15 * col_stride)
    b = khip.DevBuf(64 * n).upload(points(F, bases)); a = khip.DevBuf(64 * n).upload(points(F, [crv.add(p, p) for p in bases]))
    s = khip.DevBuf(32 * n).upload(plain(scalars, 4))
    oa = sentinel_buf(khip, 2 * n + 1); on = sentinel_buf(khip, n + 1)
    flags = khip.DevBuf(4).zero()
    khip.varbasemul_witness_dev(fid, b, a, s, num_bits, n, wit, col_stride, col_len, rows=rows, row0=row0, row_stride=row_stride, out_acc=oa, out_n=on,
                                flags=flags, bit=5)
    compare(wit, want, col_stride)
    assert np.array_equal(oa.download((2 * n + 1, 4)), np.vstack([points(F, accs), SENTINEL[None]]))
    assert np.array_equal(on.download((n + 1, 4)), np.vstack([limbs(F, ns), SENTINEL[None]]))
    assert int(flags.download((1,), dtype=np.uint32)[0]) == 0
    for buf in (wit, b, a, s, oa, on, flags):
        buf.free()


def some_scalars(F, n, num_bits, seed):
    rnd = random.Random(seed)
    ks = [rnd.randrange(1 << num_bits) for _ in range(n)]
    if num_bits == 255:
        ks[0] = F.p + 12345                                   # >= p: n_acc wraps as the oracle's % p does
        ks[-1] |= 1 << 254
    return ks


@pytest.mark.parametrize("num_bits", [5, 10, 255])
@pytest.mark.parametrize("fid", [0, 1])
def test_varbasemul_rows(khip, pool, fid, num_bits):
    F, pts = FIELDS[fid], pool[fid]
    inst = 2 * num_bits // 5
    col_len = max(COL_LEN, 3 * inst + 8)
    run_varbasemul(khip, fid, pts[:1], some_scalars(F, 1, num_bits, 600 + num_bits), num_bits, row0=col_len - inst, col_stride=col_len, col_len=col_len)
    # rows == NULL: back to back, and one row apart
    run_varbasemul(khip, fid, pts[1:4], some_scalars(F, 3, num_bits, 601 + num_bits), num_bits, col_stride=col_len, col_len=col_len)
    run_varbasemul(khip, fid, pts[4:7], some_scalars(F, 3, num_bits, 602 + num_bits), num_bits, row0=2, row_stride=inst + 1, col_stride=col_len, col_len=col_len)
    # rows: irregular (both ends, two back to back), and columns further apart than their length
    run_varbasemul(khip, fid, pts[7:10], some_scalars(F, 3, num_bits, 603 + num_bits), num_bits, rows=[col_len - inst, 0, inst], col_stride=col_len + 37,
                   col_len=col_len)


@pytest.mark.parametrize("n", [64, 65, 130])
@pytest.mark.parametrize("fid", [0, 1])
def test_varbasemul_over_several_waves(khip, pool, fid, n):
    run_varbasemul(khip, fid, pool[fid][:n], some_scalars(FIELDS[fid], n, 10, 610 + n), 10, row0=1, row_stride=5, col_stride=700, col_len=700)


@pytest.mark.parametrize("fid", [0, 1])
def test_batches_larger_than_a_slice(khip, pool, fid):
    """kh_curve_witness_set_slice_elements: 130 instances in slices of 64 + 64 + 2 (VarBaseMul, 11 inversions each) and 65 in 21 + 21 + 21 + 2 (EndoMul,
    7 each), irregular rows, the outputs at their instances' places"""
    F, pts = FIELDS[fid], pool[fid]
    try:
        khip.curve_witness_set_slice_elements(64 * 11 + 5)
        rows = [(37 * i) % 131 * 5 for i in range(130)]
        run_varbasemul(khip, fid, pts[:130], some_scalars(F, 130, 10, 620), 10, rows=rows, col_stride=700, col_len=700)
        khip.curve_witness_set_slice_elements(21 * 7 + 6)
        rows = [(11 * i) % 67 * 4 for i in range(65)]
        run_endomul(khip, fid, pts[:65], some_chals(65, 8, 720), 8, rows=rows, col_stride=300, col_len=300)
    finally:
        khip.curve_witness_set_slice_elements()


# ---- 3. EndoMul
def endo_oracle(fid, endo, base, chal, num_bits, acc0=None):
    F, crv = FIELDS[fid], CURVES[fid]
    bits = msb_bits(chal, num_bits)
    phi = (endo * base[0] % F.p, base[1])
    tp = crv.add(base, phi)
    start = acc0 or crv.add(tp, tp)
    w, acc, nacc = G.endomul_witness(F, endo, base, bits, start)
    if acc0 is None:
        want = start
        for i in range(0, num_bits, 2):
            q = phi if bits[i] else base
            want = crv.add(crv.add(want, q if bits[i + 1] else neg(F, q)), want)
        assert acc == want and nacc == chal
    rows = [(j, ENDO_COLS, w[j]) for j in range(len(w) - 1)] + [(len(w) - 1, ENDO_CLOSING_COLS, w[-1])]
    return rows, start, acc, nacc


def run_endomul(khip, fid, bases, chals, num_bits, rows=None, row0=0, row_stride=None, col_stride=COL_LEN, col_len=COL_LEN):
    F, n = FIELDS[fid], len(bases)
    endo, endo_limbs = endo_of(khip, fid)
    inst = num_bits // 4 + 1
    row_stride = inst if row_stride is None else row_stride
    placed, acc0s, accs, ns = [], [], [], []
    for st, base, k in zip(starts_of(n, rows, row0, row_stride), bases, chals):
        r, a0, acc, nacc = endo_oracle(fid, endo, base, k, num_bits)
        placed.append((st, r)); acc0s.append(a0); accs.append(acc); ns.append(nacc)
    want = expected(F, col_stride, placed)
    wit = sentinel_buf(khip, 15 * col_stride)
    b = khip.DevBuf(64 * n).upload(points(F, bases)); a = khip.DevBuf(64 * n).upload(points(F, acc0s))
    s = khip.DevBuf(16 * n).upload(plain(chals, 2))
    oa = sentinel_buf(khip, 2 * n + 1); on = sentinel_buf(khip, n + 1)
    flags = khip.DevBuf(4).zero()
    khip.endomul_witness_dev(fid, endo_limbs, b, a, s, num_bits, n, wit, col_stride, col_len, rows=rows, row0=row0, row_stride=row_stride, out_acc=oa,
                             out_n=on, flags=flags, bit=31)
    compare(wit, want, col_stride)
    assert np.array_equal(oa.download((2 * n + 1, 4)), np.vstack([points(F, accs), SENTINEL[None]]))
    assert np.array_equal(on.download((n + 1, 4)), np.vstack([limbs(F, ns), SENTINEL[None]]))
    assert int(flags.download((1,), dtype=np.uint32)[0]) == 0
    for buf in (wit, b, a, s, oa, on, flags):
        buf.free()


def some_chals(n, num_bits, seed):
    rnd = random.Random(seed)
    ks = [rnd.randrange(1 << num_bits) for _ in range(n)]
    ks[-1] |= 1 << (num_bits - 1)
    return ks


@pytest.mark.parametrize("num_bits", [4, 8, 128])
@pytest.mark.parametrize("fid", [0, 1])
def test_endomul_rows(khip, pool, fid, num_bits):
    pts = pool[fid]
    inst = num_bits // 4 + 1
    run_endomul(khip, fid, pts[10:11], some_chals(1, num_bits, 700 + num_bits), num_bits, row0=COL_LEN - inst)
    run_endomul(khip, fid, pts[11:14], some_chals(3, num_bits, 701 + num_bits), num_bits)
    run_endomul(khip, fid, pts[14:17], some_chals(3, num_bits, 702 + num_bits), num_bits, rows=[COL_LEN - inst, 0, inst], col_stride=COL_LEN + 37)
    run_endomul(khip, fid, pts[17:20], some_chals(3, num_bits, 703 + num_bits), num_bits, row0=5, row_stride=inst + 1)


@pytest.mark.parametrize("fid", [0, 1])
def test_endomul_over_two_waves(khip, pool, fid):
    run_endomul(khip, fid, pool[fid][:65], some_chals(65, 8, 710), 8, row0=2, row_stride=4, col_stride=300, col_len=300)


# ---- 4. EndoMulScalar
@pytest.mark.parametrize("num_bits", [16, 128])
@pytest.mark.parametrize("fid", [0, 1])
def test_endomul_scalar_rows(khip, fid, num_bits):
    F = FIELDS[fid]
    rnd = random.Random(800 + num_bits + fid)
    endo_scalar = rnd.randrange(F.p)
    inst = num_bits // 16
    for n, rows, row0, row_stride, col_stride in ((1, None, COL_LEN - inst, inst, COL_LEN), (65, None, 0, inst, 65 * 8 + 3),
                                                  (3, [COL_LEN - inst, 0, inst], 0, inst, COL_LEN + 9)):
        col_len = max(COL_LEN, 65 * inst) if n == 65 else COL_LEN
        col_stride = max(col_stride, col_len)
        chals = some_chals(n, num_bits, 810 + n)
        chals[0] = (1 << num_bits) - 1 if n > 1 else chals[0]
        res = [G.endomul_scalar_witness(F, k, endo_scalar, num_bits) for k in chals]
        for k, (_w, v) in zip(chals, res):
            assert v == P.challenge_to_field(F, k, endo_scalar, num_bits)
        want = expected(F, col_stride, [(st, [(j, EMS_COLS, w[j]) for j in range(inst)])
                                        for st, (w, _v) in zip(starts_of(n, rows, row0, row_stride), res)])
        wit = sentinel_buf(khip, 15 * col_stride)
        s = khip.DevBuf(16 * n).upload(plain(chals, 2))
        out = sentinel_buf(khip, n + 1)
        khip.endomul_scalar_witness_dev(fid, s, num_bits, n, wit, col_stride, col_len, rows=rows, row0=row0, row_stride=row_stride,
                                        endo_scalar=limbs(F, [endo_scalar])[0], out=out)
        compare(wit, want, col_stride)
        assert np.array_equal(out.download((n + 1, 4)), np.vstack([limbs(F, [v for _w, v in res]), SENTINEL[None]]))
        khip.endomul_scalar_witness_dev(fid, s, num_bits, n, wit, col_stride, col_len, rows=rows, row0=row0, row_stride=row_stride)     # no out, no endo_scalar
        compare(wit, want, col_stride)
        for buf in (wit, s, out):
            buf.free()


# ---- 5. zero denominators: the flag, and nobody else's cells
@pytest.mark.parametrize("fid", [0, 1])
def test_varbasemul_zero_denominators_are_flagged_and_stay_at_home(khip, pool, fid):
    """five ordinary instances; instance 2 has acc0 = base (x_0 = x_Q: the first s1 denominator), instance 4 has base = -2 acc0 and first bit 1
    (acc0 + Q = -acc0: the first s2 denominator)"""
    F, crv, pts = FIELDS[fid], CURVES[fid], pool[fid]
    num_bits, inst, n = 10, 4, 7
    bases = list(pts[20:27]); acc0s = [crv.add(p, p) for p in bases]
    ks = some_scalars(F, n, num_bits, 900)
    acc0s[2] = bases[2]
    acc0s[4] = pts[30]; bases[4] = neg(F, crv.add(pts[30], pts[30])); ks[4] |= 1 << (num_bits - 1)
    assert (acc0s[2][0] - bases[2][0]) % F.p == 0
    r_mid = crv.add(acc0s[4], bases[4])
    assert (acc0s[4][0] - r_mid[0]) % F.p == 0 and (acc0s[4][0] - bases[4][0]) % F.p != 0
    starts = [3 + 5 * i for i in range(n)]
    want = expected(F, COL_LEN, [(st, vbm_oracle(fid, b, k, num_bits)[0]) for i, (st, b, k) in enumerate(zip(starts, bases, ks)) if i not in (2, 4)])
    wit = sentinel_buf(khip, 15 * COL_LEN)
    b = khip.DevBuf(64 * n).upload(points(F, bases)); a = khip.DevBuf(64 * n).upload(points(F, acc0s)); s = khip.DevBuf(32 * n).upload(plain(ks, 4))
    flags = khip.DevBuf(4).zero()
    khip.varbasemul_witness_dev(fid, b, a, s, num_bits, n, wit, COL_LEN, COL_LEN, rows=starts, flags=flags, bit=9)
    compare(wit, want, COL_LEN, ignore_rows=[starts[i] + j for i in (2, 4) for j in range(inst)])
    assert int(flags.download((1,), dtype=np.uint32)[0]) == 1 << 9
    for buf in (wit, b, a, s, flags):
        buf.free()


@pytest.mark.parametrize("fid", [0, 1])
def test_endomul_zero_denominator_is_flagged_and_stays_at_home(khip, pool, fid):
    """five ordinary instances and one with acc0 = base and first bits 0, 1: Q_1 = T = acc0"""
    F, pts = FIELDS[fid], pool[fid]
    endo, endo_limbs = endo_of(khip, fid)
    num_bits, inst, n = 8, 3, 6
    bases = list(pts[40:46])
    ks = some_chals(n, num_bits, 910)
    ks[3] = (ks[3] & 0x3f) | 0x40
    oracle = [endo_oracle(fid, endo, b, k, num_bits) for b, k in zip(bases, ks)]
    acc0s = [o[1] for o in oracle]
    acc0s[3] = bases[3]
    starts = [COL_LEN - inst - 4 * i for i in range(n)]
    want = expected(F, COL_LEN, [(st, o[0]) for i, (st, o) in enumerate(zip(starts, oracle)) if i != 3])
    wit = sentinel_buf(khip, 15 * COL_LEN)
    b = khip.DevBuf(64 * n).upload(points(F, bases)); a = khip.DevBuf(64 * n).upload(points(F, acc0s)); s = khip.DevBuf(16 * n).upload(plain(ks, 2))
    flags = khip.DevBuf(4).zero()
    khip.endomul_witness_dev(fid, endo_limbs, b, a, s, num_bits, n, wit, COL_LEN, COL_LEN, rows=starts, flags=flags, bit=0)
    compare(wit, want, COL_LEN, ignore_rows=[starts[3] + j for j in range(inst)])
    assert int(flags.download((1,), dtype=np.uint32)[0]) == 1
    for buf in (wit, b, a, s, flags):
        buf.free()


# ---- 6. through the product: index, constraint check, proof, verification
VBM_BITS, ENDO_BITS, EMS_BITS = 10, 8, 32


def test_gadget_witnesses_satisfy_the_product(khip, pool):
    fid, F, crv, pts = khip.FP, P.Fp, CURVES[0], pool[0]
    endo, endo_limbs = endo_of(khip, fid)
    srs = khip.Srs.create(khip.VESTA, 1 << 7)
    gids = khip.gate_ids()
    Z = khip.GATE_ZERO
    types = [gids["VarBaseMul"], Z] * 2 * 3 + [gids["EndoMul"], gids["EndoMul"], Z] * 2 + [gids["CompleteAdd"]] * 4 + [gids["EndoMulScalar"]] * 2
    vbm0, endo0, cadd0, ems0 = 0, 12, 18, 22
    assert len(types) == 24
    wires = np.array([[(r, c) for c in range(7)] for r in range(len(types))], dtype=np.uint32)
    coeffs = np.zeros((len(types), 15, 4), dtype=np.uint64)
    ix = khip.NativeProverIndex.create(srs, types, wires, coeffs)
    log2_n, _zk, nch = ix.shape()
    n = 1 << log2_n
    assert nch == 1
    wit = khip.DevBuf(32 * 15 * n).zero()
    bufs = []

    def dev(arr):
        bufs.append(khip.DevBuf(arr.nbytes).upload(arr))
        return bufs[-1]

    vb = pts[50:53]
    khip.varbasemul_witness_dev(fid, dev(points(F, vb)), dev(points(F, [crv.add(p, p) for p in vb])), dev(plain(some_scalars(F, 3, VBM_BITS, 1000), 4)),
                                VBM_BITS, 3, wit, n, n, row0=vbm0)
    eb = pts[53:55]
    ek = some_chals(2, ENDO_BITS, 1001)
    khip.endomul_witness_dev(fid, endo_limbs, dev(points(F, eb)), dev(points(F, [endo_oracle(fid, endo, b, k, ENDO_BITS)[1] for b, k in zip(eb, ek)])),
                             dev(plain(ek, 2)), ENDO_BITS, 2, wit, n, n, row0=endo0)
    pairs = [(pts[60], pts[61]), (pts[62], pts[62]), (pts[63], neg(F, pts[63])), (pts[64], pts[65])]
    khip.complete_add_witness_dev(fid, dev(points(F, [a for a, _ in pairs])), dev(points(F, [b for _, b in pairs])), 4, wit, n, n, row0=cadd0)
    khip.endomul_scalar_witness_dev(fid, dev(plain(some_chals(1, EMS_BITS, 1002), 2)), EMS_BITS, 1, wit, n, n, row0=ems0)
    rep = ix.witness_check(witness_dev=wit, flags=khip.WITNESS_GATES | khip.WITNESS_WIRES)          # no kh_sync in between
    assert rep.kind == khip.WITNESS_OK, khip.witness_report_message(rep)
    sections, _ph = ix.prove(witness_dev=wit, flags=khip.PROVE_CHECK)
    vix = khip.VerifierIndex.of(ix)
    proof = khip.Proof(sections)
    ok, _trace = khip.verify(vix, proof)
    assert ok
    # the check reads these very cells: another s1 in the second VarBaseMul instance's bit row, and its base row is the first that fails
    wit.upload_at(32 * (7 * n + vbm0 + 4 + 1), limbs(F, [12345]))
    rep = ix.witness_check(witness_dev=wit, flags=khip.WITNESS_GATES | khip.WITNESS_WIRES)
    assert (rep.kind, rep.row, rep.gate) == (khip.WITNESS_GATE, vbm0 + 4, gids["VarBaseMul"]), khip.witness_report_message(rep)
    assert rep.gate_rows_violated == 1
    proof.free(); vix.free(); ix.free(); wit.free(); srs.close()
    for b in bufs:
        b.free()


# ---- 7. ordering: upload -> VarBaseMul -> kh_witness_check without a kh_sync in between
def test_producer_and_check_are_ordered_on_the_main_stream_and_on_a_private_context(khip, pool):
    fid, F, crv, pts = khip.FP, P.Fp, CURVES[0], pool[0]
    srs = khip.Srs.create(khip.VESTA, 1 << 7)
    gids = khip.gate_ids()
    inst = 8
    types = [gids["VarBaseMul"], khip.GATE_ZERO] * 2 * inst
    wires = np.array([[(r, c) for c in range(7)] for r in range(len(types))], dtype=np.uint32)
    ix = khip.NativeProverIndex.create(srs, types, wires, np.zeros((len(types), 15, 4), dtype=np.uint64))
    n = 1 << ix.shape()[0]
    bases = pts[70:70 + inst]
    ks = some_scalars(F, inst, VBM_BITS, 1100)

    def sequence():
        wit = khip.DevBuf(32 * 15 * n).zero()
        b = khip.DevBuf(64 * inst).upload(points(F, bases)); a = khip.DevBuf(64 * inst).upload(points(F, [crv.add(p, p) for p in bases]))
        s = khip.DevBuf(32 * inst).upload(plain(ks, 4))
        khip.varbasemul_witness_dev(fid, b, a, s, VBM_BITS, inst, wit, n, n)
        rep = ix.witness_check(witness_dev=wit, flags=khip.WITNESS_GATES | khip.WITNESS_WIRES)
        assert rep.kind == khip.WITNESS_OK, khip.witness_report_message(rep)
        out = wit.download((15, n, 4))
        for buf in (wit, b, a, s):
            buf.free()
        return out

    shared = sequence()
    assert shared[7, 1].any()                                  # an s1 cell: the rows were written
    lib = khip.raw()
    assert lib.kh_private_context_begin() == 0
    try:
        private = sequence()
    finally:
        assert lib.kh_private_context_end() == 0
    assert private.tobytes() == shared.tobytes()
    ix.free(); srs.close()


# ---- 8. refusals: KH_E_INVALID with a text that names the call, before anything is launched, nothing written
def test_refusals_leave_everything_untouched(khip):
    lib = khip.raw()
    n = 3
    pts1 = sentinel_buf(khip, 2 * n); pts2 = sentinel_buf(khip, 2 * n); sc = sentinel_buf(khip, n)
    wit = sentinel_buf(khip, 15 * COL_LEN)
    out = sentinel_buf(khip, 2 * n); out_n = sentinel_buf(khip, n)
    flags = sentinel_buf(khip, 1)
    vp = C.c_void_p
    rows_t = C.c_uint32 * 3
    endo = (C.c_uint64 * 4)(1, 2, 3, 4)

    def cadd(field=0, a=pts1.ptr, b=pts2.ptr, k=n, rows=None, row0=0, row_stride=1, w=wit.ptr, col_stride=COL_LEN, col_len=COL_LEN, o=out.ptr):
        return lib.kh_complete_add_witness_dev(field, vp(a), vp(b), k, rows, row0, row_stride, vp(w), col_stride, col_len, vp(o))

    def vbm(field=0, b=pts1.ptr, a=pts2.ptr, s=sc.ptr, bits=10, k=n, rows=None, row0=0, row_stride=4, w=wit.ptr, col_stride=COL_LEN, col_len=COL_LEN,
            oa=out.ptr, on=out_n.ptr, f=flags.ptr, bit=0):
        return lib.kh_varbasemul_witness_dev(field, vp(b), vp(a), vp(s), bits, k, rows, row0, row_stride, vp(w), col_stride, col_len, vp(oa), vp(on), vp(f), bit)

    def emul(field=0, e=endo, b=pts1.ptr, a=pts2.ptr, s=sc.ptr, bits=8, k=n, rows=None, row0=0, row_stride=3, w=wit.ptr, col_stride=COL_LEN,
             col_len=COL_LEN, oa=out.ptr, on=out_n.ptr, f=flags.ptr, bit=0):
        return lib.kh_endomul_witness_dev(field, e, vp(b), vp(a), vp(s), bits, k, rows, row0, row_stride, vp(w), col_stride, col_len, vp(oa), vp(on), vp(f), bit)

    def ems(field=0, s=sc.ptr, bits=32, k=n, rows=None, row0=0, row_stride=2, w=wit.ptr, col_stride=COL_LEN, col_len=COL_LEN, es=endo, o=out_n.ptr):
        return lib.kh_endomul_scalar_witness_dev(field, vp(s), bits, k, rows, row0, row_stride, vp(w), col_stride, col_len, es, vp(o))

    calls = {"kh_complete_add_witness_dev": (cadd, 1), "kh_varbasemul_witness_dev": (vbm, 4), "kh_endomul_witness_dev": (emul, 3),
             "kh_endomul_scalar_witness_dev": (ems, 2)}
    refused = []
    for name, (call, inst) in calls.items():
        refused += [
            (name, "unknown field", lambda call=call: call(field=2), None),
            (name, "null witness", lambda call=call: call(w=None), None),
            (name, "unaligned witness", lambda call=call: call(w=wit.ptr + 8, col_len=COL_LEN - 1, col_stride=COL_LEN - 1), None),
            (name, "byte count overflows", lambda call=call: call(col_stride=1 << 62), None),
            (name, "too many instances", lambda call=call: call(k=1 << 40, col_len=1 << 50, col_stride=1 << 50), None),
            (name, "an instance past the end", lambda call=call, inst=inst: call(rows=rows_t(0, 20, COL_LEN - inst + 1)), "instance 2"),
            (name, "row_stride below the instance", lambda call=call, inst=inst: call(row_stride=inst - 1), None),
            (name, "the last instance past the end", lambda call=call, inst=inst: call(row0=COL_LEN - inst * n + 1, row_stride=inst), None),
            (name, "col_len below one instance", lambda call=call, inst=inst: call(k=1, col_len=inst - 1, col_stride=inst - 1), None),
            (name, "col_stride < col_len", lambda call=call: call(col_stride=COL_LEN - 1), None),
        ]
    refused += [
        ("kh_complete_add_witness_dev", "null p1", lambda: cadd(a=None), None),
        ("kh_complete_add_witness_dev", "null p2", lambda: cadd(b=None), None),
        ("kh_complete_add_witness_dev", "unaligned p2", lambda: cadd(b=pts2.ptr + 8, k=n - 1), None),
        ("kh_complete_add_witness_dev", "unaligned out", lambda: cadd(o=out.ptr + 8, k=n - 1), None),
        ("kh_varbasemul_witness_dev", "null base", lambda: vbm(b=None), None),
        ("kh_varbasemul_witness_dev", "null acc0", lambda: vbm(a=None), None),
        ("kh_varbasemul_witness_dev", "null scalars", lambda: vbm(s=None), None),
        ("kh_varbasemul_witness_dev", "unaligned scalars", lambda: vbm(s=sc.ptr + 8, k=n - 1), None),
        ("kh_varbasemul_witness_dev", "unaligned out_n", lambda: vbm(on=out_n.ptr + 8, k=n - 1), None),
        ("kh_varbasemul_witness_dev", "flag bit 32", lambda: vbm(bit=32), None),
        ("kh_endomul_witness_dev", "null endo", lambda: emul(e=None), None),
        ("kh_endomul_witness_dev", "null chals", lambda: emul(s=None), None),
        ("kh_endomul_witness_dev", "unaligned base", lambda: emul(b=pts1.ptr + 8, k=n - 1), None),
        ("kh_endomul_scalar_witness_dev", "null chals", lambda: ems(s=None), None),
        ("kh_endomul_scalar_witness_dev", "out without endo_scalar", lambda: ems(es=None), None),
    ]
    for bits in (0, 4, 7, 256, 260):
        refused.append(("kh_varbasemul_witness_dev", f"num_bits {bits}", lambda bits=bits: vbm(bits=bits), None))
    for bits in (0, 2, 6, 132):
        refused.append(("kh_endomul_witness_dev", f"num_bits {bits}", lambda bits=bits: emul(bits=bits), None))
    for bits in (0, 8, 24, 144):
        refused.append(("kh_endomul_scalar_witness_dev", f"num_bits {bits}", lambda bits=bits: ems(bits=bits), None))
    for name, what, call, needle in refused:
        assert call() == khip.E_INVALID, (name, what)
        text = lib.kh_last_error().decode()
        assert name in text, (name, what, text)
        if needle:
            assert needle in text, (name, what, text)
    for buf, elems in ((pts1, 2 * n), (pts2, 2 * n), (sc, n), (wit, 15 * COL_LEN), (out, 2 * n), (out_n, n), (flags, 1)):
        assert np.array_equal(buf.download((elems, 4)), np.tile(SENTINEL, (elems, 1)))
    # ... and what is allowed: n == 0 with null pointers, nothing launched
    assert lib.kh_complete_add_witness_dev(0, None, None, 0, None, 0, 0, None, 0, 0, None) == 0
    assert lib.kh_varbasemul_witness_dev(1, None, None, None, 255, 0, None, 0, 0, None, 0, 0, None, None, None, 0) == 0
    assert lib.kh_endomul_witness_dev(0, None, None, None, None, 128, 0, None, 0, 0, None, 0, 0, None, None, None, 0) == 0
    assert lib.kh_endomul_scalar_witness_dev(1, None, 128, 0, None, 0, 0, None, 0, 0, None, None) == 0
    for buf in (pts1, pts2, sc, wit, out, out_n, flags):
        buf.free()
