"""Wires between the gadgets on the device (csrc/wiring.hip: kh_witness_gather_dev, kh_witness_scatter_dev, kh_generic_witness_dev) against Python
integers, and circuits whose gadgets are chained on the device through real wires: the And gadget of and.rs from its two 64-bit inputs alone (up to
the reference's seeded whole-proof vector), a chain of the curve gates and a chain of the limb gates, each held to the oracle's composed witness, the
product's witness check with copy constraints, its prover and its verifier.  Buffers are sentinel-filled as in the two gadget test files: a cell
holds the expected value where a call assigns one and the sentinel everywhere else."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest

from oracle import circuit as CC
from oracle import gates as G
from oracle import pasta as P
from oracle import poseidon as S
from oracle import views as V

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_curve_gadgets_dev import endo_of, msb_bits, points  # noqa: E402
from test_gpu_limb_gadgets_dev import SENTINEL, SIZES, flag_word, mont, plain, range_check_rows, rot_rows, sentinel_buf, sentinel_words  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = (P.Fp, P.Fq)
FIELD, INT256, INT128, LIMB88, U64 = range(5)              # KH_CELL_*: test_formats_are_the_header_s holds them to the header
FORMATS = (FIELD, INT256, INT128, LIMB88, U64)
WORDS = {FIELD: 4, INT256: 4, INT128: 2, LIMB88: 2, U64: 1}
NARROW_BITS = {INT128: 128, LIMB88: 88, U64: 64}
COL_LEN, COL_STRIDE = 50, 64


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def test_formats_are_the_header_s(khip):
    assert (khip.CELL_FIELD, khip.CELL_INT256, khip.CELL_INT128, khip.CELL_LIMB88, khip.CELL_U64) == FORMATS
    assert khip.CELL_WORDS == WORDS


# ------------------------------------------------------------------------------------------------------------ formats and buffers
def bound(F, fmt):
    """values of a format are below this"""
    return 1 << NARROW_BITS[fmt] if fmt in NARROW_BITS else F.p


def words_of(F, fmt, vals):
    """the dense side: the values of a call in `fmt`, as one array of uint64 words (a narrow format carries the low bits)"""
    if fmt == FIELD:
        return mont(F, vals).reshape(-1)
    return plain([v % (1 << NARROW_BITS[fmt]) if fmt in NARROW_BITS else v for v in vals], WORDS[fmt]).reshape(-1)


def random_witness(F, rnd, col_stride=COL_STRIDE):
    """15 columns of random canonical elements as integers"""
    return [[rnd.randrange(F.p) for _ in range(col_stride)] for _ in range(15)]


def witness_limbs(F, vals):
    return mont(F, [v for col in vals for v in col]).reshape(15, -1, 4)


def some_cells(rnd, n, col_len=COL_LEN, repeats=True):
    """n (row, column) pairs over all 15 columns: row 0 and row col_len - 1 first, then random ones; with repeats, every fifth is an earlier one"""
    cells = [(0, rnd.randrange(15)), (col_len - 1, rnd.randrange(15))]
    seen = set(cells)
    while len(cells) < n:
        if repeats and len(cells) % 5 == 4:
            cells.append(cells[rnd.randrange(len(cells))])
            continue
        c = (rnd.randrange(col_len), rnd.randrange(15))
        if c not in seen:
            seen.add(c); cells.append(c)
    return cells[:n]


def gather(khip, fid, wit, cells, fmt, flags=None, bit=0, col_stride=COL_STRIDE, col_len=COL_LEN):
    """one kh_witness_gather_dev into a sentinel-filled buffer: (the words of the n values, the four words past them)"""
    count = WORDS[fmt] * len(cells)
    out = sentinel_words(khip, count + 4)
    khip.witness_gather_dev(fid, wit, col_stride, col_len, cells, fmt, out, flags=flags, bit=bit)
    got = out.download((count + 4,))
    out.free()
    return got[:count], got[count:]


def sentinel_tail(count):
    return np.resize(SENTINEL, count + 4)[count:]


# ------------------------------------------------------------------------------------------------------------ 1. gather, every format
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("fid", [0, 1])
def test_gather_every_format(khip, fid, fmt):
    F = FIELDS[fid]
    rnd = random.Random(1000 + 10 * fid + fmt)
    for n in SIZES:
        vals = random_witness(F, rnd)
        cells = some_cells(rnd, n)
        if fmt in NARROW_BITS:
            for r, c in cells:
                vals[c][r] = rnd.randrange(bound(F, fmt))
        limbs = witness_limbs(F, vals)
        wit = khip.DevBuf(limbs.nbytes).upload(limbs)
        flags = khip.DevBuf(4).zero()
        got, tail = gather(khip, fid, wit, cells, fmt, flags=flags, bit=9)
        assert np.array_equal(got, words_of(F, fmt, [vals[c][r] for r, c in cells])), (fmt, n)
        assert np.array_equal(tail, sentinel_tail(len(got))), "the output buffer past its end"
        assert np.array_equal(wit.download(limbs.shape), limbs), "the witness was written"
        assert flag_word(flags) == 0
        wit.free(); flags.free()


# ------------------------------------------------------------------------------------------------------------ 2. fit boundaries
def boundary_values(F):
    return [0, 1, (1 << 64) - 1, 1 << 64, (1 << 88) - 1, 1 << 88, (1 << 128) - 1, 1 << 128, F.p - 1, (1 << 256) % F.p]


@pytest.mark.parametrize("fid", [0, 1])
def test_gather_fit_boundaries(khip, fid):
    F = FIELDS[fid]
    rnd = random.Random(1100 + fid)
    B = boundary_values(F)
    vals = random_witness(F, rnd)
    cells = [(3 * k + 1, (4 * k + 2) % 15) for k in range(len(B))]
    for (r, c), v in zip(cells, B):
        vals[c][r] = v
    # 130 cells that fit every format, for the one too-wide value among them
    many = [c for c in some_cells(rnd, 170, repeats=False) if c not in cells][:130]
    for r, c in many:
        vals[c][r] = rnd.randrange(1 << 64)
    limbs = witness_limbs(F, vals)
    wit = khip.DevBuf(limbs.nbytes).upload(limbs)
    PRESET = 0xa5a5005a                                            # bit 7 clear
    for fmt in FORMATS:
        wide = [fmt in NARROW_BITS and v >= bound(F, fmt) for v in B]
        # each value alone: the low bits, and the flag exactly when the value is too wide; the word's other bits stay
        for cell, v, w in zip(cells, B, wide):
            flags = khip.DevBuf(4).upload(np.array([PRESET], dtype=np.uint32))
            got, _tail = gather(khip, fid, wit, [cell], fmt, flags=flags, bit=7)
            assert np.array_equal(got, words_of(F, fmt, [v])), (fmt, hex(v))
            assert flag_word(flags) == PRESET | (int(w) << 7), (fmt, hex(v), hex(flag_word(flags)))
            flags.free()
        # all ten in one call
        flags = khip.DevBuf(4).zero()
        got, tail = gather(khip, fid, wit, cells, fmt, flags=flags, bit=31)
        assert np.array_equal(got, words_of(F, fmt, B)), fmt
        assert np.array_equal(tail, sentinel_tail(len(got)))
        assert flag_word(flags) == (int(any(wide)) << 31) & 0xffffffff
        flags.free()
        # one too-wide value among 130: the other 129 are exact (and so are its own low bits)
        if fmt in NARROW_BITS:
            where = 77
            mixed = list(many); mixed[where] = cells[B.index(1 << NARROW_BITS[fmt])]
            flags = khip.DevBuf(4).zero()
            got, _tail = gather(khip, fid, wit, mixed, fmt, flags=flags, bit=0)
            assert np.array_equal(got, words_of(F, fmt, [vals[c][r] for r, c in mixed])), fmt
            assert flag_word(flags) == 1
            flags.free()
            flags = khip.DevBuf(4).zero()
            gather(khip, fid, wit, many, fmt, flags=flags, bit=0)
            assert flag_word(flags) == 0, "130 values that fit"
            flags.free()
    wit.free()


# ------------------------------------------------------------------------------------------------------------ 3. scatter
def scatter(khip, fid, fmt, cells, vals, skip=(), flag=0, raw=None):
    """one kh_witness_scatter_dev into a sentinel-filled witness: exactly the named cells change (those of `skip` are unspecified), the values are
    not written, the flag word (bit 5) is `flag`.  raw: the words to upload instead of words_of(vals)."""
    F = FIELDS[fid]
    words = words_of(F, fmt, vals) if raw is None else raw
    v = khip.DevBuf(words.nbytes).upload(words)
    wit = sentinel_buf(khip, 15 * COL_STRIDE)
    flags = khip.DevBuf(4).zero()
    khip.witness_scatter_dev(fid, v, fmt, cells, wit, COL_STRIDE, COL_LEN, flags=flags, bit=5)
    got = wit.download((15, COL_STRIDE, 4))
    want = np.tile(SENTINEL, (15, COL_STRIDE, 1))
    for (r, c), m in zip(cells, mont(F, vals)):
        want[c, r] = m
    diff = (got != want).any(axis=2)
    for i in skip:
        diff[cells[i][1], cells[i][0]] = False
    assert not diff.any(), (fmt, "cells (column, row) that differ", np.argwhere(diff)[:8].tolist())
    assert np.array_equal(v.download(words.shape), words), "the values were written"
    assert flag_word(flags) == flag << 5, (fmt, flag_word(flags))
    for b in (v, wit, flags):
        b.free()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("fid", [0, 1])
def test_scatter_every_format(khip, fid, fmt):
    F = FIELDS[fid]
    rnd = random.Random(1200 + 10 * fid + fmt)
    for n in SIZES:
        scatter(khip, fid, fmt, some_cells(rnd, n, repeats=False), [rnd.randrange(bound(F, fmt)) for _ in range(n)])
    B = [v for v in boundary_values(F) if v < bound(F, fmt)]
    scatter(khip, fid, fmt, some_cells(rnd, len(B), repeats=False), B)


@pytest.mark.parametrize("fid", [0, 1])
def test_scatter_flags_values_that_do_not_fit(khip, fid):
    F = FIELDS[fid]
    rnd = random.Random(1300 + fid)
    n = 130
    cells = some_cells(rnd, n, repeats=False)
    for fmt, too_wide in ((INT256, F.p), (INT256, (1 << 256) - 1), (LIMB88, 1 << 88), (LIMB88, (1 << 128) - 1)):
        vals = [rnd.randrange(bound(F, fmt)) for _ in range(n)]
        raw = words_of(F, fmt, vals).reshape(n, WORDS[fmt]).copy()
        raw[101] = plain([too_wide], WORDS[fmt])[0]
        scatter(khip, fid, fmt, cells, vals, skip=(101,), flag=1, raw=raw.reshape(-1))
    scatter(khip, fid, INT256, cells, [F.p - 1] * n)               # the largest value that fits: the word stays 0
    scatter(khip, fid, LIMB88, cells, [(1 << 88) - 1] * n)


# ------------------------------------------------------------------------------------------------------------ 4. round trip, no kh_sync in between
def round_trips(khip, fid):
    F = FIELDS[fid]
    rnd = random.Random(1400 + fid)
    n = 70
    for fmt in FORMATS:
        cells = some_cells(rnd, n, repeats=False)
        words = words_of(F, fmt, [rnd.randrange(bound(F, fmt)) for _ in range(n)])
        v = khip.DevBuf(words.nbytes).upload(words)
        wit = sentinel_buf(khip, 15 * COL_STRIDE)
        flags = khip.DevBuf(4).zero()
        out = sentinel_words(khip, len(words) + 4)
        khip.witness_scatter_dev(fid, v, fmt, cells, wit, COL_STRIDE, COL_LEN, flags=flags, bit=0)
        khip.witness_gather_dev(fid, wit, COL_STRIDE, COL_LEN, cells, fmt, out, flags=flags, bit=1)
        got = out.download((len(words) + 4,))
        assert np.array_equal(got[:-4], words), fmt
        assert np.array_equal(got[-4:], sentinel_tail(len(words)))
        assert flag_word(flags) == 0
        for b in (v, wit, flags, out):
            b.free()


@pytest.mark.parametrize("fid", [0, 1])
def test_round_trip_on_the_main_stream_and_on_a_private_context(khip, fid):
    round_trips(khip, fid)
    lib = khip.raw()
    assert lib.kh_private_context_begin() == 0
    try:
        round_trips(khip, fid)
    finally:
        assert lib.kh_private_context_end() == 0


# ------------------------------------------------------------------------------------------------------------ 5. generic halves
def generic_specs(F, rnd):
    """(name, the half's five coefficients l r o m c, whether r_dev is given)"""
    p = F.p
    return [("Add", CC.generic_spec(p, "Add"), True), ("Mul", CC.generic_spec(p, "Mul"), True), ("Plus", CC.generic_spec(p, "Plus", cst=rnd.randrange(p)), True),
            ("Const", CC.generic_spec(p, "Const", cst=rnd.randrange(p)), True), ("Pub", CC.generic_spec(p, "Pub"), True),
            ("Add(right=-1, output=-2)", CC.generic_spec(p, "Add", right=-1, output=-2), True),
            ("random", [rnd.randrange(1, p) for _ in range(5)], True), ("Add, r_dev = NULL", CC.generic_spec(p, "Add"), False)]


def generic_output(F, co, l, r):
    cl, cr, c_o, cm, cc = co
    inv = pow(c_o, -1, F.p) if c_o else 0                         # c_o = 0: the row defines nothing, o = 0
    return -(cl * l + cr * r + cm * l * r + cc) * inv % F.p


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("fid", [0, 1])
def test_generic_halves(khip, fid, half):
    F = FIELDS[fid]
    rnd = random.Random(1500 + 2 * fid + half)
    assert generic_specs(F, rnd)[3][1][2] == 0 and generic_specs(F, rnd)[4][1][2] == 0
    for n in SIZES:
        ls, rs = [rnd.randrange(F.p) for _ in range(n)], [rnd.randrange(F.p) for _ in range(n)]
        lm, rm = mont(F, ls), mont(F, rs)
        l_dev, r_dev = khip.DevBuf(lm.nbytes).upload(lm), khip.DevBuf(rm.nbytes).upload(rm)
        slots = list(range(n + 2)); random.Random(n).shuffle(slots)
        placements = (dict(rows=None, row0=3, row_stride=2, col_len=2 * n + 3, col_stride=2 * n + 3),
                      dict(rows=[2 * s for s in slots[:n]], row0=0, row_stride=1, col_len=2 * n + 3, col_stride=2 * n + 8))
        for name, co, with_r in generic_specs(F, rnd):
            rr = rs if with_r else [0] * n
            os_ = [generic_output(F, co, l, r) for l, r in zip(ls, rr)]
            om = mont(F, os_)
            for pl in placements:
                starts = np.array(pl["rows"] if pl["rows"] is not None else [pl["row0"] + i * pl["row_stride"] for i in range(n)])
                wit = sentinel_buf(khip, 15 * pl["col_stride"])
                out = sentinel_buf(khip, n + 1)
                khip.generic_witness_dev(fid, mont(F, co), half, l_dev, r_dev if with_r else None, n, wit, pl["col_stride"], pl["col_len"], rows=pl["rows"],
                                         row0=pl["row0"], row_stride=pl["row_stride"], out=out)
                want = np.tile(SENTINEL, (15, pl["col_stride"], 1))
                want[3 * half, starts] = lm; want[3 * half + 1, starts] = mont(F, rr); want[3 * half + 2, starts] = om
                bad = np.argwhere((wit.download(want.shape) != want).any(axis=2))
                assert bad.size == 0, (name, n, "cells (column, row) that differ", bad[:8].tolist())
                assert np.array_equal(out.download((n + 1, 4)), np.vstack([om, SENTINEL[None]])), (name, n)
                wit.free(); out.free()
        l_dev.free(); r_dev.free()


# ------------------------------------------------------------------------------------------------------------ the And gadget on the device
def build_and(khip, fid, in1, in2, count, wit, col_stride, col_len, row0=0, flags=None, bit=0):
    """and.rs's gadget for `count` pairs of 64-bit operands (4 words each at in1, in2), instance i at row0 + 6 i: the xor rows, then the double generic
    row from the cells the rows before it hold -- (in1, in2, in1 + in2) and (in1 + in2, in1 ^ in2, in1 & in2).  Returns a scratch buffer to free
    once the stream has passed."""
    F = FIELDS[fid]
    rows = [row0 + 6 * i for i in range(count)]
    khip.xor_witness_dev(fid, in1, in2, 64, count, wit, col_stride, col_len, row0=row0, row_stride=6, flags=flags, bit=bit)
    t = khip.DevBuf(64 * count)
    khip.witness_gather_dev(fid, wit, col_stride, col_len, [(r, 0) for r in rows] + [(r, 1) for r in rows], FIELD, t)
    khip.generic_witness_dev(fid, mont(F, CC.generic_spec(F.p, "Add")), 0, t.view(0), t.view(32 * count), count, wit, col_stride, col_len, row0=row0 + 5,
                             row_stride=6)
    khip.witness_gather_dev(fid, wit, col_stride, col_len, [(r + 5, 2) for r in rows] + [(r, 2) for r in rows], FIELD, t)
    khip.generic_witness_dev(fid, mont(F, CC.generic_spec(F.p, "Add", right=-1, output=-2)), 1, t.view(0), t.view(32 * count), count, wit, col_stride, col_len,
                             row0=row0 + 5, row_stride=6)
    return t


@pytest.mark.parametrize("fid", [0, 1])
def test_and_gadget_from_two_words(khip, fid):
    F = FIELDS[fid]
    rnd = random.Random(1600 + fid)
    top = (1 << 64) - 1
    pairs = [(0, 0), (top, top), (top, 0)] + [(rnd.randrange(1 << 64), rnd.randrange(1 << 64)) for _ in range(62)]
    n, rows = len(pairs), 6 * len(pairs)
    assert n == 65
    want_rows = [r for a, b in pairs for r in G.and_witness(F, a, b, 8)]
    want = mont(F, [want_rows[r][c] for c in range(15) for r in range(rows)]).reshape(15, rows, 4)
    in1 = khip.DevBuf(32 * n).upload(plain([a for a, _ in pairs], 4)); in2 = khip.DevBuf(32 * n).upload(plain([b for _, b in pairs], 4))
    col_stride = rows + 3
    for filled in (False, True):
        wit = sentinel_buf(khip, 15 * col_stride) if filled else khip.DevBuf(32 * 15 * col_stride).zero()
        flags = khip.DevBuf(4).zero()
        t = build_and(khip, fid, in1, in2, n, wit, col_stride, rows, flags=flags)
        got = wit.download((15, col_stride, 4))
        expect = np.tile(SENTINEL, (15, col_stride, 1)) if filled else np.zeros((15, col_stride, 4), dtype=np.uint64)
        for i in range(n):                                        # the xor rows whole, cells 0..5 of the generic row
            expect[:, 6 * i:6 * i + 5] = want[:, 6 * i:6 * i + 5]
            expect[:6, 6 * i + 5] = want[:6, 6 * i + 5]
        bad = np.argwhere((got != expect).any(axis=2))
        assert bad.size == 0, ("cells (column, row) that differ", bad[:8].tolist())
        if not filled:
            assert np.array_equal(got[:, :rows], want), "the six rows of every instance are and_witness's"
        assert flag_word(flags) == 0
        for b in (wit, flags, t):
            b.free()
    in1.free(); in2.free()


def records(F, gates):
    """(gate types, wires (rows, 7, 2), coefficients (rows, 15, 4)) of an oracle gate list, as kh_prover_index_create takes them"""
    types = [g["typ"] for g in gates]
    wires = np.array([g["wires"] for g in gates], dtype=np.uint32).reshape(len(gates), 7, 2)
    co = np.stack([mont(F, list(g["coeffs"]) + [0] * (15 - len(g["coeffs"]))) for g in gates])
    return types, wires, co


# ------------------------------------------------------------------------------------------------------------ 7. the reference's whole-proof bytes
def test_device_built_and_witness_reproduces_the_reference_whole_proof_bytes(khip):
    """and.rs's seeded proof (tests/golden/and_serialization_regression.json), as test_gpu_index_create_lookup.py reproduces it from a host witness --
    here the witness is built on the device from the two uploaded words.  A witness given on the device carries its own zero-knowledge rows, so the
    test draws them from the reference's stream where the prover would (15 columns, each from its last row backwards: prover.rs:254-266)."""
    from proof_systems_amd import prover
    from test_gpu_index_create_lookup import serialized
    from test_gpu_proof_fixtures import first_difference
    with open(os.path.join(HERE, "golden", "and_serialization_regression.json")) as f:
        kat = json.load(f)
    seed, want = bytes(kat["seed"]), bytes.fromhex(kat["proof_hex"])
    C_ = P.VESTA; Fo = C_.scalar; F = prover.Fld(khip.FP)
    std = P.StdRng(seed)
    gates = []
    CC.extend_and(Fo.p, gates, 8)
    in1 = CC.gen_field_with_bits(std, 64); in2 = CC.gen_field_with_bits(std, 64)
    types, wires, co = records(Fo, gates)
    ix = prover.CreatedIndex(khip.Srs.create(khip.VESTA, 1 << 16), types, wires, co)
    n, zk = ix.n, ix.zk_rows
    wit = khip.DevBuf(32 * 15 * n).zero()
    a = khip.DevBuf(32).upload(plain([in1], 4)); b = khip.DevBuf(32).upload(plain([in2], 4))
    flags = khip.DevBuf(4).zero()
    t = build_and(khip, khip.FP, a, b, 1, wit, n, n, flags=flags)
    rng = V.RefRng(std)
    zkr = F.limbs_many(F.rand_many(rng, 15 * zk)).reshape(15, zk, 4)[:, ::-1, :]
    wit.upload_2d((n - zk) * 32, n * 32, np.ascontiguousarray(zkr))
    got = serialized(C_, ix, prover.create_proof_native(ix, None, rng, witness_on_device=wit))
    assert flag_word(flags) == 0
    assert len(want) == 6160
    assert got == want, "the proof of the device-built witness differs from the reference's bytes: first in " + first_difference(C_, got, want)
    for buf in (wit, a, b, flags, t):
        buf.free()
    ix.free()


# ------------------------------------------------------------------------------------------------------------ 8. a chain of curve gadgets
def wire(gates, pairs):
    for a, b in pairs:
        CC.connect_cell_pair(gates, a, b)


def curve_chain():
    """Poseidon -> VarBaseMul -> (EndoMulScalar -> EndoMul) -> CompleteAdd -> Generic over Fp, composed with the oracle's generators: the gate
    list with its wires, the witness rows, and the inputs no gadget produces"""
    F, crv, p = P.Fp, P.PALLAS, P.Fp.p
    rnd = random.Random(1800)
    par = S.params("fp")
    state = [rnd.randrange(p) for _ in range(3)]
    pw, pco, pout = G.poseidon_witness(F, state, par["mds"], par["rc"], 11)
    gates = [CC.gate("Poseidon", r, pco[r]) for r in range(11)] + [CC.gate("Zero", 11)]
    rows = [list(r) for r in pw]
    base = crv.mul(crv.gen, 0x1234567); acc0 = crv.add(base, base)
    vw, vacc, vn = G.varbasemul_witness(F, base, msb_bits(pout[0], 255), acc0)                 # the scalar is cell (11, 0)
    assert vn == pout[0] and len(vw) == 102
    gates += [CC.gate("VarBaseMul" if j % 2 == 0 else "Zero", 12 + j) for j in range(102)]
    rows += vw
    chal = rnd.randrange(1 << 127, 1 << 128)
    ew, _scalar = G.endomul_scalar_witness(F, chal, P.endos(crv)[1], 128)
    assert len(ew) == 8 and ew[7][1] == chal
    gates += [CC.gate("EndoMulScalar", 114 + j) for j in range(8)]
    rows += ew
    T = crv.mul(crv.gen, 0x7654321); tacc0 = crv.add(T, T)
    mw, macc, mn = G.endomul_witness(F, P.endos(crv)[0], T, msb_bits(chal, 128), tacc0)          # the challenge is cell (121, 1)
    assert mn == chal and len(mw) == 33
    gates += [CC.gate("EndoMul", 122 + j) for j in range(32)] + [CC.gate("Zero", 154)]
    rows += mw
    cw = G.complete_add_witness(F, vacc, macc)
    assert (rows[113][0], rows[113][1]) == vacc and (rows[154][4], rows[154][5]) == macc and cw[6] == 0
    gates.append(CC.gate("CompleteAdd", 155))
    rows.append(cw)
    add, sub = CC.generic_spec(p, "Add"), CC.generic_spec(p, "Add", right=-1, output=-2)
    gates.append(CC.generic_gadget(p, 156, add, sub))
    rows.append([cw[4], pout[1], generic_output(F, add, cw[4], pout[1]), cw[5], pout[2], generic_output(F, sub, cw[5], pout[2])] + [0] * 9)
    wire(gates, [((11, 0), (112, 5)), ((121, 1), (154, 6)), ((113, 0), (155, 0)), ((113, 1), (155, 1)), ((154, 4), (155, 2)), ((154, 5), (155, 3)),
                 ((155, 4), (156, 0)), ((11, 1), (156, 1)), ((155, 5), (156, 3)), ((11, 2), (156, 4))])
    assert len(gates) == len(rows) == 157
    return gates, rows, dict(state=state, base=base, acc0=acc0, chal=chal, T=T, tacc0=tacc0)


def columns(rows):
    return [[r[c] for r in rows] for c in range(15)]


def test_chain_of_curve_gadgets_with_real_wires(khip):
    from proof_systems_amd import prover
    fid, F = khip.FP, P.Fp
    gates, rows, inp = curve_chain()
    cs = CC.build(F, gates)
    CC.verify_witness(cs, columns(rows))
    spoiled = columns(rows); spoiled[5][112] = (spoiled[5][112] + 1) % F.p            # (a changed (11, 0) fails the Poseidon gate of row 10 first)
    with pytest.raises(AssertionError, match="copy constraint"):
        CC.verify_witness(cs, spoiled)
    srs = khip.Srs.create(khip.VESTA, 1 << 8)
    ix = prover.CreatedIndex(srs, *records(F, gates), public=0)
    n = ix.n
    assert n == 1 << 8 == cs["n"]
    _e, endo_limbs = endo_of(khip, fid)
    bufs = []

    def dev(arr):
        bufs.append(khip.DevBuf(arr.nbytes).upload(arr))
        return bufs[-1]

    def room(nbytes):
        bufs.append(khip.DevBuf(nbytes))
        return bufs[-1]

    wit = khip.DevBuf(32 * 15 * n).zero()
    flags = khip.DevBuf(4).zero()
    # the whole witness, no kh_sync and no download in between
    khip.poseidon_gate_witness_dev(fid, dev(mont(F, inp["state"])), 1, wit, n, n, row0=0)
    scalar = room(32)
    khip.witness_gather_dev(fid, wit, n, n, [(11, 0)], INT256, scalar)
    khip.varbasemul_witness_dev(fid, dev(points(F, [inp["base"]])), dev(points(F, [inp["acc0"]])), scalar, 255, 1, wit, n, n, row0=12, flags=flags, bit=0)
    khip.endomul_scalar_witness_dev(fid, dev(plain([inp["chal"]], 2)), 128, 1, wit, n, n, row0=114)
    chal = room(16)
    khip.witness_gather_dev(fid, wit, n, n, [(121, 1)], INT128, chal, flags=flags, bit=1)
    khip.endomul_witness_dev(fid, endo_limbs, dev(points(F, [inp["T"]])), dev(points(F, [inp["tacc0"]])), chal, 128, 1, wit, n, n, row0=122, flags=flags, bit=2)
    pts = room(128)
    khip.witness_gather_dev(fid, wit, n, n, [(113, 0), (113, 1), (154, 4), (154, 5)], FIELD, pts)
    khip.complete_add_witness_dev(fid, pts.view(0), pts.view(64), 1, wit, n, n, row0=155)
    ops = room(128)
    khip.witness_gather_dev(fid, wit, n, n, [(155, 4), (11, 1), (155, 5), (11, 2)], FIELD, ops)
    khip.generic_witness_dev(fid, mont(F, CC.generic_spec(F.p, "Add")), 0, ops.view(0), ops.view(32), 1, wit, n, n, row0=156)
    khip.generic_witness_dev(fid, mont(F, CC.generic_spec(F.p, "Add", right=-1, output=-2)), 1, ops.view(64), ops.view(96), 1, wit, n, n, row0=156)
    both = khip.WITNESS_GATES | khip.WITNESS_WIRES
    rep = ix.native.witness_check(witness_dev=wit, flags=both)
    assert rep.kind == khip.WITNESS_OK, khip.witness_report_message(rep)
    got = wit.download((15, n, 4))
    want = mont(F, [v for col in columns(rows) for v in col]).reshape(15, 157, 4)
    bad = np.argwhere((got[:, :157] != want).any(axis=2))
    assert bad.size == 0, ("cells (column, row) that differ from the oracle's", bad[:8].tolist())
    assert not got[:, 157:].any()
    assert flag_word(flags) == 0
    sections, _ph = ix.native.prove(witness_dev=wit, flags=khip.PROVE_CHECK)
    vix = khip.VerifierIndex.of(ix.native)
    proof = khip.Proof(sections)
    ok, _trace = khip.verify(vix, proof)
    assert ok
    # another n_acc in (112, 5): the cell wired to it, (11, 0), is the first that is disconnected
    khip.witness_scatter_dev(fid, dev(plain([12345], 4)), INT256, [(112, 5)], wit, n, n)
    rep = ix.native.witness_check(witness_dev=wit, flags=both)
    assert (rep.kind, rep.row, rep.col, rep.wired_row, rep.wired_col) == (khip.WITNESS_DISCONNECTED, 11, 0, 112, 5), khip.witness_report_message(rep)
    proof.free(); vix.free(); ix.free(); srs.close()
    for b in bufs + [wit, flags]:
        b.free()


# ------------------------------------------------------------------------------------------------------------ 9. a chain of limb gadgets
def limb_chain():
    """Rot64 -> Xor -> Rot64 -> multi-range-check, and an And gadget on two of their cells, over Fp: gate list with wires, witness rows, inputs"""
    F, p = P.Fp, P.Fp.p
    rnd = random.Random(1900)
    w, in2 = rnd.randrange(1 << 63, 1 << 64), rnd.randrange(1 << 64)
    rot = lambda row, r: [CC.gate("Rot64", row, [1 << r]), CC.gate("RangeCheck0", row + 1), CC.gate("RangeCheck0", row + 2)]
    gates = rot(0, 7)
    r0, rotated = rot_rows(w, 7)
    rows = [list(r) for r in r0]
    assert CC.extend_xor_gadget(p, gates, 64) == 8
    rows += G.xor_witness(F, rotated, in2, 64)
    x = rotated ^ in2
    gates += rot(8, 63)
    r8, rotated2 = rot_rows(x, 63)
    rows += [list(r) for r in r8]
    gates += [CC.gate("RangeCheck0", 11), CC.gate("RangeCheck0", 12), CC.gate("RangeCheck1", 13), CC.gate("Zero", 14)]
    rows += [list(r) for r in range_check_rows([rotated2, x, r0[0][2]], 0)]
    assert CC.extend_and(p, gates, 8) == 21
    rows += G.and_witness(F, rotated2, w, 8)
    assert (rows[0][1], rows[3][2], rows[8][1], rows[0][2], rows[0][0]) == (rotated, x, rotated2, r0[0][2], w)
    wire(gates, [((0, 1), (3, 0)), ((3, 2), (8, 0)), ((8, 1), (11, 0)), ((3, 2), (12, 0)), ((0, 2), (13, 0)), ((8, 1), (15, 0)), ((0, 0), (15, 1))])
    assert len(gates) == len(rows) == 21
    return gates, rows, dict(w=w, in2=in2)


def test_chain_of_limb_gadgets_with_real_wires_and_lookups(khip):
    from proof_systems_amd import prover
    fid, F = khip.FP, P.Fp
    gates, rows, inp = limb_chain()
    srs = khip.Srs.create(khip.VESTA, 1 << 13)
    ix = prover.CreatedIndex(srs, *records(F, gates), public=0)
    n = ix.n
    assert n == 1 << 13
    bufs = []

    def dev(arr):
        bufs.append(khip.DevBuf(arr.nbytes).upload(arr))
        return bufs[-1]

    def room(nbytes):
        bufs.append(khip.DevBuf(nbytes))
        return bufs[-1]

    wit = khip.DevBuf(32 * 15 * n).zero()
    flags = khip.DevBuf(4).zero()
    khip.rot64_witness_dev(fid, dev(plain([inp["w"]], 1)), 7, 1, wit, n, n, row0=0)
    in1 = room(32)
    khip.witness_gather_dev(fid, wit, n, n, [(0, 1)], INT256, in1)
    khip.xor_witness_dev(fid, in1, dev(plain([inp["in2"]], 4)), 64, 1, wit, n, n, row0=3, flags=flags, bit=0)
    word = room(8)
    khip.witness_gather_dev(fid, wit, n, n, [(3, 2)], U64, word, flags=flags, bit=1)
    khip.rot64_witness_dev(fid, word, 63, 1, wit, n, n, row0=8)
    limbs = room(48)
    khip.witness_gather_dev(fid, wit, n, n, [(8, 1), (3, 2), (0, 2)], LIMB88, limbs, flags=flags, bit=2)
    khip.range_check_witness_dev(fid, limbs, 1, wit, n, n, row0=11, flags=flags, bit=3)
    ops = room(64)
    khip.witness_gather_dev(fid, wit, n, n, [(8, 1), (0, 0)], INT256, ops)
    bufs.append(build_and(khip, fid, ops.view(0), ops.view(32), 1, wit, n, n, row0=15, flags=flags, bit=4))
    every = khip.WITNESS_GATES | khip.WITNESS_WIRES | khip.WITNESS_LOOKUPS
    rep, lk = khip.witness_check_full(ix.native, witness_dev=wit, flags=every)
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0, khip.witness_lookup_message(rep, lk)
    assert flag_word(flags) == 0
    got = wit.download((15, n, 4))
    want = mont(F, [v for col in columns(rows) for v in col]).reshape(15, 21, 4)
    bad = np.argwhere((got[:, :21] != want).any(axis=2))
    assert bad.size == 0, ("cells (column, row) that differ from the composed witness", bad[:8].tolist())
    assert not got[:, 21:].any()
    sections, _ph = ix.native.prove(witness_dev=wit, flags=khip.PROVE_CHECK)
    vix = khip.VerifierIndex.of(ix.native)
    proof = khip.Proof(sections)
    ok, _trace = khip.verify(vix, proof)
    assert ok
    # another word in (15, 1), the And gadget's second operand.  Its cycle is (0, 0) -> (20, 1) -> (15, 1) -> (0, 0): extend_and had wired (15, 1) to
    # (20, 1) before the chain's wire joined (0, 0), so row 0 still agrees with row 20 and (15, 1) is the first cell that differs from its target
    assert gates[0]["wires"][0] == (20, 1) and gates[15]["wires"][1] == (0, 0) and gates[20]["wires"][1] == (15, 1)
    khip.witness_scatter_dev(fid, dev(plain([inp["w"] ^ 1], 1)), U64, [(15, 1)], wit, n, n)
    rep, lk = khip.witness_check_full(ix.native, witness_dev=wit, flags=every)
    assert (rep.kind, rep.row, rep.col, rep.wired_row, rep.wired_col) == (khip.WITNESS_DISCONNECTED, 15, 1, 0, 0), khip.witness_lookup_message(rep, lk)
    assert rep.cells_disconnected == 2
    proof.free(); vix.free(); ix.free(); srs.close()
    for b in bufs + [wit, flags]:
        b.free()


def test_the_composed_limb_chain_satisfies_the_oracle():
    """the copy constraints and the gates of the chain the device test builds, on the CPU"""
    gates, rows, _inp = limb_chain()
    cs = CC.build(P.Fp, gates)
    assert cs["n"] == 1 << 13
    CC.verify_witness(cs, columns(rows))
    spoiled = columns(rows); spoiled[1][15] ^= 1
    with pytest.raises(AssertionError, match="copy constraint"):
        CC.verify_witness(cs, spoiled)


# ------------------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_leave_everything_untouched(khip):
    lib = khip.raw()
    n, LEN = 3, 40
    wit = sentinel_buf(khip, 15 * LEN)
    data = sentinel_buf(khip, 2 * n)                               # out_dev / values_dev / l_dev
    other = sentinel_buf(khip, n)                                  # r_dev
    out = sentinel_buf(khip, n)
    flags = sentinel_buf(khip, 1)
    vp = C.c_void_p
    cells_t, co_t, rows_t = C.c_uint32 * 6, C.c_uint64 * 20, C.c_uint32 * 3
    good = cells_t(0, 0, 5, 14, LEN - 1, 6)
    co = co_t(*([1, 0, 0, 0] * 5))

    def gat(field=0, w=wit.ptr, col_stride=LEN, col_len=LEN, cells=good, k=n, fmt=FIELD, o=data.ptr, f=flags.ptr, bit=0):
        return lib.kh_witness_gather_dev(field, vp(w), col_stride, col_len, cells, k, fmt, vp(o), vp(f), bit)

    def sca(field=0, o=data.ptr, fmt=FIELD, cells=good, k=n, w=wit.ptr, col_stride=LEN, col_len=LEN, f=flags.ptr, bit=0):
        return lib.kh_witness_scatter_dev(field, vp(o), fmt, cells, k, vp(w), col_stride, col_len, vp(f), bit)

    def gen(field=0, c=co, half=0, o=data.ptr, r=other.ptr, k=n, rows=None, row0=0, row_stride=1, w=wit.ptr, col_stride=LEN, col_len=LEN, out_=out.ptr):
        return lib.kh_generic_witness_dev(field, c, half, vp(o), vp(r), k, rows, row0, row_stride, vp(w), col_stride, col_len, vp(out_))

    refused = []
    for name, call in (("kh_witness_gather_dev", gat), ("kh_witness_scatter_dev", sca), ("kh_generic_witness_dev", gen)):
        refused += [
            (name, "unknown field", lambda call=call: call(field=2), None),
            (name, "null witness", lambda call=call: call(w=None), None),
            (name, "null dense buffer", lambda call=call: call(o=None), None),
            (name, "unaligned dense buffer", lambda call=call: call(o=data.ptr + 8, k=n - 1), None),
            (name, "unaligned witness", lambda call=call: call(w=wit.ptr + 8, col_len=LEN - 1, col_stride=LEN - 1), None),
            (name, "byte count overflows", lambda call=call: call(col_stride=1 << 62), None),
            (name, "too many values", lambda call=call: call(k=1 << 40, col_len=1 << 50, col_stride=1 << 50), None),
            (name, "col_stride < col_len", lambda call=call: call(col_stride=LEN - 1), None),
        ]
    for name, call in (("kh_witness_gather_dev", gat), ("kh_witness_scatter_dev", sca)):
        refused += [
            (name, "format 5", lambda call=call: call(fmt=5), None),
            (name, "format -1", lambda call=call: call(fmt=-1), None),
            (name, "null cells", lambda call=call: call(cells=None), None),
            (name, "a KH_CELL_U64 buffer at 4 bytes", lambda call=call: call(fmt=U64, o=data.ptr + 4), None),
            (name, "a KH_CELL_LIMB88 buffer at 8 bytes", lambda call=call: call(fmt=LIMB88, o=data.ptr + 8), None),
            (name, "a row past the end", lambda call=call: call(cells=cells_t(0, 0, 5, 14, LEN, 6)), "cell 2"),
            (name, "column 15", lambda call=call: call(cells=cells_t(0, 0, 5, 15, LEN - 1, 6)), "cell 1"),
            (name, "col_len 0", lambda call=call: call(col_len=0), "cell 0"),
            (name, "flag bit 32", lambda call=call: call(bit=32), None),
            (name, "unaligned flag word", lambda call=call: call(f=flags.ptr + 2), None),
        ]
    refused += [
        ("kh_generic_witness_dev", "half 2", lambda: gen(half=2), None),
        ("kh_generic_witness_dev", "half -1", lambda: gen(half=-1), None),
        ("kh_generic_witness_dev", "null coeffs", lambda: gen(c=None), None),
        ("kh_generic_witness_dev", "unaligned r_dev", lambda: gen(r=other.ptr + 8, k=n - 1), None),
        ("kh_generic_witness_dev", "unaligned out_dev", lambda: gen(out_=out.ptr + 8, k=n - 1), None),
        ("kh_generic_witness_dev", "an instance past the end", lambda: gen(rows=rows_t(0, 20, LEN)), "instance 2"),
        ("kh_generic_witness_dev", "row_stride 0", lambda: gen(row_stride=0), None),
        ("kh_generic_witness_dev", "the last instance past the end", lambda: gen(row0=LEN - n + 1), None),
        ("kh_generic_witness_dev", "col_len 0", lambda: gen(k=1, col_len=0), None),
    ]
    for name, what, call, needle in refused:
        assert call() == khip.E_INVALID, (name, what)
        text = lib.kh_last_error().decode()
        assert name in text, (name, what, text)
        if needle:
            assert needle in text, (name, what, text)
    for buf, elems in ((wit, 15 * LEN), (data, 2 * n), (other, n), (out, n), (flags, 1)):
        assert np.array_equal(buf.download((elems, 4)), np.tile(SENTINEL, (elems, 1)))
    # ... and what is allowed: n == 0 with null pointers, nothing launched; KH_CELL_U64 values that are only 8-byte aligned
    assert lib.kh_witness_gather_dev(0, None, 0, 0, None, 0, FIELD, None, None, 0) == 0
    assert lib.kh_witness_scatter_dev(1, None, U64, None, 0, None, 0, 0, None, 0) == 0
    assert lib.kh_generic_witness_dev(0, None, 1, None, None, 0, None, 0, 0, None, 0, 0, None) == 0
    words = khip.DevBuf(32).upload(plain([0, 7, 9, 0], 1))
    assert lib.kh_witness_scatter_dev(0, vp(words.ptr + 8), U64, cells_t(1, 0, 2, 3, 0, 0), 2, vp(wit.ptr), LEN, LEN, None, 0) == 0
    assert lib.kh_witness_gather_dev(0, vp(wit.ptr), LEN, LEN, cells_t(2, 3, 1, 0, 0, 0), 2, U64, vp(words.ptr + 8), None, 0) == 0
    assert words.download((4,)).tolist() == [0, 9, 7, 0]
    got = wit.download((15, LEN, 4))
    assert np.array_equal(got[0, 1], mont(P.Fp, [7])[0]) and np.array_equal(got[3, 2], mont(P.Fp, [9])[0]) and np.array_equal(got[0, 0], SENTINEL)
    for buf in (wit, data, other, out, flags, words):
        buf.free()
