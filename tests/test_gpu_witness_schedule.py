"""Witness schedules (csrc/witness_schedule.cpp, k_cell_moves in csrc/wiring.hip): the circuits test_gpu_wiring_dev.py chains with direct calls,
described once as steps over an arena and run with one call per proof.  Every comparison is exact: against the oracle's composed rows, against
the direct calls' witness for the same inputs, against Python integers for the fused wire steps.
How the arena is read back (it belongs to the run and has no debug hook): the steps that follow scatter each arena extent, in its own format,
into target cells of the same witness, and a caller-buffer KH_STEP_GATHER of those cells delivers the words to a bound buffer -- so a test sees
both the cells a fused scatter wrote and the words a fused gather produced."""
import ctypes as C
import json
import os
import random
import sys
import threading

import numpy as np
import pytest

from oracle import circuit as CC
from oracle import gates as G
from oracle import pasta as P
from oracle import views as V

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_curve_gadgets_dev import endo_of, points  # noqa: E402
from test_gpu_limb_gadgets_dev import SENTINEL, SIZES, flag_word, mont, plain, sentinel_buf, sentinel_words  # noqa: E402
from test_gpu_wiring_dev import (FIELD, FORMATS, INT128, INT256, LIMB88, NARROW_BITS, U64, WORDS, bound, columns, curve_chain, limb_chain,  # noqa: E402
                                 random_witness, records, some_cells, witness_limbs, words_of)

pytestmark = pytest.mark.gpu
FIELDS = (P.Fp, P.Fq)


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def arena(offset):
    return (-1, offset)                                            # KH_REF_ARENA: test_constants_are_the_header_s


def test_constants_are_the_header_s(khip):
    assert (khip.REF_NONE, khip.REF_ARENA, khip.STEP_NO_FLAG) == (-2, -1, 255)
    assert [khip.STEP_GATHER, khip.STEP_SCATTER, khip.STEP_GENERIC, khip.STEP_POSEIDON, khip.STEP_COMPLETE_ADD, khip.STEP_VARBASEMUL, khip.STEP_ENDOMUL,
            khip.STEP_ENDOMUL_SCALAR, khip.STEP_RANGE_CHECK, khip.STEP_XOR, khip.STEP_ROT64, khip.STEP_FF_ADD, khip.STEP_FF_MUL] == list(range(13))


def unmont(F, limbs):
    """(..., 4) Montgomery limbs -> integers, flat"""
    rinv = pow(1 << 256, -1, F.p)
    return [int.from_bytes(x.tobytes(), "little") * rinv % F.p for x in np.ascontiguousarray(limbs).reshape(-1, 4)]


# ------------------------------------------------------------------------------------------------------------ the curve chain as steps
CURVE_BUFS = ("state", "base", "acc0", "chal", "T", "tacc0")     # the bound buffers, in this order
CURVE_ARENA = 320                                                  # scalar 0 | challenge 32 | the two points 64 | the generic operands 192


def curve_steps(khip, endo_limbs):
    K, F = khip, P.Fp
    add, sub = mont(F, CC.generic_spec(F.p, "Add")), mont(F, CC.generic_spec(F.p, "Add", right=-1, output=-2))
    return [
        dict(op=K.STEP_POSEIDON, n=1, row0=0, row_stride=12, **{"in": [(0, 0)]}),
        dict(op=K.STEP_GATHER, cells=[(11, 0)], format=INT256, out=[arena(0)]),
        dict(op=K.STEP_VARBASEMUL, n=1, row0=12, row_stride=102, param=255, flag_bit=0, **{"in": [(1, 0), (2, 0), arena(0)]}),
        dict(op=K.STEP_ENDOMUL_SCALAR, n=1, row0=114, row_stride=8, param=128, **{"in": [(3, 0)]}),
        dict(op=K.STEP_GATHER, cells=[(121, 1)], format=INT128, out=[arena(32)], flag_bit=1),
        dict(op=K.STEP_ENDOMUL, n=1, row0=122, row_stride=33, param=128, consts=endo_limbs, flag_bit=2, **{"in": [(4, 0), (5, 0), arena(32)]}),
        dict(op=K.STEP_GATHER, cells=[(113, 0), (113, 1), (154, 4), (154, 5)], format=FIELD, out=[arena(64)]),
        dict(op=K.STEP_COMPLETE_ADD, n=1, row0=155, row_stride=1, **{"in": [arena(64), arena(128)]}),
        dict(op=K.STEP_GATHER, cells=[(155, 4), (11, 1), (155, 5), (11, 2)], format=FIELD, out=[arena(192)]),
        dict(op=K.STEP_GENERIC, n=1, row0=156, row_stride=1, param=0, consts=add, **{"in": [arena(192), arena(224)]}),
        dict(op=K.STEP_GENERIC, n=1, row0=156, row_stride=1, param=1, consts=sub, **{"in": [arena(256), arena(288)]}),
    ]


def curve_inputs(seed):
    """fresh inputs of the chain, of the kinds curve_chain() draws"""
    crv, rnd = P.PALLAS, random.Random(seed)
    base = crv.mul(crv.gen, rnd.randrange(1, 1 << 60)); T = crv.mul(crv.gen, rnd.randrange(1, 1 << 60))
    return dict(state=[rnd.randrange(P.Fp.p) for _ in range(3)], base=base, acc0=crv.add(base, base), chal=rnd.randrange(1 << 127, 1 << 128), T=T,
                tacc0=crv.add(T, T))


def curve_buffers(khip, inp):
    F = P.Fp
    arrs = dict(state=mont(F, inp["state"]), base=points(F, [inp["base"]]), acc0=points(F, [inp["acc0"]]), chal=plain([inp["chal"]], 2),
                T=points(F, [inp["T"]]), tacc0=points(F, [inp["tacc0"]]))
    return [khip.DevBuf(arrs[k].nbytes).upload(arrs[k]) for k in CURVE_BUFS]


def curve_direct(khip, bufs, wit, n, flags, endo_limbs, scratch=None):
    """the chain with direct calls, as test_chain_of_curve_gadgets_with_real_wires issues them; returns the scratch buffers (taken from `scratch` when given)"""
    fid, F = khip.FP, P.Fp
    state, base, acc0, chal_in, T, tacc0 = bufs
    scalar, chal, pts, ops = scratch or (khip.DevBuf(32), khip.DevBuf(16), khip.DevBuf(128), khip.DevBuf(128))
    khip.poseidon_gate_witness_dev(fid, state, 1, wit, n, n, row0=0)
    khip.witness_gather_dev(fid, wit, n, n, [(11, 0)], INT256, scalar)
    khip.varbasemul_witness_dev(fid, base, acc0, scalar, 255, 1, wit, n, n, row0=12, flags=flags, bit=0)
    khip.endomul_scalar_witness_dev(fid, chal_in, 128, 1, wit, n, n, row0=114)
    khip.witness_gather_dev(fid, wit, n, n, [(121, 1)], INT128, chal, flags=flags, bit=1)
    khip.endomul_witness_dev(fid, endo_limbs, T, tacc0, chal, 128, 1, wit, n, n, row0=122, flags=flags, bit=2)
    khip.witness_gather_dev(fid, wit, n, n, [(113, 0), (113, 1), (154, 4), (154, 5)], FIELD, pts)
    khip.complete_add_witness_dev(fid, pts.view(0), pts.view(64), 1, wit, n, n, row0=155)
    khip.witness_gather_dev(fid, wit, n, n, [(155, 4), (11, 1), (155, 5), (11, 2)], FIELD, ops)
    khip.generic_witness_dev(fid, mont(F, CC.generic_spec(F.p, "Add")), 0, ops.view(0), ops.view(32), 1, wit, n, n, row0=156)
    khip.generic_witness_dev(fid, mont(F, CC.generic_spec(F.p, "Add", right=-1, output=-2)), 1, ops.view(64), ops.view(96), 1, wit, n, n, row0=156)
    return [scalar, chal, pts, ops]


@pytest.fixture(scope="module")
def curve(khip):
    """the chain, composed once, and its schedule over 2^8 rows"""
    gates, rows, inp = curve_chain()
    _e, endo_limbs = endo_of(khip, khip.FP)
    sched = khip.WitnessSchedule.create(khip.FP, 1 << 8, curve_steps(khip, endo_limbs), arena_bytes=CURVE_ARENA, n_bufs=len(CURVE_BUFS))
    yield dict(gates=gates, rows=rows, inp=inp, sched=sched, endo=endo_limbs)
    sched.free()


def free_all(*bufs):
    for b in bufs:
        b.free()


# ------------------------------------------------------------------------------------------------------------ 1. the curve chain
def test_curve_chain_as_a_schedule(khip, curve):
    from proof_systems_amd import prover
    F, n = P.Fp, 1 << 8
    gates, rows, sched = curve["gates"], curve["rows"], curve["sched"]
    info = sched.info()
    assert (info["steps"], info["launch_groups"]) == (11, 11), info      # the gathers are apart: nothing to fuse
    assert info["resident_bytes"] == 16 * 10 and info["run_bytes"] > CURVE_ARENA
    srs = khip.Srs.create(khip.VESTA, n)
    ix = prover.CreatedIndex(srs, *records(F, gates), public=0)
    assert ix.n == n
    bufs = curve_buffers(khip, curve["inp"])
    wit, flags = khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(4).zero()
    sched.run(bufs, wit, flags=flags)                              # ... and no kh_sync from here to the verifier
    both = khip.WITNESS_GATES | khip.WITNESS_WIRES
    rep = ix.native.witness_check(witness_dev=wit, flags=both)
    assert rep.kind == khip.WITNESS_OK, khip.witness_report_message(rep)
    sections, _ph = ix.native.prove(witness_dev=wit, flags=khip.PROVE_CHECK)
    vix = khip.VerifierIndex.of(ix.native)
    proof = khip.Proof(sections)
    ok, _trace = khip.verify(vix, proof)
    assert ok
    got = wit.download((15, n, 4))
    want = mont(F, [v for col in columns(rows) for v in col]).reshape(15, 157, 4)
    bad = np.argwhere((got[:, :157] != want).any(axis=2))
    assert bad.size == 0, ("cells (column, row) that differ from the oracle's", bad[:8].tolist())
    assert not got[:, 157:].any()
    assert flag_word(flags) == 0
    # the same schedule, fresh inputs, a second witness: the direct calls' witness for them, and a satisfying one
    inp2 = curve_inputs(4100)
    bufs2 = curve_buffers(khip, inp2)
    wit2, wit3, flags2 = khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(4).zero()
    sched.run(bufs2, wit2, flags=flags2)
    scratch = curve_direct(khip, bufs2, wit3, n, flags2, curve["endo"])
    got2 = wit2.download((15, n, 4))
    assert np.array_equal(got2, wit3.download((15, n, 4)))
    assert not np.array_equal(got2, got) and flag_word(flags2) == 0
    vals = unmont(F, got2[:, :157])
    CC.verify_witness(CC.build(F, gates), [vals[157 * c:157 * (c + 1)] for c in range(15)])
    proof.free(); vix.free(); ix.free(); srs.close()
    free_all(wit, flags, wit2, wit3, flags2, *bufs, *bufs2, *scratch)


# ------------------------------------------------------------------------------------------------------------ the And gadget as steps
def and_steps(khip, in1, in2, t, count, row0=0, rows=None, flag_bit=None):
    """build_and's five calls: `count` gadgets at row0 + 6 i, or at rows[i]; in1, in2: refs of the operands (4 words each), t: an arena ref of 64 * count bytes"""
    K, F = khip, P.Fp
    starts = list(rows) if rows is not None else [row0 + 6 * i for i in range(count)]
    place = (lambda d: dict(rows=[r + d for r in starts])) if rows is not None else (lambda d: dict(row0=row0 + d, row_stride=6))
    t2 = (t[0], t[1] + 32 * count)
    return [
        dict(op=K.STEP_XOR, n=count, param=64, flag_bit=flag_bit, out=[None], **{"in": [in1, in2]}, **place(0)),
        dict(op=K.STEP_GATHER, cells=[(r, 0) for r in starts] + [(r, 1) for r in starts], format=FIELD, out=[t]),
        dict(op=K.STEP_GENERIC, n=count, param=0, consts=mont(F, CC.generic_spec(F.p, "Add")), **{"in": [t, t2]}, **place(5)),
        dict(op=K.STEP_GATHER, cells=[(r + 5, 2) for r in starts] + [(r, 2) for r in starts], format=FIELD, out=[t]),
        dict(op=K.STEP_GENERIC, n=count, param=1, consts=mont(F, CC.generic_spec(F.p, "Add", right=-1, output=-2)), **{"in": [t, t2]}, **place(5)),
    ]


# ------------------------------------------------------------------------------------------------------------ 2. the limb chain
# bound: the word, the Xor's second operand.  arena: in1 0 | word 32 | limbs 48 | And operands 96 | And scratch 160
LIMB_ARENA = 224


def limb_steps(khip):
    K = khip
    return [
        dict(op=K.STEP_ROT64, n=1, row0=0, row_stride=3, param=7, **{"in": [(0, 0)]}),
        dict(op=K.STEP_GATHER, cells=[(0, 1)], format=INT256, out=[arena(0)]),
        dict(op=K.STEP_XOR, n=1, row0=3, row_stride=5, param=64, flag_bit=0, **{"in": [arena(0), (1, 0)]}),
        dict(op=K.STEP_GATHER, cells=[(3, 2)], format=U64, out=[arena(32)], flag_bit=1),
        dict(op=K.STEP_ROT64, n=1, row0=8, row_stride=3, param=63, **{"in": [arena(32)]}),
        dict(op=K.STEP_GATHER, cells=[(8, 1), (3, 2), (0, 2)], format=LIMB88, out=[arena(48)], flag_bit=2),
        dict(op=K.STEP_RANGE_CHECK, n=1, row0=11, row_stride=4, param=0, flag_bit=3, **{"in": [arena(48)]}),
        dict(op=K.STEP_GATHER, cells=[(8, 1), (0, 0)], format=INT256, out=[arena(96)]),
    ] + and_steps(khip, arena(96), arena(128), arena(160), 1, row0=15, flag_bit=4)


def test_limb_chain_as_a_schedule(khip):
    from proof_systems_amd import prover
    fid, F = khip.FP, P.Fp
    gates, rows, inp = limb_chain()
    srs = khip.Srs.create(khip.VESTA, 1 << 13)
    ix = prover.CreatedIndex(srs, *records(F, gates), public=0)
    n = ix.n
    assert n == 1 << 13
    steps = limb_steps(khip)
    sched = khip.WitnessSchedule.create(fid, n, steps, arena_bytes=LIMB_ARENA, n_bufs=2)
    assert sched.info()["launch_groups"] == len(steps) == 13
    w, in2 = khip.DevBuf(16).upload(plain([inp["w"]], 1)), khip.DevBuf(32).upload(plain([inp["in2"]], 4))
    wit, flags = khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(4).zero()
    sched.run([w, in2], wit, flags=flags)
    every = khip.WITNESS_GATES | khip.WITNESS_WIRES | khip.WITNESS_LOOKUPS
    rep, lk = khip.witness_check_full(ix.native, witness_dev=wit, flags=every)
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0, khip.witness_lookup_message(rep, lk)
    sections, _ph = ix.native.prove(witness_dev=wit, flags=khip.PROVE_CHECK)
    vix = khip.VerifierIndex.of(ix.native)
    proof = khip.Proof(sections)
    ok, _trace = khip.verify(vix, proof)
    assert ok
    assert flag_word(flags) == 0
    got = wit.download((15, n, 4))
    want = mont(F, [v for col in columns(rows) for v in col]).reshape(15, 21, 4)
    bad = np.argwhere((got[:, :21] != want).any(axis=2))
    assert bad.size == 0, ("cells (column, row) that differ from the composed witness", bad[:8].tolist())
    assert not got[:, 21:].any()
    proof.free(); vix.free(); ix.free(); srs.close(); sched.free()
    free_all(w, in2, wit, flags)


# ------------------------------------------------------------------------------------------------------------ 3. and.rs, the reference's bytes
def test_and_witness_by_one_schedule_run_reproduces_the_reference_whole_proof_bytes(khip):
    """test_device_built_and_witness_reproduces_the_reference_whole_proof_bytes with its five direct calls replaced by one run"""
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
    sched = khip.WitnessSchedule.create(khip.FP, n, and_steps(khip, (0, 0), (1, 0), arena(0), 1, flag_bit=0), arena_bytes=64, n_bufs=2)
    wit = khip.DevBuf(32 * 15 * n).zero()
    a = khip.DevBuf(32).upload(plain([in1], 4)); b = khip.DevBuf(32).upload(plain([in2], 4))
    flags = khip.DevBuf(4).zero()
    sched.run([a, b], wit, flags=flags)
    rng = V.RefRng(std)
    zkr = F.limbs_many(F.rand_many(rng, 15 * zk)).reshape(15, zk, 4)[:, ::-1, :]
    wit.upload_2d((n - zk) * 32, n * 32, np.ascontiguousarray(zkr))
    got = serialized(C_, ix, prover.create_proof_native(ix, None, rng, witness_on_device=wit))
    assert flag_word(flags) == 0
    assert len(want) == 6160
    assert got == want, "the proof of the scheduled witness differs from the reference's bytes: first in " + first_difference(C_, got, want)
    free_all(wit, a, b, flags)
    sched.free(); ix.free()


# ------------------------------------------------------------------------------------------------------------ fused wire steps
ROWS_SRC, COL_LEN, COL_STRIDE = 50, 128, 131                       # cells are read from rows 0..49 and written to rows 64..127


def fused_round_trip(khip, fid, jobs):
    """jobs = [(format, source cells, flag bit or None)], the source cells in rows < ROWS_SRC.  One schedule: a fused gather per job into the arena,
    a fused scatter per job from there to fresh target cells, a caller-buffer gather of each job's targets into the bound buffer.  Returns what was
    read and what to expect."""
    K, F = khip, FIELDS[fid]
    free = [(r, c) for r in range(64, COL_LEN) for c in range(15)]
    gathers, scatters, reads, off, out_off = [], [], [], 0, 0
    for fmt, cells, bit in jobs:
        size = (8 * WORDS[fmt] * len(cells) + 15) & ~15
        targets, free = free[:len(cells)], free[len(cells):]
        gathers.append(dict(op=K.STEP_GATHER, cells=cells, format=fmt, out=[arena(off)], flag_bit=bit))
        scatters.append(dict(op=K.STEP_SCATTER, cells=targets, format=fmt, **{"in": [arena(off)]}))
        reads.append(dict(op=K.STEP_GATHER, cells=targets, format=fmt, out=[(0, out_off)]))
        off += size; out_off += size
    sched = K.WitnessSchedule.create(fid, COL_LEN, gathers + scatters + reads, arena_bytes=off, n_bufs=1)
    return sched, [d["cells"] for d in scatters], out_off


def run_fused(khip, fid, sched, vals, out_bytes, preset=0):
    F = FIELDS[fid]
    before = np.tile(SENTINEL, (15, COL_STRIDE, 1))
    before[:, :ROWS_SRC] = witness_limbs(F, vals)[:, :ROWS_SRC]
    wit = khip.DevBuf(before.nbytes).upload(before)
    out = sentinel_words(khip, out_bytes // 8 + 4)
    flags = khip.DevBuf(4).upload(np.array([preset], dtype=np.uint32))
    sched.run([out], wit, col_stride=COL_STRIDE, flags=flags)
    got_out, got_wit, word = out.download((out_bytes // 8 + 4,)), wit.download(before.shape), flag_word(flags)
    free_all(wit, out, flags)
    return got_out, got_wit, before, word


def every_format_jobs(F, rnd, n):
    """a gather of n cells per format, and a witness whose cells fit the formats that read them"""
    vals = random_witness(F, rnd, COL_STRIDE)
    jobs = [(fmt, some_cells(rnd, n, col_len=ROWS_SRC), None) for fmt in FORMATS]
    for fmt, cells, _bit in jobs:                                  # (widest format first: a cell two of them read fits the narrower one)
        if fmt in NARROW_BITS:
            for r, c in cells:
                vals[c][r] = rnd.randrange(bound(F, fmt))
    return jobs, vals


def check_words(F, jobs, vals, got_out):
    off = 0
    for fmt, cells, _bit in jobs:
        count = WORDS[fmt] * len(cells)
        assert np.array_equal(got_out[off:off + count], words_of(F, fmt, [vals[c][r] for r, c in cells])), (fmt, len(cells))
        off += (count + 1) & ~1
    assert np.array_equal(got_out[off:], np.resize(SENTINEL, off + 4)[off:]), "the bound buffer past its end"


# ------------------------------------------------------------------------------------------------------------ 4. fused gathers
@pytest.mark.parametrize("fid", [0, 1])
def test_fused_gathers_of_every_format(khip, fid):
    """five consecutive arena gathers, one per format: the format changes inside a wave (n = 1, 63, 65) and at its boundary (64), over several blocks (130)"""
    F = FIELDS[fid]
    rnd = random.Random(4400 + fid)
    for n in SIZES:
        jobs, vals = every_format_jobs(F, rnd, n)
        sched, _targets, out_bytes = fused_round_trip(khip, fid, jobs)
        info = sched.info()
        assert (info["steps"], info["launch_groups"]) == (15, 1 + 1 + 5), (n, info)      # the gathers as one, the scatters as one, five reads
        assert info["resident_bytes"] == 16 * 10 * n + 5 * ((8 * n + 15) & ~15)        # a 16-byte move per fused cell, 8 bytes per cell of a read
        got_out, _wit, _before, word = run_fused(khip, fid, sched, vals, out_bytes)
        check_words(F, jobs, vals, got_out)
        assert word == 0
        sched.free()


# ------------------------------------------------------------------------------------------------------------ 5. flags inside one fused wave
@pytest.mark.parametrize("fid", [0, 1])
def test_flag_bits_of_five_steps_in_one_wave(khip, fid):
    F = FIELDS[fid]
    rnd = random.Random(4500 + fid)
    vals = random_witness(F, rnd, COL_STRIDE)
    cells = some_cells(rnd, 5, col_len=ROWS_SRC, repeats=False)
    jobs = [(FIELD, [cells[0]], 3), (U64, [cells[1]], 9), (INT256, [cells[2]], 17), (LIMB88, [cells[3]], 20), (INT128, [cells[4]], 31)]
    (r1, c1), (r3, c3), (r4, c4) = cells[1], cells[3], cells[4]
    vals[c1][r1], vals[c3][r3], vals[c4][r4] = 1 << 64, 1 << 88, (1 << 128) - 1
    sched, _targets, out_bytes = fused_round_trip(khip, fid, jobs)
    assert sched.info()["launch_groups"] == 1 + 1 + 5
    PRESET = 0x40040005                                            # bits 3, 9, 17, 20, 31 clear
    got_out, _wit, _before, word = run_fused(khip, fid, sched, vals, out_bytes, preset=PRESET)
    assert word == PRESET | (1 << 9) | (1 << 20), hex(word)
    check_words(F, jobs, vals, got_out)                            # the narrow formats deliver the low bits: 0 for 2^64 and 2^88
    assert got_out[4] == 0 and got_out[10] == 0 and got_out[11] == 0
    sched.free()


# ------------------------------------------------------------------------------------------------------------ 6. fused scatters, the sequential rule
@pytest.mark.parametrize("fid", [0, 1])
def test_fused_scatters_of_every_format(khip, fid):
    """the cells the fused scatters wrote: the values, and nothing else in a witness that is sentinel-filled from row ROWS_SRC on"""
    F = FIELDS[fid]
    rnd = random.Random(4600 + fid)
    for n in SIZES:
        jobs, vals = every_format_jobs(F, rnd, n)
        sched, targets, out_bytes = fused_round_trip(khip, fid, jobs)
        _out, got, want, word = run_fused(khip, fid, sched, vals, out_bytes)
        for (fmt, cells, _bit), tcells in zip(jobs, targets):
            for (r, c), m in zip(tcells, mont(F, [vals[sc][sr] for sr, sc in cells])):
                want[c, r] = m
        bad = np.argwhere((got != want).any(axis=2))
        assert bad.size == 0, (n, "cells (column, row) that differ", bad[:8].tolist())
        assert word == 0
        sched.free()


@pytest.mark.parametrize("fid", [0, 1])
def test_a_step_that_would_change_the_result_starts_a_new_group(khip, fid):
    K, F = khip, FIELDS[fid]
    rnd = random.Random(4700 + fid)
    vals = random_witness(F, rnd, COL_STRIDE)
    c1, c2, c3 = some_cells(rnd, 3, col_len=ROWS_SRC, repeats=False)
    t1, t2 = (70, 3), (99, 14)
    value = lambda cell: mont(F, [vals[cell[1]][cell[0]]])[0]
    read = dict(op=K.STEP_GATHER, cells=[t1, t2], format=FIELD, out=[(0, 0)])
    # two scatters with the same target: one after the other, the later value stands
    same_target = [dict(op=K.STEP_GATHER, cells=[c1], format=FIELD, out=[arena(0)]), dict(op=K.STEP_GATHER, cells=[c2, c3], format=FIELD, out=[arena(32)]),
                   dict(op=K.STEP_SCATTER, cells=[t1, t2], format=FIELD, **{"in": [arena(0)]}), dict(op=K.STEP_SCATTER, cells=[t1], format=FIELD, **{"in": [arena(64)]}), read]
    # two gathers whose outputs overlap: the second one's value stands in the shared slot
    overlap = [dict(op=K.STEP_GATHER, cells=[c1, c2], format=FIELD, out=[arena(0)]), dict(op=K.STEP_GATHER, cells=[c3], format=FIELD, out=[arena(32)]),
               dict(op=K.STEP_SCATTER, cells=[t1, t2], format=FIELD, **{"in": [arena(0)]}), read]
    # ... and the same steps where nothing collides fuse
    apart = [dict(op=K.STEP_GATHER, cells=[c1, c2], format=FIELD, out=[arena(0)]), dict(op=K.STEP_GATHER, cells=[c3], format=FIELD, out=[arena(64)]),
             dict(op=K.STEP_SCATTER, cells=[t1], format=FIELD, **{"in": [arena(64)]}), dict(op=K.STEP_SCATTER, cells=[t2], format=FIELD, **{"in": [arena(0)]}), read]
    for name, steps, groups, want in (("same target", same_target, 1 + 2 + 1, (c3, c2)), ("overlap", overlap, 2 + 1 + 1, (c1, c3)), ("apart", apart, 1 + 1 + 1, (c3, c1))):
        sched = K.WitnessSchedule.create(fid, COL_LEN, steps, arena_bytes=96, n_bufs=1)
        assert sched.info()["launch_groups"] == groups, name
        got_out, got, before, _word = run_fused(khip, fid, sched, vals, 64)
        assert np.array_equal(got_out[:8].reshape(2, 4), np.stack([value(want[0]), value(want[1])])), name
        before[t1[1], t1[0]], before[t2[1], t2[0]] = value(want[0]), value(want[1])
        assert np.array_equal(got, before), name
        sched.free()


# ------------------------------------------------------------------------------------------------------------ 7. resident rows[]
def test_and_gadgets_at_explicit_rows_run_twice(khip):
    fid, F = khip.FP, P.Fp
    rnd = random.Random(4800)
    n = 65
    slots = list(range(n + 2)); random.Random(n).shuffle(slots)
    starts = [6 * s for s in slots[:n]]
    col_len = 6 * (n + 2); col_stride = col_len + 5
    sched = khip.WitnessSchedule.create(fid, col_len, and_steps(khip, (0, 0), (1, 0), arena(0), n, rows=starts, flag_bit=6), arena_bytes=64 * n, n_bufs=2)
    info = sched.info()
    assert info["launch_groups"] == 5 and info["resident_bytes"] == 3 * ((4 * n + 15) & ~15) + 2 * 16 * 2 * n      # three rows[] tables, two fused gathers
    top = (1 << 64) - 1
    for run in range(2):
        pairs = [(0, 0), (top, top), (top, 0)][run:] + [(rnd.randrange(1 << 64), rnd.randrange(1 << 64)) for _ in range(62 + run)]
        assert len(pairs) == n
        in1 = khip.DevBuf(32 * n).upload(plain([a for a, _ in pairs], 4)); in2 = khip.DevBuf(32 * n).upload(plain([b for _, b in pairs], 4))
        wit, flags = sentinel_buf(khip, 15 * col_stride), khip.DevBuf(4).zero()
        sched.run([in1, in2], wit, col_stride=col_stride, flags=flags)
        expect = np.tile(SENTINEL, (15, col_stride, 1))
        for r, (a, b) in zip(starts, pairs):                      # the xor rows whole, cells 0..5 of the generic row
            w = G.and_witness(F, a, b, 8)
            want = mont(F, [w[k][c] for c in range(15) for k in range(6)]).reshape(15, 6, 4)
            expect[:, r:r + 5] = want[:, :5]
            expect[:6, r + 5] = want[:6, 5]
        bad = np.argwhere((wit.download(expect.shape) != expect).any(axis=2))
        assert bad.size == 0, (run, "cells (column, row) that differ", bad[:8].tolist())
        assert flag_word(flags) == 0
        free_all(in1, in2, wit, flags)
    sched.free()


# ------------------------------------------------------------------------------------------------------------ 8. nothing is staged per run
def test_a_run_stages_no_table(khip):
    fid, F = khip.FP, P.Fp
    rnd = random.Random(4900)
    staged = lambda: khip.counter("table_staged_words")
    vals = random_witness(F, rnd, COL_STRIDE)
    limbs = witness_limbs(F, vals)
    wit, out = khip.DevBuf(limbs.nbytes).upload(limbs), khip.DevBuf(32 * 130)
    cells = some_cells(rnd, 130, col_len=ROWS_SRC)
    s0 = staged()
    khip.witness_gather_dev(fid, wit, COL_STRIDE, COL_LEN, cells, FIELD, out)
    s1 = staged()
    assert s1 - s0 == 260
    jobs, vals = every_format_jobs(F, rnd, 130)
    sched, _targets, out_bytes = fused_round_trip(khip, fid, jobs)
    s2 = staged()
    assert s2 - s1 == sched.info()["resident_bytes"] // 4 > 0
    for _ in range(3):
        got_out, _w, _b, _f = run_fused(khip, fid, sched, vals, out_bytes)
        check_words(F, jobs, vals, got_out)
    assert staged() == s2
    sched.free()
    free_all(wit, out)


# ------------------------------------------------------------------------------------------------------------ 9. two threads, one schedule
def test_two_threads_run_one_schedule_on_private_contexts(khip, curve):
    n, sched, lib = 1 << 8, curve["sched"], khip.raw()
    inputs = [curve_inputs(4910), curve_inputs(4920)]
    alone = []
    for inp in inputs:                                             # what a lone run gives
        bufs, wit, flags = curve_buffers(khip, inp), khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(4).zero()
        sched.run(bufs, wit, flags=flags)
        alone.append(wit.download((15, n, 4)))
        assert flag_word(flags) == 0
        free_all(wit, flags, *bufs)
    assert not np.array_equal(alone[0], alone[1])
    work = [(curve_buffers(khip, inp), khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(4).zero()) for inp in inputs]
    khip.sync()
    errors, gate = [], threading.Barrier(2)

    def worker(k):
        try:
            assert lib.kh_private_context_begin() == 0
            try:
                gate.wait(timeout=60)
                for _ in range(3):                                 # (the same witness again: both threads are inside runs at the same time)
                    sched.run(work[k][0], work[k][1], flags=work[k][2])
                khip.sync()
            finally:
                assert lib.kh_private_context_end() == 0
        except BaseException as e:                                 # noqa: BLE001 -- reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, (bufs, wit, flags) in enumerate(work):
        assert np.array_equal(wit.download((15, n, 4)), alone[k]), k
        assert flag_word(flags) == 0
        free_all(wit, flags, *bufs)


# ------------------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_at_create_and_at_run(khip):
    K, lib = khip, khip.raw()
    LEN = 40
    co = np.array([1, 0, 0, 0] * 5, dtype=np.uint64)
    UNTOUCHED = 0x5a5a5a5a

    def refused(steps, needles, field=0, col_len=LEN, arena_bytes=256, n_bufs=2):
        arr, _keep = K.WitnessSchedule.pack(steps)
        h = C.c_void_p(UNTOUCHED)
        assert lib.kh_witness_schedule_create(field, col_len, arr, len(steps), arena_bytes, n_bufs, C.byref(h)) == K.E_INVALID, needles
        text = lib.kh_last_error().decode()
        for needle in ("kh_witness_schedule_create",) + tuple(needles):
            assert needle in text, (needles, text)
        assert h.value == UNTOUCHED, "*out was written"

    ok = dict(op=K.STEP_POSEIDON, n=1, row0=0, row_stride=12, **{"in": [(0, 0)]})
    gat = lambda **kw: dict(dict(op=K.STEP_GATHER, cells=[(0, 0), (5, 14), (LEN - 1, 6)], format=FIELD, out=[arena(0)]), **kw)
    sca = lambda **kw: dict(dict(op=K.STEP_SCATTER, cells=[(0, 0), (5, 14), (LEN - 1, 6)], format=FIELD, **{"in": [arena(0)]}), **kw)
    gen = lambda **kw: dict(dict(op=K.STEP_GENERIC, n=3, row0=0, row_stride=1, param=0, consts=co, **{"in": [arena(0), arena(96)]}), **kw)
    step = lambda op, **kw: dict(dict(op=op, n=1, row0=0, row_stride=40, **{"in": [arena(0), arena(64), arena(128)]}), **kw)
    refused([ok, dict(op=13, n=1)], ["step 1", "unknown op 13"])
    refused([dict(op=-1, n=1)], ["step 0", "unknown op"])
    refused([ok], ["unknown field"], field=2)
    refused([ok, gat(format=5)], ["step 1 (KH_STEP_GATHER)", "format 5"])
    refused([sca(format=-1)], ["step 0 (KH_STEP_SCATTER)", "format -1"])
    refused([ok, ok, gat(cells=[(0, 0), (5, 14), (LEN, 6)])], ["step 2 (KH_STEP_GATHER)", "cell 2", f"row {LEN}"])
    refused([sca(cells=[(0, 0), (5, 15)])], ["step 0 (KH_STEP_SCATTER)", "cell 1", "column 15"])
    refused([ok, gen(rows=[0, 20, LEN])], ["step 1 (KH_STEP_GENERIC)", "instance 2"])
    refused([dict(ok, row0=LEN - 11)], ["step 0 (KH_STEP_POSEIDON)", "do not fit"])
    refused([gat(out=[arena(256 - 64)])], ["step 0", "out[0]", "past the arena"])
    refused([gen(**{"in": [arena(0), arena(192)]})], ["step 0", "in[1]", "past the arena"])
    refused([gat(out=[arena(8)])], ["step 0", "out_dev must be 16-byte aligned"])
    refused([gat(format=U64, out=[arena(4)])], ["step 0", "8-byte aligned"])
    refused([step(K.STEP_ROT64, param=3, **{"in": [(1, 4)]})], ["step 0 (KH_STEP_ROT64)", "words_dev must be 8-byte aligned"])
    refused([gat(out=[None])], ["step 0", "null out_dev"])
    refused([sca(**{"in": [None]})], ["step 0", "null values_dev"])
    refused([step(K.STEP_COMPLETE_ADD, **{"in": [arena(0)]})], ["step 0 (KH_STEP_COMPLETE_ADD)", "null p2_dev"])
    refused([gat(out=[(2, 0)])], ["step 0", "out[0]", "buffer 2 of 2"])
    refused([sca(**{"in": [(-3, 0)]})], ["step 0", "in[0]", "buffer -3"])
    refused([gen(param=2)], ["step 0 (KH_STEP_GENERIC)", "half is 2"])
    refused([gen(consts=None)], ["step 0 (KH_STEP_GENERIC)", "null coeffs"])
    refused([step(K.STEP_VARBASEMUL, param=254)], ["step 0 (KH_STEP_VARBASEMUL)", "num_bits 254"])
    refused([step(K.STEP_ENDOMUL, param=130, consts=co[:4])], ["step 0 (KH_STEP_ENDOMUL)", "num_bits 130"])
    refused([step(K.STEP_ENDOMUL, param=128)], ["step 0 (KH_STEP_ENDOMUL)", "null endo"])
    refused([step(K.STEP_ENDOMUL_SCALAR, param=24)], ["step 0 (KH_STEP_ENDOMUL_SCALAR)", "num_bits 24"])
    refused([step(K.STEP_RANGE_CHECK, param=2)], ["step 0 (KH_STEP_RANGE_CHECK)", "compact is 2"])
    refused([step(K.STEP_XOR, param=255)], ["step 0 (KH_STEP_XOR)", "bits 255"])
    refused([step(K.STEP_ROT64, param=64)], ["step 0 (KH_STEP_ROT64)", "rot 64"])
    refused([step(K.STEP_FF_ADD, sign=0, consts=(1 << 256) - 189)], ["step 0 (KH_STEP_FF_ADD)", "sign is 0"])
    refused([step(K.STEP_FF_MUL)], ["step 0 (KH_STEP_FF_MUL)", "null modulus"])
    refused([step(K.STEP_FF_MUL, consts=np.zeros(6, dtype=np.uint64))], ["step 0 (KH_STEP_FF_MUL)", "modulus is zero"])
    refused([gat(flag_bit=32)], ["step 0 (KH_STEP_GATHER)", "flag_bit 32"])
    refused([step(K.STEP_XOR, param=64, flag_bit=254)], ["step 0 (KH_STEP_XOR)", "flag_bit 254"])
    # at run: only what changes between runs, before anything is launched
    sched = K.WitnessSchedule.create(0, LEN, [gat(**{"in": [(9, 5)]}), sca(cells=[(1, 1), (2, 2), (3, 3)]),      # (a ref the call does not have is ignored)
                                               gat(cells=[(1, 1)], out=[(0, 0)]), gat(cells=[(2, 2)], out=[(1, 0)])],
                                     arena_bytes=96, n_bufs=2)
    wit, b0, b1, flags = sentinel_buf(khip, 15 * LEN), sentinel_buf(khip, 1), sentinel_buf(khip, 1), sentinel_buf(khip, 1)
    vp = C.c_void_p

    def run(bufs=(b0.ptr, b1.ptr), n_bufs=2, w=wit.ptr, col_stride=LEN, f=flags.ptr):
        return lib.kh_witness_schedule_run(sched.handle, (vp * 2)(*bufs), n_bufs, vp(w), col_stride, vp(f))

    for what, call in (("one buffer too few", lambda: run(n_bufs=1)), ("one too many", lambda: run(n_bufs=3)), ("a null bound buffer", lambda: run(bufs=(b0.ptr, None))),
                       ("a misaligned bound buffer", lambda: run(bufs=(b0.ptr + 8, b1.ptr))), ("col_stride < col_len", lambda: run(col_stride=LEN - 1)),
                       ("a misaligned witness", lambda: run(w=wit.ptr + 8)), ("a null witness", lambda: run(w=None)),
                       ("a misaligned flag word", lambda: run(f=flags.ptr + 2)), ("a byte count that overflows", lambda: run(col_stride=1 << 62))):
        assert call() == K.E_INVALID, what
        assert "kh_witness_schedule_run" in lib.kh_last_error().decode(), what
    assert lib.kh_witness_schedule_run(None, None, 0, vp(wit.ptr), LEN, None) == K.E_INVALID
    for buf, elems in ((wit, 15 * LEN), (b0, 1), (b1, 1), (flags, 1)):
        assert np.array_equal(buf.download((elems, 4)), np.tile(SENTINEL, (elems, 1)))
    # ... and what is allowed: a run without a flag word, steps without instances, an empty schedule
    assert run(f=None) == 0
    assert np.array_equal(b0.download((1, 4))[0], SENTINEL) and np.array_equal(wit.download((15, LEN, 4))[1, 1], SENTINEL)       # (1, 1) <- (0, 0) = sentinel
    empty = K.WitnessSchedule.create(1, 0, [dict(op=K.STEP_GATHER, cells=[], format=U64, out=[None]), dict(op=K.STEP_XOR, n=0, param=64)], arena_bytes=0, n_bufs=0)
    assert empty.info() == dict(steps=2, launch_groups=0, resident_bytes=0, run_bytes=0)
    assert lib.kh_witness_schedule_run(empty.handle, None, 0, None, 0, None) == K.E_INVALID      # a run always needs its witness
    assert lib.kh_witness_schedule_run(empty.handle, None, 0, vp(wit.ptr), LEN, None) == 0
    none = K.WitnessSchedule.create(0, LEN, [], arena_bytes=0, n_bufs=0)
    assert none.info()["steps"] == 0
    for s in (sched, empty, none):
        s.free()
    free_all(wit, b0, b1, flags)
