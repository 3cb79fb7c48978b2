"""kh_proofs_from_msgpack / kh_proof_to_msgpack / kh_proof_to_wire / kh_proof_prev_challenges / kh_verifier_index_from_msgpack / _to_msgpack: the
reference's serialised ProverProof and VerifierIndex (rmp-serde) read and written by the library itself (csrc/proof_msgpack.cpp over csrc/proof_wire.hpp).
Every comparison is exact equality:

  1. each of the reference's forty stored proofs, from the file's own inner bytes: the handles hold what tests/test_gpu_verify.py builds through the oracle,
     the digest is the oracle's, kh_verify accepts, and both structures are written back byte for byte;
  2. three proofs in one call: one decode launch, the handles of the single calls, kh_batch_verify accepts;
  3. kh_prove* followed by kh_proof_to_msgpack gives the committed .proof.bin (no Python serialiser in between);
  4. kh_verifier_index_of followed by kh_verifier_index_to_msgpack gives the index bytes inside test_generic_gate.bin;
  5. a two-chunk proof at the smallest size;  6. kh_proof_to_wire;  7. malformed input.

Two cases of part 3 take 10 to 16 seconds, none of it in the library: the committed fixtures library_gates_pallas_2_13 and and_lookup_vesta_2_13 are
defined on circuits that the oracle builds in Python (make_proof_fixtures.library_circuit / and_circuit at 2^13 rows), as in the tests they come from."""
import ctypes as C
import os
import re
import sys

import msgpack
import numpy as np
import pytest

from oracle import fixtures as FX
from oracle import kimchi as K
from oracle import pasta as P
from oracle import prover as OPR
from oracle import views as V

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_proof_fixtures as M  # noqa: E402
import test_gpu_verify as TV  # noqa: E402
from test_gpu_index_create import created, fixture_case  # noqa: E402
from test_gpu_proof_fixtures import first_difference, load  # noqa: E402
from test_gpu_verify import FIXTURES, curve_of, khip, srs16  # noqa: E402,F401  (module-scoped fixtures: the library, one 2^16 SRS per curve)
from test_msgpack_wire import inner_bytes  # noqa: E402
from test_reference_fixtures import HERE as REF, generic_test_circuit  # noqa: E402

pytestmark = pytest.mark.gpu
DECODE, ENCODE = "point_codec_launches", "point_codec_encode_launches"


def cid_of(khip, curve):
    return khip.VESTA if curve is P.VESTA else khip.PALLAS


def assert_sections_equal(got, want, skip=()):
    """two {section: (xy, inf) | limbs} maps hold the same entries; an absent section is an empty one"""
    for name in set(got) | set(want):
        if name in skip:
            continue
        g, w = got.get(name), want.get(name)
        gl, wl = [np.asarray(x) for x in (g if isinstance(g, tuple) else (g,)) if x is not None], [np.asarray(x) for x in (w if isinstance(w, tuple) else (w,)) if x is not None]
        if not (gl and len(gl[0])) and not (wl and len(wl[0])):
            continue
        assert len(gl) == len(wl) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(gl, wl)), name


def assert_prev_equal(got, want):
    assert len(got) == len(want)
    for (gc, (gxy, ginf)), (wc, (wxy, winf)) in zip(got, want):
        assert np.array_equal(gc, np.asarray(wc).reshape(-1, 4)) and np.array_equal(gxy, wxy) and np.array_equal(ginf, winf)


def edited(blob, change):
    """the msgpack bytes with `change` applied to the unpacked structure, packed again in the canonical (shortest) form the files have"""
    obj = msgpack.unpackb(blob, raw=True)
    assert msgpack.packb(obj, use_bin_type=True) == blob
    change(obj)
    return msgpack.packb(obj, use_bin_type=True)


def wire_sections(pb):
    """the records of a serialised proof sliced out in Python, section by section in KH_PROOF_*'s layout"""
    cm, op, ev, ft, _prev = msgpack.unpackb(pb, raw=True)
    cat = lambda comms: b"".join(bytes(x) for c in comms for x in c[0])
    pe = lambda e: b"".join(bytes(x) for part in e for x in part)
    some = lambda es: [e for e in es if e is not None]
    cols = [ev[2]] + list(ev[5:11]) + list(ev[1]) + list(ev[4]) + list(ev[3]) + some(ev[11:17]) + some(ev[19]) + some([ev[17], ev[18], ev[20], ev[21]]) + some(ev[22:26])
    out = {"w_comm": cat(cm[0]), "z_comm": cat([cm[1]]), "t_comm": cat([cm[2]]), "evals": b"".join(pe(e) for e in cols), "public_evals": pe(ev[0]) if ev[0] is not None else b"",
           "ft_eval1": bytes(ft), "lr": b"".join(bytes(x) for lr in op[0] for x in lr), "delta": bytes(op[1]), "z1_z2": bytes(op[2]) + bytes(op[3]), "sg": bytes(op[4])}
    if cm[3] is not None:
        out.update({"lookup_sorted_comm": cat(cm[3][0]), "lookup_aggreg_comm": cat([cm[3][1]]), "lookup_runtime_comm": cat([cm[3][2]]) if cm[3][2] is not None else b""})
    return out


def read_reference(khip, srs16, name):
    """(curve id, proof bytes, index bytes, the oracle's fixture, VerifierIndex, Proof) of a stored reference proof, both handles from the bytes"""
    Cv = curve_of(name)
    cid = cid_of(khip, Cv)
    pb, vb = inner_bytes(name)
    fx = FX.load(os.path.join(REF, name + ".bin"), Cv)
    vix = khip.VerifierIndex.from_msgpack(srs16(cid), vb)
    try:
        return cid, pb, vb, fx, vix, khip.Proof.from_msgpack(cid, pb)
    except Exception:
        vix.free()
        raise


# ---------------------------------------------------------------------------------------------------- 1. the reference's forty files
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_file_is_read_verified_and_written_back(khip, srs16, name):
    assert len(FIXTURES) == 40
    Cv = curve_of(name)
    d0, e0 = khip.counter(DECODE), khip.counter(ENCODE)
    cid, pb, vb, fx, vix, proof = read_reference(khip, srs16, name)
    try:
        assert khip.counter(DECODE) == d0 + 2                               # one launch for the index, one for the proof
        _index_args, ps, pub, prev = TV.fixture_sections(khip, Cv, fx)
        assert_sections_equal(proof.sections(), ps)
        assert_prev_equal(proof.prev_challenges(), prev)
        ovix, _oproof = FX.oracle_views(fx, Cv.srs_h())
        assert Cv.base.from_mont(P.from_limbs(vix.digest())) == K.verifier_index_digest(Cv, ovix)
        ok, _trace = khip.verify(vix, proof, pub, proof.prev_challenges())
        assert ok
        e1 = khip.counter(ENCODE)
        assert proof.to_msgpack(cid) == pb
        assert khip.counter(ENCODE) == e1 + 1                               # the size query launched nothing, the writing call once
        assert vix.to_msgpack(fx["vindex"]["prev_challenges"]) == vb
        assert khip.counter(ENCODE) == e1 + 2 and e1 == e0
        with pytest.raises(khip.KhError, match="prev_challenges"):          # an index that carries its count requires the argument to equal it
            vix.to_msgpack(fx["vindex"]["prev_challenges"] + 1)
    finally:
        proof.free(); vix.free()


# ---------------------------------------------------------------------------------------------------- 2. a batch in one call
def test_three_proofs_in_one_call_take_one_launch(khip, srs16):
    names = ["test_generic_gate", "test_runtime_table", "test_recursion"]    # a plain one, one with (runtime) lookups, the recursive one
    assert all(curve_of(n) is P.VESTA for n in names)
    single = [read_reference(khip, srs16, n) for n in names]
    d0 = khip.counter(DECODE)
    batch = khip.Proof.from_msgpack(khip.VESTA, [s[1] for s in single])
    assert khip.counter(DECODE) == d0 + 1 and len(batch) == 3
    items = []
    for (cid, pb, _vb, fx, vix, alone), got in zip(single, batch):
        assert_sections_equal(got.sections(), alone.sections())
        assert_prev_equal(got.prev_challenges(), alone.prev_challenges())
        assert got.to_msgpack(cid) == pb
        items.append((vix, got, TV.elems(P.VESTA.scalar, fx["public"]), got.prev_challenges()))
    assert len(batch[2].prev_challenges()) == 1 and batch[1].sections()["lookup_runtime_comm"][0].shape[0] == 1
    ok, _traces = khip.batch_verify(items)
    assert ok
    for (_c, _p, _v, _f, vix, alone), got in zip(single, batch):
        got.free(); alone.free(); vix.free()


# ---------------------------------------------------------------------------------------------------- 3. the product's own proof bytes
def and_lookup_case(khip):
    from proof_systems_amd import prover
    from test_gpu_index_create_lookup import created as created_lookup
    rec, want = load("and_lookup_vesta_2_13")
    F = prover.Fld(khip.FP)
    cs, wrows = M.and_circuit(P.VESTA.scalar, rec["log2_n"])
    ix = created_lookup(khip, khip.Srs.create(khip.VESTA, 1 << rec["log2_srs"]), cs, F)
    return rec, want, P.VESTA, ix, np.stack([F.limbs_many([r[c] for r in wrows]) for c in range(15)]), []


def prove_handle(ix, wit, rng, prev=()):
    """create_proof_native's call of kh_prove_full (the same draws from `rng`), keeping the handle"""
    from proof_systems_amd import prover
    F, nx = ix.F, prover.native_index(ix)
    rnd = F.limbs_many(F.rand_many(rng, nx.randomness_count(True)))
    return nx.prove_handle(witness=np.asarray(wit, dtype=np.uint64).reshape(15, -1, 4), randomness=rnd, prev=[(F.limbs_many(list(ch)), cm) for ch, cm in prev])


# a stored index of another shape per case: with lookups for the proofs without, without for the one with
OTHER_SHAPE = {"bench_vesta_2_10": "test_runtime_table", "library_gates_pallas_2_13": "rot_prove_and_verify_pallas", "and_lookup_vesta_2_13": "test_generic_gate",
               "bench_vesta_2_16_prev1": "test_runtime_table"}


@pytest.mark.parametrize("name", ["bench_vesta_2_10", "library_gates_pallas_2_13", "and_lookup_vesta_2_13", "bench_vesta_2_16_prev1"])
def test_prove_then_to_msgpack_gives_the_committed_proof_bytes(khip, srs16, name):
    rec, want, Cv, ix, wit, prev = and_lookup_case(khip) if name.startswith("and_lookup") else fixture_case(khip, name)
    cid = cid_of(khip, Cv)
    proof = prove_handle(ix, wit, V.RefRng(P.StdRng(bytes.fromhex(rec["seed_hex"]))), prev)
    vix = khip.VerifierIndex.of(ix.native)
    bare = khip.Proof(proof.sections())                                     # the same proof through kh_proof_from_sections: no shape, no previous challenges
    try:
        e0 = khip.counter(ENCODE)
        ln = C.c_size_t(0)
        assert khip.raw().kh_proof_to_msgpack(cid, proof._h, None, None, 0, C.byref(ln)) == 0 and ln.value == len(want)
        assert khip.counter(ENCODE) == e0                                   # the size query launches nothing
        small = np.zeros(len(want), dtype=np.uint8)
        assert khip.raw().kh_proof_to_msgpack(cid, proof._h, None, small.ctypes.data_as(khip.U8P), len(want) - 1, C.byref(ln)) == khip.E_INVALID
        assert ln.value == len(want) and not small.any() and khip.counter(ENCODE) == e0
        got = proof.to_msgpack(cid)
        assert khip.counter(ENCODE) == e0 + 1
        assert got == want, "kh_proof_to_msgpack differs from the committed proof: first in " + first_difference(Cv, got, want)
        assert proof.to_msgpack(cid, shape=vix) == want                     # both known, and they agree
        assert len(proof.prev_challenges()) == len(prev)
        with pytest.raises(khip.KhError, match="no shape") as ei:
            bare.to_msgpack(cid)
        assert ei.value.code == khip.E_INVALID
        other = khip.VerifierIndex.from_msgpack(srs16(cid), inner_bytes(OTHER_SHAPE[name])[1])
        with pytest.raises(khip.KhError, match="is not the shape index's") as ei:      # both known, and they disagree
            proof.to_msgpack(cid, shape=other)
        other.free()
        assert ei.value.code == khip.E_INVALID
        if not prev:                                                        # (a handle from sections carries no previous challenges either)
            assert bare.to_msgpack(cid, shape=vix) == want
        else:
            assert bare.to_msgpack(cid, shape=vix) == edited(want, lambda pr: pr.__setitem__(4, []))
    finally:
        bare.free(); proof.free(); vix.free(); ix.free()


# ---------------------------------------------------------------------------------------------------- 4. the product's own index bytes
def test_verifier_index_of_then_to_msgpack_gives_the_reference_index_bytes(khip, srs16):
    from proof_systems_amd import prover
    F = prover.Fld(khip.FP)
    rows, _wit = generic_test_circuit()
    co = np.stack([F.limbs_many(r) for r in rows])
    wires = np.array([[(r, c) for c in range(7)] for r in range(len(rows))], dtype=np.uint32)
    ix = prover.CreatedIndex(srs16(khip.VESTA), ["Generic"] * len(rows), wires, co)
    vix = khip.VerifierIndex.of(ix.native)
    try:
        e0 = khip.counter(ENCODE)
        got = vix.to_msgpack(0)
        assert khip.counter(ENCODE) == e0 + 1
        assert got == inner_bytes("test_generic_gate")[1]
        assert msgpack.unpackb(vix.to_msgpack(3), raw=True)[4] == 3            # an index made from a prover index carries no count: the argument is written
    finally:
        vix.free(); ix.free()


# ---------------------------------------------------------------------------------------------------- 5. two chunks at the smallest size
def test_a_two_chunk_proof_round_trips(khip):
    from proof_systems_amd import prover
    Cv = P.VESTA; F = prover.Fld(khip.FP)
    cs, rows = M.bench_circuit(Cv.scalar, 10, 9)
    srs = khip.Srs.create(khip.VESTA, 1 << 9)
    ix = created(khip, srs, cs, F)
    assert ix.native.shape()[2] == 2
    wit = np.tile(F.limbs(1), (15, rows, 1))
    seed = bytes([5] * 32)
    want = OPR.serialize_proof(Cv, V.device_views(ix, prover.create_proof_native(ix, wit, V.RefRng(P.StdRng(seed))))[2])
    proof = prove_handle(ix, wit, V.RefRng(P.StdRng(seed)))
    vix = khip.VerifierIndex.of(ix.native)
    try:
        got = proof.to_msgpack(khip.VESTA)
        assert got == want, "first difference in " + first_difference(Cv, got, want)
        back = khip.Proof.from_msgpack(khip.VESTA, got)
        assert_sections_equal(back.sections(), proof.sections(), skip=("public_comm", "challenges"))
        assert back.sections()["w_comm"][0].shape[0] == 30 and back.sections()["public_evals"].shape[0] == 4
        ok, _trace = khip.verify(vix, back)
        assert ok
        assert back.to_msgpack(khip.VESTA) == want
        back.free()
    finally:
        proof.free(); vix.free(); ix.free(); srs.close()


# ---------------------------------------------------------------------------------------------------- 6. kh_proof_to_wire
@pytest.mark.parametrize("name", ["test_runtime_table", "rot_prove_and_verify_pallas"])
def test_proof_to_wire_gives_the_records_of_the_file(khip, name):
    cid = cid_of(khip, curve_of(name))
    pb, _vb = inner_bytes(name)
    proof = khip.Proof.from_msgpack(cid, pb)
    e0 = khip.counter(ENCODE)
    wire = proof.to_wire(cid)
    assert khip.counter(ENCODE) == e0 + 1
    want = wire_sections(pb)
    for s in khip.PROOF_SECTIONS:
        assert wire[s] == want.get(s, b""), s
    again = khip.proofs_from_wire(cid, [wire])[0]
    assert_sections_equal(again.sections(), proof.sections())
    again.free(); proof.free()


# ---------------------------------------------------------------------------------------------------- 7. malformed input
def off_curve_record(curve):
    B = curve.base
    x = next(x for x in range(1, 100) if pow((x ** 3 + 5) % B.p, (B.p - 1) // 2, B.p) != 1)
    return x.to_bytes(32, "little") + b"\x00"


def test_malformed_proofs_are_refused(khip, srs16):
    pb, vb = inner_bytes("test_generic_gate")
    INVALID = khip.E_INVALID

    def refused(blob, words, launches):
        d0 = khip.counter(DECODE)
        rc, handles = khip.proofs_from_msgpack_raw(khip.VESTA, [pb, blob], out_before=7)      # a good proof first: nothing of the call is kept
        msg = khip.raw().kh_last_error().decode()
        assert rc == INVALID and handles == [0, 0], (rc, handles, msg)
        assert khip.counter(DECODE) == d0 + launches, msg
        for w in ["kh_proofs_from_msgpack", "proof 1"] + words:
            assert w in msg, (w, msg)

    def set_at(path, value):
        def change(obj):
            for k in path[:-1]:
                obj = obj[k]
            obj[path[-1]] = value
        return change
    for n in (0, 1, 100, len(pb) // 2, len(pb) - 1):                           # five truncation lengths: the text says the bytes end short, at an offset inside them
        refused(pb[:n], ["offset"], 0)
        msg = khip.raw().kh_last_error().decode()
        assert 0 <= int(re.search(r"offset (\d+)", msg).group(1)) <= n and ("found the end of the %d bytes" % n in msg or "than the buffer has" in msg), msg
    refused(pb + b"\xc0", ["offset %d" % len(pb), "expected the end of the buffer, found type byte 0xc0"], 0)
    assert pb[2] == 0x9f
    refused(pb[:2] + b"\x9e" + pb[3:], ["offset 2", "w_comm", "15"], 0)       # w with 14 entries
    z_twice = lambda pr: pr[2][2][0].append(pr[2][2][0][0])
    refused(edited(pb, z_twice), ["evals.z", "2 values at zeta and 1 at zeta omega"], 0)
    refused(edited(pb, set_at([3], pb[-33:-2][:31])), ["a bin of 32 bytes, found one of 31"], 0)
    refused(edited(pb, set_at([3], b"\xff" * 32)), ["section %d" % khip.PROOF_SECTIONS["ft_eval1"], "element 0", "canonical"], 0)
    w00 = msgpack.unpackb(pb, raw=True)[0][0][0][0][0]
    refused(edited(pb, set_at([0, 0, 2, 0, 0], w00[:32] + b"\xc0")), ["section 0", "point 2", "KH_POINT_BAD_FLAGS"], 1)
    refused(edited(pb, set_at([1, 4], off_curve_record(P.VESTA))), ["section %d" % khip.PROOF_SECTIONS["sg"], "point 0", "KH_POINT_NOT_ON_CURVE"], 1)
    # the contrast: another canonical value decodes, and the verifier says no
    z0 = msgpack.unpackb(pb, raw=True)[2][2][0][0]
    changed = edited(pb, set_at([2, 2, 0, 0], bytes([z0[0] ^ 1]) + z0[1:]))
    vix = khip.VerifierIndex.from_msgpack(srs16(khip.VESTA), vb)
    proof = khip.Proof.from_msgpack(khip.VESTA, changed)
    rc, ok, _tr = khip.batch_verify_raw([(vix, proof, None, ())])
    assert rc == 0 and ok == 0
    proof.free(); vix.free()


def test_malformed_indexes_are_refused(khip, srs16):
    vb = inner_bytes("test_generic_gate")[1]
    lb = inner_bytes("test_runtime_table")[1]
    srs = srs16(khip.VESTA)

    def refused(blob, words, launches=0):
        d0 = khip.counter(DECODE)
        b = np.frombuffer(blob, dtype=np.uint8)
        h = C.c_void_p(7)
        rc = khip.raw().kh_verifier_index_from_msgpack(srs._h, b.ctypes.data_as(khip.U8P), b.size, C.byref(h))
        msg = khip.raw().kh_last_error().decode()
        assert rc == khip.E_INVALID and h.value is None, (rc, h.value, msg)
        assert khip.counter(DECODE) == d0 + launches, msg
        for w in ["kh_verifier_index_from_msgpack"] + words:
            assert w in msg, (w, msg)

    def domain_with(k, flip):
        def change(vi):
            d = bytearray(vi[0]); d[k] ^= flip; vi[0] = bytes(d)
        return change
    refused(vb[:700], ["offset"])
    msg = khip.raw().kh_last_error().decode()
    assert "found the end of the 700 bytes" in msg or "than the buffer has" in msg, msg
    refused(vb + b"\x00", ["offset %d" % len(vb), "expected the end of the buffer"])
    refused(edited(vb, lambda vi: vi.__setitem__(1, 32768)), ["max_poly_size 32768", "65536"])
    refused(edited(vb, domain_with(12 + 64, 1)), ["group_gen"])               # a changed group generator
    refused(edited(vb, domain_with(8, 1)), ["is not 2^log_size"])
    refused(edited(lb, lambda vi: vi[20].__setitem__(0, not vi[20][0])), ["joint_lookup_used"])       # the lookup flags against each other
    refused(edited(lb, lambda vi: vi[20][4][2].__setitem__(2, False)), ["runtime_tables_selector is present", "uses_runtime_tables is false"])
    refused(edited(lb, lambda vi: vi[20][4][2][0].__setitem__(0, True)), ["pattern 0 is absent", "feature bit is true"])
    refused(edited(vb, lambda vi: vi[19].__setitem__(0, b"\xff" * 32)), ["shifts", "element 0", "canonical"])
    sigma0 = msgpack.unpackb(vb, raw=True)[5][0][0][0]
    refused(edited(vb, lambda vi: vi[5][3][0].__setitem__(0, sigma0[:32] + b"\xc0")), ["section sigma_comm", "point 3", "KH_POINT_BAD_FLAGS"], launches=1)
    refused(edited(vb, lambda vi: vi[7][0].__setitem__(0, off_curve_record(P.VESTA))), ["section generic_comm", "point 0", "KH_POINT_NOT_ON_CURVE"], launches=1)
