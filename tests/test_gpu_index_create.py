"""kh_prover_index_create: the prover and verifier index built natively from a gate list (ConstraintSystem::create(gates).public(k).build() +
ProverIndex::verifier_index(), no lookup argument), held to bytes the repository already has -- the reference's own stored verifier index
(tests/golden/ref_fixtures/test_generic_gate.bin) and the committed whole-proof fixtures (tests/golden/proof_fixtures/) -- and to the Python
ProverIndex + set_wiring where no fixture exists.  The refusals are host-side checks: nothing here launches a kernel on bad input."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import fixtures as FX
from oracle import kimchi as K
from oracle import pasta as P
from oracle import prover as OPR
from oracle import views as V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import make_proof_fixtures as M  # noqa: E402
from test_gpu_proof_fixtures import bench_index, first_difference, load  # noqa: E402


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def records(khip, cs, F):
    """(gate ids, wires (rows, 7, 2), coefficients (rows, 15, 4)) of an oracle constraint system, up to its last row with gate constraints
    (the rows behind it are the Zero rows build() padded the domain with)"""
    gids = khip.gate_ids()
    gates = cs["gates"]
    rows = max(r for r, g in enumerate(gates) if g["typ"] != "Zero") + 1
    types = [khip.GATE_ZERO if g["typ"] == "Zero" else gids[g["typ"]] for g in gates[:rows]]
    wires = np.array([g["wires"] for g in gates[:rows]], dtype=np.uint32).reshape(rows, 7, 2)
    co = np.stack([F.limbs_many([cs["coefficients"][c][r] for r in range(rows)]) for c in range(15)], axis=1)
    return types, wires, co


def created(khip, srs, cs, F):
    from proof_systems_amd import prover
    types, wires, co = records(khip, cs, F)
    return prover.CreatedIndex(srs, types, wires, co, public=cs["public"])


def serialized(C_, ix, proof):
    return OPR.serialize_proof(C_, V.device_views(ix, proof)[2])


def bench_records(khip, F, gates):
    types = [khip.gate_ids()["Generic"]] * gates
    wires = np.zeros((gates, 7, 2), dtype=np.uint32)
    wires[:, :, 0] = np.arange(gates, dtype=np.uint32)[:, None]; wires[:, :, 1] = np.arange(7, dtype=np.uint32)[None, :]
    co = np.zeros((gates, 15, 4), dtype=np.uint64)
    co[:, 0, :] = F.limbs(1); co[:, 4, :] = F.limbs(F.p - 1)
    return types, wires, co


# ---- 1. the reference's own verifier index
def test_generic_gate_circuit_reproduces_the_reference_verifier_index(khip):
    from proof_systems_amd import prover
    from test_reference_fixtures import generic_test_circuit
    C_ = P.VESTA
    F = prover.Fld(khip.FP)
    v = FX.load(os.path.join(HERE, "golden", "ref_fixtures", "test_generic_gate.bin"), C_)["vindex"]
    rows, _wit = generic_test_circuit()
    co = np.stack([F.limbs_many(r) for r in rows])
    wires = np.array([[(r, c) for c in range(7)] for r in range(len(rows))], dtype=np.uint32)
    ix = prover.CreatedIndex(khip.Srs.create(khip.VESTA, 32), ["Generic"] * len(rows), wires, co)
    assert ix.native.shape() == (5, 3, 1)
    one = lambda t: V.chunks(C_, t)
    assert [one(t) for t in ix.sigma_comm] == v["sigma_comm"]
    assert [one(t) for t in ix.coefficients_comm] == v["coefficients_comm"]
    assert one(ix.generic_comm) == v["generic_comm"]
    h = C_.srs_h()
    for k, key in enumerate(("psm_comm", "complete_add_comm", "mul_comm", "emul_comm", "endomul_scalar_comm")):
        assert one(ix.selector_comms[k]) == v[key] == [h], key
    assert ix.optional_comms == {}
    assert ix.shifts == v["shifts"]
    vix_ref = dict(v); vix_ref["h"] = h
    assert C_.base.from_mont(P.from_limbs(ix.digest)) == K.verifier_index_digest(C_, vix_ref)
    ix.free()


# ---- 2. the committed proof fixtures, byte for byte, from an index built by kh_prover_index_create alone
def fixture_case(khip, name):
    from proof_systems_amd import prover
    rec, want = load(name)
    cid = 0 if rec["curve"] == "vesta" else 1
    C_ = P.CURVES[cid]; Fo = C_.scalar
    F = prover.Fld(khip.FP if cid == 0 else khip.FQ)
    prev, wit = [], None
    if name.startswith("generic_public"):
        cs, w = M.generic_circuit(Fo, rec["log2_n"], rec["log2_srs"])
        wit = np.stack([F.limbs_many(col) for col in w])
    elif name.startswith("library_gates"):
        cs, w = M.library_circuit(Fo, rec["log2_n"])
        wit = np.stack([F.limbs_many(col) for col in w])
    else:
        cs, rows = M.bench_circuit(Fo, rec["log2_n"], rec["log2_srs"])
        wit = np.tile(F.limbs(1), (15, rows, 1))
    srs = khip.Srs.create(cid, 1 << rec["log2_srs"])
    ix = created(khip, srs, cs, F)
    if rec.get("prev_challenges"):
        std = P.StdRng(M.PREV_SEED)
        chals = [P.field_rand(Fo, std) for _ in range(rec["log2_srs"])]
        bc = khip.b_poly_coefficients(ix.fid, F.limbs_many(chals), len(chals))[0]
        prev = [(chals, srs.commit_non_hiding(bc, 1))]
    return rec, want, C_, ix, wit, prev


@pytest.mark.parametrize("name", ["bench_vesta_2_10", "bench_vesta_2_16", "bench_pallas_2_16", "bench_vesta_2_17_over_2_16", "bench_vesta_2_16_prev1",
                                  "generic_public_vesta_2_16", "library_gates_vesta_2_13"])
def test_created_index_reproduces_the_committed_proof_bytes(khip, name):
    from proof_systems_amd import prover
    rec, want, C_, ix, wit, prev = fixture_case(khip, name)
    assert ix.native.shape() == (rec["log2_n"], rec["zk_rows"], rec["num_chunks"])
    assert hex(C_.base.from_mont(P.from_limbs(ix.digest))) == rec["verifier_index_digest_hex"]
    seed = bytes.fromhex(rec["seed_hex"])
    proof = prover.create_proof_native(ix, wit, V.RefRng(P.StdRng(seed)), prev_challenges=prev)
    got = serialized(C_, ix, proof)
    assert got == want, "the created index's proof differs from the committed one: first in " + first_difference(C_, got, want)
    ix.free()


# ---- 3. parity with the Python index: ForeignFieldAdd rows, copy constraints, public inputs at 2^12
def ffadd_circuit(F, rows=4000, npub=2):
    """Generic rows (public inputs first), ForeignFieldAdd rows with the foreign modulus' three 88-bit limbs and the sign as their coefficients
    (oracle/gates.py::foreign_field_add_row), Zero rows after each of them, and copy constraints between generic cells"""
    m = 0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f        # secp256k1's base field
    L = (1 << 88) - 1
    fm = [m & L, (m >> 88) & L, m >> 176]
    p = F.p
    types, coeffs = [], []
    for r in range(rows):
        if r < npub:
            types.append("Generic"); coeffs.append([1] + [0] * 14)
        elif r % 5 == 1:
            types.append("ForeignFieldAdd"); coeffs.append(fm + [1 if r % 2 else p - 1] + [0] * 11)
        elif r % 5 == 2:
            types.append("Zero"); coeffs.append([0] * 15)
        else:
            types.append("Generic"); coeffs.append([1, 1, p - 1, 0, 0, 3, 0, 0, 0, 7, 0, 0, 0, 0, 0])
    wires = [[(r, c) for c in range(7)] for r in range(rows)]
    for r in range(npub, rows - 8, 5):                   # a cycle over (r, 0) -> (r + 3, 2) -> (r + 4, 1) -> (r, 0)
        a, b, c = (r, 0), (r + 3, 2), (r + 4, 1)
        wires[a[0]][a[1]], wires[b[0]][b[1]], wires[c[0]][c[1]] = b, c, a
    return types, wires, np.stack([F.limbs_many(row) for row in coeffs])


def test_created_index_equals_the_python_index_with_foreign_field_add(khip):
    from proof_systems_amd import prover
    F = prover.Fld(khip.FP)
    types, wires, co = ffadd_circuit(F)
    srs = khip.Srs.create(khip.VESTA, 1 << 12)
    ix = prover.CreatedIndex(srs, types, wires, co, public=2)
    assert ix.native.shape() == (12, 3, 1) and ix.optional == ["ForeignFieldAdd"]
    pix = prover.ProverIndex(khip.VESTA, 12, co, srs=srs, gate_types=types, public=2)
    pix.set_wiring(wires)
    same = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(np.asarray(a[1], np.uint8), np.asarray(b[1], np.uint8))
    for key in ("sigma_comm", "coefficients_comm", "selector_comms"):
        assert all(same(a, b) for a, b in zip(getattr(ix, key), getattr(pix, key))), key
    assert same(ix.generic_comm, pix.generic_comm) and same(ix.optional_comms["ForeignFieldAdd"], pix.optional_comms["ForeignFieldAdd"])
    assert ix.shifts == pix.shifts and np.array_equal(np.asarray(ix.digest).reshape(-1), np.asarray(pix.digest).reshape(-1))
    # the proof (the witness does not satisfy the circuit: check=False) from the same stream
    wit = np.tile(F.limbs(5), (15, 4000, 1))
    seed = bytes([12, 9] + [42] * 30)
    p1 = prover.create_proof_native(ix, wit, V.RefRng(P.StdRng(seed)), check=False)
    p2 = prover.create_proof_native(pix, wit, V.RefRng(P.StdRng(seed)), check=False)
    assert serialized(P.VESTA, ix, p1) == serialized(P.VESTA, pix, p2)
    ix.free(); pix.free()


# ---- 4. refusals: KH_E_INVALID, a message, no handle; host-side, before any device work
def raw_create(khip, srs, types, wires, co, public=0):
    lib = khip.raw()
    t = np.ascontiguousarray(types, dtype=np.int32); w = np.ascontiguousarray(wires, dtype=np.uint32); c = np.ascontiguousarray(co, dtype=np.uint64)
    h = C.c_void_p()
    rc = lib.kh_prover_index_create(srs._h, C.c_size_t(len(t)), t.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    c.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_uint(public), C.byref(h))
    return rc, h.value, lib.kh_last_error().decode()


def test_invalid_gate_lists_are_refused_before_any_device_work(khip):
    from proof_systems_amd import prover
    F = prover.Fld(khip.FP)
    srs = khip.Srs.create(khip.VESTA, 32)
    gids = khip.gate_ids()
    types, wires, co = bench_records(khip, F, 20)               # n = 32, zk_rows = 3
    KH_E_INVALID = -1

    def refused(t=types, w=wires, c=co, public=0, what=""):
        rc, h, msg = raw_create(khip, srs, t, w, c, public)
        assert rc == KH_E_INVALID and h is None and msg, (what, rc, msg)
        return msg
    for name in ("Xor16", "RangeCheck0", "RangeCheck1", "Rot64", "ForeignFieldMul"):
        t = list(types); t[7] = gids[name]
        assert "lookup" in refused(t=t, what=name)
    t = list(types); t[3] = gids["Permutation"]
    refused(t=t, what="Permutation")
    for bad in (99, -2):
        t = list(types); t[3] = bad
        refused(t=t, what=bad)
    w = wires.copy(); w[5, 2, 0] = 32
    refused(w=w, what="row = n")
    w = wires.copy(); w[5, 2, 1] = 7
    refused(w=w, what="col = 7")
    c = co.copy(); c[4, 9] = np.frombuffer(F.p.to_bytes(32, "little"), dtype=np.uint64)
    refused(c=c, what="coefficient = p")
    refused(t=types[:1], w=wires[:1], c=co[:1], what="one gate")
    refused(public=29, what="public inputs")
    # attach_lookup on a created index
    ix = khip.NativeProverIndex.create(srs, types, wires, co)
    bufs = [khip.DevBuf(32 * 32) for _ in range(3)]
    with pytest.raises(khip.KhError, match="kh_prover_index_create"):
        ix.attach_lookup(["Xor"], bufs[:1], bufs[:1], bufs[:1], bufs[:1], None, bufs)
    ix.free()
    for b in bufs:
        b.free()
    # a valid create still works and reproduces the reference shape
    rc, h, _ = raw_create(khip, srs, types, wires, co, 3)
    assert rc == 0 and h
    khip.raw().kh_prover_index_free(C.c_void_p(h))


# ---- 5. lifetime: the index keeps nothing of the caller's arrays; several indices on one SRS
def test_created_index_owns_its_data_and_several_share_an_srs(khip):
    from proof_systems_amd import prover
    rec, want = load("bench_vesta_2_10")
    F = prover.Fld(khip.FP)
    srs = khip.Srs.create(khip.VESTA, 1 << 10)
    seed = bytes.fromhex(rec["seed_hex"])
    wit = np.tile(F.limbs(1), (15, rec["gates"], 1))
    types, wires, co = bench_records(khip, F, rec["gates"])
    a = prover.CreatedIndex(srs, types, wires, co)
    wires[:] = 3; co[:] = 0xfffffffffffffff; types[:] = [0] * len(types)
    del wires, co
    b = prover.CreatedIndex(srs, *bench_records(khip, F, rec["gates"]))
    c = prover.CreatedIndex(srs, *bench_records(khip, F, rec["gates"]))
    for ix in (a, b, c):
        assert serialized(P.VESTA, ix, prover.create_proof_native(ix, wit, V.RefRng(P.StdRng(seed)))) == want
    b.free()                                             # freed in creation order and against it
    assert serialized(P.VESTA, c, prover.create_proof_native(c, wit, V.RefRng(P.StdRng(seed)))) == want
    a.free()
    assert serialized(P.VESTA, c, prover.create_proof_native(c, wit, V.RefRng(P.StdRng(seed)))) == want
    c.free()


# ---- 6. a C caller with only the header
def test_a_c_program_creates_the_index_from_a_gate_list(khip, tmp_path):
    from proof_systems_amd import prover
    rec, _want = load("bench_vesta_2_10")
    src = os.path.join(HERE, "cpp", "test_index_create.cpp")
    exe = str(tmp_path / "test_index_create")
    libdir = os.path.join(ROOT, "proof_systems_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lkimchi_hip", "-Wl,-rpath," + libdir,
                           "-Wl,--allow-shlib-undefined", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    pix, F = bench_index(khip, rec)                      # the Python-built index of the same circuit
    nx = prover.native_index(pix)
    count = nx.randomness_count(True)
    rnd = F.limbs_many(F.rand_many(V.RefRng(P.StdRng(bytes.fromhex(rec["seed_hex"]))), count))
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.array([count], dtype=np.uint64), rnd.reshape(-1)]).tofile(inp)
    r = subprocess.run([exe, str(rec["log2_n"]), inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "INDEX_CREATE_OK" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    digest = raw[:32].view(np.uint64)
    assert hex(P.VESTA.base.from_mont(P.from_limbs(digest))) == rec["verifier_index_digest_hex"]
    want, _ph = nx.prove(witness=np.tile(F.limbs(1), (15, rec["gates"], 1)), randomness=rnd)
    pos = 32
    for name, sid in khip.PROOF_SECTIONS.items():
        if sid > 11:
            break
        cnt, pts = (int(x) for x in raw[pos:pos + 16].view(np.uint64)); pos += 16
        w = 8 if pts else 4
        limbs = raw[pos:pos + 8 * w * cnt].view(np.uint64).reshape(cnt, w); pos += 8 * w * cnt
        if pts:
            flags = raw[pos:pos + cnt]; pos += cnt
            assert np.array_equal(limbs, want[name][0]) and np.array_equal(flags, want[name][1]), name
        else:
            assert np.array_equal(limbs, want[name]), name
    pix.free()
