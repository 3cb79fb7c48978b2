"""kh_prover_index_create_lookup: the prover and verifier index of a circuit WITH a lookup argument built natively from its gate list, its
lookup tables and its runtime-table configurations -- held to the reference's own whole-proof vector (and.rs, 6160 bytes), the committed
and_lookup fixture, the oracle's index (oracle/circuit.py::build + oracle/prover.py::Index) section for section, and the Python
ProverIndex + LookupIndex + attach_lookup path column for column.  Every comparison is exact equality."""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import types as pytypes

import numpy as np
import pytest

from oracle import circuit as CC
from oracle import gates as G
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
from test_gpu_proof_fixtures import first_difference, load  # noqa: E402
from test_gpu_prover_parity import runtime_table_circuit  # noqa: E402

KH_E_INVALID = -1


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def fld(khip):
    from proof_systems_amd import prover
    return prover.Fld(khip.FP)


def records(khip, cs, F):
    """(gate types, wires (rows, 7, 2), coefficients (rows, 15, 4)) of an oracle constraint system up to its last row that is not a Zero row"""
    gates = cs["gates"]
    rows = max(r for r, g in enumerate(gates) if g["typ"] != "Zero") + 1
    types = [g["typ"] for g in gates[:rows]]
    wires = np.array([g["wires"] for g in gates[:rows]], dtype=np.uint32).reshape(rows, 7, 2)
    co = np.stack([F.limbs_many([cs["coefficients"][c][r] for r in range(rows)]) for c in range(15)], axis=1)
    return types, wires, co


def created(khip, srs, cs, F, tables=None, runtime=None):
    from proof_systems_amd import prover
    types, wires, co = records(khip, cs, F)
    return prover.CreatedIndex(srs, types, wires, co, public=cs["public"], tables=tables, runtime_tables=runtime)


def python_index(khip, cs, srs, F, tables=(), runtime=None):
    """the Python path the native call replaces: ProverIndex + set_wiring + LookupIndex + attach_lookup"""
    from proof_systems_amd import prover, lookup as LK
    types, wires, co = records(khip, cs, F)
    ix = prover.ProverIndex(khip.VESTA, cs["log2_n"], co, srs=srs, gate_types=types, public=cs["public"], zk_rows=cs["zk_rows"])
    ix.set_wiring(wires.tolist())
    ix.attach_lookup(LK.LookupIndex(ix.fid, cs["gate_types"], list(tables), cs["log2_n"], cs["zk_rows"], runtime_tables=runtime))
    return ix


def serialized(C_, ix, proof):
    return OPR.serialize_proof(C_, V.device_views(ix, proof)[2])


def vindex_of(ix):
    """the verifier index of a created index in the oracle's representation, lookup index included (no proof involved)"""
    c, vix, _ = V.device_views(ix, None)
    LI = getattr(ix, "lookup", None)
    ch = lambda t: V.chunks(c, t)
    vix["lookup_index"] = None if LI is None else {
        "joint_lookup_used": LI.joint_lookup_used, "lookup_table": [ch(t) for t in LI.table_comm],
        "lookup_selectors": {q: (ch(LI.selector_comm[q]) if q in LI.patterns else None) for q in K.LOOKUP_PATTERN_ORDER},
        "table_ids": ch(LI.table_ids_comm) if LI.table_ids_comm else None, "max_per_row": LI.max_per_row, "max_joint_size": LI.max_joint_size,
        "patterns": list(LI.patterns), "uses_runtime_tables": LI.runtime_selector is not None,
        "runtime_tables_selector": ch(LI.runtime_selector_comm) if LI.runtime_selector_comm else None}
    return c, vix


def assert_vindex_equals_the_oracle(ix, oix):
    c, vix = vindex_of(ix)
    want = oix.vindex
    for key in ("sigma_comm", "coefficients_comm", "generic_comm", "psm_comm", "complete_add_comm", "mul_comm", "emul_comm", "endomul_scalar_comm", "optional_comms",
                "shifts", "zk_rows", "log2_n", "max_poly_size"):
        assert vix[key] == want[key], key
    lo, lw = vix["lookup_index"], want["lookup_index"]
    assert (lo is None) == (lw is None)
    for key in lw or ():
        assert lo[key] == lw[key], "lookup_index." + key
    assert c.base.from_mont(P.from_limbs(ix.digest)) == oix.digest, "digest"


def assert_columns_equal_the_python_index(ix, pix):
    """every lookup column of the created index, element for element: selectors (d1, coefficient form, d8), table columns, table ids, runtime
    selector (three forms), the three atoms on d8"""
    LI, nx = pix.lookup, ix.native
    n = pix.n
    for k, q in enumerate(LI.patterns):
        assert np.array_equal(nx.lookup_column("selector_d1", k), LI.d_selectors[q].download((n, 4))), ("selector", q)
        assert np.array_equal(nx.lookup_column("selector_c", k), LI.sel_c[q].download((n, 4))), ("selector coefficients", q)
        assert np.array_equal(nx.lookup_column("selector_d8", k), LI.sel8[q].download((8 * n, 4))), ("selector d8", q)
    assert nx.lookup_column("selector_d1", len(LI.patterns)) is None
    for k, b in enumerate(LI.d_table_cols):
        assert np.array_equal(nx.lookup_column("table_d1", k), b.download((n, 4))), ("table column", k)
    assert nx.lookup_column("table_d1", len(LI.d_table_cols)) is None
    ids = nx.lookup_column("table_ids_d1")
    assert (ids is None) == (LI.d_table_ids is None) and (ids is None or np.array_equal(ids, LI.d_table_ids.download((n, 4)))), "table ids"
    for k, b in enumerate((LI.d_runtime_selector, LI.rtsel_c, LI.rtsel8)):
        got = nx.lookup_column("runtime_selector", k)
        assert (got is None) == (b is None) and (got is None or np.array_equal(got, b.download((n if k < 2 else 8 * n, 4)))), ("runtime selector", k)
    for k, b in enumerate(LI.atoms8):
        assert np.array_equal(nx.lookup_column("atom_d8", k), b.download((8 * n, 4))), ("atom", k)


def and_inputs(F, std):
    gates = []
    CC.extend_and(F.p, gates, 8)
    in1 = CC.gen_field_with_bits(std, 64); in2 = CC.gen_field_with_bits(std, 64)
    return gates, G.and_witness(F, in1, in2, 8)


# ---- 1. the reference's whole-proof vector from an index no Python built
def test_created_lookup_index_reproduces_the_reference_whole_proof_bytes(khip):
    from proof_systems_amd import prover
    with open(os.path.join(HERE, "golden", "and_serialization_regression.json")) as f:
        kat = json.load(f)
    seed, want = bytes(kat["seed"]), bytes.fromhex(kat["proof_hex"])
    C_ = P.VESTA; Fo = C_.scalar; F = fld(khip)
    std = P.StdRng(seed)
    gates, rows = and_inputs(Fo, std)
    types = [g["typ"] for g in gates]
    wires = np.array([g["wires"] for g in gates], dtype=np.uint32)
    co = np.stack([F.limbs_many(list(g["coeffs"]) + [0] * (15 - len(g["coeffs"]))) for g in gates])
    ix = prover.CreatedIndex(khip.Srs.create(khip.VESTA, 1 << 16), types, wires, co)
    assert ix.lookup.patterns == ["Xor"] and ix.lookup.max_per_row == 4 and ix.lookup.max_joint_size == 3 and ix.lookup.table_ids_comm is None
    wit = np.stack([F.limbs_many([r[c] for r in rows]) for c in range(15)])
    got = serialized(C_, ix, prover.create_proof_native(ix, wit, V.RefRng(std)))
    assert len(want) == 6160
    assert got == want, "the created lookup index's proof differs from the reference's bytes: first in " + first_difference(C_, got, want)
    ix.free()


# ---- 2. the committed lookup fixture
def test_created_lookup_index_reproduces_the_committed_and_lookup_fixture(khip):
    from proof_systems_amd import prover
    rec, want = load("and_lookup_vesta_2_13")
    C_ = P.VESTA; F = fld(khip)
    cs, wrows = M.and_circuit(C_.scalar, rec["log2_n"])
    ix = created(khip, khip.Srs.create(khip.VESTA, 1 << rec["log2_srs"]), cs, F)
    assert ix.native.shape() == (rec["log2_n"], rec["zk_rows"], rec["num_chunks"])
    assert hex(C_.base.from_mont(P.from_limbs(ix.digest))) == rec["verifier_index_digest_hex"]
    wit = np.stack([F.limbs_many([r[c] for r in wrows]) for c in range(15)])
    got = serialized(C_, ix, prover.create_proof_native(ix, wit, V.RefRng(P.StdRng(bytes.fromhex(rec["seed_hex"])))))
    assert got == want, "the created lookup index's proof differs from the committed one: first in " + first_difference(C_, got, want)
    ix.free()


# ---- 3. + 4. parity with the oracle index and the Python index on every feature
def fixed_table_circuit(Fo, rows=300):
    """(a) Lookup gates into two fixed tables with ids 5 (two columns) and 9 (one column): no table 0, so the dummy entry is a padding row, and a table-id column"""
    rnd = random.Random(31)
    t5 = {"id": 5, "data": [[7 * j + 1 for j in range(40)], [j * j + 3 for j in range(40)]]}
    t9 = {"id": 9, "data": [[11 * j + 2 for j in range(25)]]}
    gates = [CC.gate("Lookup", r) for r in range(rows)]
    wit = [[0] * rows for _ in range(15)]
    for r in range(rows):
        t = t5 if rnd.random() < 0.6 else t9
        wit[0][r] = t["id"]
        for k in range(3):
            j = rnd.randrange(len(t["data"][0]))
            wit[1 + 2 * k][r] = t["data"][0][j]
            wit[2 + 2 * k][r] = t["data"][1][j] if len(t["data"]) > 1 else 0
    return CC.build(Fo, gates, lookup_tables=[t5, t9]), [t5, t9], wit


def mixed_circuit(Fo):
    """(c) RangeCheck0, RangeCheck1, Rot64, ForeignFieldMul, Xor16 and Generic rows: both gate tables, three patterns, a domain set by the lookup
    domain size (4096 + 256 + 1) and not by the 40 gates.  The witness holds valid lookups (values of the tables in the looked-up cells) but
    does not satisfy the gates."""
    rnd = random.Random(8)
    p = Fo.p
    order = ["Generic", "RangeCheck0", "RangeCheck1", "Zero", "Rot64", "RangeCheck0", "ForeignFieldMul", "Zero", "Xor16", "Generic"] * 4
    gates = []
    for r, t in enumerate(order):
        co = CC.generic_spec(p, "Add") + CC.generic_spec(p, "Mul") if t == "Generic" else [rnd.randrange(1, 1 << 60) for _ in range(4)] if t not in ("Zero", "Xor16") else []
        gates.append(CC.gate(t, r, co))
    CC.connect_cell_pair(gates, (0, 0), (9, 1)); CC.connect_cell_pair(gates, (10, 2), (29, 0))
    cs = CC.build(Fo, gates)
    pats = cs["lookup"].info.pattern_by_row(cs["gate_types"])
    wit = [[rnd.randrange(1, 1 << 20) for _ in order] for _ in range(15)]
    for r in range(len(order)):
        if pats[r] in ("RangeCheck", "ForeignFieldMul"):
            for c in (range(3, 7) if pats[r] == "RangeCheck" else range(7, 11)):
                wit[c][r] = rnd.randrange(1 << 12)
        elif pats[r] == "Xor":
            for k in range(4):
                a, b = rnd.randrange(16), rnd.randrange(16)
                wit[3 + k][r], wit[7 + k][r], wit[11 + k][r] = a, b, a ^ b
    return cs, wit


def combined_circuit(Fo, rows=120):
    """(e) every kind of table in one index: the caller's fixed tables (ids 5 and 9), both gate tables (a RangeCheck0 and a Xor16 row), then two runtime
    tables (ids 12 and 13) behind them -- the documented order fixed, range check, XOR, runtime, a runtime offset that is not zero, and the caller's
    data next to generated segments.  Every lookup is in its table; the RangeCheck0 and Xor16 rows hold zeros, which satisfy both gates."""
    rnd = random.Random(47)
    _cs, tabs, _w = fixed_table_circuit(Fo, rows=2)
    cfg = [{"id": 12, "first_column": [21, 22, 23, 24]}, {"id": 13, "first_column": [31, 32, 33]}]
    rts = [(12, [41, 42, 43, 44]), (13, [51, 52, 53])]
    gates = [CC.gate("Lookup", r) for r in range(rows)] + [CC.gate("RangeCheck0", rows, [0]), CC.gate("Xor16", rows + 1), CC.gate("Zero", rows + 2)]
    wit = [[0] * (rows + 3) for _ in range(15)]
    for r in range(rows):
        kind = rnd.randrange(3)
        if kind < 2:
            t = tabs[kind]
            first, second = t["data"][0], (t["data"][1] if len(t["data"]) > 1 else [0] * len(t["data"][0]))
            wit[0][r] = t["id"]
        else:
            k = rnd.randrange(2)
            first, second = cfg[k]["first_column"], rts[k][1]
            wit[0][r] = cfg[k]["id"]
        for k in range(3):
            j = rnd.randrange(len(first))
            wit[1 + 2 * k][r], wit[2 + 2 * k][r] = first[j], second[j]
    return CC.build(Fo, gates, lookup_tables=tabs, runtime_tables=cfg), tabs, cfg, rts, wit


def many_tables_circuit(Fo, rows=60, ntab=40):
    """(f) more fixed tables than prefix offsets fit the table kernel's arguments: 40 one-column tables of three entries, ids 1..40"""
    rnd = random.Random(3)
    tabs = [{"id": t + 1, "data": [[100 * t + 7, 100 * t + 8, 100 * t + 9]]} for t in range(ntab)]
    wit = [[0] * rows for _ in range(15)]
    for r in range(rows):
        t = rnd.randrange(ntab)
        wit[0][r] = t + 1
        for k in range(3):
            wit[1 + 2 * k][r] = tabs[t]["data"][0][rnd.randrange(3)]
    return CC.build(Fo, [CC.gate("Lookup", r) for r in range(rows)], lookup_tables=tabs), tabs, wit


def parity_case(name, Fo):
    """(cs, fixed tables, runtime cfg, runtime values, witness, log2 of the SRS, satisfied)"""
    if name == "fixed_tables":
        cs, tabs, wit = fixed_table_circuit(Fo)
        return cs, tabs, None, (), wit, cs["log2_n"], True
    if name.startswith("runtime"):
        chunks = int(name[-1])
        cs, cfg, rts, wit = runtime_table_circuit(Fo)
        if chunks > 1:
            cs = CC.build(Fo, [CC.gate("Lookup", r) for r in range(20)], runtime_tables=cfg, max_poly_size=(1 << cs["log2_n"]) // chunks)
        return cs, [], cfg, rts, wit, cs["log2_n"] - (chunks - 1), True
    if name == "combined":
        cs, tabs, cfg, rts, wit = combined_circuit(Fo)
        return cs, tabs, cfg, rts, wit, cs["log2_n"], True
    if name == "many_tables":
        cs, tabs, wit = many_tables_circuit(Fo)
        return cs, tabs, None, (), wit, cs["log2_n"], True
    if name == "mixed":
        cs, wit = mixed_circuit(Fo)
        return cs, [], None, (), wit, cs["log2_n"], False
    log_srs = int(name.split("_")[-1])                      # (d) the chunked AND circuit
    gates, rows = and_inputs(Fo, P.StdRng(bytes([61] * 32)))
    cs = CC.build(Fo, gates, max_poly_size=1 << log_srs)
    return cs, [], None, (), [[r[c] for r in rows] for c in range(15)], log_srs, True


@pytest.mark.parametrize("name", ["fixed_tables", "runtime_chunks_1", "runtime_chunks_2", "mixed", "and_chunked_8", "and_chunked_7", "combined", "many_tables"])
def test_created_lookup_index_equals_the_oracle_index_and_the_python_columns(khip, name):
    from proof_systems_amd import prover
    C_ = P.VESTA; Fo = C_.scalar; F = fld(khip)
    cs, tabs, cfg, rts, wit, log_srs, satisfied = parity_case(name, Fo)
    size = 1 << log_srs
    srs = khip.Srs.create(khip.VESTA, size)
    ix = created(khip, srs, cs, F, tables=tabs, runtime=cfg)
    nch = max(1, (1 << cs["log2_n"]) // size)
    assert ix.native.shape() == (cs["log2_n"], cs["zk_rows"], nch)
    assert ix.optional == cs["optional"] and ix.lookup.patterns == cs["lookup"].info.patterns
    if name == "mixed":
        assert cs["log2_n"] == 13 and ix.lookup.patterns == ["Xor", "RangeCheck", "ForeignFieldMul"] and len(ix.optional) == 5
    if name == "fixed_tables":
        assert ix.lookup.table_ids_comm is not None and ix.lookup.patterns == ["Lookup"]
    if name == "combined":                                  # 40 + 25 fixed entries, 4096 + 256 of the gate tables, then the runtime rows
        assert ix.lookup.patterns == ["Xor", "Lookup", "RangeCheck"] and (ix.lookup.runtime_offset, ix.lookup.runtime_len) == (40 + 25 + 4096 + 256, 7)
    osrs = OPR.Srs(C_, size)
    oix = OPR.Index(C_, cs, osrs)
    assert_vindex_equals_the_oracle(ix, oix)
    pix = python_index(khip, cs, srs, F, tabs, cfg)
    assert np.array_equal(np.asarray(ix.digest).reshape(-1), np.asarray(pix.digest).reshape(-1))
    assert_columns_equal_the_python_index(ix, pix)
    if cfg is not None:
        assert (ix.lookup.runtime_offset, ix.lookup.runtime_len) == (pix.lookup.runtime_offset, sum(l_ for _i, l_ in pix.lookup.runtime_tables))
    w = np.stack([F.limbs_many(col) for col in wit])
    seed = bytes([71, log_srs] + [9] * 30)
    got = serialized(C_, ix, prover.create_proof_native(ix, w, V.RefRng(P.StdRng(seed)), runtime_tables=rts, check=satisfied))
    if satisfied:
        oproof = OPR.create_proof(oix, wit, P.StdRng(seed), runtime_tables=rts) if rts else OPR.create_proof(oix, wit, P.StdRng(seed))
        assert got == OPR.serialize_proof(C_, oproof), "first difference in " + first_difference(C_, got, OPR.serialize_proof(C_, oproof))
    else:                                                   # the witness does not satisfy the gates: the Python index's proof from the same stream
        assert got == serialized(C_, pix, prover.create_proof_native(pix, w, V.RefRng(P.StdRng(seed)), check=False))
    with pytest.raises(khip.KhError, match="kh_prover_index_create_lookup"):
        bufs = [khip.DevBuf(32) for _ in range(3)]
        ix.native.attach_lookup(["Xor"], bufs[:1], bufs[:1], bufs[:1], bufs[:1], None, bufs)
    ix.free(); pix.free_lookup(); pix.free()


@pytest.mark.parametrize("log_srs,zk", [(7, 3), (6, 5)])
def test_atom_kernel_equals_the_host_restatement(khip, log_srs, zk):
    """the three row-set atoms of a 2^7 domain (zk_rows 3: one chunk; 5: two chunks) against lookup.atom_columns, Python integers on the host"""
    from proof_systems_amd import prover, lookup as LK
    F = fld(khip)
    cs, tabs, _wit = fixed_table_circuit(P.VESTA.scalar, rows=40)
    cs = CC.build(P.VESTA.scalar, [CC.gate("Lookup", r) for r in range(40)], lookup_tables=tabs, max_poly_size=1 << log_srs)
    assert cs["log2_n"] == 7 and cs["zk_rows"] == zk
    ix = created(khip, khip.Srs.create(khip.VESTA, 1 << log_srs), cs, F, tables=tabs)
    assert ix.native.shape() == (7, zk, 128 >> log_srs)
    host = LK.atom_columns(pytypes.SimpleNamespace(F=F, n=128, logn=7, zk_rows=zk), 3)
    for k, b in enumerate(host):
        assert np.array_equal(ix.native.lookup_column("atom_d8", k), b.download((8 * 128, 4))), ("atom", k)
        b.free()
    ix.free()


# ---- 5. refusals: KH_E_INVALID, a message, no handle (the checks are host code ahead of the first device call; the library has no launch counter to assert on)
def raw_create_lookup(khip, srs, types, wires, co, tables=(), runtime=(), public=0):
    lib = khip.raw()
    t = np.ascontiguousarray(types, dtype=np.int32); w = np.ascontiguousarray(wires, dtype=np.uint32); c = np.ascontiguousarray(co, dtype=np.uint64)
    keep = [np.ascontiguousarray(d, dtype=np.uint64) for _i, d in tables] + [np.ascontiguousarray(d, dtype=np.uint64) for _i, d in runtime]
    u64p = C.POINTER(C.c_uint64)
    tc = (khip.LookupTableC * max(len(tables), 1))(*[khip.LookupTableC(i, d.shape[0], d.shape[1], d.ctypes.data_as(u64p)) for (i, _), d in zip(tables, keep)])
    rc_ = (khip.RuntimeTableCfgC * max(len(runtime), 1))(*[khip.RuntimeTableCfgC(i, d.shape[0], d.ctypes.data_as(u64p)) for (i, _), d in zip(runtime, keep[len(tables):])])
    h = C.c_void_p()
    rc = lib.kh_prover_index_create_lookup(srs._h, C.c_size_t(len(t)), t.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           c.ctypes.data_as(u64p), C.c_uint(public), tc, C.c_size_t(len(tables)), rc_, C.c_size_t(len(runtime)), C.byref(h))
    return rc, h.value, lib.kh_last_error().decode()


def lookup_records(khip, F, rows):
    types = [khip.GATE_LOOKUP] * rows
    wires = np.zeros((rows, 7, 2), dtype=np.uint32)
    wires[:, :, 0] = np.arange(rows, dtype=np.uint32)[:, None]; wires[:, :, 1] = np.arange(7, dtype=np.uint32)[None, :]
    return types, wires, np.zeros((rows, 15, 4), dtype=np.uint64)


def test_invalid_lookup_inputs_are_refused_with_a_message_and_no_handle(khip):
    from test_gpu_index_create import raw_create
    F = fld(khip)
    srs = khip.Srs.create(khip.VESTA, 64)
    gids = khip.gate_ids()
    types, wires, co = lookup_records(khip, F, 20)              # n = 32 without tables, zk_rows = 3
    tab = lambda cols: np.stack([F.limbs_many(c) for c in cols])
    good = (4, tab([[1, 2, 3], [4, 5, 6]]))

    def refused(what, t=types, tables=(good,), runtime=()):
        rc, h, msg = raw_create_lookup(khip, srs, t, wires, co, tables, runtime)
        assert rc == KH_E_INVALID and h is None and msg, (what, rc, msg)
        return msg
    assert "collision" in refused("two fixed tables with one id", tables=(good, (4, tab([[9]]))))
    xor = list(types); xor[3] = gids["Xor16"]
    assert "collision" in refused("a fixed table with the XOR table's id", t=xor, tables=((0, tab([[0, 1], [0, 1], [0, 1]])),))
    rc0 = list(types); rc0[3] = gids["RangeCheck0"]
    assert "collision" in refused("a runtime table with the range-check table's id", t=rc0, tables=(), runtime=((1, tab([[5, 6]])[0]),))
    assert "twice" in refused("duplicate runtime ids", runtime=((7, tab([[5, 6]])[0]), (7, tab([[8]])[0])))
    assert "zero" in refused("table 0 without a zero entry", tables=((0, tab([[1, 2, 0], [4, 0, 6]])),))
    assert "zero" in refused("runtime table 0 without a zero entry", runtime=((0, tab([[5, 6]])[0]),))
    # the domain grows with the tables, so only the exact fit is too long: 60 entries of a table 0 (no dummy row) give n = 64 = 60 + 1 + zk_rows
    assert "entries" in refused("too many entries", tables=((0, tab([list(range(60))])),))
    big = good[1].copy(); big[1, 2] = np.frombuffer(F.p.to_bytes(32, "little"), dtype=np.uint64)
    assert ">= p" in refused("a table value = p", tables=((4, big),))
    generic = [gids["Generic"]] * 20
    assert "pattern" in refused("runtime tables without a pattern", t=generic, tables=(), runtime=((7, tab([[5, 6]])[0]),))
    refused("a table without columns", tables=((4, np.zeros((0, 3, 4), dtype=np.uint64)),))
    bad = list(types); bad[3] = gids["Permutation"]
    refused("Permutation", t=bad)
    bad = list(types); bad[3] = 99
    refused("an unknown gate id", t=bad)
    # valid inputs next to the refused ones: a table 0 WITH a zero entry; no tables at all; tables but no pattern = kh_prover_index_create
    for tables in (((0, tab([[1, 0, 3], [4, 0, 6]])),), ()):
        rc, h, msg = raw_create_lookup(khip, srs, types, wires, co, tables)
        assert rc == 0 and h, msg
        khip.raw().kh_prover_index_free(C.c_void_p(h))
    # the old entry point still refuses every gate with a lookup pattern, and GateType::Lookup, with its old words
    for name in ("Xor16", "RangeCheck0", "RangeCheck1", "Rot64", "ForeignFieldMul"):
        t = list(generic); t[7] = gids[name]
        rc, h, msg = raw_create(khip, srs, t, wires, co)
        assert rc == KH_E_INVALID and h is None and "kh_prover_index_new + kh_prover_index_attach_lookup" in msg, (name, msg)
    t = list(generic); t[7] = khip.GATE_LOOKUP
    rc, h, msg = raw_create(khip, srs, t, wires, co)
    assert rc == KH_E_INVALID and h is None and msg


def test_without_patterns_the_lookup_entry_point_gives_the_plain_index(khip):
    from proof_systems_amd import prover
    from test_gpu_index_create import bench_records
    F = fld(khip)
    srs = khip.Srs.create(khip.VESTA, 1 << 10)
    types, wires, co = bench_records(khip, F, 1000)
    a = khip.NativeProverIndex.create(srs, types, wires, co)
    b = khip.NativeProverIndex.create_lookup(srs, types, wires, co)
    va, vb = a.verifier_index(), b.verifier_index()
    assert a.shape() == b.shape() and vb["lookup_info"] is None and b.lookup_column("atom_d8", 0) is None
    for key, v in va.items():
        if key != "lookup_info":
            assert all(np.array_equal(x, y) for x, y in zip(v, vb[key])) if isinstance(v, tuple) else np.array_equal(v, vb[key]), key
    a.free(); b.free()


# ---- 6. lifetime: nothing of the caller's arrays is kept; several lookup indices on one SRS, freed in any order
def test_created_lookup_indices_own_their_data_and_share_an_srs(khip):
    from proof_systems_amd import prover
    C_ = P.VESTA; F = fld(khip)
    cs, tabs, wit = fixed_table_circuit(C_.scalar)
    srs = khip.Srs.create(khip.VESTA, 1 << cs["log2_n"])
    types, wires, co = records(khip, cs, F)
    tl = [(t["id"], np.stack([F.limbs_many(c) for c in t["data"]])) for t in tabs]
    gids = {"Lookup": khip.GATE_LOOKUP}
    ids = [gids[t] for t in types]
    a = khip.NativeProverIndex.create_lookup(srs, ids, wires, co, 0, tl)
    want_digest = a.verifier_index()["digest"]
    for _i, d in tl:
        d[:] = 0xfffffffffffffff                             # the caller's tables, wires and coefficients are overwritten after the call
    wires[:] = 3; co[:] = 0xfffffffffffffff
    ixs = [created(khip, srs, cs, F, tables=tabs) for _ in range(3)]
    w = np.stack([F.limbs_many(col) for col in wit])
    seed = bytes([5, 6] + [7] * 30)
    want = serialized(C_, ixs[0], prover.create_proof_native(ixs[0], w, V.RefRng(P.StdRng(seed))))
    assert np.array_equal(ixs[1].vindex["digest"], want_digest)
    sec, _ph = a.prove(witness=w, randomness=F.limbs_many(F.rand_many(V.RefRng(P.StdRng(seed)), a.randomness_count(True))))
    ref, _ph = ixs[0].native.prove(witness=w, randomness=F.limbs_many(F.rand_many(V.RefRng(P.StdRng(seed)), a.randomness_count(True))))
    assert all(np.array_equal(np.asarray(sec[k][0] if isinstance(sec[k], tuple) else sec[k]), np.asarray(ref[k][0] if isinstance(ref[k], tuple) else ref[k])) for k in sec)
    ixs[1].free()                                            # freed against the creation order, the others keep proving
    assert serialized(C_, ixs[2], prover.create_proof_native(ixs[2], w, V.RefRng(P.StdRng(seed)))) == want
    a.free(); ixs[0].free()
    assert serialized(C_, ixs[2], prover.create_proof_native(ixs[2], w, V.RefRng(P.StdRng(seed)))) == want
    bufs = [khip.DevBuf(32 * 8 << cs["log2_n"]) for _ in range(3)]
    with pytest.raises(khip.KhError, match="kh_prover_index_create_lookup"):
        ixs[2].native.attach_lookup(["Lookup"], bufs[:1], bufs[:1], bufs[:1], bufs[:1], None, bufs)
    with pytest.raises(khip.KhError, match="kh_prover_index_create_lookup"):
        ixs[2].native.attach_runtime_tables(bufs[0], bufs[1], bufs[2], 0, 1)
    ixs[2].free()
    for b in bufs:
        b.free()


# ---- 7. a C caller with only the header
def test_a_c_program_creates_a_lookup_index_and_proves(khip, tmp_path):
    from proof_systems_amd import prover
    rows, entries = 100, 20
    src = os.path.join(HERE, "cpp", "test_index_create_lookup.cpp")
    exe = str(tmp_path / "test_index_create_lookup")
    libdir = os.path.join(ROOT, "proof_systems_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lkimchi_hip", "-Wl,-rpath," + libdir,
                           "-Wl,--allow-shlib-undefined", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    C_ = P.VESTA; Fo = C_.scalar; F = fld(khip)
    tabs = [{"id": 3, "data": [[3 * j + 1 for j in range(entries)], [j * j + 2 for j in range(entries)]]}]
    cs = CC.build(Fo, [CC.gate("Lookup", r) for r in range(rows)], lookup_tables=tabs)
    assert cs["log2_n"] == 7
    wit = [[0] * rows for _ in range(15)]
    for r in range(rows):
        wit[0][r] = 3
        for k in range(3):
            e = (3 * r + k) % entries
            wit[1 + 2 * k][r], wit[2 + 2 * k][r] = tabs[0]["data"][0][e], tabs[0]["data"][1][e]
    srs = khip.Srs.create(khip.VESTA, 128)
    pix = python_index(khip, cs, srs, F, tabs)               # the Python-built index of the same circuit
    nx = prover.native_index(pix)
    count = nx.randomness_count(True)
    rnd = F.limbs_many(F.rand_many(V.RefRng(P.StdRng(bytes([77] * 32))), count))
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.array([count], dtype=np.uint64), rnd.reshape(-1)]).tofile(inp)
    r = subprocess.run([exe, str(rows), str(entries), inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "INDEX_CREATE_LOOKUP_OK" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    assert np.array_equal(raw[:32].view(np.uint64), np.asarray(pix.digest).reshape(-1))
    pos = 32

    def section():
        nonlocal pos
        cnt, pts = (int(x) for x in raw[pos:pos + 16].view(np.uint64)); pos += 16
        wd = 8 if pts else 4
        limbs = raw[pos:pos + 8 * wd * cnt].view(np.uint64).reshape(cnt, wd); pos += 8 * wd * cnt
        flags = None
        if pts:
            flags = raw[pos:pos + cnt]; pos += cnt
        return limbs, flags
    LI = pix.lookup
    same = lambda got, comms: np.array_equal(got[0], np.concatenate([np.asarray(c[0]).reshape(-1, 8) for c in comms])) and \
        np.array_equal(got[1], np.concatenate([np.asarray(c[1], np.uint8).reshape(-1) for c in comms]))
    assert same(section(), LI.table_comm), "table commitments"
    assert same(section(), [LI.table_ids_comm]), "table-id commitment"
    assert same(section(), [LI.selector_comm[q] for q in LI.patterns]), "pattern selector commitments"
    assert section()[0].shape[0] == 0, "runtime selector commitment of an index without runtime tables"
    info = section()[0].reshape(-1)
    assert list(info[:5]) == [LI.max_per_row, LI.max_joint_size, int(LI.joint_lookup_used), 0, 1 << khip.LOOKUP_PATTERN_IDS["Lookup"]] and info[5] == len(LI.d_table_cols)
    want, _ph = nx.prove(witness=np.stack([F.limbs_many(col) for col in wit]), randomness=rnd)
    for name in khip.PROOF_SECTIONS:
        limbs, flags = section()
        if isinstance(want[name], tuple):
            assert limbs.shape[0] == want[name][0].shape[0] and (flags is None or (np.array_equal(limbs, want[name][0]) and np.array_equal(flags, want[name][1]))), name
        else:
            assert np.array_equal(limbs, want[name]), name
    assert pos == raw.shape[0]
    pix.free_lookup(); pix.free()
