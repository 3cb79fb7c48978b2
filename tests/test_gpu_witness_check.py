"""kh_witness_check: the first unsatisfied row of a witness, found on the device (csrc/witness_check.hip), against the oracle.

The expected report is computed here from oracle/gates.py's `*_row` functions (one value per constraint) and the oracle constraint system's `gates`
list, walking the rows in the reference's order (ProverIndex::verify, constraints.rs): rows upwards, within a row the seven wires by column, then the
row's gate.  Kind, row, gate id, constraint mask / wired cell and the two counts must be equal exactly -- the check is deterministic."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

from oracle import circuit as CC
from oracle import gates as G
from oracle import pasta as P
from proof_systems_amd import polish as OP

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import make_proof_fixtures as M  # noqa: E402
from test_gates import gate_rows, on_both_fields, tables  # noqa: E402

GATE_NAMES = list(OP.GATES) + ["Generic"]
NCONSTRAINTS = dict(G.ROW_MACHINES, Generic=2)
LOOKUP_GATES = ("Xor16", "RangeCheck0", "RangeCheck1", "Rot64", "ForeignFieldMul")


# ---------------------------------------------------------------------------------------------------------------- the oracle side
def row_constraints(F, typ, curr, nxt, co, pub):
    """the constraints of one row, one value each, in the order of polish.GATES / oracle.gates"""
    from oracle import poseidon as S
    p = F.p
    if typ == "Generic":
        return [(co[0] * curr[0] + co[1] * curr[1] + co[2] * curr[2] + co[3] * curr[0] * curr[1] + co[4] - pub) % p,
                (co[5] * curr[3] + co[6] * curr[4] + co[7] * curr[5] + co[8] * curr[3] * curr[4] + co[9]) % p]
    if typ == "Poseidon":
        return G.poseidon_row(F, curr, nxt, co, S.params("fp" if F is P.Fp else "fq")["mds"])
    if typ == "CompleteAdd":
        return G.complete_add_row(F, curr)
    if typ == "VarBaseMul":
        return G.varbasemul_row(F, curr, nxt)
    if typ == "EndoMul":
        return G.endomul_row(F, curr, nxt, P.endos(P.PALLAS if F is P.Fp else P.VESTA)[0])
    if typ == "EndoMulScalar":
        return G.endomul_scalar_row(F, curr)
    if typ == "Xor16":
        return G.xor16_row(F, curr, nxt)
    if typ == "RangeCheck0":
        return G.range_check0_row(F, curr, nxt, co)
    if typ == "RangeCheck1":
        return G.range_check1_row(F, curr, nxt)
    if typ == "Rot64":
        return G.rot64_row(F, curr, nxt, co)
    if typ == "ForeignFieldAdd":
        return G.foreign_field_add_row(F, curr, nxt, co)
    if typ == "ForeignFieldMul":
        return G.foreign_field_mul_row(F, curr, nxt, co)
    raise NotImplementedError(typ)


class Circuit:
    """an oracle constraint system with what the expected report needs: gate type, wires and coefficients of the recorded rows, a witness as rows"""

    def __init__(self, cs, witness_cols):
        self.cs, self.F, self.n, self.public = cs, cs["F"], cs["n"], cs["public"]
        gates = cs["gates"]
        self.rows = len(witness_cols[0])                                                   # the recorded rows, what the index is created from: the witness's (build() pads behind them)
        self.types = [g["typ"] for g in gates[:self.rows]]
        self.wires = [list(g["wires"]) for g in gates[:self.rows]]
        self.co = [[cs["coefficients"][c][r] for c in range(15)] for r in range(self.rows)]
        wr = len(witness_cols[0])
        self.w = [[witness_cols[c][r] % self.F.p for c in range(15)] for r in range(wr)]       # witness rows (host witness: padded with zeros)
        self._base = None

    def cell(self, w, r, c):
        return w[r][c] if r < len(w) else 0

    def mask(self, w, r):
        typ = self.types[r] if r < self.rows else "Zero"
        if typ in ("Zero", "Lookup"):
            return 0
        curr = [self.cell(w, r, c) for c in range(15)]
        nxt = [self.cell(w, (r + 1) % self.n, c) for c in range(15)]
        vals = row_constraints(self.F, typ, curr, nxt, self.co[r], curr[0] if r < self.public else 0)
        assert len(vals) == NCONSTRAINTS[typ]
        return sum(1 << i for i, v in enumerate(vals) if v % self.F.p)

    def base_masks(self):
        if self._base is None:
            self._base = [self.mask(self.w, r) for r in range(self.rows)]
        return self._base

    def expected(self, khip, w=None, touched=None, gates=True, wires=True):
        """(kind, row, gate id, mask, col, wired_row, wired_col, gate rows violated, cells disconnected) for the witness rows `w` (default: the
        circuit's own); touched: the rows that differ from the circuit's own witness (only they and their predecessors are evaluated again)"""
        w = self.w if w is None else w
        if touched is None:
            masks = [self.mask(w, r) for r in range(self.rows)]
        else:
            masks = list(self.base_masks())
            for t in touched:
                for r in (t, (t - 1) % self.n):
                    if r < self.rows:
                        masks[r] = self.mask(w, r)
        gids = khip.gate_ids()
        first, nrows, ncells = None, 0, 0
        for r in range(self.rows):
            for c in range(7):
                r2, c2 = self.wires[r][c]
                if wires and self.cell(w, r, c) != self.cell(w, r2, c2):
                    ncells += 1
                    first = first or (khip.WITNESS_DISCONNECTED, r, -1, 0, c, r2, c2)
            if gates and masks[r]:
                nrows += 1
                first = first or (khip.WITNESS_GATE, r, gids[self.types[r]], masks[r], 0, 0, 0)
        return (first or (khip.WITNESS_OK, 0, -1, 0, 0, 0, 0)) + (nrows, ncells)

    def records(self, khip, F):
        gids = khip.gate_ids()
        types = [khip.GATE_ZERO if t == "Zero" else gids[t] for t in self.types]
        wires = np.array(self.wires, dtype=np.uint32).reshape(self.rows, 7, 2)
        co = np.stack([F.limbs_many(self.co[r]) for r in range(self.rows)])
        return types, wires, co

    def limbs(self, F, w=None):
        w = self.w if w is None else w
        return np.stack([F.limbs_many([row[c] for row in w]) for c in range(15)])


def got(rep):
    return (rep.kind, rep.row, rep.gate, rep.constraints, rep.col, rep.wired_row, rep.wired_col, rep.gate_rows_violated, rep.cells_disconnected)


def gate_circuit(name, F=P.Fp):
    """the satisfied instance of tests/test_gates.py from row 0: live rows carry the gate type, the others are Zero"""
    p = F.p
    if name == "Generic":
        rnd = random.Random(7)
        gates, rows = [], []
        for r in range(4):
            a, b = rnd.randrange(p), rnd.randrange(p)
            gates.append(CC.generic_gadget(p, r, CC.generic_spec(p, "Add"), CC.generic_spec(p, "Mul")))
            rows.append([a, b, (a + b) % p, b, a, a * b % p] + [0] * 9)
    else:
        w, co, ngate = tables(name, random.Random(7), F)
        live = set(gate_rows(name, ngate))
        gates = [CC.gate(name if k in live else "Zero", k, [c % p for c in co[k]] if k in live else []) for k in range(len(w))]
        rows = [list(r) for r in w]
    return Circuit(CC.build(F, gates), [[r[c] for r in rows] for c in range(15)])


# ---------------------------------------------------------------------------------------------------------------- the device side
@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


@pytest.fixture(scope="module")
def srs13(khip):
    return khip.Srs.create(khip.VESTA, 1 << 13)


@pytest.fixture(scope="module")
def srs13_pallas(khip):
    return khip.Srs.create(khip.PALLAS, 1 << 13)


def created(khip, srs, circ):
    from proof_systems_amd import prover
    F = prover.Fld(khip.FP if srs.curve == khip.VESTA else khip.FQ)
    types, wires, co = circ.records(khip, F)
    return prover.CreatedIndex(srs, types, wires, co, public=circ.public), F


def check(khip, ix, circ, F, w=None, touched=None, flags=None, limbs=None):
    flags = khip.WITNESS_GATES | khip.WITNESS_WIRES if flags is None else flags
    rep = khip.witness_check(ix.native, limbs if limbs is not None else circ.limbs(F, w), flags=flags)
    want = circ.expected(khip, w, touched, gates=bool(flags & khip.WITNESS_GATES), wires=bool(flags & khip.WITNESS_WIRES))
    assert got(rep) == want, (got(rep), want)
    return rep


def spoiled(circ, cells, delta=1):
    w = [list(r) for r in circ.w]
    for r, c in cells:
        w[r][c] = (w[r][c] + delta) % circ.F.p
    return w


# ---- 1. every constraint of every gate
@pytest.mark.parametrize("name,Fo", on_both_fields(GATE_NAMES))
def test_every_constraint_of_every_gate(khip, request, name, Fo):
    """over Fq (a Pallas SRS): the comparing sink's other instantiation, with the gate_fixed_constants(field = 1, ...) tables -- the "fq" MDS, Vesta's endo coefficient"""
    circ = gate_circuit(name, Fo)
    ix, F = created(khip, request.getfixturevalue("srs13" if Fo is P.Fp else "srs13_pallas"), circ)
    assert F.p == Fo.p
    assert ix.n == circ.n and (name not in LOOKUP_GATES or circ.n == (1 << 9 if name == "Xor16" else 1 << 13)), ix.n     # the gate tables set the lookup gates' domain
    base = circ.limbs(F)
    rep = check(khip, ix, circ, F, limbs=base)
    if name != "ForeignFieldMul":                                  # (its oracle instance is random rows)
        assert rep.kind == khip.WITNESS_OK
    full = (1 << NCONSTRAINTS[name]) - 1
    seen_set, seen_clear = 0, 0
    for r, t in enumerate(circ.types):
        if t == name:
            seen_set |= circ.base_masks()[r]; seen_clear |= full & ~circ.base_masks()[r]
    delta_rnd = random.Random(7).randrange(2, F.p)
    violated = 0
    for r in range(len(circ.w)):
        for c in range(15):
            for delta in (1, delta_rnd):
                w = spoiled(circ, [(r, c)], delta)
                limbs = base.copy(); limbs[c, r] = F.limbs(w[r][c])
                rep = check(khip, ix, circ, F, w=w, touched=[r], limbs=limbs)
                violated += rep.kind != khip.WITNESS_OK
                for q, t in enumerate(circ.types):
                    if t == name and q in (r, r - 1):
                        mk = circ.mask(w, q)
                        seen_set |= mk; seen_clear |= full & ~mk
    assert violated > 0
    # the spoils above exercise every constraint both ways: each bit set in some report, and clear in some (ForeignFieldMul's random rows never clear one)
    assert seen_set == full, (name, bin(seen_set))
    assert seen_clear == (0 if name == "ForeignFieldMul" else full), (name, bin(seen_clear))
    ix.free()


# ---- 2. block and wave boundaries, the minimum across blocks
def library_indexes(khip, srs, Fo):
    out = {}
    for logn in (7, 8):
        cs, wit = M.library_circuit(Fo, logn)
        circ = Circuit(cs, wit)
        ix, F = created(khip, srs, circ)
        out[logn] = (circ, ix, F)
    yield out
    for _c, ix, _F in out.values():
        ix.free()


@pytest.fixture(scope="module")
def library(khip, srs13):
    yield from library_indexes(khip, srs13, P.Fp)


@pytest.fixture(scope="module")
def library_pallas(khip, srs13_pallas):
    """the same circuits over Fq (points on Vesta, the "fq" Poseidon parameters), indexed over a Pallas SRS"""
    yield from library_indexes(khip, srs13_pallas, P.Fq)


def nearest_gate_row(circ, r):
    return min((q for q, t in enumerate(circ.types) if t != "Zero"), key=lambda q: (abs(q - r), q))


@pytest.mark.parametrize("logn,lib", [pytest.param(7, "library", id="7"), pytest.param(8, "library", id="8"),
                                      pytest.param(7, "library_pallas", id="7-fq"), pytest.param(8, "library_pallas", id="8-fq")])
def test_block_and_wave_boundaries(khip, request, logn, lib):
    circ, ix, F = request.getfixturevalue(lib)[logn]
    assert ix.srs.curve == (khip.VESTA if lib == "library" else khip.PALLAS) and F.p == circ.F.p
    assert ix.n == 1 << logn and (logn != 8 or circ.rows > 128)
    assert check(khip, ix, circ, F).kind == khip.WITNESS_OK
    last = max(q for q, t in enumerate(circ.types) if t != "Zero")
    for target in (0, 63, 64, 127, 128, last):
        r = nearest_gate_row(circ, min(target, last))
        rep = check(khip, ix, circ, F, w=spoiled(circ, [(r, 0)]), touched=[r])
        assert rep.kind == khip.WITNESS_GATE and rep.row in (r, r - 1), (target, r, rep.row)
    if logn == 8:                                                  # two cells in different blocks at once: the lower row wins, both are counted
        lo, hi = nearest_gate_row(circ, 40), nearest_gate_row(circ, 200)
        assert lo < 128 <= hi
        rep = check(khip, ix, circ, F, w=spoiled(circ, [(lo, 0), (hi, 0)]), touched=[lo, hi])
        assert rep.kind == khip.WITNESS_GATE and rep.row in (lo, lo - 1) and rep.gate_rows_violated >= 2


# ---- 3. - 6. wiring, public inputs, both fields, the chunked shape
def wired_circuit(Fo, log2_n, log_srs):
    """generic_circuit + one cross-row pair in column 6 (no generic constraint reads it), holding the same value in both cells"""
    cs, wit = M.generic_circuit(Fo, log2_n, log_srs)
    gates = [dict(g, wires=list(g["wires"])) for g in cs["gates"][:len(wit[0])]]
    CC.connect_cell_pair(gates, (4, 6), (9, 6))
    wit = [list(col) for col in wit]
    wit[6][4] = wit[6][9] = 77
    cs2 = CC.build(Fo, gates, public=cs["public"], max_poly_size=(1 << log_srs) if log_srs < log2_n else None)
    assert cs2["log2_n"] == log2_n
    return Circuit(cs2, wit)


@pytest.mark.parametrize("curve,log2_n", [(0, 5), (1, 5), (0, 6)])
def test_wiring_public_inputs_fields_and_chunks(khip, curve, log2_n):
    Fo = P.Fp if curve == 0 else P.Fq
    circ = wired_circuit(Fo, log2_n, 5)
    srs = khip.Srs.create(khip.VESTA if curve == 0 else khip.PALLAS, 32)
    ix, F = created(khip, srs, circ)
    assert ix.native.shape() == (log2_n, 3 if log2_n == 5 else 5, 1 if log2_n == 5 else 2)
    assert check(khip, ix, circ, F).kind == khip.WITNESS_OK
    # a broken wired cell: the lowest (row, column) and its partner; both cells of the pair count
    rep = check(khip, ix, circ, F, w=spoiled(circ, [(9, 6)]))
    assert (rep.kind, rep.row, rep.col, rep.wired_row, rep.wired_col, rep.cells_disconnected) == (khip.WITNESS_DISCONNECTED, 4, 6, 9, 6, 2)
    # (r, 0) ~ (r, 4): spoiling (5, 4) breaks the wire (first: cell (5, 0)) and the second generic constraint of row 5 -- the wire comes first
    rep = check(khip, ix, circ, F, w=spoiled(circ, [(5, 4)]))
    assert (rep.kind, rep.row, rep.col, rep.wired_row, rep.wired_col) == (khip.WITNESS_DISCONNECTED, 5, 0, 5, 4)
    # a gate violation on a lower row than a wire violation wins, and the other way round
    rep = check(khip, ix, circ, F, w=spoiled(circ, [(3, 2), (9, 6)]))
    assert (rep.kind, rep.row, rep.constraints) == (khip.WITNESS_GATE, 3, 1) and rep.cells_disconnected == 2
    rep = check(khip, ix, circ, F, w=spoiled(circ, [(4, 6), (8, 2)]))
    assert (rep.kind, rep.row, rep.col) == (khip.WITNESS_DISCONNECTED, 4, 6) and rep.gate_rows_violated == 1
    # the gates alone do not see the wire, the wires alone not the gate
    w = spoiled(circ, [(9, 6), (12, 5)])
    assert check(khip, ix, circ, F, w=w, flags=khip.WITNESS_GATES).row == 12
    assert check(khip, ix, circ, F, w=w, flags=khip.WITNESS_WIRES).kind == khip.WITNESS_DISCONNECTED
    assert check(khip, ix, circ, F, w=spoiled(circ, [(9, 6)]), flags=khip.WITNESS_GATES).kind == khip.WITNESS_OK
    # public inputs: any value in the three public cells satisfies row r < 3 (without the public term row 0 would fail)
    w = spoiled(circ, [(0, 0), (1, 0), (2, 0)], delta=123456789)
    assert check(khip, ix, circ, F, w=w).kind == khip.WITNESS_OK
    ix.free()
    # a public row whose coefficient is spoiled in the gate list fails with constraint 0
    bad = wired_circuit(Fo, log2_n, 5)
    bad.co[1][0] = 2
    ix, F = created(khip, srs, bad)
    rep = check(khip, ix, bad, F)
    assert (rep.kind, rep.row, rep.constraints, rep.gate) == (khip.WITNESS_GATE, 1, 1, khip.gate_ids()["Generic"])
    ix.free()
    srs.close()


# ---- 7. device witness
def test_device_witness(khip, library):
    circ, ix, F = library[8]
    n, zk = ix.n, ix.zk_rows
    rnd = random.Random(3)

    def padded(w, zk_random):
        cols = np.zeros((15, n, 4), dtype=np.uint64)
        cols[:, :len(w)] = circ.limbs(F, w)
        if zk_random:
            cols[:, n - zk:] = F.limbs_many([rnd.randrange(F.p) for _ in range(15 * zk)]).reshape(15, zk, 4)
        return cols

    buf = khip.DevBuf(15 * n * 32)
    for w, touched in ((None, None), (spoiled(circ, [(nearest_gate_row(circ, 130), 0)]), [nearest_gate_row(circ, 130)])):
        want = circ.expected(khip, w, touched if touched is not None else [])
        for zk_random in (False, True):                            # the zero-knowledge rows are Zero rows wired to themselves: their values do not matter
            buf.upload(padded(circ.w if w is None else w, zk_random))
            assert got(khip.witness_check(ix.native, witness_dev=buf)) == want
        assert got(khip.witness_check(ix.native, circ.limbs(F, w))) == want
    buf.free()


# ---- 8. an index from kh_prover_index_new (the Python ProverIndex), and the refusals
def test_index_from_columns_and_refusals(khip, srs13, library):
    from proof_systems_amd import prover
    circ, cix, F = library[7]
    co = np.stack([F.limbs_many(circ.co[r]) for r in range(circ.rows)])
    pix = prover.ProverIndex(khip.VESTA, 7, co, srs13, gate_types=circ.types)
    r = nearest_gate_row(circ, 70)
    for w, touched in ((None, []), (spoiled(circ, [(r, 0)]), [r])):
        want = circ.expected(khip, w, touched, wires=False)
        a = khip.witness_check(prover.native_index(pix), circ.limbs(F, w), flags=khip.WITNESS_GATES)
        b = khip.witness_check(cix.native, circ.limbs(F, w), flags=khip.WITNESS_GATES)
        assert got(a) == got(b) == want
    assert pix.check_witness(circ.limbs(F)).ok and cix.check_witness(circ.limbs(F)).ok
    rep = cix.check_witness(circ.limbs(F, spoiled(circ, [(r, 0)])))
    assert not rep and rep.kind == "gate" and rep.gate == circ.types[rep.row] and str(rep.row) in rep.message
    with pytest.raises(khip.KhError, match="KH_WITNESS_WIRES needs the gate list's wires"):
        khip.witness_check(prover.native_index(pix), circ.limbs(F), flags=khip.WITNESS_WIRES)
    # refusals leave *out untouched
    lib = khip.raw()
    w = circ.limbs(F)
    rep = khip.WitnessReportC(kind=99, row=12345)
    buf = khip.DevBuf(15 * cix.n * 32)
    wp = w.ctypes.data_as(C.POINTER(C.c_uint64))
    nat = cix.native._h
    many = np.zeros((15, cix.n - cix.zk_rows + 1, 4), dtype=np.uint64)
    for args in ((None, wp, w.shape[1], None, 3, C.byref(rep)), (nat, wp, w.shape[1], None, 3, None), (nat, wp, w.shape[1], None, 0, C.byref(rep)),
                 (nat, wp, w.shape[1], None, 4, C.byref(rep)), (nat, wp, w.shape[1], C.c_void_p(buf.ptr), 3, C.byref(rep)), (nat, None, 0, None, 3, C.byref(rep)),
                 (nat, many.ctypes.data_as(C.POINTER(C.c_uint64)), many.shape[1], None, 3, C.byref(rep))):
        assert lib.kh_witness_check(*args) == -1 and lib.kh_last_error()
        assert (rep.kind, rep.row) == (99, 12345)
    buf.free()
    pix.free()


# ---- 9. agreement with the prover's own check
def test_agrees_with_the_prover_check(khip, library):
    agrees_with_the_prover_check(khip, library[7])


def test_agrees_with_the_prover_check_on_pallas(khip, library_pallas):
    agrees_with_the_prover_check(khip, library_pallas[7])


def agrees_with_the_prover_check(khip, lib):
    from proof_systems_amd import prover
    circ, ix, F = lib
    rng = lambda: P.StdRng(bytes([5] * 32))
    from oracle import views as V
    prover.create_proof_native(ix, circ.limbs(F), V.RefRng(rng()), check=True)
    for r in (nearest_gate_row(circ, 2), nearest_gate_row(circ, 64), nearest_gate_row(circ, 110)):
        w = circ.limbs(F, spoiled(circ, [(r, 0)]))
        assert khip.witness_check(ix.native, w).kind == khip.WITNESS_GATE
        with pytest.raises(khip.KhError, match="the witness does not satisfy the constraints"):
            prover.create_proof_native(ix, w, V.RefRng(rng()), check=True)


# ---- 10. the message
def test_report_message(khip, library):
    circ, ix, F = library[7]
    r = nearest_gate_row(circ, 20)
    rep = khip.witness_check(ix.native, circ.limbs(F, spoiled(circ, [(r, 0)])))
    msg = khip.witness_report_message(rep)
    name = {g: t for t, g in khip.gate_ids().items()}[rep.gate]
    assert msg.startswith("row %d: gate %s, constraint" % (rep.row, name)) and "of %d" % NCONSTRAINTS[name] in msg and "(%d row" % rep.gate_rows_violated in msg
    for i in range(NCONSTRAINTS[name]):
        assert ((" %d," % i in msg or " %d of" % i in msg) == bool(rep.constraints >> i & 1)), (i, msg)
    assert khip.witness_report_message(khip.witness_check(ix.native, circ.limbs(F))) == "the witness satisfies the circuit"
    rep2 = khip.WitnessReportC(kind=khip.WITNESS_DISCONNECTED, row=12, col=0, wired_row=12, wired_col=4, cells_disconnected=2)
    assert khip.witness_report_message(rep2).startswith("row 12, column 0 is wired to (12, 4) but holds a different value")
    # truncation: NUL-terminated inside cap, the return value is the whole length
    buf = C.create_string_buffer(b"\xff" * 32, 32)
    full = khip.raw().kh_witness_report_message(C.byref(rep), buf, C.c_size_t(10))
    assert full == len(msg) and buf.raw[:10] == msg[:9].encode() + b"\0" and buf.raw[10:] == b"\xff" * 22
    assert khip.raw().kh_witness_report_message(C.byref(rep), None, C.c_size_t(0)) == len(msg)
    assert khip.raw().kh_witness_report_message(None, buf, C.c_size_t(10)) == -1
