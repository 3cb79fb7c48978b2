"""kh_witness_check_full with KH_WITNESS_LOOKUPS: the first looked-up tuple of a witness that is in no table, found on the device
(csrc/witness_check.hip: k_witness_lookup_build / k_witness_lookup_probe), against a brute-force restatement.

The expected result is computed here from the oracle's lookup constraint system (oracle.lookup.LookupCS: table_cols, table_ids, selectors, info,
PATTERNS): the set of table tuples (id, c_0, .., c_{W-1}) of the rows t < L = n - zk_rows - 1 (column 1 of the runtime rows = the call's runtime
values), then the rows r < L in order, every joint lookup of every pattern whose selector is 1 on the row.  It gives the first (row, joint lookup),
the number of misses and the looked-up tuple; kind, row, pattern, joint lookup, columns, limbs and count must be equal exactly.

Section 10 runs tables whose tuples are made to collide under the tuple hash (tests/lookup_collisions.py, pinned to csrc/lookup_hash.hpp by
tests/test_lookup_hash.py): every table row's home slot is one of the last two of the 1024 slots, so the index's table is one probe chain across the end of
the slot array -- with random entries at a load of 0.2 a chain has one or two slots."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import circuit as CC
from oracle import gates as G
from oracle import lookup as OL
from oracle import pasta as P
from oracle import views as V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_proof_fixtures as M  # noqa: E402
sys.path.insert(0, HERE)
import lookup_collisions as LC  # noqa: E402

PATTERN_IDS = {"Xor": 0, "Lookup": 1, "RangeCheck": 2, "ForeignFieldMul": 3}
Fo = P.Fp                       # the default field of the cases (a Vesta SRS); the `*_on_pallas` tests run the same bodies with the brute force on P.Fq


# ---------------------------------------------------------------------------------------------------------------- the brute-force side
class Case:
    """an oracle constraint system with lookups, its gate records and a witness (15 columns of integers)"""

    def __init__(self, gates, wit, tables=(), runtime_cfg=None, runtime=None, Fo=Fo):
        self.gates, self.tables, self.runtime_cfg, self.Fo = gates, list(tables), runtime_cfg, Fo
        self.cs = CC.build(Fo, gates, lookup_tables=self.tables, runtime_tables=runtime_cfg)
        self.L = self.cs["lookup"]
        self.n, self.zk = self.cs["n"], self.cs["zk_rows"]
        self.rows = len(gates)
        self.wit = [list(c) for c in wit]
        self.runtime = runtime                          # the second columns of the runtime tables, concatenated
        self._sets = {}

    def table_set(self, runtime):
        key = tuple(runtime) if runtime is not None else None
        if key not in self._sets:
            L, lim = self.L, self.n - self.zk - 1
            cols = [list(c) for c in L.table_cols]
            if runtime is not None:
                cols[1][L.runtime_offset:L.runtime_offset + len(runtime)] = [v % self.Fo.p for v in runtime]
            self._sets[key] = {((L.table_ids[t] if L.table_ids is not None else 0),) + tuple(c[t] for c in cols) for t in range(lim)}
        return self._sets[key]

    def misses(self, wit=None, runtime="own"):
        """[(row, joint lookup, pattern id, table id, entry values, witness columns)] in the order of the report's key, for rows < L"""
        wit = self.wit if wit is None else wit
        runtime = self.runtime if runtime == "own" else runtime
        table, L = self.table_set(runtime), self.L
        W = len(L.table_cols)
        cell = lambda c, r: wit[c][r] % self.Fo.p if r < len(wit[c]) else 0
        out = []
        for r in range(self.n - self.zk - 1):
            for q in L.info.patterns:
                if not L.selectors[q][r]:
                    continue
                for s, (tid, entries) in enumerate(OL.PATTERNS[q]["lookups"]):
                    cols = [e[0][1][1] for e in entries]
                    vals = [cell(c, r) for c in cols]
                    tup = ((tid[1] if tid[0] == "const" else cell(tid[1], r)),) + tuple(vals) + (0,) * (W - len(vals))
                    if tup not in table:
                        out.append((r, s, PATTERN_IDS[q], tup[0], vals, cols))
        return sorted(out, key=lambda m: (m[0], m[1], m[2]))

    def records(self, khip, F):
        gids = khip.gate_ids()
        special = {"Zero": khip.GATE_ZERO, "Lookup": khip.GATE_LOOKUP}
        types = [special[g["typ"]] if g["typ"] in special else gids[g["typ"]] for g in self.gates]
        wires = np.array([g["wires"] for g in self.gates], dtype=np.uint32).reshape(self.rows, 7, 2)
        co = np.stack([F.limbs_many([c % self.Fo.p for c in (list(g["coeffs"]) + [0] * 15)[:15]]) for g in self.gates])
        return types, wires, co

    def limbs(self, F, wit=None):
        return np.stack([F.limbs_many([v % self.Fo.p for v in col]) for col in (self.wit if wit is None else wit)])

    def spoiled(self, cells):
        """the witness with the cells {(row, column): value} replaced"""
        w = [list(c) for c in self.wit]
        for (r, c), v in cells.items():
            w[c][r] = v % self.Fo.p
        return w


def expect(khip, F, case, rep, lk, wit=None, runtime="own"):
    """the report of a call with KH_WITNESS_LOOKUPS alone against the brute force"""
    ms = case.misses(wit, runtime)
    assert lk.lookups_missing == len(ms), (lk.lookups_missing, len(ms))
    if not ms:
        assert rep.kind == khip.WITNESS_OK and (lk.pattern, lk.slot, lk.ncells) == (-1, -1, 0)
        return ms
    r, s, q, tid, vals, cols = ms[0]
    assert (rep.kind, rep.row) == (khip.WITNESS_LOOKUP, r), (rep.kind, rep.row, ms[0])
    assert (lk.pattern, lk.slot, lk.ncells, list(lk.cols)[:lk.ncells]) == (q, s, len(cols), cols), ((lk.pattern, lk.slot, lk.ncells, list(lk.cols)), ms[0])
    assert list(lk.table_id) == [int(x) for x in F.limbs(tid)]
    for k, v in enumerate(vals):
        assert list(lk.entry[k]) == [int(x) for x in F.limbs(v)], k
    return ms


# ---------------------------------------------------------------------------------------------------------------- circuits
def fixed_case(Fo=Fo):
    """509 Lookup rows (domain 2^9, L = 508: row 507 is the last checked row, row 508 is not checked) into two tables with the same first two columns:
    id 5 of width 2, id 9 of width 4 whose columns 2 and 3 are non-zero on some rows -- those rows can never be looked up"""
    ent = 40
    c0 = [7 * j + 1 for j in range(ent)]; c1 = [j * j + 3 for j in range(ent)]
    c2 = [0] * ent
    c3 = [(j + 1) if j % 3 == 0 else 0 for j in range(ent)]               # rows 0, 3, 6, ..: a non-zero tail
    c2[4] = 77                                                             # (column 2 belongs to the key: (9, c0, c1) of row 4 is not in the table either)
    tables = [{"id": 5, "data": [c0, c1]}, {"id": 9, "data": [c0, c1, c2, c3]}]
    rows = 509
    gates = [CC.gate("Lookup", r) for r in range(rows)]
    wit = [[0] * rows for _ in range(15)]
    for r in range(rows):
        tid = 5 if r % 3 else 9
        wit[0][r] = tid
        for k in range(3):
            j = (5 * r + 7 * k) % ent
            if tid == 9:
                j = [1, 2, 5, 7, 8, 10][(r + k) % 6]                       # rows of table 9 with a zero tail
            wit[1 + 2 * k][r], wit[2 + 2 * k][r] = c0[j], c1[j]
    case = Case(gates, wit, tables, Fo=Fo)
    assert case.n == 512 and case.zk == 3 and len(case.L.table_cols) == 4 and case.L.table_ids is not None
    return case


def no_id_case():
    """one table with id 0: the index has no table-id column"""
    c0 = [0] + [3 * j + 2 for j in range(1, 30)]; c1 = [0] + [j + 100 for j in range(1, 30)]
    rows = 100
    wit = [[0] * rows for _ in range(15)]
    for r in range(rows):
        for k in range(3):
            j = (r + 11 * k) % 30
            wit[1 + 2 * k][r], wit[2 + 2 * k][r] = c0[j], c1[j]
    case = Case([CC.gate("Lookup", r) for r in range(rows)], wit, [{"id": 0, "data": [c0, c1]}])
    assert case.n == 128 and case.L.table_ids is None
    return case


def xor_case(Fo=Fo):
    """rows 0..9 Zero, a 64-bit xor from row 10 (four Xor16 rows and its zero row), row 15 a Zero row whose cell 0 is wired to cell (11, 3): 2^9"""
    a, b = 0x0123456789abcdef, 0xfedcba9876543210 ^ 0x1111
    xw = G.xor_witness(Fo, a, b, 64)
    gates = [CC.gate("Zero", r) for r in range(10)] + [CC.gate("Xor16", 10 + i) for i in range(4)] + [CC.gate("Zero", 14), CC.gate("Zero", 15)]
    CC.connect_cell_pair(gates, (11, 3), (15, 0))
    rows = [[0] * 15 for _ in range(10)] + [list(r) for r in xw] + [[0] * 15]
    rows[15][0] = rows[11][3]
    case = Case(gates, [[r[c] for r in rows] for c in range(15)], Fo=Fo)
    assert case.n == 512 and case.L.info.patterns == ["Xor"]
    return case


def range_case(Fo=Fo):
    """RangeCheck0, RangeCheck1, Rot64, ForeignFieldMul, Xor16 and Generic rows at 2^13: the 4096-entry table with id 1, the XOR table, the table-id
    column and thousands of padding rows.  The looked-up cells hold table values; the gates themselves are not satisfied (only the lookups are asked for)."""
    import random
    rnd = random.Random(8)
    order = ["Generic", "RangeCheck0", "RangeCheck1", "Zero", "Rot64", "RangeCheck0", "ForeignFieldMul", "Zero", "Xor16", "Generic"] * 4
    gates = []
    for r, t in enumerate(order):
        co = CC.generic_spec(Fo.p, "Add") + CC.generic_spec(Fo.p, "Mul") if t == "Generic" else [rnd.randrange(1, 1 << 60) for _ in range(4)] if t not in ("Zero", "Xor16") else []
        gates.append(CC.gate(t, r, co))
    info = OL.LookupInfo(order)
    pats = info.pattern_by_row(order)
    wit = [[rnd.randrange(1, 1 << 20) for _ in order] for _ in range(15)]
    for r in range(len(order)):
        if pats[r] in ("RangeCheck", "ForeignFieldMul"):
            for c in (range(3, 7) if pats[r] == "RangeCheck" else range(7, 11)):
                wit[c][r] = rnd.randrange(1 << 12)
        elif pats[r] == "Xor":
            for k in range(4):
                x, y = rnd.randrange(16), rnd.randrange(16)
                wit[3 + k][r], wit[7 + k][r], wit[11 + k][r] = x, y, x ^ y
    case = Case(gates, wit, Fo=Fo)
    assert case.n == 1 << 13 and case.L.info.patterns == ["Xor", "RangeCheck", "ForeignFieldMul"] and case.L.table_ids is not None
    return case


def runtime_case(Fo=Fo):
    """kimchi/src/tests/lookup.rs::test_runtime_table's shape: 20 Lookup rows into five runtime tables, ids 1..5; the second column comes with the call"""
    first, data = [8, 9, 8, 7, 1], [0, 2, 3, 4, 5]
    cfg = [{"id": tid, "first_column": list(first)} for tid in range(1, 6)]
    wit = [[0] * 20 for _ in range(15)]
    for r in range(20):
        wit[0][r] = 1 + r % 5
        for k in range(3):
            idx = (r + 2 * k) % 5
            wit[1 + 2 * k][r], wit[2 + 2 * k][r] = first[idx], data[idx]
    return Case([CC.gate("Lookup", r) for r in range(20)], wit, runtime_cfg=cfg, runtime=data * 5, Fo=Fo)


# ---------------------------------------------------------------------------------------------------------------- the device side
@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


@pytest.fixture(scope="module")
def F(khip):
    from proof_systems_amd import prover
    return prover.Fld(khip.FP)


@pytest.fixture(scope="module")
def srs13(khip):
    return khip.Srs.create(khip.VESTA, 1 << 13)


def created(khip, F, srs, case):
    from proof_systems_amd import prover
    types, wires, co = case.records(khip, F)
    ix = prover.CreatedIndex(srs, types, wires, co, public=0, tables=case.tables or None, runtime_tables=case.runtime_cfg)
    assert ix.n == case.n and ix.zk_rows == case.zk
    return ix


def made(khip, F, srs13, build):
    case = build() if F.fid == khip.FP else build(P.Fq)
    assert case.Fo.p == F.p and srs13.curve == (khip.VESTA if F.fid == khip.FP else khip.PALLAS)
    ix = created(khip, F, srs13, case)
    return case, ix, case.limbs(F)


@pytest.fixture(scope="module")
def F_pallas(khip):
    from proof_systems_amd import prover
    return prover.Fld(khip.FQ)


@pytest.fixture(scope="module")
def srs13_pallas(khip):
    return khip.Srs.create(khip.PALLAS, 1 << 13)


def index_fixture(khip, F, srs13, build):
    case, ix, base = made(khip, F, srs13, build)
    yield case, ix, base
    ix.free()


@pytest.fixture(scope="module")
def fixed_pallas(khip, F_pallas, srs13_pallas):
    yield from index_fixture(khip, F_pallas, srs13_pallas, fixed_case)


@pytest.fixture(scope="module")
def ranged_pallas(khip, F_pallas, srs13_pallas):
    yield from index_fixture(khip, F_pallas, srs13_pallas, range_case)


@pytest.fixture(scope="module")
def xored_pallas(khip, F_pallas, srs13_pallas):
    yield from index_fixture(khip, F_pallas, srs13_pallas, xor_case)


@pytest.fixture(scope="module")
def runtimed_pallas(khip, F_pallas, srs13_pallas):
    yield from index_fixture(khip, F_pallas, srs13_pallas, runtime_case)


@pytest.fixture(scope="module")
def fixed(khip, F, srs13):
    case, ix, base = made(khip, F, srs13, fixed_case)
    yield case, ix, base
    ix.free()


@pytest.fixture(scope="module")
def ranged(khip, F, srs13):
    case, ix, base = made(khip, F, srs13, range_case)
    yield case, ix, base
    ix.free()


@pytest.fixture(scope="module")
def xored(khip, F, srs13):
    case, ix, base = made(khip, F, srs13, xor_case)
    yield case, ix, base
    ix.free()


@pytest.fixture(scope="module")
def runtimed(khip, F, srs13):
    case, ix, base = made(khip, F, srs13, runtime_case)
    yield case, ix, base
    ix.free()


@pytest.fixture(scope="module")
def library(khip, F, srs13):
    """the library-gate circuits of 2^7 and 2^8 rows (no lookup index), built anew"""
    yield from library_indexes(khip, F, srs13, Fo)


@pytest.fixture(scope="module")
def library_pallas(khip, F_pallas, srs13_pallas):
    yield from library_indexes(khip, F_pallas, srs13_pallas, P.Fq)


def library_indexes(khip, F, srs13, Fo):
    from proof_systems_amd import prover
    out = {}
    for logn in (7, 8):
        cs, wit = M.library_circuit(Fo, logn)
        rows = len(wit[0])
        gids = khip.gate_ids()
        types = [khip.GATE_ZERO if g["typ"] == "Zero" else gids[g["typ"]] for g in cs["gates"][:rows]]
        wires = np.array([g["wires"] for g in cs["gates"][:rows]], dtype=np.uint32).reshape(rows, 7, 2)
        co = np.stack([F.limbs_many([cs["coefficients"][c][r] for c in range(15)]) for r in range(rows)])
        out[logn] = (prover.CreatedIndex(srs13, types, wires, co), np.stack([F.limbs_many([v % Fo.p for v in col]) for col in wit]), types)
    yield out
    for ix, _w, _t in out.values():
        ix.free()


def patched(F, base, cells):
    limbs = base.copy()
    for (r, c), v in cells.items():
        limbs[c, r] = F.limbs(v % F.p)
    return limbs


def run(khip, F, case, ix, base, cells=None, runtime="own", flags=None):
    """spoil `cells`, call with KH_WITNESS_LOOKUPS alone (or `flags`), compare with the brute force; returns (report, lookup record, misses)"""
    cells = cells or {}
    rt = case.runtime if runtime == "own" else runtime
    rep, lk = khip.witness_check_full(ix.native, patched(F, base, cells), runtime=F.limbs_many([v % F.p for v in rt]) if rt is not None else None,
                                      flags=khip.WITNESS_LOOKUPS if flags is None else flags)
    ms = expect(khip, F, case, rep, lk, case.spoiled(cells), rt) if flags is None else None
    return rep, lk, ms


# ---- 1. fixed tables, the Lookup pattern: entry, id, tail, several rows, wave boundaries, the last row
def test_fixed_tables_entries_ids_and_tails(khip, F, fixed):
    fixed_tables_entries_ids_and_tails_body(khip, F, fixed)


def test_fixed_tables_entries_ids_and_tails_on_pallas(khip, F_pallas, fixed_pallas):
    fixed_tables_entries_ids_and_tails_body(khip, F_pallas, fixed_pallas)


def fixed_tables_entries_ids_and_tails_body(khip, F, fixed):
    case, ix, base = fixed
    Fo = case.Fo
    rep, lk, ms = run(khip, F, case, ix, base)
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0 and not ms
    w = case.wit
    r5 = next(r for r in range(20, 500) if w[0][r] == 5)
    r9 = next(r for r in range(20, 500) if w[0][r] == 9)
    c0, c1, c3 = case.tables[1]["data"][0], case.tables[1]["data"][1], case.tables[1]["data"][3]
    # an entry cell: the second joint lookup (columns 3, 4) of a row
    rep, lk, ms = run(khip, F, case, ix, base, {(r5, 4): w[4][r5] + 1})
    assert ms == [(r5, 1, 1, 5, [w[3][r5], (w[4][r5] + 1) % Fo.p], [3, 4])]
    # the id cell to an unknown id: all three lookups of the row miss, the first is reported
    rep, lk, ms = run(khip, F, case, ix, base, {(r9, 0): 6})
    assert [m[:2] for m in ms] == [(r9, 0), (r9, 1), (r9, 2)] and lk.lookups_missing == 3
    # the id cell to the other table's id.  9 -> 5: table 5 has the same entries, still satisfied
    rep, lk, ms = run(khip, F, case, ix, base, {(r9, 0): 5})
    assert rep.kind == khip.WITNESS_OK and not ms
    # 5 -> 9 on a row that looks up entry j: in table 9 exactly when row j of it has a zero tail and a zero column 2
    js = [[j for j in range(40) if (c0[j], c1[j]) == (w[1 + 2 * k][r5], w[2 + 2 * k][r5])][0] for k in range(3)]
    rep, lk, ms = run(khip, F, case, ix, base, {(r5, 0): 9})
    assert [m[1] for m in ms] == [k for k in range(3) if c3[js[k]] or js[k] == 4]
    # a cell that matches a row of table 9 with a non-zero tail (row 3: column 3 holds 4) and nothing else
    assert c3[3] == 4
    rep, lk, ms = run(khip, F, case, ix, base, {(r9, 1): c0[3], (r9, 2): c1[3]})
    assert [m[:2] for m in ms] == [(r9, 0)]
    # ... while the same entry under id 5 is in the table
    rep, lk, ms = run(khip, F, case, ix, base, {(r5, 1): c0[3], (r5, 2): c1[3]})
    assert not ms
    # the key includes column 2: row 4 of table 9 is (c0, c1, 77, 0) -- a two-cell lookup of (c0, c1) misses it
    rep, lk, ms = run(khip, F, case, ix, base, {(r9, 5): c0[4], (r9, 6): c1[4]})
    assert [m[:2] for m in ms] == [(r9, 2)]


def test_fixed_tables_lowest_row_and_slot_counts_and_boundaries(khip, F, fixed):
    fixed_tables_lowest_row_and_slot_counts_and_boundaries_body(khip, F, fixed)


def test_fixed_tables_lowest_row_and_slot_counts_and_boundaries_on_pallas(khip, F_pallas, fixed_pallas):
    fixed_tables_lowest_row_and_slot_counts_and_boundaries_body(khip, F_pallas, fixed_pallas)


def fixed_tables_lowest_row_and_slot_counts_and_boundaries_body(khip, F, fixed):
    case, ix, base = fixed
    w, lim = case.wit, case.n - case.zk - 1
    assert lim == 508 and case.rows == 509
    bump = lambda r, c: {(r, c): w[c][r] + 1}
    # several rows at once, in different waves and blocks: the lowest row, within it the lowest joint lookup, the exact count
    cells = {}
    for r, c in ((300, 2), (70, 5), (70, 3), (450, 1), (129, 6)):
        cells.update(bump(r, c))
    rep, lk, ms = run(khip, F, case, ix, base, cells)
    assert (rep.row, lk.slot, lk.lookups_missing) == (70, 1, 5)
    # wave boundaries (64 rows), the block boundary (256 rows) and the last checked row, each alone
    for r in (0, 63, 64, 127, 128, 255, 256, lim - 1):
        rep, lk, ms = run(khip, F, case, ix, base, bump(r, 1))
        assert (rep.kind, rep.row, lk.slot, lk.lookups_missing) == (khip.WITNESS_LOOKUP, r, 0, 1), r
    # row L is a Lookup row of the gate list, but the lookup argument does not cover it
    rep, lk, ms = run(khip, F, case, ix, base, bump(lim, 1))
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0
    rep, lk, ms = run(khip, F, case, ix, base, {**bump(lim, 1), **bump(lim - 1, 6)})
    assert (rep.row, lk.slot, lk.lookups_missing) == (lim - 1, 2, 1)


# ---- 2. no table-id column: the id cell still counts
def test_without_an_id_column_an_unknown_table_id_is_reported(khip, F, srs13):
    case, ix, base = made(khip, F, srs13, no_id_case)
    assert ix.lookup.table_ids_comm is None
    rep, lk, ms = run(khip, F, case, ix, base)
    assert rep.kind == khip.WITNESS_OK
    rep, lk, ms = run(khip, F, case, ix, base, {(37, 0): 5})
    assert (rep.kind, rep.row, lk.pattern, lk.slot, lk.lookups_missing) == (khip.WITNESS_LOOKUP, 37, 1, 0, 3)
    assert list(lk.table_id) == [int(x) for x in F.limbs(5)]
    ix.free()


# ---- 3. the gate tables: Xor16 at 2^9, the range-check patterns at 2^13
def test_xor_table(khip, F, xored):
    xor_table_body(khip, F, xored)


def test_xor_table_on_pallas(khip, F_pallas, xored_pallas):
    xor_table_body(khip, F_pallas, xored_pallas)


def xor_table_body(khip, F, xored):
    case, ix, base = xored
    rep, lk, ms = run(khip, F, case, ix, base)
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0
    w = case.wit
    rep, lk, ms = run(khip, F, case, ix, base, {(12, 13): w[13][12] ^ 1})                     # an output nybble that is not the xor
    assert ms == [(12, 2, 0, 0, [w[5][12], w[9][12], w[13][12] ^ 1], [5, 9, 13])]
    rep, lk, ms = run(khip, F, case, ix, base, {(13, 3): 16})                                 # a nybble of 16
    assert [m[:2] for m in ms] == [(13, 0)]
    rep, lk, ms = run(khip, F, case, ix, base, {(14, 3): 1})                                  # the zero row carries no pattern
    assert not ms


def test_range_check_table_and_next_rows(khip, F, ranged):
    range_check_table_and_next_rows_body(khip, F, ranged)


def test_range_check_table_and_next_rows_on_pallas(khip, F_pallas, ranged_pallas):
    range_check_table_and_next_rows_body(khip, F_pallas, ranged_pallas)


def range_check_table_and_next_rows_body(khip, F, ranged):
    case, ix, base = ranged
    Fo = case.Fo
    order = [g["typ"] for g in case.gates]
    rep, lk, ms = run(khip, F, case, ix, base)
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0
    first = lambda t, k=0: [r for r, x in enumerate(order) if x == t][k]
    for typ, col in (("RangeCheck0", 4), ("Rot64", 6), ("RangeCheck1", 3), ("ForeignFieldMul", 10)):
        r = first(typ, 1)
        rep, lk, ms = run(khip, F, case, ix, base, {(r, col): 4096})                          # the first value that is not a 12-bit limb
        assert len(ms) == 1 and ms[0][0] == r and ms[0][5] == [col] and ms[0][3] == 1 and lk.pattern == (3 if typ == "ForeignFieldMul" else 2), (typ, ms)
        rep, lk, ms = run(khip, F, case, ix, base, {(r, col): 4095})
        assert not ms
    # the `next` rows of RangeCheck1 and ForeignFieldMul are Zero rows of the gate list that carry the pattern
    r1, rf = first("RangeCheck1", 2) + 1, first("ForeignFieldMul", 2) + 1
    assert order[r1] == order[rf] == "Zero"
    rep, lk, ms = run(khip, F, case, ix, base, {(r1, 5): 4096})
    assert [(m[0], m[1], m[2]) for m in ms] == [(r1, 2, 2)]
    rep, lk, ms = run(khip, F, case, ix, base, {(rf, 8): Fo.p - 1})
    assert [(m[0], m[1], m[2]) for m in ms] == [(rf, 1, 3)]
    rep, lk, ms = run(khip, F, case, ix, base, {(rf, 3): 4096, (r1, 7): 4096})               # cells their patterns do not read
    assert not ms
    # the Xor16 rows of the same circuit look up into the XOR table (id 0) next to the range-check table (id 1): 5 is a 12-bit limb, not a nybble pair
    rx = first("Xor16", 3)
    rep, lk, ms = run(khip, F, case, ix, base, {(rx, 4): 5, (rx, 8): 17, (rx, 12): 0})
    assert [(m[0], m[1], m[2], m[3]) for m in ms] == [(rx, 1, 0, 0)]


def test_two_patterns_on_one_row_count_separately(khip, F, srs13):
    """ForeignFieldMul's `next` row is an Xor16 row: both selectors are 1 there, and joint lookup s of both patterns is checked and counted"""
    def build():
        gates = [CC.gate("ForeignFieldMul", 0, [1, 2, 3, 4]), CC.gate("Xor16", 1), CC.gate("Zero", 2), CC.gate("Zero", 3)]
        wit = [[0] * 4 for _ in range(15)]
        for c in range(7, 11):
            wit[c][0] = 100 + c
        return Case(gates, wit)
    case, ix, base = made(khip, F, srs13, build)
    assert case.L.selectors["Xor"][1] == 1 and case.L.selectors["ForeignFieldMul"][1] == 1
    rep, lk, ms = run(khip, F, case, ix, base)
    assert rep.kind == khip.WITNESS_OK
    # cell (1, 8) is read by Xor as part of (w4, w8, w12) and by ForeignFieldMul alone: 16 is a 12-bit limb, not a nybble
    rep, lk, ms = run(khip, F, case, ix, base, {(1, 8): 16})
    assert [(m[0], m[1], m[2]) for m in ms] == [(1, 1, 0)]
    # 4096 is neither: joint lookup 1 of both patterns misses; the lower pattern id is reported, both are counted
    rep, lk, ms = run(khip, F, case, ix, base, {(1, 8): 4096})
    assert [(m[0], m[1], m[2]) for m in ms] == [(1, 1, 0), (1, 1, 3)] and (lk.pattern, lk.lookups_missing) == (0, 2)
    ix.free()


# ---- 4. runtime tables
def test_runtime_tables(khip, F, runtimed):
    runtime_tables_body(khip, F, runtimed)


def test_runtime_tables_on_pallas(khip, F_pallas, runtimed_pallas):
    runtime_tables_body(khip, F_pallas, runtimed_pallas)


def runtime_tables_body(khip, F, runtimed):
    case, ix, base = runtimed
    Fo = case.Fo
    rep, lk, ms = run(khip, F, case, ix, base)
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0
    # the same witness against another runtime vector: entry 1 of table 3 changes, the rows that look up (3, 9, 2) miss
    other = list(case.runtime); other[2 * 5 + 1] = 6
    rep, lk, ms = run(khip, F, case, ix, base, runtime=other)
    hits = [(r, k) for r in range(20) for k in range(3) if case.wit[0][r] == 3 and (case.wit[1 + 2 * k][r], case.wit[2 + 2 * k][r]) == (9, 2)]
    assert hits and [m[:2] for m in ms] == hits and rep.row == hits[0][0]
    # ... and a witness that looks up the new value passes with it, and only with it
    r, k = hits[0]
    rep, lk, ms = run(khip, F, case, ix, base, {(r, 2 + 2 * k): 6}, runtime=other)
    assert [m[:2] for m in ms] == hits[1:]
    rep, lk, ms = run(khip, F, case, ix, base, {(r, 2 + 2 * k): 6})
    assert [m[:2] for m in ms] == [hits[0]]
    # all zeros as runtime values: what the fixed second column holds; every lookup of a non-zero second value misses
    rep, lk, ms = run(khip, F, case, ix, base, runtime=[0] * 25)
    assert len(ms) == sum(1 for r in range(20) for k in range(3) if case.wit[2 + 2 * k][r])
    # a wrong number of runtime values, none at all, a value that is not reduced
    w = patched(F, base, {})
    for rt in (F.limbs_many(case.runtime[:24]), F.limbs_many(case.runtime + [1]), None):
        with pytest.raises(khip.KhError, match="RuntimeTablesInconsistent"):
            khip.witness_check_full(ix.native, w, runtime=rt, flags=khip.WITNESS_LOOKUPS)
    big = F.limbs_many(case.runtime); big[7] = np.frombuffer(Fo.p.to_bytes(32, "little"), dtype=np.uint64)
    with pytest.raises(khip.KhError, match="runtime value 7"):
        khip.witness_check_full(ix.native, w, runtime=big, flags=khip.WITNESS_LOOKUPS)
    # without the flag the runtime arguments are not read
    rep, lk = khip.witness_check_full(ix.native, w, runtime=None, flags=khip.WITNESS_GATES | khip.WITNESS_WIRES)
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0


# ---- 5. order across kinds
def test_order_across_kinds(khip, F, xored):
    case, ix, base = xored
    w = case.wit
    G_, W_, L_ = khip.WITNESS_GATES, khip.WITNESS_WIRES, khip.WITNESS_LOOKUPS
    assert run(khip, F, case, ix, base, flags=G_ | W_ | L_)[0].kind == khip.WITNESS_OK
    # cell (11, 3) is wired to (15, 0), is a nybble of row 11's decomposition and the first cell of its first lookup: + 16 breaks all three
    cells = {(11, 3): w[3][11] + 16}
    rep, lk, _ = run(khip, F, case, ix, base, cells, flags=G_ | W_ | L_)
    assert (rep.kind, rep.row, rep.col, rep.wired_row, rep.wired_col) == (khip.WITNESS_DISCONNECTED, 11, 3, 15, 0)
    assert (rep.gate_rows_violated, rep.cells_disconnected, lk.lookups_missing, lk.pattern) == (1, 2, 1, -1)
    rep, lk, _ = run(khip, F, case, ix, base, cells, flags=G_ | L_)
    assert (rep.kind, rep.row, rep.gate, rep.constraints) == (khip.WITNESS_GATE, 11, khip.gate_ids()["Xor16"], 1) and (lk.lookups_missing, lk.pattern) == (1, -1)
    rep, lk, _ = run(khip, F, case, ix, base, cells, flags=L_)
    assert (rep.kind, rep.row, lk.pattern, lk.slot, lk.ncells, list(lk.cols)) == (khip.WITNESS_LOOKUP, 11, 0, 0, 3, [3, 7, 11])
    assert (rep.gate_rows_violated, rep.cells_disconnected) == (0, 0)
    rep, lk, _ = run(khip, F, case, ix, base, cells, flags=W_ | L_)
    assert rep.kind == khip.WITNESS_DISCONNECTED
    # row 10 starts the chain: an output nybble off by one with the output value moved along satisfies the gate and misses the XOR table;
    # a nybble of row 11 off by one violates row 11's gate (and its lookup).  The miss on row 10 comes first
    d = (w[11][10] ^ 1) - w[11][10]
    cells = {(10, 11): w[11][10] ^ 1, (10, 2): w[2][10] + d, (11, 9): w[9][11] ^ 1}
    rep, lk, _ = run(khip, F, case, ix, base, cells, flags=G_ | L_)
    assert (rep.kind, rep.row, lk.pattern, lk.slot) == (khip.WITNESS_LOOKUP, 10, 0, 0)
    assert (rep.gate_rows_violated, lk.lookups_missing) == (1, 2)
    rep, lk, _ = run(khip, F, case, ix, base, cells, flags=G_)
    assert (rep.kind, rep.row) == (khip.WITNESS_GATE, 11)


# ---- 6. device witness = host witness; an attached index = the created one
def test_device_witness_and_attached_index(khip, F, srs13, fixed):
    from proof_systems_amd import prover, lookup as LK
    case, ix, base = fixed
    types, wires, co = case.records(khip, F)
    pix = prover.ProverIndex(khip.VESTA, case.cs["log2_n"], co, srs=srs13, gate_types=[g["typ"] for g in case.gates], public=0, zk_rows=case.zk)
    pix.set_wiring(wires.tolist())
    pix.attach_lookup(LK.LookupIndex(pix.fid, case.cs["gate_types"], list(case.tables), case.cs["log2_n"], case.zk, runtime_tables=None))
    nat = prover.native_index(pix)
    n = case.n
    buf = khip.DevBuf(15 * n * 32)
    rnd = np.random.default_rng(3)
    fields = lambda rep, lk: ((rep.kind, rep.row, rep.gate, rep.constraints, rep.col, rep.wired_row, rep.wired_col, rep.gate_rows_violated, rep.cells_disconnected),
                              (lk.pattern, lk.slot, lk.ncells, list(lk.cols), list(lk.table_id), [list(e) for e in lk.entry], lk.lookups_missing))
    flags = khip.WITNESS_GATES | khip.WITNESS_LOOKUPS
    for cells in ({}, {(200, 3): 12345, (77, 6): 1}, {(507, 0): 77}):
        host = patched(F, base, cells)
        want = fields(*khip.witness_check_full(ix.native, host, flags=flags))
        ms = case.misses(case.spoiled(cells))
        assert want[1][6] == len(ms) and (want[0][0], want[0][1]) == ((khip.WITNESS_LOOKUP, ms[0][0]) if ms else (khip.WITNESS_OK, 0))
        cols = np.zeros((15, n, 4), dtype=np.uint64)
        cols[:, :host.shape[1]] = host
        lim = rnd.integers(0, 1 << 62, size=(15, case.zk, 4), dtype=np.uint64)              # the zero-knowledge rows hold anything
        cols[:, n - case.zk:] = lim
        buf.upload(cols)
        assert fields(*khip.witness_check_full(ix.native, witness_dev=buf, flags=flags)) == want
        assert fields(*khip.witness_check_full(nat, host, flags=flags)) == want
        assert fields(*khip.witness_check_full(nat, witness_dev=buf, flags=flags)) == want
    rep = pix.check_witness(patched(F, base, {(77, 6): 1}), lookups=True)
    assert not rep and rep.kind == "lookup" and rep.row == 77 and rep.lookup["pattern"] == "Lookup" and rep.lookup["cols"] == [5, 6] and rep.lookups_missing == 1
    assert ix.check_witness(base, lookups=True).ok
    buf.free()
    pix.free_lookup(); pix.free()


# ---- 7. agreement with the prover
def test_agrees_with_the_prover(khip, F, fixed):
    agrees_with_the_prover_body(khip, F, fixed)


def test_agrees_with_the_prover_on_pallas(khip, F_pallas, fixed_pallas):
    agrees_with_the_prover_body(khip, F_pallas, fixed_pallas)


def agrees_with_the_prover_body(khip, F, fixed):
    from proof_systems_amd import prover
    case, ix, base = fixed
    rng = lambda: V.RefRng(P.StdRng(bytes([5] * 32)))
    rep, lk, ms = run(khip, F, case, ix, base)
    assert rep.kind == khip.WITNESS_OK
    prover.create_proof_native(ix, base, rng(), check=True)
    for r, c in ((3, 1), (200, 4), (507, 5)):
        cells = {(r, c): case.wit[c][r] + 1}
        rep, lk, ms = run(khip, F, case, ix, base, cells)
        assert rep.row == r and lk.lookups_missing == 1
        with pytest.raises(khip.KhError, match=r"lookup in row %d \(" % r):
            prover.create_proof_native(ix, patched(F, base, cells), rng(), check=True)


# ---- 8. refusals and messages
def test_refusals_leave_the_outputs_untouched(khip, F, fixed, runtimed, library):
    case, ix, base = fixed
    rcase, rix, rbase = runtimed
    plain = library[7][0]
    lib = khip.raw()
    u64p = C.POINTER(C.c_uint64)
    rep = khip.WitnessReportC(kind=99, row=12345)
    lk = khip.WitnessLookupC(pattern=42, slot=7, lookups_missing=999)
    wp, rows = base.ctypes.data_as(u64p), base.shape[1]
    rwp, rrows = rbase.ctypes.data_as(u64p), rbase.shape[1]
    pw = library[7][1]
    rt = F.limbs_many(rcase.runtime)
    rtp = rt.ctypes.data_as(u64p)
    big = rt.copy(); big[0] = np.frombuffer(Fo.p.to_bytes(32, "little"), dtype=np.uint64)
    buf = khip.DevBuf(15 * case.n * 32)
    R, K = C.byref(rep), C.byref(lk)
    for what, args in (
            ("lookups on an index without a lookup index", (plain.native._h, pw.ctypes.data_as(u64p), pw.shape[1], None, None, 0, 4, R, K)),
            ("lookup_out NULL", (ix.native._h, wp, rows, None, None, 0, 4, R, None)),
            ("out NULL", (ix.native._h, wp, rows, None, None, 0, 4, None, K)),
            ("one runtime value too few", (rix.native._h, rwp, rrows, None, rtp, 24, 4, R, K)),
            ("no runtime values", (rix.native._h, rwp, rrows, None, None, 0, 4, R, K)),
            ("runtime values without runtime tables", (ix.native._h, wp, rows, None, rtp, 25, 4, R, K)),
            ("a runtime value = p", (rix.native._h, rwp, rrows, None, big.ctypes.data_as(u64p), 25, 4, R, K)),
            ("flags 0", (ix.native._h, wp, rows, None, None, 0, 0, R, K)),
            ("an unknown flag", (ix.native._h, wp, rows, None, None, 0, 8, R, K)),
            ("both witnesses", (ix.native._h, wp, rows, C.c_void_p(buf.ptr), None, 0, 4, R, K)),
            ("no witness", (ix.native._h, None, 0, None, None, 0, 4, R, K)),
            ("no index", (None, wp, rows, None, None, 0, 4, R, K))):
        assert lib.kh_witness_check_full(*args) == -1 and lib.kh_last_error(), what
        assert (rep.kind, rep.row, lk.pattern, lk.slot, lk.lookups_missing) == (99, 12345, 42, 7, 999), what
    assert lib.kh_witness_check(ix.native._h, wp, rows, None, 4, R) == -1 and rep.kind == 99                  # the old entry point does not take the flag
    buf.free()


def test_messages(khip, F, ranged, fixed):
    case, ix, base = ranged
    order = [g["typ"] for g in case.gates]
    r = [q for q, t in enumerate(order) if t == "RangeCheck0"][2]
    rep, lk, ms = run(khip, F, case, ix, base, {(r, 5): 4096})
    msg = khip.witness_lookup_message(rep, lk)
    assert msg == "row %d: lookup 2 of pattern RangeCheck (column 5), table id 1: the value is not in the table (1 lookup missing)" % r
    assert khip.witness_report_message(rep) == "row %d: a looked-up value is in no table (kh_witness_lookup_message names it)" % r
    rep2, lk2, _ = run(khip, F, case, ix, base)
    assert khip.witness_lookup_message(rep2, lk2) == "the witness satisfies the circuit"
    fcase, fix, fbase = fixed
    rep3, lk3, _ = run(khip, F, fcase, fix, fbase, {(37, 0): 6, (40, 0): 6})
    assert khip.witness_lookup_message(rep3, lk3) == "row 37: lookup 0 of pattern Lookup (columns 1, 2), table id 6: the value is not in the table (6 lookups missing)"
    # truncation: NUL-terminated inside cap, the return value is the whole length
    lib = khip.raw()
    buf = C.create_string_buffer(b"\xff" * 32, 32)
    full = lib.kh_witness_lookup_message(C.byref(rep), C.byref(lk), buf, C.c_size_t(10))
    assert full == len(msg) and buf.raw[:10] == msg[:9].encode() + b"\0" and buf.raw[10:] == b"\xff" * 22
    assert lib.kh_witness_lookup_message(C.byref(rep), C.byref(lk), None, C.c_size_t(0)) == len(msg)
    assert lib.kh_witness_lookup_message(None, C.byref(lk), buf, C.c_size_t(10)) == -1
    assert lib.kh_witness_lookup_message(C.byref(rep), None, buf, C.c_size_t(10)) == -1


# ---- 9. gates and wires through the new entry point = kh_witness_check
def test_gates_and_wires_equal_the_old_entry_point(khip, F, library):
    gates_and_wires_equal_the_old_entry_point_body(khip, F, library)


def test_gates_and_wires_equal_the_old_entry_point_on_pallas(khip, F_pallas, library_pallas):
    gates_and_wires_equal_the_old_entry_point_body(khip, F_pallas, library_pallas)


def gates_and_wires_equal_the_old_entry_point_body(khip, F, library):
    fields = lambda rep: (rep.kind, rep.row, rep.gate, rep.constraints, rep.col, rep.wired_row, rep.wired_col, rep.gate_rows_violated, rep.cells_disconnected)
    for logn in (7, 8):
        ix, w, types = library[logn]
        live = [r for r, t in enumerate(types) if t != khip.GATE_ZERO]
        variants = [w]
        for r in (live[1], live[len(live) // 2], live[-1]):
            v = w.copy(); v[0, r] = F.limbs(123456789); variants.append(v)
        kinds = set()
        for v in variants:
            for flags in (1, 2, 3):
                old = khip.witness_check(ix.native, v, flags=flags)
                new, lk = khip.witness_check_full(ix.native, v, flags=flags)
                assert fields(new) == fields(old), (logn, flags)
                assert (lk.pattern, lk.slot, lk.ncells, lk.lookups_missing) == (-1, -1, 0, 0)
                kinds.add(old.kind)
        assert {khip.WITNESS_OK, khip.WITNESS_GATE} <= kinds, kinds


# ---- 10. forced collisions: every table tuple's home slot is 1022 or 1023 of 1024 (domain 2^9, L = 508)
LIM, CAP = 508, 1024
LAST_TWO = (CAP - 2, CAP - 1)
TAIL_THEN_PLAIN, PLAIN_THEN_TAIL = 40, 70                         # entries of table 9 that stand next to a copy of themselves with a non-zero tail
RT_POOL = (17, 4242, 99)                                          # the runtime table's values: three values, each many times


def entry(x):
    return (x, x * x + 3)


def colliding_case(Fo=Fo):
    """509 Lookup rows into two fixed tables, id 5 of width 2 and id 9 of width 4, 100 + 103 entries: x = 1, 2, .. kept when (id, x, x^2 + 3, 0) has its
    home slot in the last two.  Table 9 also holds, for the predecessor rule of k_witness_lookup_build (a row equal to its predecessor in id and columns
    0..2 is skipped -- unless that predecessor has a non-zero tail and was never inserted):
      entry 40 preceded by a copy with tail 11   the copy is not inserted, so entry 40 must insert itself
      entry 70 followed by a copy with tail 12   the copy is not inserted, entry 70 is
      one more colliding entry with tail 5 alone: never in the set
    Every entry with a zero tail is looked up by a checked row of the sound witness."""
    x5 = LC.tuple_colliders(Fo, 5, LIM, LAST_TWO, 100)
    x9 = LC.tuple_colliders(Fo, 9, LIM, LAST_TWO, 101)
    x9, lone = x9[:100], x9[100]
    rows9 = []
    for j, x in enumerate(x9):
        if j == TAIL_THEN_PLAIN:
            rows9.append(entry(x) + (0, 11))
        rows9.append(entry(x) + (0, 0))
        if j == PLAIN_THEN_TAIL:
            rows9.append(entry(x) + (0, 12))
    rows9.append(entry(lone) + (0, 5))
    tables = [{"id": 5, "data": [list(x5), [entry(x)[1] for x in x5]]}, {"id": 9, "data": [list(c) for c in zip(*rows9)]}]
    rows = 509
    wit = [[0] * rows for _ in range(15)]
    for r in range(rows):
        tid, xs = (9, x9) if r % 3 == 0 else (5, x5)
        wit[0][r] = tid
        for k in range(3):
            wit[1 + 2 * k][r], wit[2 + 2 * k][r] = entry(xs[(3 * (r // 3 if tid == 9 else r) + k) % 100])
    case = Case([CC.gate("Lookup", r) for r in range(rows)], wit, tables, Fo=Fo)
    assert case.n == 512 and case.zk == 3 and len(case.L.table_cols) == 4 and case.L.table_ids is not None
    looked = {(wit[0][r], wit[1 + 2 * k][r]) for r in range(LIM) for k in range(3)}
    assert looked == {(5, x) for x in x5} | {(9, x) for x in x9}
    case.x5, case.x9, case.lone = x5, x9, lone
    return case


def colliding_runtime_case(Fo=Fo):
    """300 Lookup rows: even rows into a fixed table id 5 (80 colliding entries), odd rows into a runtime table id 7 of 120 entries whose second column --
    the call's runtime values -- holds three values only; its first column is x = 1, 2, .. kept when (7, x, RT_POOL[x % 3], 0) collides"""
    x5 = LC.tuple_colliders(Fo, 5, LIM, LAST_TWO, 80)
    first = LC.tuple_colliders(Fo, 7, LIM, LAST_TWO, 120, entry=lambda x: (x, RT_POOL[x % 3], 0))
    runtime = [RT_POOL[x % 3] for x in first]
    assert all(runtime.count(v) >= 20 for v in RT_POOL)
    rows = 300
    wit = [[0] * rows for _ in range(15)]
    for r in range(rows):
        wit[0][r] = 7 if r % 2 else 5
        for k in range(3):
            j = 3 * (r // 2) + k
            wit[1 + 2 * k][r], wit[2 + 2 * k][r] = (first[j % 120], runtime[j % 120]) if r % 2 else entry(x5[j % 80])
    case = Case([CC.gate("Lookup", r) for r in range(rows)], wit, [{"id": 5, "data": [list(x5), [entry(x)[1] for x in x5]]}],
                runtime_cfg=[{"id": 7, "first_column": list(first)}], runtime=runtime, Fo=Fo)
    assert case.n == 512 and case.zk == 3
    case.x5, case.first = x5, first
    return case


def chain_of(case):
    """the preconditions, on the table the index really has: the oracle's table_cols / table_ids over all L rows (column 1 of the runtime rows = the
    call's values), the rows k_witness_lookup_build inserts (a zero tail), their distinct (id, c0, c1, c2), the mirror's home slots.  Every home is one
    of the last two slots -- but the all-zero tuple of the padding rows, whose hash is 0: slot 0, inside the chain --; the occupied slots are ONE run across
    the end of the array; the key in its last slot is displaced by tuples - 3 at least (three home slots).  Returns the run."""
    L, Fo = case.L, case.Fo
    assert case.n - case.zk - 1 == LIM and LC.slots(LIM) == CAP
    cols = [list(c) for c in L.table_cols]
    if case.runtime is not None:
        cols[1][L.runtime_offset:L.runtime_offset + len(case.runtime)] = [v % Fo.p for v in case.runtime]
    tuples = {}
    for t in range(LIM):
        if not any(c[t] for c in cols[3:]):
            tuples.setdefault((L.table_ids[t], cols[0][t], cols[1][t], cols[2][t] if len(cols) > 2 else 0))
    assert (0, 0, 0, 0) in tuples and L.entries < LIM
    homes = {tup: LC.tuple_home(*(LC.mont_limbs(Fo, v) for v in tup), LIM) for tup in tuples}
    assert homes.pop((0, 0, 0, 0)) == 0 and set(homes.values()) == set(LAST_TWO)
    run = LC.longest_run(list(homes.values()) + [0], CAP)
    assert len(tuples) >= 200 and len(run.slots) == len(tuples) and run.occupied == set(run.slots) and run.slots[0] == CAP - 2
    assert run.wraps and 0 in run.occupied and run.displacement >= len(tuples) - 3
    return run


def absent_cell(case, tid, x, second, slot):
    """v such that (tid, x, v, 0) is no table tuple and has its home in `slot`: the tuple of a row that looks (tid, x, second) up, ONE cell replaced"""
    v = LC.tuple_colliders(case.Fo, tid, LIM, {slot}, 1, exclude={second}, entry=lambda v: (x, v, 0))[0]
    assert (tid, x, v) + (0,) * (len(case.L.table_cols) - 2) not in case.table_set(case.runtime)
    return v


def thrice(khip, F, case, ix, base, cells=None, runtime="own"):
    """three runs of one call (the build's atomics arrive in another order each time), each against the brute force; returns the last"""
    for _ in range(3):
        out = run(khip, F, case, ix, base, cells, runtime)
    return out


@pytest.fixture(scope="module")
def colliding(khip, F, srs13):
    yield from index_fixture(khip, F, srs13, colliding_case)


@pytest.fixture(scope="module")
def colliding_pallas(khip, F_pallas, srs13_pallas):
    yield from index_fixture(khip, F_pallas, srs13_pallas, colliding_case)


@pytest.fixture(scope="module")
def colliding_rt(khip, F, srs13):
    yield from index_fixture(khip, F, srs13, colliding_runtime_case)


@pytest.fixture(scope="module")
def colliding_rt_pallas(khip, F_pallas, srs13_pallas):
    yield from index_fixture(khip, F_pallas, srs13_pallas, colliding_runtime_case)


def test_colliding_tables(khip, F, colliding):
    colliding_tables_body(khip, F, colliding)


def test_colliding_tables_on_pallas(khip, F_pallas, colliding_pallas):
    colliding_tables_body(khip, F_pallas, colliding_pallas)


def colliding_tables_body(khip, F, fixture):
    case, ix, base = fixture
    chain = chain_of(case)
    head = chain.slots[0]
    behind = chain.slots[chain.slots.index(CAP - 1) + 1:]
    mid = behind[len(behind) // 2]
    assert head == CAP - 2 and len(behind) >= 198 and 0 < mid < 250
    w = case.wit
    # the sound witness: every zero-tail entry of both tables is looked up, entry 40 and entry 70 of table 9 (the predecessor rule, both orders) among them
    rep, lk, ms = thrice(khip, F, case, ix, base)
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0 and not ms
    for j in (TAIL_THEN_PLAIN, PLAIN_THEN_TAIL):
        assert any(w[0][r] == 9 and w[1 + 2 * k][r] == case.x9[j] for r in range(LIM) for k in range(3))
    t9 = list(zip(*case.tables[1]["data"]))
    a, b = t9.index(entry(case.x9[TAIL_THEN_PLAIN]) + (0, 0)), t9.index(entry(case.x9[PLAIN_THEN_TAIL]) + (0, 0))
    assert t9[a - 1] == t9[a][:3] + (11,) and t9[b + 1] == t9[b][:3] + (12,)
    # the entry that exists with a non-zero tail only is in no lookup's reach
    r9 = next(r for r in range(20, 500) if w[0][r] == 9)
    rep, lk, ms = thrice(khip, F, case, ix, base, {(r9, 1): case.lone, (r9, 2): entry(case.lone)[1]})
    assert [m[:2] for m in ms] == [(r9, 0)]
    # one cell replaced, the tuple absent: home = the head of the chain (the probe walks all of it, the wrap included) / the middle behind the wrap
    r5 = next(r for r in range(200, 500) if w[0][r] == 5)
    for slot in (head, mid):
        v = absent_cell(case, 5, w[3][r5], w[4][r5], slot)
        rep, lk, ms = thrice(khip, F, case, ix, base, {(r5, 4): v})
        assert ms == [(r5, 1, 1, 5, [w[3][r5], v], [3, 4])], slot
        v = absent_cell(case, 9, w[5][r9], w[6][r9], slot)
        rep, lk, ms = thrice(khip, F, case, ix, base, {(r9, 6): v})
        assert ms == [(r9, 2, 1, 9, [w[5][r9], v], [5, 6])], slot
    # several misses in one wave (rows 64 .. 127), of both kinds: the lowest row and joint lookup, the exact count
    cells = {}
    for r, k, slot in ((100, 2, head), (71, 1, mid), (71, 2, head), (126, 0, mid), (64, 0, head)):
        cells[(r, 2 + 2 * k)] = absent_cell(case, w[0][r], w[1 + 2 * k][r], w[2 + 2 * k][r], slot)
    rep, lk, ms = thrice(khip, F, case, ix, base, cells)
    assert (rep.row, lk.slot, lk.lookups_missing) == (64, 0, 5) and [m[:2] for m in ms] == [(64, 0), (71, 1), (71, 2), (100, 2), (126, 0)]


def test_colliding_runtime_table(khip, F, colliding_rt):
    colliding_runtime_table_body(khip, F, colliding_rt)


def test_colliding_runtime_table_on_pallas(khip, F_pallas, colliding_rt_pallas):
    colliding_runtime_table_body(khip, F_pallas, colliding_rt_pallas)


def colliding_runtime_table_body(khip, F, fixture):
    case, ix, base = fixture
    chain = chain_of(case)
    head = chain.slots[0]
    behind = chain.slots[chain.slots.index(CAP - 1) + 1:]
    mid = behind[len(behind) // 2]
    w = case.wit
    rep, lk, ms = thrice(khip, F, case, ix, base)
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0 and not ms
    # a runtime row's value replaced by an absent one whose tuple starts at the head of the chain / in its middle; a fixed row likewise
    r7, r5 = 151, 150
    assert w[0][r7] == 7 and w[0][r5] == 5
    for slot in (head, mid):
        v = absent_cell(case, 7, w[1][r7], w[2][r7], slot)
        assert v not in RT_POOL
        rep, lk, ms = thrice(khip, F, case, ix, base, {(r7, 2): v})
        assert ms == [(r7, 0, 1, 7, [w[1][r7], v], [1, 2])], slot
        v = absent_cell(case, 5, w[3][r5], w[4][r5], slot)
        rep, lk, ms = thrice(khip, F, case, ix, base, {(r5, 4): v})
        assert ms == [(r5, 1, 1, 5, [w[3][r5], v], [3, 4])], slot
    # another of the three values for one entry: the tuple the witness looks up is gone (the new one need not collide: it takes any slot)
    other = list(case.runtime)
    j = 50
    other[j] = RT_POOL[(RT_POOL.index(other[j]) + 1) % 3]
    hits = [(r, k) for r in range(300) for k in range(3) if w[0][r] == 7 and w[1 + 2 * k][r] == case.first[j]]
    rep, lk, ms = thrice(khip, F, case, ix, base, runtime=other)
    assert hits and [m[:2] for m in ms] == hits and rep.row == hits[0][0]
    r, k = hits[0]
    rep, lk, ms = thrice(khip, F, case, ix, base, {(r, 2 + 2 * k): other[j]}, runtime=other)
    assert [m[:2] for m in ms] == hits[1:]
