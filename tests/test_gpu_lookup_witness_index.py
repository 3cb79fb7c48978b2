"""kh_lookup_witness_dev on a real index: where a table sits (kh_prover_index_lookup_table), a witness written by two calls from device inputs to
proof bytes with the runtime values in device memory (kh_witness_check_full_runtime_dev, kh_prove_full_runtime_dev), and KH_STEP_LOOKUP in a
witness schedule.

The circuit: 300 Lookup rows in a 2^9 domain -- even rows read the fixed table id 5 (width 2), odd rows the runtime table id 7 -- beside a second
fixed table id 9 of width 4 with the same first two columns, some of whose rows have a non-zero tail.  Expected values are the integers of the
brute force of test_gpu_witness_lookups.py (Case: the oracle's LookupCS and a Python set of table tuples); every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import circuit as CC
from oracle import pasta as P

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_witness_lookups import Case, expect  # noqa: E402

pytestmark = pytest.mark.gpu
ENT, RT, ROWS = 40, 20, 300


def lookup_circuit(Fo):
    c0 = [7 * j + 1 for j in range(ENT)]; c1 = [j * j + 3 for j in range(ENT)]
    c2 = [0] * ENT
    c3 = [(j + 1) if j % 3 == 0 else 0 for j in range(ENT)]               # rows 0, 3, 6, ..: a non-zero tail
    tables = [{"id": 5, "data": [c0, c1]}, {"id": 9, "data": [c0, c1, c2, c3]}]
    first = [1000 + 3 * j for j in range(RT)]
    runtime = [(j * j * 7 + 11) % Fo.p for j in range(RT)]
    wit = [[0] * ROWS for _ in range(15)]
    for r in range(ROWS):
        wit[0][r] = 7 if r % 2 else 5
        for k in range(3):
            j = (5 * r + 7 * k) % (RT if r % 2 else ENT)
            wit[1 + 2 * k][r], wit[2 + 2 * k][r] = (first[j], runtime[j]) if r % 2 else (c0[j], c1[j])
    case = Case([CC.gate("Lookup", r) for r in range(ROWS)], wit, tables, runtime_cfg=[{"id": 7, "first_column": first}], runtime=runtime, Fo=Fo)
    assert case.n == 512 and case.zk == 3 and len(case.L.table_cols) == 4
    return case


class Circuit:
    def __init__(self, khip, curve, Fo):
        from proof_systems_amd import prover
        self.khip, self.Fo = khip, Fo
        self.F = F = prover.Fld(khip.FP if curve == khip.VESTA else khip.FQ)
        self.srs = khip.Srs.create(curve, 1 << 9)
        self.case = case = lookup_circuit(Fo)
        self.records = case.records(khip, F)
        self.ix = prover.CreatedIndex(self.srs, *self.records, public=0, tables=case.tables, runtime_tables=case.runtime_cfg)
        self.nat, self.n = self.ix.native, case.n
        self.want = np.zeros((15, self.n, 4), dtype=np.uint64)            # the brute force's witness, padded with zeros to the domain
        self.want[:, :ROWS] = case.limbs(F)
        self.rt_dev = khip.DevBuf(32 * RT).upload(F.limbs_many(case.runtime))

    def tid(self, t):
        return self.F.limbs(t)

    def keys_dev(self, rows, wit=None):
        """the n x 3 keys of these rows of the brute force's witness, on the device"""
        w = self.case.wit if wit is None else wit
        return self.khip.DevBuf(96 * len(rows)).upload(self.F.limbs_many([w[1 + 2 * k][r] for r in rows for k in range(3)]))

    def write(self, wit, flags, rt_dev=None):
        """the witness by two calls: table 5 on the even rows, table 7 (its keys from the index, its values from the runtime buffer) on the odd rows"""
        K, fid = self.khip, self.F.fid
        t5, t7 = self.nat.lookup_table(5), self.nat.lookup_table(7)
        even, odd = list(range(0, ROWS, 2)), list(range(1, ROWS, 2))
        k5, k7 = self.keys_dev(even), self.keys_dev(odd)
        K.lookup_witness_dev(fid, self.tid(5), t5["keys"], t5["values"], t5["len"], k5, len(even), wit, self.n, self.n, row0=0, row_stride=2, flags=flags, bit=0)
        K.lookup_witness_dev(fid, self.tid(7), t7["keys"], (rt_dev or self.rt_dev).view(32 * t7["runtime_first"]), t7["len"], k7, len(odd), wit, self.n, self.n,
                             rows=odd, flags=flags, bit=1)
        k5.free(); k7.free()

    def free(self):
        self.rt_dev.free(); self.ix.free(); self.srs.close()


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


@pytest.fixture(scope="module")
def circ(khip):
    c = Circuit(khip, khip.VESTA, P.Fp)
    yield c
    c.free()


@pytest.fixture(scope="module")
def circ_pallas(khip):
    c = Circuit(khip, khip.PALLAS, P.Fq)
    yield c
    c.free()


def word(buf):
    return int(buf.download((1,), dtype=np.uint32)[0])


# ---- 5. kh_prover_index_lookup_table
def test_lookup_table_positions_and_columns(khip, circ):
    from proof_systems_amd import prover, lookup as LK
    case, F, nat, L = circ.case, circ.F, circ.nat, circ.case.L
    c0, c1 = case.tables[0]["data"]
    first = case.runtime_cfg[0]["first_column"]
    assert L.runtime_offset == 2 * ENT and L.runtime_tables == [(7, RT)]
    for tid, first_row, keys, values, is_rt in ((5, 0, c0, c1, False), (9, ENT, c0, c1, False), (7, L.runtime_offset, first, [0] * RT, True)):
        t = nat.lookup_table(tid)
        assert (t["first_row"], t["len"], t["is_runtime"], t["runtime_first"]) == (first_row, len(keys), is_rt, 0), tid
        got_k, got_v = np.zeros((len(keys), 4), np.uint64), np.zeros((len(keys), 4), np.uint64)
        khip.sync()
        for arr, view in ((got_k, t["keys"]), (got_v, t["values"])):
            assert khip.raw().kh_dev_download(arr.ctypes.data_as(C.c_void_p), C.c_void_p(view.ptr), arr.nbytes) == 0
        assert np.array_equal(got_k, F.limbs_many(keys)) and np.array_equal(got_v, F.limbs_many(values)), tid
        assert [L.table_cols[0][first_row + j] for j in range(len(keys))] == keys                # (the oracle's combined table has them there)
    # NULL outputs are skipped; an id the index has not, an attached index
    lib = khip.raw()
    ln = C.c_size_t(0)
    assert lib.kh_prover_index_lookup_table(nat._h, 9, None, C.byref(ln), None, None, None, None) == 0 and ln.value == ENT
    ln = C.c_size_t(77)
    assert lib.kh_prover_index_lookup_table(nat._h, 6, None, C.byref(ln), None, None, None, None) == khip.E_NOTFOUND and ln.value == 77
    assert nat.lookup_table(6) is None
    types, wires, co = circ.records
    pix = prover.ProverIndex(khip.VESTA, case.cs["log2_n"], co, srs=circ.srs, gate_types=[g["typ"] for g in case.gates], public=0, zk_rows=case.zk)
    pix.set_wiring(wires.tolist())
    pix.attach_lookup(LK.LookupIndex(pix.fid, case.cs["gate_types"], list(case.tables), case.cs["log2_n"], case.zk, runtime_tables=None))
    attached = prover.native_index(pix)
    assert lib.kh_prover_index_lookup_table(attached._h, 5, None, C.byref(ln), None, None, None, None) == khip.E_NOTFOUND and ln.value == 77
    assert attached.lookup_table(5) is None
    pix.free_lookup(); pix.free()


# ---- 6. end to end: device inputs to proof bytes
def end_to_end_body(khip, circ):
    case, F, nat, n = circ.case, circ.F, circ.nat, circ.n
    wit, flags = khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(4).zero()
    circ.write(wit, flags)
    got = wit.download((15, n, 4))
    assert word(flags) == 0
    assert np.array_equal(got, circ.want)
    rep, lk = nat.witness_check_full(witness_dev=wit, runtime_dev=(circ.rt_dev, RT))
    assert rep.kind == khip.WITNESS_OK and lk.lookups_missing == 0
    # the proof with the runtime values on the device = the proof with them on the host (the downloaded witness in a second buffer)
    rnd = F.limbs_many(F.rand_many(np.random.default_rng(3), nat.randomness_count(False)))
    dev_sections = nat.prove(witness_dev=wit, randomness=rnd, runtime_dev=(circ.rt_dev, RT))[0]
    wit2 = khip.DevBuf(32 * 15 * n).upload(got)
    host_sections = nat.prove(witness_dev=wit2, randomness=rnd, runtime=F.limbs_many(case.runtime))[0]
    assert sorted(dev_sections) == sorted(host_sections) and "lookup_runtime_comm" in dev_sections
    for name, sec in host_sections.items():
        for a, b in zip(sec if isinstance(sec, tuple) else (sec,), dev_sections[name] if isinstance(sec, tuple) else (dev_sections[name],)):
            assert a.shape == b.shape and np.array_equal(a, b), name
    vix = khip.VerifierIndex.of(nat)
    proof = khip.Proof(dev_sections)
    ok, _trace = khip.verify(vix, proof, None, ())
    assert ok
    proof.free(); vix.free()
    # one runtime value overwritten on the device: the rows that read it miss, the first in the brute force's order is named
    other = list(case.runtime); other[5] = (other[5] + 1) % case.Fo.p      # (entry 5: what slot 0 of row 1 reads)
    rt2 = khip.DevBuf(32 * RT).upload(F.limbs_many(case.runtime))
    rt2.upload_at(32 * 5, F.limbs(other[5]))
    rep, lk = nat.witness_check_full(witness_dev=wit, runtime_dev=(rt2, RT), flags=khip.WITNESS_LOOKUPS)
    ms = expect(khip, F, case, rep, lk, None, other)
    assert ms and all(m[0] % 2 == 1 for m in ms)
    # a row that reads table 9 at an entry with a non-zero tail (entry 3: column 3 holds 4): no flag -- the call reads two columns --, named by the check
    c0, c1, _c2, c3 = case.tables[1]["data"]
    assert c3[3] and not c3[1] and not c3[2]
    cells = {(10, 0): 9}
    for k, j in enumerate((3, 1, 2)):
        cells[(10, 1 + 2 * k)], cells[(10, 2 + 2 * k)] = c0[j], c1[j]
    spoiled = case.spoiled(cells)
    t9 = nat.lookup_table(9)
    k9 = circ.keys_dev([10], spoiled)
    khip.lookup_witness_dev(F.fid, circ.tid(9), t9["keys"], t9["values"], t9["len"], k9, 1, wit, n, n, row0=10, flags=flags, bit=2)
    assert word(flags) == 0
    want = circ.want.copy(); want[:, :ROWS] = case.limbs(F, spoiled)
    assert np.array_equal(wit.download((15, n, 4)), want)
    rep, lk = nat.witness_check_full(witness_dev=wit, runtime_dev=(circ.rt_dev, RT), flags=khip.WITNESS_LOOKUPS)
    ms = expect(khip, F, case, rep, lk, spoiled)
    assert [(m[0], m[1]) for m in ms] == [(10, 0)] and rep.row == 10
    # refusals of the device forms: a misaligned pointer, a wrong count
    with pytest.raises(khip.KhError, match="16-byte aligned"):
        nat.witness_check_full(witness_dev=wit, runtime_dev=(circ.rt_dev.view(8), RT), flags=khip.WITNESS_LOOKUPS)
    with pytest.raises(khip.KhError, match="RuntimeTablesInconsistent"):
        nat.witness_check_full(witness_dev=wit, runtime_dev=(circ.rt_dev, RT - 1), flags=khip.WITNESS_LOOKUPS)
    with pytest.raises(khip.KhError, match="16-byte aligned"):
        nat.prove(witness_dev=wit, randomness=rnd, runtime_dev=(circ.rt_dev.view(8), RT))
    with pytest.raises(khip.KhError, match="RuntimeTablesInconsistent"):
        nat.prove(witness_dev=wit, randomness=rnd, runtime_dev=(circ.rt_dev, RT + 1))
    for b in (wit, wit2, flags, rt2, k9):
        b.free()


def test_end_to_end(khip, circ):
    end_to_end_body(khip, circ)


def test_end_to_end_on_pallas(khip, circ_pallas):
    end_to_end_body(khip, circ_pallas)


# ---- 7. KH_STEP_LOOKUP in a schedule
M = 70                      # instances of the schedule's Lookup step: odd rows 1, 3, .., 139 (two waves of lanes per slot)
SRC = 400                   # the keys wait in cells (SRC + i, 7 + k)
ARENA = 2 * 96 * M          # the gathered keys | the step's values
PICK = (305, 2)             # where value (instance 5, slot 1) is scattered to


def lookup_steps(khip, circ, table_len=RT, consts="id", keys_ref=(0, 0), values_ref=(1, 0)):
    K = khip
    src = [(SRC + i, 7 + k) for i in range(M) for k in range(3)]
    return [
        dict(op=K.STEP_GATHER, cells=src, format=K.CELL_FIELD, out=[(K.REF_ARENA, 0)]),
        dict(op=K.STEP_LOOKUP, n=M, rows=list(range(1, 2 * M, 2)), param=table_len, consts=circ.tid(7) if consts == "id" else consts, flag_bit=4,
             **{"in": [(K.REF_ARENA, 0), keys_ref, values_ref]}, out=[(K.REF_ARENA, 96 * M)]),
        dict(op=K.STEP_SCATTER, cells=[PICK], format=K.CELL_FIELD, **{"in": [(K.REF_ARENA, 96 * M + 32 * (3 * 5 + 1))]}),
    ]


def test_schedule_step_equals_the_direct_calls(khip, circ):
    case, F, nat, n = circ.case, circ.F, circ.nat, circ.n
    t7 = nat.lookup_table(7)
    rows = list(range(1, 2 * M, 2))
    src = [(SRC + i, 7 + k) for i in range(M) for k in range(3)]
    base = np.zeros((15, n, 4), dtype=np.uint64)                          # the witness before either path: the keys in their source cells
    keys = F.limbs_many([case.wit[1 + 2 * k][r] for r in rows for k in range(3)]).reshape(M, 3, 4)
    for i in range(M):
        for k in range(3):
            base[7 + k, SRC + i] = keys[i, k]
    sched = khip.WitnessSchedule.create(F.fid, n, lookup_steps(khip, circ), arena_bytes=ARENA, n_bufs=2)
    info = sched.info()
    slots = info["run_bytes"] - ARENA
    assert (info["steps"], info["launch_groups"]) == (3, 3)
    assert slots >= 4 * 2 * RT and slots % 4 == 0 and (slots // 4) & (slots // 4 - 1) == 0, info       # a power of two of at least 2 table_len u32 slots
    wd, ws, flags = khip.DevBuf(base.nbytes), khip.DevBuf(base.nbytes), khip.DevBuf(4).zero()
    kbuf, obuf = khip.DevBuf(96 * M), khip.DevBuf(96 * M)
    for seed, runtime in ((0, case.runtime), (1, [(v * 3 + 1) % case.Fo.p for v in case.runtime])):
        rt = khip.DevBuf(32 * RT).upload(F.limbs_many(runtime))
        wd.upload(base); ws.upload(base)
        # the direct calls
        khip.witness_gather_dev(F.fid, wd, n, n, src, khip.CELL_FIELD, kbuf)
        khip.lookup_witness_dev(F.fid, circ.tid(7), t7["keys"], rt.view(32 * t7["runtime_first"]), t7["len"], kbuf, M, wd, n, n, rows=rows, out_values=obuf,
                                flags=flags, bit=4)
        khip.witness_scatter_dev(F.fid, obuf.view(32 * (3 * 5 + 1)), khip.CELL_FIELD, [PICK], wd, n, n)
        direct = wd.download((15, n, 4))
        # the expectation in integers: the rows of the brute force's witness with this run's values, the picked value
        first = case.runtime_cfg[0]["first_column"]
        at = dict(zip(first, runtime))
        want = base.copy()
        for i, r in enumerate(rows):
            want[0, r] = F.limbs(7)
            for k in range(3):
                want[1 + 2 * k, r] = keys[i, k]
                want[2 + 2 * k, r] = F.limbs(at[case.wit[1 + 2 * k][r]])
        want[PICK[1], PICK[0]] = F.limbs(at[case.wit[3][rows[5]]])
        assert np.array_equal(direct, want), seed
        staged = khip.counter("table_staged_words")
        sched.run([t7["keys"], rt], ws, flags=flags)
        assert khip.counter("table_staged_words") == staged
        assert np.array_equal(ws.download((15, n, 4)), direct), seed
        assert word(flags) == 0
        rt.free()
    sched.free()
    for b in (wd, ws, flags, kbuf, obuf):
        b.free()


def test_schedule_create_refusals(khip, circ):
    lib = khip.raw()
    n = circ.n
    for what, kw, needle in (
            ("table_len 0", dict(table_len=0), "table_len"),
            ("null consts", dict(consts=None), "table_id"),
            ("in[1] in the arena: table_len x 32 bytes end past it where n x 32 would fit", dict(keys_ref=(khip.REF_ARENA, ARENA - 32 * M)), "in[1]"),
            ("a misaligned in[2]", dict(values_ref=(1, 8)), "table_values_dev")):
        steps = lookup_steps(khip, circ, **kw)
        if what.startswith("in[1]"):
            steps[1]["param"] = M + 1                                     # (M + 1) x 32 bytes from ARENA - 32 M end 32 bytes past the arena; M x 32 fit
        arr, _keep = khip.WitnessSchedule.pack(steps)
        h = C.c_void_p(0x1234)
        assert lib.kh_witness_schedule_create(circ.F.fid, n, arr, len(steps), ARENA, 2, C.byref(h)) == khip.E_INVALID, what
        text = lib.kh_last_error().decode()
        assert "step 1 (KH_STEP_LOOKUP)" in text and needle in text, (what, text)
        assert h.value == 0x1234, what
    # ... and the same step with the table where it fits is accepted
    steps = lookup_steps(khip, circ, keys_ref=(khip.REF_ARENA, ARENA - 32 * M))
    steps[1]["param"] = M
    khip.WitnessSchedule.create(circ.F.fid, n, steps, arena_bytes=ARENA, n_bufs=2).free()
