"""kh_lookup_sorted_dev (csrc/lookup_sorted.hip) -- the `sorted` step of the lookup argument, kimchi/src/circuits/lookup/constraints.rs:90-194, as a
device hash join + expansion over device-resident columns -- against the host entry point kh_lookup_sorted (csrc/host_lookup.cpp, itself pinned to
the reference algorithm by tests/test_lookup_sorted.py): EXACT equality of every limb, the layout contract (only elements 0 .. lookup_rows of each
output column are written, rows from lookup_rows on are not read), the missing-value report, scratch reuse, the argument refusals; and kh_prove /
the Python prover on the device path (proof bytes, proofs equal to each other, the error of a spoiled witness, the call counter).

The host function shares the hash and the probing scheme with the kernels, so the cases with forced collisions (collision_case of
tests/test_lookup_sorted.py: the whole table one probe chain across the end of the slot array) are held to the pure-Python reference_sorted as well."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

from oracle import pasta as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_collisions as LC  # noqa: E402
from test_lookup_sorted import COLLISION_CASES, collision_case, miss_rows, reference_sorted  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x5e5e5e5e5e5e5e5e, 0xa1a1a1a1a1a1a1a1, 0x0123456789abcdef, 0xfedcba9876543210], dtype=np.uint64)
KH_E_INVALID = -1


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def generated(lookup_rows, distinct, mpr):
    """inputs as tests/test_lookup_sorted.py generates them: the dummy value 0 in the pool, repeated table entries, arrays 4 rows longer than the rows
    used, with values behind the used rows that are not in the table"""
    rnd = random.Random(1000 * lookup_rows + mpr)
    n = lookup_rows + 4
    pool = [(0, 0, 0, 0)] + [tuple(rnd.getrandbits(64) for _ in range(4)) for _ in range(distinct - 1)]
    table = [pool[k] if k < distinct else pool[rnd.randrange(distinct)] for k in range(lookup_rows)] + [tuple(rnd.getrandbits(64) for _ in range(4)) for _ in range(4)]
    values = [[pool[rnd.randrange(distinct)] if rnd.random() < 0.8 else (0, 0, 0, 0) for _ in range(n)] for _ in range(mpr)]
    values[0][lookup_rows] = (9, 9, 9, 9)                        # garbage at row lookup_rows: must be ignored (value_stride > lookup_rows)
    return np.array(table, dtype=np.uint64), np.array(values, dtype=np.uint64)


def run_dev(khip, table, values, lookup_rows, mpr, pad=7):
    """kh_lookup_sorted_dev over uploaded copies, out_stride = lookup_rows + pad, the output filled with a sentinel first.  Returns the
    (mpr + 1, lookup_rows + 1, 4) columns after checking that every other element still holds the sentinel; ValueError(row) passes through."""
    table = np.ascontiguousarray(table, dtype=np.uint64); values = np.ascontiguousarray(values, dtype=np.uint64)
    assert values.shape[0] == mpr and values.shape[2] == 4
    stride = lookup_rows + pad
    d_t = khip.DevBuf(table.nbytes).upload(table)
    d_v = khip.DevBuf(values.nbytes).upload(values)
    d_o = khip.DevBuf((mpr + 1) * stride * 32).upload(np.tile(SENTINEL, ((mpr + 1) * stride, 1)))
    try:
        khip.lookup_sorted_dev(d_t, lookup_rows, d_v, values.shape[1], mpr, d_o, stride)
        full = d_o.download((mpr + 1, stride, 4))
    finally:
        for b in (d_t, d_v, d_o):
            b.free()
    assert np.array_equal(full[:, lookup_rows + 1:], np.broadcast_to(SENTINEL, (mpr + 1, stride - lookup_rows - 1, 4))), "an element behind the column was written"
    return np.ascontiguousarray(full[:, :lookup_rows + 1])


def check_equal_to_host(khip, table, values, lookup_rows, mpr):
    want = khip.lookup_sorted(table, lookup_rows, values, mpr)
    before = khip.counter("lookup_sorted_dev")
    got = run_dev(khip, table, values, lookup_rows, mpr)
    assert khip.counter("lookup_sorted_dev") == before + 1
    assert got.shape == want.shape == (mpr + 1, lookup_rows + 1, 4)
    assert np.array_equal(got, want), "first difference at (column, index, limb) %s" % (tuple(np.argwhere(got != want)[0]),)
    return got


# the host test's own six; a 2^7 domain with 3 zk rows (no multiple of a block or a wave, the last column even); a size at which the prefix sum and the
# expansion cross many blocks and a run straddles a column boundary
@pytest.mark.parametrize("lookup_rows,distinct,mpr", [(1, 1, 1), (12, 5, 3), (60, 60, 4), (500, 37, 3), (4092, 1500, 4), (300, 299, 1), (124, 40, 2),
                                                      (8188, 4096, 4)])
def test_device_columns_equal_the_host_columns(khip, lookup_rows, distinct, mpr):
    table, values = generated(lookup_rows, distinct, mpr)
    check_equal_to_host(khip, table, values, lookup_rows, mpr)


@pytest.mark.parametrize("zero_at", ["first", "last"])
def test_all_dummy_values(khip, zero_at):
    """every looked-up value is 0 and the table holds 0 once: one run covers four whole columns, every add lands on one counter.  With the 0 entry last
    the run ends at the very last position and feeds the repeated final element."""
    lookup_rows, distinct, mpr = 1020, 300, 4
    rnd = random.Random(77)
    pool = [tuple(rnd.getrandbits(64) for _ in range(4)) for _ in range(distinct - 1)]
    rest = [pool[k] if k < distinct - 1 else pool[rnd.randrange(distinct - 1)] for k in range(lookup_rows - 1)]
    table = [(0, 0, 0, 0)] + rest if zero_at == "first" else rest + [(0, 0, 0, 0)]
    assert table.count((0, 0, 0, 0)) == 1 and table.index((0, 0, 0, 0)) == (0 if zero_at == "first" else lookup_rows - 1)
    values = np.zeros((mpr, lookup_rows, 4), dtype=np.uint64)
    check_equal_to_host(khip, np.array(table, dtype=np.uint64), values, lookup_rows, mpr)


def test_a_table_of_one_repeated_value(khip):
    """257 copies of one value, 3 lookups per row: only the first occurrence collects counts"""
    lookup_rows, mpr = 257, 3
    v = (11, 22, 33, 44)
    table = np.array([v] * lookup_rows, dtype=np.uint64)
    values = np.array([[v] * lookup_rows] * mpr, dtype=np.uint64)
    check_equal_to_host(khip, table, values, lookup_rows, mpr)


def test_a_repeated_value_that_is_not_contiguous(khip):
    """two values alternating over 1001 entries, then a run of a third: the repeats of a hot key are neither neighbours nor in table order of arrival"""
    lookup_rows, mpr = 1301, 2
    a, b, c = (5, 0, 0, 9), (5, 0, 0, 8), (0, 0, 0, 0)
    table = np.array([a if k % 2 == 0 else b for k in range(1001)] + [c] * 300, dtype=np.uint64)
    rnd = random.Random(9)
    values = np.array([[(a, b, c)[rnd.randrange(3)] for _ in range(lookup_rows)] for _ in range(mpr)], dtype=np.uint64)
    check_equal_to_host(khip, table, values, lookup_rows, mpr)


def test_keys_that_differ_in_one_limb_only(khip):
    """(k,0,0,0), (0,k,0,0), (0,0,k,0), (0,0,0,k) for k = 1 .. 64: hash and comparison use all 32 bytes"""
    mpr = 2
    keys = [tuple(k if j == limb else 0 for j in range(4)) for limb in range(4) for k in range(1, 65)]
    lookup_rows = len(keys)
    rnd = random.Random(5)
    table = np.array(keys, dtype=np.uint64)
    values = np.array([[keys[rnd.randrange(lookup_rows)] for _ in range(lookup_rows)] for _ in range(mpr)], dtype=np.uint64)
    check_equal_to_host(khip, table, values, lookup_rows, mpr)


def test_layout_only_the_columns_are_written_and_rows_behind_are_not_read(khip):
    """out_stride = lookup_rows + 7 over a sentinel (checked inside run_dev for every case of this file; here with another padding too), value_stride >
    lookup_rows with values at rows lookup_rows .. that are not in the table"""
    lookup_rows, distinct, mpr = 124, 40, 2
    table, values = generated(lookup_rows, distinct, mpr)
    values[:, lookup_rows:] = (7, 7, 7, 7)
    want = khip.lookup_sorted(table, lookup_rows, values, mpr)
    for pad in (7, 1, 33):
        assert np.array_equal(run_dev(khip, table, values, lookup_rows, mpr, pad=pad), want)


@pytest.mark.parametrize("offenders,row", [([(2, 5), (0, 9)], 9), ([(1, 40), (1, 17)], 17)], ids=["two-slots", "one-slot"])
def test_a_missing_value_reports_the_row_the_host_reports(khip, offenders, row):
    """the first offender in slot-major order (lowest slot, then lowest row), KH_E_INVALID, the host's text; the output stays untouched; a correct call
    on the same context afterwards gives the right columns (status and slots are cleared per call)"""
    lookup_rows, distinct, mpr = 60, 20, 3
    table, values = generated(lookup_rows, distinct, mpr)
    good = values.copy()
    for s, r in offenders:
        values[s, r] = (1, 2, 3, 4)
    with pytest.raises(ValueError) as host:
        khip.lookup_sorted(table, lookup_rows, values, mpr)
    host_text = khip.raw().kh_last_error().decode()
    assert host.value.args[0] == row
    before = khip.counter("lookup_sorted_dev")
    with pytest.raises(ValueError) as dev:
        run_dev(khip, table, values, lookup_rows, mpr)
    assert dev.value.args[0] == host.value.args[0] == row
    assert khip.raw().kh_last_error().decode() == host_text and "not in the table" in host_text and f"row {row} " in host_text
    assert khip.counter("lookup_sorted_dev") == before
    # the raw call: KH_E_INVALID, and nothing of the output was written
    d_t = khip.DevBuf(table.nbytes).upload(table); d_v = khip.DevBuf(values.nbytes).upload(values)
    stride = lookup_rows + 1
    d_o = khip.DevBuf((mpr + 1) * stride * 32).upload(np.tile(SENTINEL, ((mpr + 1) * stride, 1)))
    bad = C.c_size_t(0)
    rc = khip.raw().kh_lookup_sorted_dev(d_t.ptr, lookup_rows, d_v.ptr, values.shape[1], mpr, d_o.ptr, stride, C.byref(bad))
    assert rc == KH_E_INVALID and bad.value == row
    assert np.array_equal(d_o.download(((mpr + 1) * stride, 4)), np.tile(SENTINEL, ((mpr + 1) * stride, 1)))
    for b in (d_t, d_v, d_o):
        b.free()
    check_equal_to_host(khip, table, good, lookup_rows, mpr)


def test_two_shapes_back_to_back_reuse_the_scratch(khip):
    big = generated(4092, 1500, 4); small = generated(12, 5, 3)
    check_equal_to_host(khip, big[0], big[1], 4092, 4)
    check_equal_to_host(khip, small[0], small[1], 12, 3)
    check_equal_to_host(khip, big[0], big[1], 4092, 4)


def test_argument_refusals_launch_nothing(khip):
    lookup_rows, distinct, mpr = 12, 5, 3
    table, values = generated(lookup_rows, distinct, mpr)
    stride = lookup_rows + 1
    d_t = khip.DevBuf(table.nbytes).upload(table); d_v = khip.DevBuf(values.nbytes).upload(values)
    d_o = khip.DevBuf((mpr + 1) * stride * 32).upload(np.tile(SENTINEL, ((mpr + 1) * stride, 1)))
    vs = values.shape[1]
    lib = khip.raw()
    bad = C.c_size_t(0)
    before = khip.counter("lookup_sorted_dev")
    refused = {
        "null table": (None, lookup_rows, d_v.ptr, vs, mpr, d_o.ptr, stride),
        "null values": (d_t.ptr, lookup_rows, None, vs, mpr, d_o.ptr, stride),
        "null output": (d_t.ptr, lookup_rows, d_v.ptr, vs, mpr, None, stride),
        "lookup_rows == 0": (d_t.ptr, 0, d_v.ptr, vs, mpr, d_o.ptr, stride),
        "max_per_row == 0": (d_t.ptr, lookup_rows, d_v.ptr, vs, 0, d_o.ptr, stride),
        "value_stride < lookup_rows": (d_t.ptr, lookup_rows, d_v.ptr, lookup_rows - 1, mpr, d_o.ptr, stride),
        "out_stride < lookup_rows + 1": (d_t.ptr, lookup_rows, d_v.ptr, vs, mpr, d_o.ptr, lookup_rows),
        "(max_per_row + 1) * lookup_rows == 2^31": (d_t.ptr, 1 << 29, d_v.ptr, 1 << 29, 3, d_o.ptr, (1 << 29) + 1),
        "(max_per_row + 1) * lookup_rows > 2^31": (d_t.ptr, 3, d_v.ptr, 3, 1 << 30, d_o.ptr, 4),
    }
    for what, args in refused.items():
        assert lib.kh_lookup_sorted_dev(*args, C.byref(bad)) == KH_E_INVALID, what
        assert lib.kh_last_error().decode().startswith("kh_lookup_sorted_dev"), what
    assert khip.counter("lookup_sorted_dev") == before
    assert np.array_equal(d_o.download(((mpr + 1) * stride, 4)), np.tile(SENTINEL, ((mpr + 1) * stride, 1)))
    # bad_row may be null
    assert lib.kh_lookup_sorted_dev(d_t.ptr, lookup_rows, d_v.ptr, vs, mpr, d_o.ptr, stride, None) == 0
    assert np.array_equal(d_o.download((mpr + 1, stride, 4)), khip.lookup_sorted(table, lookup_rows, values, mpr))
    for b in (d_t, d_v, d_o):
        b.free()


# ---------------------------------------------------------------------------------------------------------------- forced collisions
def raw_call(khip, table, values, lookup_rows, mpr):
    """(return code, bad_row, whether the sentinel-filled output is untouched) of the C entry point"""
    d_t = khip.DevBuf(table.nbytes).upload(table); d_v = khip.DevBuf(values.nbytes).upload(values)
    stride = lookup_rows + 1
    fill = np.tile(SENTINEL, ((mpr + 1) * stride, 1))
    d_o = khip.DevBuf((mpr + 1) * stride * 32).upload(fill)
    bad = C.c_size_t(0)
    try:
        rc = khip.raw().kh_lookup_sorted_dev(d_t.ptr, lookup_rows, d_v.ptr, values.shape[1], mpr, d_o.ptr, stride, C.byref(bad))
        untouched = np.array_equal(d_o.download(((mpr + 1) * stride, 4)), fill)
    finally:
        for b in (d_t, d_v, d_o):
            b.free()
    return rc, bad.value, untouched


@pytest.mark.parametrize("mpr", (1, 3))
@pytest.mark.parametrize("lookup_rows,merge", COLLISION_CASES)
def test_colliding_tables_equal_the_reference_algorithm(khip, lookup_rows, merge, mpr):
    """k_sorted_build / k_sorted_count on a table that is one probe chain across the end of the slot array (the preconditions are asserted in
    collision_case): 600 and 1024 entries span several blocks of k_sorted_build, whose threads then contend for the slots of ONE chain; 8 and 1024 are
    at exactly half load; in the 48 and 600 cases the hot key sits at entries 9, 23 and L - 1 of the chain.  Three runs each: the atomics arrive in
    another order every time, the columns may not change.  An absent value whose home is the head of the chain, or its middle behind the wrap, is
    reported only after the walk: the row, KH_E_INVALID, nothing written."""
    case = collision_case(P.Fp, lookup_rows, mpr, merge)
    table, values = np.array(case.table, dtype=np.uint64), np.array(case.values, dtype=np.uint64)
    want = np.array(reference_sorted(list(case.table), case.values, lookup_rows, mpr), dtype=np.uint64)
    assert want.shape == (mpr + 1, lookup_rows + 1, 4)
    host = khip.lookup_sorted(table, lookup_rows, values, mpr)
    for attempt in range(3):
        got = run_dev(khip, table, values, lookup_rows, mpr)
        assert np.array_equal(got, want), "run %d: first difference from the reference at (column, index, limb) %s" % (attempt, tuple(np.argwhere(got != want)[0]))
        assert np.array_equal(got, host)
    for name, absent in case.misses:
        row = miss_rows(lookup_rows)[name]
        bad = values.copy()
        bad[mpr - 1, row] = absent
        with pytest.raises(ValueError) as ref:
            reference_sorted(list(case.table), [[tuple(int(x) for x in v) for v in col] for col in bad], lookup_rows, mpr)
        assert ref.value.args[0] == row
        with pytest.raises(ValueError) as dev:
            run_dev(khip, table, bad, lookup_rows, mpr)
        assert dev.value.args[0] == row, name
        for attempt in range(3):
            assert raw_call(khip, table, bad, lookup_rows, mpr) == (KH_E_INVALID, row, True), (name, attempt)
    assert np.array_equal(run_dev(khip, table, values, lookup_rows, mpr), want)      # status and slots are cleared per call


def test_tiny_random_tables_at_sixteen_slots(khip):
    """64 tables of 1 .. 8 entries (16 slots, up to half load) of random canonical elements with repeats: the collisions that happen by themselves at
    the smallest capacity, against the reference and the host"""
    rnd = random.Random(64)
    collided = repeats = 0
    for _ in range(64):
        lookup_rows, mpr = rnd.randrange(1, 9), rnd.randrange(1, 4)
        pool = [LC.mont_limbs(P.Fp, rnd.randrange(P.Fp.p)) for _ in range(rnd.randrange((lookup_rows + 1) // 2, lookup_rows + 1))]
        keys = pool + [rnd.choice(pool) for _ in range(lookup_rows - len(pool))]
        rnd.shuffle(keys)
        vals = [[rnd.choice(keys) for _ in range(lookup_rows)] for _ in range(mpr)]
        assert LC.slots(lookup_rows) == 16
        repeats += len(set(keys)) < lookup_rows
        collided += LC.longest_run([LC.home(k, lookup_rows) for k in dict.fromkeys(keys)], 16).displacement > 0
        table, values = np.array(keys, dtype=np.uint64), np.array(vals, dtype=np.uint64)
        want = np.array(reference_sorted(keys, vals, lookup_rows, mpr), dtype=np.uint64)
        got = run_dev(khip, table, values, lookup_rows, mpr)
        assert np.array_equal(got, want) and np.array_equal(got, khip.lookup_sorted(table, lookup_rows, values, mpr)), (lookup_rows, mpr, keys)
    assert collided >= 16 and repeats >= 16, (collided, repeats)    # (fixed by the seed: 19 of the 64 tables have a displaced key, 34 a repeated one)


# ---------------------------------------------------------------------------------------------------------------- prover level

def test_kh_prove_reproduces_the_committed_lookup_proof_on_the_device_path(khip):
    """the 2^13 AND-gadget fixture (Xor16 rows + 4-bit XOR-table lookups): the same bytes, and the sorted columns came from kh_lookup_sorted_dev -- once"""
    committed_lookup_proof_on_the_device_path(khip, "and_lookup_vesta_2_13")


def test_kh_prove_reproduces_the_committed_pallas_lookup_proof_on_the_device_path(khip):
    """the same over Fq: the sort, the join and the layout kernels' other instantiation inside a Pallas proof"""
    committed_lookup_proof_on_the_device_path(khip, "and_lookup_pallas_2_13")


def committed_lookup_proof_on_the_device_path(khip, name):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_proof_fixtures as M
    from oracle import pasta as P, prover as OPR, views as V
    from proof_systems_amd import prover
    from test_gpu_proof_fixtures import first_difference, load
    from test_gpu_prover_parity import _limbs, device_index
    rec, want = load(name)
    cid = ["vesta", "pallas"].index(rec["curve"])
    assert (khip.VESTA, khip.PALLAS) == (0, 1)
    Cv = P.CURVES[cid]; Fo = Cv.scalar
    cs, wrows = M.and_circuit(Fo, rec["log2_n"])
    ix = device_index(khip, cs, cid, khip.Srs.create(cid, 1 << rec["log2_srs"]))
    wit = np.stack([_limbs(Fo, [r[c] for r in wrows]) for c in range(15)])
    before = khip.counter("lookup_sorted_dev")
    nproof = prover.create_proof_native(ix, wit, V.RefRng(P.StdRng(bytes.fromhex(rec["seed_hex"]))))
    assert khip.counter("lookup_sorted_dev") == before + 1
    got = OPR.serialize_proof(Cv, V.device_views(ix, nproof)[2])
    assert got == want, "kh_prove (lookups) differs from the committed proof: first in " + first_difference(Cv, got, want)
    ix.free()


def two_table_circuit(khip, cid):
    """the 2^9 circuit of tests/test_gpu_prover.py: 30 generic rows, 200 Lookup gates into two user tables with ids 0 and 3"""
    from proof_systems_amd import lookup as LK, prover
    logn = 9; n = 1 << logn
    rnd = random.Random(21)
    fid = khip.FP if cid == 0 else khip.FQ
    F = prover.Fld(fid)
    tables = [{"id": 0, "data": [list(range(40)), [0] + [rnd.randrange(F.p) for _ in range(39)]]},
              {"id": 3, "data": [list(range(25)), [rnd.randrange(F.p) for _ in range(25)]]}]
    ngen, nlook = 30, 200
    co = np.zeros((ngen, 15, 4), dtype=np.uint64)
    co[:, 0, :] = F.limbs(1); co[:, 4, :] = F.limbs(F.p - 7)
    gates = ["Generic"] * ngen + ["Lookup"] * nlook + ["Zero"] * (n - 3 - ngen - nlook)
    rows = ngen + nlook
    wit = [[0] * rows for _ in range(15)]
    for r in range(ngen):
        wit[0][r] = 7
    for r in range(ngen, rows):
        t = tables[rnd.randrange(2)]
        wit[0][r] = t["id"]
        for i in range(3):
            e = rnd.randrange(len(t["data"][0]))
            wit[2 * i + 1][r], wit[2 * i + 2][r] = t["data"][0][e], t["data"][1][e]
    ix = prover.ProverIndex(cid, logn, co)
    LI = LK.LookupIndex(fid, gates, tables, logn)
    ix.attach_lookup(LI)
    return ix, LI, F, wit, ngen


@pytest.mark.parametrize("cid", [0, 1])
def test_native_and_python_provers_agree_on_the_device_path(khip, cid):
    from oracle import views as V
    from proof_systems_amd import prover
    ix, LI, F, wit, ngen = two_table_circuit(khip, cid)
    w = np.stack([F.limbs_many(c) for c in wit])
    c0 = khip.counter("lookup_sorted_dev")
    proof = prover.create_proof(ix, w, np.random.default_rng(8))
    c1 = khip.counter("lookup_sorted_dev")
    nproof = prover.create_proof_native(ix, w, np.random.default_rng(8))
    c2 = khip.counter("lookup_sorted_dev")
    assert c1 == c0 + 1 and c2 == c1 + 1
    assert nproof["challenges"] == proof["challenges"] and V.device_views(ix, nproof)[2] == V.device_views(ix, proof)[2]
    spoiled = ngen + 5
    wit[2][spoiled] = (wit[2][spoiled] + 1) % F.p                       # a looked-up value that is not in its table
    wb = np.stack([F.limbs_many(c) for c in wit])
    with pytest.raises(khip.KhError, match="not in the table") as e:
        prover.create_proof_native(ix, wb, np.random.default_rng(8))
    assert f"lookup in row {spoiled} " in str(e.value)
    with pytest.raises(ValueError) as e:
        prover.create_proof(ix, wb, np.random.default_rng(8))
    assert e.value.args[0] == spoiled
    assert khip.counter("lookup_sorted_dev") == c2
    ix.free()


def test_lookup_py_device_path_equals_its_python_path(khip):
    """proof_systems_amd/lookup.py: sorted_columns_dev (values, join and layout on the device) against sorted_columns (Python integers, the
    restatement of lookup/constraints.rs:90-194) on the two-table circuit; and written in place into padded columns"""
    lookup_py_device_path_equals_its_python_path(khip, 0)


def test_lookup_py_device_path_equals_its_python_path_on_pallas(khip):
    lookup_py_device_path_equals_its_python_path(khip, 1)


def lookup_py_device_path_equals_its_python_path(khip, cid):
    from proof_systems_amd import lookup as LK
    ix, LI, F, wit, ngen = two_table_circuit(khip, cid)
    n, zk = LI.n, LI.zk_rows
    jc = 0x1234567890abcdef1234567890abcdef % F.p
    wfull = np.zeros((15, n, 4), dtype=np.uint64)
    wfull[:, :len(wit[0])] = np.stack([F.limbs_many(c) for c in wit])
    ev = khip.DevBuf(15 * n * 32).upload(wfull)
    d_wit = [ev.view(i * n * 32) for i in range(15)]
    d_table = LI.joint_table_dev(jc, None)
    table_ints = F.values(d_table.download((n, 4)))
    want = np.stack([F.limbs_many(c) for c in LK.sorted_columns(LI, [c + [0] * (n - len(c)) for c in wit], table_ints, jc)])
    assert want.shape == (LI.max_per_row + 1, n - zk, 4)
    got = LK.sorted_columns_dev(LI, d_wit, d_table, jc)
    assert np.array_equal(got, want)
    assert np.array_equal(LK.sorted_columns_host(LI, d_wit, d_table, jc), want)
    ns = LI.max_per_row + 1
    out = khip.DevBuf(ns * n * 32).upload(np.tile(SENTINEL, (ns * n, 1)))
    assert LK.sorted_columns_dev(LI, d_wit, d_table, jc, out=out) is None
    full = out.download((ns, n, 4))
    assert np.array_equal(full[:, :n - zk], want) and np.array_equal(full[:, n - zk:], np.broadcast_to(SENTINEL, (ns, zk, 4)))
    for b in (out, ev, d_table):
        b.free()
    ix.free()
