"""kh_lookup_witness_dev (csrc/lookup_rows.hip): the rows of GateType::Lookup written on the device from a table's two columns and the keys.

The expected values are a Python dict over the integers this file puts into the table, first occurrence wins; every comparison is exact: the whole
15 x COL_LEN witness against a sentinel-filled array with the expected cells replaced, so a cell the call must not write is checked too.

Random keys at half load give probe chains of one or two slots; section 5 runs tables whose keys are made to collide (collision_case of
tests/test_lookup_sorted.py, on the hash mirror tests/test_lookup_hash.py pins): the whole table is one chain across the end of the slot array."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

from oracle import pasta as P

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lookup_collisions as LC  # noqa: E402
from test_gpu_limb_gadgets_dev import SENTINEL, SIZES, flag_word, mont, sentinel_buf  # noqa: E402
from test_lookup_sorted import collision_case  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = (P.Fp, P.Fq)
COL_LEN = 512
TABLE_ID = 5


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def fid(khip, F):
    return khip.FP if F.p == P.Fp.p else khip.FQ


def table40(F):
    """40 entries: the key 0 (entry 3), and entry 23 repeats the key of entry 9 with another value -- the lower row's value is the table's"""
    keys = [7 * j + 1 for j in range(40)]
    keys[3] = 0
    keys[23] = keys[9]
    values = [(j * j + 3) * 1000003 % F.p for j in range(40)]
    assert values[23] != values[9]
    return keys, values


def first_wins(keys, values):
    d = {}
    for k, v in zip(keys, values):
        d.setdefault(k, v)
    return d


class Table:
    def __init__(self, khip, F, keys, values):
        self.keys, self.values, self.len = keys, values, len(keys)
        self.k_dev = khip.DevBuf(32 * self.len).upload(mont(F, keys))
        self.v_dev = khip.DevBuf(32 * self.len).upload(mont(F, values))
        self.at = first_wins(keys, values)

    def free(self):
        self.k_dev.free(); self.v_dev.free()


def expected(F, rows, keys3, table_at, tid=TABLE_ID):
    """(the 15 x COL_LEN x 4 witness after the call on a sentinel-filled one, the n x 3 x 4 values): a key that is not in the table reads zero"""
    n = len(rows)
    flat = [k for ks in keys3 for k in ks]
    vals = [table_at.get(k, 0) for k in flat]
    km, vm = mont(F, flat).reshape(n, 3, 4), mont(F, vals).reshape(n, 3, 4)
    w = np.tile(SENTINEL, (15, COL_LEN, 1))
    w[0, rows] = mont(F, [tid])[0]
    for k in range(3):
        w[2 * k + 1, rows] = km[:, k]
        w[2 * k + 2, rows] = vm[:, k]
    return w, vm


def call(khip, F, tab, rows_kw, keys3, out=True, flags=None, bit=0, tid=TABLE_ID):
    """one call on a fresh sentinel-filled witness; returns (witness, out values or None)"""
    n = len(keys3)
    kd = khip.DevBuf(96 * n).upload(mont(F, [k for ks in keys3 for k in ks]))
    wit = sentinel_buf(khip, 15 * COL_LEN)
    od = sentinel_buf(khip, 3 * n) if out else None
    khip.lookup_witness_dev(fid(khip, F), mont(F, [tid])[0], tab.k_dev, tab.v_dev, tab.len, kd, n, wit, COL_LEN, COL_LEN, out_values=od, flags=flags, bit=bit,
                            **rows_kw)
    w = wit.download((15, COL_LEN, 4))
    o = od.download((n, 3, 4)) if out else None
    for b in (kd, wit) + ((od,) if out else ()):
        b.free()
    return w, o


def placements(n):
    rows = random.Random(n).sample(range(COL_LEN), n)             # out of order, with gaps
    return (("rows[]", dict(rows=rows), rows), ("row0 / row_stride", dict(row0=5, row_stride=3), [5 + 3 * i for i in range(n)]))


# ---- 1. rows and values
@pytest.mark.parametrize("F", FIELDS, ids=("fp", "fq"))
@pytest.mark.parametrize("n", SIZES)
def test_rows_and_values(khip, F, n):
    keys, values = table40(F)
    tab = Table(khip, F, keys, values)
    assert tab.at[keys[9]] == values[9] and tab.at[0] == values[3]
    rnd = random.Random(100 + n)
    keys3 = [[rnd.choice(keys) for _ in range(3)] for _ in range(n)]
    keys3[0] = [0, keys[23], keys[39]]                             # the key 0, the repeated key, the last entry
    keys3[-1][2] = keys[9]
    for what, kw, rows in placements(n):
        want_w, want_o = expected(F, rows, keys3, tab.at)
        w, o = call(khip, F, tab, kw, keys3)
        assert np.array_equal(o, want_o), what
        assert np.array_equal(w, want_w), what
        w, _ = call(khip, F, tab, kw, keys3, out=False)           # out_values_dev = NULL: the same cells
        assert np.array_equal(w, want_w), what
    tab.free()


# ---- 2. table sizes: one entry, two, and 4096 entries in 8192 slots (probe chains longer than one, where random keys happen to make them: section 5 makes them)
@pytest.mark.parametrize("F", FIELDS, ids=("fp", "fq"))
@pytest.mark.parametrize("table_len", (1, 2, 4096))
def test_table_sizes(khip, F, table_len):
    rnd = random.Random(table_len)
    keys, seen = [], set()
    while len(keys) < table_len:                                   # distinct keys
        k = rnd.randrange(1 << 250)
        if k not in seen:
            seen.add(k); keys.append(k)
    values = [rnd.randrange(F.p) for _ in range(table_len)]
    tab = Table(khip, F, keys, values)
    n = 130
    picks = [0, table_len - 1] + [rnd.randrange(table_len) for _ in range(3 * n - 2)]       # the first entry, the last, entries in between
    keys3 = [[keys[picks[3 * i + k]] for k in range(3)] for i in range(n)]
    rows = list(range(7, 7 + n))
    want_w, want_o = expected(F, rows, keys3, tab.at)
    flags = khip.DevBuf(4).zero()
    w, o = call(khip, F, tab, dict(row0=7, row_stride=1), keys3, flags=flags, bit=3)
    assert np.array_equal(o, want_o) and np.array_equal(w, want_w)
    assert flag_word(flags) == 0
    flags.free(); tab.free()


# ---- 3. misses
def test_misses_raise_the_flag_and_read_zero(khip):
    F = P.Fp
    keys, values = table40(F)
    tab = Table(khip, F, keys, values)
    n = 130
    rnd = random.Random(9)
    keys3 = [[rnd.choice(keys) for _ in range(3)] for _ in range(n)]
    hit = [list(ks) for ks in keys3]
    keys3[0][1], keys3[64][0], keys3[129][2] = 2, F.p - 1, 7 * 40 + 1                          # absent keys, in different slots
    kw, rows = dict(row0=100, row_stride=2), [100 + 2 * i for i in range(n)]
    want_w, want_o = expected(F, rows, keys3, tab.at)
    zero = np.zeros(4, dtype=np.uint64)
    for i, k in ((0, 1), (64, 0), (129, 2)):
        assert np.array_equal(want_o[i, k], zero) and np.array_equal(want_w[2 * k + 2, rows[i]], zero)
    preset = 0x00500003
    word = lambda: khip.DevBuf(4).upload(np.array([preset], dtype=np.uint32))
    flags = word()
    w, o = call(khip, F, tab, kw, keys3, flags=flags, bit=17)
    assert flag_word(flags) == preset | (1 << 17)
    assert np.array_equal(o, want_o) and np.array_equal(w, want_w)
    flags.free()
    flags = word()                                                  # no miss: the word stays as it was
    hw, ho = expected(F, rows, hit, tab.at)
    w, o = call(khip, F, tab, kw, hit, flags=flags, bit=17)
    assert flag_word(flags) == preset and np.array_equal(o, ho) and np.array_equal(w, hw)
    flags.free()
    w, o = call(khip, F, tab, kw, keys3, flags=None)              # flags_dev = NULL: the same cells
    assert np.array_equal(o, want_o) and np.array_equal(w, want_w)
    tab.free()


# ---- 4. refusals of the direct call
def test_refusals_leave_everything_untouched(khip):
    lib = khip.raw()
    F = P.Fp
    n, L = 3, 8
    tk, tv, keys = sentinel_buf(khip, L), sentinel_buf(khip, L), sentinel_buf(khip, 3 * n)
    wit, out, flags = sentinel_buf(khip, 15 * COL_LEN), sentinel_buf(khip, 3 * n), sentinel_buf(khip, 1)
    vp = C.c_void_p
    id_t, rows_t = C.c_uint64 * 4, C.c_uint32 * 3
    good = id_t(*[int(x) for x in mont(F, [TABLE_ID])[0]])
    p_limbs = id_t(*[int(x) for x in np.frombuffer(F.p.to_bytes(32, "little"), dtype=np.uint64)])

    def go(field=0, tid=good, k_=tk.ptr, v_=tv.ptr, tl=L, a=keys.ptr, k=n, rows=None, row0=0, row_stride=1, w=wit.ptr, col_stride=COL_LEN, col_len=COL_LEN,
           o=out.ptr, f=flags.ptr, bit=0):
        return lib.kh_lookup_witness_dev(field, tid, vp(k_), vp(v_), tl, vp(a), k, rows, row0, row_stride, vp(w), col_stride, col_len, vp(o), vp(f), bit)

    refused = [
        ("unknown field", lambda: go(field=2), None),
        ("null witness", lambda: go(w=None), None),
        ("null keys", lambda: go(a=None), None),
        ("unaligned keys", lambda: go(a=keys.ptr + 8), None),
        ("unaligned out", lambda: go(o=out.ptr + 8), None),
        ("unaligned witness", lambda: go(w=wit.ptr + 8, col_len=COL_LEN - 1, col_stride=COL_LEN - 1), None),
        ("byte count overflows", lambda: go(col_stride=1 << 62), None),
        ("too many instances", lambda: go(k=1 << 40, col_len=1 << 50, col_stride=1 << 50), None),
        ("an instance past the end", lambda: go(rows=rows_t(0, 20, COL_LEN)), "instance 2"),
        ("row_stride 0", lambda: go(row_stride=0), None),
        ("the last instance past the end", lambda: go(row0=COL_LEN - n + 1), None),
        ("col_len 0", lambda: go(k=1, col_len=0, col_stride=0), None),
        ("col_stride < col_len", lambda: go(col_stride=COL_LEN - 1), None),
        ("null table_id", lambda: go(tid=None), "table_id"),
        ("table_id = p", lambda: go(tid=p_limbs), "table_id"),
        ("table_len 0", lambda: go(tl=0), "table_len"),
        ("table_len 2^31", lambda: go(tl=1 << 31), "table_len"),
        ("table_len 2^32 + 8", lambda: go(tl=(1 << 32) + 8), "table_len"),
        ("null table keys", lambda: go(k_=None), "table_keys_dev"),
        ("null table values", lambda: go(v_=None), "table_values_dev"),
        ("unaligned table keys", lambda: go(k_=tk.ptr + 8), "table_keys_dev"),
        ("unaligned table values", lambda: go(v_=tv.ptr + 4), "table_values_dev"),
        ("3 n lanes past the grid limit", lambda: go(k=(1 << 36) // 3 + 1, col_len=1 << 50, col_stride=1 << 50), "instances"),
        ("flag bit 32", lambda: go(bit=32), None),
        ("unaligned flag word", lambda: go(f=flags.ptr + 2), None),
    ]
    for what, run, needle in refused:
        assert run() == khip.E_INVALID, what
        text = lib.kh_last_error().decode()
        assert "kh_lookup_witness_dev" in text, (what, text)
        if needle:
            assert needle in text, (what, text)
    for buf, elems in ((tk, L), (tv, L), (keys, 3 * n), (wit, 15 * COL_LEN), (out, 3 * n), (flags, 1)):
        assert np.array_equal(buf.download((elems, 4)), np.tile(SENTINEL, (elems, 1)))
    # ... and what is allowed: n == 0 with null pointers, nothing launched
    assert lib.kh_lookup_witness_dev(0, None, None, None, 1, None, 0, None, 0, 0, None, 0, 0, None, None, 0) == 0
    for b in (tk, tv, keys, wit, out, flags):
        b.free()


# ---- 5. forced collisions: the table is one probe chain that wraps from the last slot to slot 0
COLLIDING = (1, 2, 8, 48, 600, 1024)                              # blocks are one wave: 600 and 1024 entries are 10 and 16 blocks of k_lookup_build on ONE chain
PRESET = 0x00500003


def colliding_table(khip, F, table_len):
    """the keys of collision_case (its preconditions are asserted there: homes in the last two slots, one chain across the wrap, displacement; 8 and 1024
    at exactly half load; 48 and 600 with ONE key at entries 9, 23 and L - 1) with distinct non-zero values -- so the three entries of the repeated key
    differ in their values, and every probe of it must read entry 9's"""
    case = collision_case(F, table_len, 1)
    keys = list(case.keys)
    rnd = random.Random(31 * table_len)
    values = [rnd.randrange(1, F.p) for _ in keys]
    assert len(set(values)) == table_len and len(set(keys)) == case.distinct
    tab = Table(khip, F, keys, values)
    if case.distinct < table_len:
        assert keys[9] == keys[23] == keys[-1] and tab.at[keys[23]] == tab.at[keys[-1]] == values[9] and values[9] not in (values[23], values[-1])
    return case, tab


def preset_word(khip):
    return khip.DevBuf(4).upload(np.array([PRESET], dtype=np.uint32))


@pytest.mark.parametrize("F", FIELDS, ids=("fp", "fq"))
@pytest.mark.parametrize("table_len", COLLIDING)
def test_colliding_tables(khip, F, table_len):
    """every entry of the table probed at least once (130 instances = 390 probes a call, so up to three calls), through both placements, three runs
    each: the build's atomics arrive in another order every time, the witness may not change.  Then absent keys -- home = the head of the chain, home =
    its middle behind the wrap -- in lanes 0, 64 and 129: zero values, exactly the caller's bit over a preset word."""
    case, tab = colliding_table(khip, F, table_len)
    n = 130
    rnd = random.Random(500 + table_len)
    keys3 = None
    for first in range(0, table_len, 3 * n):
        picks = list(range(first, min(first + 3 * n, table_len)))
        picks += [rnd.randrange(table_len) for _ in range(3 * n - len(picks))]
        rnd.shuffle(picks)
        keys3 = [[tab.keys[picks[3 * i + k]] for k in range(3)] for i in range(n)]
        for what, kw, rows in placements(n):
            want_w, want_o = expected(F, rows, keys3, tab.at)
            for attempt in range(3):
                flags = preset_word(khip)
                w, o = call(khip, F, tab, kw, keys3, flags=flags, bit=17)
                assert flag_word(flags) == PRESET, (what, attempt)                # no miss: the word stays as it was
                assert np.array_equal(o, want_o), (what, attempt)
                assert np.array_equal(w, want_w), (what, attempt)
                flags.free()
    head, mid = case.absent["head"], case.absent.get("mid", case.absent["head"])        # (one entry: nothing of the chain lies behind the wrap)
    assert head not in tab.at and mid not in tab.at
    keys3[0][1], keys3[64][0], keys3[129][2] = head, mid, head
    zero = np.zeros(4, dtype=np.uint64)
    for what, kw, rows in placements(n):
        want_w, want_o = expected(F, rows, keys3, tab.at)
        for i, k in ((0, 1), (64, 0), (129, 2)):
            assert np.array_equal(want_o[i, k], zero) and np.array_equal(want_w[2 * k + 2, rows[i]], zero)
        for attempt in range(3):
            flags = preset_word(khip)
            w, o = call(khip, F, tab, kw, keys3, flags=flags, bit=17)
            assert flag_word(flags) == PRESET | (1 << 17), (what, attempt)
            assert np.array_equal(o, want_o) and np.array_equal(w, want_w), (what, attempt)
            flags.free()
    tab.free()


def test_a_colliding_table_as_a_schedule_step(khip):
    """the 600-entry table (a repeated key inside the chain) and keys with both kinds of misses as a KH_STEP_LOOKUP step: the witness and the flag word of
    the direct call, which equal the expectation"""
    F, table_len, n, bit = P.Fp, 600, 130, 4
    case, tab = colliding_table(khip, F, table_len)
    rnd = random.Random(77)
    picks = [9, 23, table_len - 1] + [rnd.randrange(table_len) for _ in range(3 * n - 3)]
    keys3 = [[tab.keys[picks[3 * i + k]] for k in range(3)] for i in range(n)]
    keys3[5][2], keys3[64][0] = case.absent["head"], case.absent["mid"]
    what, kw, rows = placements(n)[0]
    want_w, want_o = expected(F, rows, keys3, tab.at)
    flags = preset_word(khip)
    direct, o = call(khip, F, tab, kw, keys3, flags=flags, bit=bit)
    assert flag_word(flags) == PRESET | (1 << bit) and np.array_equal(o, want_o) and np.array_equal(direct, want_w)
    flags.free()
    step = dict(op=khip.STEP_LOOKUP, n=n, rows=rows, param=table_len, consts=mont(F, [TABLE_ID])[0], flag_bit=bit,
                **{"in": [(2, 0), (0, 0), (1, 0)]}, out=[(khip.REF_ARENA, 0)])
    sched = khip.WitnessSchedule.create(fid(khip, F), COL_LEN, [step], arena_bytes=96 * n, n_bufs=3)
    slots = (sched.info()["run_bytes"] - 96 * n) // 4
    assert slots >= LC.slots(table_len) and slots & (slots - 1) == 0
    kd = khip.DevBuf(96 * n).upload(mont(F, [k for ks in keys3 for k in ks]))
    for attempt in range(3):
        wit, flags = sentinel_buf(khip, 15 * COL_LEN), preset_word(khip)
        sched.run([tab.k_dev, tab.v_dev, kd], wit, flags=flags)
        assert np.array_equal(wit.download((15, COL_LEN, 4)), direct), attempt
        assert flag_word(flags) == PRESET | (1 << bit), attempt
        wit.free(); flags.free()
    sched.free(); kd.free(); tab.free()
