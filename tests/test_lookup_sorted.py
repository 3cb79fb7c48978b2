"""kh_lookup_sorted (csrc/host_lookup.cpp) -- the `sorted` step of the lookup argument, kimchi/src/circuits/lookup/constraints.rs:90-194, as native
host code -- against the oracle's restatement of the same function (oracle/lookup.py::sorted_columns' counting and snake layout, here on opaque
32-byte values): tables with repeated entries, the dummy value, 1 to 4 lookups per row, a looked-up value that is not in the table.  No GPU.

The second half holds the same function to the same reference on tables whose keys are MADE to collide (tests/lookup_collisions.py: field elements whose
home slots are the last two of the slot array), so that the whole table is one probe chain that wraps from the last slot to slot 0 -- random keys at
half load give chains of one or two slots.  collision_case() is also what tests/test_gpu_lookup_sorted_dev.py runs on the device."""
import collections
import functools
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_collisions as LC  # noqa: E402


def reference_sorted(table, values, lookup_rows, mpr):
    """the reference's algorithm on hashable values: counts over the table (a repeated entry counts once), every entry repeated count times in
    table order, cut into mpr + 1 columns sharing one element, odd columns reversed"""
    counts = {}
    for t in table[:lookup_rows]:
        counts.setdefault(t, 1)
    for r in range(lookup_rows):
        for s in range(mpr):
            v = values[s][r]
            if v not in counts:
                raise ValueError(r)
            counts[v] += 1
    cols = [[] for _ in range(mpr + 1)]
    i = 0
    for t in table[:lookup_rows]:
        c = counts[t]
        counts[t] = 1
        for j in range(c):
            cols[(i + j) // lookup_rows].append(t)
        i += c
    for k in range(mpr):
        cols[k].append(cols[k + 1][0])
    cols[mpr].append(cols[mpr][-1])
    for k in range(1, mpr + 1, 2):
        cols[k].reverse()
    return cols


@pytest.mark.parametrize("lookup_rows,distinct,mpr", [(1, 1, 1), (12, 5, 3), (60, 60, 4), (500, 37, 3), (4092, 1500, 4), (300, 299, 1)])
def test_sorted_columns_equal_the_reference_algorithm(lookup_rows, distinct, mpr):
    import proof_systems_amd.khip as khip
    rnd = random.Random(1000 * lookup_rows + mpr)
    n = lookup_rows + 4                                         # the arrays are longer than the rows used (zero-knowledge rows behind them)
    pool = [(0, 0, 0, 0)] + [tuple(rnd.getrandbits(64) for _ in range(4)) for _ in range(distinct - 1)]
    table = [pool[k] if k < distinct else pool[rnd.randrange(distinct)] for k in range(lookup_rows)] + [tuple(rnd.getrandbits(64) for _ in range(4)) for _ in range(4)]
    values = [[pool[rnd.randrange(distinct)] if rnd.random() < 0.8 else (0, 0, 0, 0) for _ in range(n)] for _ in range(mpr)]
    want = reference_sorted(table, values, lookup_rows, mpr)
    got = khip.lookup_sorted(np.array(table, dtype=np.uint64), lookup_rows, np.array(values, dtype=np.uint64), mpr)
    assert got.shape == (mpr + 1, lookup_rows + 1, 4)
    assert [[tuple(int(x) for x in v) for v in col] for col in got] == want
    # a value outside the table: the row comes back, as ProverError::ValueNotInTable(row)
    bad_row = rnd.randrange(lookup_rows)
    values[mpr - 1][bad_row] = (1, 2, 3, 4)
    with pytest.raises(ValueError) as e:
        khip.lookup_sorted(np.array(table, dtype=np.uint64), lookup_rows, np.array(values, dtype=np.uint64), mpr)
    assert e.value.args[0] == bad_row
    # ... but only rows below lookup_rows are looked at
    values[mpr - 1][bad_row] = (0, 0, 0, 0)
    values[0][lookup_rows] = (9, 9, 9, 9)
    khip.lookup_sorted(np.array(table, dtype=np.uint64), lookup_rows, np.array(values, dtype=np.uint64), mpr)


# ---------------------------------------------------------------------------------------------------------------- forced collisions
COLLISION_SIZES = (1, 2, 7, 8, 48, 600, 1024)                  # 8 and 1024: exactly half load (slots = 2 L), one run of L slots that starts at the end of the array
COLLISION_CASES = [(L, False) for L in COLLISION_SIZES] + [(48, True)]
CollisionCase = collections.namedtuple("CollisionCase", "table values misses run distinct keys absent")


@functools.lru_cache(maxsize=None)
def collision_case(F, lookup_rows, mpr, merge=False):
    """a table of lookup_rows entries (Montgomery limbs of elements of F) that is ONE probe chain across the end of the slot array, values drawn from it,
    and absent values that must walk that chain: .misses = (("head", limbs), ("mid", limbs), ("limb0", limbs), ..); .keys and .absent hold the same elements as integers.

    merge = False   every home slot is cap - 2 or cap - 1 (cap - 1 alone for one or two entries, so that two entries already reach slot 0).  In the 48
                    and 600 cases entries 9, 23 and L - 1 hold the same key, with other keys of the chain between them, and about a third of the values
                    look that key up: its counts belong to entry 9, and counts that go to entry 23 or L - 1 shift everything behind
    merge = True    two clusters, homes cap - 4 .. cap - 1 and 0 .. 1 (the dummy value 0 among them: its limbs and its hash are zero): the first spills
                    over the wrap into the second's home slots and pushes its keys along
    The preconditions are asserted here, on the mirror's home slots of the table's distinct keys: every home in the target set; the occupied slots are one
    run that holds the last slot and slot 0; the largest displacement (index order) is at least distinct - (number of target slots) -- the key in the run's
    last slot cannot be nearer to a home, in any order.  (With every key distinct and two target slots that is L - 2; the repeated key of the 48 and 600
    cases takes one slot, so the chain has L - 2 slots and no key can be displaced by more than L - 3.)"""
    L, cap = lookup_rows, LC.slots(lookup_rows)
    mask = cap - 1
    rnd = random.Random(7000 * L + 10 * mpr + merge)
    repeated = L in (48, 600) and not merge
    distinct = L - 2 if repeated else L
    if merge:
        targets = set(range(cap - 4, cap)) | {0, 1}
        keys = LC.colliders(F, L, range(cap - 4, cap), distinct // 2) + [0] + LC.colliders(F, L, {0, 1}, distinct - distinct // 2 - 1)
    else:
        targets = {cap - 1} if L <= 2 else {cap - 2, cap - 1}
        keys = LC.colliders(F, L, targets, distinct)
    rnd.shuffle(keys)                                          # table order is not value order
    if repeated:
        keys.insert(23, keys[9]); keys.append(keys[9])
        assert keys[9] == keys[23] == keys[L - 1] and len(set(keys[10:23])) == 13 and keys[9] not in keys[10:23] + keys[24:L - 1]
    assert len(keys) == L and len(set(keys)) == distinct
    table = [LC.mont_limbs(F, x) for x in keys]
    homes = [LC.home(k, L) for k in dict.fromkeys(table)]
    run = LC.longest_run(homes, cap)
    assert set(homes) <= targets and 2 * distinct <= cap
    assert len(run.slots) == distinct and run.occupied == set(run.slots), "the table is not one chain"
    assert run.wraps and mask in run.occupied and (L == 1 or 0 in run.occupied), "the chain does not cross the end of the slot array"
    assert run.displacement >= distinct - len(targets), run.displacement
    hot = table[9] if repeated else None
    # the first column looks every entry up once, but for two fifths of its rows in the tables of more than 8 entries, which draw like the further columns: any entry, or -- three times in ten
    # where a key is repeated -- that key.  So nearly every slot of the chain is reached from a home in front of it, and the counts differ
    draw = lambda: hot if repeated and rnd.random() < 0.3 else rnd.choice(table)
    cover = list(table)
    rnd.shuffle(cover)
    values = [[draw() if s or (L > 8 and rnd.random() < 0.4) else cover[r] for r in range(L)] for s in range(mpr)]
    if repeated:
        assert sum(col.count(hot) for col in values) >= L // 16
    assert (0, 0, 0, 0) not in table or merge                  # the dummy value 0 is looked up only where the table holds it
    # absent values: home = the head of the chain (walks every slot of it, the wrap included), home = the middle of the part behind the wrap
    behind = run.slots[run.slots.index(mask) + 1:]
    wanted = [("head", run.slots[0])] + ([("mid", behind[len(behind) // 2])] if behind else [])
    absent = {name: LC.colliders(F, L, {slot}, 1, exclude=keys)[0] for name, slot in wanted}
    misses = [(name, LC.mont_limbs(F, x)) for name, x in absent.items()]
    # ... and, per limb, a value that differs from a table entry in THAT limb only and whose home is the head of the chain: its walk passes the entry
    # it nearly equals, which a comparison that skips a limb would take for it.  (32 opaque bytes to the join; not canonical, so not in .absent)
    near = table[L // 2]
    for j in range(4):
        t = next(t for t in range(1, 1 << 20) if t != near[j] and LC.home(near[:j] + (t,) + near[j + 1:], L) == run.slots[0])
        misses.append(("limb%d" % j, near[:j] + (t,) + near[j + 1:]))
    misses = tuple(misses)
    assert all(m not in table for _n, m in misses) and len(misses) == (5 if L == 1 else 6)
    return CollisionCase(tuple(table), tuple(tuple(col) for col in values), misses, run, distinct, tuple(keys), absent)


def miss_rows(lookup_rows):
    """where the tests put the absent values, one at a time: the head-of-chain one in a middle row, the mid-chain one in the last row, .."""
    return {"head": 5 * lookup_rows // 7, "mid": lookup_rows - 1, "limb0": 0, "limb1": lookup_rows // 3, "limb2": lookup_rows // 2, "limb3": lookup_rows - 1}


def with_value(values, s, r, v):
    out = [list(col) for col in values]
    out[s][r] = v
    return out


@pytest.mark.parametrize("mpr", (1, 3))
@pytest.mark.parametrize("lookup_rows,merge", COLLISION_CASES)
def test_colliding_tables_equal_the_reference_algorithm(lookup_rows, merge, mpr):
    import proof_systems_amd.khip as khip
    from oracle import pasta as P
    case = collision_case(P.Fp, lookup_rows, mpr, merge)
    table, values = list(case.table), [list(col) for col in case.values]
    want = reference_sorted(table, values, lookup_rows, mpr)
    got = khip.lookup_sorted(np.array(table, dtype=np.uint64), lookup_rows, np.array(values, dtype=np.uint64), mpr)
    assert got.shape == (mpr + 1, lookup_rows + 1, 4)
    assert [[tuple(int(x) for x in v) for v in col] for col in got] == want
    for name, absent in case.misses:
        row = miss_rows(lookup_rows)[name]
        bad = with_value(values, mpr - 1, row, absent)
        with pytest.raises(ValueError) as ref:
            reference_sorted(table, bad, lookup_rows, mpr)
        with pytest.raises(ValueError) as e:
            khip.lookup_sorted(np.array(table, dtype=np.uint64), lookup_rows, np.array(bad, dtype=np.uint64), mpr)
        assert e.value.args[0] == ref.value.args[0] == row, name
