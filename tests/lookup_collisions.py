"""Forced collisions for the lookup hash tables (csrc/lookup_hash.hpp; the tables of lookup_sorted.hip, lookup_rows.hip, witness_check.hip and
host_lookup.cpp): a mirror of the hash, the tuple hash and the capacity rule on Python integers, and searches for canonical field elements (tuples of
them) whose home slot -- hash & (slots - 1), where linear probing starts -- lies in a given set.  A helper module, no test of its own:
tests/test_lookup_hash.py holds the mirror to the C++ header output for output, so inputs made here collide in what the library compiles, not only here.

All tables probe h -> (h + 1) & (slots - 1) and hold at most slots / 2 keys.  Which slots END UP occupied does not depend on the order in which the
keys arrive (a key takes the first free slot from its home on, and the union of such walks is the same for every order), so `longest_run`, which
inserts in index order, describes the device tables too as far as the occupied set goes; which key sits in which slot does depend on the order."""
import collections
import functools

import numpy as np

M64 = (1 << 64) - 1
MUL0, MUL1, MUL2 = 0x9e3779b97f4a7c15, 0xbf58476d1ce4e5b9, 0x94d049bb133111eb
R = 1 << 256                                                   # the Montgomery radix of both fields


def key_hash(limbs):
    """hash(Key) of lookup_hash.hpp: four 64-bit limbs, least significant first"""
    l0, l1, l2, l3 = limbs
    h = (l0 * MUL0 & M64) ^ l1
    h = ((h ^ (h >> 29)) * MUL1 & M64) ^ l2
    h = ((h ^ (h >> 32)) * MUL2 & M64) ^ l3
    return h ^ (h >> 31)


def tuple_hash(tid, k1, k2, k3):
    """hash(Tuple) of lookup_hash.hpp: the table id and three entries, each four limbs; 32 bits"""
    h = key_hash(tid)
    for k in (k1, k2, k3):
        h = ((h ^ (h >> 27)) * MUL0 + key_hash(k)) & M64
    return (h ^ (h >> 32)) & 0xffffffff


def slots(L):
    """lookup_slots(L): a power of two, at least 16 and at least 2 L"""
    cap = 16
    while cap < 2 * L:
        cap <<= 1
    return cap


def mont_limbs(F, x):
    """the canonical Montgomery limbs of the field element x, as the library stores it"""
    m = x % F.p * R % F.p
    return tuple((m >> (64 * i)) & M64 for i in range(4))


def home(key, L):
    """the home slot of a key (four limbs) in a table of L entries.  (The kernels cut the hash to 32 bits first: slots(L) <= 2^32, the same slot.)"""
    return key_hash(key) & (slots(L) - 1)


def tuple_home(tid, k1, k2, k3, L):
    return tuple_hash(tid, k1, k2, k3) & (slots(L) - 1)


# ---- the search.  One candidate in slots / len(homes) qualifies, about a million hashes for 1024 keys at 2048 slots: the hashes of the Montgomery forms of
# x = 1, 2, .. are computed once per field in numpy's wrapping 64-bit arithmetic and kept; every element handed out is confirmed with key_hash itself.
_CHUNK = 1 << 16
_hashes = {}                                                   # p -> [numpy uint64 arrays of _CHUNK hashes: x = 1 + chunk * _CHUNK + i]


def _hash_chunk(p, chunk):
    got = _hashes.setdefault(p, [])
    while len(got) <= chunk:
        x0 = 1 + len(got) * _CHUNK
        m, step, raw = x0 * R % p, R % p, []
        for _ in range(_CHUNK):
            raw.append(m.to_bytes(32, "little"))
            m += step
            if m >= p:
                m -= p
        l = np.frombuffer(b"".join(raw), dtype=np.uint64).reshape(_CHUNK, 4)
        h = l[:, 0] * np.uint64(MUL0) ^ l[:, 1]
        h = (h ^ (h >> np.uint64(29))) * np.uint64(MUL1) ^ l[:, 2]
        h = (h ^ (h >> np.uint64(32))) * np.uint64(MUL2) ^ l[:, 3]
        got.append(h ^ (h >> np.uint64(31)))
    return got[chunk]


@functools.lru_cache(maxsize=None)
def _colliders(p, L, homes, count, exclude):
    class F:
        pass
    F.p = p
    mask, out, chunk = slots(L) - 1, [], 0
    wanted = np.array(sorted(homes), dtype=np.uint64)
    while len(out) < count:
        h = _hash_chunk(p, chunk) & np.uint64(mask)
        for i in np.flatnonzero(np.isin(h, wanted)):
            x = 1 + chunk * _CHUNK + int(i)
            if x in exclude:
                continue
            assert x < p and home(mont_limbs(F, x), L) in homes   # what counts is the mirror the C++ test pins, not the numpy copy above
            out.append(x)
            if len(out) == count:
                break
        chunk += 1
    return tuple(out)


def colliders(F, L, homes, count, exclude=()):
    """the first `count` field elements x = 1, 2, .. (integers below F.p, none of `exclude`) whose Montgomery limbs have their home slot, in a table
    of L entries, in `homes`"""
    return list(_colliders(F.p, L, frozenset(homes), count, frozenset(exclude)))


def tuple_colliders(F, tid, L, homes, count, exclude=(), entry=lambda x: (x, x * x + 3, 0)):
    """the same for tuples with a fixed table id: the first `count` x = 1, 2, .. (none of `exclude`) for which the tuple (tid,) + entry(x), every part
    as Montgomery limbs, has its home slot in `homes`.  Returns the x."""
    homes = frozenset(homes)
    t, out, x = mont_limbs(F, tid), [], 0
    while len(out) < count:
        x += 1
        if x not in exclude and tuple_home(t, *(mont_limbs(F, v) for v in entry(x)), L) in homes:
            out.append(x)
    return out


Run = collections.namedtuple("Run", "slots wraps displacement occupied")


def longest_run(homes, cap):
    """linear probing of keys with these home slots, inserted in index order (one home per DISTINCT key).  Returns
         slots         the longest cyclic run of occupied slots, in walking order
         wraps         the run holds slot cap - 1 and slot 0: walking it steps cap - 1 -> 0 between two occupied slots.  (A run of one slot, [cap - 1],
                       counts as well: the walk that leaves it for the empty slot behind makes that step)
         displacement  the largest distance between a key's slot and its home
         occupied      every occupied slot
       slots, wraps and occupied hold for any arrival order; the displacement is this order's, but the key in the last slot of a run that starts at the
       lowest home is displaced by at least len(run) - (number of distinct homes) whatever the order."""
    assert len(homes) <= cap // 2 and cap & (cap - 1) == 0
    mask, taken, disp = cap - 1, set(), 0
    for h in homes:
        assert 0 <= h < cap
        s = h
        while s in taken:
            s = (s + 1) & mask
        taken.add(s)
        disp = max(disp, (s - h) & mask)
    best = []
    for s in sorted(taken):
        if (s - 1) & mask in taken:
            continue                                            # not the start of a run
        run = [s]
        while (run[-1] + 1) & mask in taken:
            run.append((run[-1] + 1) & mask)
        if len(run) > len(best):
            best = run
    wraps = best == [mask] or any(a == mask and b == 0 for a, b in zip(best, best[1:]))
    return Run(best, wraps, disp, frozenset(taken))
