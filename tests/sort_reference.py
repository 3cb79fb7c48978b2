"""The front half of an MSM restated in plain Python / numpy, with nothing of the library in it: signed digits (plain and GLV), the keys and entries of
the counting sort, the task plan.  tests/test_gpu_msm_sort.py compares kh_debug_msm_sort with it, exactly; tests/test_sort_reference.py pins it against brute
force on the CPU.  Also the scalar constructions both use.  The GLV split is tools/gen_glv_params.py's own integer arithmetic (params, split)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import gen_glv_params as GLV  # noqa: E402
from oracle import pasta as P  # noqa: E402

FP = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001      # scalars of Vesta (curve id 0)
FQ = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001      # scalars of Pallas (curve id 1)
R = 1 << 256
MAX_K = 256
SORT_PLAIN, SORT_FUSED, SORT_PARTITIONED = 0, 1, 2
FUSED_V, FUSED_T, FUSED_G, FUSED_B, FUSED_KPT, FUSED_C = 17, 1024, 16, 64, 2, 16


def modulus(curve):
    return FP if curve == 0 else FQ


def glv_params(curve):
    p = GLV.params(P.VESTA if curve == 0 else P.PALLAS)
    assert p["r"] == modulus(curve)
    return p


def limbs(values):
    """Python integers below 2^256 -> (n, 4) uint64"""
    return np.array([[(int(v) >> (64 * t)) & 0xffffffffffffffff for t in range(4)] for v in values], np.uint64).reshape(-1, 4)


def ints(a):
    a = np.asarray(a, np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in a]


def to_mont(values, r):
    return [v * R % r for v in values]


def canonical(values, r, mont):
    """what the digit kernels see of an input word: out of Montgomery form, or a canonical value that may carry one excess p"""
    if mont:
        rinv = pow(R, -1, r)
        return [v * rinv % r for v in values]
    assert all(v < 2 * r for v in values)
    return [v - r if v >= r else v for v in values]


# ---------------------------------------------------------------------------------- digits
def recode(values, c, W, neg=None):
    """signed c-bit digits of non-negative integers, (W, n) int64: v = window + carry; v > 2^(c-1) -> v - 2^c and carry.  neg (bool per value, GLV): a value
    that will be negated takes v >= 2^(c-1) -> v - 2^c instead, and its digits are negated.  The last carry must be zero."""
    n = len(values)
    L = np.zeros((n, 5), np.uint64)
    L[:, :4] = limbs(values)
    half, mask = 1 << (c - 1), (1 << c) - 1
    neg = np.zeros(n, bool) if neg is None else np.asarray(neg, bool)
    out = np.zeros((W, n), np.int64)
    carry = np.zeros(n, np.int64)
    for w in range(W):
        bit = c * w
        lo, sh = bit // 64, bit % 64
        if lo >= 4:
            win = np.zeros(n, np.int64)
        else:
            x = L[:, lo] >> np.uint64(sh)
            if sh + c > 64:
                x = x | (L[:, lo + 1] << np.uint64(64 - sh))
            win = (x & np.uint64(mask)).astype(np.int64)
        v = win + carry
        down = np.where(neg, v >= half, v > half)
        d = np.where(down, v - (1 << c), v)
        carry = down.astype(np.int64)
        out[w] = np.where(neg, -d, d)
    assert not carry.any(), "a carry out of the top window"
    return out


def digits(curve, words, mont, c, W, glv=False, skip=None):
    """the digit matrix (W, n) of n input words (Python integers); glv: rows 0 .. W/2 - 1 of k1, rows W/2 .. W - 1 of k2; skip: zero columns"""
    r = modulus(curve)
    can = canonical(words, r, mont)
    if glv:
        p = glv_params(curve)
        k12 = [GLV.split(p, v) for v in can]
        Wh = W // 2
        out = np.concatenate([recode([abs(k[h]) for k in k12], c, Wh, [k[h] < 0 for k in k12]) for h in (0, 1)])
    else:
        out = recode(can, c, W)
    if skip is not None:
        out[:, np.asarray(skip, bool)] = 0
    return out


# ---------------------------------------------------------------------------------- keys and entries
def keys_entries(D, nb, precomp, offset, stride, batch, wide_low=None):
    """D: (k, W, n) digits -> (key, entry) of every non-zero digit, sorted by (key, entry).  wide_low: the wide path's permutation of the bucket, per MSM"""
    k, W, n = D.shape
    j, w, i = np.nonzero(D)
    d = D[j, w, i]
    b = np.abs(d) - 1
    assert b.size == 0 or b.max() < nb
    if wide_low is not None:
        b = ((b & 255) << wide_low) | (b >> 8)
    key = (j if precomp else j * W + w) * nb + b
    entry = (offset + (w * stride if precomp else 0) + j * batch + i) | ((d < 0).astype(np.int64) << 31)
    o = np.lexsort((entry, key))
    return key[o].astype(np.int64), entry[o].astype(np.int64)


def counts_of(key, nkeys):
    return np.bincount(key, minlength=nkeys).astype(np.int64)


def exclusive(v):
    return np.concatenate([[0], np.cumsum(v)]).astype(np.int64)


def device_sorted(off, entries, nkeys):
    """the device's entries as (key of the slice they lie in, entry), sorted inside every slice"""
    cnt = np.diff(off[:nkeys + 1].astype(np.int64))
    key = np.repeat(np.arange(nkeys, dtype=np.int64), cnt)
    e = entries.astype(np.int64)
    o = np.lexsort((e, key))
    return key[o], e[o]


# ---------------------------------------------------------------------------------- tasks
def k_slot(total, nkeys):
    """4 log2(entries per key) + 8.5, whose integer part is pick_K's table slot"""
    return 4.0 * math.log2(total / nkeys) + 8.5


def pick_K(total, room, kmin, ktab, nkeys, margin=0.05):
    """pick_K of msm.hip.  The device takes the table slot from __log2f: the input must keep the slot value `margin` away from an integer wherever the two
    neighbouring slots would give another K (asserted: a property of the test's input)."""
    K = (total + room - 1) // room
    lo = kmin
    if total and nkeys:
        x = k_slot(total, nkeys)
        slot = lambda y: min(max(int(y) if y >= 0 else 0, 0), 47)
        los = {int(ktab[slot(y)]) or kmin for y in (x - margin, x, x + margin)}
        assert len(los) == 1, f"entries / keys = {total} / {nkeys}: table slot value {x:.4f} is within {margin} of a boundary that matters"
        lo, = los
    return lo if K < lo else min(K, MAX_K)


def tasks(cnt, K):
    """per key: tasks nt = ceil(count / K), their length len = ceil(count / nt); toff"""
    nt = (cnt + K - 1) // K
    ln = np.where(nt > 0, (cnt + np.maximum(nt, 1) - 1) // np.maximum(nt, 1), 0)
    return nt, ln, exclusive(nt)


def infer_K(cnt, toff):
    """the set of K in 1 .. MAX_K that give these task counts"""
    nt = np.diff(toff.astype(np.int64))
    return [K for K in range(1, MAX_K + 1) if np.array_equal((cnt + K - 1) // K, nt)]


def fused_fits(n, k, W, nb):
    """msm_plan's conditions for k_sort_fused other than precomp / wide / fused_off / M < 2^22 / CUs"""
    nkeys, tot_e = k * nb, W * n
    bpg = min(FUSED_G, FUSED_B // (2 * k))
    threads = bpg * k * 2 * FUSED_T
    kpt = (nkeys + 1 + threads - 1) // threads
    chunk4 = (tot_e // 4 + bpg - 1) // bpg + 1
    return k <= 4 and nb >= 2048 and kpt <= FUSED_KPT and n >= 4 and tot_e % 4 == 0 and chunk4 <= FUSED_V * FUSED_T and nb // 2 <= FUSED_C * FUSED_T


# ---------------------------------------------------------------------------------- scalar constructions (Python integers below r unless said)
def uniform(rng, n, r):
    return [int.from_bytes(rng.bytes(40), "little") % r for _ in range(n)]


def witness(rng, n, r):
    """the benchmark circuit's column: n - 10 ones, seven zeros, three random values"""
    return [1] * (n - 10) + [0] * 7 + uniform(rng, 3, r)


def alternating(n, a, b):
    return [a if i % 2 == 0 else b for i in range(n)]


def one_nonzero(n, at, v):
    s = [0] * n
    s[at] = v
    return s


def boundary(rng, n, r, c):
    """windows drawn from {0, 2^(c-1), 2^(c-1) + 1, 2^c - 1, random} (below bit 254, so the value is below r), behind 0, 1, r - 1, r - 2"""
    half, top = 1 << (c - 1), (1 << c) - 1
    out = [0, 1, r - 1, r - 2]
    while len(out) < n:
        v = 0
        for w in range((254 + c - 1) // c):
            pick = int(rng.integers(0, 5))
            v |= [0, half, half + 1, top, int(rng.integers(0, top + 1))][pick] << (c * w)
        out.append(v & ((1 << 254) - 1))
    return out[:n]


def carry_chain(c, W):
    """every window below the top one is 2^c - 1: the carry of window 0 runs into the top window"""
    return (1 << (c * (W - 1))) - 1


def glv_boundary(curve, c, count, seed):
    """scalars whose GLV split is a chosen (k1, k2) with k1 or k2 NEGATIVE and a window of that magnitude equal to 2^(c-1): -> [(s, k1, k2)].  The pairs
    are kept below 2^120, well inside the region the split's rounding maps back to itself; every one is confirmed with the split."""
    p = glv_params(curve)
    r, lam = p["r"], p["lam"]
    rng = np.random.default_rng(seed)
    half = 1 << (c - 1)
    out = []
    nwin = 120 // c
    while len(out) < count:
        mags = []
        for h in range(2):
            m = int.from_bytes(rng.bytes(15), "little") & ((1 << (c * nwin)) - 1)
            w = int(rng.integers(0, nwin))
            m = (m & ~(((1 << c) - 1) << (c * w))) | (half << (c * w))
            if w:                                      # no carry into the chosen window: the window below it is empty (0 + carry stays put)
                m &= ~(((1 << c) - 1) << (c * (w - 1)))
            mags.append(m)
        signs = [(-1, 1), (1, -1), (-1, -1)][len(out) % 3]
        k1, k2 = signs[0] * mags[0], signs[1] * mags[1]
        s = (k1 + k2 * lam) % r
        if GLV.split(p, s) == (k1, k2):
            out.append((s, k1, k2))
    return out
