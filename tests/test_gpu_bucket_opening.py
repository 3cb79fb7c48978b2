"""The first addition of a bucket in the MSM accumulation kernels (csrc/msm.hip: wide_task29 of k_acc_wide29 / k_acc_wide_rest, and k_accumulate29): a task
of two or more entries opens with the affine + affine addition aadd29 (csrc/field29.cuh) on entries 0 and 1 and runs madd29 from entry 2; a task of one
entry converts its point as before.  Every result bit-exact against the C oracle, on both curves.

The scalars are put together from the signed window digits d_w in (-2^(c-1), 2^(c-1)] that the device's decomposition gives back (it is unique; _digits
below restates it and every test checks its input with it): digit d of scalar i in window w puts the table point 2^(c w) G_i, negated for d < 0, into bucket
|d| of the one bucket group that the windows of a table set share.  That decides how many entries every bucket holds and which points meet in it; the order
of a bucket's entries is the sort's, so the cases below hold for every order."""
import os
from collections import Counter

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu
THREADS = min(64, os.cpu_count() or 8)
WIDE_C, NARROW_C = 20, 16


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    k.set_wide_min_n(1 << 12)
    yield k
    k.set_wide_min_n(1 << 19)


def _digits(v, c):
    """signed c-bit window digits of the canonical scalar v, lowest window first (emit_digits of csrc/msm.hip)"""
    out, carry = [], 0
    for _ in range((255 + c - 1) // c):
        d = (v & ((1 << c) - 1)) + carry
        v >>= c
        carry = 1 if d > (1 << (c - 1)) else 0
        out.append(d - (carry << c))
    assert v == 0 and carry == 0
    return out


def _scalar(digs, c):
    """{window: signed digit} -> the scalar; the highest digit must be positive"""
    v = sum(d << (c * w) for w, d in digs.items())
    assert 0 < v < (1 << 254)
    got = _digits(v, c)
    assert all(got[w] == digs.get(w, 0) for w in range(len(got)))
    return v


def _bucket_sizes(vals, c):
    cnt = Counter()
    for v in vals:
        for d in _digits(v, c):
            if d:
                cnt[abs(d)] += 1
    return cnt


def _wide_ran(khip):
    return any(name == "reduce_a1" for name, _ in khip.last_timings())


def _run(khip, cid, g, vals, wide):
    """one MSM of the canonical scalars vals over the basis g, through a handle of its own and through the device-resident entry point, against the oracle"""
    sc = cref.ints_to_limbs(vals)
    want, winf = cref.msm(cid, g, sc, scalars_mont=False, threads=THREADS)
    srs = khip.Srs(cid, g)
    got, ginf = srs.msm(sc, mont=False)
    assert _wide_ran(khip) == wide, "the MSM did not take the table set this test is about"
    buf = khip.DevBuf(sc.nbytes).upload(sc)
    got2, ginf2 = srs.msm_batch_dev(buf.ptr, len(vals), 1, mont=False)
    buf.free(); srs.close()
    assert bool(ginf) == winf and (winf or np.array_equal(got, want))
    assert bool(ginf2[0]) == winf and (winf or np.array_equal(got2[0], want))


def _neg(cid, pt):
    fid = 1 if cid == 0 else 0                       # the base field of Vesta is Fq, of Pallas Fp
    out = pt.copy()
    out[4:] = cref.field_op(fid, "sub", np.zeros((1, 4), np.uint64), pt[4:].reshape(1, 4))[0]
    return out


class _Plan:
    """collects (bucket, sign) entries into scalars: a positive entry is a scalar of one digit, a negative one gets a positive digit one window up whose
    bucket nothing else uses (a bucket of one entry)"""

    def __init__(self, c, rng, first_free):
        self.c, self.rng, self.free, self.vals = c, rng, first_free, []
        self.top = 255 // c - 1                      # highest window that holds a full digit, minus the one a companion digit needs

    def fresh(self):
        self.free += 1
        return self.free

    def entry(self, bucket, negative, window=None):
        """returns the index of the scalar (= of the basis point) that carries the entry"""
        w = int(self.rng.integers(0, self.top)) if window is None else window
        digs = {w: -bucket, w + 1: self.fresh()} if negative else {w: bucket}
        self.vals.append(_scalar(digs, self.c))
        return len(self.vals) - 1

    def pad(self, n):
        assert len(self.vals) <= n, len(self.vals)
        self.vals += [0] * (n - len(self.vals))
        return self.vals


def _chains(c, n, nset, rng):
    """n scalars whose digits come from a set of nset bucket numbers, signs at random (the top window: small and positive)"""
    half = 1 << (c - 1)
    W = (255 + c - 1) // c
    topmax = 1 << (254 - c * (W - 1) - 1)
    small = rng.choice(np.arange(1, topmax), size=nset // 2, replace=False)
    large = rng.choice(np.arange(topmax, half + 1), size=nset - nset // 2, replace=False)
    mags = np.concatenate([small, large])
    vals = []
    for _ in range(n):
        digs = {w: int(rng.choice(mags)) * (1 if rng.integers(0, 2) else -1) for w in range(W - 1)}
        digs[W - 1] = int(rng.choice(small))
        vals.append(_scalar(digs, c))
    return vals


@pytest.mark.parametrize("cid", [0, 1])
def test_wide_chains_of_flagship_length(khip, cid):
    """2^12 scalars, 20-bit digits from 2^11 values: 13 x 2^12 entries in at most 2^11 buckets, ~26 per bucket as at 2^20 uniform scalars"""
    n = 1 << 12
    vals = _chains(WIDE_C, n, 1 << 11, np.random.default_rng(40 + cid))
    sizes = _bucket_sizes(vals, WIDE_C)
    assert 2 * sum(1 for k in sizes.values() if k >= 2) >= len(sizes) and sum(sizes.values()) == 13 * n and len(sizes) <= 1 << 11
    _run(khip, cid, khip.srs_generate(cid, 0, n), vals, wide=True)


def _short_buckets(c, n, rng, reps):
    """buckets of exactly 1, 2 and 3 entries; the first two entries of the 2- and 3-entry buckets in all four sign combinations"""
    plan = _Plan(c, rng, first_free=1 << 10)
    want = {}
    b = 0
    for rep in range(reps):
        for s1 in (False, True):
            for s2 in (False, True):
                for size in (2, 3):
                    b += 1
                    plan.entry(b, s1); plan.entry(b, s2)
                    if size == 3:
                        plan.entry(b, bool(rng.integers(0, 2)))
                    want[b] = size
        b += 1
        plan.entry(b, False)
        want[b] = 1
    assert b < (1 << 10)
    vals = plan.pad(n)
    sizes = _bucket_sizes(vals, c)
    assert all(sizes[k] == v for k, v in want.items()) and all(v == 1 for k, v in sizes.items() if k not in want)
    assert {1, 2, 3} == set(sizes.values())
    return vals


@pytest.mark.parametrize("cid", [0, 1])
def test_wide_buckets_of_one_two_and_three_entries(khip, cid):
    n = 1 << 12
    vals = _short_buckets(WIDE_C, n, np.random.default_rng(50 + cid), reps=100)
    _run(khip, cid, khip.srs_generate(cid, 0, n), vals, wide=True)


def _refusals(khip, cid, c, n, rng, reps):
    """A basis with repeated and related points, and scalars that bring them together in one bucket and one window:
    P, P            the opening is refused, the exact path doubles;
    P, -P           refused, the bucket is the identity;
    A, B, -(A + B)  in every order the opening is fine and the third entry meets its opposite: refused there, the bucket is the identity;
    A, B, A + B     refused at the third entry when that is A + B's turn, fine otherwise;
    P, P, Q         and a repeated point with company."""
    g = khip.srs_generate(cid, 0, n)
    plan = _Plan(c, rng, first_free=1 << 10)
    b = 0

    def same_window(bucket, signs):
        w = int(rng.integers(0, plan.top))
        return [plan.entry(bucket, s, window=w) for s in signs]

    for rep in range(reps):
        b += 1; i, j = same_window(b, (False, False)); g[j] = g[i]
        b += 1; i, j = same_window(b, (True, True)); g[j] = g[i]
        b += 1; i, j = same_window(b, (False, True)); g[j] = g[i]
        b += 1; i, j = same_window(b, (False, False)); g[j] = _neg(cid, g[i])
        b += 1; i, j, k = same_window(b, (False, False, True))
        s, sinf = cref.point_add(cid, g[i], g[j]); assert not sinf
        g[k] = s                                                   # entered negated: -(A + B)
        b += 1; i, j, k = same_window(b, (False, False, False))
        g[k] = _neg(cid, cref.point_add(cid, g[i], g[j])[0])
        b += 1; i, j, k = same_window(b, (False, True, False))
        g[k] = cref.point_add(cid, g[i], _neg(cid, g[j]))[0]       # A, -B, A - B
        b += 1; i, j, k = same_window(b, (False, False, False)); g[j] = g[i]
    assert b < (1 << 10)
    return g, plan.pad(n)


@pytest.mark.parametrize("cid", [0, 1])
def test_wide_refused_openings_and_refused_third_entries(khip, cid):
    n = 1 << 12
    g, vals = _refusals(khip, cid, WIDE_C, n, np.random.default_rng(60 + cid), reps=24)
    _run(khip, cid, g, vals, wide=True)


@pytest.mark.parametrize("cid", [0, 1])
def test_wide_split_buckets_open_every_chunk(khip, cid):
    """skewed scalars: a few buckets hold nearly all entries and are split into chunks, so k_acc_wide_rest runs the opening with jt > 0 (and the
    divisions that place a chunk); one in eight scalars random, so that unsplit buckets run beside them"""
    n = 1 << 12
    rng = np.random.default_rng(70 + cid)
    heavy = _chains(WIDE_C, 2, 1 << 11, rng)
    rest = _chains(WIDE_C, n // 8, 1 << 11, rng)
    vals = [rest[i // 8] if i % 8 == 0 else heavy[i % 2] for i in range(n)]
    sizes = _bucket_sizes(vals, WIDE_C)
    assert max(sizes.values()) >= n // 4 and min(sizes.values()) <= 4
    _run(khip, cid, khip.srs_generate(cid, 0, n), vals, wide=True)


# ---- the narrow path: k_accumulate29 over the tables at c = 16, fewer scalars than the wide threshold
@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("logn", [10, 11])
def test_narrow_chains(khip, cid, logn):
    n = 1 << logn
    vals = _chains(NARROW_C, n, 1 << (logn - 1), np.random.default_rng(80 + cid + logn))
    sizes = _bucket_sizes(vals, NARROW_C)
    assert 2 * sum(1 for k in sizes.values() if k >= 2) >= len(sizes)
    _run(khip, cid, khip.srs_generate(cid, 0, n), vals, wide=False)


@pytest.mark.parametrize("cid", [0, 1])
def test_narrow_buckets_of_one_two_and_three_entries(khip, cid):
    n = 1 << 11
    vals = _short_buckets(NARROW_C, n, np.random.default_rng(90 + cid), reps=60)
    _run(khip, cid, khip.srs_generate(cid, 0, n), vals, wide=False)


@pytest.mark.parametrize("cid", [0, 1])
def test_narrow_refused_openings_and_refused_third_entries(khip, cid):
    n = 1 << 11
    g, vals = _refusals(khip, cid, NARROW_C, n, np.random.default_rng(100 + cid), reps=24)
    _run(khip, cid, g, vals, wide=False)
