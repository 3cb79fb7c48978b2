"""Inputs and expected values for the MSM's bucket-sum stage and reduction tails (csrc/msm.hip, "6 bucket sums" and "7 reduce"), shared by
tests/test_reduction_reference.py (CPU) and tests/test_gpu_reduction_tails.py.

Every record is m G for a small known m: a palette of m in -3 .. 3, 0 being the all-zero identity record, G the first SRS point of the curve.  A non-zero
entry is held in three XYZZ representations (x l^2 | y l^3 | l^2 | l^3: l = 1 and two random l), so records that are equal as group elements need not be
equal as bytes.  The expected value of any weighted sum of records is then ONE scalar multiplication, (sum w_i m_i mod r) G -- no tree, no tail, nothing
of the code under test.  tests/test_reduction_reference.py pins that against literal point additions.

The geometry of the marginal tail is restated here (MargGeom, marginal_bucket of csrc/msm_plan.hpp); the same CPU test holds the restatement to the header's
own functions, compiled on the host."""
import numpy as np

from oracle import cref
from oracle import pasta as P

REPS = 3


def order(cid):
    """the group order: Vesta's scalars are Fp, Pallas's Fq"""
    return P.Fp.p if cid == 0 else P.Fq.p


class Palette:
    def __init__(self, cid, seed=2024):
        self.cid, self.r, self.fid = cid, order(cid), 1 - cid                       # fid: the base field of the curve's coordinates
        self.g = cref.srs_generate(cid, 0, 1)[0]
        rng = np.random.default_rng(seed + cid)
        lam = rng.integers(0, 1 << 64, size=(REPS, 4), dtype=np.uint64)
        lam[:, 3] &= np.uint64((1 << 61) - 1)                                       # any value below the modulus is a Montgomery element
        lam[0] = cref.field_op(self.fid, "to_mont", cref.ints_to_limbs([1]))[0]
        assert all(any(int(w) for w in l) for l in lam)
        self.affine = {}                                                            # m -> affine m G
        self.table = np.zeros((7, REPS, 16), dtype=np.uint64)                       # [m + 3][representation] -> record; row 3 (m = 0) stays zero
        for m in (-3, -2, -1, 1, 2, 3):
            xy, inf = cref.point_mul(cid, self.g, cref.ints_to_limbs([m % self.r])[0], scalar_mont=False)
            assert not inf
            self.affine[m] = xy
            for k in range(REPS):
                l2 = cref.field_op(self.fid, "mul", lam[k], lam[k]); l3 = cref.field_op(self.fid, "mul", l2, lam[k])
                self.table[m + 3, k, 0:4] = cref.field_op(self.fid, "mul", xy[:4], l2)[0]
                self.table[m + 3, k, 4:8] = cref.field_op(self.fid, "mul", xy[4:], l3)[0]
                self.table[m + 3, k, 8:12] = l2[0]; self.table[m + 3, k, 12:16] = l3[0]
        self._expect = {}

    def records(self, ms, reps=None):
        """(n, 16) records of the palette values ms; reps: the representation of each (default: rotating with the index)"""
        ms = np.asarray(ms, dtype=np.int64).reshape(-1)
        assert ms.size == 0 or (ms.min() >= -3 and ms.max() <= 3)
        reps = np.arange(ms.size) % REPS if reps is None else np.asarray(reps, dtype=np.int64).reshape(-1)
        return self.table[ms + 3, reps]

    def expect(self, total):
        """(affine limbs, infinity) of total G"""
        s = int(total) % self.r
        if s not in self._expect:
            self._expect[s] = (np.zeros(8, np.uint64), True) if s == 0 else cref.point_mul(self.cid, self.g, cref.ints_to_limbs([s])[0], scalar_mont=False)
        return self._expect[s]

    def same(self, got, ginf, total):
        want, winf = self.expect(total)
        return bool(ginf) == bool(winf) and (bool(winf) or np.array_equal(np.asarray(got).reshape(8), want))


# ---- the geometry of the marginal tail (msm_plan.hpp: marginal_geometry, marginal_bucket)
def geometry(c):
    """(nb, shifts, widths) of the three digit fields of a bucket index at window width c"""
    bits = c - 1
    f0 = (bits + 2) // 3; f1 = (bits - f0 + 1) // 2; f2 = bits - f0 - f1
    return 1 << bits, (0, f0, f0 + f1), (f0, f1, f2)


def marginal_bucket(c, j, v, e):
    """the bucket whose digit j is v and whose other bits are e"""
    _nb, sh, wd = geometry(c)
    s, f = sh[j], wd[j]
    return ((e >> s) << (s + f)) | (v << s) | (e & ((1 << s) - 1))


def plane_weights(c):
    """(3, nb): the weight of bucket t in plane j, digit_j(t) + [j == 0]"""
    nb, sh, wd = geometry(c)
    t = np.arange(nb, dtype=np.int64)
    return np.stack([((t >> sh[j]) & ((1 << wd[j]) - 1)) + (1 if j == 0 else 0) for j in range(3)])


def plane_totals(c, ms, groups):
    """(groups, 3) integers: sum_t weight_j(t) m_t"""
    return np.asarray(ms, dtype=np.int64).reshape(groups, -1) @ plane_weights(c).T


def segment_totals(nb, ms, groups):
    """(groups,) integers: sum_t (t + 1) m_t"""
    return np.asarray(ms, dtype=np.int64).reshape(groups, nb) @ (np.arange(nb, dtype=np.int64) + 1)


# ---- bucket contents, as palette values (groups * nb,)
def single(nb, ts, ms=None):
    """one group per t of ts: bucket t holds a non-zero value, every other bucket the identity"""
    out = np.zeros((len(ts), nb), dtype=np.int64)
    for q, t in enumerate(ts):
        out[q, t] = (1, -2, 3, -1, 2, -3)[q % 6] if ms is None else ms[q]
    return out.reshape(-1)


def all_equal(nb, groups):
    """every bucket of group q holds the same group element (the caller rotates the representations): every tree level is a doubling"""
    return np.repeat(np.array([(1, -2, 3)[q % 3] for q in range(groups)], dtype=np.int64), nb)


def palette(nb, groups, seed):
    return np.random.default_rng(seed).integers(-3, 4, size=groups * nb).astype(np.int64)


def zero_sum(n, rng):
    """n (even) non-zero palette values that sum to zero, shuffled"""
    assert n % 2 == 0
    half = rng.choice(np.array([-3, -2, -1, 1, 2, 3]), size=n // 2)
    v = np.concatenate([half, -half]); rng.shuffle(v)
    return v.astype(np.int64)


def first_summed(tail, cnt):
    """The e < cnt of a marginal whose sum a kernel holds before it meets the rest (tail as in kh_debug_bucket_tail; thread / quad i takes e = i, i + stride, ..):
    1  k_marginals_q: 64 quads, the first wave = quads 0 .. 15;    2  k_marginals_h: 256 threads, the first wave = threads 0 .. 63;
    0  k_marginals is ONE wave, so there the set is lanes 0, 4, 8, .. of it: lane 0 holds their sum after the shuffle tree's level d = 4, two levels from the end."""
    pick = {0: lambda e: e % 64 % 4 == 0, 1: lambda e: e % 64 < 16, 2: lambda e: e % 256 < 64}[tail]
    return [e for e in range(cnt) if pick(e)]


def cancel(c, groups, first, seed):
    """Palette contents in which the buckets marginal_bucket(c, 0, 0, e), e in `first`, -- those a kernel sums before it meets the rest of the marginal v = 0
    of plane 0 -- hold non-zero values that sum to zero, while the marginal as a whole does not: a partial sum passes through the identity mid-tree."""
    nb, _sh, wd = geometry(c)
    cnt = nb >> wd[0]
    rng = np.random.default_rng(seed)
    out = rng.integers(-3, 4, size=(groups, nb)).astype(np.int64)
    first = sorted(first)
    assert 0 < len(first) < cnt and all(0 <= e < cnt for e in first)
    rest = [e for e in range(cnt) if e not in set(first)]
    for q in range(groups):
        out[q, [marginal_bucket(c, 0, 0, e) for e in first]] = zero_sum(len(first), rng)
        out[q, [marginal_bucket(c, 0, 0, e) for e in rest]] = rng.choice(np.array([1, 2, 3]), size=len(rest))      # positive: their sum is not zero
    return out.reshape(-1)


def cancel_holds(c, ms, groups, first):
    """the property cancel() promises, from the contents alone"""
    nb, _sh, wd = geometry(c)
    m = np.asarray(ms).reshape(groups, nb)
    inside = [marginal_bucket(c, 0, 0, e) for e in first]
    whole = [marginal_bucket(c, 0, 0, e) for e in range(nb >> wd[0])]
    return all((m[q, inside] != 0).all() and m[q, inside].sum() == 0 and m[q, whole].sum() != 0 for q in range(groups))
