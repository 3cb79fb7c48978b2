"""The tail of the wide-window MSM (csrc/msm.hip: k_wide_a1 -> k_wide_l2 -> k_wide_a2), bit-exact against oracle.cref.msm.

The 2^19 buckets of the 20-bit windows, and with them the whole geometry of the tail, do not depend on the number of scalars: bucket
t = (a, b), a = its top 9 bits, b = its low 10, goes into the hi-digit marginal H_a and the lo-digit marginal L_b.  Level one sums chunks of 16
buckets of a marginal, level two runs of 4 chunk records (64 buckets), k_wide_a2 the last 16 (H_a) or 8 (L_b) run records.  Every input here is BUILT so
that named records of that geometry are the occupied ones, and the construction is checked on the CPU (the signed digits of every scalar, the
reference result as the expected multiple of one point) before the GPU runs: the construction, not a counter, is what says that a path was taken.

A digit d != 0 of window w puts the point 2^(20 w) P into bucket |d| - 1.  The thirteenth window holds bits 240..254 of a scalar below the 255-bit
group order, so no scalar has thirteen digits of one value beyond 2^14: the placed scalars repeat d over the TWELVE full windows and leave the
thirteenth empty (a zero digit touches no bucket).  A negative digit needs its carry: -e in windows 0..11 comes with +1 in window 12, so such an MSM
occupies bucket e - 1 and bucket 0 (one entry per point); -2^19 is no digit at all (digits lie in (-2^19, 2^19]), so t = 2^19 - 1 is placed
with the positive sign only."""
import numpy as np
import pytest

from oracle import cref
from oracle import pasta as P

pytestmark = pytest.mark.gpu
N = 1 << 12
C, W = 20, 13
LO, HI, RLOG, FLOG = 10, 9, 4, 2          # msm.hip: WideGeom of c = 20
REP12 = sum(1 << (C * w) for w in range(12))


def _order(cid):
    return P.Fp.p if cid == 0 else P.Fq.p


def digits(s):
    """signed 20-bit digits of the canonical scalar s, in (-2^19, 2^19] (msm.hip, emit_digits)"""
    out, carry = [], 0
    for w in range(W):
        v = ((s >> (C * w)) & ((1 << C) - 1)) + carry
        carry = 1 if v > (1 << (C - 1)) else 0
        out.append(v - (carry << C))
    assert carry == 0 and sum(d << (C * w) for w, d in enumerate(out)) == s
    return out


def buckets_of(scalars):
    return {abs(d) - 1 for s in scalars for d in digits(s) if d}


def placed(t, negative):
    """the scalar whose twelve low digits are all +-(t + 1)"""
    d = t + 1
    if not negative:
        s = d * REP12
        assert digits(s) == [d] * 12 + [0] and buckets_of([s]) == {t}
        return s
    s = (1 << 240) - d * REP12
    assert digits(s) == [-d] * 12 + [1] and buckets_of([s]) == {t, 0}
    return s


def boundary_buckets():
    """t on each side of every chunk boundary of both levels, in both planes, plus the corners of the bucket range"""
    ts = {0, 1023, 1024, (1 << 19) - 1}
    a0, b0 = 5, 37                                            # some marginal of each plane
    for b in range(1 << RLOG, 1 << LO, 1 << RLOG):            # H_a0: multiples of 16 (level one) -- every fourth of them a multiple of 64 (level two)
        ts |= {(a0 << LO) + b - 1, (a0 << LO) + b}
    for a in range(1 << RLOG, 1 << HI, 1 << RLOG):            # L_b0: the same in the hi digit
        ts |= {((a - 1) << LO) + b0, (a << LO) + b0}
    run = 1 << (RLOG + FLOG)
    assert all(((a0 << LO) + run * j in ts and (a0 << LO) + run * j - 1 in ts) for j in range(1, (1 << LO) // run))
    assert all((((run * j) << LO) + b0 in ts and ((run * j - 1) << LO) + b0 in ts) for j in range(1, (1 << HI) // run))
    return sorted(ts)


class Box:
    """one basis per curve on the device, the sum of its points, one scalar buffer"""

    def __init__(self, khip, cid):
        self.khip, self.cid, self.q = khip, cid, _order(cid)
        self.g = cref.srs_generate(cid, 0, N, threads=8)
        self.srs = khip.Srs(cid, self.g)
        one = cref.ints_to_limbs([1] * N)
        self.total, inf = cref.msm(cid, self.g, one, scalars_mont=False, threads=8)
        assert not inf
        self.rep = khip.Srs(cid, np.tile(self.g[0], (N, 1)))          # one point, N times
        self.buf = khip.DevBuf(2 * N * 32)

    def run(self, srs, rows):
        """rows: k arrays of N scalars (limbs) -> k results through the wide path"""
        k = len(rows)
        self.buf.upload(np.concatenate(rows))
        got, ginf = srs.msm_batch_dev(self.buf.ptr, N, k, mont=False)
        assert any(name == "reduce_a1" for name, _ in self.khip.last_timings()), "the wide path did not serve this MSM"
        return got, ginf

    def close(self):
        self.buf.free(); self.srs.close(); self.rep.close()


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    k.set_wide_min_n(N)
    yield k
    k.set_wide_min_n(1 << 19)


@pytest.fixture(scope="module", params=[0, 1], ids=["vesta", "pallas"])
def box(khip, request):
    b = Box(khip, request.param)
    yield b
    b.close()


def _same(got, ginf, want, winf):
    return bool(ginf) == bool(winf) and (bool(winf) or np.array_equal(got, want))


@pytest.mark.parametrize("k", [1, 2])
def test_uniform_scalars(box, k):
    """254-bit uniform scalars: 13 x 2^12 entries in 2^19 buckets, so most chunk and run records are the identity record"""
    rng = np.random.default_rng(11 + box.cid)
    rows = []
    for _ in range(k):
        sc = rng.integers(0, 1 << 64, size=(N, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)
        rows.append(sc)
    got, ginf = box.run(box.srs, rows)
    for j in range(k):
        want, winf = cref.msm(box.cid, box.g, rows[j], scalars_mont=False, threads=8)
        assert _same(got[j], ginf[j], want, winf), j


@pytest.mark.parametrize("k", [1, 2])
def test_placed_buckets(box, k):
    """All N scalars equal to the scalar of one bucket t: bucket t (a hot bucket: k_bucket_sum_wide) holds the only record of the tail that is not the
    identity -- t at the corners of the range and on each side of every chunk boundary of both levels in both planes, both signs.  The reference is
    s (P_0 + ... + P_(N-1)), a one-point cref.msm."""
    cases = [(t, neg) for t in boundary_buckets() for neg in (False, True) if not (neg and t == (1 << 19) - 1)]
    scal = [placed(t, neg) for t, neg in cases]
    wants = [cref.msm(box.cid, box.total.reshape(1, 8), cref.ints_to_limbs([s]), scalars_mont=False) for s in scal]
    # the construction once in full: the N-point reference is that multiple of the sum
    full = np.tile(cref.ints_to_limbs([scal[1]]), (N, 1))
    w, winf = cref.msm(box.cid, box.g, full, scalars_mont=False, threads=8)
    assert _same(w, winf, *wants[1])
    if len(cases) % 2:
        cases.append(cases[0]); scal.append(scal[0]); wants.append(wants[0])
    for i in range(0, len(cases), k):
        rows = [np.tile(cref.ints_to_limbs([scal[i + j]]), (N, 1)) for j in range(k)]
        got, ginf = box.run(box.srs, rows)
        for j in range(k):
            assert _same(got[j], ginf[j], *wants[i + j]), cases[i + j]


def _single(t, negative):
    """one digit +-(t + 1) in window 0 (a negative one with its carry: +1 in window 1, i.e. the point 2^20 P in bucket 0)"""
    s = (t + 1) if not negative else (1 << C) - (t + 1)
    assert digits(s)[:2] == ([t + 1, 0] if not negative else [-(t + 1), 1]) and not any(digits(s)[2:])
    return s


# (first bucket, distance to the second): the pair lies in ONE marginal -- H_a for a distance in the lo digit, L_b for one in the hi digit --
# in neighbouring chunks of one run (distance 2^rlog: level two meets two equal chunk sums) or inside one chunk (distance 1: level one refuses and
# its marker is an input of level two)
PAIRS = [("H, two chunks", (7 << LO) + 200, 1 << RLOG), ("L, two chunks", (64 << LO) + 300, (1 << RLOG) << LO),
         ("H, one chunk", (7 << LO) + 200, 1), ("L, one chunk", (64 << LO) + 300, 1 << LO)]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("opposite", [False, True], ids=["equal", "opposite"])
def test_forced_exact_path(box, k, opposite):
    """A basis of one point P repeated.  Two scalars put P (window 0) into buckets t and t + dist of one marginal and into nothing else of it; a third puts
    P into another chunk of the same run, so the exact redo of the run has a lazy record to add as well.  Equal chunk sums cannot be added by add29: the
    run comes out as a marker and k_wide_a2 redoes it (a doubling); with opposite signs the pair sums to the identity, which must arrive as the identity."""
    q = box.q
    rows_all, wants = [], []
    for name, t, dist in PAIRS:
        chunk = (lambda x: (x & ((1 << LO) - 1)) >> RLOG) if name[0] == "H" else (lambda x: (x >> LO) >> RLOG)
        run = lambda x: chunk(x) >> FLOG
        marg = (lambda x: x >> LO) if name[0] == "H" else (lambda x: x & ((1 << LO) - 1))
        t2 = t + dist
        t3 = t + 2 * (1 << RLOG) * (1 if name[0] == "H" else 1 << LO)
        assert marg(t) == marg(t2) == marg(t3) and run(t) == run(t2) == run(t3)
        assert (chunk(t2) - chunk(t) == (0 if "one chunk" in name else 1)) and chunk(t3) == chunk(t) + 2
        vals = [_single(t, False), _single(t2, opposite), _single(t3, False)]
        assert buckets_of(vals) == {t, t2, t3} | ({0} if opposite else set())
        sc = cref.ints_to_limbs(vals + [0] * (N - 3))
        g = np.tile(box.g[0], (N, 1))
        want = cref.msm(box.cid, g, sc, scalars_mont=False, threads=8)
        assert _same(*want, *cref.msm(box.cid, box.g[:1], cref.ints_to_limbs([sum(vals) % q]), scalars_mont=False)), name
        rows_all.append(sc); wants.append(want)
    for i in range(0, len(rows_all), k):
        got, ginf = box.run(box.rep, rows_all[i:i + k])
        for j in range(k):
            assert _same(got[j], ginf[j], *wants[i + j]), PAIRS[i + j][0]


@pytest.mark.parametrize("k", [1, 2])
def test_cancelling_pair_alone(box, k):
    """P and -P in neighbouring chunks of one run and nothing else in it: the run's exact sum is the identity, and so is the whole MSM apart from the
    carry's entry in bucket 0."""
    rows, wants = [], []
    for name, t, dist in PAIRS[:2]:
        vals = [_single(t, False), _single(t + dist, True)]
        sc = cref.ints_to_limbs(vals + [0] * (N - 2))
        want = cref.msm(box.cid, np.tile(box.g[0], (N, 1)), sc, scalars_mont=False, threads=8)
        assert _same(*want, *cref.msm(box.cid, box.g[:1], cref.ints_to_limbs([sum(vals) % box.q]), scalars_mont=False))
        rows.append(sc); wants.append(want)
    for i in range(0, 2, k):
        got, ginf = box.run(box.rep, rows[i:i + k])
        for j in range(k):
            assert _same(got[j], ginf[j], *wants[i + j]), PAIRS[i + j][0]


@pytest.mark.parametrize("k", [1, 2])
def test_single_hot_bucket(box, k):
    """All scalars equal to one random 20-bit value: one bucket with N entries, summed by k_bucket_sum_wide, is the only input of the tail."""
    rng = np.random.default_rng(5 + box.cid)
    rows, wants = [], []
    for _ in range(k):
        d = int(rng.integers(1, 1 << 19))
        assert buckets_of([d]) == {d - 1}
        rows.append(np.tile(cref.ints_to_limbs([d]), (N, 1)))
        wants.append(cref.msm(box.cid, box.total.reshape(1, 8), cref.ints_to_limbs([d]), scalars_mont=False))
        assert _same(*wants[-1], *cref.msm(box.cid, box.g, rows[-1], scalars_mont=False, threads=8))
    got, ginf = box.run(box.srs, rows)
    for j in range(k):
        assert _same(got[j], ginf[j], *wants[j]), j
