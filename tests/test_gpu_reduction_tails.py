"""The MSM's bucket-sum stage and its reduction tails over narrow windows, each kernel on buckets the test builds (kh_debug_bucket_sums,
kh_debug_bucket_tail: csrc/msm.hip launch_bucket_sums / launch_narrow_tail, the functions msm_launch itself calls), exact against a reference that has no
tail in it.

In a whole MSM the plan picks the kernel and the scalars decide where the boundaries fall; here the test names both.  And in a tree over random bucket
sums no two operands are ever equal, opposite or the identity above the leaves, so the three mechanisms that make the folds of coop.cuh / block_sum.cuh
exact -- quad_add's identity selection, its wave-uniform early-out, its doubling fallback (and the dbl branch of add) -- never run there.  Every record
here is m G for a small known m (tests/reduction_inputs.py: a palette of -3 .. 3 in three XYZZ representations each), so collisions happen at every level,
and the expected value of any sum is (sum w m mod r) G, one cref.point_mul.  tests/test_reduction_reference.py pins that reference, the geometry restated in
Python and the `cancel` construction on the CPU.  All comparisons are exact: affine limbs and the infinity byte.

Contents, named for what they force:
  single     one occupied bucket per group: t = 0, nb - 1, each side of every digit (segment) boundary; plane j must be exactly (digit_j(t) + [j == 0]) P
  all_equal  every bucket the same group element in rotating representations: every level of every tree is a doubling
  palette    m_t uniform in -3 .. 3: equal, opposite and identity operands at every level
  cancel     the buckets a kernel sums first (reduction_inputs.first_summed) sum to zero, the marginal as a whole does not
  empty      all identity: every output is the point at infinity"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reduction_inputs as RI  # noqa: E402

pytestmark = pytest.mark.gpu

MARGINALS, MARGINALS_Q, MARGINALS_H, SEGMENTS = 0, 1, 2, 3
# (tail, c), the smallest that reach each boundary -- k_marginals (64 threads): c = 7, 64 buckets, 16 of 64 lanes load; c = 10, exactly one bucket per lane;
# c = 12, widths 4/4/3, 2 - 4 additions in sequence.  k_marginals_q (64 quads): c = 7, waves 1 - 3 hold identities only (the whole-wave early-out); c = 12 and
# c = 13, up to 4 per quad.  k_marginals_h (256 lanes): c = 14, the smallest the plan sends there, 256 / 512 / 512 buckets per marginal; c = 16, 4 per lane.
MARGINAL_SHAPES = [(MARGINALS, 7), (MARGINALS, 10), (MARGINALS, 12), (MARGINALS_Q, 7), (MARGINALS_Q, 12), (MARGINALS_Q, 13), (MARGINALS_H, 14), (MARGINALS_H, 16)]
# (nb, m): one block of k_reduce_seg with idle lanes; 16 segments; nseg = 512, one exactly full k_sum_level block; nblk1 = 2; the largest, 16 per segment.
# Three groups make ngroups * nseg ragged against k_reduce_seg's 128 threads in the small shapes.
SEGMENT_SHAPES = [(8, 4), (64, 4), (2048, 4), (1024, 1), (32768, 16)]
CONTENTS = ["single", "all_equal", "palette", "cancel", "empty"]


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


@pytest.fixture(scope="module", params=[0, 1], ids=["vesta", "pallas"])
def pal(request):
    return RI.Palette(request.param)


def triples(ts):
    """a list of buckets as one call of one group and calls of three"""
    ts = list(ts)
    while len(ts) % 3:
        ts.append(ts[0])
    return [ts[:1]] + [ts[i:i + 3] for i in range(0, len(ts), 3)]


def marginal_cases(content, tail, c):
    """[(groups, palette values (groups * nb,))]: every content with 1 and with 3 groups"""
    nb, sh, wd = RI.geometry(c)
    if content == "single":
        ts = [0, nb - 1, (1 << sh[1]) - 1, 1 << sh[1], (1 << sh[2]) - 1, 1 << sh[2]]
        return [(len(t), RI.single(nb, t)) for t in triples(ts)]
    if content == "cancel":
        first = RI.first_summed(tail, nb >> wd[0])
        cases =[(g, RI.cancel(c, g, first, seed=100 * c + g)) for g in (1, 3)]
        assert all(RI.cancel_holds(c, ms, g, first) for g, ms in cases)
        return cases
    make = {"all_equal": lambda g: RI.all_equal(nb, g), "palette": lambda g: RI.palette(nb, g, seed=10 * c + g), "empty": lambda g: np.zeros(g * nb, np.int64)}[content]
    return [(g, make(g)) for g in (1, 3)]


# every shape with every content, but for `cancel` in k_marginals_q at c = 7: there the first wave holds the WHOLE marginal (16 buckets for 16 quads), so no
# part of it can cancel while the whole does not -- that shape is there for the identities of the three other waves
MARGINAL_CASES = [(t, c, content) for t, c in MARGINAL_SHAPES for content in CONTENTS if (t, c, content) != (MARGINALS_Q, 7, "cancel")]


@pytest.mark.parametrize("fin", [0, 1], ids=["fin", "fin_q"])
@pytest.mark.parametrize("tail,c,content", MARGINAL_CASES, ids=["%s-c%d-%s" % (("marginals", "marginals_q", "marginals_h")[t], c, n) for t, c, n in MARGINAL_CASES])
def test_marginal_tail(khip, pal, tail, c, fin, content):
    """the three plane sums of every group, unfolded: plane j = sum_t (digit_j(t) + [j == 0]) B_t"""
    for groups, ms in marginal_cases(content, tail, c):
        if content == "single":
            assert all(np.count_nonzero(row) == 1 for row in ms.reshape(groups, -1))
        got, ginf = khip.debug_bucket_tail(pal.cid, tail, fin, c, 0, groups, pal.records(ms))
        totals = RI.plane_totals(c, ms, groups)
        for q in range(groups):
            for j in range(3):
                assert pal.same(got[q, j], ginf[q, j], totals[q, j]), (groups, q, j, int(totals[q, j]))
        if content == "empty":
            assert ginf.all()


def segment_cases(content, nb, m):
    if content == "single":
        ts = sorted({0, nb - 1, m - 1, m % nb, nb - m, max(nb - m - 1, 0), nb // 2 - 1, nb // 2})
        return [(len(t), RI.single(nb, t)) for t in triples(ts)]
    if content == "cancel":                    # the buckets of segment 1 are occupied and sum to zero: its running sum ends at the identity, which the
        cases = []                             # double-and-add then multiplies (m = 1: segments 1 and 2 hold opposite points, which meet in k_sum_level)
        for g in (1, 3):
            rng = np.random.default_rng(nb + g)
            ms = rng.integers(-3, 4, size=(g, nb)).astype(np.int64)
            n = max(m, 2)
            for q in range(g):
                ms[q, m:m + n] = RI.zero_sum(n, rng)
                assert (ms[q, m:m + n] != 0).all() and ms[q, m:m + n].sum() == 0
            cases.append((g, ms.reshape(-1)))
        return cases
    make = {"all_equal": lambda g: RI.all_equal(nb, g), "palette": lambda g: RI.palette(nb, g, seed=nb + m + g), "empty": lambda g: np.zeros(g * nb, np.int64)}[content]
    return [(g, make(g)) for g in (1, 3)]


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("nb,m", SEGMENT_SHAPES)
def test_segment_tail(khip, pal, nb, m, content):
    """k_reduce_seg -> k_sum_level -> k_sum_final: sum_t (t + 1) B_t, one record per group"""
    for groups, ms in segment_cases(content, nb, m):
        got, ginf = khip.debug_bucket_tail(pal.cid, SEGMENTS, 0, nb, m, groups, pal.records(ms))
        totals = RI.segment_totals(nb, ms, groups)
        for q in range(groups):
            assert pal.same(got[q], ginf[q], totals[q]), (groups, q, int(totals[q]))
        if content == "empty":
            assert ginf.all()


# 17 lists, so that k_bucket_sum_q's last quads are clamped to the last key: lengths on either side of both SMALL_NT values (4, 16), of CHUNK (128: one chunk
# item against two), of two items against three, and of 64 chunk sums against 65 in k_bucket_big (64 quads); empty lists at both ends
NT = [0, 1, 3, 4, 5, 16, 17, 127, 128, 129, 255, 256, 257, 8191, 8192, 8193, 0]


@pytest.mark.parametrize("hot_equal", [False, True], ids=["palette", "hot_all_equal"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["sum_nt4", "sum_nt16", "sum_q"])
def test_bucket_sums(khip, pal, kind, hot_equal):
    """bucket i = the sum of its list, through k_bucket_sum (SMALL_NT 4 and 16) or k_bucket_sum_q and the two hot-bucket kernels"""
    toff = np.concatenate([[0], np.cumsum(NT)]).astype(np.uint32)
    ms = RI.palette(int(toff[-1]), 1, seed=7 + kind)
    if hot_equal:                              # the three largest lists: one group element each, every level of both hot kernels' trees a doubling
        for i, v in zip((13, 14, 15), (2, -3, 1)):
            ms[toff[i]:toff[i + 1]] = v
    reps = np.random.default_rng(9).integers(0, RI.REPS, size=ms.size)
    got, ginf = khip.debug_bucket_sums(pal.cid, kind, toff, pal.records(ms, reps))
    for i in range(len(NT)):
        total = int(ms[toff[i]:toff[i + 1]].sum())
        assert pal.same(got[i], ginf[i], total), (i, NT[i], total)
    assert ginf[0] and ginf[16]


def test_shapes_no_plan_produces_are_refused(khip, pal):
    rec = lambda n: np.zeros((n, 16), np.uint64)
    for args, n in [((MARGINALS, 0, 6, 0, 1), 32), ((MARGINALS_Q, 1, 17, 0, 1), 1 << 16),       # c outside 7 .. 16
                    ((MARGINALS_H, 0, 12, 0, 1), 1 << 11),                                       # k_marginals_h below 256 buckets per marginal
                    ((SEGMENTS, 0, 64, 3, 1), 64), ((SEGMENTS, 0, 64, 32, 1), 64),               # m does not divide nb; m beyond a plan's 16
                    ((SEGMENTS, 0, 1 << 16, 16, 1), 1 << 16), ((4, 0, 7, 0, 1), 64), ((MARGINALS, 2, 7, 0, 1), 64)]:
        with pytest.raises(khip.KhError):
            khip.debug_bucket_tail(pal.cid, *args, rec(n))
    with pytest.raises(khip.KhError):
        khip.debug_bucket_sums(pal.cid, 3, [0, 1], rec(1))
    with pytest.raises(khip.KhError):
        khip.debug_bucket_sums(pal.cid, 0, [0, 2, 1, 2], rec(2))
