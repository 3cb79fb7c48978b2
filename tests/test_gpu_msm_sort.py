"""The MSM's front half stage by stage (csrc/msm.hip: k_digits*, the four sorts, the task plan), from scalars, through kh_debug_msm_sort -- the launches an
MSM makes (msm_launch_sort), the plan's geometry, the reservation's buffers, and nothing behind them -- exact against tests/sort_reference.py (pinned on the
CPU by tests/test_sort_reference.py).  A whole MSM returns the right point with toff, the length ranking, the split and hot lists or pick_K's three
restatements wrong; here they are outputs.  Every workspace the sort hands on is poisoned with 0xff bytes before the launch.

Checks on every case (check_case): (a) digits, (b) off = the scan of the per-key counts and off[nkeys] = the number of non-zero digits, (c) per key the same
set of entries, (d) toff and the task total, (e) empty hand-over list and hot / split counters, (f) no poison left, (g) the sort path the case was written
for.  Where the keys are ranked: a permutation, task length non-increasing, rnt, roff.  On the wide path: the interleaved per-partition order, ptot, the split
pairs and keys, the hot list with its arrival counters, the identity records of empty buckets at their true bucket number.

There are no tolerances.  The one number the device computes in floating point is pick_K's table slot; sort_reference.pick_K asserts that the input keeps it
away from every boundary that matters."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu
PLAIN, FUSED, PART = SR.SORT_PLAIN, SR.SORT_FUSED, SR.SORT_PARTITIONED
POISON = 0xffffffff


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def contents(name, curve, n, k, c, W, seed=0):
    """-> (words (k * n Python integers), mont, inf or None): the scalar contents of the issue, by name"""
    r = SR.modulus(curve)
    rng = np.random.default_rng(1000 * seed + n + 7 * k + c)
    mont, inf = 0, None
    if name == "uniform":
        s = SR.uniform(rng, n * k, r)
    elif name == "uniform_mont":
        s, mont = SR.to_mont(SR.uniform(rng, n * k, r), r), 1
    elif name == "all_equal":
        s = [SR.uniform(rng, 1, r)[0]] * (n * k)
    elif name == "alternating":
        a, b = SR.uniform(rng, 2, r)
        s = SR.alternating(n * k, a, b)
    elif name == "witness":
        s = [v for _ in range(k) for v in SR.witness(rng, n, r)]
    elif name == "zeros":
        s = [0] * (n * k)
    elif name == "one_nonzero":
        s = SR.one_nonzero(n * k, (n * k) // 2, SR.uniform(rng, 1, r)[0])
    elif name == "inf_half":
        s, inf = SR.uniform(rng, n * k, r), rng.integers(0, 2, size=n * k).astype(np.uint8)
    elif name == "boundary":
        s = SR.boundary(rng, n * k, r, c)
    elif name == "boundary_mont":
        s, mont = SR.to_mont(SR.boundary(rng, n * k, r, c), r), 1
    elif name == "excess_p":
        s = ([r, r + 5, 5, r + r - 1] * (n * k))[:n * k]
    elif name == "carry_chain":
        s = ([SR.carry_chain(c, W), 1, SR.carry_chain(c, W) - 1] * (n * k))[:n * k]
    elif name == "glv_boundary":
        built = [b[0] for b in SR.glv_boundary(curve, c, 40, seed=c + curve)]
        s = (built * (n * k // len(built) + 1))[:n * k]
    else:
        raise KeyError(name)
    return s, mont, inf


def check_case(khip, curve, words, k, mont, path, inf=None, offset=0, stride=0, batch_stride=0, wide=False, ranked=None, **shape):
    n = len(words) // k
    mask = None
    if inf is not None:                                    # indexed as a basis' infinity bytes: inf[offset + j * batch_stride + i]
        mask = np.zeros(offset + (k - 1) * batch_stride + n, np.uint8)
        for j in range(k):
            mask[offset + j * batch_stride:offset + j * batch_stride + n] = inf[j * n:(j + 1) * n]
    g = khip.debug_msm_sort(curve, SR.limbs(words), k=k, mont=mont, inf=mask, offset=offset, stride=stride, batch_stride=batch_stride, wide=wide, **shape)
    c, W, nb, nkeys, precomp = g["c"], g["W"], g["nb"], g["nkeys"], g["precomp"]
    # (g) the path this case was written for
    assert (g["sort"], bool(g["wide"])) == (path, wide), (g["sort"], g["wide"])
    if ranked is not None:
        assert g["ranked"] == ranked
    assert nkeys == g["ngroups"] * nb and g["glv"] == int(bool(shape.get("glv")))
    # (a) digits
    D = np.stack([SR.digits(curve, words[j * n:(j + 1) * n], mont, c, W, glv=bool(g["glv"]), skip=None if inf is None else inf[j * n:(j + 1) * n]) for j in range(k)])
    assert np.array_equal(g["digits"], D), "digits"
    # (b) offsets, (f) none of them poison
    key, ent = SR.keys_entries(D, nb, precomp, offset, stride or offset + n, batch_stride, wide_low=g["part_low"] if wide else None)
    cnt = SR.counts_of(key, nkeys)
    off = g["off"].astype(np.int64)
    assert int(off[nkeys]) == np.count_nonzero(D) == int(g["counts"][5]), ("off[nkeys]", int(off[nkeys]), np.count_nonzero(D))
    assert np.array_equal(off, SR.exclusive(cnt)), "off"
    # (c) per key the same entries
    assert g["entries"].shape[0] == ent.shape[0] and not (g["entries"] == POISON).any()
    dkey, dent = SR.device_sorted(off, g["entries"], nkeys)
    assert np.array_equal(dkey, key) and np.array_equal(dent, ent), "entries"
    # (d) the task plan
    total = int(cnt.sum())
    K = SR.pick_K(total, g["room"], g["kmin"], g["ktab"], nkeys)
    nt, ln, toff = SR.tasks(cnt, K)
    assert int(g["toff"][nkeys]) == int(toff[-1]) == int(g["counts"][6]), ("tasks", int(g["toff"][nkeys]), int(toff[-1]), K)
    assert np.array_equal(g["toff"].astype(np.int64), toff), ("toff", K)
    # (e) the lists the accumulation and the bucket sums start from
    assert g["counts"][0] == 0, "handed[0]"
    if not wide:
        assert g["counts"][1] == 0 and g["counts"][2] == 0, "hot-bucket counters"
    if g["ranked"] == 1:
        order = g["order"].astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(nkeys)), "order is no permutation of the keys"
        assert (np.diff(ln[order]) <= 0).all(), "task length along the order"
        assert g["rnt"][nkeys] == 0 and np.array_equal(g["rnt"][:nkeys].astype(np.int64), nt[order]), "rnt"
        assert np.array_equal(g["roff"].astype(np.int64), SR.exclusive(nt[order])), "roff"
    if wide:
        check_wide(g, k, cnt, nt, ln)
    g.update(K=K, cnt=cnt, ref_key=key, ref_ent=ent)
    return g


def check_wide(g, k, cnt, nt, ln):
    nb, nkeys, low, og, hot_nt = g["nb"], g["nkeys"], g["part_low"], g["wide_og"], g["hot_nt"]
    nbl, nparts = 1 << low, 256 * k
    assert g["ranked"] == 2 and nbl * 256 == nb
    order = g["order"].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(nkeys)), "order is no permutation of the keys"
    r = np.arange(nbl)
    for q in range(nparts):                                # partition q = (MSM j, low bucket byte): permuted keys q * nbl ..
        keys = order[(r // og) * nparts * og + q * og + r % og]
        assert np.array_equal(np.sort(keys), q * nbl + r), ("partition", q)
        assert (np.diff(ln[keys]) <= 0).all(), ("task length along the order of partition", q)
    assert np.array_equal(g["ptot"].astype(np.int64), nt.reshape(nparts, nbl).sum(axis=1)), "ptot"
    split = np.nonzero(nt > 1)[0]
    assert g["counts"][3] == int((nt[split] - 1).sum()) and g["counts"][4] == split.size, "split counters"
    pairs = sorted(map(tuple, g["xpairs"].tolist()))
    assert pairs == [(int(key), j) for key in split for j in range(1, int(nt[key]))], "the extra chunks' (key, chunk) pairs"
    assert sorted(g["slist"].tolist()) == split.tolist(), "slist"
    hot = np.nonzero(nt > hot_nt)[0]
    assert g["counts"][1] == hot.size and sorted(g["big_keys"].tolist()) == hot.tolist(), "hot list"
    assert not g["big_arrivals"].any(), "arrival counters"
    # identity records: exactly the empty buckets, at group * nb + (local index << 8 | partition)
    key = np.arange(nkeys)
    grp, kk = key // nb, key % nb
    true = grp * nb + (((kk & (nbl - 1)) << 8) | (kk >> low))
    want = np.zeros(nkeys, np.uint8)
    want[true] = cnt == 0
    assert np.array_equal(g["b29_zero"], want), "identity records of the empty buckets"


# ---------------------------------------------------------------------------------- plain sort, no tables: c from the size
SMALL = ["uniform", "uniform_mont", "all_equal", "alternating", "witness", "zeros", "one_nonzero", "inf_half", "boundary", "boundary_mont", "excess_p", "carry_chain"]


@pytest.mark.parametrize("curve", [0, 1], ids=["vesta", "pallas"])
@pytest.mark.parametrize("content", SMALL)
def test_plain_c4_every_content(khip, curve, content):
    """n = 200: c = 4, 8 buckets, 64 windows"""
    s, mont, inf = contents(content, curve, 200, 1, 4, 64)
    g = check_case(khip, curve, s, 1, mont, PLAIN, inf=inf, ranked=0)
    assert (g["c"], g["nb"], g["W"]) == (4, 8, 64)


@pytest.mark.parametrize("curve", [0, 1], ids=["vesta", "pallas"])
@pytest.mark.parametrize("content", ["uniform", "boundary", "witness", "inf_half", "carry_chain"])
def test_plain_c7_batch_with_offset_and_batch_stride(khip, curve, content):
    s, mont, inf = contents(content, curve, 1061, 3, 7, 37)
    g = check_case(khip, curve, s, 3, mont, PLAIN, inf=inf, offset=7, batch_stride=2000, ranked=0)
    assert (g["c"], g["W"]) == (7, 37)


@pytest.mark.parametrize("content", ["uniform", "all_equal", "boundary"])
def test_plain_c13_two_uneven_slices(khip, content):
    s, mont, inf = contents(content, 0, 70001, 1, 13, 20)
    g = check_case(khip, 0, s, 1, mont, PLAIN, ranked=0)
    assert (g["c"], g["S"]) == (13, 2)


@pytest.mark.parametrize("content", ["uniform", "witness"])
def test_plain_ranked(khip, content):
    """n = 2^16, k = 4: M >= 2^22, k_len_starts / k_len_rank run"""
    s, mont, inf = contents(content, 1, 1 << 16, 4, 13, 20)
    check_case(khip, 1, s, 4, mont, PLAIN, ranked=1)


# ---------------------------------------------------------------------------------- over the tables
@pytest.mark.parametrize("content", ["uniform", "all_equal", "witness", "boundary", "zeros"])
def test_plain_over_tables_c16(khip, content):
    s, mont, inf = contents(content, 0, 4096, 1, 16, 16)
    check_case(khip, 0, s, 1, mont, PLAIN, precomp_c=16, fused_off=True, ranked=0)


@pytest.mark.parametrize("curve", [0, 1], ids=["vesta", "pallas"])
@pytest.mark.parametrize("c,n", [(13, 1000), (16, 1000)])
@pytest.mark.parametrize("fused_off", [True, False], ids=["plain", "fused"])
@pytest.mark.parametrize("content", ["glv_boundary", "uniform", "boundary"])
def test_glv_digits_and_sort(khip, curve, c, n, fused_off, content):
    """the split's rows, with magnitudes that are negated and hold a window of exactly 2^(c-1)"""
    s, mont, inf = contents(content, curve, n, 1, c, 2 * ((128 + c - 1) // c))
    g = check_case(khip, curve, s, 1, mont, PLAIN if fused_off else FUSED, precomp_c=c, glv=True, fused_off=fused_off, stride=n + 24)
    assert g["W"] == 2 * ((128 + c - 1) // c)


FUSED_LAST = max(n for n in range(69000, 70000) if SR.fused_fits(n, 1, 16, 1 << 15))


@pytest.mark.parametrize("n,k,content", [(5, 1, "uniform"), (5, 1, "zeros"), (4096, 1, "uniform"), (4096, 1, "boundary"), (4096, 1, "all_equal"), (4096, 1, "witness"),
                                         (4096, 1, "zeros"), (4096, 1, "one_nonzero"), (4096, 1, "inf_half"), (4096, 3, "uniform"), (4096, 3, "alternating"),
                                         (1 << 16, 1, "uniform"), (1 << 16, 1, "witness"), (FUSED_LAST, 1, "boundary")])
def test_fused_c16(khip, n, k, content):
    """32 blocks (k = 1), 60 blocks (k = 3); the digit +2^15 packs to 0x7fff beside the 0xffff of "no entry" (boundary)"""
    s, mont, inf = contents(content, 0, n, k, 16, 16)
    check_case(khip, 0, s, k, mont, FUSED, inf=inf, precomp_c=16, ranked=0)


@pytest.mark.parametrize("content", ["uniform", "alternating"])
def test_four_msms_64_blocks(khip, content):
    """k = 4 makes 64 blocks, but at c = 16 the plan does not fuse it: 4 * 2^15 + 1 keys over 2^16 threads are three keys per thread, one more than FUSED_KPT, so
    n = 4096, k = 4 takes the multi-launch sort (sort_reference.fused_fits restates the condition).  The 64-block launch is reached at c = 13."""
    s, mont, inf = contents(content, 0, 4096, 4, 16, 16)
    assert not SR.fused_fits(4096, 4, 16, 1 << 15)
    check_case(khip, 0, s, 4, mont, PLAIN, precomp_c=16, ranked=0)
    s, mont, inf = contents(content, 0, 4096, 4, 13, 20)
    assert SR.fused_fits(4096, 4, 20, 1 << 12)
    check_case(khip, 0, s, 4, mont, FUSED, precomp_c=13, ranked=0)


def test_fused_limit(khip):
    """the last n whose chunk fits FUSED_V int4's per thread takes the fused sort, the next one does not"""
    assert SR.fused_fits(FUSED_LAST, 1, 16, 1 << 15) and not SR.fused_fits(FUSED_LAST + 1, 1, 16, 1 << 15) and FUSED_LAST == 69628
    s, mont, inf = contents("uniform", 0, FUSED_LAST + 1, 1, 16, 16)
    assert khip.debug_msm_sort(0, SR.limbs(s[:FUSED_LAST]), precomp_c=16, echo_only=True)["sort"] == FUSED
    check_case(khip, 0, s, 1, mont, PLAIN, precomp_c=16, ranked=0)


@pytest.mark.parametrize("content", ["uniform", "boundary", "witness"])
def test_fused_c13(khip, content):
    s, mont, inf = contents(content, 1, 1000, 1, 13, 20)
    check_case(khip, 1, s, 1, mont, FUSED, precomp_c=13, ranked=0)


# ---------------------------------------------------------------------------------- partitioned, narrow
@pytest.mark.parametrize("content", ["uniform", "all_equal", "alternating", "witness", "zeros"])
def test_partitioned_64_blocks(khip, content):
    """precomp_c 16, n = 2^14, k = 8: 64 pass-A blocks; the uniform, mixed and idle branches of lds_inc_agg; off[nkeys] from the designated block"""
    s, mont, inf = contents(content, 0, 1 << 14, 8, 16, 16)
    g = check_case(khip, 0, s, 8, mont, PART, precomp_c=16, ranked=0)
    assert g["part_nblk"] == 64


@pytest.mark.parametrize("content", ["uniform", "one_nonzero"])
def test_partitioned_odd_size(khip, content):
    s, mont, inf = contents(content, 0, (1 << 17) + 3, 1, 16, 16)
    check_case(khip, 0, s, 1, mont, PART, precomp_c=16, ranked=0)


def test_partitioned_ranked(khip):
    s, mont, inf = contents("uniform", 0, 1 << 15, 8, 16, 16)
    check_case(khip, 0, s, 8, mont, PART, precomp_c=16, ranked=1)


@pytest.mark.parametrize("content", ["uniform", "all_equal"])
def test_partitioned_two_cus_clamps_the_task_length(khip, content):
    """room = 512: ceil(entries / room) is far above MAX_K and clamps to 256.  all_equal: buckets of 2^14 entries, 64 tasks each at K = 256 and 65 at 255, so
    the task counts give the clamp away (uniform buckets hold eight entries: one task at any K near it)"""
    s, mont, inf = contents(content, 0, 1 << 14, 8, 16, 16)
    g = check_case(khip, 0, s, 8, mont, PART, precomp_c=16, num_cus=2)
    assert g["room"] == 512 and g["K"] == SR.MAX_K and (int(g["counts"][5]) + 511) // 512 > SR.MAX_K
    if content == "all_equal":
        assert SR.infer_K(g["cnt"], g["toff"]) == [SR.MAX_K]


def test_wide_two_cus_clamps_the_task_length(khip):
    """pass B's own call of pick_K at the clamp: 13 buckets of 2^15 entries, 128 tasks each at K = 256"""
    s, mont, inf = contents("all_equal", 0, 1 << 15, 1, 20, 13)
    g = check_case(khip, 0, s, 1, mont, PART, precomp_c=16, wide=True, num_cus=2)
    assert g["K"] == SR.MAX_K and SR.infer_K(g["cnt"], g["toff"]) == [SR.MAX_K]


# ---------------------------------------------------------------------------------- wide
@pytest.mark.parametrize("n,k,content", [(4096, 1, "uniform"), (4096, 1, "all_equal"), (4096, 1, "zeros"), (4096, 1, "witness"), (5000, 2, "uniform"), (5000, 2, "boundary"),
                                         (5000, 2, "alternating")])
def test_wide(khip, n, k, content):
    s, mont, inf = contents(content, 0, n, k, 20, 13)
    g = check_case(khip, 0, s, k, mont, PART, precomp_c=16, wide=True)
    assert (g["c"], g["W"], g["part_low"]) == (20, 13, 11)
    if content == "all_equal":
        assert g["counts"][1] > 0 and g["counts"][4] > 0      # a hot and split bucket


@pytest.mark.parametrize("stage", [(0, 2), (2560, 8), (3000, 1), (28672, 2)], ids=lambda s: "stage%d_%d" % s)
@pytest.mark.parametrize("content", ["uniform", "all_equal", "witness"])
def test_wide_staged(khip, stage, content):
    """n = 2^15 under the staging settings of test_wide_sort_staging_settings: direct, staged in up to eight passes, staged where one pass is enough, the
    default; all_equal: one bucket holds a partition's every entry -- it straddles the staging area's end, and no bucket starts in the passes behind it"""
    s, mont, inf = contents(content, 0, 1 << 15, 1, 20, 13)
    g = check_case(khip, 0, s, 1, mont, PART, precomp_c=16, wide=True, stage_entries=stage[0], stage_maxpass=stage[1])
    assert g["stage_now"] == stage[0] and g["part2_maxpass"] == stage[1]


# ---------------------------------------------------------------------------------- the sorts against each other
def slot_is_clear(g):
    x = SR.k_slot(int(g["counts"][5]), g["nkeys"])
    return abs(x - round(x)) >= 0.05


@pytest.mark.parametrize("n,k,other", [(4096, 1, PLAIN), (1 << 16, 2, PART)], ids=["fused_plain", "fused_partitioned"])
def test_fused_sort_equals_the_multi_launch_sort(khip, n, k, other):
    """the same scalars through k_sort_fused and through the multi-launch path the shape takes without it: identical off and toff, per key the same entries,
    empty lists, and the same task length -- three restatements of pick_K"""
    s, mont, inf = contents("uniform", 0, n, k, 16, 16, seed=1)
    a = check_case(khip, 0, s, k, mont, FUSED, precomp_c=16)
    b = check_case(khip, 0, s, k, mont, other, precomp_c=16, fused_off=True)
    assert slot_is_clear(a) and slot_is_clear(b)
    assert np.array_equal(a["off"], b["off"]) and np.array_equal(a["toff"], b["toff"])
    for x, y in zip(SR.device_sorted(a["off"], a["entries"], a["nkeys"]), SR.device_sorted(b["off"], b["entries"], b["nkeys"])):
        assert np.array_equal(x, y)
    assert not a["counts"][:3].any() and not b["counts"][:3].any()
    Ka, Kb = (SR.infer_K(g["cnt"], g["toff"]) for g in (a, b))
    assert Ka == Kb and a["K"] in Ka and a["K"] == b["K"]


# ---------------------------------------------------------------------------------- refusals
def test_refusals(khip):
    one = SR.limbs([1] * 8)
    bad = [dict(k=0), dict(k=9), dict(precomp_c=6), dict(precomp_c=17), dict(glv=True), dict(precomp_c=16, glv=True, wide=True), dict(num_cus=1025),
           dict(offset=3, stride=5), dict(inf=np.zeros(3, np.uint8))]
    for kw in bad:
        with pytest.raises(khip.KhError) as e:
            khip.debug_msm_sort(0, np.zeros((0, 4), np.uint64) if kw.get("k") == 0 else (SR.limbs([1] * 9) if kw.get("k") == 9 else one), echo_only=True, **kw)
        assert e.value.code == khip.E_INVALID, kw
    with pytest.raises(khip.KhError) as e:                 # n W k above 2^26
        khip.debug_msm_sort(0, np.zeros(((1 << 22) + 4, 4), np.uint64), precomp_c=16, echo_only=True)
    assert e.value.code == khip.E_INVALID and "2^26" in str(e.value)
    with pytest.raises(khip.KhError):
        khip.debug_msm_sort(2, one, echo_only=True)
