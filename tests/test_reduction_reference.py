"""The reference of tests/test_gpu_reduction_tails.py, pinned without the device (tests/reduction_inputs.py).

1. The scalar-domain reference -- the expected value of a weighted sum of palette records is (sum w m mod r) G, one cref.point_mul -- equals the literal
   accumulation by cref.point_add: all three planes of a marginal tail at c = 7, a segment tail, one bucket-sum list.
2. The three XYZZ representations of a palette entry are the same group element: x / zz and y / zzz are the affine coordinates.
3. The Python restatement of the marginal geometry is the header's: tests/cpp/print_marginal_map.cpp prints marginal_geometry and marginal_bucket of
   csrc/msm_plan.hpp (g++, AddressSanitizer and UBSan, host code only) for every window width the GPU tests use.
4. The `cancel` contents have the property they are named for, in every shape the GPU tests build them for."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reduction_inputs as RI  # noqa: E402
from oracle import cref  # noqa: E402

WIDTHS = (7, 10, 12, 13, 14, 16)


@pytest.fixture(scope="module", params=[0, 1], ids=["vesta", "pallas"])
def pal(request):
    return RI.Palette(request.param)


def literal(pal, ms, weights):
    """sum_i weights[i] (ms[i] G) by repeated cref.point_add of the affine palette points"""
    acc, inf = np.zeros(8, np.uint64), True
    for m, w in zip(ms, weights):
        for _ in range(int(w) if m else 0):
            acc, inf = cref.point_add(pal.cid, acc, pal.affine[int(m)], p_inf=inf)
    return acc, inf


def test_scalar_reference_is_the_literal_accumulation(pal):
    c = 7
    nb, _sh, _wd = RI.geometry(c)
    ms = RI.palette(nb, 1, seed=3)
    assert set(ms.tolist()) == set(range(-3, 4))
    totals = RI.plane_totals(c, ms, 1)[0]
    for j in range(3):
        got, ginf = literal(pal, ms, RI.plane_weights(c)[j])
        assert pal.same(got, ginf, totals[j]), j
    got, ginf = literal(pal, ms, np.arange(nb) + 1)
    assert pal.same(got, ginf, RI.segment_totals(nb, ms, 1)[0])
    # one bucket-sum list (weight 1), a zero total (the identity) and a single entry
    lst = RI.palette(129, 1, seed=4)
    assert pal.same(*literal(pal, lst, np.ones(129)), lst.sum())
    zs = RI.zero_sum(16, np.random.default_rng(5))
    acc, inf = literal(pal, zs, np.ones(16))
    assert inf and pal.same(acc, inf, 0) and pal.expect(0)[1]
    assert pal.same(pal.affine[-2], False, -2) and not pal.same(pal.affine[-2], False, 2)


def test_representations_are_one_group_element(pal):
    for m in (-3, -2, -1, 1, 2, 3):
        recs = pal.records([m] * RI.REPS, reps=range(RI.REPS))
        assert len({r.tobytes() for r in recs}) == RI.REPS                         # different bytes ...
        for r in recs:                                                             # ... one point
            x = cref.field_op(pal.fid, "mul", r[0:4], cref.field_op(pal.fid, "inv", r[8:12]))[0]
            y = cref.field_op(pal.fid, "mul", r[4:8], cref.field_op(pal.fid, "inv", r[12:16]))[0]
            assert np.array_equal(np.concatenate([x, y]), pal.affine[m]), m
            zz3 = cref.field_op(pal.fid, "mul", cref.field_op(pal.fid, "sqr", r[8:12]), r[8:12])
            assert np.array_equal(zz3, cref.field_op(pal.fid, "sqr", r[12:16]))      # zz^3 = zzz^2
    assert not pal.records([0, 0, 0]).any()
    assert np.array_equal(pal.records([1, 1, 1, 1])[0], pal.records([1, 1, 1, 1])[3])   # rotating: index 3 is representation 0 again


def test_geometry_is_the_headers(tmp_path):
    exe = str(tmp_path / "print_marginal_map")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "print_marginal_map.cpp"), "-o", exe])
    run = subprocess.run([exe] + [str(c) for c in WIDTHS], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 2 * len(WIDTHS)
    for c, head, body in zip(WIDTHS, lines[0::2], lines[1::2]):
        nb, sh, wd = RI.geometry(c)
        assert [int(x) for x in head.split()] == [c, nb, *sh, *wd]
        want = [RI.marginal_bucket(c, j, v, e) for j in range(3) for v in range(1 << wd[j]) for e in range(nb >> wd[j])]
        assert [int(x) for x in body.split()] == want, c
        # and the weights are the digits of that map: bucket marginal_bucket(c, j, v, e) has weight v + [j == 0] in plane j
        w = RI.plane_weights(c)
        k = 0
        for j in range(3):
            for v in range(1 << wd[j]):
                n = nb >> wd[j]
                assert (w[j, want[k:k + n]] == v + (j == 0)).all()
                k += n


@pytest.mark.parametrize("tail,c", [(0, 7), (0, 10), (0, 12), (1, 12), (1, 13), (2, 14), (2, 16)])
def test_cancel_contents_cancel(tail, c):
    nb, _sh, wd = RI.geometry(c)
    first = RI.first_summed(tail, nb >> wd[0])
    ms = RI.cancel(c, 3, first, seed=c)
    assert RI.cancel_holds(c, ms, 3, first)
    assert not RI.cancel_holds(c, RI.all_equal(nb, 3), 3, first) and not RI.cancel_holds(c, np.zeros(3 * nb, np.int64), 3, first)
