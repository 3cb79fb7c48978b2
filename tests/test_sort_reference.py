"""tests/sort_reference.py against brute force, on the CPU: the digit recoding, the GLV rows, the keys and entries, the task plan, and the scalar
constructions tests/test_gpu_msm_sort.py feeds the device -- so that a disagreement there is the device's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_reference as SR  # noqa: E402

CURVES = [0, 1]


def value_of(col, c):
    return sum(int(d) << (c * w) for w, d in enumerate(col))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("c", [4, 7, 13, 16, 20])
def test_digits_sum_to_the_scalar_and_lie_in_the_half_open_range(curve, c):
    r = SR.modulus(curve)
    W = (256 + c - 1) // c
    rng = np.random.default_rng(c)
    s = SR.boundary(rng, 40, r, c) + SR.uniform(rng, 20, r) + [SR.carry_chain(c, W)]
    half = 1 << (c - 1)
    for mont, words in ((0, s), (1, SR.to_mont(s, r)), (0, [v + r for v in s if v + r < 1 << 256 and v < r])):
        D = SR.digits(curve, words, mont, c, W)
        want = s if len(words) == len(s) else [v for v in s if v + r < 1 << 256 and v < r]
        assert D.shape == (W, len(words)) and (D > -half).all() and (D <= half).all()
        assert [value_of(D[:, i], c) for i in range(len(words))] == want
    # the digit exactly at +2^(c-1) stays positive; one above it goes negative with a carry
    D = SR.digits(curve, [half, half + 1], 0, c, W)
    assert list(D[:2, 0]) == [half, 0] and list(D[:2, 1]) == [-(half - 1), 1]
    # the carry chain reaches the top window
    D = SR.digits(curve, [SR.carry_chain(c, W)], 0, c, W)
    assert D[0, 0] == -1 and not D[1:W - 1, 0].any() and D[W - 1, 0] == 1


@pytest.mark.parametrize("curve", CURVES)
def test_canonical_input_with_one_excess_modulus(curve):
    r = SR.modulus(curve)
    D = SR.digits(curve, [r, r + 5, 5, 0], 0, 16, 16)
    assert not D[:, 0].any() and np.array_equal(D[:, 1], D[:, 2]) and D[0, 2] == 5 and not D[:, 3].any()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("c", [13, 16])
def test_glv_rows_and_the_constructed_pairs(curve, c):
    p = SR.glv_params(curve)
    r, lam = p["r"], p["lam"]
    Wh = (128 + c - 1) // c
    half = 1 << (c - 1)
    built = SR.glv_boundary(curve, c, 36, seed=c + curve)
    assert len(built) >= 32
    rng = np.random.default_rng(5)
    s = [b[0] for b in built] + SR.uniform(rng, 30, r) + [0, 1, r - 1, lam, r - lam]
    D = SR.digits(curve, s, 0, c, 2 * Wh, glv=True)
    assert (D > -half).all() and (D <= half).all()
    for i, v in enumerate(s):
        k1, k2 = value_of(D[:Wh, i], c), value_of(D[Wh:, i], c)
        assert (k1 + k2 * lam - v) % r == 0 and (k1, k2) == SR.GLV.split(p, v)
    for i, (v, k1, k2) in enumerate(built):
        assert SR.GLV.split(p, v) == (k1, k2) and (k1 < 0 or k2 < 0)
        hit = False
        for h, kk in enumerate((k1, k2)):
            wins = [(abs(kk) >> (c * w)) & ((1 << c) - 1) for w in range(Wh)]
            if kk < 0 and half in wins:
                w = wins.index(half)
                hit = True
                assert D[h * Wh + w, i] == half                # -(2^(c-1) - 2^c) = +2^(c-1): never the negative digit that would pack to "no entry"
        assert hit
    assert np.array_equal(SR.digits(curve, SR.to_mont(s, r), 1, c, 2 * Wh, glv=True), D)
    Dz = SR.digits(curve, s, 0, c, 2 * Wh, glv=True, skip=[i % 2 for i in range(len(s))])
    assert not Dz[:, 1::2].any() and np.array_equal(Dz[:, 0::2], D[:, 0::2])


def test_keys_and_entries_against_a_loop():
    rng = np.random.default_rng(3)
    k, W, n, nb = 2, 3, 17, 8
    D = rng.integers(-nb + 1, nb + 1, size=(k, W, n))
    for precomp in (0, 1):
        key, ent = SR.keys_entries(D, nb, precomp, offset=5, stride=100, batch=1000)
        want = sorted(((j if precomp else j * W + w) * nb + abs(int(D[j, w, i])) - 1, (5 + (w * 100 if precomp else 0) + j * 1000 + i) | (int(D[j, w, i] < 0) << 31))
                      for j in range(k) for w in range(W) for i in range(n) if D[j, w, i])
        assert list(zip(key.tolist(), ent.tolist())) == want
        nkeys = (k if precomp else k * W) * nb
        cnt = SR.counts_of(key, nkeys)
        off = SR.exclusive(cnt)
        assert off[-1] == np.count_nonzero(D) and len(off) == nkeys + 1
        shuffled = np.concatenate([rng.permutation(ent[off[q]:off[q + 1]]) for q in range(nkeys)])
        k2, e2 = SR.device_sorted(off, shuffled, nkeys)
        assert np.array_equal(k2, key) and np.array_equal(e2, ent)
    # the wide permutation: (b & 255) << low | b >> 8 is a bijection of the bucket range
    nb, low = 1 << 19, 11
    D = np.array([[[1, -nb, 257, 256, 0]]])
    key, _ = SR.keys_entries(D, nb, 1, 0, 8, 0, wide_low=low)
    assert sorted(key.tolist()) == sorted([0, (255 << low) | (nb - 1 >> 8), 1, 255 << low])
    b = np.arange(nb)
    assert np.array_equal(np.sort(((b & 255) << low) | (b >> 8)), b)


def test_task_plan():
    ktab = np.zeros(48, np.uint8)
    assert SR.pick_K(0, 100, 8, ktab, 10) == 8                       # a job with no entry
    assert SR.pick_K(1000, 100, 8, ktab, 10) == 10 and SR.pick_K(1001, 100, 8, ktab, 10) == 11
    assert SR.pick_K(10 ** 6, 512, 8, ktab, 10) == SR.MAX_K           # the clamp
    ktab[:] = 4
    ktab[20:] = 12
    assert SR.pick_K(3 * 4096, 10 ** 6, 8, ktab, 4096) == 4          # 4 log2(3) + 8.5 = 14.84
    assert SR.pick_K(9 * 4096, 10 ** 6, 8, ktab, 4096) == 12         # 21.18
    with pytest.raises(AssertionError):
        SR.pick_K(int(4096 * 2 ** (11.5 / 4)) + 1, 10 ** 6, 8, ktab, 4096)      # slot value 20.0..: the neighbours disagree
    cnt = np.array([0, 1, 8, 9, 16, 17, 100])
    nt, ln, toff = SR.tasks(cnt, 8)
    assert nt.tolist() == [0, 1, 1, 2, 2, 3, 13] and ln.tolist() == [0, 1, 8, 5, 8, 6, 8] and toff.tolist() == [0, 0, 1, 2, 4, 6, 9, 22]
    assert SR.infer_K(cnt, toff) == [8]


def test_fused_limit_is_where_the_chunk_outgrows_the_registers():
    fits = [n for n in range(1, 1 << 17) if SR.fused_fits(n, 1, 16, 1 << 15)]
    assert fits == list(range(4, 69629))                   # ceil(n / 4) + 1 int4's per thread-chunk against FUSED_V * FUSED_T = 17408
    # four MSMs at c = 16 have 2^17 + 1 keys for 2^16 threads: three keys per thread, one more than FUSED_KPT -- three MSMs fit, and four at c = 13
    assert not SR.fused_fits(4096, 4, 16, 1 << 15) and SR.fused_fits(4096, 3, 16, 1 << 15) and SR.fused_fits(4096, 4, 20, 1 << 12)
    assert not SR.fused_fits(4096, 5, 20, 1 << 12) and not SR.fused_fits(1000, 1, 37, 1 << 10)


@pytest.mark.parametrize("curve", CURVES)
def test_scalar_constructions(curve):
    r = SR.modulus(curve)
    rng = np.random.default_rng(1)
    w = SR.witness(rng, 50, r)
    assert w[:40] == [1] * 40 and w[40:47] == [0] * 7 and all(0 < v < r for v in w[47:])
    assert all(v < r for v in SR.boundary(rng, 64, r, 16)) and SR.boundary(rng, 64, r, 16)[:4] == [0, 1, r - 1, r - 2]
    D = SR.digits(curve, SR.boundary(rng, 200, r, 16), 0, 16, 16)
    assert (D == 1 << 15).any() and (D == -(1 << 15) + 1).any()       # +2^(c-1), which packs to 0x7fff beside the fused sort's 0xffff, is reached
    assert SR.ints(SR.limbs([0, 1, r - 1, r + 5])) == [0, 1, r - 1, r + 5]
    assert SR.one_nonzero(5, 3, 9) == [0, 0, 0, 9, 0] and SR.alternating(4, 1, 2) == [1, 2, 1, 2]
