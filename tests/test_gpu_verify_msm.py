"""kh_ipa_verify_msm (csrc/opening.cpp) -- the one device computation that decides kh_batch_verify's *ok -- alone against the oracle, on a 2^7 SRS of each
curve:   sum_i w_i <b_poly_coefficients(chals_i), G>  +  sum_j e_j X_j  == 0 ?

The reference scalar vector sum_i w_i s_i, s_i[j] = prod over the set bits b of j of chals_i[rounds - 1 - b], is computed here in Python integers and
multiplied into the SRS by the C oracle (cref.msm): S.  Then for k = 1, 3, 9 challenge sets: the extra (S, -1) gives zero and (S, -2) does not; a zero
weight (the reference recomputed) still gives zero; an infinity-flagged extra with a random scalar and garbage coordinates changes nothing; and k = 0
is the ad-hoc MSM alone."""
import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

ROUNDS = 7


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


@pytest.fixture(scope="module", params=["vesta", "pallas"])
def setup(khip, request):
    from proof_systems_amd import prover
    curve = khip.VESTA if request.param == "vesta" else khip.PALLAS
    F = prover.Fld(khip.FP if curve == khip.VESTA else khip.FQ)                 # the curve's scalar field
    srs = khip.Srs.create(curve, 1 << ROUNDS)
    g = srs.get_g(0, 1 << ROUNDS)
    assert g.shape == (1 << ROUNDS, 8) and np.array_equal(g, cref.srs_generate(curve, 0, 1 << ROUNDS, threads=8))
    yield khip, curve, F, srs, g
    srs.close()


def reference_point(curve, F, g, chals, weights):
    """S = <sum_i w_i b_poly_coefficients(chals_i), g> with the vector in Python integers: ((8,) limbs, inf)"""
    n = 1 << ROUNDS
    vec = [0] * n
    for ch, w in zip(chals, weights):
        assert len(ch) == ROUNDS
        for j in range(n):
            s = 1
            for b in range(ROUNDS):
                if j >> b & 1:
                    s = s * ch[ROUNDS - 1 - b] % F.p
            vec[j] = (vec[j] + w * s) % F.p
    return cref.msm(curve, g, F.limbs_many(vec), threads=8)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_the_batch_msm_equals_the_oracle(setup, k):
    khip, curve, F, srs, g = setup
    rng = np.random.default_rng(1000 + k)
    chals = [F.rand_many(rng, ROUNDS) for _ in range(k)]
    weights = F.rand_many(rng, k)
    assert all(weights) and all(all(c) for c in chals)
    ch_l = F.limbs_many([c for ch in chals for c in ch])

    def msm(ws, extras, scalars, inf=None):
        return khip.ipa_verify_msm(srs, ch_l, F.limbs_many(ws), np.stack(extras), F.limbs_many(scalars), inf)
    S, s_inf = reference_point(curve, F, g, chals, weights)
    assert not s_inf
    assert msm(weights, [S], [F.p - 1])
    assert not msm(weights, [S], [F.p - 2])
    # one weight zero: that challenge set drops out of the reference
    w0 = list(weights); w0[k // 2] = 0
    S0, s0_inf = reference_point(curve, F, g, chals, w0)
    if k == 1:
        assert s0_inf                                                           # nothing left: the sum over G is the point at infinity already
        garbage = rng.integers(0, 1 << 63, size=8, dtype=np.uint64)
        assert msm(w0, [garbage], [F.rand(rng)], np.array([1], np.uint8))
        assert not msm(w0, [S], [1])
    else:
        assert not s0_inf and not np.array_equal(S0, S)
        assert msm(w0, [S0], [F.p - 1])
        assert not msm(w0, [S], [F.p - 1])
    # an infinity-flagged extra with a random scalar and garbage coordinates changes nothing, before or after the real one
    garbage = rng.integers(0, 1 << 64, size=8, dtype=np.uint64, endpoint=False)
    r = F.rand(rng)
    assert r
    for extras, scalars, inf in (([S, garbage], [F.p - 1, r], [0, 1]), ([garbage, S], [r, F.p - 1], [1, 0])):
        assert msm(weights, extras, scalars, np.array(inf, np.uint8))
        assert not msm(weights, extras, [F.p - 2 if s == F.p - 1 else s for s in scalars], np.array(inf, np.uint8))


def test_without_challenge_sets_the_extras_alone_decide(setup):
    khip, curve, F, srs, g = setup
    none = np.zeros((0, 4), np.uint64)
    pt = g[5]
    assert khip.ipa_verify_msm(srs, none, none, np.stack([pt, pt]), F.limbs_many([1, F.p - 1]))
    assert not khip.ipa_verify_msm(srs, none, none, np.stack([pt]), F.limbs_many([1]))
