"""kh_verify / kh_batch_verify reject a proof after ANY one of its values is changed, not the first of each section (csrc/verifier.cpp): a verifier that
leaves one evaluation out of the sponge or the opening list, one chunk of t_comm or one round of lr out of the MSM, or honours an `inf` flag in the MSM
that it did not absorb, still accepts every honest proof.  On the smallest bench proof (2^7), the lookup proof (2^9: table ids, a runtime table) and
the recursive one (two previous challenges), every value in turn:

  * each element of evals, public_evals, ft_eval1, z1_z2 replaced by another canonical element;
  * each point of every point section negated, and again with its `inf` flag set (a point already at infinity is skipped and counted: under a tenth);
  * each point of every verifier-index section negated (one at infinity: replaced by a finite point), with the digest recomputed and with the prover's
    digest kept; the library-gates circuit as a fourth index here, the one whose coefficient and selector commitments are all finite;
  * each public input; each scalar and each commitment chunk of each previous challenge;
  * in a batch of five: the bad item first, in the middle and last, for z1, z2, sg, delta, an lr point and an evaluation, with the caller's `rand` and
    with the library's; and two items whose sg are off by +H and -H with z2 adjusted, which only the weights sg_rand_base^i tell from an honest batch.

Every mutation is asserted to differ and to be well formed before the call; every call returns KH_OK with ok = 0."""
import numpy as np
import pytest

from oracle import pasta as P

from test_gpu_verify import ELEMENT_SECTIONS, POINT_SECTIONS, Made, M, bench_records, circuit_records, khip, lookup_case  # noqa: F401

pytestmark = pytest.mark.gpu

VINDEX_POINT_SECTIONS = ("sigma_comm", "coefficients_comm", "generic_comm", "selector_comm", "optional_comm", "lookup_table_comm", "lookup_table_ids_comm",
                         "lookup_selector_comm", "lookup_runtime_selector_comm")
R256 = 1 << 256


# ---------------------------------------------------------------------------------------------------- mutations
def to_int(limbs):
    return int.from_bytes(np.ascontiguousarray(limbs, dtype=np.uint64).tobytes(), "little")


def to_limbs(v, words=4):
    return np.frombuffer(v.to_bytes(8 * words, "little"), dtype=np.uint64).copy()


def other_element(limbs, p, bit):
    """another canonical element: bit `bit` flipped; where that lands at or above the modulus, the element plus one"""
    v = to_int(limbs)
    assert v < p
    w = v ^ (1 << bit)
    if w >= p:
        w = (v + 1) % p
    assert w != v and 0 <= w < p
    return to_limbs(w)


def on_curve(xy, q):
    rinv = pow(R256, -1, q)
    xm, ym = to_int(xy[:4]), to_int(xy[4:])
    x, y = xm * rinv % q, ym * rinv % q
    return xm < q and ym < q and (y * y - x * x * x - 5) % q == 0


def negated(xy, q):
    """-P: on the curve, every limb of y another value (the Montgomery form of -y is q - y R)"""
    y = to_int(xy[4:])
    assert 0 < y < q
    out = np.array(xy, dtype=np.uint64)
    out[4:] = to_limbs(q - y)
    assert on_curve(xy, q) and on_curve(out, q) and not np.array_equal(out, xy)
    return out


def element_changes(sections, p):
    """(label, sections) for every element of every element section"""
    for name in ELEMENT_SECTIONS:
        arr = sections.get(name)
        for j in range(len(arr) if arr is not None else 0):
            e = arr.copy()
            e[j] = other_element(arr[j], p, (7 * j + 3) % 255)                 # a different bit from element to element, low and high limbs
            yield (name, j), dict(sections, **{name: e})


def point_changes(pts, q, skipped):
    """(label, (xy, inf)) for every point of a point section: negated, then flagged as infinity; points already flagged are counted in `skipped`"""
    xy, inf = pts
    for j in range(len(inf)):
        if inf[j]:
            skipped.append(j)
            continue
        x2 = xy.copy(); x2[j] = negated(xy[j], q)
        yield (j, "negated"), (x2, inf.copy())
        i2 = inf.copy(); i2[j] = 1
        assert i2[j] != inf[j]
        yield (j, "inf"), (xy.copy(), i2)


# ---------------------------------------------------------------------------------------------------- the proofs
@pytest.fixture(scope="module")
def small(khip):
    """the smallest bench proof, the recursive one and one with public inputs over a 2^7 Vesta SRS; the lookup proof over 2^9"""
    from proof_systems_amd import prover
    FV = prover.Fld(khip.FP)
    srs7, srs9 = khip.Srs.create(khip.VESTA, 1 << 7), khip.Srs.create(khip.VESTA, 1 << 9)
    out = {}
    out["bench"] = Made(khip, srs7, *bench_records(khip, FV, (1 << 7) - 10))
    std = P.StdRng(M.PREV_SEED)
    prev = []
    for rounds in (7, 8):
        chals = FV.limbs_many([P.field_rand(P.Fp, std) for _ in range(rounds)])
        prev.append((chals, srs7.commit_non_hiding(khip.b_poly_coefficients(khip.FP, chals, rounds)[0], 1 << (rounds - 7))))
    out["recursive"] = Made(khip, srs7, *bench_records(khip, FV, (1 << 7) - 10), prev=prev)
    case = lookup_case()
    types, wires, co = case.records(khip, FV)
    out["lookup"] = Made(khip, srs9, types, wires, co, case.limbs(FV), tables=case.tables, runtime_cfg=case.runtime_cfg, runtime=FV.limbs_many(case.runtime))
    cs, wit = M.library_circuit(P.Fp, 7)
    out["library"] = Made(khip, srs7, *circuit_records(khip, FV, P.Fp, cs, wit))
    cs, wit = M.generic_circuit(P.Fp, 7, 7, npub=3)
    out["public"] = Made(khip, srs7, *circuit_records(khip, FV, P.Fp, cs, wit), public=3)
    for m in out.values():
        m.p, m.q = prover.MOD[khip.FP], prover.MOD[khip.FQ]                     # Vesta: scalars in Fp, coordinates in Fq
        ok, _t = m.verify()
        assert ok
    yield out
    for m in out.values():
        m.free()
    srs7.close(); srs9.close()


SWEPT = ("bench", "lookup", "recursive")


def rejected(m, sections=None, **kw):
    ok, _trace = m.verify(sections, **kw)                                       # KH_OK: anything else raises
    return not ok


@pytest.mark.parametrize("name", SWEPT)
def test_every_changed_element_is_rejected(khip, small, name):
    m = small[name]
    count = 0
    for label, sections in element_changes(m.sections, m.p):
        assert rejected(m, sections), label
        count += 1
    assert count == sum(len(m.sections[s]) for s in ELEMENT_SECTIONS) and count >= 2 * 43 + 2 + 1 + 2


@pytest.mark.parametrize("name", SWEPT)
def test_every_negated_and_every_flagged_point_is_rejected(khip, small, name):
    m = small[name]
    present = [s for s in POINT_SECTIONS if isinstance(m.sections.get(s), tuple) and len(m.sections[s][1])]       # (an absent section is an empty array)
    assert {"w_comm", "z_comm", "t_comm", "lr", "delta", "sg"} <= set(present)
    assert ("lookup_sorted_comm" in present and "lookup_aggreg_comm" in present and "lookup_runtime_comm" in present) == (name == "lookup")
    for s in present:
        skipped, count = [], 0
        for label, pts in point_changes(m.sections[s], m.q, skipped):
            assert rejected(m, dict(m.sections, **{s: pts})), (s,) + label
            count += 1
        total = len(m.sections[s][1])
        assert 10 * len(skipped) < total and count == 2 * (total - len(skipped)), (s, skipped)


@pytest.mark.parametrize("digest", ["recomputed", "kept"])
@pytest.mark.parametrize("name", SWEPT + ("library",))
def test_every_changed_index_commitment_is_rejected(khip, small, name, digest):
    """Every commitment of the verifier index negated.  The bench and the lookup circuits use two coefficient columns and no library gate, so most of
    their coefficient and selector commitments are the point at infinity: there is nothing to negate, and instead of being skipped such a commitment is
    replaced by a finite point (its flag cleared) -- nothing is left out.  The library circuit, whose coefficient, selector and sigma commitments are
    all finite, is swept as well, so that every position of those sections is also negated once."""
    m = small[name]
    vi = m.ix.native.verifier_index()
    if digest == "recomputed":
        vi = dict(vi, digest=None)
    gids = khip.gate_ids()
    args = (m.srs, m.ix.log2_n, m.ix.zk_rows, 0, len(m.prev), [gids[g] for g in m.ix.optional])

    def verify_with(sections):
        vix = khip.VerifierIndex(*args, sections)
        proof = khip.Proof(m.sections)
        try:
            ok, _t = khip.verify(vix, proof, None, m.prev)
            return ok, vix.digest()
        finally:
            proof.free(); vix.free()
    ok, dg = verify_with(vi)
    assert ok and np.array_equal(dg, m.vix.digest())                            # the index rebuilt from its sections is the prover's
    present = [s for s in VINDEX_POINT_SECTIONS if len(vi[s][1])]
    assert {"sigma_comm", "coefficients_comm", "generic_comm", "selector_comm"} <= set(present)
    assert ({"lookup_table_comm", "lookup_table_ids_comm", "lookup_selector_comm", "lookup_runtime_selector_comm"} <= set(present)) == (name == "lookup")
    finite = vi["sigma_comm"][0][0]
    assert not vi["sigma_comm"][1][0] and on_curve(finite, m.q)
    for s in present:
        xy, inf = vi[s]
        raised = 0
        for j in range(len(inf)):
            x2, i2 = xy.copy(), inf.copy()
            if inf[j]:
                x2[j] = finite; i2[j] = 0                                       # infinity -> a finite point of the curve
                raised += 1
            else:
                x2[j] = negated(xy[j], m.q)
            assert i2[j] == 0 and (inf[j] or not np.array_equal(x2[j], xy[j]))
            ok, dg = verify_with(dict(vi, **{s: (x2, i2)}))
            assert not ok, (s, j)
            assert np.array_equal(dg, m.vix.digest()) == (digest == "kept"), (s, j)
        if name == "library" and s in ("sigma_comm", "coefficients_comm", "generic_comm", "selector_comm"):
            assert raised == 0, (s, raised)                                     # every position of these sections negated at least here
        if s.startswith("lookup_") or s in ("sigma_comm", "generic_comm"):
            assert raised == 0, (s, raised)


def test_every_changed_public_input_is_rejected(khip, small):
    m = small["public"]
    assert len(m.public) == 3
    for j in range(len(m.public)):
        pub = np.array(m.public, dtype=np.uint64)
        pub[j] = other_element(m.public[j], m.p, (11 * j + 1) % 255)
        assert rejected(m, public=pub), j
    for label, sections in element_changes({"public_evals": m.sections["public_evals"]}, m.p):
        assert rejected(m, dict(m.sections, **sections)), label


def test_every_changed_value_of_a_previous_challenge_is_rejected(khip, small):
    m = small["recursive"]
    assert [len(c) for c, _cm in m.prev] == [7, 8] and [len(cm[1]) for _c, cm in m.prev] == [1, 2]
    for k, (chals, comm) in enumerate(m.prev):
        def with_(c=chals, cm=comm):
            prev = list(m.prev); prev[k] = (c, cm)
            return prev
        for j in range(len(chals)):
            c2 = np.array(chals, dtype=np.uint64)
            c2[j] = other_element(chals[j], m.p, (13 * j + 5) % 255)
            assert rejected(m, prev=with_(c=c2)), (k, "scalar", j)
        skipped = []
        for label, cm2 in point_changes((np.asarray(comm[0]), np.asarray(comm[1])), m.q, skipped):
            assert rejected(m, prev=with_(cm=cm2)), (k, "chunk") + label
        assert not skipped


# ---------------------------------------------------------------------------------------------------- position in a batch
def batch_mutations(sections, p, q):
    """{label: sections} with one value of the opening (or one evaluation) changed"""
    def elem(name, j, bit):
        e = sections[name].copy(); e[j] = other_element(e[j], p, bit)
        return dict(sections, **{name: e})

    def neg(name, j):
        xy, inf = sections[name]
        assert not inf[j]
        x2 = xy.copy(); x2[j] = negated(xy[j], q)
        return dict(sections, **{name: (x2, inf)})
    return {"z1": elem("z1_z2", 0, 0), "z2": elem("z1_z2", 1, 200), "sg": neg("sg", 0), "delta": neg("delta", 0), "lr[9]": neg("lr", 9), "evals[57]": elem("evals", 57, 64)}


@pytest.fixture(scope="module")
def five(khip, small):
    m = small["bench"]
    secs = [m.prove(seed=90 + i) for i in range(5)]
    items = [m.item(s) for s in secs]
    ok, _t = khip.batch_verify(items, None)
    assert ok
    yield m, secs, items
    for it in items:
        it[1].free()


@pytest.mark.parametrize("at", [0, 2, 4])
def test_a_bad_item_is_found_at_every_position_of_a_batch(khip, small, five, at):
    m, secs, items = five
    rand = m.F.limbs_many([0x1234567, 0x89abcdef01])
    muts = batch_mutations(secs[at], m.p, m.q)
    assert len(muts) == 6
    for label, sections in muts.items():
        bad = list(items); bad[at] = m.item(sections)
        try:
            for r in (rand, None):
                ok, _t = khip.batch_verify(bad, r)
                assert not ok, (at, label, "rand given" if r is not None else "rand drawn")
        finally:
            bad[at][1].free()


def test_two_sg_errors_that_cancel_without_the_weights_are_rejected(khip, small, five):
    """Item 0 claims sg + H and z2 - z1, item 4 claims sg - H and z2 + z1.  Each still satisfies its opening equation c Q + delta = z1 (sg + b0 U) + z2 H;
    only sg = <s, G> fails, by +H and by -H.  The final MSM weighs these two checks with sg_rand_base^0 and sg_rand_base^4: equal weights would cancel
    the errors and accept."""
    m, secs, items = five
    h = khip.srs_h(khip.VESTA)
    assert on_curve(h, m.q)

    def shifted(sections, sign):
        xy, inf = sections["sg"]
        assert not inf[0]
        sg, sginf = khip.points_sum(khip.VESTA, np.stack([xy[0], h if sign > 0 else negated(h, m.q)]))
        assert not sginf and on_curve(sg, m.q) and not np.array_equal(sg, xy[0])
        z = sections["z1_z2"]
        z1, z2 = to_int(z[0]), to_int(z[1])
        z_new = np.stack([z[0], to_limbs((z2 - sign * z1) % m.p)])             # Montgomery limbs are linear: (z2 -+ z1) R
        assert not np.array_equal(z_new[1], z[1])
        return dict(sections, sg=(sg.reshape(1, 8), inf.copy()), z1_z2=z_new)
    plus, minus = m.item(shifted(secs[0], +1)), m.item(shifted(secs[4], -1))
    try:
        for it in (plus, minus):
            ok, _t = khip.verify(*it)
            assert not ok
        bad = [plus] + items[1:4] + [minus]
        for r in (m.F.limbs_many([0x1234567, 0x89abcdef01]), None):
            ok, _t = khip.batch_verify(bad, r)
            assert not ok
    finally:
        plus[1].free(); minus[1].free()


def test_two_z2_errors_that_cancel_without_the_weights_are_rejected(khip, small, five):
    """Item 0 claims z2 + 1, item 4 claims z2 - 1: the opening equations fail by -H and by +H.  The final MSM weighs the two equations with rand_base^0
    and rand_base^4: equal weights would cancel the errors and accept."""
    m, secs, items = five
    one = to_int(m.F.limbs(1))

    def shifted(sections, sign):
        z = sections["z1_z2"]
        z_new = np.stack([z[0], to_limbs((to_int(z[1]) + sign * one) % m.p)])
        assert not np.array_equal(z_new[1], z[1]) and to_int(z_new[1]) < m.p
        return dict(sections, z1_z2=z_new)
    plus, minus = m.item(shifted(secs[0], +1)), m.item(shifted(secs[4], -1))
    try:
        for it in (plus, minus):
            ok, _t = khip.verify(*it)
            assert not ok
        bad = [plus] + items[1:4] + [minus]
        for r in (m.F.limbs_many([0x1234567, 0x89abcdef01]), None):
            ok, _t = khip.batch_verify(bad, r)
            assert not ok
    finally:
        plus[1].free(); minus[1].free()
