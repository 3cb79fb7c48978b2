"""kh_verify / kh_batch_verify -- kimchi::verifier::verify as one native call (csrc/verifier.cpp; the constant term on the device through
gates.hip's per-item-constants kernels) -- against the reference's OWN forty stored proofs (tests/golden/ref_fixtures/, read with
oracle/fixtures.py) and against the oracle verifier that is pinned on them (oracle/kimchi.py):

  1. every stored proof is accepted through kh_verifier_index_new + kh_proof_from_sections, and what the verifier derived on the way -- the
     challenges, the linearisation's constant term, the combined inner product -- and the index digest it computed equal the oracle's;
  2. the tampered copies tests/test_reference_fixtures.py rejects are rejected (ok = 0, return KH_OK);
  3. proofs of the native prover, smallest shapes that reach each branch, through kh_verifier_index_of: accepted, and rejected after one value of
     each proof section in turn is changed;
  4. a batch of eight over three indexes: accepted, rejected with one item tampered, and every item's trace is the one kh_verify gives alone
     (two items with different alpha share a launch of the per-item-constants kernels);
  5. everything malformed is KH_E_INVALID with a text that names the item, *ok untouched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import circuit as CC
from oracle import cref
from oracle import fixtures as FX
from oracle import kimchi as K
from oracle import pasta as P

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_proof_fixtures as M  # noqa: E402
from test_gpu_witness_lookups import Case, xor_case  # noqa: E402
from test_reference_fixtures import HERE as REF, PALLAS_FIXTURES, SRS_LEN, lagrange_commitments  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = sorted(f[:-4] for f in os.listdir(REF) if f.endswith(".bin"))
PATTERNS = ("Xor", "Lookup", "RangeCheck", "ForeignFieldMul")
POINT_SECTIONS = ("w_comm", "z_comm", "t_comm", "lr", "delta", "sg", "lookup_sorted_comm", "lookup_aggreg_comm", "lookup_runtime_comm")
ELEMENT_SECTIONS = ("evals", "public_evals", "ft_eval1", "z1_z2")


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


@pytest.fixture(scope="module")
def srs16(khip):
    """one 2^16 SRS per curve, made on first use: the size every stored proof was made over"""
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = khip.Srs.create(curve, SRS_LEN)
        return made[curve]
    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def g_vesta():
    return cref.srs_generate(0, 0, SRS_LEN, threads=8)


# ---------------------------------------------------------------------------------------------------- limbs
def elems(F, vals):
    return cref.ints_to_limbs([F.to_mont(v % F.p) for v in vals]).reshape(-1, 4) if len(vals) else np.zeros((0, 4), np.uint64)


def points(curve, pts):
    """[(x, y) | None] -> (xy (k, 8), inf (k,)) in the base field's Montgomery limbs"""
    B = curve.base
    xy = np.zeros((len(pts), 8), dtype=np.uint64)
    inf = np.zeros(len(pts), dtype=np.uint8)
    for i, p in enumerate(pts):
        if p is None:
            inf[i] = 1
        else:
            xy[i] = cref.ints_to_limbs([B.to_mont(p[0]), B.to_mont(p[1])]).reshape(8)
    return xy, inf


def ints(F, limbs):
    return [F.from_mont(v) for v in cref.limbs_to_ints(np.asarray(limbs).reshape(-1, 4))]


# ---------------------------------------------------------------------------------------------------- a stored proof as sections
def fixture_sections(khip, curve, fx):
    """(arguments of kh_verifier_index_new without the SRS, proof sections, public limbs, prev) of a loaded fixture"""
    F = curve.scalar
    v, pr = fx["vindex"], fx["proof"]
    flat = lambda comms: points(curve, [c for cm in comms for c in cm])
    gids = khip.gate_ids()
    opt = [(name, c) for name, c in zip(K.OPTIONAL_GATES, v["optional_comms"]) if c is not None]
    vs = {"sigma_comm": flat(v["sigma_comm"]), "coefficients_comm": flat(v["coefficients_comm"]), "generic_comm": flat([v["generic_comm"]]),
          "selector_comm": flat([v[k] for k in ("psm_comm", "complete_add_comm", "mul_comm", "emul_comm", "endomul_scalar_comm")]),
          "optional_comm": flat([c for _n, c in opt])}
    li = v["lookup_index"]
    if li:
        sel = [li["lookup_selectors"][q] for q in PATTERNS if li["lookup_selectors"].get(q) is not None]
        vs["lookup_table_comm"] = flat(li["lookup_table"])
        if li["table_ids"] is not None:
            vs["lookup_table_ids_comm"] = flat([li["table_ids"]])
        vs["lookup_selector_comm"] = flat(sel)
        if li["runtime_tables_selector"] is not None:
            vs["lookup_runtime_selector_comm"] = flat([li["runtime_tables_selector"]])
        mask = sum(1 << k for k, q in enumerate(PATTERNS) if li["lookup_selectors"].get(q) is not None)
        vs["lookup_info"] = [li["max_per_row"], li["max_joint_size"], int(li["joint_lookup_used"]), int(li["runtime_tables_selector"] is not None), mask,
                             len(li["lookup_table"]), 0, 0]
    index_args = (v["log2_n"], v["zk_rows"], v["public"], v["prev_challenges"], [gids[n] for n, _c in opt], vs)
    ev = pr["evals"]
    cols = [ev[k] for k in K.EVAL_ORDER] + list(ev["w"]) + list(ev["coefficients"]) + list(ev["s"]) + [e for e in ev["optional_gate_selectors"] if e is not None]
    if li:
        cols += [e for e in ev["lookup_sorted"] if e is not None] + [ev["lookup_aggregation"], ev["lookup_table"]]
        cols += [ev[k] for k in ("runtime_lookup_table", "runtime_lookup_table_selector") if ev[k] is not None]
        cols += [ev["lookup_selectors"][q] for q in PATTERNS if ev["lookup_selectors"].get(q) is not None]
    op = pr["opening"]
    ps = {"w_comm": flat(pr["w_comm"]), "z_comm": flat([pr["z_comm"]]), "t_comm": flat([pr["t_comm"]]),
          "evals": elems(F, [x for e in cols for part in e for x in part]), "ft_eval1": elems(F, [pr["ft_eval1"]]),
          "lr": points(curve, [p for lr in op["lr"] for p in lr]), "delta": points(curve, [op["delta"]]), "z1_z2": elems(F, [op["z1"], op["z2"]]),
          "sg": points(curve, [op["sg"]])}
    if ev["public"] is not None:
        ps["public_evals"] = elems(F, list(ev["public"][0]) + list(ev["public"][1]))
    if pr["lookup"]:
        ps["lookup_sorted_comm"] = flat(pr["lookup"]["sorted"]); ps["lookup_aggreg_comm"] = flat([pr["lookup"]["aggreg"]])
        if pr["lookup"]["runtime"] is not None:
            ps["lookup_runtime_comm"] = flat([pr["lookup"]["runtime"]])
    prev = [(elems(F, chals), points(curve, comm)) for chals, comm in pr["prev_challenges"]]
    return index_args, ps, elems(F, fx["public"]), prev


def fixture_item(khip, srs, curve, fx):
    """the live (vix, proof, public, prev) item of a loaded fixture: what kh_verify / kh_batch_verify take; the caller frees item[1] and item[0]"""
    index_args, ps, pub, prev = fixture_sections(khip, curve, fx)
    vix = khip.VerifierIndex(srs, *index_args)
    try:
        return (vix, khip.Proof(ps), pub, prev)
    except Exception:
        vix.free()
        raise


def native_verify(khip, srs, curve, fx):
    vix, proof, pub, prev = fixture_item(khip, srs, curve, fx)
    try:
        ok, trace = khip.verify(vix, proof, pub, prev)
        return ok, trace, vix.digest()
    finally:
        proof.free(); vix.free()


def curve_of(name):
    return P.PALLAS if name in PALLAS_FIXTURES else P.VESTA


# ---------------------------------------------------------------------------------------------------- 1. the reference's forty proofs
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_proof_is_accepted_and_the_trace_equals_the_oracle(khip, srs16, g_vesta, name, monkeypatch):
    assert len(FIXTURES) == 40
    C = curve_of(name); F = C.scalar
    cid = khip.VESTA if C is P.VESTA else khip.PALLAS
    fx = FX.load(os.path.join(REF, name + ".bin"), C)
    ok, trace, digest = native_verify(khip, srs16(cid), C, fx)
    assert ok
    # ---- the oracle on the same bytes
    h = C.srs_h()
    vix, proof = FX.oracle_views(fx, h)
    if fx["public"]:
        assert C is P.VESTA
        vix["public_comm"] = K.public_commitment(C, h, lagrange_commitments(g_vesta, vix["log2_n"], len(fx["public"])), fx["public"])
    want_digest = K.verifier_index_digest(C, vix)
    assert C.base.from_mont(P.from_limbs(digest)) == want_digest
    ch = K.fiat_shamir(C, vix, proof, want_digest)
    got = ints(F, trace["challenges"])
    assert got[:6] == [ch[k] for k in ("beta", "gamma", "alpha", "zeta", "v", "u")]
    assert got[6] == (ch["joint_combiner"] if vix["lookup_index"] else 0)
    ev = proof["evals"]
    ct = (K.generic_constant_term(F, ev, ch["alpha"]) + K.gate_library_constant_term(C, ev, ch["alpha"])) % F.p
    if vix["lookup_index"]:
        ct = (ct + K.lookup_constant_term(F, vix, ev, ch, ch["zeta"])) % F.p
    assert ints(F, trace["constant_term"]) == [ct]
    seen = {}

    def spy(curve, n, h_, batch, rng):                                      # the item K.verify hands to SRS::verify
        seen["cip"] = batch[0]["combined_inner_product"]
        return [], [], []
    monkeypatch.setattr(P, "ipa_verify_terms", spy)
    K.verify(C, vix, proof, None, h, None, final_msm=lambda *a: True)
    assert ints(F, trace["combined_inner_product"]) == [seen["cip"]]


# ---------------------------------------------------------------------------------------------------- 2. tampering
def bump(e, point):
    """an evaluation (chunks at zeta, chunks at zeta omega) with its first chunk at `point` (0 / 1) increased by one"""
    out = [list(e[0]), list(e[1])]
    out[point][0] += 1
    return (out[0], out[1])


def t_z_omega(fx): fx["proof"]["evals"]["z"] = bump(fx["proof"]["evals"]["z"], 1)
def t_ft_eval1(fx): fx["proof"]["ft_eval1"] += 1
def t_swap_sigma(fx): s = fx["vindex"]["sigma_comm"]; s[2], s[3] = s[3], s[2]
def t_w4(fx): fx["proof"]["evals"]["w"][4] = bump(fx["proof"]["evals"]["w"][4], 0)
def t_w1(fx): fx["proof"]["evals"]["w"][1] = bump(fx["proof"]["evals"]["w"][1], 0)
def t_sorted(fx): fx["proof"]["evals"]["lookup_sorted"][2] = bump(fx["proof"]["evals"]["lookup_sorted"][2], 0)
def t_aggreg(fx): fx["proof"]["evals"]["lookup_aggregation"] = bump(fx["proof"]["evals"]["lookup_aggregation"], 1)
def t_drop_table_ids(fx): fx["vindex"]["lookup_index"]["table_ids"] = None
def t_public(fx): fx["public"][2] = 4
def t_l_point(fx): lr = fx["proof"]["opening"]["lr"]; lr[0] = (lr[1][1], lr[0][1])          # L of round 0 replaced by another point of the curve
def t_z1(fx): fx["proof"]["opening"]["z1"] += 1


TAMPERINGS = [("test_poseidon", t_z_omega), ("test_poseidon", t_ft_eval1), ("test_poseidon", t_swap_sigma), ("test_poseidon", t_w4),
              ("lookup_gate_proving_works_multiple_tables", t_sorted), ("lookup_gate_proving_works_multiple_tables", t_aggreg),
              ("lookup_gate_proving_works_multiple_tables", t_drop_table_ids), ("test_generic_gate_pub", t_public),
              ("verify_range_check_valid_proof1", t_w1), ("test_runtime_table", t_w1), ("test_recursion", t_w1), ("test_poseidon", t_l_point), ("test_poseidon", t_z1)]


@pytest.mark.parametrize("name,mutate", TAMPERINGS, ids=[f"{n}-{m.__name__}" for n, m in TAMPERINGS])
def test_tampered_reference_proof_is_rejected(khip, srs16, name, mutate):
    C = P.VESTA
    fx = FX.load(os.path.join(REF, name + ".bin"), C)
    mutate(fx)
    ok, _trace, _digest = native_verify(khip, srs16(khip.VESTA), C, fx)          # KH_OK: no exception
    assert not ok


# ---------------------------------------------------------------------------------------------------- 3. round trips with the native prover
class Made:
    """an index from a gate list, one proof of it (sections) and what kh_verify takes besides"""

    def __init__(self, khip, srs, types, wires, co, wit, public=0, tables=None, runtime_cfg=None, runtime=None, prev=(), seed=1):
        from proof_systems_amd import prover
        self.khip, self.srs = khip, srs
        self.ix = prover.CreatedIndex(srs, types, wires, co, public=public, tables=tables, runtime_tables=runtime_cfg)
        F = self.F = self.ix.F
        self.wit, self.prev, self.runtime = wit, list(prev), runtime
        self.public = wit[0, :public] if public else None
        self.vix = khip.VerifierIndex.of(self.ix.native)
        self.sections = self.prove(seed)

    def prove(self, seed):
        F, nx = self.F, self.ix.native
        rnd = F.limbs_many(F.rand_many(np.random.default_rng(seed), nx.randomness_count(True)))
        return nx.prove(witness=self.wit, randomness=rnd, prev=self.prev, runtime=self.runtime)[0]

    def verify(self, sections=None, **kw):
        proof = self.khip.Proof(self.sections if sections is None else sections)
        try:
            return self.khip.verify(self.vix, proof, kw.get("public", self.public), kw.get("prev", self.prev))
        finally:
            proof.free()

    def item(self, sections=None):
        proof = self.khip.Proof(self.sections if sections is None else sections)
        return (self.vix, proof, self.public, self.prev)

    def free(self):
        self.vix.free(); self.ix.free()


def tampered(khip, curve_id, sections, name):
    """the sections with one value of section `name` changed to another canonical one: an element's lowest limb bit flipped; a point negated (on the
    curve, every limb of y another value)"""
    out = dict(sections)
    if name in ELEMENT_SECTIONS:
        e = sections[name].copy(); e[0, 0] ^= np.uint64(1)
        out[name] = e
    else:
        xy, inf = sections[name][0].copy(), sections[name][1].copy()
        base = khip.FQ if curve_id == khip.VESTA else khip.FP
        xy[0, 4:] = khip.debug_field_op(base, "neg", xy[0:1, 4:])[0]
        out[name] = (xy, inf)
    return out


def bench_records(khip, F, rows):
    wires = np.array([[[r, c] for c in range(7)] for r in range(rows)], dtype=np.uint32)
    co = np.zeros((rows, 15, 4), dtype=np.uint64)
    co[:, 0, :] = F.limbs(1); co[:, 4, :] = F.limbs(F.p - 1)               # 1 * w0 - 1 = 0
    return ["Generic"] * rows, wires, co, np.tile(F.limbs(1), (15, rows, 1))


def circuit_records(khip, F, Fo, cs, wit):
    rows = len(wit[0])
    types = [g["typ"] for g in cs["gates"][:rows]]
    wires = np.array([g["wires"] for g in cs["gates"][:rows]], dtype=np.uint32).reshape(rows, 7, 2)
    co = np.stack([F.limbs_many([cs["coefficients"][c][r] for c in range(15)]) for r in range(rows)])
    return types, wires, co, np.stack([F.limbs_many([v % Fo.p for v in col]) for col in wit])


def lookup_case(Fo=P.Fp):
    """30 Lookup rows into a caller's table with id 5 (even rows) and a runtime table with id 7 (odd rows): table ids, a synthesised dummy table, runtime rows"""
    ent = 12
    c0 = [7 * j + 1 for j in range(ent)]; c1 = [j * j + 3 for j in range(ent)]
    first, data = [8, 9, 8, 7, 1], [0, 2, 3, 4, 5]
    rows = 30
    wit = [[0] * rows for _ in range(15)]
    for r in range(rows):
        wit[0][r] = 5 if r % 2 == 0 else 7
        for k in range(3):
            j = (5 * r + 7 * k) % (ent if r % 2 == 0 else 5)
            wit[1 + 2 * k][r], wit[2 + 2 * k][r] = (c0[j], c1[j]) if r % 2 == 0 else (first[j], data[j])
    return Case([CC.gate("Lookup", r) for r in range(rows)], wit, [{"id": 5, "data": [c0, c1]}], runtime_cfg=[{"id": 7, "first_column": first}], runtime=data, Fo=Fo)


def xor_case_2_13():
    """test_gpu_witness_lookups.xor_case (a 64-bit xor: four Xor16 rows, their zero row, a wired cell) followed by Zero rows up to 5000: a 2^13 domain"""
    base = xor_case()
    rows = 5000
    gates = list(base.gates) + [CC.gate("Zero", r) for r in range(base.rows, rows)]
    case = Case(gates, [list(col) + [0] * (rows - base.rows) for col in base.wit])
    assert case.n == 1 << 13 and case.L.info.patterns == ["Xor"]
    return case


@pytest.fixture(scope="module")
def made(khip):
    """the circuits of parts 3 to 5, built once; three of them share one 2^7 Vesta SRS (the batch)"""
    from proof_systems_amd import prover
    FV, FP_ = prover.Fld(khip.FP), prover.Fld(khip.FQ)
    srs7, srs7p, srs9 = khip.Srs.create(khip.VESTA, 1 << 7), khip.Srs.create(khip.PALLAS, 1 << 7), khip.Srs.create(khip.VESTA, 1 << 9)
    srs13 = khip.Srs.create(khip.VESTA, 1 << 13)
    out = {}
    out["bench_vesta"] = Made(khip, srs7, *bench_records(khip, FV, (1 << 7) - 10))
    out["bench_pallas"] = Made(khip, srs7p, *bench_records(khip, FP_, (1 << 7) - 10))
    out["two_chunks"] = Made(khip, srs7, *bench_records(khip, FV, 200))
    assert out["two_chunks"].ix.num_chunks == 2 and out["two_chunks"].ix.log2_n == 8
    # create_recursive: one previous challenge of log2(SRS) rounds, one of log2(SRS) + 1 (a two-chunk commitment), comm = commit_non_hiding(b_poly_coefficients)
    std = P.StdRng(M.PREV_SEED)
    prev = []
    for rounds in (7, 8):
        chals = FV.limbs_many([P.field_rand(P.Fp, std) for _ in range(rounds)])
        prev.append((chals, srs7.commit_non_hiding(khip.b_poly_coefficients(khip.FP, chals, rounds)[0], 1 << (rounds - 7))))
    out["recursive"] = Made(khip, srs7, *bench_records(khip, FV, (1 << 7) - 10), prev=prev)
    cs, wit = M.library_circuit(P.Fp, 7)
    out["library"] = Made(khip, srs7, *circuit_records(khip, FV, P.Fp, cs, wit))
    case = lookup_case()
    types, wires, co = case.records(khip, FV)
    out["lookup"] = Made(khip, srs9, types, wires, co, case.limbs(FV), tables=case.tables, runtime_cfg=case.runtime_cfg,
                         runtime=FV.limbs_many(case.runtime))
    case = xor_case_2_13()
    types, wires, co = case.records(khip, FV)
    out["xor"] = Made(khip, srs13, types, wires, co, case.limbs(FV))
    # the Pallas twins (circuits over Fq: points on Vesta, Vesta's endo coefficient, the "fq" Poseidon parameters; the lookup side on the other field's
    # kernels); the xor twin is the 2^9 AND circuit (Xor16 rows with their XOR-table lookups, generic rows) over a 2^9 SRS
    srs9p = khip.Srs.create(khip.PALLAS, 1 << 9)
    cs, wit = M.library_circuit(P.Fq, 7)
    out["library_pallas"] = Made(khip, srs7p, *circuit_records(khip, FP_, P.Fq, cs, wit))
    case = lookup_case(P.Fq)
    types, wires, co = case.records(khip, FP_)
    out["lookup_pallas"] = Made(khip, srs9p, types, wires, co, case.limbs(FP_), tables=case.tables, runtime_cfg=case.runtime_cfg,
                                runtime=FP_.limbs_many(case.runtime))
    cs, wrows = M.and_circuit(P.Fq, 9)
    assert cs["lookup"] is not None and cs["log2_n"] == 9
    out["xor_pallas"] = Made(khip, srs9p, *circuit_records(khip, FP_, P.Fq, cs, [[r[c] for r in wrows] for c in range(15)]))
    for name in ("library_pallas", "lookup_pallas", "xor_pallas"):
        assert out[name].ix.curve == khip.PALLAS and out[name].F.p == P.Fq.p
    yield out
    for m in out.values():
        m.free()
    for s in (srs7, srs7p, srs9, srs13, srs9p):
        s.close()


ROUND_TRIPS = ["bench_vesta", "bench_pallas", "two_chunks", "recursive", "lookup", "xor", "library", "library_pallas", "lookup_pallas", "xor_pallas"]


@pytest.mark.parametrize("name", ROUND_TRIPS)
def test_native_proof_is_accepted_and_every_changed_section_is_rejected(khip, made, name):
    m = made[name]
    ok, _trace = m.verify()
    assert ok
    changed = [s for s in POINT_SECTIONS + ELEMENT_SECTIONS if s in m.sections and len(m.sections[s][0] if isinstance(m.sections[s], tuple) else m.sections[s])]
    assert {"w_comm", "z_comm", "t_comm", "evals", "public_evals", "ft_eval1", "lr", "delta", "z1_z2", "sg"} <= set(changed)
    kind = name[:-len("_pallas")] if name.endswith("_pallas") else name
    assert ("lookup_sorted_comm" in changed) == (kind in ("lookup", "xor")) and ("lookup_runtime_comm" in changed) == (kind == "lookup")
    for s in changed:
        ok, _trace = m.verify(tampered(khip, m.ix.curve, m.sections, s))
        assert not ok, s


# ---------------------------------------------------------------------------------------------------- 4. batch
def test_batch_of_eight_over_three_indexes(khip, made):
    batch_over_indexes(khip, made, ["bench_vesta", "library", "two_chunks", "bench_vesta", "library", "two_chunks", "library", "bench_vesta"], 5)


def test_pallas_batch_of_four_over_two_indexes(khip, made):
    """a batch takes one SRS, so one curve: the Pallas library proofs (live EndoMul / EndoMulScalar / Poseidon terms in the constant term, with Vesta's endo
    coefficient and the "fq" MDS in the per-item constants) in a batch of their own, between generic-only items"""
    batch_over_indexes(khip, made, ["bench_pallas", "library_pallas", "library_pallas", "bench_pallas"], 2)


def batch_over_indexes(khip, made, order, spoil):
    F = made[order[0]].F
    curve = made[order[0]].ix.curve
    secs = [made[n].prove(seed=40 + i) for i, n in enumerate(order)]            # different proofs: every item has its own alpha
    alone = [made[n].verify(s) for n, s in zip(order, secs)]
    assert all(ok for ok, _t in alone) and len({tuple(t["challenges"][2]) for _ok, t in alone}) == len(order)
    rand = F.limbs_many([0x1234567, 0x89abcdef01])
    items = [made[n].item(s) for n, s in zip(order, secs)]
    ok, traces = khip.batch_verify(items, rand)
    assert ok
    for i, ((_ok, want), got) in enumerate(zip(alone, traces)):
        for k in want:
            assert np.array_equal(want[k], got[k]), (i, k)
    ok, _t = khip.batch_verify(items, None)                                     # rand_base, sg_rand_base drawn by the library
    assert ok
    bad = list(items)
    bad[spoil] = made[order[spoil]].item(tampered(khip, curve, secs[spoil], "evals"))
    ok, traces = khip.batch_verify(bad, rand)
    assert not ok
    for it in items + [bad[spoil]]:
        it[1].free()


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_malformed_input_is_refused_before_any_device_work(khip, made):
    b, lk, xr, pal = made["bench_vesta"], made["lookup"], made["xor"], made["bench_pallas"]
    INVALID = khip.E_INVALID
    keep = []

    def proof(sections):
        keep.append(khip.Proof(sections))
        return keep[-1]

    def refused(items, rand=None, names=None, count=None):
        rc, ok, _tr = khip.batch_verify_raw(items, rand, ok_before=7, count=count)
        msg = khip.raw().kh_last_error().decode()
        assert rc == INVALID and ok == 7, (rc, ok, msg)
        for n in names or ():
            assert n in msg, (n, msg)
        return msg
    good = b.item(); keep.append(good[1])
    with_ = lambda sections, **kw: (b.vix, proof(dict(b.sections, **kw) if sections is None else sections), None, ())
    # null pointers, an empty batch
    refused([(None, good[1])], names=["item 0", "null"])
    refused([good, (b.vix, None)], names=["item 1", "null"])
    refused([good], count=0, names=["empty"])
    assert khip.raw().kh_verify(None, None, None) == INVALID
    # one batch, one SRS: a Vesta item and an index over another handle (a second 2^7 SRS of the same curve)
    other_srs = khip.Srs.create(khip.VESTA, 1 << 7)
    other = Made(khip, other_srs, *bench_records(khip, b.F, (1 << 7) - 10))
    it2 = other.item(); keep.append(it2[1])
    refused([good, it2], names=["item 1", "SRS"])
    # rand with a zero element / an element >= p
    one = b.F.limbs(1)
    refused([good], rand=np.stack([one, np.zeros(4, np.uint64)]), names=["rand[1]", "zero"])
    refused([good], rand=np.stack([np.full(4, 2**64 - 1, np.uint64), one]), names=["rand[0]", "canonical"])
    # a limb vector >= p, a point off the curve
    e = b.sections["evals"].copy(); e[3, 3] = np.uint64(2**64 - 1)
    refused([good, with_(None, evals=e)], names=["item 1", "evals", "element 3", "canonical"])
    z = b.sections["z1_z2"].copy(); z[1] = np.uint64(2**64 - 1)
    refused([with_(None, z1_z2=z)], names=["item 0", "z1_z2"])
    xy, inf = b.sections["w_comm"]; xy = xy.copy(); xy[2, 0] ^= np.uint64(1)
    refused([with_(None, w_comm=(xy, inf))], names=["item 0", "w_comm", "point 2", "not on the curve"])
    xy, inf = b.sections["sg"]; xy = xy.copy(); xy[0, 5] ^= np.uint64(4)
    refused([with_(None, sg=(xy, inf))], names=["item 0", "sg", "not on the curve"])
    # the reference's structural errors: chunk counts, public inputs, previous challenges, rounds, lookup sections, optional gates
    xy, inf = b.sections["t_comm"]
    refused([with_(None, t_comm=(xy[:-1], inf[:-1]))], names=["item 0", "t_comm", "6 points, 7 expected"])
    refused([with_(None, evals=b.sections["evals"][:-2])], names=["item 0", "evals"])
    xy, inf = b.sections["lr"]
    refused([with_(None, lr=(xy[:-2], inf[:-2]))], names=["item 0", "lr", "12 points, 14 expected"])
    refused([(b.vix, good[1], np.stack([one]), ())], names=["item 0", "1 public inputs, the index has 0"])
    vi = b.ix.native.verifier_index()
    vix1 = khip.VerifierIndex(b.srs, b.ix.log2_n, b.ix.zk_rows, 0, 1, [], vi)                    # an index that expects one previous challenge
    refused([(vix1, good[1], None, ())], names=["item 0", "0 previous challenges, the index has 1"])
    ok, _t = khip.verify(khip.VerifierIndex(b.srs, b.ix.log2_n, b.ix.zk_rows, 0, 0, [], vi), good[1])      # (the same sections with the right count: accepted)
    assert ok
    rec = made["recursive"]
    chals, comm = rec.prev[1]
    refused([(rec.vix, proof(rec.sections), None, [rec.prev[0], (chals, (comm[0][:1], comm[1][:1]))])], names=["item 0", "previous challenge 1"])
    refused([with_(None, lookup_sorted_comm=lk.sections["lookup_sorted_comm"])], names=["item 0", "no lookup index"])
    no_lookup = {k: v for k, v in lk.sections.items() if not k.startswith("lookup_")}
    refused([(lk.vix, proof(no_lookup), None, ())], names=["item 0", "no lookup commitments"])
    no_runtime = {k: v for k, v in lk.sections.items() if k != "lookup_runtime_comm"}
    refused([(lk.vix, proof(no_runtime), None, ())], names=["item 0", "lookup_runtime_comm"])
    # an optional-gate selector evaluation (Xor16's) without its commitment: the xor circuit's index without its optional gate
    vi = dict(xr.ix.native.verifier_index()); vi["optional_comm"] = None; vi["digest"] = None
    vix_no_opt = khip.VerifierIndex(xr.srs, xr.ix.log2_n, xr.ix.zk_rows, 0, 0, [], vi)
    refused([(vix_no_opt, proof(xr.sections), None, ())], names=["item 0", "optional-gate selector evaluations"])
    # kh_verifier_index_new itself: a section with the wrong number of points, a point off the curve, an optional gate that is none
    vi = b.ix.native.verifier_index()
    for change, word in (({"sigma_comm": (vi["sigma_comm"][0][:-1], vi["sigma_comm"][1][:-1])}, "sigma_comm"), ({"optional_comm": vi["generic_comm"]}, "optional_comm")):
        with pytest.raises(khip.KhError, match=word) as ei:
            khip.VerifierIndex(b.srs, b.ix.log2_n, b.ix.zk_rows, 0, 0, [], dict(vi, **change))
        assert ei.value.code == INVALID
    xy = vi["generic_comm"][0].copy(); xy[0, 1] ^= np.uint64(1)
    with pytest.raises(khip.KhError, match="not on the curve"):
        khip.VerifierIndex(b.srs, b.ix.log2_n, b.ix.zk_rows, 0, 0, [], dict(vi, generic_comm=(xy, vi["generic_comm"][1])))
    with pytest.raises(khip.KhError, match="optional gate"):
        khip.VerifierIndex(b.srs, b.ix.log2_n, b.ix.zk_rows, 0, 0, [khip.gate_ids()["Poseidon"]], dict(vi, optional_comm=vi["generic_comm"]))
    # a Pallas proof against a Vesta index: its points are not on that curve
    refused([(b.vix, proof(pal.sections), None, ())], names=["item 0"])
    for p_ in keep:
        p_.free()
    vix1.free(); vix_no_opt.free(); other.free(); other_srs.close()


def test_a_c_program_verifies_and_sees_the_rejection(khip):
    """tests/cpp/test_verify.cpp: index, proof, kh_verify, one flipped limb rejected, a non-canonical limb refused -- the C ABI without Python"""
    exe = os.path.join(HERE, "cpp", "test_verify")
    if not os.path.exists(exe):
        import __graft_entry__ as ge
        ge.build()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_verify OK" in r.stdout, r.stdout + r.stderr
