"""kh_batch_verify on the batches its phase 2 is written for (csrc/verifier.cpp; gates.hip: k_gate_batch_*): items with and without a lookup index,
optional gates, runtime tables, public inputs and previous challenges side by side in one two-row column table, and more than the 128 items of one block.

  A. the reference's own stored proofs (tests/golden/ref_fixtures/) as ONE batch per curve, lookup and plain items alternating: accepted, every item's
     trace is the one kh_verify gives that item alone, each of test_gpu_verify.TAMPERINGS applied to its one item rejects the batch (return KH_OK) and
     leaves the other items' traces alone; a batch of one and the full batch again in between (the gate_batch scratch shrinks in use and is reused);
  B. proofs of the native prover over ONE 2^9 SRS, one of every kind test_gpu_verify.made spreads over three: a batch of all kinds, and 130 items
     (two blocks of k_gate_batch_*; the clamped idle lanes) with items 127, 128 and 129 pairwise different and a lookup item on both sides of it.

Every comparison is exact: limbs equal, ok is 0 or 1."""
import os

import numpy as np
import pytest

from oracle import fixtures as FX
from oracle import pasta as P

from test_gpu_verify import (FIXTURES, REF, PALLAS_FIXTURES, TAMPERINGS, Made, M, bench_records, circuit_records, fixture_item, khip, lookup_case,  # noqa: F401
                             srs16, tampered, xor_case)

pytestmark = pytest.mark.gpu

TRACE_KEYS = ("challenges", "constant_term", "ft_eval0", "combined_inner_product")


def same_trace(want, got, where):
    assert set(want) == set(TRACE_KEYS)
    for k in TRACE_KEYS:
        assert np.array_equal(want[k], got[k]), (where, k)


def alternating(names, flag):
    """`names` reordered so that the ones with `flag` and the ones without alternate for as long as both last"""
    a, b = [n for n in names if flag[n]], [n for n in names if not flag[n]]
    out = [n for pair in zip(a, b) for n in pair]
    return out + a[len(b):] + b[len(a):], min(len(a), len(b))


# ---------------------------------------------------------------------------------------------------- A. the reference's proofs as one batch
class RefBatch:
    """the stored proofs of one curve as live items in mixed order, with the trace kh_verify gives each alone"""

    def __init__(self, khip, srs, curve, names):
        self.khip, self.srs, self.curve = khip, srs, curve
        fxs = {n: FX.load(os.path.join(REF, n + ".bin"), curve) for n in names}
        self.has_lookup = {n: bool(fxs[n]["vindex"]["lookup_index"]) for n in names}
        self.order, self.mixed = alternating(names, self.has_lookup)
        self.items = [fixture_item(khip, srs, curve, fxs[n]) for n in self.order]
        self.alone = []
        for it in self.items:
            ok, trace = khip.verify(*it)
            assert ok
            self.alone.append(trace)
        self.rand = prover_field(khip, curve).limbs_many([0x1234567, 0x89abcdef01])

    def accepted(self, rand):
        ok, traces = self.khip.batch_verify(self.items, rand)
        assert ok
        for i, (want, got) in enumerate(zip(self.alone, traces)):
            same_trace(want, got, (i, self.order[i]))

    def free(self):
        for it in self.items:
            it[1].free(); it[0].free()


def prover_field(khip, curve):
    from proof_systems_amd import prover
    return prover.Fld(khip.FP if curve is P.VESTA else khip.FQ)


@pytest.fixture(scope="module")
def vesta_batch(khip, srs16):
    b = RefBatch(khip, srs16(khip.VESTA), P.VESTA, [n for n in FIXTURES if n not in PALLAS_FIXTURES])
    yield b
    b.free()


def test_the_reference_vesta_proofs_as_one_mixed_batch(khip, vesta_batch):
    b = vesta_batch
    assert len(b.items) == 38 and b.mixed >= 8
    for i in range(2 * b.mixed - 1):
        assert b.has_lookup[b.order[i]] != b.has_lookup[b.order[i + 1]], i
    b.accepted(b.rand)
    b.accepted(None)                                                            # rand_base, sg_rand_base drawn by the library


def test_the_reference_pallas_proofs_as_one_batch(khip, srs16):
    b = RefBatch(khip, srs16(khip.PALLAS), P.PALLAS, sorted(PALLAS_FIXTURES))
    try:
        assert len(b.items) == 2
        b.accepted(b.rand)
        b.accepted(None)
    finally:
        b.free()


@pytest.mark.parametrize("name,mutate", TAMPERINGS, ids=[f"{n}-{m.__name__}" for n, m in TAMPERINGS])
def test_one_tampered_item_rejects_the_mixed_batch_and_moves_no_other_trace(khip, vesta_batch, name, mutate):
    b = vesta_batch
    at = b.order.index(name)
    fx = FX.load(os.path.join(REF, name + ".bin"), P.VESTA)
    mutate(fx)
    bad_item = fixture_item(khip, b.srs, P.VESTA, fx)
    try:
        # a batch of one between two full batches: the gate_batch scratch is used at 1/38 of its size, then in full again
        ok, traces = khip.batch_verify([b.items[at]], b.rand)
        assert ok
        same_trace(b.alone[at], traces[0], (at, name, "batch of one"))
        bad = list(b.items); bad[at] = bad_item
        ok, traces = khip.batch_verify(bad, b.rand)                             # KH_OK: no exception
        assert not ok
        for i, (want, got) in enumerate(zip(b.alone, traces)):
            if i != at:
                same_trace(want, got, (i, b.order[i], "beside the tampered item"))
        b.accepted(b.rand)
    finally:
        bad_item[1].free(); bad_item[0].free()


# ---------------------------------------------------------------------------------------------------- B. every kind over one SRS; two blocks
LOG_SRS = 9                                                                     # the smallest size all kinds build at: lookup_case and xor_case need 2^9
KINDS = ("lookup", "public", "xor", "library", "recursive", "two_lengths", "small_domain", "bench")


@pytest.fixture(scope="module")
def mixed(khip):
    """one Made of every kind over one 2^9 Vesta SRS"""
    from proof_systems_amd import prover
    FV = prover.Fld(khip.FP)
    n = 1 << LOG_SRS
    srs = khip.Srs.create(khip.VESTA, n)
    out = {}
    out["bench"] = Made(khip, srs, *bench_records(khip, FV, n - 10))
    out["two_lengths"] = Made(khip, srs, *bench_records(khip, FV, n + 90))
    assert out["two_lengths"].ix.num_chunks == 2 and out["two_lengths"].ix.log2_n == LOG_SRS + 1
    out["small_domain"] = Made(khip, srs, *bench_records(khip, FV, (1 << 7) - 10))
    assert out["small_domain"].ix.num_chunks == 1 and out["small_domain"].ix.log2_n == 7
    std = P.StdRng(M.PREV_SEED)
    prev = []
    for rounds in (LOG_SRS, LOG_SRS + 1):                                       # a one-chunk and a two-chunk commitment
        chals = FV.limbs_many([P.field_rand(P.Fp, std) for _ in range(rounds)])
        prev.append((chals, srs.commit_non_hiding(khip.b_poly_coefficients(khip.FP, chals, rounds)[0], 1 << (rounds - LOG_SRS))))
    out["recursive"] = Made(khip, srs, *bench_records(khip, FV, n - 10), prev=prev)
    cs, wit = M.library_circuit(P.Fp, 7)                                       # (a 2^7 domain: the circuit generator is slow in Python)
    out["library"] = Made(khip, srs, *circuit_records(khip, FV, P.Fp, cs, wit))
    case = lookup_case()
    types, wires, co = case.records(khip, FV)
    out["lookup"] = Made(khip, srs, types, wires, co, case.limbs(FV), tables=case.tables, runtime_cfg=case.runtime_cfg, runtime=FV.limbs_many(case.runtime))
    case = xor_case()
    assert case.n == n
    types, wires, co = case.records(khip, FV)
    out["xor"] = Made(khip, srs, types, wires, co, case.limbs(FV))
    cs, wit = M.generic_circuit(P.Fp, LOG_SRS, LOG_SRS, npub=3)
    out["public"] = Made(khip, srs, *circuit_records(khip, FV, P.Fp, cs, wit), public=3)
    assert set(out) == set(KINDS)
    # what makes the kinds different for phase 2: lookup index (with and without runtime table / table ids), optional gate, public inputs, previous challenges
    vi = {k: m.ix.native.verifier_index() for k, m in out.items()}
    assert [k for k in KINDS if vi[k]["lookup_info"]] == ["lookup", "xor"]
    assert len(vi["lookup"]["lookup_runtime_selector_comm"][1]) == 1 and len(vi["lookup"]["lookup_table_ids_comm"][1]) == 1
    assert [k for k in KINDS if len(vi[k]["optional_comm"][1])] == ["xor"]
    assert out["public"].public is not None and len(out["public"].public) == 3 and len(out["recursive"].prev) == 2
    yield out
    for m in out.values():
        m.free()
    srs.close()


def test_one_batch_of_every_kind_over_one_srs(khip, mixed):
    F = mixed["bench"].F
    items = [mixed[k].item() for k in KINDS]
    try:
        alone = []
        for k, it in zip(KINDS, items):
            ok, trace = khip.verify(*it)
            assert ok, k
            alone.append(trace)
        assert len({tuple(t["challenges"][2]) for t in alone}) == len(KINDS)    # every item its own alpha
        for rand in (F.limbs_many([0x1234567, 0x89abcdef01]), None):
            ok, traces = khip.batch_verify(items, rand)
            assert ok
            for k, want, got in zip(KINDS, alone, traces):
                same_trace(want, got, k)
        ok, traces = khip.batch_verify(items[::-1], None)                       # the same items at other positions of the column table
        assert ok
        for k, want, got in zip(KINDS[::-1], alone[::-1], traces):
            same_trace(want, got, (k, "reversed"))
    finally:
        for it in items:
            it[1].free()


def test_a_batch_of_130_items_spans_two_blocks(khip, mixed):
    """k_gate_batch_* runs 128 items per block: items 128 and 129 are the second block's, its other 126 lanes are clamped to item 129"""
    F = mixed["bench"].F
    secs = {k: mixed[k].prove(seed=70 + j) for j, k in enumerate(KINDS)}       # eight different proofs, one of every kind
    pool = {k: mixed[k].item(secs[k]) for k in KINDS}
    order = [KINDS[i % len(KINDS)] for i in range(130)]
    assert all(a != b for a, b in zip(order, order[1:])) and len({order[127], order[128], order[129]}) == 3
    lookups = [i for i, k in enumerate(order) if k in ("lookup", "xor")]
    assert min(lookups) < 128 <= max(lookups)
    items = [pool[k] for k in order]
    rand = F.limbs_many([0xfedcba987, 0x13579bdf02468])
    bad_items = []
    try:
        ok, traces = khip.batch_verify(items, rand)
        assert ok
        for i in (0, 127, 128, 129):
            ok, want = khip.verify(*items[i])
            assert ok
            same_trace(want, traces[i], (i, order[i]))
        for at in (129, 128):
            bad = list(items)
            bad[at] = mixed[order[at]].item(tampered(khip, khip.VESTA, secs[order[at]], "evals"))
            bad_items.append(bad[at])
            ok, _t = khip.batch_verify(bad, rand)
            assert not ok, at
    finally:
        for it in list(pool.values()) + bad_items:
            it[1].free()
