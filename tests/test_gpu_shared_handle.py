"""One SRS handle (and one index) shared by several host threads: up to KH_IPA_OPENINGS openings run over a handle's window tables at once, each with
a workspace and a U slot of its own (include/kimchi_hip.h, kh_ipa_begin).  The reference's provers share one Arc<SRS> and call
SRS::open(&self) from several threads (poly-commitment/src/ipa.rs:898-1060); every value an opening produces beside others must be the bytes it
produces alone.

No thread may stay parked: all threads are daemon threads, every barrier / join / event wait has a time limit, and every path out of an opening frees it
(a begin that waits for a workspace then goes on and ends by itself)."""
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAIT = 15.0                      # seconds: every barrier, event wait and join below

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def _rs(rng, k):
    a = rng.integers(0, 1 << 64, size=(k, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 61) - 1)                    # any 4-limb value < p is a valid Montgomery element
    return a


def _case(khip, cid, logn, seed):
    """seeded inputs of one opening: a (shorter than the SRS), b, the U base, the blinders of every round, the challenges"""
    n = 1 << logn
    rng = np.random.default_rng(1000 * seed + 10 * logn + cid)
    return {"a": _rs(rng, max(1, n - 3)), "b": _rs(rng, n), "U": khip.srs_generate(cid, (1 << 21) + seed, 1)[0], "r": _rs(rng, 2 * logn),
            "chals": [int.from_bytes(rng.bytes(16), "little") for _ in range(logn)]}


def _open_steps(khip, srs, case, sync=None, op=None):
    """One opening through the step API: [L | R and their flags of every round ..., a0, b0, sg, its flag] as bytes.  sync(): called behind the begin and
    behind every round.  The opening is freed whatever happens."""
    op = khip.IpaOpening(srs, case["a"], case["b"], case["U"]) if op is None else op
    try:
        out = []
        if sync:
            sync()
        for j, ch in enumerate(case["chals"]):
            xy, inf = op.round_lr(case["r"][2 * j], case["r"][2 * j + 1])
            out += [xy.tobytes(), inf.tobytes()]
            op.round_fold(ch)
            if sync:
                sync()
        a0, b0, sg, sginf = op.finish()
        return out + [a0.tobytes(), b0.tobytes(), np.asarray(sg).tobytes(), bytes([int(bool(sginf))])]
    finally:
        op.free()


_STUCK = []                      # threads that did not end in time: whatever they may still be using is not freed any more


def _settle(threads):
    """waits (with a limit) for the threads to end; the ones that do not are remembered"""
    for t in threads:
        t.join(timeout=WAIT + 5)
    _STUCK.extend(t for t in threads if t.is_alive())


def _release(*handles):
    """closes / frees the handles -- unless a thread of this module may still be inside a call on one of them: then they are leaked (a failing test must not
    free device tables under a running opening)"""
    if any(t.is_alive() for t in _STUCK):
        return
    for h in handles:
        if h is not None:
            (h.close if hasattr(h, "close") else h.free)()


def _in_threads(targets):
    """runs the callables in daemon threads; returns (results, errors) once all have ended -- or fails if one has not"""
    res, errs = [None] * len(targets), []

    def run(i, f):
        try:
            res[i] = f()
        except BaseException as e:                         # noqa: BLE001 -- reported by the caller
            errs.append((i, repr(e)))
    th = [threading.Thread(target=run, args=(i, f), daemon=True) for i, f in enumerate(targets)]
    for t in th:
        t.start()
    _settle(th)
    assert not any(t.is_alive() for t in th), "a thread is still running"
    return res, errs


def _interleaved(khip, cid, logn):
    """two openings alone, then the same two from two threads in lockstep (a barrier behind both begins and behind each round):
    (sequential, concurrent, growth of the counters over the concurrent pair, errors)"""
    names = ("ipa_concurrent", "rebase_switch", "rebase_abandon")
    srs = khip.Srs.create(cid, 1 << logn)
    try:
        cases = [_case(khip, cid, logn, s) for s in (1, 2)]
        want = [_open_steps(khip, srs, c) for c in cases]
        before = {k: khip.counter(k) for k in names}
        bar = threading.Barrier(2)

        def sync():
            bar.wait(timeout=WAIT)                         # (a time-out breaks the barrier for the other thread too: both free their openings and end)
        got, errs = _in_threads([lambda c=c: _open_steps(khip, srs, c, sync) for c in cases])
        return want, got, {k: khip.counter(k) - before[k] for k in names}, errs
    finally:
        _release(srs)


@pytest.mark.parametrize("cid,logn", [(0, 3), (1, 3), (0, 10), (1, 10)])
def test_interleaved_rounds_of_two_openings_on_one_handle(khip, cid, logn):
    """Two openings with different inputs on ONE handle, their rounds forced to alternate: the second begin must not wait for the first opening to be freed
    (the barrier behind the begins would time out), every L, R, a0, b0, sg equals the opening run alone, and ipa_concurrent counts the second begin.
    8 points: no window tables (the plain MSM path over n + 1 + KH_IPA_OPENINGS points); 2^10: tables, the rebase planned."""
    want, got, grown, errs = _interleaved(khip, cid, logn)
    assert not errs, errs
    assert got[0] == want[0] and got[1] == want[1]
    assert want[0] != want[1]
    assert grown["ipa_concurrent"] >= 1


def _child(mode):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=dict(os.environ, **({"KH_IPA_REBASE_WAIT": "1"} if mode == "rebased" else {"KH_IPA_REBASE": "0"})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def test_interleaved_openings_switch_to_their_own_rebased_tables():
    """The same two interleaved openings at 2^10 in a process with KH_IPA_REBASE_WAIT=1: each materialises its folded basis in its own workspace and switches
    to it at the earliest round (rebase_switch grows by 2 over the concurrent pair); the bytes are those of a process that never rebases (KH_IPA_REBASE=0)."""
    plain = _child("plain")
    reb = _child("rebased")
    assert plain["errors"] == [] and reb["errors"] == []
    assert plain["grown"]["rebase_switch"] == 0
    assert reb["grown"]["rebase_switch"] == 2 and reb["grown"]["rebase_abandon"] == 0
    assert reb["concurrent"] == reb["sequential"] == plain["sequential"] == plain["concurrent"]
    assert reb["grown"]["ipa_concurrent"] >= 1


def _whole_opening(khip, srs, cid, n, seed):
    """kh_ipa_open with seeded inputs: every output as bytes"""
    rng = np.random.default_rng(7000 + seed)
    logn = n.bit_length() - 1
    a_dev = khip.DevBuf(n * 32); b_dev = khip.DevBuf(n * 32)
    sp = khip.Sponge(khip.Sponge.FQ, cid)
    try:
        a_dev.upload(_rs(rng, n)); b_dev.upload(_rs(rng, n))
        sp.absorb_fr(_rs(rng, 2))
        out = khip.ipa_open(srs, a_dev, b_dev, n, _rs(rng, 1)[0], _rs(rng, 1)[0], sp, _rs(rng, 2 * logn + 2))
        return [np.asarray(x).tobytes() if not isinstance(x, bool) else bytes([int(x)]) for x in out]
    finally:
        sp.free(); a_dev.free(); b_dev.free()


def test_four_whole_openings_at_once(khip):
    """Four threads, each one kh_ipa_open (sponge, rounds, the halves of sg on a side slot, delta, z1, z2) with its own inputs on one 2^12 handle: the
    results are the four obtained one after the other.  (Whether they overlap is timing; the bytes are the assertion.)"""
    cid, n = 0, 1 << 12
    srs = khip.Srs.create(cid, n)
    try:
        want = [_whole_opening(khip, srs, cid, n, s) for s in range(4)]
        assert len({tuple(w) for w in want}) == 4
        got, errs = _in_threads([lambda s=s: _whole_opening(khip, srs, cid, n, s) for s in range(4)])
        assert not errs, errs
        assert got == want
    finally:
        _release(srs)


def test_the_fifth_opening_waits_for_a_workspace(khip):
    """KH_IPA_OPENINGS threads begin and hold; a further begin blocks (ipa_waited grows BEFORE it blocks, which is how this test sees it) until one holder
    frees, then completes; all five results are the ones obtained alone and no call returns an error."""
    cid, logn, K = 0, 10, khip.IPA_OPENINGS
    srs = khip.Srs.create(cid, 1 << logn)
    go = [threading.Event() for _ in range(K)]
    th = []
    try:
        cases = [_case(khip, cid, logn, 10 + s) for s in range(K + 1)]
        want = [_open_steps(khip, srs, c) for c in cases]
        begun = threading.Barrier(K + 1)
        res, errs = [None] * (K + 1), []

        def holder(t):
            try:
                op = khip.IpaOpening(srs, cases[t]["a"], cases[t]["b"], cases[t]["U"])
                first = [True]

                def held():                                # behind the begin only, not behind every round
                    if first[0]:
                        first[0] = False
                        begun.wait(timeout=WAIT)
                        assert go[t].wait(timeout=WAIT), "never released"
                res[t] = _open_steps(khip, srs, cases[t], sync=held, op=op)
            except BaseException as e:                     # noqa: BLE001
                errs.append((t, repr(e)))
                begun.abort()

        def fifth():
            try:
                res[K] = _open_steps(khip, srs, cases[K])
            except BaseException as e:                     # noqa: BLE001
                errs.append((K, repr(e)))
        th += [threading.Thread(target=holder, args=(t,), daemon=True) for t in range(K)]
        for t in th:
            t.start()
        waited0 = khip.counter("ipa_waited")
        begun.wait(timeout=WAIT)                           # four openings are live, each on its own workspace
        f = threading.Thread(target=fifth, daemon=True)
        th.append(f)
        f.start()
        deadline = time.monotonic() + WAIT
        while khip.counter("ipa_waited") == waited0 and time.monotonic() < deadline and f.is_alive():
            time.sleep(0.001)
        saw_wait = khip.counter("ipa_waited") - waited0
        still_blocked = f.is_alive() and res[K] is None
        go[0].set()                                        # one holder finishes and frees: the fifth gets its workspace
        f.join(timeout=WAIT)
        assert not f.is_alive(), "the fifth opening never got a workspace"
        for e in go:
            e.set()
        _settle(th)
        assert not any(t.is_alive() for t in th)
        assert not errs, errs
        assert saw_wait == 1 and still_blocked
        assert res == want
    finally:
        for e in go:                                       # whatever failed: every holder goes on, frees its opening and ends before the handle is closed
            e.set()
        _settle(th)
        _release(srs)


@pytest.mark.parametrize("logn", [3, 10])
def test_a_second_begin_by_the_same_thread_is_still_an_error(khip, logn):
    """openings of ONE thread do not interleave on a handle: KH_E_INVALID as before, and the first opening is unharmed"""
    cid = 1
    srs = khip.Srs.create(cid, 1 << logn)
    try:
        c1, c2 = _case(khip, cid, logn, 21), _case(khip, cid, logn, 22)
        want = _open_steps(khip, srs, c1)
        op = khip.IpaOpening(srs, c1["a"], c1["b"], c1["U"])
        try:
            with pytest.raises(khip.KhError, match="in this thread"):
                khip.IpaOpening(srs, c2["a"], c2["b"], c2["U"])
        except BaseException:
            op.free()
            raise
        assert _open_steps(khip, srs, c1, op=op) == want
    finally:
        _release(srs)


def test_provers_share_one_index(khip):
    """Three threads run kh_prove over ONE index (one SRS handle: their openings overlap on it) with the same seeded randomness, several proofs each: every
    proof is the proof made alone (the comparison of test_native_provers_on_several_threads); one proof per thread with the library's own randomness is
    accepted by kh_verify (against the verifier index of the same circuit built from its gate list on the same SRS handle: an index made from columns
    carries none)."""
    from oracle import views as V
    from proof_systems_amd import prover
    ix = prover.bench_circuit_index(khip.VESTA, 10)
    vix = cix = None
    try:
        F, n = ix.F, ix.n
        rows = n - 10
        wit = np.zeros((15, rows, 4), dtype=np.uint64); wit[0, :, :] = F.limbs(1)
        alone = V.device_views(ix, prover.create_proof_native(ix, wit, np.random.default_rng(77)))[2]
        nx = prover.native_index(ix)
        co = np.zeros((rows, 15, 4), dtype=np.uint64)
        co[:, 0, :] = F.limbs(1); co[:, 4, :] = F.limbs(F.p - 1)           # bench_circuit_index: 1 * w0 - 1 = 0, every cell wired to itself
        cix = prover.CreatedIndex(ix.srs, ["Generic"] * rows, np.array([[[r, c] for c in range(7)] for r in range(rows)], dtype=np.uint32), co)
        assert np.array_equal(np.asarray(cix.digest).reshape(-1), np.asarray(ix.digest).reshape(-1))
        vix = khip.VerifierIndex.of(cix.native)

        def work():
            seeded = [V.device_views(ix, prover.create_proof_native(ix, wit, np.random.default_rng(77), check=(r == 0)))[2] for r in range(3)]
            return seeded, nx.prove(witness=wit, randomness=None)[0]
        got, errs = _in_threads([work] * 3)
        assert not errs, errs
        for seeded, sections in got:
            assert all(s == alone for s in seeded)
            proof = khip.Proof(sections)
            try:
                assert khip.verify(vix, proof)[0]
            finally:
                proof.free()
    finally:
        _release(vix, cix, ix)


@pytest.mark.parametrize("logn", [3, 10])
def test_blinding_base_is_refused_during_an_opening_and_used_after_it(khip, logn):
    """kh_srs_set_blinding_base while an opening is live: KH_E_INVALID (the rounds read H from the handle's tables).  After the free it is accepted and the next
    opening's first L is the one a fresh handle with that H gives -- and not the one under the old H."""
    cid = 0
    c = _case(khip, cid, logn, 31)
    H2 = khip.srs_generate(cid, 12345, 1)[0]
    srs, fresh = khip.Srs.create(cid, 1 << logn), khip.Srs.create(cid, 1 << logn)

    def first_l(s):
        op = khip.IpaOpening(s, c["a"], c["b"], c["U"])
        try:
            return op.round_lr(c["r"][0], c["r"][1])[0].tobytes()
        finally:
            op.free()
    try:
        op = khip.IpaOpening(srs, c["a"], c["b"], c["U"])
        try:
            old = op.round_lr(c["r"][0], c["r"][1])[0].tobytes()           # (H is in the tables now: the new one must replace it)
            with pytest.raises(khip.KhError, match="opening is in progress"):
                srs.set_blinding_base(H2)
        finally:
            op.free()
        assert np.array_equal(srs.blinding_commitment(), khip.srs_h(cid))
        srs.set_blinding_base(H2)
        fresh.set_blinding_base(H2)
        new = first_l(srs)
        assert new == first_l(fresh)
        assert new != old
    finally:
        _release(srs, fresh)


def test_wide_tables_are_not_released_under_another_contexts_msm(khip):
    """A handle is shared between contexts: kh_srs_set_wide_tables(srs, 0) is refused while ANY context has an MSM over the handle in flight.  One thread submits
    from a private context and keeps the ticket; this thread (the shared context, whose own slots are idle) asks for the release."""
    from oracle import cref
    n = 1 << 12
    rng = np.random.default_rng(5)
    g = cref.srs_generate(0, 0, n, threads=8)
    sc = _rs(rng, n)
    want, winf = cref.msm(0, g, sc, threads=8)
    khip.set_wide_min_n(n)
    submitted, release = threading.Event(), threading.Event()
    srs, started = None, []
    try:
        srs = khip.Srs(khip.VESTA, g)
        assert srs.has_wide_tables()

        def submitter():
            lib = khip.raw()
            assert lib.kh_private_context_begin() == 0
            try:
                ticket = srs.msm_submit_host(sc)
                try:
                    khip.sync()                            # the kernels are done: what is in flight is the JOB (its slot, its ticket), which is what the handle counts
                    submitted.set()
                    assert release.wait(timeout=WAIT), "never released"
                finally:
                    out, inf = khip.Srs.msm_wait(ticket)
                return out[0].tobytes(), bool(inf[0])
            finally:
                lib.kh_private_context_end()
        res, errs = [None], []

        def run():
            try:
                res[0] = submitter()
            except BaseException as e:                     # noqa: BLE001
                errs.append(repr(e))
                submitted.set()
        t = threading.Thread(target=run, daemon=True)
        started.append(t)
        t.start()
        assert submitted.wait(timeout=WAIT)
        assert not errs, errs
        refused = None
        try:
            srs.set_wide_tables(False)
        except khip.KhError as e:
            refused = str(e)
        finally:
            release.set()
        t.join(timeout=WAIT)
        assert not t.is_alive() and not errs, errs
        assert refused is not None and "in flight" in refused
        assert srs.has_wide_tables()
        assert res[0] == (want.tobytes(), bool(winf))
        srs.set_wide_tables(False)                         # the job has been waited for: released now
        assert not srs.has_wide_tables()
        got, ginf = srs.msm(sc)
        assert ginf == winf and np.array_equal(got, want)
    finally:
        release.set()
        _settle(started)
        khip.set_wide_min_n(1 << 19)
        _release(srs)


if __name__ == "__main__":                                 # the child process of test_interleaved_openings_switch_to_their_own_rebased_tables
    sys.path.insert(0, ROOT)
    import proof_systems_amd.khip as _khip
    _khip.init(0)
    _want, _got, _grown, _errs = _interleaved(_khip, 0, 10)
    digest = lambda parts: hashlib.sha256(b"".join(b"".join(p) for p in parts)).hexdigest() if all(p is not None for p in parts) else None
    print(json.dumps({"sequential": digest(_want), "concurrent": digest(_got), "errors": _errs, "grown": _grown}))
