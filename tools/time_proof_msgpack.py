#!/usr/bin/env python3
"""Serialised proofs and verifier indexes at the C ABI (csrc/proof_msgpack.cpp) against the route a caller had before, on one MI355X.

Conditions, written down before the first run.  Routes ALTERNATE in one process, 2 warm-up rounds and then `reps` (9) measured ones; every figure is the
wall time of the call with a closing kh_sync, median [min .. max].  Phase timers off.  Inputs are built outside the timed region, handles are freed
outside it.  The times include the ctypes call overhead of the Python wrapper, on both sides alike.  No figure here is a pass / fail threshold: what
comes out is reported.  The expectation: the framing walk adds microseconds to calls that are bound by one kernel launch and its copies.
  intake, 1 and 8 proofs of the fixture bench_vesta_2_16 (proved here by kh_prove_full, serialised by kh_proof_to_msgpack):
    new   kh_proofs_from_msgpack on the msgpack bytes: structure walk + one decode launch;
    old   kh_proofs_from_wire on sections split beforehand (the parent's route; its split -- the caller's serde -- is NOT timed: a bound in its favour.
          profiles/point_codec.txt has it at 0.485 / 0.842 ms).
  kh_verifier_index_from_msgpack on the index bytes of the same circuit (27 commitments through one decode launch, the digest sponge on the host), beside
    kh_verifier_index_of on the prover index (no decode: the cost of the handle alone).
  kh_proof_to_msgpack (size query + one encode launch + the walk) and kh_verifier_index_to_msgpack.
The clock state (rocm-smi --showclocks, read only) is recorded before and after.

Usage: tools/time_proof_msgpack.py [reps] [--out FILE]      (FILE: profiles/proof_msgpack.txt unless given)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time_limb_gadgets as TL  # noqa: E402  (clocks)
from time_lookup_witness import Tee  # noqa: E402
from time_point_codec import alternate, fmt  # noqa: E402


def timed_part(reps):
    from oracle import pasta as P, views as V
    from proof_systems_amd import khip as K
    from test_gpu_index_create import fixture_case
    K.init(0, timers=False)
    print(f"## serialised proofs and indexes: one MI355X (gfx950), {time.strftime('%Y-%m-%d')}")
    TL.clocks("before")
    rec, want, _C, ix, wit, prev = fixture_case(K, "bench_vesta_2_16")
    F, nx, cid = ix.F, ix.native, K.VESTA
    rnd = F.limbs_many(F.rand_many(V.RefRng(P.StdRng(bytes.fromhex(rec["seed_hex"]))), nx.randomness_count(True)))
    proof = nx.prove_handle(witness=wit, randomness=rnd, prev=prev)
    blob = proof.to_msgpack(cid)
    assert blob == want, "kh_proof_to_msgpack does not give the committed proof bytes"
    wire = proof.to_wire(cid)
    vix = K.VerifierIndex.of(nx)
    vblob = vix.to_msgpack(0)
    free = lambda made: [p.free() for p in made]
    free1 = lambda h: h.free()
    none = lambda _r: None
    print(f"## intake of bench_vesta_2_16 proofs ({len(blob)} bytes each), wall time with a closing kh_sync, median [min .. max] of {reps}")
    for k in (1, 8):
        blobs, wires = [blob] * k, [wire] * k
        r = alternate(K, {"new": (lambda: K.Proof.from_msgpack(cid, blobs), free), "old": (lambda: K.proofs_from_wire(cid, wires), free)}, reps)
        print(f"  {k} proof{'s' if k > 1 else ' '}: new  kh_proofs_from_msgpack (walk + one decode launch)        {fmt(r['new'])}")
        print(f"            old  kh_proofs_from_wire on pre-split sections               {fmt(r['old'])}")
        print(f"            new - old (medians) = {1e3 * (r['new'][0] - r['old'][0]):.1f} us")
    srs = ix.srs
    r = alternate(K, {"from_msgpack": (lambda: K.VerifierIndex.from_msgpack(srs, vblob), free1), "of": (lambda: K.VerifierIndex.of(nx), free1),
                      "proof_to": (lambda: proof.to_msgpack(cid), none), "index_to": (lambda: vix.to_msgpack(0), none)}, reps)
    print(f"## the index of the same circuit ({len(vblob)} bytes) and the writers, median [min .. max] of {reps}")
    print(f"  kh_verifier_index_from_msgpack (walk + one decode launch + digest)     {fmt(r['from_msgpack'])}")
    print(f"  kh_verifier_index_of (no decode)                                       {fmt(r['of'])}")
    print(f"  kh_proof_to_msgpack (size query, then one encode launch + walk)        {fmt(r['proof_to'])}")
    print(f"  kh_verifier_index_to_msgpack (size query, then one encode launch)      {fmt(r['index_to'])}")
    back = K.VerifierIndex.from_msgpack(srs, vblob)
    assert back.to_msgpack(0) == vblob and (back.digest() == vix.digest()).all()
    back.free(); vix.free(); proof.free(); ix.free()
    TL.clocks("after")


if __name__ == "__main__":
    reps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 9)
    assert reps >= 5
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "proof_msgpack.txt")
    sys.stdout = Tee(out)
    timed_part(reps)
