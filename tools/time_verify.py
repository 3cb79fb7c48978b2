#!/usr/bin/env python3
"""Times kh_verify / kh_batch_verify on the committed bench_vesta_2_16 proof (tests/golden/proof_fixtures/): the proof is made again by kh_prove from the
fixture's seed -- z1, z2 and ft_eval1 are compared with the committed bytes, so it is that proof --, then verified alone and as a batch of 8 (the same
proof eight times: the verifier's work does not depend on the proofs being different).  Median of 20 wall-clock runs after warm-up, split into the
phases kh_verify_last_phase_seconds reports: transcript (validation, Fiat-Shamir replay, public commitment), constant term (staged upload, one
launch per gate type, download), scalars (ft_eval0, combined inner product, the terms of SRS::verify), final MSM.
Usage: python tools/time_verify.py [runs]"""
import json
import os
import statistics
import sys
import time

import msgpack
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import proof_systems_amd.khip as khip  # noqa: E402
from oracle import pasta as P, views as V  # noqa: E402
from proof_systems_amd import prover  # noqa: E402

NAME = "bench_vesta_2_16"
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
fix = os.path.join(ROOT, "tests", "golden", "proof_fixtures")
rec = json.load(open(os.path.join(fix, NAME + ".json")))
raw = msgpack.unpackb(open(os.path.join(fix, NAME + ".proof.bin"), "rb").read(), raw=True)
khip.init(0)
F = prover.Fld(khip.FP)
rows = rec["gates"]
srs = khip.Srs.create(khip.VESTA, 1 << rec["log2_srs"])
wires = np.array([[[r, c] for c in range(7)] for r in range(rows)], dtype=np.uint32)
co = np.zeros((rows, 15, 4), dtype=np.uint64)
co[:, 0, :] = F.limbs(1); co[:, 4, :] = F.limbs(F.p - 1)                   # BenchmarkCtx::new (bench.rs:59-96): 1 * w0 - 1 = 0
ix = prover.CreatedIndex(srs, ["Generic"] * rows, wires, co)
nx = ix.native
rng = V.RefRng(P.StdRng(bytes.fromhex(rec["seed_hex"])))
sections = nx.prove(witness=np.tile(F.limbs(1), (15, rows, 1)), randomness=F.limbs_many(F.rand_many(rng, nx.randomness_count(True))))[0]
le = lambda b: int.from_bytes(bytes(b), "little")
committed = [le(raw[1][2]), le(raw[1][3]), le(raw[3])]                     # ProverProof: [commitments, [lr, delta, z1, z2, sg], evals, ft_eval1, prev]
assert F.values(sections["z1_z2"]) + F.values(sections["ft_eval1"]) == committed, "kh_prove did not reproduce the committed proof"
vix = khip.VerifierIndex.of(nx)
proof = khip.Proof(sections)


def measure(k):
    items = [(vix, proof)] * k
    for _ in range(3):
        ok, _tr = khip.batch_verify(items)
        assert ok
    wall, phases = [], {p: [] for p in khip.VERIFY_PHASES}
    for _ in range(runs):
        khip.sync()
        t0 = time.perf_counter()
        rc, ok, _tr = khip.batch_verify_raw(items)
        wall.append(time.perf_counter() - t0)
        assert rc == 0 and ok == 1
        for p, v in khip.verify_last_phase_seconds().items():
            phases[p].append(v)
    return statistics.median(wall), {p: statistics.median(v) for p, v in phases.items()}


print(f"{NAME}: domain 2^{rec['log2_n']}, SRS 2^{rec['log2_srs']}, {rows} generic gates; median of {runs} runs after 3 warm-up runs; wall clock incl. the ctypes call")
single, sp = measure(1)
batch, bp = measure(8)
for label, k, w, ph in (("kh_verify, one proof", 1, single, sp), ("kh_batch_verify, 8 proofs", 8, batch, bp)):
    host = ph["transcript"] + ph["scalars"]
    print(f"{label}: {1e3 * w:.3f} ms  =  transcript + scalars (host) {1e3 * host:.3f} ms [transcript {1e3 * ph['transcript']:.3f}, scalars {1e3 * ph['scalars']:.3f}]"
          f"  +  constant term (upload, launches, download) {1e3 * ph['constant_term']:.3f} ms  +  final MSM {1e3 * ph['final_msm']:.3f} ms")
print(f"batch of 8: {1e3 * batch:.3f} ms against 8 x single = {8e3 * single:.3f} ms  ({8 * single / batch:.2f}x)")
proof.free(); vix.free(); ix.free(); srs.close()
