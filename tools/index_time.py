#!/usr/bin/env python3
"""Times kh_prover_index_create (the prover + verifier index from a gate list, one native call) against the Python ProverIndex path (+ set_wiring
where the circuit is wired) on the same circuits, on one device: the benchmark circuit (kimchi/src/bench.rs:59-96) at 2^16 and 2^20 over Vesta, and
generic_public (tests/golden/make_proof_fixtures.py: addition / multiplication gates, 3 public inputs, copy constraints) at 2^16; and
kh_prover_index_create_lookup against ProverIndex + LookupIndex + attach_lookup on two circuits with a lookup argument: and_lookup (the AND gadgets of
the committed fixture, XOR table) at 2^13 and a mixed circuit of RangeCheck0 / RangeCheck1 / Rot64 / ForeignFieldMul / Xor16 / Generic rows (both gate
tables, three patterns, five optional gates) at 2^16.  Every timed
call ends with a device synchronisation; one warm-up call per circuit first.  The native time is split into the phases the call records
(kh_prover_index_phase_seconds): validation + upload + column kernel, transforms, commitments, masking + digest.

    python tools/index_time.py [--reps 5] [--only lookup|plain] [--out profiles/index_time.txt] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def bench_records(khip, F, gates):
    types = np.full(gates, khip.gate_ids()["Generic"], dtype=np.int32)
    wires = np.zeros((gates, 7, 2), dtype=np.uint32)
    wires[:, :, 0] = np.arange(gates, dtype=np.uint32)[:, None]; wires[:, :, 1] = np.arange(7, dtype=np.uint32)[None, :]
    co = np.zeros((gates, 15, 4), dtype=np.uint64)
    co[:, 0, :] = F.limbs(1); co[:, 4, :] = F.limbs(F.p - 1)
    return types, wires, co


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("lookup", "plain"), default=None, help="the cases with / without a lookup argument alone")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    a = ap.parse_args()
    import proof_systems_amd.khip as khip
    from proof_systems_amd import prover
    import make_proof_fixtures as M
    from oracle import pasta as P
    khip.init(0)
    F = prover.Fld(khip.FP)
    lines = ["# tools/index_time.py --reps %d: seconds per call (median of the timed calls after one warm-up), device-synchronised" % a.reps]
    cases = []                                           # (name, log2_n, native create, Python path)
    gid = khip.gate_ids()

    def records(cs):
        rows = max(r for r, g in enumerate(cs["gates"]) if g["typ"] != "Zero") + 1
        special = {"Zero": khip.GATE_ZERO, "Lookup": khip.GATE_LOOKUP}
        gt = np.array([special[g["typ"]] if g["typ"] in special else gid[g["typ"]] for g in cs["gates"][:rows]], dtype=np.int32)
        gw = np.array([g["wires"] for g in cs["gates"][:rows]], dtype=np.uint32).reshape(rows, 7, 2)
        gc = np.stack([F.limbs_many([cs["coefficients"][k][r] for r in range(rows)]) for k in range(15)], axis=1)
        return gt, gw, gc, [g["typ"] for g in cs["gates"][:rows]], [g["wires"] for g in cs["gates"][:rows]]
    if a.only != "lookup":
        for logn in (16, 20):
            gates = (1 << logn) - 10
            t, w, c = bench_records(khip, F, gates)
            cases.append(("bench_vesta_2_%d" % logn, logn, lambda srs, t=t, w=w, c=c: khip.NativeProverIndex.create(srs, t, w, c, 0),
                          lambda srs, logn=logn: prover.bench_circuit_index(khip.VESTA, logn, srs)))
        cs = M.generic_circuit(P.VESTA.scalar, 16, 16)[0]
        gt, gw, gc, names, wl = records(cs)

        def py_generic(srs, cs=cs, gc=gc, names=names, wl=wl):
            ix = prover.ProverIndex(khip.VESTA, 16, gc, srs=srs, gate_types=names, public=cs["public"], zk_rows=cs["zk_rows"])
            ix.set_wiring(wl)
            return ix
        cases.append(("generic_public_vesta_2_16", 16, lambda srs, gt=gt, gw=gw, gc=gc, pub=cs["public"]: khip.NativeProverIndex.create(srs, gt, gw, gc, pub), py_generic))
    if a.only != "plain":
        from oracle import circuit as CC
        from proof_systems_amd import lookup as LK
        p = P.VESTA.scalar.p
        order = ["Generic", "RangeCheck0", "RangeCheck1", "Zero", "Rot64", "RangeCheck0", "ForeignFieldMul", "Zero", "Xor16", "Generic"]
        mixed = []
        for r in range(((1 << 16) - 16) // 10 * 10):
            t = order[r % 10]
            mixed.append(CC.gate(t, r, CC.generic_spec(p, "Add") + CC.generic_spec(p, "Mul") if t == "Generic" else [r + 1, 2 * r + 1, 3, 5] if t not in ("Zero", "Xor16") else []))
        for name, logn, cs in (("and_lookup_vesta_2_13", 13, M.and_circuit(P.VESTA.scalar, 13)[0]), ("mixed_lookup_vesta_2_16", 16, CC.build(P.VESTA.scalar, mixed))):
            assert cs["log2_n"] == logn and cs["lookup"] is not None
            gt, gw, gc, names, wl = records(cs)

            class PyLookupIndex:                         # the Python path's index and its lookup index, freed together
                def __init__(self, srs, cs=cs, gc=gc, names=names, wl=wl, logn=logn):
                    self.ix = prover.ProverIndex(khip.VESTA, logn, gc, srs=srs, gate_types=names, public=cs["public"], zk_rows=cs["zk_rows"])
                    self.ix.set_wiring(wl)
                    self.ix.attach_lookup(LK.LookupIndex(self.ix.fid, cs["gate_types"], [], logn, cs["zk_rows"]))

                def free(self):
                    self.ix.free_lookup(); self.ix.free()
            cases.append((name, logn, lambda srs, gt=gt, gw=gw, gc=gc: khip.NativeProverIndex.create_lookup(srs, gt, gw, gc, 0), PyLookupIndex))
    srs_cache = {}
    for name, logn, create, py in cases:
        srs = srs_cache.get(logn) or srs_cache.setdefault(logn, khip.Srs.create(khip.VESTA, 1 << logn))
        if srs.lagrange_chunks(logn) == 0:
            srs.compute_lagrange(logn)
        reps = a.reps if logn < 20 else max(2, a.reps // 2)
        nat, phases = [], []
        for i in range(reps + 1):
            khip.sync()
            t0 = time.perf_counter()
            ix = create(srs)
            khip.sync()
            dt = time.perf_counter() - t0
            if i:
                nat.append(dt); phases.append(ix.phase_seconds())
            ix.free()
        pyt = []
        for i in range(min(reps, 3) + 1):
            khip.sync()
            t0 = time.perf_counter()
            ix = py(srs)
            khip.sync()
            dt = time.perf_counter() - t0
            if i:
                pyt.append(dt)
            ix.free()
        med = lambda v: float(np.median(v))
        ph = {k: med([p[k] for p in phases]) for k in khip.INDEX_PHASES}
        lines.append("%-28s native %.4f s  [%s]  python %.4f s  (%.1fx)" % (name, med(nat), "  ".join("%s %.4f" % kv for kv in ph.items()), med(pyt),
                                                                            med(pyt) / med(nat)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines[1 if a.append else 0:]) + "\n")


if __name__ == "__main__":
    main()
