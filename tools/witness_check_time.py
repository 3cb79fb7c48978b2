#!/usr/bin/env python3
"""What kh_witness_check costs, and what a caller had before it.  On one MI355X: the 2^16 bench circuit (Generic only) and the 2^13 library_gates fixture
circuit, each satisfied and with one spoiled cell -- per-kernel times (kh_last_timings), the wall time of the call from a host and from a device
witness, next to a failing kh_prove(KH_PROVE_CHECK) on the same spoiled witness and the oracle's verify_witness on the CPU.  Best of `reps`.
Usage: tools/witness_check_time.py [reps] [--no-oracle]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_proof_fixtures as M  # noqa: E402
from oracle import circuit as CC, pasta as P  # noqa: E402
from proof_systems_amd import khip, prover  # noqa: E402


def best(fn, reps):
    out, t = None, float("inf")
    for _ in range(reps):
        khip.sync()
        t0 = time.perf_counter(); out = fn(); t = min(t, time.perf_counter() - t0)
    return t * 1e3, out


def case(name, cs, wit_cols, reps, oracle):
    F = prover.Fld(khip.FP)
    rows = len(wit_cols[0])
    gids = khip.gate_ids()
    types = [khip.GATE_ZERO if g["typ"] == "Zero" else gids[g["typ"]] for g in cs["gates"][:rows]]
    wires = np.array([g["wires"] for g in cs["gates"][:rows]], dtype=np.uint32)
    co = np.stack([F.limbs_many([cs["coefficients"][c][r] for r in range(rows)]) for c in range(15)], axis=1)
    ix = prover.CreatedIndex(khip.Srs.create(khip.VESTA, cs["n"]), types, wires, co, public=cs["public"])
    n = ix.n
    good = np.stack([F.limbs_many(col) for col in wit_cols])
    r = next(q for q in range(rows // 2, rows) if cs["gates"][q]["typ"] != "Zero")
    bad = good.copy(); bad[0, r] = F.limbs((wit_cols[0][r] + 1) % F.p)
    dev = khip.DevBuf(15 * n * 32)
    print(f"## {name}: 2^{ix.log2_n} rows, {rows} recorded, gates {sorted(ix.live_gate_types)}")
    for label, w in (("satisfied", good), ("spoiled (row %d, column 0)" % r, bad)):
        pad = np.zeros((15, n, 4), dtype=np.uint64); pad[:, :rows] = w
        dev.upload(pad)
        t_host, rep = best(lambda: khip.witness_check(ix.native, w), reps)
        t_dev, rep_d = best(lambda: khip.witness_check(ix.native, witness_dev=dev), reps)
        assert (rep.kind, rep.row) == (rep_d.kind, rep_d.row)
        khip.witness_check(ix.native, witness_dev=dev); khip.sync()
        kern = ", ".join(f"{k} {v * 1e3:.1f}" for k, v in khip.last_timings() if k.startswith("check_"))
        print(f"{label}: {khip.witness_report_message(rep)}")
        print(f"  kh_witness_check host witness {t_host:.3f} ms, device witness {t_dev:.3f} ms; kernels (us, each with its event gap): {kern}")
        if rep.kind != khip.WITNESS_OK:
            def failing():
                try:
                    prover.create_proof_native(ix, w, None, check=True)
                except khip.KhError as e:
                    return str(e)
                raise AssertionError("kh_prove accepted the spoiled witness")
            t_prove, msg = best(failing, reps)
            print(f"  kh_prove(KH_PROVE_CHECK) on the same witness: {t_prove:.3f} ms until '{msg[-60:]}'")
    if oracle:
        t0 = time.perf_counter(); CC.verify_witness(cs, wit_cols); t = time.perf_counter() - t0
        print(f"  oracle verify_witness (CPU, Python integers), satisfied witness: {t * 1e3:.0f} ms")
    dev.free(); ix.free()


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
    khip.init(0)
    cs, rows = M.bench_circuit(P.Fp, 16, 16)
    case("bench circuit", cs, [[1] * rows for _ in range(15)], reps, "--no-oracle" not in sys.argv)
    cs, wit = M.library_circuit(P.Fp, 13)
    case("library_gates fixture circuit", cs, wit, reps, "--no-oracle" not in sys.argv)
