#!/usr/bin/env python3
"""What kh_witness_check costs, and what a caller had before it.  On one MI355X: the 2^16 bench circuit (Generic only) and the 2^13 library_gates fixture
circuit, each satisfied and with one spoiled cell -- per-kernel times (kh_last_timings), the wall time of the call from a host and from a device
witness, next to a failing kh_prove(KH_PROVE_CHECK) on the same spoiled witness and the oracle's verify_witness on the CPU.  Best of `reps`.
Then the lookups (kh_witness_check_full with KH_WITNESS_LOOKUPS): the 2^13 and_lookup fixture circuit (Xor16) and a 2^16 range-check circuit, each
satisfied and with one spoiled limb -- the call from a device witness, the two kernels, and kh_prove's own refusal of the same witness.
Usage: tools/witness_check_time.py [reps] [--no-oracle] [--no-lookups]"""
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


def lookup_case(name, cs, wit_cols, spoil, reps):
    """spoil = (row, column, value): one looked-up cell that leaves its table"""
    F = prover.Fld(khip.FP)
    rows = len(wit_cols[0])
    gids = khip.gate_ids()
    types = [khip.GATE_ZERO if g["typ"] == "Zero" else gids[g["typ"]] for g in cs["gates"][:rows]]
    wires = np.array([g["wires"] for g in cs["gates"][:rows]], dtype=np.uint32)
    co = np.stack([F.limbs_many([cs["coefficients"][c][r] for r in range(rows)]) for c in range(15)], axis=1)
    ix = prover.CreatedIndex(khip.Srs.create(khip.VESTA, cs["n"]), types, wires, co, public=cs["public"])
    n = ix.n
    good = np.stack([F.limbs_many([v % F.p for v in col]) for col in wit_cols])
    r, c, v = spoil
    bad = good.copy(); bad[c, r] = F.limbs(v % F.p)
    dev = khip.DevBuf(15 * n * 32)
    print(f"## {name}: 2^{ix.log2_n} rows, {rows} recorded, gates {sorted(ix.live_gate_types)}, patterns {ix.lookup.patterns}")
    L_, ALL = khip.WITNESS_LOOKUPS, khip.WITNESS_GATES | khip.WITNESS_WIRES | khip.WITNESS_LOOKUPS
    for label, w in (("satisfied", good), ("spoiled (row %d, column %d)" % (r, c), bad)):
        pad = np.zeros((15, n, 4), dtype=np.uint64); pad[:, :rows] = w
        dev.upload(pad)
        t_l, (rep, lk) = best(lambda: khip.witness_check_full(ix.native, witness_dev=dev, flags=L_), reps)
        khip.sync()
        kern = ", ".join(f"{k} {v_ * 1e3:.1f}" for k, v_ in khip.last_timings() if k.startswith("check_lookup"))
        t_all, (rep_a, lk_a) = best(lambda: khip.witness_check_full(ix.native, witness_dev=dev, flags=ALL), reps)
        t_old, _ = best(lambda: khip.witness_check(ix.native, witness_dev=dev), reps)
        assert lk.lookups_missing == lk_a.lookups_missing
        print(f"{label}: {khip.witness_lookup_message(rep, lk)}")
        print(f"  kh_witness_check_full device witness: lookups alone {t_l:.3f} ms, gates + wires + lookups {t_all:.3f} ms (kh_witness_check, gates + wires: {t_old:.3f} ms); "
              f"kernels (us, each with its event gap): {kern}")
        if rep.kind != khip.WITNESS_OK:
            def failing():
                try:
                    prover.create_proof_native(ix, w, None, check=True)
                except khip.KhError as e:
                    return str(e)
                raise AssertionError("kh_prove accepted the spoiled witness")
            t_prove, msg = best(failing, reps)
            print(f"  kh_prove(KH_PROVE_CHECK) on the same witness: {t_prove:.3f} ms until '{msg[-70:]}'")
    dev.free(); ix.free()


def range_check_circuit(F, log2_n):
    """RangeCheck0 rows (coefficient 0: the row stands alone) up to the domain: six 12-bit limbs and eight crumbs of an 88-bit value per row"""
    import random
    rnd = random.Random(16)
    rows = (1 << log2_n) - 8
    gates = [CC.gate("RangeCheck0", r, [0]) for r in range(rows)]
    wit = [[0] * rows for _ in range(15)]
    for r in range(rows):
        v = rnd.randrange(1 << 88)
        wit[0][r] = v
        for k in range(6):
            wit[1 + k][r] = (v >> (76 - 12 * k)) & 4095
        for k in range(8):
            wit[7 + k][r] = (v >> (14 - 2 * k)) & 3
    cs = CC.build(F, gates)
    assert cs["log2_n"] == log2_n, cs["log2_n"]
    return cs, wit


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
    khip.init(0)
    cs, rows = M.bench_circuit(P.Fp, 16, 16)
    case("bench circuit", cs, [[1] * rows for _ in range(15)], reps, "--no-oracle" not in sys.argv)
    cs, wit = M.library_circuit(P.Fp, 13)
    case("library_gates fixture circuit", cs, wit, reps, "--no-oracle" not in sys.argv)
    if "--no-lookups" not in sys.argv:
        cs, wrows = M.and_circuit(P.Fp, 13)
        wit = [[r[c] for r in wrows] for c in range(15)]
        lookup_case("and_lookup fixture circuit", cs, wit, (2, 4, 16), reps)
        cs, wit = range_check_circuit(P.Fp, 16)
        lookup_case("range-check circuit", cs, wit, (len(wit[0]) // 2, 5, 4096), reps)
