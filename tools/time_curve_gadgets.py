#!/usr/bin/env python3
"""The curve gates' witness on the device (csrc/curve_gadgets.hip): what the four calls cost on one MI355X.

  static part (no GPU; hipcc cross-compiles): registers / scratch / occupancy of the kernels (-Rpass-analysis=kernel-resource-usage).
  timed part, both fields: kh_varbasemul_witness_dev at 255 bits and kh_endomul_witness_dev at 128 bits for n = 1, 64, 642 (the most a 2^16-row circuit
    holds) and 2^14; kh_complete_add_witness_dev and kh_endomul_scalar_witness_dev (128 bits) at 2^16.  Per call: the device time -- the sum of the
    library's own HIP-event phases (kh_last_timings: chain, denominators, cells per slice; the denominators phase contains the batch inversion's one
    host-side inversion and the stream wait before it) -- and the host's wall time around call + kh_sync; median [min .. max] of `reps` after two
    warm-up calls.  Inputs are random field elements (the arithmetic does not care whether a point is on the curve).
  Each VarBaseMul figure stands beside two estimates from the measured one-wave chain of profiles/poseidon_dev.txt (1155 products in 0.51 ms): the
    chain of this design, num_bits x (madd + add + 2) = 26 products per bit, and the chain of a lane that inverts twice per bit as the reference's
    generator does, 2 x num_bits x 380.  No time is a threshold: nobody had measured these kernels before.
  The clock state (rocm-smi --showclocks, read only) is recorded before and after the timed part.

Usage: tools/time_curve_gadgets.py [reps] [--static]"""
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, "proof_systems_amd", "csrc", "curve_gadgets.hip")
CHAIN_MS_PER_PRODUCT = 0.51 / 1155           # profiles/poseidon_dev.txt: one wave's chain of 55 x 21 products
CHAIN_SIZES = (1, 64, 642, 1 << 14)
ROW_SIZE = 1 << 16


def static_part():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, SRC], stderr=subprocess.PIPE, text=True, check=True)
    print("## kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    name, res = None, {}
    for l in r.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            mm = re.match(r"_ZN2kh(\d+)", m.group(1))                    # _ZN2kh7k_chainINS_8FpParamsELb1EEE... -> k_chain<FpParams, 1>
            k0 = mm.end(); k1 = k0 + int(mm.group(1))
            t = re.match(r"INS_\d+(\w+?)E(?:Lb(\d))?", m.group(1)[k1:])
            name = m.group(1)[k0:k1] + "<" + t.group(1) + (", endo = " + t.group(2) if t.group(2) else "") + ">"
            res = {}
        m = re.search(r"(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", l)
        if m and name:
            res[m.group(1).split(" ")[0]] = int(m.group(2))
            if m.group(1).startswith("LDS"):
                print(f"{name}: VGPRs {res['VGPRs']}, SGPRs {res['TotalSGPRs']}, scratch {res['ScratchSize']} B/lane, occupancy {res['Occupancy']} waves/SIMD, LDS {res['LDS']} B")


def clocks(label):
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=30).stdout
        lines = [l.strip() for l in out.split("\n") if re.search(r"GPU\[0\].*(sclk|mclk)", l)]
        print(f"## clocks {label}: " + ("; ".join(lines) if lines else "rocm-smi printed no sclk / mclk line for GPU[0]"))
    except Exception as e:                                                 # the tool may be missing: the times stand, their clock state is then unknown
        print(f"## clocks {label}: not recorded ({type(e).__name__})")


def call_ms(khip, fn, reps):
    """-> (device ms: median, min, max; wall ms: median; the phases of the median call)"""
    def once():
        t0 = time.perf_counter()
        fn(); khip.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ph = {}
        for k, ms in khip.last_timings():
            ph[k] = ph.get(k, 0.0) + ms
        return sum(ph.values()), wall, ph
    once(); once()                                                        # warm-up: code load, clocks, the pool's blocks
    runs = sorted((once() for _ in range(reps)), key=lambda r: r[0])
    dev = [r[0] for r in runs]
    return statistics.median(dev), dev[0], dev[-1], statistics.median(r[1] for r in runs), runs[len(runs) // 2][2]


def elements(rng, count):
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64); a[:, 3] &= np.uint64((1 << 61) - 1)      # any 4-limb value < p is a canonical element
    return a


def timed_part(reps):
    from proof_systems_amd import khip
    khip.init(0)
    clocks("before")
    print(f"## device time per call (HIP events around the phases, summed; median [min .. max] of {reps} after 2 warm-up calls) and wall time of call + kh_sync")
    rng = np.random.default_rng(11)
    for fid, fname in ((khip.FP, "Fp"), (khip.FQ, "Fq")):
        endo = khip.endos((khip.PALLAS, khip.VESTA)[fid])[0]
        for what, bits, inst, words in (("varbasemul", 255, 102, 4), ("endomul", 128, 33, 2)):
            for n in CHAIN_SIZES:
                base = khip.DevBuf(64 * n).upload(elements(rng, 2 * n)); acc0 = khip.DevBuf(64 * n).upload(elements(rng, 2 * n))
                sc = khip.DevBuf(8 * words * n).upload(rng.integers(0, 1 << 63, size=(n, words), dtype=np.uint64))
                wit = khip.DevBuf(32 * 15 * inst * n)
                if what == "varbasemul":
                    fn = lambda: khip.varbasemul_witness_dev(fid, base, acc0, sc, bits, n, wit, inst * n, inst * n)
                else:
                    fn = lambda: khip.endomul_witness_dev(fid, endo, base, acc0, sc, bits, n, wit, inst * n, inst * n)
                med, lo, hi, wall, ph = call_ms(khip, fn, reps)
                line = (f"{fname} {what:<10} {bits} bits n = {n:>6}: {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]  wall {wall:8.3f} ms  ("
                        + ", ".join(f"{k} {v:.3f}" for k, v in ph.items()) + f"; {(n + 63) // 64} waves of k_chain)")
                if what == "varbasemul":
                    line += (f"\n{'':<36}estimates from 0.51 ms / 1155 products: this chain, {26 * bits} products, {26 * bits * CHAIN_MS_PER_PRODUCT:.2f} ms; "
                             f"an inversion per slope, {2 * bits * 380} products, {2 * bits * 380 * CHAIN_MS_PER_PRODUCT:.1f} ms")
                print(line, flush=True)
                for b in (base, acc0, sc, wit):
                    b.free()
                khip.trim()
        n = ROW_SIZE
        p1 = khip.DevBuf(64 * n).upload(elements(rng, 2 * n)); p2 = khip.DevBuf(64 * n).upload(elements(rng, 2 * n))
        wit = khip.DevBuf(32 * 15 * 8 * n)
        med, lo, hi, wall, _ph = call_ms(khip, lambda: khip.complete_add_witness_dev(fid, p1, p2, n, wit, 8 * n, 8 * n), reps)
        print(f"{fname} complete_add         n = {n:>6}: {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]  wall {wall:8.3f} ms  ({n / med * 1e-3:.1f} M rows/s; one Fermat inversion per lane)")
        sc = khip.DevBuf(16 * n).upload(rng.integers(0, 1 << 63, size=(n, 2), dtype=np.uint64))
        med, lo, hi, wall, _ph = call_ms(khip, lambda: khip.endomul_scalar_witness_dev(fid, sc, 128, n, wit, 8 * n, 8 * n), reps)
        print(f"{fname} endomul_scalar 128 b n = {n:>6}: {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]  wall {wall:8.3f} ms  ({8 * n / med * 1e-3:.1f} M rows/s)", flush=True)
        for b in (p1, p2, wit, sc):
            b.free()
        khip.trim()
    clocks("after")


if __name__ == "__main__":
    reps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 9)
    assert reps >= 5
    static_part()
    if "--static" not in sys.argv:
        timed_part(reps)
