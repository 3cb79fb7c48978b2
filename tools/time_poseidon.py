#!/usr/bin/env python3
"""Poseidon on the device (csrc/poseidon.hip): what the three kernels cost on one MI355X, next to their VALU issue bound.

  static part (no GPU; hipcc cross-compiles): registers / scratch / occupancy of the six kernels (-Rpass-analysis=kernel-resource-usage) and the VALU
    instructions of one permutation -- the opcode histogram of the rolled round loop of k_poseidon_permute<FpParams> x 55; the same for the three-lane kernel -- priced with the per-opcode issue
    cycles of profiles/r04_valu_rates.json (tools/microbench.hip), the way DESIGN.md section 3 prices k_acc_wide29: instructions x cycles / 1024 SIMDs / 2.4 GHz.
    A wave cannot finish before its own instructions have issued, so below 1024 waves the bound is ONE wave's issue time.
  timed part: n = 5461 (the gadgets of one 2^16-row circuit), 2^16, 2^20 permutations on both fields; device time of each kernel from the library's own
    HIP events around the launch (kh_last_timings; median of `reps` after a warm-up), permutations/s, fraction of the issue bound at the nominal clock.
    k_poseidon_hash is timed on two-element messages (one permutation per hash); kh_poseidon_gate_witness_dev at row stride 12 in columns of 12 n rows, once
    with each of its kernels (kh_poseidon_set_split_max_n: k_poseidon_gate_rows, one lane per permutation; k_poseidon_gate_rows3, three).
  context line: the same number of permutations through kh_sponge_absorb on ONE host thread (csrc/host_sponge.cpp), no device.

Usage: tools/time_poseidon.py [reps] [--static] [--permute-only] [--no-host]     (KH_LIB=<another build> times that build: the same-box A/B of two builds)"""
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, "proof_systems_amd", "csrc", "poseidon.hip")
ROUNDS, SIMDS, CLOCK = 55, 1024, 2.4e9
SIZES = (5461, 1 << 16, 1 << 20)


def static_part():
    """-> {kernel: (issue cycles of one wave, permutations per wave)}"""
    rates = json.load(open(os.path.join(ROOT, "profiles", "r04_valu_rates.json")))
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "poseidon.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                            "-o", asm, SRC], stderr=subprocess.PIPE, text=True, check=True)
        lines = open(asm).read().split("\n")
    print("## kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    name = None
    for l in r.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            mm = re.match(r"_ZN2kh(\d+)", m.group(1))                    # _ZN2kh18k_poseidon_permuteINS_8FpParamsEEE... -> k_poseidon_permute<FpParams>
            k0 = mm.end(); k1 = k0 + int(mm.group(1))
            name = m.group(1)[k0:k1] + "<" + re.match(r"INS_\d+(\w+?)E", m.group(1)[k1:]).group(1) + ">"
            res = {}
        m = re.search(r"(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", l)
        if m and name:
            res[m.group(1).split(" ")[0]] = int(m.group(2))
            if m.group(1).startswith("LDS"):
                print(f"{name}: VGPRs {res['VGPRs']}, SGPRs {res['TotalSGPRs']}, scratch {res['ScratchSize']} B/lane, occupancy {res['Occupancy']} waves/SIMD, LDS {res['LDS']} B")
    print("## VALU instructions of one permutation (static: the kernel's one loop, the rolled rounds, x 55 + what is outside it)")
    cycles = {}
    for kname, per_wave, what in (("k_poseidon_permute", 64, "one lane per permutation: 21 products per round"),
                                  ("k_poseidon_gate_rows3", 21, "three lanes per permutation: 7 products per round and lane")):
        kern = "_ZN2kh%d%sINS_8FpParamsE" % (len(kname), kname)
        start = next(i for i, l in enumerate(lines) if l.startswith(kern) and l.split(";")[0].strip().endswith(":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [l.split(";")[0].strip() for l in lines[start + 1:end]]
        body = [l for l in body if l and (not l.startswith(".") or l.endswith(":"))]
        labels = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
        back = [(labels[l.split()[1]], i) for i, l in enumerate(body) if l.startswith(("s_cbranch", "s_branch")) and l.split()[1] in labels and labels[l.split()[1]] < i]
        assert back, "no loop (the rolled rounds) in " + kname
        lo, hi = min(b[0] for b in back), max(b[1] for b in back)     # one source loop: the compiler may lay it out with several backward branches
        ops = lambda seg: [l.split()[0] for l in seg if not l.endswith(":")]
        loop, rest = ops(body[lo:hi + 1]), ops(body[:lo] + body[hi + 1:])
        assert "s_swappc_b64" not in loop, "the round loop calls a function: its instructions are not in the loop's count"
        hist = Counter(op for op in loop if op.startswith("v_"))
        cyc = lambda h: sum(c * rates["cycles"].get(o.replace("_e32", "").replace("_e64", ""), rates["default_cycles"]) for o, c in h.items())
        valu_loop, valu_rest = sum(hist.values()), sum(op.startswith("v_") for op in rest)
        wave_cycles = ROUNDS * cyc(hist) + cyc(Counter(op for op in rest if op.startswith("v_")))
        cycles[kname] = (wave_cycles, per_wave)
        print(f"{kname}<FpParams> ({what}; {per_wave} permutations per wave)")
        print(f"  round loop: {len(loop)} instructions, {valu_loop} VALU ({hist['v_mad_u64_u32']} v_mad_u64_u32), {sum(op.startswith('ds_bpermute') for op in loop)} ds_bpermute_b32, "
              f"{4 * len(loop) / 1024:.0f}-{8 * len(loop) / 1024:.0f} KB of code; outside the loop {valu_rest} VALU")
        print(f"  per wave: {ROUNDS * valu_loop + valu_rest} VALU instructions, {wave_cycles:.0f} issue cycles at {cyc(hist) / valu_loop:.2f} cycles per instruction "
              f"(profiles/r04_valu_rates.json) = {wave_cycles / CLOCK * 1e6:.1f} us at 2.4 GHz")
        print("  top opcodes per round: " + ", ".join(f"{o} {c}" for o, c in hist.most_common(8)))
    return cycles


def issue_bound_ms(wave_cycles, per_wave, n):
    waves = (n + per_wave - 1) // per_wave
    return wave_cycles * max(1.0, waves / SIMDS) / CLOCK * 1e3


def kernel_ms(khip, name, fn, reps):
    def once():
        fn(); khip.sync()
        t = [ms for k, ms in khip.last_timings() if k == name]
        assert len(t) == 1, (name, khip.last_timings())
        return t[0]
    once(); once()                                                        # warm-up: code load, clocks
    ts = [once() for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def timed_part(cycles, reps, permute_only):
    from proof_systems_amd import khip
    khip.init(0)
    print(f"## device time per kernel (library {os.path.basename(khip.LIB_PATH)}; HIP events around the launch, median [min .. max] of {reps} after 2 warm-up launches)")
    rng = np.random.default_rng(5)
    for fid, fname in ((khip.FP, "Fp"), (khip.FQ, "Fq")):
        for n in SIZES:
            st = rng.integers(0, 1 << 63, size=(3 * n, 4), dtype=np.uint64); st[:, 3] &= np.uint64((1 << 61) - 1)      # any 4-limb value < p is a canonical element
            states = khip.DevBuf(96 * n).upload(st)
            one, three = cycles["k_poseidon_permute"], cycles["k_poseidon_gate_rows3"]
            cases = [("poseidon_permute", one, lambda: khip.poseidon_permute_dev(fid, states, n))]
            if not permute_only:
                dig = khip.DevBuf(32 * n)
                wit = khip.DevBuf(32 * 15 * 12 * n)

                def gate_rows(split_max):
                    khip.poseidon_set_split_max_n(split_max)
                    khip.poseidon_gate_witness_dev(fid, states, n, wit, 12 * n, 12 * n)
                    khip.poseidon_set_split_max_n()
                cases += [("poseidon_hash", one, lambda: khip.poseidon_hash_dev(fid, states, 2, n, dig)),
                          ("poseidon_gate_rows", one, lambda: gate_rows(0)),
                          ("poseidon_gate_rows3", three, lambda: gate_rows(1 << 40))]
            for name, (wave_cycles, per_wave), fn in cases:
                bound = issue_bound_ms(wave_cycles, per_wave, n)
                med, lo, hi = kernel_ms(khip, name, fn, reps)
                print(f"{fname} n = {n:>7} k_{name:<19} {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]  {n / med * 1e-3:8.2f} M permutations/s  "
                      f"issue bound {bound:.3f} ms -> {bound / med:.2f} of it ({(n + per_wave - 1) // per_wave} waves)")
            states.free()
            if not permute_only:
                dig.free(); wit.free()
            khip.trim()


def host_part():
    from proof_systems_amd import khip
    print("## context, NOT a device number: the same permutations through kh_sponge_absorb on one host thread (2 n elements absorbed = n - 1 permutations)")
    rng = np.random.default_rng(6)
    for curve, fname in ((khip.VESTA, "Fp"), (khip.PALLAS, "Fq")):
        for n in SIZES:
            x = rng.integers(0, 1 << 63, size=(2 * n, 4), dtype=np.uint64); x[:, 3] &= np.uint64((1 << 61) - 1)
            sp = khip.Sponge(khip.Sponge.FR, curve)
            t0 = time.perf_counter(); sp.absorb(x); t = time.perf_counter() - t0
            print(f"host {fname} n = {n:>7}: {t * 1e3:9.2f} ms ({t / (n - 1) * 1e6:.2f} us per permutation)")


if __name__ == "__main__":
    reps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 9)
    assert reps >= 7
    wc = static_part()
    if "--static" not in sys.argv:
        timed_part(wc, reps, "--permute-only" in sys.argv)
        if "--no-host" not in sys.argv and "--permute-only" not in sys.argv:
            host_part()
