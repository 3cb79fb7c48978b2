#!/usr/bin/env python3
"""The optional gates' witness on the device (csrc/limb_gadgets.hip): what the five calls cost on one MI355X.

  static part (no GPU; hipcc cross-compiles): registers / scratch / occupancy of the kernels (-Rpass-analysis=kernel-resource-usage).
  timed part, both fields: each call at the instance count that fills 2^16 rows and at the one that fills 2^20 (16384 / 262144 multi-range-checks,
    21845 / 349525 rotations, 13107 / 209715 64-bit xors, 32768 / 524288 foreign-field additions and multiplications), instances packed densely.
    Per call: the device time -- the library's own HIP-event phase (kh_last_timings) -- and the host's wall time around call + kh_sync; median
    [min .. max] of `reps` after two warm-up calls; the bytes of witness cells written / device time as a fraction of 8 TB/s, the HBM figure VERDICT.md
    uses.  Inputs are random integers in range.
  The comparison, in the same run: the only way the rows reached the device before these calls, kh_dev_upload_2d of the same 15 columns of that many
    rows from host memory (wall time of upload + kh_sync; the host's generation of the rows is NOT in it, which flatters the upload).  The condition is
    that each call at the 2^16-row size takes less wall time than that upload; every line says whether it does.  No other time is a threshold: nobody
    had measured these kernels before.
  The clock state (rocm-smi --showclocks, read only) is recorded before and after the timed part.

Usage: tools/time_limb_gadgets.py [reps] [--static]"""
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, "proof_systems_amd", "csrc", "limb_gadgets.hip")
HBM_BYTES_PER_S = 8e12
ROW_SIZES = (1 << 16, 1 << 20)
SECP = (1 << 256) - (1 << 32) - 977


def static_part():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, SRC], stderr=subprocess.PIPE, text=True, check=True)
    print("## kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    name, res = None, {}
    for l in r.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            mm = re.match(r"_ZN2kh(\d+)", m.group(1))                    # _ZN2kh8k_ff_mulINS_8FpParamsEEE... -> k_ff_mul<FpParams>
            k0 = mm.end(); k1 = k0 + int(mm.group(1))
            t = re.match(r"INS_\d+(\w+?)E", m.group(1)[k1:])
            name = m.group(1)[k0:k1] + "<" + t.group(1) + ">"
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


def call_ms(khip, fn, reps, timed_phases=True):
    """-> device ms (median, min, max), wall ms (median, min, max)"""
    def once():
        t0 = time.perf_counter()
        fn(); khip.sync()
        wall = (time.perf_counter() - t0) * 1e3
        return (sum(ms for _k, ms in khip.last_timings()) if timed_phases else 0.0), wall
    once(); once()                                                        # warm-up: code load, clocks, the pool's blocks
    runs = [once() for _ in range(reps)]
    dev, wall = sorted(r[0] for r in runs), sorted(r[1] for r in runs)
    return (statistics.median(dev), dev[0], dev[-1]), (statistics.median(wall), wall[0], wall[-1])


def limbs(rng, count):
    """count random 88-bit limbs as (count, 2) uint64"""
    a = rng.integers(0, 1 << 63, size=(count, 2), dtype=np.uint64)
    a[:, 1] &= np.uint64((1 << 24) - 1)
    return a


def elements(rng, count):
    """count random foreign elements below 2^255 (below every modulus used here) as (3 count, 2) uint64"""
    a = limbs(rng, 3 * count)
    a[2::3, 1] &= np.uint64((1 << 15) - 1)
    return a


def timed_part(reps):
    from proof_systems_amd import khip
    khip.init(0)
    clocks("before")
    print(f"## per call: device time (the call's HIP-event phase) and wall time of call + kh_sync, median [min .. max] of {reps} after 2 warm-up calls;")
    print("## cells written / device time against 8 TB/s; beside it kh_dev_upload_2d of the same 15 columns from host memory (wall, upload + kh_sync)")
    nprng = np.random.default_rng(11)
    missed = []
    for rows in ROW_SIZES:
        host = nprng.integers(0, 1 << 62, size=(15, rows, 4), dtype=np.uint64)
        wit = khip.DevBuf(32 * 15 * rows)
        _d, up = call_ms(khip, lambda: wit.upload_2d(0, 32 * rows, host), reps, timed_phases=False)
        print(f"rows = 2^{rows.bit_length() - 1}: kh_dev_upload_2d of 15 x {rows} elements ({15 * 32 * rows / 1e6:.1f} MB): wall {up[0]:8.3f} ms [{up[1]:.3f} .. {up[2]:.3f}]",
              flush=True)
        for fid, fname in ((khip.FP, "Fp"), (khip.FQ, "Fq")):
            def dev(arr):
                return khip.DevBuf(arr.nbytes).upload(arr)
            n4, n5, n3, n2 = rows // 4, rows // 5, rows // 3, rows // 2
            rc_in = dev(limbs(nprng, 3 * n4))
            x1, x2 = dev(nprng.integers(0, 1 << 63, size=(n5, 4), dtype=np.uint64) * np.array([1, 0, 0, 0], dtype=np.uint64)), \
                dev(nprng.integers(0, 1 << 63, size=(n5, 4), dtype=np.uint64) * np.array([1, 0, 0, 0], dtype=np.uint64))
            words = dev(nprng.integers(0, 1 << 63, size=(n3,), dtype=np.uint64))
            fa, fb = dev(elements(nprng, n2)), dev(elements(nprng, n2))
            checks = khip.DevBuf(144 * n2)
            flags = khip.DevBuf(4).zero()
            calls = (
                ("range_check", n4, 60, lambda: khip.range_check_witness_dev(fid, rc_in, n4, wit, rows, rows, flags=flags)),
                ("range_check compact", n4, 60, lambda: khip.range_check_witness_dev(fid, rc_in, n4, wit, rows, rows, compact=True, flags=flags)),
                ("xor 64 bits", n5, 75, lambda: khip.xor_witness_dev(fid, x1, x2, 64, n5, wit, rows, rows, flags=flags)),
                ("rot64 by 13", n3, 45, lambda: khip.rot64_witness_dev(fid, words, 13, n3, wit, rows, rows)),
                ("foreign_field_add", n2, 11, lambda: khip.foreign_field_add_witness_dev(fid, SECP, fa, fb, 1, n2, wit, rows, rows, flags=flags)),
                ("foreign_field_mul", n2, 27, lambda: khip.foreign_field_mul_witness_dev(fid, SECP, fa, fb, n2, wit, rows, rows, flags=flags)),
                ("foreign_field_mul + out_checks", n2, 27 + 4.5, lambda: khip.foreign_field_mul_witness_dev(fid, SECP, fa, fb, n2, wit, rows, rows, out_checks=checks,
                                                                                                          flags=flags)),
            )
            for what, n, cells, fn in calls:
                d, w = call_ms(khip, fn, reps)
                nbytes = 32 * cells * n
                verdict = "faster than the upload" if w[0] < up[0] else "SLOWER than the upload"
                if w[0] >= up[0] and rows == ROW_SIZES[0]:
                    missed.append(f"{fname} {what}")
                print(f"  {fname} {what:<31} n = {n:>7}: device {d[0]:7.3f} ms [{d[1]:.3f} .. {d[2]:.3f}]  wall {w[0]:7.3f} ms [{w[1]:.3f} .. {w[2]:.3f}]  "
                      f"{nbytes / 1e6:6.1f} MB written, {nbytes / (d[0] * 1e-3) / HBM_BYTES_PER_S * 100 if d[0] > 0 else float('nan'):5.1f} % of 8 TB/s; {verdict} "
                      f"({up[0] / w[0]:.1f} x)", flush=True)
            assert int(flags.download((1,), dtype=np.uint32)[0]) == 0
            for b in (rc_in, x1, x2, words, fa, fb, checks, flags):
                b.free()
        wit.free()
        khip.trim()
    clocks("after")
    print("## condition (each call at 2^16 rows takes less wall time than the upload of the same columns): "
          + ("met by every call" if not missed else "MISSED by " + ", ".join(missed)))


if __name__ == "__main__":
    reps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 9)
    assert reps >= 5
    static_part()
    if "--static" not in sys.argv:
        timed_part(reps)
