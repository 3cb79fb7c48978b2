#!/usr/bin/env python3
"""The value steps (csrc/value_steps.hip: kh_field_inverse_dev, kh_field_sqrt_dev, kh_field_bits_dev) against the host hop they replace, on one MI355X.

  static part (no GPU; hipcc cross-compiles): registers / scratch / occupancy of the three kernels (-Rpass-analysis=kernel-resource-usage).
  timed part: the is_zero circuit of tests/test_gpu_value_steps.py -- per instance one double generic row, b = 1 - x y and x b = 0, y = the inverse of
    x or zero -- at 2^12 and 2^16 instances over Fp, x in column 0 of a witness of as many rows.  Two routes ALTERNATE in one process, 2 warm-up rounds
    and then `reps` (9) measured ones, median [min .. max]:
      new: ONE kh_witness_schedule_run: gather x into the arena, KH_STEP_INVERSE, the two generic halves;
      old: schedule part 1 (everything in front of the advice: here the gather of x, into a bound buffer), kh_dev_download of x, kh_dev_upload of y,
           kh_sync, schedule part 2 (the two generic halves).  The host's own inversion is NOT timed (y is computed beforehand), in the old route's
           favour.
    For each route (a) the host time until its last call has returned and (b) the wall time with a closing kh_sync.  The phase timers are off
    (kh_set_phase_timers(0), as under kh_prove).  Buffers and schedules are created outside the timed region.
  The condition, written down before the first run, on (a): the new route's median is below the old route's at both sizes AND the min .. max ranges
    do not overlap: MET; ranges that overlap: LEVEL; a median that is not below: MISSED.  (b) is reported with no condition: at 2^12 one lone Fermat
    chain of about 0.2 ms on the device is expected to lose to a hop of 33-41 us on wall time.
  The clock state (rocm-smi --showclocks, read only) is recorded before and after the timed part.

  --kernels: nothing is timed by the tool; the three direct calls run 5 times at 2^12 and 2^16 elements (Fp; squares for the root; 64 bits of a
    KH_CELL_FIELD value) for a run of their own under `rocprofv3 --kernel-trace --stats`, and the field products per element that the shapes and
    the launcher's constants give are printed for the file.
  --parse DIR: the kernel times of such a run (the *kernel_trace.csv under DIR), median per kernel and grid.

Usage: tools/time_value_steps.py [reps] [--static] [--kernels] [--parse DIR] [--out FILE]      (FILE: profiles/value_steps_dev.txt unless given)"""
import csv
import glob
import os
import random
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time_limb_gadgets as TL  # noqa: E402  (clocks)
from time_lookup_witness import Tee  # noqa: E402
from time_witness_schedule import alternate, fmt  # noqa: E402

CSRC = os.path.join(ROOT, "proof_systems_amd", "csrc")
SIZES = (1 << 12, 1 << 16)
P_FP = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001


def stamp(what):
    print(f"## {what}: one MI355X (gfx950), {time.strftime('%Y-%m-%d')}")


def static_part():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, os.path.join(CSRC, "value_steps.hip")], stderr=subprocess.PIPE, text=True, check=True)
    print("## kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    name, res = None, {}
    for l in r.stderr.split("\n"):
        m = re.search(r"Function Name: _ZN2kh(\d+)(\w+)", l)
        if m:
            name, res = m.group(2)[:int(m.group(1))] + ("<Fp>" if "FpParams" in l else "<Fq>"), {}
        m = re.search(r"(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", l)
        if m and name:
            res[m.group(1).split(" ")[0]] = int(m.group(2))
            if m.group(1).startswith("LDS"):
                print(f"{name}: VGPRs {res['VGPRs']}, SGPRs {res['TotalSGPRs']}, scratch {res['ScratchSize']} B/lane, occupancy {res['Occupancy']} waves/SIMD, LDS {res['LDS']} B")


def launcher_constants():
    src = open(os.path.join(CSRC, "api_internal.hpp")).read()
    return int(re.search(r"INV_RUN = (\d+);", src).group(1)), int(re.search(r"INV_MAX_BLOCKS = (\d+);", src).group(1))


def mont(vals):
    return np.frombuffer(b"".join((v % P_FP * (1 << 256) % P_FP).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def timed_part(reps):
    from oracle import circuit as CC
    from proof_systems_amd import khip
    K = khip
    K.init(0, timers=False)
    stamp("timed part")
    TL.clocks("before")
    print(f"## is_zero circuit, Fp: (a) host time until the route's last call has returned, (b) wall time with a closing kh_sync, median [min .. max] of {reps}")
    print("## after 2 warm-up rounds, the routes alternating in one process.  Phase timers off.  The old route's host inversion is not timed.")
    p, fid = P_FP, K.FP
    half0, half1 = mont([0, 0, 1, 1, -1]), mont([0, 0, 0, 1, 0])
    assert CC.generic_spec(p, "Mul") == [0, 0, p - 1, 1, 0]           # (the coefficient order l r o m c)
    rnd = random.Random(41)
    verdicts = []
    for n in SIZES:
        e = 32 * n
        xs = [0 if i % 97 == 5 else rnd.randrange(1, 1 << 64) for i in range(n)]
        ys = mont([pow(x, -1, p) if x else 0 for x in xs])           # the host's turn of the old route, done beforehand
        cells = [(i, 0) for i in range(n)]
        A = lambda off: (K.REF_ARENA, off)
        gen = lambda x, y, b: [dict(op=K.STEP_GENERIC, n=n, row0=0, row_stride=1, param=0, consts=half0, out=[b], **{"in": [x, y]}),
                               dict(op=K.STEP_GENERIC, n=n, row0=0, row_stride=1, param=1, consts=half1, **{"in": [x, b]})]
        new = K.WitnessSchedule.create(fid, n, [dict(op=K.STEP_GATHER, cells=cells, format=K.CELL_FIELD, out=[A(0)]),
                                                dict(op=K.STEP_INVERSE, n=n, out=[A(e)], **{"in": [A(0)]})] + gen(A(0), A(e), A(2 * e)), arena_bytes=3 * e, n_bufs=0)
        part1 = K.WitnessSchedule.create(fid, n, [dict(op=K.STEP_GATHER, cells=cells, format=K.CELL_FIELD, out=[(0, 0)])], arena_bytes=0, n_bufs=2)
        part2 = K.WitnessSchedule.create(fid, n, gen((0, 0), (1, 0), A(0)), arena_bytes=e, n_bufs=2)
        start = np.zeros((15, n, 4), dtype=np.uint64)
        start[0] = mont(xs)
        wit_new, wit_old = K.DevBuf(start.nbytes).upload(start), K.DevBuf(start.nbytes).upload(start)
        xbuf, ybuf = K.DevBuf(e), K.DevBuf(e)

        def route_new():
            new.run([], wit_new)

        def route_old():
            part1.run([xbuf, ybuf], wit_old)
            xbuf.download((n, 4))
            ybuf.upload(ys)
            K.sync()
            part2.run([xbuf, ybuf], wit_old)

        r = alternate(K, {"new": route_new, "old": route_old}, reps)
        got = wit_new.download(start.shape)
        assert np.array_equal(got, wit_old.download(start.shape)) and np.array_equal(got[1], ys) and np.array_equal(got[2], mont([int(x == 0) for x in xs]))
        verdict = "MISSED" if r["new"][0] >= r["old"][0] else "MET" if r["new"][2] < r["old"][1] else "LEVEL"
        verdicts.append((n, verdict))
        print(f"  n = 2^{n.bit_length() - 1}: new {fmt(r['new'])};  old {fmt(r['old'])}: (a) {verdict} (old / new = {r['old'][0] / r['new'][0]:.2f}), "
              f"(b) old / new = {r['old'][3] / r['new'][3]:.2f}", flush=True)
        for s in (new, part1, part2):
            s.free()
        for b in (wit_new, wit_old, xbuf, ybuf):
            b.free()
    TL.clocks("after")
    print("## condition on (a) (new below old at 2^12 and at 2^16, ranges apart): " + ", ".join(f"2^{n.bit_length() - 1} {v}" for n, v in verdicts))


def sqrt_products(a):
    """the field products fe_sqrt spends on one element of Fp (the oracle's loop, counted)"""
    p = P_FP
    t = (p - 1) >> 32
    e = (t - 1) // 2
    count = e.bit_length() + bin(e).count("1") + 2 + 31              # the ladder as the kernel walks it, x and b, the residue test
    if a == 0:
        return 0
    z, w = pow(5, t, p), pow(a, e, p)
    x = a * w % p
    b = x * w % p
    if pow(b, 1 << 31, p) != 1:
        return count
    v = 32
    while b != 1:
        k, c = 0, b
        while c != 1:
            c = c * c % p; k += 1
        w = pow(z, 1 << (v - k - 1), p)
        z = w * w % p; b = b * z % p; x = x * w % p
        count += k + (v - k - 1) + 3
        v = k
    return count


def kernels_part():
    from proof_systems_amd import khip
    K = khip
    K.init(0, timers=False)
    run, max_blocks = launcher_constants()
    stamp("kernel-trace run")
    chain = 254 + bin((P_FP - 2) & ((1 << 254) - 1)).count("1")
    print(f"## field products per element (Fp), from the shapes and INV_RUN = {run}, INV_MAX_BLOCKS = {max_blocks}:")
    print(f"##   k_field_inverse: (3 ({run} - 1) + {chain}) / {run} = {(3 * (run - 1) + chain) / run:.2f} (a Fermat chain each: {chain}); blocks of 64 lanes: "
          + ", ".join(f"{min((n + 64 * run - 1) // (64 * run), max_blocks)} at 2^{n.bit_length() - 1}" for n in SIZES))
    rnd = random.Random(43)
    for n in SIZES:
        vals = [rnd.randrange(1, P_FP) for _ in range(n)]
        sq = [v * v % P_FP for v in vals]
        per = [sqrt_products(a) for a in sq]
        waves = [max(per[i:i + 64]) for i in range(0, n, 64)]
        print(f"##   k_field_sqrt at 2^{n.bit_length() - 1} (random squares): mean {statistics.mean(per):.1f} per element, {statistics.mean(waves):.1f} per wave (its longest lane)")
        x, s = K.DevBuf(32 * n).upload(mont(vals)), K.DevBuf(32 * n).upload(mont(sq))
        out, bits = K.DevBuf(32 * n), K.DevBuf(32 * n * 64)
        for _ in range(5):
            K.field_inverse_dev(K.FP, x, n, out)
            K.field_sqrt_dev(K.FP, s, n, out)
            K.field_bits_dev(K.FP, x, K.CELL_FIELD, 64, n, bits)
        K.sync()
        for b in (x, s, out, bits):
            b.free()
    print("##   k_field_bits (KH_CELL_FIELD, 64 bits): the reduction half of one product per element, 64 stores of 32 bytes")


def parse_part(where):
    rows = []
    for f in glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "k_field_" in r["Kernel_Name"]]
    groups = {}
    for r in rows:
        name = re.search(r"k_field_\w+?(?=<|I?NS|\(|$)", r["Kernel_Name"])
        key = (name.group(0) if name else r["Kernel_Name"], int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"]))
        groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("## rocprofv3 --kernel-trace, a run of its own (tools/time_value_steps.py --kernels): kernel time in us, median [min .. max] of the dispatches")
    for (name, grid), t in sorted(groups.items()):
        print(f"  {name} grid {grid} lanes: {statistics.median(t):8.1f} us [{min(t):.1f} .. {max(t):.1f}] ({len(t)} dispatches)")


if __name__ == "__main__":
    reps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 9)
    assert reps >= 5
    if "--kernels" in sys.argv:
        kernels_part()
        sys.exit(0)
    if "--parse" in sys.argv:
        parse_part(sys.argv[sys.argv.index("--parse") + 1])
        sys.exit(0)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "value_steps_dev.txt")
    sys.stdout = Tee(out)
    static_part()
    if "--static" not in sys.argv:
        timed_part(reps)
