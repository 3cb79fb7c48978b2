#!/usr/bin/env python3
"""kh_lookup_witness_dev (csrc/lookup_rows.hip) against the host hop it replaces, on one MI355X.

  static part (no GPU; hipcc cross-compiles): registers / scratch / occupancy of the kernels of lookup_rows.hip (-Rpass-analysis=kernel-resource-usage).
  timed part: n = 2^12 and 2^16 Lookup rows (one instance per row of a witness of n rows, 3 n keys) over a table of 2^12 entries, Fp.  The variants
    ALTERNATE in one process, 2 warm-up rounds and then `reps` (9) measured ones, median [min .. max]:
      (a) the host time until kh_lookup_witness_dev has returned,
      (b) its wall time including a closing kh_sync,
      (c) the hop it replaces, on entry points the library had before: kh_dev_download of the 3 n keys, kh_dev_upload_2d of seven cells per row
          (columns 0..6 of the n rows), then kh_sync -- wall time; the host's own table lookup is NOT counted, so (c) is a lower bound in the old
          path's favour,
      (d) the same call at n = 1, (a) and (b): the price of clearing and building the hash set over the 2^12 entries, which every call pays -- the
          number a later decision to cache the set per index has to rest on.
    The phase timers are off (kh_set_phase_timers(0), as under kh_prove).  Buffers are allocated outside the timed region.
  The condition, written down before the first run and reported per size as MET or MISSED: (b) < (c) at 2^12 and at 2^16.
  The clock state (rocm-smi --showclocks, read only) is recorded before and after the timed part.

Usage: tools/time_lookup_witness.py [reps] [--static] [--out FILE]      (FILE: profiles/lookup_witness_dev.txt unless given)"""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_limb_gadgets as TL  # noqa: E402  (clocks)
from time_witness_schedule import alternate, fmt  # noqa: E402

SRC = os.path.join(ROOT, "proof_systems_amd", "csrc", "lookup_rows.hip")
TABLE_LEN = 1 << 12
SIZES = (1 << 12, 1 << 16)


def static_part():
    """time_limb_gadgets.static_part for kernels that are not templates"""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, SRC], stderr=subprocess.PIPE, text=True, check=True)
    print("## kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    name, res = None, {}
    for l in r.stderr.split("\n"):
        m = re.search(r"Function Name: _ZN2kh(\d+)(\w+)", l)
        if m:
            name, res = m.group(2)[:int(m.group(1))], {}
        m = re.search(r"(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", l)
        if m and name:
            res[m.group(1).split(" ")[0]] = int(m.group(2))
            if m.group(1).startswith("LDS"):
                print(f"{name}: VGPRs {res['VGPRs']}, SGPRs {res['TotalSGPRs']}, scratch {res['ScratchSize']} B/lane, occupancy {res['Occupancy']} waves/SIMD, LDS {res['LDS']} B")


class Tee:
    def __init__(self, path):
        self.f, self.out = open(path, "w"), sys.stdout

    def write(self, s):
        self.f.write(s); self.out.write(s)

    def flush(self):
        self.f.flush(); self.out.flush()


def elements(rng, k):
    """k canonical elements of either field: the top limb is below 2^60"""
    v = rng.integers(0, 1 << 63, size=(k, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << 60) - 1)
    return v


def timed_part(reps):
    from proof_systems_amd import khip
    khip.init(0, timers=False)
    TL.clocks("before")
    print(f"## (a) host time until the call has returned, (b) wall time with a closing kh_sync, median [min .. max] of {reps} after 2 warm-up rounds,")
    print("## the variants alternating in one process.  Phase timers off.  Table: 2^12 entries.")
    rng = np.random.default_rng(23)
    tk, tv = elements(rng, TABLE_LEN), elements(rng, TABLE_LEN)
    tk_dev, tv_dev = khip.DevBuf(tk.nbytes).upload(tk), khip.DevBuf(tv.nbytes).upload(tv)
    tid = np.array([5, 0, 0, 0], dtype=np.uint64)
    verdicts = []
    for n in SIZES:
        pick = rng.integers(0, TABLE_LEN, size=3 * n)
        keys = tk[pick]
        keys_dev = khip.DevBuf(keys.nbytes).upload(keys)
        wit, flags = khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(4).zero()
        cells = np.zeros((7, n, 4), dtype=np.uint64)                  # what the host would send: id, key, value, key, value, key, value per row
        cells[0] = tid
        for k in range(3):
            cells[2 * k + 1], cells[2 * k + 2] = keys[k::3], tv[pick[k::3]]

        def dev(m=n):
            khip.lookup_witness_dev(khip.FP, tid, tk_dev, tv_dev, TABLE_LEN, keys_dev, m, wit, n, n, row0=0, row_stride=1, flags=flags, bit=0)

        def hop():
            keys_dev.download((3 * n, 4))
            wit.upload_2d(0, 32 * n, cells)

        r = alternate(khip, {"dev": dev, "hop": hop, "one": lambda: dev(1)}, reps)
        dev()
        got = wit.download((15, n, 4))
        assert np.array_equal(got[:7], cells) and not got[7:].any() and int(flags.download((1,), dtype=np.uint32)[0]) == 0
        ok = r["dev"][3] < r["hop"][3]
        verdicts.append((n, ok))
        print(f"  n = 2^{n.bit_length() - 1}: kh_lookup_witness_dev {fmt(r['dev'])};  (c) hop before {r['hop'][3]:6.3f} ms [{r['hop'][4]:.3f} .. {r['hop'][5]:.3f}];  "
              f"(d) n = 1 {fmt(r['one'])}: " + ("MET" if ok else "MISSED") + f" ((c) / (b) = {r['hop'][3] / r['dev'][3]:.2f})", flush=True)
        for b in (keys_dev, wit, flags):
            b.free()
    TL.clocks("after")
    missed = [f"2^{n.bit_length() - 1}" for n, ok in verdicts if not ok]
    print("## condition ((b) < (c) at 2^12 and at 2^16): " + ("MET at both sizes" if not missed else "MISSED at " + ", ".join(missed)))


if __name__ == "__main__":
    reps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 9)
    assert reps >= 5
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "lookup_witness_dev.txt")
    sys.stdout = Tee(out)
    static_part()
    if "--static" not in sys.argv:
        timed_part(reps)
