#!/usr/bin/env python3
"""Wires between the gadgets on the device (csrc/wiring.hip): what kh_witness_gather_dev, kh_witness_scatter_dev and kh_generic_witness_dev cost on
one MI355X.

  static part (no GPU; hipcc cross-compiles): registers / scratch / occupancy of the kernels (-Rpass-analysis=kernel-resource-usage).
  timed part, both fields, each KH_CELL_* format: a scatter and a gather of n = 2^12 and 2^16 distinct cells spread over random rows and columns of a
    2^16-row witness, and one generic half over 2^16 rows.  Per call: the device time -- the library's own HIP-event phase (kh_last_timings) -- and
    the host's wall time around call + kh_sync; median [min .. max] of `reps` after two warm-up calls.  The scattered values are in range, so the
    gather that follows reads cells that fit and the flag word stays 0.
  The comparison, in the same run: what the library offered for one hop between two gadgets before these calls -- kh_dev_download of the n elements
    (which waits for the stream), then kh_dev_upload of n values of the target format and kh_sync (wall time; the host's conversion between the two is
    NOT in it, which flatters that path).  The condition is that a gather of n cells followed by a scatter of n cells (wall time of both calls +
    kh_sync; beside it the part that has passed when both calls have returned, what a caller pays who does not wait) takes less than that, at both
    sizes; every line says whether it does.  No other time is a threshold: nobody had measured these kernels.
  The clock state (rocm-smi --showclocks, read only) is recorded before and after the timed part.

Usage: tools/time_wiring.py [reps] [--static]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_limb_gadgets as TL  # noqa: E402  (static_part, clocks, call_ms: the same report for another source file)

TL.SRC = os.path.join(ROOT, "proof_systems_amd", "csrc", "wiring.hip")
ROWS = 1 << 16
SIZES = (1 << 12, 1 << 16)
FORMAT_NAMES = ("FIELD", "INT256", "INT128", "LIMB88", "U64")


def wall_ms(khip, fn, reps):
    """-> wall ms of fn + kh_sync, and of fn alone (until the calls have returned: what the host pays when nothing waits), each (median, min, max)"""
    def once():
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        khip.sync()
        return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3
    once(); once()
    runs = [once() for _ in range(reps)]
    total, queued = sorted(r[0] for r in runs), sorted(r[1] for r in runs)
    return (statistics.median(total), total[0], total[-1]), (statistics.median(queued), queued[0], queued[-1])


def values(rng, fmt, n, words):
    """n random values of a format, in range: (n, words) uint64"""
    a = rng.integers(0, 1 << 63, size=(n, words), dtype=np.uint64)
    if fmt <= 1:
        a[:, 3] &= np.uint64((1 << 60) - 1)                       # below p
    elif fmt == 3:
        a[:, 1] &= np.uint64((1 << 24) - 1)                       # below 2^88
    return a


def timed_part(reps):
    from proof_systems_amd import khip
    khip.init(0)
    TL.clocks("before")
    print(f"## per call: device time (the call's HIP-event phase) and wall time of call + kh_sync, median [min .. max] of {reps} after 2 warm-up calls;")
    print("## `hop before`: kh_dev_download of n elements + kh_dev_upload of n values of the format + kh_sync (wall), the host conversion not counted;")
    print(f"## `gather + scatter`: both calls + kh_sync (wall).  Cells: distinct, spread over random rows and columns of 15 x 2^{ROWS.bit_length() - 1}.")
    rng = np.random.default_rng(17)
    wit = khip.DevBuf(32 * 15 * ROWS).upload(values(rng, 0, 15 * ROWS, 4))
    missed, total = [], 0
    for n in SIZES:
        where = rng.choice(15 * ROWS, size=n, replace=False)
        cells = np.stack([where % ROWS, where // ROWS], axis=1).astype(np.uint32)
        elems = khip.DevBuf(32 * n).upload(values(rng, 0, n, 4))
        for fid, fname in ((khip.FP, "Fp"), (khip.FQ, "Fq")):
            for fmt, name in enumerate(FORMAT_NAMES):
                words = khip.CELL_WORDS[fmt]
                host = values(rng, fmt, n, words)
                dense = khip.DevBuf(8 * words * n).upload(host)
                flags = khip.DevBuf(4).zero()

                def hop_before():
                    elems.download((n, 4))
                    dense.upload(host)

                def pair():
                    khip.witness_gather_dev(fid, wit, ROWS, ROWS, cells, fmt, dense, flags=flags, bit=0)
                    khip.witness_scatter_dev(fid, dense, fmt, cells, wit, ROWS, ROWS, flags=flags, bit=1)

                sd, sw = TL.call_ms(khip, lambda: khip.witness_scatter_dev(fid, dense, fmt, cells, wit, ROWS, ROWS, flags=flags, bit=1), reps)
                gd, gw = TL.call_ms(khip, lambda: khip.witness_gather_dev(fid, wit, ROWS, ROWS, cells, fmt, dense, flags=flags, bit=0), reps)
                before, _q = wall_ms(khip, hop_before, reps)
                both, queued = wall_ms(khip, pair, reps)
                ok = both[0] < before[0]
                total += 1
                if not ok:
                    missed.append(f"{fname} {name} n = 2^{n.bit_length() - 1}")
                print(f"  {fname} {name:<6} n = 2^{n.bit_length() - 1}: scatter device {sd[0]:6.3f} ms [{sd[1]:.3f} .. {sd[2]:.3f}] wall {sw[0]:6.3f} ms [{sw[1]:.3f} .. {sw[2]:.3f}];  "
                      f"gather device {gd[0]:6.3f} ms [{gd[1]:.3f} .. {gd[2]:.3f}] wall {gw[0]:6.3f} ms [{gw[1]:.3f} .. {gw[2]:.3f}];  "
                      f"gather + scatter wall {both[0]:6.3f} ms [{both[1]:.3f} .. {both[2]:.3f}] ({queued[0]:.3f} ms until both calls have returned), hop before {before[0]:6.3f} ms [{before[1]:.3f} .. {before[2]:.3f}]: "
                      + (f"faster than the hop before ({before[0] / both[0]:.1f} x)" if ok else f"SLOWER than the hop before ({before[0] / both[0]:.2f} x)"), flush=True)
                assert int(flags.download((1,), dtype=np.uint32)[0]) == 0
                dense.free(); flags.free()
        elems.free()
    l, r, out = (khip.DevBuf(32 * ROWS).upload(values(rng, 0, ROWS, 4)) for _ in range(3))
    coeffs = values(rng, 0, 5, 4)
    for fid, fname in ((khip.FP, "Fp"), (khip.FQ, "Fq")):
        for half in (0, 1):
            d, w = TL.call_ms(khip, lambda: khip.generic_witness_dev(fid, coeffs, half, l, r, ROWS, wit, ROWS, ROWS, out=out), reps)
            print(f"  {fname} generic half {half} n = 2^{ROWS.bit_length() - 1} rows: device {d[0]:6.3f} ms [{d[1]:.3f} .. {d[2]:.3f}]  wall {w[0]:6.3f} ms [{w[1]:.3f} .. {w[2]:.3f}]  "
                  f"({(3 + 1 + 2) * 32 * ROWS / 1e6:.1f} MB moved)", flush=True)
    for b in (l, r, out, wit):
        b.free()
    TL.clocks("after")
    print("## condition (a gather of n cells followed by a scatter of n cells takes less wall time than download + upload + kh_sync of the same n values, "
          "at n = 2^12 and 2^16): " + ("met by every format in both fields" if not missed else f"MISSED by every one of the {total} lines above" if len(missed) == total
                           else "MISSED by " + ", ".join(missed)))


if __name__ == "__main__":
    reps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 9)
    assert reps >= 5
    TL.static_part()
    if "--static" not in sys.argv:
        timed_part(reps)
