#!/usr/bin/env python3
"""Every kernel launch of one MSM per path of the driver (csrc/msm_plan.hpp), for a comparison of two builds launch by launch.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o TAG -- python tools/msm_launch_list.py run      (KH_LIB selects the build)
    python tools/msm_launch_list.py compare PARENT_kernel_trace.csv CHANGE_kernel_trace.csv

run: seeded scalars, once each, synchronous -- the wide path (set_wide_min_n, as smoke() reaches it), the partitioned sort (15 columns of 2^15), the
one-launch sort (2^12 over the tables), the multi-launch sort over the tables (a batch of 5 at 2^12), a plain basis of 512 points, and one kh_ipa_open at 2^13
(the spread hint, the rebased GLV tables; KH_IPA_REBASE_WAIT=1 makes the round of the switch the same in every run).
compare: both traces in dispatch order, side by side: kernel, grid, workgroup, LDS bytes; the last line says whether they are the same list."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    os.environ.setdefault("KH_IPA_REBASE_WAIT", "1")
    sys.path.insert(0, ROOT)
    import numpy as np
    from proof_systems_amd import khip
    khip.init(0)
    rng = np.random.default_rng(11)

    def rs(*shape):
        a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
        a[..., 3] &= np.uint64((1 << 61) - 1)
        return a

    n = 1 << 12
    khip.set_wide_min_n(n)
    srs = khip.Srs.create(khip.VESTA, n)
    srs.msm(rs(n)); srs.close()                                 # wide windows
    khip.set_wide_min_n(1 << 19)
    srs = khip.Srs.create(khip.VESTA, 1 << 15)
    srs.msm_batch(rs(15, 1 << 15)); srs.close()                 # partitioned sort, digit planes
    srs = khip.Srs.create(khip.VESTA, n)
    srs.msm(rs(n))                                              # one-launch sort
    srs.msm_batch(rs(5, n)); srs.close()                        # a batch of 5: multi-launch sort over the tables
    srs = khip.Srs.create(khip.VESTA, 512)
    srs.msm(rs(512)); srs.close()                               # plain basis: per-window buckets, segment reduction
    n = 1 << 13
    srs = khip.Srs.create(khip.VESTA, n)
    a_dev = khip.DevBuf(n * 32); b_dev = khip.DevBuf(n * 32); sp = khip.Sponge(khip.Sponge.FQ, khip.VESTA)
    a_dev.upload(rs(n)); b_dev.upload(rs(n)); sp.absorb_fr(rs(2))
    khip.ipa_open(srs, a_dev, b_dev, n, rs(1)[0], rs(1)[0], sp, rs(2 * 13 + 2))
    khip.sync()
    sp.free(); a_dev.free(); b_dev.free(); srs.close()
    print("msm_launch_list: done")


def launches(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    name = lambda r: re.sub(r"\(.*$", "", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("kh::", ""))
    dims = lambda r, k: "x".join(r["%s_Size_%s" % (k, d)] for d in "XYZ")
    return [(name(r), dims(r, "Grid"), dims(r, "Workgroup"), r["LDS_Block_Size"]) for r in rows]


def compare(pa, pb):
    a, b = launches(pa), launches(pb)
    fmt = lambda t: "%-44s grid %-16s wg %-10s lds %6s" % t if t else ""
    differ = 0
    for i in range(max(len(a), len(b))):
        x, y = a[i] if i < len(a) else None, b[i] if i < len(b) else None
        differ += x != y
        print("%5d  %s | %s" % (i, fmt(x), "same" if x == y else "DIFFERENT: " + fmt(y)))
    print("parent %d launches, change %d launches, %d differ: %s" % (len(a), len(b), differ, "the same list" if not differ else "NOT the same list"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(run() if sys.argv[1] == "run" else compare(sys.argv[2], sys.argv[3]))
