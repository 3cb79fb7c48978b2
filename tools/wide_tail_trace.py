#!/usr/bin/env python3
"""The wide MSM's tail chain and sort chain from two rocprofv3 kernel-trace databases of tools/msm_loop.py: one with two MSMs in flight
(`wide pipe 40 20 2`) and one with a single MSM in flight (`wide sync 12`).  Per kernel: time per MSM pipelined (steady state: the
launches between the fifth and the third-last accumulation) and alone, and how far the first stretches the second; then the sums of
the two chains and tools/timeline.py's account of the pipelined trace (step time, share of time with no accumulation running).
Usage: tools/wide_tail_trace.py pipelined.db alone.db"""
import os
import sqlite3
import subprocess
import sys

TAIL = ("k_wide_a1", "k_wide_l2", "k_wide_a2", "k_marginals_q", "k_marginal_fin_q")
ACC = ("k_acc_wide29",)


def short(name):
    return name.split("(")[0].replace("void ", "").replace("kh::", "").split("<")[0]


def launches(path):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    namecol = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = [(short(n), s, e) for n, s, e in db.execute(f"select {namecol}, start, end from kernels order by start")]
    acc = [(s, e) for n, s, e in rows if n in ACC]
    lo, hi = (acc[4][0], acc[-3][1]) if len(acc) > 8 else (acc[1][0], acc[-1][1])
    return [r for r in rows if lo <= r[1] and r[2] <= hi], len([a for a in acc if lo <= a[0] and a[1] <= hi])


def table(rows, nacc):
    """name -> total ns per MSM (a kernel launched several times per MSM, such as the scans, counts with all its launches)"""
    out = {}
    for n, s, e in rows:
        out[n] = out.get(n, 0.0) + (e - s) / nacc
    return out


def main():
    pipe, nacc_p = launches(sys.argv[1])
    alone, nacc_a = launches(sys.argv[2])
    tp, ta = table(pipe, nacc_p), table(alone, nacc_a)
    order = []
    for n, s, e in alone:                                   # launch order of one MSM
        if n not in order:
            order.append(n)
    print(f"{'kernel':28s} {'pipelined us':>13s} {'alone us':>10s} {'stretch':>8s}   chain")
    sums = {"tail": [0.0, 0.0], "sort": [0.0, 0.0]}
    for key in order:
        base = key
        chain = "acc" if base in ACC or base in ("k_acc_wide_rest", "k_bucket_sum_wide") else "tail" if base in TAIL else "sort"
        p, a = tp.get(key, float("nan")), ta[key]
        if chain in sums:
            sums[chain][0] += p; sums[chain][1] += a
        print(f"{key:28s} {p / 1e3:13.1f} {a / 1e3:10.1f} {p / a:8.2f}   {chain}")
    for c, (p, a) in sums.items():
        print(f"{c + ' chain, sum':28s} {p / 1e3:13.1f} {a / 1e3:10.1f}")
    print()
    sys.stdout.flush()
    subprocess.check_call([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "timeline.py"), sys.argv[1]])


if __name__ == "__main__":
    main()
