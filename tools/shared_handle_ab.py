#!/usr/bin/env python3
"""What sharing one SRS handle and one index between prover threads costs or gains: tools/prover_concurrent.py <log2_n> 1 2 4 --native in three
configurations, alternated, each run in a process of its own:
  (a) another build of the library (--parent-lib, e.g. the parent commit's: openings on one handle queue), --shared
  (b) this build, --shared            (one handle and index for all threads)
  (c) this build, a handle and an index per thread (the tool's default)
Prints every run's proofs/s, then median and min-max per configuration and thread count, and the device memory in use after warm-up for (b) and (c).
Usage: python tools/shared_handle_ab.py [--parent-lib PATH] [--reps 5] [--logn 16]"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--logn", type=int, default=16)
args = ap.parse_args()
COUNTS = ["1", "2", "4"]
configs = {"b": ({}, ["--shared", "--mem"]), "c": ({}, ["--mem"])}
if args.parent_lib:
    configs = {"a": ({"KH_LIB": os.path.abspath(args.parent_lib)}, ["--shared"]), **configs}
rate = {c: {t: [] for t in COUNTS} for c in configs}
mem = {c: {t: [] for t in COUNTS} for c in configs}
for rep in range(args.reps):
    for c, (env, extra) in configs.items():
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prover_concurrent.py"), str(args.logn)] + COUNTS + ["--native"] + extra,
                           env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        if r.returncode != 0:
            sys.exit(f"config ({c}) run {rep + 1} ended with {r.returncode}:\n{r.stderr.decode()[-2000:]}")
        out = r.stdout.decode()
        for t, v in re.findall(r"^(\d+) prover\(s\) in flight: ([0-9.]+) proofs/s", out, re.M):
            rate[c][t].append(float(v))
        for t, v in re.findall(r"^(\d+) prover\(s\), \w+ index / handle: (\d+) MiB", out, re.M):
            mem[c][t].append(int(v))
        print(f"run {rep + 1} ({c}): " + "  ".join(f"{t} thread(s) {rate[c][t][-1]:.1f}" for t in COUNTS) + " proofs/s", flush=True)
print()
for c in configs:
    for t in COUNTS:
        v = rate[c][t]
        line = f"({c}) {t} thread(s): median {statistics.median(v):.1f} proofs/s, range {min(v):.1f}-{max(v):.1f} over {len(v)} runs"
        if mem[c][t]:
            line += f"; device memory in use after warm-up {min(mem[c][t])}-{max(mem[c][t])} MiB"
        print(line)
