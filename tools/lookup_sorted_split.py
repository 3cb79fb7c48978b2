#!/usr/bin/env python3
"""Where the `sorted` step of a lookup proof spends its time, on the circuit of tools/lookup_prover_time.py (Lookup gates into two user tables) at
2^log2_n rows: the host route (download of the looked-up values and the combined table, kh_lookup_sorted on one host thread, padding, upload of the
columns) piece by piece, against kh_lookup_sorted_dev over the same device buffers.  Best of `reps` each.  Usage: tools/lookup_sorted_split.py [log2_n] [reps]"""
import os, sys, time, random
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proof_systems_amd.khip as khip
from proof_systems_amd import prover, lookup as LK
khip.init(0)
logn = int(sys.argv[1]) if len(sys.argv) > 1 else 16
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = 1 << logn
rnd = random.Random(21)
F = prover.Fld(khip.FP)
tsz = min(n // 4, 4096)
tables = [{"id": 0, "data": [list(range(tsz)), [0] + [rnd.randrange(F.p) for _ in range(tsz - 1)]]},
          {"id": 3, "data": [list(range(tsz // 2)), [rnd.randrange(F.p) for _ in range(tsz // 2)]]}]
ngen = 30; nlook = n - 3 - ngen - 8
gates = ["Generic"] * ngen + ["Lookup"] * nlook + ["Zero"] * (n - 3 - ngen - nlook)
rows = ngen + nlook
wit = [[0] * n for _ in range(15)]
for r in range(ngen):
    wit[0][r] = 7
for r in range(ngen, rows):
    t = tables[rnd.randrange(2)]
    wit[0][r] = t["id"]
    for i in range(3):
        e = rnd.randrange(len(t["data"][0]))
        wit[2 * i + 1][r], wit[2 * i + 2][r] = t["data"][0][e], t["data"][1][e]
LI = LK.LookupIndex(khip.FP, gates, tables, logn)
mpr, ns, zk, L = LI.max_per_row, LI.max_per_row + 1, LI.zk_rows, n - LI.zk_rows - 1
ev = khip.DevBuf(15 * n * 32).upload(np.stack([F.limbs_many(c) for c in wit]))
jc = 0x9e3779b97f4a7c15f39cc0605cedc834 % F.p
d_table = LI.joint_table_dev(jc, None)
d_vals = LK.lookup_values_dev(LI, [ev.view(i * n * 32) for i in range(15)], jc)
d_out = khip.DevBuf(ns * n * 32).zero()
khip.sync()


def best(f):
    ts = []
    for _ in range(reps):
        khip.sync(); t0 = time.perf_counter(); r = f(); khip.sync(); ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), r


t_down, (vals, table) = best(lambda: (d_vals.download((mpr, n, 4)), d_table.download((n, 4))))
t_join, srt = best(lambda: khip.lookup_sorted(table, L, vals, mpr))
full = np.zeros((ns, n, 4), dtype=np.uint64)
def pad():
    full[:, :n - zk] = srt
t_pad, _ = best(pad)
t_up, _ = best(lambda: d_out.upload(full))
t_dev, _ = best(lambda: khip.lookup_sorted_dev(d_table, L, d_vals, n, mpr, d_out, n))
assert np.array_equal(d_out.download((ns, n, 4))[:, :n - zk], srt)
print(f"2^{logn} rows, {mpr} lookups per row, {ns} sorted columns; best of {reps}, ms")
print(f"host route: download {(mpr + 1) * n * 32 / 1e6:.1f} MB {t_down:.3f}  kh_lookup_sorted {t_join:.3f}  pad {t_pad:.3f}  upload {ns * n * 32 / 1e6:.1f} MB {t_up:.3f}  sum {t_down + t_join + t_pad + t_up:.3f}")
print(f"device route: kh_lookup_sorted_dev (launches + the status read-back) {t_dev:.3f}")
