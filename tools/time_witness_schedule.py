#!/usr/bin/env python3
"""Witness schedules (csrc/witness_schedule.cpp; k_cell_moves in csrc/wiring.hip) against the direct calls they replace, on one MI355X.

  static part (no GPU; hipcc cross-compiles): registers / scratch / occupancy of the kernels of wiring.hip (-Rpass-analysis=kernel-resource-usage).
  timed part: the curve chain and the limb chain of tests/test_gpu_wiring_dev.py (as tests/test_gpu_witness_schedule.py writes them as steps), and
    the gather + scatter pair of profiles/wiring_dev.txt at n = 2^12 and 2^16 cells, both fields, each KH_CELL_* format.  Per workload the direct
    calls and one kh_witness_schedule_run ALTERNATE in one process, 2 warm-up rounds and then `reps` (9) measured ones, each variant timed as
      (a) the host time until the last call has returned,
      (b) the wall time including a closing kh_sync,
    median [min .. max]; (c) is the number of launcher invocations -- the direct calls (each with a table copy queued in front of it where it takes
    rows[] or cells) against the schedule's launch_groups.  The time of kh_witness_schedule_create is one call's, taken once.  For the pair, `hop
    before` is what wiring_dev.txt defines: kh_dev_download of the n elements + kh_dev_upload of n values of the format + kh_sync (wall, the host
    conversion not counted).  The phase timers are off (kh_set_phase_timers(0), as under kh_prove): an event between two kernels costs the stream
    6-10 us.  Scratch of the direct variants is allocated outside the timed region.
  The conditions, written down before the first run and reported per line as MET or MISSED:
    1. on both chains, (a) and (b) of the schedule run are below the direct calls' in the same process;
    2. the gather + scatter pair as a schedule takes less wall time (b) than the hop before, at 2^12 and at 2^16 -- the condition the wiring work
       missed on all 20 lines.
  The clock state (rocm-smi --showclocks, read only) is recorded before and after the timed part.

Usage: tools/time_witness_schedule.py [reps] [--static]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time_limb_gadgets as TL  # noqa: E402  (static_part, clocks: the same report for another source file)
from time_wiring import FORMAT_NAMES, ROWS, SIZES, values  # noqa: E402

TL.SRC = os.path.join(ROOT, "proof_systems_amd", "csrc", "wiring.hip")


def alternate(khip, variants, reps):
    """variants: {name: fn}.  -> {name: ((a) median, min, max, (b) median, min, max)} in ms, the variants taking turns"""
    runs = {name: [] for name in variants}
    for rep in range(2 + reps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            khip.sync()
            t2 = time.perf_counter()
            if rep >= 2:
                runs[name].append(((t1 - t0) * 1e3, (t2 - t0) * 1e3))
    out = {}
    for name, r in runs.items():
        a, b = sorted(x[0] for x in r), sorted(x[1] for x in r)
        out[name] = (statistics.median(a), a[0], a[-1], statistics.median(b), b[0], b[-1])
    return out


def fmt(t):
    return f"(a) {t[0]:6.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]  (b) {t[3]:6.3f} ms [{t[4]:.3f} .. {t[5]:.3f}]"


def created(khip, *args, **kw):
    t0 = time.perf_counter()
    s = khip.WitnessSchedule.create(*args, **kw)
    return s, (time.perf_counter() - t0) * 1e3


def chains(khip, reps, verdicts):
    import test_gpu_witness_schedule as T
    from oracle import circuit as CC, pasta as P
    from test_gpu_limb_gadgets_dev import mont, plain
    from test_gpu_wiring_dev import FIELD, INT256, LIMB88, U64, limb_chain
    fid = khip.FP
    # the curve chain: 11 direct calls (4 of them gathers with a cell table) against 11 launch groups
    n = 1 << 8
    _e, endo = T.endo_of(khip, fid)
    sched, create_ms = created(khip, fid, n, T.curve_steps(khip, endo), arena_bytes=T.CURVE_ARENA, n_bufs=len(T.CURVE_BUFS))
    bufs = T.curve_buffers(khip, T.curve_inputs(5100))
    wit_d, wit_s, flags = khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(4).zero()
    scratch = (khip.DevBuf(32), khip.DevBuf(16), khip.DevBuf(128), khip.DevBuf(128))
    r = alternate(khip, {"direct": lambda: T.curve_direct(khip, bufs, wit_d, n, flags, endo, scratch=scratch),
                         "schedule": lambda: sched.run(bufs, wit_s, flags=flags)}, reps)
    assert np.array_equal(wit_d.download((15, n, 4)), wit_s.download((15, n, 4))) and int(flags.download((1,), dtype=np.uint32)[0]) == 0
    report("curve chain (157 rows in 2^8)", r, 11, 4, sched, create_ms, verdicts)
    sched.free()
    for b in (wit_d, wit_s, flags, *bufs, *scratch):
        b.free()
    # the limb chain: 13 direct calls (6 gathers) against 13 launch groups
    n = 1 << 13
    _gates, _rows, inp = limb_chain()
    sched, create_ms = created(khip, fid, n, T.limb_steps(khip), arena_bytes=T.LIMB_ARENA, n_bufs=2)
    w, in2 = khip.DevBuf(16).upload(plain([inp["w"]], 1)), khip.DevBuf(32).upload(plain([inp["in2"]], 4))
    wit_d, wit_s, flags = khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(32 * 15 * n).zero(), khip.DevBuf(4).zero()
    in1, word, limbs, ops = khip.DevBuf(32), khip.DevBuf(8), khip.DevBuf(48), khip.DevBuf(64)
    t = khip.DevBuf(64)
    add, sub = mont(P.Fp, CC.generic_spec(P.Fp.p, "Add")), mont(P.Fp, CC.generic_spec(P.Fp.p, "Add", right=-1, output=-2))

    def direct():
        khip.rot64_witness_dev(fid, w, 7, 1, wit_d, n, n, row0=0)
        khip.witness_gather_dev(fid, wit_d, n, n, [(0, 1)], INT256, in1)
        khip.xor_witness_dev(fid, in1, in2, 64, 1, wit_d, n, n, row0=3, flags=flags, bit=0)
        khip.witness_gather_dev(fid, wit_d, n, n, [(3, 2)], U64, word, flags=flags, bit=1)
        khip.rot64_witness_dev(fid, word, 63, 1, wit_d, n, n, row0=8)
        khip.witness_gather_dev(fid, wit_d, n, n, [(8, 1), (3, 2), (0, 2)], LIMB88, limbs, flags=flags, bit=2)
        khip.range_check_witness_dev(fid, limbs, 1, wit_d, n, n, row0=11, flags=flags, bit=3)
        khip.witness_gather_dev(fid, wit_d, n, n, [(8, 1), (0, 0)], INT256, ops)
        # (build_and of tests/test_gpu_wiring_dev.py, its scratch block allocated outside the timed region)
        khip.xor_witness_dev(fid, ops.view(0), ops.view(32), 64, 1, wit_d, n, n, row0=15, row_stride=6, flags=flags, bit=4)
        khip.witness_gather_dev(fid, wit_d, n, n, [(15, 0), (15, 1)], FIELD, t)
        khip.generic_witness_dev(fid, add, 0, t.view(0), t.view(32), 1, wit_d, n, n, row0=20, row_stride=6)
        khip.witness_gather_dev(fid, wit_d, n, n, [(20, 2), (15, 2)], FIELD, t)
        khip.generic_witness_dev(fid, sub, 1, t.view(0), t.view(32), 1, wit_d, n, n, row0=20, row_stride=6)

    r = alternate(khip, {"direct": direct, "schedule": lambda: sched.run([w, in2], wit_s, flags=flags)}, reps)
    assert np.array_equal(wit_d.download((15, n, 4)), wit_s.download((15, n, 4))) and int(flags.download((1,), dtype=np.uint32)[0]) == 0
    report("limb chain (21 rows in 2^13)", r, 13, 6, sched, create_ms, verdicts)
    sched.free()
    for b in (wit_d, wit_s, flags, w, in2, in1, word, limbs, ops, t):
        b.free()


def report(name, r, calls, tables, sched, create_ms, verdicts):
    info = sched.info()
    ok = r["schedule"][0] < r["direct"][0] and r["schedule"][3] < r["direct"][3]
    verdicts.append((f"condition 1, {name}", ok))
    print(f"  {name}: direct {fmt(r['direct'])}  (c) {calls} calls, {tables} with a table copy in front;  schedule run {fmt(r['schedule'])}  "
          f"(c) {info['launch_groups']} launch groups;  create {create_ms:.3f} ms, {info['resident_bytes']} B resident, {info['run_bytes']} B per run: "
          + ("MET" if ok else "MISSED") + f" ((a) {r['direct'][0] / r['schedule'][0]:.2f} x, (b) {r['direct'][3] / r['schedule'][3]:.2f} x)", flush=True)


def pairs(khip, reps, verdicts):
    rng = np.random.default_rng(17)
    wit = khip.DevBuf(32 * 15 * ROWS).upload(values(rng, 0, 15 * ROWS, 4))
    for n in SIZES:
        where = rng.choice(15 * ROWS, size=n, replace=False)
        cells = np.stack([where % ROWS, where // ROWS], axis=1).astype(np.uint32)
        elems = khip.DevBuf(32 * n).upload(values(rng, 0, n, 4))
        for fid, fname in ((khip.FP, "Fp"), (khip.FQ, "Fq")):
            for f, name in enumerate(FORMAT_NAMES):
                words = khip.CELL_WORDS[f]
                host = values(rng, f, n, words)
                dense = khip.DevBuf(8 * words * n).upload(host)
                flags = khip.DevBuf(4).zero()
                khip.witness_scatter_dev(fid, dense, f, cells, wit, ROWS, ROWS)          # the cells fit the format from here on
                sched, create_ms = created(khip, fid, ROWS, [dict(op=khip.STEP_GATHER, cells=cells, format=f, out=[(khip.REF_ARENA, 0)], flag_bit=0),
                                                              dict(op=khip.STEP_SCATTER, cells=cells, format=f, flag_bit=1, **{"in": [(khip.REF_ARENA, 0)]})],
                                           arena_bytes=8 * words * n, n_bufs=0)

                def hop_before():
                    elems.download((n, 4))
                    dense.upload(host)

                def direct():
                    khip.witness_gather_dev(fid, wit, ROWS, ROWS, cells, f, dense, flags=flags, bit=0)
                    khip.witness_scatter_dev(fid, dense, f, cells, wit, ROWS, ROWS, flags=flags, bit=1)

                r = alternate(khip, {"hop": hop_before, "direct": direct, "schedule": lambda: sched.run([], wit, flags=flags)}, reps)
                ok = r["schedule"][3] < r["hop"][3]
                label = f"{fname} {name:<6} n = 2^{n.bit_length() - 1}"
                verdicts.append((f"condition 2, {label}", ok))
                print(f"  {label}: hop before (b) {r['hop'][3]:6.3f} ms [{r['hop'][4]:.3f} .. {r['hop'][5]:.3f}];  direct gather + scatter {fmt(r['direct'])}  "
                      f"(c) 2 calls, 2 table copies;  schedule run {fmt(r['schedule'])}  (c) {sched.info()['launch_groups']} launch groups;  create {create_ms:.3f} ms: "
                      + (f"MET ({r['hop'][3] / r['schedule'][3]:.1f} x faster than the hop before)" if ok else f"MISSED ({r['hop'][3] / r['schedule'][3]:.2f} x)"), flush=True)
                assert int(flags.download((1,), dtype=np.uint32)[0]) == 0
                sched.free(); dense.free(); flags.free()
        elems.free()
    wit.free()


def timed_part(reps):
    from proof_systems_amd import khip
    khip.init(0, timers=False)
    TL.clocks("before")
    print(f"## (a) host time until the last call has returned, (b) wall time with a closing kh_sync, median [min .. max] of {reps} after 2 warm-up rounds,")
    print("## the variants alternating in one process; (c) launcher invocations.  Phase timers off.")
    verdicts = []
    chains(khip, reps, verdicts)
    pairs(khip, reps, verdicts)
    TL.clocks("after")
    for cond, text in (("condition 1", "on both chains, (a) and (b) of the schedule run are below the direct calls'"),
                       ("condition 2", "the gather + scatter pair as a schedule takes less wall time than the hop before, at 2^12 and 2^16")):
        mine = [(w, ok) for w, ok in verdicts if w.startswith(cond)]
        missed = [w.split(", ", 1)[1] for w, ok in mine if not ok]
        print(f"## {cond} ({text}): " + (f"MET on all {len(mine)} lines" if not missed else f"MISSED on {len(missed)} of {len(mine)} lines: " + "; ".join(missed)))


if __name__ == "__main__":
    reps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 9)
    assert reps >= 5
    TL.static_part()
    if "--static" not in sys.argv:
        timed_part(reps)
