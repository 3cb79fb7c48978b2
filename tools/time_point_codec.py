#!/usr/bin/env python3
"""Compressed points on the device (csrc/point_codec.hip) against the routes a caller had before, on one MI355X.

  static part (no GPU; hipcc cross-compiles): registers / scratch / occupancy of the two kernels (-Rpass-analysis=kernel-resource-usage).
  timed part, written down before the first run.  Two routes ALTERNATE in one process, 2 warm-up rounds and then `reps` (9) measured ones; every figure is
  the wall time of the route with a closing kh_sync, median [min .. max].  Phase timers off.  Inputs are built outside the timed region, handles and
  proofs are freed outside it.  No figure here is a pass / fail threshold: what comes out is reported.
    route A, the SRS of 2^16 points (Vesta):
      new   kh_srs_create_compressed: 2^16 records of 33 bytes in host memory -> a handle with its window tables;
      old   kh_srs_create from affine points in host memory.  The library has no host decoder (and gets none), so the old route's decode -- one
            square root per point on the caller's CPU -- is NOT timed: the affine points are the oracle's (cref.srs_generate), made beforehand.  The
            old figure is therefore a lower bound of the old route, in its favour: new - old is what the decode costs on the device.
      beside them, the decode kernel alone: kh_points_decompress_dev over the same 2^16 resident records (the anchor: k_field_sqrt at 2^16 random
      squares, 479 us, profiles/value_steps_dev.txt), and kh_points_compress_dev over the 2^16 points.
    route B, proof intake, 1 and 8 proofs of the fixture bench_vesta_2_16 (proved here by kh_prove_full, then put into the serialised form):
      new   kh_proofs_from_wire: the records of all the proofs through one launch, scalars converted on the host;
      old   a host decode of the same bytes, then kh_proof_from_sections per proof.  The only host decoder in the tree is the test oracle's
            (oracle.pasta.Curve.decompress, Python integers): it is what "old" times, and it is no fast host.  So a third line, "old, decode not
            timed", gives kh_proof_from_sections from ready affine sections: the bound no host decoder can beat.  The one-proof intake is a single wave whose time is its longest lane's root: it is not expected to beat a fast host.
  The clock state (rocm-smi --showclocks, read only) is recorded before and after the timed part.

Usage: tools/time_point_codec.py [reps] [--static] [--out FILE]      (FILE: profiles/point_codec.txt unless given)"""
import os
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

CSRC = os.path.join(ROOT, "proof_systems_amd", "csrc")


def static_part():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-o", os.devnull, os.path.join(CSRC, "point_codec.hip")], stderr=subprocess.PIPE, text=True, check=True)
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
                assert res["ScratchSize"] == 0, "the codec kernels must not use per-lane scratch memory"


def alternate(khip, variants, reps):
    """variants: {name: (fn, cleanup)} -> {name: (median, min, max)} in ms of fn + kh_sync, the variants taking turns; cleanup(result) is not timed"""
    runs = {name: [] for name in variants}
    for rep in range(2 + reps):
        for name, (fn, cleanup) in variants.items():
            t0 = time.perf_counter()
            made = fn()
            khip.sync()
            t1 = time.perf_counter()
            cleanup(made)
            if rep >= 2:
                runs[name].append((t1 - t0) * 1e3)
    return {name: (statistics.median(r), min(r), max(r)) for name, r in runs.items()}


def fmt(t):
    return f"{t[0]:8.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"


def route_a(K, reps):
    from oracle import cref
    cid, n = K.VESTA, 1 << 16
    g = cref.srs_generate(cid, 0, n, threads=8)
    rec = np.ascontiguousarray(cref.compress(cid, g))
    close = lambda s: s.close()
    r = alternate(K, {"new": (lambda: K.Srs.from_compressed(cid, rec), close), "old": (lambda: K.Srs(cid, g), close)}, reps)
    check = K.Srs.from_compressed(cid, rec)
    assert np.array_equal(check.get_g(), g)
    check.close()
    print(f"## route A: the SRS of 2^16 points (Vesta) from host memory, wall time with a closing kh_sync, median [min .. max] of {reps}")
    print(f"  new  kh_srs_create_compressed (33-byte records)            {fmt(r['new'])}")
    print(f"  old  kh_srs_create (affine points; the decode NOT timed)   {fmt(r['old'])}")
    print(f"  new - old (medians) = {r['new'][0] - r['old'][0]:.3f} ms: the upload is {n * 31 / 1024:.0f} KiB smaller, the decode is on the device")
    drec, dxy, dinf, dst, dout = K.DevBuf(n * 33).upload(rec), K.DevBuf(n * 64), K.DevBuf(n), K.DevBuf(n), K.DevBuf(n * 33)
    none = lambda _r: None
    k = alternate(K, {"decompress": (lambda: K.points_decompress_dev(cid, drec, n, dxy, dinf, dst), none),
                      "compress": (lambda: K.points_compress_dev(cid, dxy, None, n, dout), none)}, reps)
    assert np.array_equal(dxy.download((n, 8)), g) and np.array_equal(dout.download((n, 33), np.uint8), rec)
    print(f"  kh_points_decompress_dev, 2^16 resident records            {fmt(k['decompress'])}")
    print(f"  kh_points_compress_dev, 2^16 resident points               {fmt(k['compress'])}")
    for b in (drec, dxy, dinf, dst, dout):
        b.free()


def route_b(K, reps):
    from oracle import cref, pasta as P, views as V
    from test_gpu_index_create import fixture_case
    from test_gpu_point_codec import to_wire
    rec, _want, C_, ix, wit, prev = fixture_case(K, "bench_vesta_2_16")
    F, nx = ix.F, ix.native
    rnd = F.limbs_many(F.rand_many(V.RefRng(P.StdRng(bytes.fromhex(rec["seed_hex"]))), nx.randomness_count(True)))
    sections = nx.prove(witness=wit, randomness=rnd, prev=prev)[0]
    wire = to_wire(C_.cid, F, sections)
    points = sum(len(v[1]) for v in sections.values() if isinstance(v, tuple)) - len(sections["public_comm"][1])
    R = 1 << 256

    def host_decode(w):
        out = {}
        for name, v in w.items():
            b = bytes(v)
            if name in ("public_comm", "challenges"):
                continue
            if isinstance(sections[name], tuple):
                pts = [C_.decompress(b[i:i + 33]) for i in range(0, len(b), 33)]
                xy = np.frombuffer(b"".join((0 if pt is None else pt[k] * R % C_.base.p).to_bytes(32, "little") for pt in pts for k in (0, 1)), dtype=np.uint64).reshape(-1, 8)
                out[name] = (xy, np.array([pt is None for pt in pts], dtype=np.uint8))
            else:
                out[name] = F.limbs_many([int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)])
        return out

    free = lambda made: [p.free() for p in made]
    print(f"## route B: proof intake, bench_vesta_2_16 ({points} points a proof), wall time with a closing kh_sync, median [min .. max] of {reps}")
    for k in (1, 8):
        wires = [wire] * k
        ready = [host_decode(wire)] * k
        r = alternate(K, {"new": (lambda: K.proofs_from_wire(C_.cid, wires), free),
                          "old": (lambda: [K.Proof(host_decode(w)) for w in wires], free),
                          "bound": (lambda: [K.Proof(s) for s in ready], free)}, reps)
        got, = K.proofs_from_wire(C_.cid, [wire])
        ref = K.Proof(host_decode(wire))
        a, b = got.sections(), ref.sections()
        assert all(np.array_equal(a[s][0], b[s][0]) and np.array_equal(a[s][1], b[s][1]) if isinstance(a[s], tuple) else np.array_equal(a[s], b[s]) for s in a)
        got.free(); ref.free()
        print(f"  {k} proof{'s' if k > 1 else ' '}: new  kh_proofs_from_wire                                  {fmt(r['new'])}")
        print(f"            old  oracle (Python) decode + kh_proof_from_sections       {fmt(r['old'])}")
        print(f"            old, decode not timed: kh_proof_from_sections alone        {fmt(r['bound'])}")
    ix.free()


def timed_part(reps):
    from proof_systems_amd import khip as K
    K.init(0, timers=False)
    print(f"## timed part: one MI355X (gfx950), {time.strftime('%Y-%m-%d')}")
    TL.clocks("before")
    route_a(K, reps)
    route_b(K, reps)
    TL.clocks("after")


if __name__ == "__main__":
    reps = next((int(a) for a in sys.argv[1:] if a.isdigit()), 9)
    assert reps >= 5
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "point_codec.txt")
    sys.stdout = Tee(out)
    static_part()
    if "--static" not in sys.argv:
        timed_part(reps)
