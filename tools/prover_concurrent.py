#!/usr/bin/env python3
"""Proof throughput with several provers in flight on one GPU: T host threads, each producing proofs of the benchmark circuit back to back.  One
proof is mostly latency chains (opening rounds, transcript on the host), so independent proofs overlap.  By default every thread has its own index /
SRS handle; --shared: ONE index and ONE SRS handle serve all threads (their openings run side by side on the handle's KH_IPA_OPENINGS workspaces).
--mem: also print the device memory in use (hipMemGetInfo) once every thread has warmed up, per thread count.
Usage: tools/prover_concurrent.py [log2_n] [threads ...] [--native] [--shared] [--mem]"""
import os, sys, threading, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proof_systems_amd.khip as khip
from proof_systems_amd import prover
khip.init(0)
logn = int(sys.argv[1]) if len(sys.argv) > 1 else 16
NATIVE = "--native" in sys.argv                        # kh_prove (C++ host loop, the library draws the randomness: no Python between the steps, no GIL)
SHARED = "--shared" in sys.argv                        # one index / SRS handle for all threads
MEM = "--mem" in sys.argv
counts = [int(x) for x in sys.argv[2:] if not x.startswith("--")] or [1, 2, 4]
tmax = max(counts)
ixs = [prover.bench_circuit_index(khip.VESTA, logn) for _ in range(1 if SHARED else tmax)]
F = prover.Fld(ixs[0].fid)
wit = np.tile(F.limbs(1), (15, (1 << logn) - 10, 1))
for ix in ixs:
    prover.create_proof(ix, wit, np.random.default_rng(1), check=False)
PROOFS = 6
nxs = [prover.native_index(ix) for ix in ixs] if NATIVE else []
if SHARED:
    ixs, nxs = ixs * tmax, nxs * tmax


def device_memory_in_use():
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return total.value - free.value


for T in counts:
    bar = threading.Barrier(T + 1)
    mem_line = None

    def work(t):
        rng = np.random.default_rng(100 + t)
        try:
            if NATIVE:                                  # this thread's own library context: warm it (workspaces, graphs) outside the timed region
                nxs[t].prove(witness=wit, randomness=None, flags=0)
            if MEM:
                bar.wait()               # every thread is warm: the main thread reads the device memory in use, then all go on to the timed region
            bar.wait()
            for _ in range(PROOFS):
                if NATIVE:
                    nxs[t].prove(witness=wit, randomness=None, flags=0)
                else:
                    prover.create_proof(ixs[t], wit, rng, check=False)
            bar.wait()
        except BaseException:
            bar.abort()                  # a failing prover must not leave the others (and the GPU box) waiting at the barrier
            raise
    th = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(T)]
    for t in th:
        t.start()
    if MEM:
        bar.wait()
        mem_line = f"{T} prover(s), {'shared' if SHARED else 'own'} index / handle: {device_memory_in_use() / 2**20:.0f} MiB of device memory in use after warm-up"
    bar.wait(); t0 = time.perf_counter(); bar.wait(); dt = time.perf_counter() - t0
    for t in th:
        t.join()
    if mem_line:
        print(mem_line)
    print(f"{T} prover(s) in flight: {T * PROOFS / dt:.1f} proofs/s = {T * PROOFS * (1 << logn) / dt / 1e6:.2f} M constraints/s  ({1e3 * dt / PROOFS:.1f} ms per proof per thread)")
