"""csrc/msm_plan.hpp on the host: every decision the MSM driver makes before its first launch is one pure function of the shape, the basis' facts, the
device's sizes and the knobs.  tests/cpp/test_msm_plan.cpp sweeps it (n, k, table kinds, CU counts, flags, the staged scatter's settings) against the
conditions the kernels of msm.hip rely on and pins five shapes to the values the driver computed before the plan existed.  Built with g++ under
AddressSanitizer and UBSan here -- host code only, no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_holds_the_kernels_conditions_over_the_sweep_and_the_pinned_shapes(tmp_path):
    exe = str(tmp_path / "test_msm_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_msm_plan.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    counts = dict(zip(run.stdout.split()[::2], map(int, run.stdout.split()[1::2])))
    assert counts["plans"] >= 19 * 9 * 5 * 3 * 3 * 5 and all(counts[p] > 0 for p in ("refused", "fused", "partitioned", "plain", "wide", "staged")), run.stdout
    # the kernels' index formulas (marginal_bucket, wide_a1_item): plans whose bucket maps were walked
    assert counts["marginal_maps"] > 0 and counts["wide_item_maps"] > 0, run.stdout
