#!/bin/bash
# Collects the round's committed evidence on a machine with the GPU: rocprofv3 kernel stats + PMC passes for the MSM and the
# NTT workloads (tools/profile_msm.py: every PMC pass its own run, never combined with a trace), the pipelined kernel trace + timeline, the static
# opcode mixes, the A/B of the two table sets, the PCIe-inclusive rates, and finally bench.py --full's line (which then finds profiles of ITS OWN build).
# Usage: tools/collect_profiles.sh r06 OUT_DIR   (the files land in OUT_DIR/prof)
R=${1:-r06}
OUT=${2:?usage: tools/collect_profiles.sh ROUND OUT_DIR}
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
mkdir -p $OUT/prof
python tools/profile_msm.py $OUT/prof/${R}_msm20 > $OUT/prof/${R}_msm20_summary.txt 2>&1
python tools/profile_msm.py $OUT/prof/${R}_ntt --workload ntt > $OUT/prof/${R}_ntt_summary.txt 2>&1
python tools/valu_mix.py $OUT/prof/${R}_k_acc_wide29_valu_mix.json > /dev/null 2>&1
python tools/valu_mix.py $OUT/prof/${R}_k_ntt_pass_valu_mix.json --kernel ntt > /dev/null 2>&1
(cd /tmp && rocprofv3 --kernel-trace -d /tmp/pipe_$R -o t -- python $OLDPWD/tools/msm_loop.py wide pipe 40 20 2 > /dev/null 2>&1)
DB=$(find /tmp/pipe_$R -name "*.db" | head -1)
python tools/rocpd_stats.py $DB $OUT/prof/${R}_msm20_pipelined_kernel_stats.csv > /dev/null
python tools/timeline.py $DB > $OUT/prof/${R}_msm20_pipelined_timeline.txt
python tools/wide_ab.py 20 20 5 > $OUT/prof/${R}_wide_ab.txt 2>&1
python tools/pcie_inclusive.py > $OUT/prof/${R}_pcie_inclusive.txt 2>&1
python tools/bench_ntt.py > $OUT/prof/${R}_bench_ntt.txt 2>&1
(cd /tmp && rocprofv3 --kernel-trace -d /tmp/proof_$R -o t -- python $OLDPWD/tools/prover_time.py 16 --native > /dev/null 2>&1)
PDB=$(find /tmp/proof_$R -name "*.db" | head -1)
python tools/proof_timeline.py $PDB > $OUT/prof/${R}_proof_timeline.txt 2>&1
python tools/round_timeline.py $PDB > $OUT/prof/${R}_round_timeline.txt 2>&1
python tools/proof_busy.py $PDB $OUT/prof/${R}_proof_busy.json > /dev/null 2>&1
KH_IPA_TIMING=1 python tools/prover_time.py 16 --native > $OUT/prof/${R}_prover_time_ipa_timing.txt 2>&1
# bench.py last: copy the fresh PMC / mix files where it looks for them
cp $OUT/prof/${R}_proof_busy.json $OUT/prof/${R}_msm20_pmc.json $OUT/prof/${R}_ntt_pmc.json $OUT/prof/${R}_k_acc_wide29_valu_mix.json $OUT/prof/${R}_k_ntt_pass_valu_mix.json profiles/ 2>/dev/null
python bench.py --full > $OUT/prof/${R}_bench_stdout.txt 2> $OUT/prof/${R}_bench_stderr.txt
grep '^{' $OUT/prof/${R}_bench_stdout.txt | tail -1 > $OUT/prof/${R}_bench_line.json
rm -rf $OUT/prof/*_passes
ls -la $OUT/prof | head -40
