#!/bin/bash
# One GPU call: parity tests, rocprofv3 trace + PMC passes, HBM traffic table, then the bench line
# (which reads the traffic table).  Usage (repo root, on the GPU box):  bash tools/gpu_round.sh <tag>
set -u
TAG=${1:-r01}
K=${2:-}
mkdir -p gpurun_out
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread \
    ${K:+-k "$K"} > gpurun_out/pytest_gpu_$TAG.log 2>&1 || { echo "pytest failed $?"; tail -30 gpurun_out/pytest_gpu_$TAG.log; exit 1; }
tail -3 gpurun_out/pytest_gpu_$TAG.log
bash tools/gpu_profile.sh $TAG || exit 1
python3 tools/pmc_traffic.py gpurun_out/prof_$TAG gpurun_out/prof_$TAG/traffic.json profiles/traffic.json || exit 1
# the full bench line (bench.py --full: with the CPU baseline and the stream step) and its summary,
# written by the bench step of tools/gpu_job.sh into its <tag> folder
bash tools/gpu_job.sh $TAG bench || exit 1
