#!/usr/bin/env bash
# GPU box: the full bench line plus the raw amd-smi clock JSON its clock sampler parses.
#   OUT=<directory> bash scripts/bench_probe.sh      (default: bench_out/)
set -u
O=${OUT:-bench_out}
mkdir -p "$O"
(amd-smi metric -g 0 --clock --json > $O/amdsmi_clock.json 2>&1 || true)
timeout -k 10 300 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
rc=$?; tail -c 3000 $O/bench_default.json; tail -5 $O/bench_default.err; exit $rc
