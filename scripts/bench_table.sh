#!/usr/bin/env bash
# GPU box: the full bench line (every leg, with CPU baseline) + batch sweep for DESIGN.md §5.3
#   OUT=<directory> bash scripts/bench_table.sh      (default: bench_out/)
set -u
O=${OUT:-bench_out}
mkdir -p "$O"
timeout -k 10 300 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err || exit 3
for b in ${BATCHES:-1 64 256 1024 2048 4096}; do
  timeout -k 10 200 python bench.py --batch $b > $O/bt_$b.json 2>/dev/null || exit 3
  python3 -c "
import json
d=[json.loads(l) for l in open('$O/bt_$b.json') if l.startswith('{')][-1]
print('B=$b %.0f/s step %.3f ms br %.3f ms ks %.3f ok=%s' % (d['value'], d['ms_per_step'], d['roofline']['kernel_ms'], d['roofline']['keyswitch_ms'], d['truth_table_ok']))" | tee -a $O/bt_summary.txt
done
