#!/usr/bin/env bash
# the small-batch launches' rotation form: LDS extension (default at B <= CUs) vs TFHE_AMD_V6_RREG=1
# (the register rotation, its scalar-branch permutation form); RREG_BATCHES (default "1 256");
# OUT=<directory> for the lines (default: bench_out/)
set -u
O=${OUT:-bench_out}
mkdir -p "$O"
for rep in 1 2 3; do
for v in 0 1; do
  for b in ${RREG_BATCHES:-1 256}; do
    TFHE_AMD_V6_RREG=$v timeout -k 10 200 python bench.py --full --batch $b --steps 40 --warmup 10 --no-cpu-baseline --no-clock --no-ceiling --no-circuits --extra-batches none --strong-batch none --host-batches none --parity-samples 8 > $O/rreg_${v}_${b}_$rep.json 2>/dev/null || exit 3
    python3 -c "
import json
d=[json.loads(l) for l in open('$O/rreg_${v}_${b}_$rep.json') if l.startswith('{')][-1]
print('RREG=$v B=$b rep $rep  %8.1f /s  br %.4f ms  parity %d/%d' % (d['value'], d['roofline']['kernel_ms'], d['parity']['checked_per_rank']-d['parity']['mismatches'], d['parity']['checked_per_rank']))" | tee -a $O/rreg_ab.txt
  done
done
done
