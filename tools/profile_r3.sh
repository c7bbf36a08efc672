#!/bin/bash
# Round-3 profile batch (GPU box, repo root): kernel stats + FETCH/WRITE PMC passes (tools/profile_r.sh), request-size PMC passes,
# timeline overlap, and the bench lines that go to profiles/.   bash tools/profile_r3.sh <outdir>
set -u
R=r03
O=${1:?usage: bash tools/profile_r3.sh <outdir>}
bash tools/profile_r.sh $R > $O/profile_$R.log 2>&1
bash tools/pmc_bytes.sh $O/prof_${R}_bytes > $O/pmc_bytes_$R.log 2>&1
bash tools/trace_overlap.sh $O/prof_${R}_overlap > $O/overlap_$R.log 2>&1
python bench.py --full > $O/bench_full.json 2> $O/bench_full.err
python bench.py --steps 20 --warmup 5 --no-marlin > $O/bench_driver_flags.json 2> $O/bench_driver_flags.err
python bench.py --full --curve bls12_381 --log-n 22 --steps 12 --warmup 4 --no-marlin > $O/bls22.json 2> $O/bls22.err
python bench.py --full --workload marlin > $O/marlin.json 2> $O/marlin.err
python bench.py --full --log-n 24 --steps 6 --warmup 2 --no-cpu-baseline --no-marlin > $O/bn24.json 2> $O/bn24.err
ZKP_TABLE_BUDGET_GB=24 python bench.py --full --log-n 24 --steps 6 --warmup 2 --no-cpu-baseline --no-marlin > $O/bn24_budget24.json 2> $O/bn24_budget24.err
for f in bench_full bench_driver_flags bls22 marlin bn24 bn24_budget24; do echo $f; tail -1 $O/$f.json | cut -c1-220; done
