# BLS12-381 2^22 accumulate-occupancy A/B: bash tools/bls_ab.sh <outdir>   (reads each run's full record, <run>.detail.json)
O=${1:?usage: bash tools/bls_ab.sh <outdir>}
mkdir -p $O
for v in "base" "ZKP_G1_ACC_WAVES=3" "ZKP_G2_ACC_OCC=2" "ZKP_G1_ACC_WAVES=3 ZKP_G2_ACC_OCC=2"; do
  tag=$(echo "$v" | tr ' =' '__')
  export ZKP_BENCH_DETAIL=$O/bls_$tag.detail.json
  if [ "$v" = base ]; then env python bench.py --full --curve bls12_381 --log-n 22 --steps 12 --warmup 4 --no-marlin --no-extra-configs --no-cpu-baseline > $O/bls_$tag.json 2>/dev/null
  else env $v python bench.py --full --curve bls12_381 --log-n 22 --steps 12 --warmup 4 --no-marlin --no-extra-configs --no-cpu-baseline > $O/bls_$tag.json 2>/dev/null; fi
  python -c "
import json,sys;d=json.load(open('$ZKP_BENCH_DETAIL'));print('$v', d['value'], d['ms_per_step'], d['latency']['ms_per_proof'], d['valu_roof']['g1_accumulate'], d['valu_roof']['g2_accumulate']['frac'], d['phases_ms']['ms_msm_acc'])"
done
