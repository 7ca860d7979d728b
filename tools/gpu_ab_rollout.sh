# A/B: the best-of-k rollout on the batch-MFMA kernel (default) vs the
# four-wave family (SGG_LSTM_NO_MFMA=1); bench headline, rollout launch time
set -o pipefail
OUT=${OUT:-bench_out}   # where the results go (relative to the repository root)
mkdir -p $OUT
for v in 0 1 0 1; do
  if [ $v = 1 ]; then export SGG_LSTM_NO_MFMA=1; else unset SGG_LSTM_NO_MFMA; fi
  SGG_BENCH_TABLE=$OUT/ro_$v.txt timeout -k 10 300 python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline --no-scaling-reference --no-real-data --no-legs > $OUT/ro_$v.json 2> $OUT/ro_$v.err || { echo BENCH_FAIL; tail -5 $OUT/ro_$v.err; exit 1; }
  python - $OUT/ro_$v.json $v <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("no_mfma", sys.argv[2], "value %.1f ms %.4f" % (d["value"], d["ms_per_step"]), [(r["kernel"][5:40], r["shape"], round(r["avg_us"], 1)) for r in d["launch_table"] if "25600" in str(r["shape"])])
PY
done
