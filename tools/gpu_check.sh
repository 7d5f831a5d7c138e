#!/bin/bash
# Run ON THE GPU BOX from the repo root: GPU test suite, then the full bench line.
#   bash tools/gpu_check.sh TAG [bench args...]   -> $OUT/{gputest,bench}_TAG.*   (OUT defaults to out/gpu_check)
TAG=${1:-x}; shift
OUT=${OUT:-out/gpu_check}
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/gputest_$TAG.log 2>&1
RC=$?
tail -3 $OUT/gputest_$TAG.log
[ $RC -ne 0 ] && exit $RC
timeout -k 10 900 python bench.py --full "$@" > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -5 $OUT/bench_$TAG.err; exit 1; }
python - <<PY
import json
d = json.loads(open("$OUT/bench_$TAG.json").read().strip().splitlines()[-1])
r = d["roofline"]
print("value", d["value"], "ms/step", d["ms_per_step"], "kernel ms", r["avg_kernel_ms"], "frac", r["frac"], "valu", r.get("valu", {}).get("frac"),
      {k: v["value"] for k, v in d.get("other_configs", {}).items() if isinstance(v, dict)}, {k: v for k, v in d.get("cpu_baseline", {}).items() if k in ("value", "cores", "single_thread_value", "gpu_result_bit_identical_on_sample")})
PY
