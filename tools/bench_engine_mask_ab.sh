#!/bin/bash
# in-pipeline engine A/B: value + gated GEMM per engine mask
for e in 3 2 3 2; do
  tools/gpu_step.sh 200 r03p_e$e.log python -u bench.py --full --no-cpu-baseline --gemm-engine $e || exit 1
  python3 - "$e" <<'PY'
import json,sys
d=[json.loads(l) for l in open(f"gpurun_out/r03p_e{sys.argv[1]}.log") if l.startswith("{")][0]
g={k:v["avg_us"] for k,v in d["kernels"].items() if "Gated" in k or "rglru" in k}
print("engine", sys.argv[1], "value", d["value"], "prefill_ms", d["prefill_ms"], g, flush=True)
PY
done
