"""One line per bench.py result file: the headline and, for a --full run, the extra workloads.  line.py result.json label rep"""
import json
import sys

d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(*sys.argv[2:4], "ms_per_step %.5f" % d["ms_per_step"], "value %.4g" % d["value"], "fused kernel ms %.5f" % d.get("kernel_ms", {}).get("fused", 0.0))
for w in (d.get("extra_workloads") or {}).values():
    if isinstance(w, dict) and "ms_per_step" in w:
        print("   ", w.get("workload"), w.get("pipeline"), "ms_per_step %.5f" % w["ms_per_step"], "kernels %.5f" % w.get("kernels_total_ms", 0.0), "blocking %.5f" % w.get("blocking_ms", 0.0))
