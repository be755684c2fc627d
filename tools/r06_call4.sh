#!/bin/bash
# r06: locate tests + index --verify test, repeats-genome configuration (default and DICEY_VERIFY_CH=4), kernel stats
cd "$GRAFT_REPO_ROOT"
ROOT=$PWD
export TMPDIR=/tmp
O=gpurun_out/r06
T=${1:-c}
mkdir -p $O
timeout 900 python -m pytest tests/test_gpu_locate_topk.py tests/test_gpu_cli.py::test_index_verify_accepts_its_file_and_refuses_foreign_ones tests/test_gpu_parity.py -m gpu -x -q > $O/pytest_$T.log 2>&1
tail -4 $O/pytest_$T.log
timeout 900 python bench.py --full --genome repeats --steps 30 --warmup 8 --no-extras --no-extra-configs --cpu-seconds 3 --parity-queries 300 --keep-index \
  --detail-out $O/repeats_detail_$T.json > $O/repeats_$T.json 2> $O/repeats_$T.err
FM9=$(ls /dev/shm/dicey_bench_*repeats*.fm9 | head -1)
for CH in 4 2; do
DICEY_VERIFY_CH=$CH timeout 600 python bench.py --full --genome repeats --fm9 $FM9 --steps 30 --warmup 8 --no-extras --no-extra-configs --no-cpu-baseline --parity-queries 0 \
  --detail-out $O/repeats_detail_${T}_ch$CH.json > $O/repeats_${T}_ch$CH.json 2> $O/repeats_${T}_ch$CH.err
done
python - $T <<'PY'
import json, sys
for sfx in ("", "_ch4", "_ch2"):
    try:
        d = json.load(open("gpurun_out/r06/repeats_detail_%s%s.json" % (sys.argv[1], sfx)))
        print("repeats%s:" % sfx, "%.1f M" % (d["value"] / 1e6), "%.3f ms" % d["ms_per_step"], {k: round(v, 3) for k, v in d["phases_ms"].items()}, d.get("parity_sample"),
              "one at a time %.1f M" % (d.get("value_one_in_flight", {}).get("value", 0) / 1e6))
    except Exception as e:
        print(sfx, e)
PY
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $ROOT/$O/trace_rep_$T -o trace --output-format csv -- python $ROOT/bench.py --full --genome repeats --fm9 $FM9 --no-cpu-baseline --no-extras --no-extra-configs --parity-queries 0 --steps 12 --warmup 4 --detail-out $ROOT/$O/rep_traced_detail_$T.json > $ROOT/$O/rep_traced_$T.json 2> $ROOT/$O/rep_trace_$T.err)
python - $T <<'PY'
import csv, sys, os
sys.path.insert(0, "tools")
from profnames import short_kernel_name
T = sys.argv[1]
rows = list(csv.DictReader(open("gpurun_out/r06/trace_rep_%s/trace_kernel_stats.csv" % T)))
with open("gpurun_out/r06/repeats_kernel_stats_%s.csv" % T, "w") as f:
    f.write("kernel,calls,total_ms,avg_us,min_us,max_us\n")
    for r in rows:
        n = short_kernel_name(r["Name"])
        f.write('"%s",%s,%.3f,%.2f,%.2f,%.2f\n' % (n[:90], r["Calls"], float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
        if int(r["Calls"]) >= 5 and "dg::" in n and float(r["AverageNs"]) > 15e3:
            print("%-46s calls %4s avg %9.1f min %9.1f max %9.1f us" % (n[:46], r["Calls"], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
PY
rm -rf $O/trace_rep_$T/*/*.db; find $O -name "*.db" -delete
rm -f /dev/shm/dicey_bench_*
