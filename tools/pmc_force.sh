#!/bin/bash
# GPU box: hardware counters of the fermion-force kernel k_force<16, false, false> -- one call at 64^4, m = 16, four shifts in
# one launch (tools/force_time.py --single) under rocprofv3 --pmc, one pass per counter group, nothing else traced.
# usage: tools/pmc_force.sh [outdir]      prints one line per kernel and counter (average per launch)
# (the derived FETCH_SIZE / WRITE_SIZE cannot be collected in one pass here: the profiler refuses the request)
out=${1:-bench_out/pmc_force}
export TMPDIR=/tmp
i=0
for g in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR" \
         "SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_ANY"; do
  i=$((i+1)); rm -rf "$out/$i"
  timeout -k 10 300 rocprofv3 --pmc $g --output-format csv -d "$out/$i" -- python tools/force_time.py --single \
      > "$out.$i.log" 2>&1 || { echo "pass $i failed: $g"; tail -3 "$out.$i.log"; exit 1; }
done
python3 - "$out" <<'PY'
import collections, csv, glob, re, sys
agg = collections.defaultdict(lambda: [0.0, 0])
for f in glob.glob(sys.argv[1] + "/*/**/*_counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        m = re.search(r"(k_\w+<[^>]*>)", r["Kernel_Name"])
        if not m or not m.group(1).startswith(("k_force", "k_hop4b")):
            continue
        a = agg[(m.group(1), r["Counter_Name"])]
        a[0] += float(r["Counter_Value"])
        a[1] += 1
for (k, c), (v, n) in sorted(agg.items()):
    print("%-36s %-22s %.6g  (launches %d)" % (k, c, v / n, n))
PY
