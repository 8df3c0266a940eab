#!/bin/bash
# usage: PARENT_TREE=<checkout of the parent commit, library built> bash profiles/sampled_ab.sh [OUT_DIR] [ROUNDS]
# Same-box, same-session A/B of the fused rollout at the BASELINE shapes (250-step launches, full outputs):
#   parent  the parent commit's ring-fed nig_rollout        (its own package and libnig.so, from PARENT_TREE)
#   ring    this commit's ring-fed nig_rollout              (required to hold the same instructions: profiles/isa_diff.py)
#   sampled this commit's nig_rollout_sampled
# alternating the three ROUNDS times; every process warms its shapes up before it times them (profiles/bench_sampled.py).
# The spread of the repeated `parent` runs is the yardstick for "ring == parent".  Then (unless NO_TRACE is set) one
# rocprofv3 kernel trace of each of this commit's two paths, for kernel times without the launch overhead.  Every GPU step
# has its own time limit and the chain stops at the first step that fails.
OUT=${1:-profiles/sampled}; ROUNDS=${2:-3}
HERE=$(cd "$(dirname "$0")/.." && pwd)
export NIG_NO_AUTOBUILD=1
mkdir -p "$OUT"
: > "$OUT/ab.jsonl"
for r in $(seq 1 "$ROUNDS"); do
  if [ -n "$PARENT_TREE" ]; then
    timeout -k 10 240 python "$HERE/profiles/bench_sampled.py" --mode ring --tree "$PARENT_TREE" --tag parent >> "$OUT/ab.jsonl" || { echo "parent run failed: stopped"; exit 1; }
  fi
  timeout -k 10 240 python "$HERE/profiles/bench_sampled.py" --mode ring --tag this >> "$OUT/ab.jsonl" &&
  timeout -k 10 240 python "$HERE/profiles/bench_sampled.py" --mode sampled --tag this >> "$OUT/ab.jsonl" || { echo "a step failed: stopped"; exit 1; }
done
if [ -z "$NO_TRACE" ] && command -v rocprofv3 >/dev/null; then
  for m in ring sampled; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/trace_$m" -o "$m" --output-format csv -- \
        python "$HERE/profiles/bench_sampled.py" --mode $m --tag trace --launches 5 > "$OUT/trace_$m.jsonl" || { echo "trace $m failed: stopped"; exit 1; }
  done
fi
python - "$OUT/ab.jsonl" <<'PY' | tee "$OUT/ab.txt"
import json, statistics, sys
rows = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
keys = sorted({(r["shape"], r["tag"], r["mode"]) for r in rows})
print("%-20s %-8s %-8s %10s %10s %10s   per-process medians" % ("shape", "build", "path", "median us", "min us", "max us"))
for k in keys:
    rs = [r for r in rows if (r["shape"], r["tag"], r["mode"]) == k]
    allus = [x for r in rs for x in r["kernel_us"]]
    print("%-20s %-8s %-8s %10.1f %10.1f %10.1f   %s" % (*k, statistics.median(allus), min(allus), max(allus), [r["median_us"] for r in rs]))
PY
