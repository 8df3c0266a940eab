#!/bin/bash
# usage: bash profiles/launch_ab.sh <other libnig.so> [out dir]
# Do two builds of the library start the same kernels?  profiles/launch_sweep.py under rocprofv3 --kernel-trace, once per library
# (<other> through NIG_LIB_PATH, then the tree's), each in a process and under a time limit of its own; profiles/launch_trace.py
# turns each trace into its ordered launch list; the two lists are compared.  Record of one such run: profiles/launch_plan/.
set -u
export NIG_NO_AUTOBUILD=1
OTHER=$1; OUT=${2:-launch_ab_out}; mkdir -p "$OUT"
one() {   # tag, library
  NIG_LIB_PATH=$2 timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d "$OUT/trace_$1" -o "$1" -- python3 profiles/launch_sweep.py > "$OUT/sweep_$1.log" 2>&1 \
    || { echo "sweep $1 failed: $?"; tail -30 "$OUT/sweep_$1.log"; return 1; }
  python3 profiles/launch_trace.py "$(find "$OUT/trace_$1" -name '*kernel_trace.csv' | head -1)" "$OUT/launches_$1.txt" && rm -rf "$OUT/trace_$1"
}
one other "$OTHER" && one tree "$PWD/neorl-industrial-gym_amd/libnig.so" && {
  if cmp "$OUT/launches_other.txt" "$OUT/launches_tree.txt"; then echo "LAUNCH LISTS IDENTICAL"; else echo "LAUNCH LISTS DIFFER"; exit 1; fi
}
