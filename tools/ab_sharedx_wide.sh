#!/bin/bash
# the knob below is read by the laboratory build only: make -C sglang_awq_amd/csrc lab  (-DAWQ_LAB -> sglang_awq_amd/lib_ab)
export LD_LIBRARY_PATH=sglang_awq_amd/lib_ab:$LD_LIBRARY_PATH
# A/B of the shared-activation GEMV for 33 .. 64 rows on wide matrices (awq_repacked_sharedx_wide.hip, AWQ_SHAREDX_WIDE=1; =2 also
# runs 65 .. 128 rows as two passes of it) against the route it replaces (AWQ_SHAREDX_WIDE=0: passes of the 32-row GEMV or under-filled
# tiles; with KBENCH_WS=1 the split-K tiles where they apply) with tools/kbench rgemm: 16 rotating weight sets, graph replay, the
# sides alternating in one call.  The first shape runs twice: the spread of identical runs.  One matrix per strip width G = 3 .. 8
# and a deep one; M = 32 with the knob off is the floor quoted beside the table (one pass of the 32-row kernel).
out=${1:-ab_sharedx_wide.log}
rows=${2:-"32 33 40 48 49 56 64"}
: > $out
run() { echo -n "[$1] " >> $out; env $1 timeout -k 10 120 tools/kbench rgemm $2 $3 $4 128 ${5:-16} 1600 1 >> $out 2>&1 || exit 1; }
first=1
default_shapes="4096 22016;4096 12288;4096 16384;4096 20480;4096 28672;4096 32768;8192 28672 8"
IFS=';' read -ra shapes <<< "${AB_SHAPES:-$default_shapes}"
for shape in "${shapes[@]}"; do
  set -- $shape
  for M in $rows; do
    for rep in $(seq 1 $((first + 1))); do
      for cfg in "AWQ_SHAREDX_WIDE=0 KBENCH_WS=0" "AWQ_SHAREDX_WIDE=2 KBENCH_WS=0" "AWQ_SHAREDX_WIDE=0 KBENCH_WS=1"; do
        [ $M -le 32 ] && [ "$cfg" != "AWQ_SHAREDX_WIDE=0 KBENCH_WS=0" ] && continue
        run "$cfg" $M $1 $2 $3
      done
    done
  done
  first=0
done
