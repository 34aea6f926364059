#!/bin/bash
# the knob below is read by the laboratory build only: make -C sglang_awq_amd/csrc lab  (-DAWQ_LAB -> sglang_awq_amd/lib_ab)
export LD_LIBRARY_PATH=sglang_awq_amd/lib_ab:$LD_LIBRARY_PATH
# A/B of the shared-activation decode GEMV (awq_repacked_sharedx.hip, AWQ_SHAREDX=1) against the route it replaces (AWQ_SHAREDX=0:
# two-row-tile gemv_repacked_kernel, or gemv_rps_kernel where KBENCH_WS=1 gives it a workspace) with tools/kbench rgemm: 16 rotating
# weight sets, graph replay, both sides alternating in one call.  The first shape runs twice: the spread of identical runs.
# Shapes: the four linears of a 7B layer (gate_up also with the SiLU-mul epilogue) and the per-rank shapes of a 70B model at TP 8.
out=${1:-ab_sharedx.log}
rows=${2:-"17 24 32"}
: > $out
run() { echo -n "[$1] " >> $out; env $1 tools/kbench rgemm $2 $3 $4 128 16 1600 1 ${5:-0} >> $out 2>&1 || exit 1; }
first=1
# AB_SHAPES: another list of "K N [fuse]" (e.g. one matrix per strip width: N = 16384, 20480, 28672, 32768 are 4, 5, 7, 8 column groups)
default_shapes="4096 12288;4096 4096;4096 22016;4096 22016 2;11008 4096;8192 1280;1024 8192;8192 7168;3584 8192"
IFS=';' read -ra shapes <<< "${AB_SHAPES:-$default_shapes}"
for shape in "${shapes[@]}"; do
  set -- $shape
  for M in $rows; do
    for rep in $(seq 1 $((first + 1))); do
      for cfg in "AWQ_SHAREDX=0 KBENCH_WS=0" "AWQ_SHAREDX=1 KBENCH_WS=0" "AWQ_SHAREDX=0 KBENCH_WS=1"; do
        [ -n "$3" ] && [ "$cfg" = "AWQ_SHAREDX=0 KBENCH_WS=1" ] && continue   # the fused entry takes no workspace
        run "$cfg" $M $1 $2 $3
      done
    done
    first=0
  done
done
