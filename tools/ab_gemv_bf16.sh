#!/bin/bash
# the knob below is read by the laboratory build only: make -C sglang_awq_amd/csrc lab  (-DAWQ_LAB -> sglang_awq_amd/lib_ab)
export LD_LIBRARY_PATH=${AB_LIB:-sglang_awq_amd/lib_ab}:$LD_LIBRARY_PATH
# A/B of the straight-line bf16 decode GEMV (awq_repacked_gemv_bf16.hip, forced as variant 7) against the route it would replace
# (AWQ_GEMV_BF16=0: gemv_rpx_kernel, or gemv_sharedx_bf16_kernel on 5- and 6-group strips) with tools/kbench rgemm: 16 rotating
# weight sets, graph replay, the sides alternating in one call, every configuration AB_REPS times: the spread of identical runs.
# Beside each pair the fp16 route (gemv_rp2_kernel where it has the shape) on the same shape and rows: what bf16 still costs.
# One matrix per strip width G = 1 .. 8 (two at G = 2 and 3) and three deep ones at 1 / 8 / 16 rows; two deeper ones (the one-row long form) at one row.
# A cell the new kernel has no instantiation for prints kbench's refusal and goes on: it stays unrouted.
out=${1:-ab_gemv_bf16.log}
rows=${2:-"1 8 16"}
reps=${AB_REPS:-2}
sides=${AB_SIDES:-"old new f16"}
: > $out
# run <label> M K N sets variant dtype; a refused variant (status -7) is a cell without an instantiation, anything else ends the run
run() {
  echo -n "[$1] " >> $out
  env AWQ_GEMV_BF16=0 KBENCH_WS=0 timeout -k 10 120 tools/kbench rgemm $2 $3 $4 128 $5 1600 1 0 $6 $7 >> $out 2>&1
  local rc=$?
  [ $rc -eq 0 ] && return 0
  [ $rc -ge 124 ] && exit 1
  [ $6 -eq 7 ] && tail -1 $out | grep -q "variant" && return 0
  exit 1
}
default_shapes="4096 4096;4096 8192;4096 11008;4096 12288;4096 16384;4096 20480;4096 22016;4096 28672;4096 32768;11008 4096;8192 7168;8192 28672 8;14336 4096 16 1;28672 8192 8 1"
IFS=';' read -ra shapes <<< "${AB_SHAPES:-$default_shapes}"
for shape in "${shapes[@]}"; do
  set -- $shape
  sets=${3:-16}
  for M in $rows; do
    [ -n "$4" ] && [ $M -gt $4 ] && continue
    for rep in $(seq 1 $reps); do
      for side in $sides; do
        case $side in
          old) run "bf16 parent" $M $1 $2 $sets 0 1 ;;
          new) run "bf16 gemv" $M $1 $2 $sets 7 1 ;;
          f16) run "fp16 route" $M $1 $2 $sets 0 0 ;;
        esac
      done
    done
  done
done
