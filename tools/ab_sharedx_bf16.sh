#!/bin/bash
# the knob below is read by the laboratory build only: make -C sglang_awq_amd/csrc lab  (-DAWQ_LAB -> sglang_awq_amd/lib_ab)
export LD_LIBRARY_PATH=${AB_LIB:-sglang_awq_amd/lib_ab}:$LD_LIBRARY_PATH
# A/B of the bf16 shared-activation GEMV (awq_repacked_sharedx_bf16.hip, forced as variant 3) against the route it would replace
# (AWQ_SHAREDX_BF16=0: gemv_rpx_kernel in 16-row launches, the generic tiles from 33 rows) with tools/kbench rgemm: 16 rotating
# weight sets, graph replay, the sides alternating in one call, every configuration AB_REPS times: the spread of identical runs.
# Beside each pair the fp16 shared-activation kernel on the same shape and rows (variant 1 up to 32 rows, 2 above): what the bf16
# dequantisation still costs.  One matrix per strip width G = 1 .. 8 and two deep ones; 33 rows and up on G >= 3 only.
# AB_LIB=<dir of another lab build> (e.g. one made with EXTRA="-DAWQ_LAB -DSXB_DEQUANT_F16=1") and AB_SIDES="new" time that
# build's kernel alone: the dequantisation A/B.
out=${1:-ab_sharedx_bf16.log}
rows=${2:-"1 8 16 17 24 32 33 48 49 64"}
reps=${AB_REPS:-2}
sides=${AB_SIDES:-"old new f16"}
: > $out
# run <label> <env> M K N sets variant dtype
run() { echo -n "[$1] " >> $out; env $2 KBENCH_WS=0 timeout -k 10 120 tools/kbench rgemm $3 $4 $5 128 $6 1600 1 0 $7 $8 >> $out 2>&1 || exit 1; }
default_shapes="4096 22016;4096 4096;8192 7168;4096 12288;4096 16384;4096 20480;4096 28672;4096 32768;11008 4096;8192 28672 8"
IFS=';' read -ra shapes <<< "${AB_SHAPES:-$default_shapes}"
for shape in "${shapes[@]}"; do
  set -- $shape
  sets=${3:-16}
  for M in $rows; do
    [ $M -gt 32 ] && [ $2 -le 8192 ] && continue
    for rep in $(seq 1 $reps); do
      for side in $sides; do
        case $side in
          old) run "bf16 parent" AWQ_SHAREDX_BF16=0 $M $1 $2 $sets 0 1 ;;
          new) run "bf16 shared-x" AWQ_SHAREDX_BF16=0 $M $1 $2 $sets 3 1 ;;
          f16) run "fp16 shared-x" AWQ_SHAREDX_BF16=0 $M $1 $2 $sets $([ $M -le 32 ] && echo 1 || echo 2) 0 ;;
        esac
      done
    done
  done
done
