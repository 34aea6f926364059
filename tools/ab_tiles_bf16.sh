#!/bin/bash
# the knob below is read by the laboratory build only: make -C sglang_awq_amd/csrc lab  (-DAWQ_LAB -> sglang_awq_amd/lib_ab)
export LD_LIBRARY_PATH=${AB_LIB:-sglang_awq_amd/lib_ab}:$LD_LIBRARY_PATH
# A/B of the hand-pipelined bf16 tiles (awq_repacked_prefill_bf16.hip, forced as variant 4: the planned form; AB_SIDES may add
# "wide" / "narrow": variants 5 / 6) against the route they would replace (AWQ_TILES_BF16=0: the generic 128 x 256 tiles, or the
# two-launch bf16 GEMV at 33 .. 64 rows on wide matrices) with tools/kbench rgemm: rotating weight sets, graph replay, the sides
# alternating in one call, old and new AB_REPS times each: the spread of identical runs.  Beside each pair the fp16 route on the same
# shape and rows (what the bf16 dequantisation still costs).  Fewer iterations at many rows: every run times 0.1 .. 0.5 s of work.
out=${1:-ab_tiles_bf16.log}
rows=${2:-"33 64 65 96 128 160 256 512 2048 4096"}
reps=${AB_REPS:-2}
sides=${AB_SIDES:-"old new f16"}
: > $out
# run <label> M K N sets iters variant dtype
run() { echo -n "[$1] " >> $out; env AWQ_TILES_BF16=0 KBENCH_WS=0 timeout -k 10 120 tools/kbench rgemm $2 $3 $4 128 $5 $6 1 0 $7 $8 >> $out 2>&1 || exit 1; }
default_shapes="4096 4096;4096 12288;4096 22016;11008 4096;8192 28672 8"
IFS=';' read -ra shapes <<< "${AB_SHAPES:-$default_shapes}"
for shape in "${shapes[@]}"; do
  set -- $shape
  sets=${3:-16}
  for M in $rows; do
    iters=$([ $M -le 256 ] && echo 800 || { [ $M -le 512 ] && echo 400 || { [ $M -le 2048 ] && echo 160 || echo 96; }; })
    for rep in $(seq 1 $reps); do
      for side in $sides; do
        case $side in
          old) run "bf16 parent" $M $1 $2 $sets $iters 0 1 ;;
          new) run "bf16 tiles" $M $1 $2 $sets $iters 4 1 ;;
          wide) run "bf16 tiles 256+192" $M $1 $2 $sets $iters 5 1 ;;
          narrow) run "bf16 tiles 128" $M $1 $2 $sets $iters 6 1 ;;
          f16) if [ $rep -eq 1 ]; then run "fp16 route" $M $1 $2 $sets $iters 0 0; fi ;;
        esac
      done
    done
  done
done
