#!/bin/bash
# the knob below is read by the laboratory build only: make -C sglang_awq_amd/csrc lab  (-DAWQ_LAB -> sglang_awq_amd/lib_ab)
export LD_LIBRARY_PATH=${AB_LIB:-sglang_awq_amd/lib_ab}:$LD_LIBRARY_PATH
# A/B of the hand-pipelined small-group tiles (awq_repacked_prefill_sg.hip, fp16 with group size 64 / 32, forced as variant 8: the
# planned form; AB_SIDES may add "wide" / "narrow": variants 9 / 10) against the route they would replace (AWQ_TILES_SG=0: the generic
# 128 x 256 tiles) with tools/kbench rgemm: rotating weight sets, graph replay, the sides alternating in one call, old and new AB_REPS
# times each: the spread of identical runs.  Beside each pair the fp16 g = 128 route on the same shape and rows (what the small groups
# still cost).  Fewer iterations at many rows: every run times 0.1 .. 0.5 s of work.  AB_ROUNDS=1 appends full rounds of 16 x 16 tiles
# per width at K = 4096 (the round constants of awq_dispatch.h).  Every kbench run has its own time limit; the first failure ends the script.
out=${1:-ab_tiles_sg.log}
rows=${2:-"33 64 65 96 128 160 256 512 2048 4096"}
reps=${AB_REPS:-2}
sides=${AB_SIDES:-"old new g128"}
groups=${AB_GROUPS:-"64 32"}
: > $out
# run <label> M K N g sets iters variant
run() { echo -n "[$1] " >> $out; env AWQ_TILES_SG=0 KBENCH_WS=0 timeout -k 10 120 tools/kbench rgemm $2 $3 $4 $5 $6 $7 1 0 $8 0 >> $out 2>&1 || exit 1; }
default_shapes="4096 4096;4096 12288;4096 22016;11008 4096;8192 28672 8"
IFS=';' read -ra shapes <<< "${AB_SHAPES:-$default_shapes}"
for shape in "${shapes[@]}"; do
  set -- $shape
  sets=${3:-16}
  for M in $rows; do
    iters=$([ $M -le 256 ] && echo 800 || { [ $M -le 512 ] && echo 400 || { [ $M -le 2048 ] && echo 160 || echo 96; }; })
    for g in $groups; do
      for rep in $(seq 1 $reps); do
        for side in $sides; do
          case $side in
            old) run "g$g parent" $M $1 $2 $g $sets $iters 0 ;;
            new) run "g$g tiles" $M $1 $2 $g $sets $iters 8 ;;
            wide) run "g$g tiles 256+192" $M $1 $2 $g $sets $iters 9 ;;
            narrow) run "g$g tiles 128" $M $1 $2 $g $sets $iters 10 ;;
            g128) if [ $rep -eq 1 ] && [ $g = "${groups%% *}" ]; then run "g128 route" $M $1 $2 128 $sets $iters 0; fi ;;
          esac
        done
      done
    done
  done
done
if [ "${AB_ROUNDS:-0}" = 1 ]; then
  echo "# full rounds of 16 x 16 tiles per width at K = 4096 and the 128- against 256-wide tiling at 256 rows on 4096 x 11008" >> $out
  for rep in $(seq 1 $reps); do
    for g in $groups; do
      run "g$g 256-wide: 16 x 16 tiles, variant 9" 2048 4096 4096 $g 16 160 9
      run "g$g 192-wide: 16 x 16 tiles, variant 8" 2048 4096 3072 $g 16 160 8
      run "g$g 128-wide: 16 x 16 tiles, variant 10" 2048 4096 2048 $g 16 160 10
      run "g$g 128-wide: 172 tiles at 256 rows, variant 10" 256 4096 11008 $g 16 800 10
      run "g$g 256-wide: 86 tiles at 256 rows, variant 9" 256 4096 11008 $g 16 800 9
    done
  done
fi
