#!/bin/bash
# A/B of the bf16 split-K tiles (awq_repacked_prefill_bf16.hip, SPLIT form + the reduce launch; forced as variant 11: the planned tile
# width; AB_SIDES may add "wide" / "narrow": variants 12 / 13) against the route they would replace from 65 rows: the one-workgroup-per-
# tile bf16 tiles as planned (variant 4, no workspace).  tools/kbench rgemm against the product library: rotating weight sets, graph
# replay, the sides alternating, old and new AB_REPS times each: the spread of identical runs.  Beside each pair the fp16 route on the
# same shape and rows with its workspace (fp16's own split-K tiles where they are routed).  Every GPU step under its own time limit; the
# first failure ends the script.
out=${1:-ab_split_tiles_bf16.log}
rows=${2:-"65 96 128 160 256 512"}
reps=${AB_REPS:-2}
sides=${AB_SIDES:-"old new f16"}
: > $out
# run <label> M K N sets iters variant dtype
# (a cell outside the forced variant's domain — fewer than two slices — is refused before anything is launched: logged, not an error)
run() {
  echo -n "[$1] " >> $out
  timeout -k 10 120 tools/kbench rgemm $2 $3 $4 128 $5 $6 1 0 $7 $8 >> $out 2>&1 && return
  [ $? -eq 1 ] && tail -n 1 $out | grep -q "variant cannot run" || exit 1
}
default_shapes="4096 4096;4096 12288;4096 22016;11008 4096;8192 8192;8192 28672 8"
IFS=';' read -ra shapes <<< "${AB_SHAPES:-$default_shapes}"
for shape in "${shapes[@]}"; do
  set -- $shape
  sets=${3:-16}
  for M in $rows; do
    iters=$([ $M -le 256 ] && echo 800 || echo 400)
    for rep in $(seq 1 $reps); do
      for side in $sides; do
        case $side in
          old) run "bf16 tiles" $M $1 $2 $sets $iters 4 1 ;;
          new) run "bf16 split" $M $1 $2 $sets $iters 11 1 ;;
          wide) if [ $rep -eq 1 ]; then run "bf16 split 256" $M $1 $2 $sets $iters 12 1; fi ;;
          narrow) if [ $rep -eq 1 ]; then run "bf16 split 128" $M $1 $2 $sets $iters 13 1; fi ;;
          f16) if [ $rep -eq 1 ]; then run "fp16 route" $M $1 $2 $sets $iters 0 0; fi ;;
        esac
      done
    done
  done
done
