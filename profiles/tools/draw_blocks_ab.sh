#!/bin/bash
# A/B of two builds of the library around the proposal draw, alternating:
#   bash profiles/tools/draw_blocks_ab.sh LIBDIR OUTDIR
# LIBDIR holds parent.so (the parent commit's libnautilus_hip.so) and pr.so.
#   1. five pairs of the default bench line (first pair with --dump-outputs,
#      compared array by array) -> OUTDIR/bench_<lib>_<i>.json, step_runs.txt
#   2. five pairs of tools/draw_bench.py -> OUTDIR/draw_alone.txt
#   3. counter passes over nb_draw_kernel, one counter per rocprofv3 pass,
#      kernel trace only -> OUTDIR/draw_pmc_raw.txt
#   4. pairs of bench.py --full --no-cpu-baseline (roofline_draw) while the
#      time budget lasts -> OUTDIR/full_<lib>_<i>.json, full_runs.txt
# Every GPU step runs under its own time limit; the script stops at the first
# step that fails.
L=$(realpath "$1"); O=$(realpath -m "$2"); mkdir -p "$O"
T=$(dirname "$0")
T0=$(date +%s)
el() { echo $(( $(date +%s) - T0 )); }
check() { [ "$1" -ne 0 ] && { echo "FAILED ($1): $2"; exit 1; }; return 0; }
export TMPDIR=/tmp

for i in 1 2 3 4 5; do
  for v in parent pr; do
    extra=""; [ $i -eq 1 ] && extra="--dump-outputs $O/dump_$v"
    NAUTILUS_HIP_LIB=$L/$v.so timeout -k 10 240 python bench.py --gpus 1 --steps 20 --warmup 3 $extra > $O/bench_${v}_$i.json 2> $O/bench_${v}_$i.err
    check $? "bench $v $i"
    python $T/draw_blocks_pick.py line $O/bench_${v}_$i.json "$v $i" | tee -a $O/step_runs.txt
  done
done
python $T/draw_blocks_pick.py dumps $O/dump_parent $O/dump_pr | tee $O/dump_compare.txt

for i in 1 2 3 4 5; do
  for v in parent pr; do
    echo "== run $i $v" | tee -a $O/draw_alone.txt
    NAUTILUS_HIP_LIB=$L/$v.so timeout -k 10 120 python $T/draw_bench.py 2>/dev/null | tee -a $O/draw_alone.txt
    check ${PIPESTATUS[0]} "draw_bench $v $i"
  done
done

pass() {  # lib n_dim counter
  local d=/tmp/pd_$1_$2_$3; rm -rf $d
  NAUTILUS_HIP_LIB=$L/$1.so timeout -k 10 180 rocprofv3 --pmc $3 --kernel-trace --output-format csv -d $d -o p -- python $T/draw_pmc.py $2 > $d.log 2>&1
  check $? "pmc $1 $2 $3"
  python $T/draw_blocks_pick.py pmc $d $3 "$1 n_dim=$2" | tee -a $O/draw_pmc_raw.txt
}
for c in SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_BUSY_CYCLES SQ_WAVES GRBM_GUI_ACTIVE; do
  for v in parent pr; do pass $v 50 $c; done
done
for c in SQ_ACTIVE_INST_VALU SQ_INSTS_VALU GRBM_GUI_ACTIVE; do
  for v in parent pr; do pass $v 100 $c; done
done

T0=$(date +%s)
for i in 1 2 3 4 5; do
  [ $(el) -gt 560 ] && { echo "time budget: stopping before pair $i"; break; }
  for v in parent pr; do
    NAUTILUS_HIP_LIB=$L/$v.so timeout -k 10 400 python bench.py --gpus 1 --steps 20 --warmup 3 --full --no-cpu-baseline > $O/full_${v}_$i.json 2> $O/full_${v}_$i.err
    check $? "bench --full $v $i"
    python $T/draw_blocks_pick.py line $O/full_${v}_$i.json "full $v $i" | tee -a $O/full_runs.txt
  done
done
