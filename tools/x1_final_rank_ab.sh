#!/bin/bash
# Who ranks the k-NN entries of the fused tail: the final kernel (ARROWSPACE_X1_FINAL_RANK=1, default) against the first kernel's
# last block (=0), same box, interleaved.
#   bash tools/x1_final_rank_ab.sh [pairs]         the headline (python bench.py --gpus 1 --steps 200 --warmup 20), `pairs` (5) times 0 then 1
#   bash tools/x1_final_rank_ab.sh side            the side shapes (the tail is half of the step), once per switch position
#   bash tools/x1_final_rank_ab.sh blocks          blocks of the first tail kernel (as_set_tuning("x1_blocks"): 64 / 128 / 256), new form
# Every run under its own time limit; the first run that fails ends the script.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
line() {   # $1 = label; the bench's JSON line on stdin
  python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$1', 'q/s=%.1f' % d['value'], 'ms_per_step=%.5f' % d['ms_per_step'], 'in-dist q/s', d.get('in_distribution_queries', {}).get('value'), 'verified.mismatches', d.get('verified', {}).get('mismatches'), 'fallback_rate', d.get('fallback_rate', {}).get('rate'), 'reruns', d.get('fallback_rate', {}).get('searches_with_rerun'))"
}
case "${1:-5}" in
  side)
    for shape in "--n 200000 --d 768" "--n 400000 --d 384 --k 4 --topk 2"; do
      for v in 0 1; do
        ARROWSPACE_X1_FINAL_RANK=$v timeout -k 10 300 python bench.py --gpus 1 --steps 300 --warmup 30 --full --no-cpu-baseline --no-live-traffic --no-threaded --no-distributions --no-host-build $shape 2>/dev/null \
          | grep '^{"metric"' | line "x1_final_rank=$v [$shape]" || exit 1
      done
    done
    ;;
  blocks)
    timeout -k 10 400 python tools/x1_blocks_bench.py 2>/dev/null || exit 1
    ;;
  *)
    for rep in $(seq 1 "${1:-5}"); do
      for v in 0 1; do
        ARROWSPACE_X1_FINAL_RANK=$v timeout -k 10 400 python bench.py --gpus 1 --steps 200 --warmup 20 2>/dev/null | grep '^{"metric"' | line "x1_final_rank=$v pair $rep" || exit 1
      done
    done
    ;;
esac
