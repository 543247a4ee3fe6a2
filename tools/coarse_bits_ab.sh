#!/bin/bash
# Width of the single query's coarse operand: the 8-bit tiles (ARROWSPACE_COARSE_BITS=8) against the nibble tiles (=4), same box,
# interleaved, over plain bench.py runs.
#   bash tools/coarse_bits_ab.sh [pairs]         the headline (python bench.py --gpus 1 --steps 200 --warmup 20), `pairs` (5) times 8 then 4
#   bash tools/coarse_bits_ab.sh side            side shapes that the automatic rule leaves on 8 bits: -1 (auto) against 8, once each
# Every run under its own time limit; the first run that fails ends the script, nothing is tried again.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
line() {   # $1 = label; the bench's JSON line on stdin
  python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('$1', 'q/s=%.1f' % d['value'], 'ms_per_step=%.5f' % d['ms_per_step'], 'operand', d.get('scan_operand', d.get('config', {}).get('scan_operand')), 'zero_lambda', d.get('zero_lambda'), 'index_build_sec %.2f' % d.get('index_build_sec', float('nan')))"
}
case "${1:-5}" in
  side)
    for shape in "--n 200000 --d 768" "--n 400000 --d 384 --k 4 --topk 2"; do
      for v in 8 -1; do
        ARROWSPACE_COARSE_BITS=$v timeout -k 10 300 python bench.py --gpus 1 --steps 300 --warmup 30 $shape 2>/dev/null \
          | grep '^{"metric"' | line "coarse_bits=$v [$shape]" || exit 1
      done
    done
    ;;
  *)
    for rep in $(seq 1 "${1:-5}"); do
      for v in 8 4; do
        ARROWSPACE_COARSE_BITS=$v timeout -k 10 400 python bench.py --gpus 1 --steps 200 --warmup 20 2>/dev/null | grep '^{"metric"' | line "coarse_bits=$v pair $rep" || exit 1
      done
    done
    ;;
esac
