#!/bin/bash
# Runs on the GPU box: bench.py --full (live PMC traffic passes + CPU baseline), wall time of the whole command, the roofline objects.
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd /tmp && export TMPDIR=/tmp && cd "$ROOT" || exit 1
T=$(mktemp -d)
S=$(date +%s)
python bench.py --full "$@" > "$T"/bench_live.json 2> "$T"/bench_live.err || { tail -20 "$T"/bench_live.err; exit 1; }
echo "whole command: $(( $(date +%s) - S )) s"
python - "$T"/bench_live.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["roofline"])
print("batch traffic", d["roofline_batch"]["traffic"], "build traffic", d["roofline_build"]["traffic"])
PY
