#!/bin/bash
root=$(cd "$(dirname "$0")/.." && pwd); out=$(mkdir -p "${1:?usage: bash tools/r6_check_box.sh OUT}" && cd "$1" && pwd)
cd "$root"
python bench.py --full --config 2048x1024 --steps 3 --no-cpu-baseline --no-io --no-other-configs > "$out/plain.json" 2> "$out/plain.err"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof" -- python3 "$root/bench.py" --full --config 2048x1024 --steps 2 --no-cpu-baseline --no-io --no-other-configs > "$out/prof.json" 2> "$out/prof.err"
cd "$root"; rm -rf "$out/prof"
python - "$out" <<'PY'
import json, sys
for f in ("plain", "prof"):
    j = json.loads(open(f"{sys.argv[1]}/{f}.json").read().strip().splitlines()[-1])
    print(f, j["value"], json.dumps(j["box"])[:700])
PY
