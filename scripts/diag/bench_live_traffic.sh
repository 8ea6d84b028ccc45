cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${1:?usage: bench_live_traffic.sh OUTPUT_DIR}; mkdir -p "$OUT"
T0=$(date +%s)
python3 bench.py --full > "$OUT/bench_live_line.json" 2> "$OUT/bench_live.err"; echo rc=$?
echo "wall $(( $(date +%s) - T0 )) s"; wc -c "$OUT/bench_live_line.json"
python3 - "$OUT/bench_live_line.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["roofline"]); print(d.get("roofline_mixdec"))
f=json.load(open(d["full"])); print(f.get("live_traffic_bytes_per_launch")); print(f["roofline_mixdec"].get("traffic"), f["roofline_mixdec"].get("traffic_source"))
PY
