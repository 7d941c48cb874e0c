(python -m pytest tests -m gpu -q -x 2>&1 | grep -E "passed|failed|Error" | tail -5)
OUT=${1:?usage: tools/gpu_check.sh <outdir>}; mkdir -p "$OUT"
python bench.py --full --cpu-baseline off > "$OUT/b1.json" 2>"$OUT/b1.err"; python bench.py --full --scans 8 --cpu-baseline off > "$OUT/b8.json" 2>>"$OUT/b1.err"
python - "$OUT" <<'PY'
import json, os, sys
for f in ("b1.json", "b8.json"):
    d=json.load(open(os.path.join(sys.argv[1], f))); r=d['roofline']; print(d['value'], d['ms_per_step'], r['avg_launch_us'], r['first_round_launch_us'], r['final_launch_us'])
PY
python tools/stamps.py 16 2>&1 | tail -17
