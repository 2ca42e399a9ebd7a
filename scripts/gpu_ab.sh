# A/B of in-tree library variants: bench.py --full per lib (LNERF_LIB), fused/dw kernel times
set -u
cd "$GRAFT_REPO_ROOT"
LOGS="${LNERF_LOG_DIR:-logs}"; mkdir -p "$LOGS"
for lib in "$@"; do
  LNERF_LIB=$lib timeout -k 10 120 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-render ${BENCH_ARGS:-} > "$LOGS/ab.log" 2>&1 || { echo "$lib failed"; tail -5 "$LOGS/ab.log"; exit 1; }
  python - "$lib" "$LOGS/ab.log" <<'PY'
import json, sys
line = [l for l in open(sys.argv[2]) if l.startswith("{")][-1]
d = json.loads(line)
print(sys.argv[1], d["mfma"][:6], "ms/step %.4f" % d["ms_per_step"], {k: round(v, 4) for k, v in d["kernels_ms"].items()})
PY
done
