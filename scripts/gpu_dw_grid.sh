set -u
cd "$GRAFT_REPO_ROOT"
LOGS="${LNERF_LOG_DIR:-logs}"; mkdir -p "$LOGS"
for r in 1 2; do
for g in 0 384 768 1024; do
  timeout -k 10 120 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-render --no-cfg2 --dw-grid $g > "$LOGS/grid.log" 2>&1 || { echo "grid $g failed"; tail -3 "$LOGS/grid.log"; exit 1; }
  python -c "import json,sys;d=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1]);k=d['kernels_ms'];print('grid $g', round(d['ms_per_step'],4), 'dw', round(k['dw'],4), 'reduce', round(k['reduce'],4), 'fused', round(k['fused'],4))" "$LOGS/grid.log"
done
done
