set -u
cd "$GRAFT_REPO_ROOT"
LOGS="${LNERF_LOG_DIR:-logs}"; mkdir -p "$LOGS"
for r in 1 2; do for g in 32 64 128 256 512; do
  timeout -k 10 120 python bench.py --full --config cfg2 --dw-grid $g --steps 50 --warmup 10 --no-render --no-cpu-baseline --no-cfg2 > "$LOGS/c2.log" 2>&1 || { tail -3 "$LOGS/c2.log"; exit 1; }
  python -c "
import json, sys; d=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1]); print($g, round(d['ms_per_step'],4), {k: round(v,4) for k,v in d['kernels_ms'].items()})" "$LOGS/c2.log"
done; done
