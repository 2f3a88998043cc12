# Whole validation on one GPU: the GPU suite, smoke() and the full benchmark line.
#   tools/gpu/validate.sh [OUTDIR]   (default validate_out/)
set -o pipefail
O=${1:-validate_out}
mkdir -p "$O"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$O/pytest_gpu.log" 2>&1 && \
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1 && \
timeout -k 10 500 python -u bench.py --full > "$O/bench.log" 2>&1
