set -o pipefail
OUT=${OUT:-bench_logs}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 150 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 && \
timeout -k 10 240 python -u bench.py --full --check > "$OUT/bench_c2.log" 2>&1 && \
timeout -k 10 200 python -u bench.py --config c2 --separate --check > "$OUT/bench_c2sep.log" 2>&1 && \
timeout -k 10 200 python -u bench.py --config c2enc --check > "$OUT/bench_c2enc.log" 2>&1 && \
timeout -k 10 200 python -u bench.py --config c3 > "$OUT/bench_c3.log" 2>&1 && \
timeout -k 10 200 python -u bench.py --config c3r --check > "$OUT/bench_c3r.log" 2>&1 && \
timeout -k 10 200 python -u bench.py --full --config c4 --check > "$OUT/bench_c4.log" 2>&1 && \
timeout -k 10 300 python -u bench.py --config c5 --stream-gib 128 > "$OUT/bench_c5.log" 2>&1 && \
timeout -k 10 300 python -u bench.py --config c5r --stream-gib 128 --check > "$OUT/bench_c5r.log" 2>&1 && \
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
rc=$?
tail -3 "$OUT/pytest_gpu.log"; cat "$OUT"/bench_*.log "$OUT/smoke.log" | grep -v amdgpu.ids
exit $rc
