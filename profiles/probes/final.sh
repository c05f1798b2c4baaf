cd "$(dirname "$0")/../.." && mkdir -p bench_out/final && timeout -k 10 900 python -m pytest tests -x -q -m gpu > bench_out/final/pytest.log 2>&1; echo suite rc=$?; tail -3 bench_out/final/pytest.log | cut -c1-220
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > bench_out/final/smoke.log 2>&1; echo smoke rc=$?; tail -2 bench_out/final/smoke.log | cut -c1-300
timeout -k 10 400 python3 bench.py --full --steps 5 --warmup 1 > bench_out/final/headline.json 2> bench_out/final/headline.log; echo bench rc=$?
