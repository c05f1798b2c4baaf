cd "$(dirname "$0")/../.." && mkdir -p bench_out/adna_t
NABWA_TIMING=1 timeout -k 10 500 python3 bench.py --full --adna --reads 1000000 --steps 1 --warmup 0 --no-cpu --no-e2e > bench_out/adna_t/out.json 2> bench_out/adna_t/err.log; echo rc=$?
grep "kernel D" bench_out/adna_t/err.log | head -5
