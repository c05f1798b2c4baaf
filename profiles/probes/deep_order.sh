cd "$(dirname "$0")/../.." && mkdir -p bench_out/do
NABWA_DEEP_DUMP=$PWD/bench_out/do/dump.bin timeout -k 10 300 python3 bench.py --full --adna --reads 1000000 --steps 1 --warmup 0 --no-cpu --no-e2e > bench_out/do/out.json 2> bench_out/do/err.log || exit 1
ls -la bench_out/do/dump.bin
python3 profiles/probes/deep_order_probe.py bench_out/do/dump.bin 4096 | tee bench_out/do/probe.txt
