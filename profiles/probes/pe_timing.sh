cd "$(dirname "$0")/../.." && mkdir -p bench_out/pe_t
NABWA_TIMING=1 timeout -k 10 500 python3 bench.py --full --pe --pairs 1000000 --steps 2 --warmup 1 --no-cpu > bench_out/pe_t/out.json 2> bench_out/pe_t/err.log; echo rc=$?
python3 -c "import json;d=json.load(open('bench_out/pe_t/out.json'));print(d['value'], d['config']['stage_ms'], d['roofline']['search_kernel_ms'], d['roofline']['deep_kernel_ms'])"
grep -v "^\[synth\]" bench_out/pe_t/err.log | grep -i "pe_finish\|finish\|posn\|pairing\|rescue\|kernel D" | tail -24
