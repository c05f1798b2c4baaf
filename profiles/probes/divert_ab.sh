cd "$(dirname "$0")/../.." && mkdir -p bench_out/dv
for dv in 0 4 3; do
export NABWA_DIVERT_CLS=$dv
timeout -k 10 300 python3 bench.py --full --pe --pairs 1000000 --steps 2 --warmup 1 --no-cpu > bench_out/dv/pe.json 2> bench_out/dv/pe.err || { tail -3 bench_out/dv/pe.err; exit 1; }
python3 -c "import json;d=json.load(open('bench_out/dv/pe.json'));print('divert $dv pe', d['value'], d['config']['stage_ms']['search (kernels W, S, D)'], d['roofline']['search_kernel_ms'], d['roofline']['deep_kernel_ms'], d['config']['second_pass_reads'], d['config']['checksum'])"
timeout -k 10 300 python3 bench.py --full --steps 3 --warmup 1 --no-cpu --no-e2e > bench_out/dv/h.json 2> bench_out/dv/h.err || exit 1
python3 -c "import json;d=json.load(open('bench_out/dv/h.json'));r=d['roofline'];print('divert $dv headline', d['value'], r['search_kernel_ms'], r['deep_kernel_ms'], d['config']['second_pass_reads'], d['config']['checksum'])"
done
