cd "$(dirname "$0")/../.." && mkdir -p bench_out/abf
for v in own2 own4 own8 own16; do
export NABWA_LIB=$PWD/gpurun_ab/lib_$v.so
timeout -k 10 300 python3 bench.py --full --steps 4 --warmup 1 --no-cpu --no-e2e > bench_out/abf/$v.json 2> bench_out/abf/$v.err || { echo "$v failed"; tail -3 bench_out/abf/$v.err; continue; }
python3 -c "import json;d=json.load(open('bench_out/abf/$v.json'));r=d['roofline'];print('$v', d['value'], 'S', r['search_kernel_ms'], 'D', r['deep_kernel_ms'], 'W', r['width_kernel']['kernel_ms'], d['config']['checksum'])"
done
