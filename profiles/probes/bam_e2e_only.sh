cd "$(dirname "$0")/../.." && mkdir -p bench_out/t1
NABWA_TIMING=1 timeout -k 10 300 python3 bench.py --full --steps 2 --warmup 1 --no-cpu > bench_out/t1/head.json 2> bench_out/t1/head.err; echo rc=$?
python3 -c "import json;d=json.load(open('bench_out/t1/head.json'));print('e2e', d['e2e']['reads_per_s'], d['e2e']['first_batch_reads_per_s'], d['e2e']['stage_ms'])"
grep -n "se_posn\|bam_batch\|se_refine" bench_out/t1/head.err | tail -6 | cut -c1-300
