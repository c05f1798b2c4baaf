// tests/emu/bam_sort_host_main.cpp -- TEST INFRASTRUCTURE ONLY.  The host half of `nabwa_bam2bam --sort` (csrc/bam_sort_host.hpp) as a
// stand-alone program: the NABWA_SORT=host sort of a run and the merge of sorted runs by their keys.
//
//     bam_sort_host_main RECORDS THREADS RUN_BYTES [REPEATS]
//
// RECORDS: a file of BAM records back to back (u32 block_size + block).  They are cut into runs as the tool cuts them (a run is closed by
// the record that brings it to RUN_BYTES; 0: one run), every run is sorted by THREADS threads, the runs are merged, and the result goes to
// stdout (not with REPEATS: a timing run).  stderr: "runs <R>" and, per repeat, "sort_ms <milliseconds>" for the sorting of the runs alone.
// Exit 3: a bad block_size.
#include <stdio.h>
#include <stdlib.h>
#include <chrono>
#include "../../network-aware-bwa_amd/csrc/bam_sort_host.hpp"

int main(int argc, char **argv)
{
	if (argc < 4) { fprintf(stderr, "usage: bam_sort_host_main RECORDS THREADS RUN_BYTES [REPEATS]\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	fseek(f, 0, SEEK_END);
	const long size = ftell(f);
	fseek(f, 0, SEEK_SET);
	std::vector<uint8_t> in((size_t)size);
	if (size && fread(in.data(), 1, (size_t)size, f) != (size_t)size) { perror(argv[1]); return 2; }
	fclose(f);
	const int nt = atoi(argv[2]), repeats = argc > 4 ? atoi(argv[4]) : 1;
	const int64_t run_bytes = atoll(argv[3]);
	std::vector<int64_t> off(1, 0);
	for (size_t q = 0; q < in.size(); ) { uint32_t bs; memcpy(&bs, &in[q], 4); q += 4 + (size_t)bs; off.push_back((int64_t)q); }
	if (off.back() != (int64_t)in.size()) { fprintf(stderr, "the last record runs past the file\n"); return 2; }
	const size_t n = off.size() - 1;
	std::vector<size_t> cut(1, 0);                      /* runs: records cut[r] .. cut[r + 1] - 1 */
	for (size_t i = 0; i < n; ++i) if (run_bytes > 0 && off[i + 1] - off[cut.back()] >= run_bytes) cut.push_back(i + 1);
	if (cut.back() != n) cut.push_back(n);
	const size_t R = cut.size() - 1;
	std::vector<uint8_t> sorted(in.size() ? in.size() : 1);
	std::vector<std::vector<int64_t>> roff(R);
	std::vector<std::vector<uint64_t>> rkeys(R);
	for (int rep = 0; rep < repeats; ++rep) {
		const auto t0 = std::chrono::steady_clock::now();
		for (size_t r = 0; r < R; ++r) {
			const size_t m = cut[r + 1] - cut[r];
			roff[r].assign(m + 1, 0); rkeys[r].assign(m, 0);
			const int64_t bad = bam_sort_host(nt, (int64_t)m, in.data(), off.data() + cut[r], sorted.data() + off[cut[r]], roff[r].data(), rkeys[r].data());
			if (bad >= 0) { fprintf(stderr, "bad block_size at record %lld of run %zu\n", (long long)bad, r); return 3; }
		}
		fprintf(stderr, "sort_ms %.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	}
	fprintf(stderr, "runs %zu\n", R);
	if (argc > 4) return 0;                            /* REPEATS given: a timing run, nothing is written */
	std::vector<const std::vector<uint64_t>*> keys;
	for (auto &k : rkeys) keys.push_back(&k);
	bam_sort_merge(keys, [&](size_t r, size_t i) {
		fwrite(sorted.data() + off[cut[r]] + roff[r][i], 1, (size_t)(roff[r][i + 1] - roff[r][i]), stdout);
	});
	return 0;
}
