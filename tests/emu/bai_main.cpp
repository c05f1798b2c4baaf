// tests/emu/bai_main.cpp -- TEST INFRASTRUCTURE ONLY.  The bodies of the BAM index (csrc/bai_body.hpp, through bai_emu.cpp) as a stand-alone
// program for AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_bai_emu.py):
//
//     bai_main CASES
//
// CASES is the file tests/bai_cases.py:write_case_file writes: per case n_ref, its calls (records, their stream offset, and the damaged
// record the Python oracle expects, -1: none), the block table, and the file and stats the oracle expects of the sound calls.  Every case
// runs at each of the 16 start alignments: each call's records in a heap buffer of its own that ends with the last record's last byte, the
// first record at residue a; the block table and the file in buffers exactly as long as they are.
// Exit 0 and "ok <checks>" on stdout, or 3 with the case that failed on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

extern "C" void *emu_bai_create(int32_t n_ref);
extern "C" void emu_bai_destroy(void *h);
extern "C" int64_t emu_bai_add(void *h, int64_t n_rec, const uint8_t *in, const int64_t *off, int64_t stream_off, int n_blocks);
extern "C" int64_t emu_bai_finish(void *h, int64_t n_blk, const int64_t *blk_u, const int64_t *blk_c, uint8_t *out, int64_t cap, uint64_t *stats);

static FILE *f;
static void get(void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "the case file is cut short\n"); exit(2); } }
static int64_t get64() { int64_t v; get(&v, 8); return v; }

struct Call { int64_t n_rec, n_bytes, stream_off, want_bad; std::vector<int64_t> off; std::vector<uint8_t> data; };

int main(int argc, char **argv)
{
	if (argc != 2 || !(f = fopen(argv[1], "rb"))) { fprintf(stderr, "usage: bai_main CASES\n"); return 2; }
	const int64_t n_cases = get64(), n_stats = get64();
	long checks = 0;
	for (int64_t c = 0; c < n_cases; ++c) {
		const int64_t n_ref = get64(), n_calls = get64();
		std::vector<Call> calls((size_t)n_calls);
		for (Call &k : calls) {
			k.n_rec = get64(); k.n_bytes = get64(); k.stream_off = get64(); k.want_bad = get64();
			k.off.resize((size_t)k.n_rec + 1); get(k.off.data(), k.off.size() * 8);
			k.data.resize((size_t)k.n_bytes); get(k.data.data(), (size_t)k.n_bytes);
		}
		const int64_t n_blk = get64();
		std::vector<int64_t> blk_u((size_t)n_blk + 1), blk_c((size_t)n_blk + 1);
		get(blk_u.data(), blk_u.size() * 8); get(blk_c.data(), blk_c.size() * 8);
		const int64_t n_want = get64();
		std::vector<uint8_t> want((size_t)n_want);
		std::vector<uint64_t> want_stats((size_t)n_stats);
		get(want.data(), want.size()); get(want_stats.data(), want_stats.size() * 8);
		for (int a = 0; a < 16; ++a) {
			void *h = emu_bai_create((int32_t)n_ref);
			for (size_t k = 0; k < calls.size(); ++k) {
				const Call &K = calls[k];
				uint8_t *buf = (uint8_t*)malloc((size_t)(a + K.n_bytes ? a + K.n_bytes : 1));      /* malloc's blocks start on a 16-byte boundary */
				if (K.n_bytes) memcpy(buf + a, K.data.data(), (size_t)K.n_bytes);
				std::vector<int64_t> off(K.off);
				for (int64_t &o : off) o += a;
				const int64_t bad = emu_bai_add(h, K.n_rec, buf, off.data(), K.stream_off, 1 + (int)((c + a + (int64_t)k) % 5));
				free(buf);
				if (bad != K.want_bad) { fprintf(stderr, "case %lld call %zu at residue %d: damaged record %lld (expected %lld)\n", (long long)c, k, a, (long long)bad, (long long)K.want_bad); return 3; }
				++checks;
			}
			int64_t *bu = (int64_t*)malloc(blk_u.size() * 8), *bc = (int64_t*)malloc(blk_c.size() * 8);
			memcpy(bu, blk_u.data(), blk_u.size() * 8); memcpy(bc, blk_c.data(), blk_c.size() * 8);
			uint64_t *stats = (uint64_t*)malloc((size_t)n_stats * 8);
			const int64_t size = emu_bai_finish(h, n_blk, bu, bc, nullptr, 0, stats);
			uint8_t *out = (uint8_t*)malloc((size_t)(size > 0 ? size : 1));
			const int64_t n = size == n_want ? emu_bai_finish(h, n_blk, bu, bc, out, size, stats) : -1;
			const bool same = n == n_want && !memcmp(out, want.data(), (size_t)n_want) && !memcmp(stats, want_stats.data(), (size_t)n_stats * 8);
			free(out); free(stats); free(bu); free(bc);
			emu_bai_destroy(h);
			if (!same) { fprintf(stderr, "case %lld at residue %d: another file or other counters than the oracle's (%lld bytes, expected %lld)\n", (long long)c, a, (long long)size, (long long)n_want); return 3; }
			++checks;
		}
	}
	fclose(f);
	printf("ok %ld\n", checks);
	return 0;
}
