// tests/emu/markdup_main.cpp -- TEST INFRASTRUCTURE ONLY.  The bodies of duplicate marking (csrc/markdup_body.hpp, through markdup_emu.cpp) as a
// stand-alone program for AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_markdup_emu.py):
//
//     markdup_main CASES
//
// CASES is the file tests/markdup_cases.py:write_case_file writes: per case its options, its calls (records, and the damaged record the
// Python oracle expects, -1: none) and the dup[] and stats the oracle expects of the sound calls.  Every case runs at each of the 16 start
// alignments: each call's records in a heap buffer of its own that ends with the last record's last byte, the first record at residue a.
// Exit 0 and "ok <checks>" on stdout, or 3 with the case that failed on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

extern "C" void *emu_markdup_create(int min_qual, int single_ends, uint32_t exclude_flags);
extern "C" void emu_markdup_destroy(void *h);
extern "C" int64_t emu_markdup_add(void *h, int64_t n_rec, const uint8_t *in, const int64_t *off, int n_blocks, int reverse);
extern "C" int64_t emu_markdup_resolve(void *h, uint8_t *dup, uint64_t *stats);

static FILE *f;
static void get(void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "the case file is cut short\n"); exit(2); } }
static int64_t get64() { int64_t v; get(&v, 8); return v; }

struct Call { int64_t n_rec, n_bytes, want_bad; std::vector<int64_t> off; std::vector<uint8_t> data; };

int main(int argc, char **argv)
{
	if (argc != 2 || !(f = fopen(argv[1], "rb"))) { fprintf(stderr, "usage: markdup_main CASES\n"); return 2; }
	const int64_t n_cases = get64(), n_stats = get64();
	long checks = 0;
	for (int64_t c = 0; c < n_cases; ++c) {
		const int64_t min_qual = get64(), single_ends = get64(), excl = get64(), n_calls = get64(), n_ord = get64();
		std::vector<Call> calls((size_t)n_calls);
		for (Call &k : calls) {
			k.n_rec = get64(); k.n_bytes = get64(); k.want_bad = get64();
			k.off.resize((size_t)k.n_rec + 1); get(k.off.data(), k.off.size() * 8);
			k.data.resize((size_t)k.n_bytes); get(k.data.data(), (size_t)k.n_bytes);
		}
		std::vector<uint8_t> want_dup((size_t)n_ord);
		std::vector<uint64_t> want_stats((size_t)n_stats);
		get(want_dup.data(), want_dup.size()); get(want_stats.data(), want_stats.size() * 8);
		for (int a = 0; a < 16; ++a) {
			void *h = emu_markdup_create((int)min_qual, (int)single_ends, (uint32_t)excl);
			for (size_t k = 0; k < calls.size(); ++k) {
				const Call &K = calls[k];
				uint8_t *buf = (uint8_t*)malloc((size_t)(a + K.n_bytes ? a + K.n_bytes : 1));      /* malloc's blocks start on a 16-byte boundary */
				if (K.n_bytes) memcpy(buf + a, K.data.data(), (size_t)K.n_bytes);
				std::vector<int64_t> off(K.off);
				for (int64_t &o : off) o += a;
				const int64_t bad = emu_markdup_add(h, K.n_rec, buf, off.data(), 1 + (int)((c + a + (int64_t)k) % 5), a & 1);
				free(buf);
				if (bad != K.want_bad) { fprintf(stderr, "case %lld call %zu at residue %d: damaged record %lld (expected %lld)\n", (long long)c, k, a, (long long)bad, (long long)K.want_bad); return 3; }
				++checks;
			}
			uint8_t *dup = (uint8_t*)malloc((size_t)(n_ord ? n_ord : 1));
			uint64_t *stats = (uint64_t*)malloc((size_t)n_stats * 8);
			const int64_t n = emu_markdup_resolve(h, dup, stats);
			const bool same = n == n_ord && (n_ord == 0 || !memcmp(dup, want_dup.data(), (size_t)n_ord)) && !memcmp(stats, want_stats.data(), (size_t)n_stats * 8);
			free(dup); free(stats);
			emu_markdup_destroy(h);
			if (!same) { fprintf(stderr, "case %lld at residue %d: other marks or counters than the oracle's\n", (long long)c, a); return 3; }
			++checks;
		}
	}
	fclose(f);
	printf("ok %ld\n", checks);
	return 0;
}
