// tests/emu/damage_main.cpp -- TEST INFRASTRUCTURE ONLY.  The bodies of the damage profile (csrc/damage_body.hpp, through damage_emu.cpp) as a
// stand-alone program for AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_damage_asan.py):
//
//     damage_main CASES
//
// CASES is the file tests/damage_cases.py:write_case_file writes: the reference, then per case its options, records, the table the Python oracle
// expects and the damaged record it expects (-1: none).  The .pac lies in a heap buffer of exactly l_pac / 4 + 1 bytes.  Every case runs twice:
// as one call on a heap buffer that ends with the last record's last byte, and record by record, each record alone in a heap buffer that ends
// with its last byte (at every start alignment in turn), the totals adding up.  Both must give the expected table, or name the expected record.
// Exit 0 and "ok <checks>" on stdout, or 3 with the case that failed on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

extern "C" int64_t emu_damage_run(int64_t n_rec, const uint8_t *in, const int64_t *off, const uint8_t *pac, int64_t l_pac, int n_holes, const int64_t *hole_off,
								  const int32_t *hole_len, int n_contigs, const int64_t *contig_off, int n_pos, int min_mapq, uint32_t exclude_flags,
								  uint32_t require_flags, int n_blocks, uint64_t *totals);

static FILE *f;
static void get(void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "the case file is cut short\n"); exit(2); } }
static int64_t get64() { int64_t v; get(&v, 8); return v; }

int main(int argc, char **argv)
{
	if (argc != 2 || !(f = fopen(argv[1], "rb"))) { fprintf(stderr, "usage: damage_main CASES\n"); return 2; }
	const int64_t l_pac = get64(), n_holes = get64(), n_contigs = get64();
	uint8_t *pac = (uint8_t*)malloc((size_t)(l_pac / 4 + 1));
	get(pac, (size_t)(l_pac / 4 + 1));
	std::vector<int64_t> hole_off((size_t)n_holes), contig_off((size_t)n_contigs);
	std::vector<int32_t> hole_len((size_t)n_holes);
	for (int64_t i = 0; i < n_holes; ++i) { hole_off[(size_t)i] = get64(); hole_len[(size_t)i] = (int32_t)get64(); }
	get(contig_off.data(), (size_t)n_contigs * 8);
	const int64_t n_cases = get64();
	long checks = 0;
	for (int64_t c = 0; c < n_cases; ++c) {
		const int64_t n_rec = get64(), n_bytes = get64(), n_pos = get64(), min_mapq = get64(), excl = get64(), req = get64(), want_bad = get64(), n_words = get64();
		std::vector<int64_t> off((size_t)n_rec + 1);
		get(off.data(), off.size() * 8);
		uint8_t *data = (uint8_t*)malloc((size_t)(n_bytes ? n_bytes : 1));      /* ends with the last record's last byte */
		get(data, (size_t)n_bytes);
		std::vector<uint64_t> want((size_t)n_words), got((size_t)n_words, 0), zero((size_t)n_words, 0);
		get(want.data(), want.size() * 8);
		auto run = [&](int64_t n, const uint8_t *in, const int64_t *o, int n_blocks) {
			return emu_damage_run(n, in, o, pac, l_pac, (int)n_holes, hole_off.data(), hole_len.data(), (int)n_contigs, contig_off.data(), (int)n_pos, (int)min_mapq,
								  (uint32_t)excl, (uint32_t)req, n_blocks, got.data());
		};
		/* the whole case as one call */
		const int64_t bad = run(n_rec, data, off.data(), 1 + (int)(c % 5));
		if (bad != want_bad || got != (want_bad < 0 ? want : zero)) { fprintf(stderr, "case %lld as one call: damaged record %lld (expected %lld), or another table\n", (long long)c, (long long)bad, (long long)want_bad); return 3; }
		++checks;
		/* record by record */
		std::fill(got.begin(), got.end(), 0);
		int64_t first_bad = -1;
		for (int64_t i = 0; i < n_rec; ++i) {
			const int64_t size = off[(size_t)i + 1] - off[(size_t)i], a = (i + c) % 16;
			uint8_t *buf = (uint8_t*)malloc((size_t)(a + size));                 /* malloc's blocks start on a 16-byte boundary: the record at residue a */
			memcpy(buf + a, data + off[(size_t)i], (size_t)size);
			const int64_t o2[2] = { a, a + size };
			const int64_t b = run(1, buf, o2, 1);
			free(buf);
			if (b >= 0 && first_bad < 0) first_bad = i;
			if (b < -1 || b > 0) { fprintf(stderr, "case %lld record %lld alone: %lld\n", (long long)c, (long long)i, (long long)b); return 3; }
			++checks;
		}
		if (first_bad != want_bad || (want_bad < 0 && got != want)) { fprintf(stderr, "case %lld record by record: damaged record %lld (expected %lld), or another table\n", (long long)c, (long long)first_bad, (long long)want_bad); return 3; }
		++checks;
		free(data);
	}
	free(pac);
	fclose(f);
	printf("ok %ld\n", checks);
	return 0;
}
