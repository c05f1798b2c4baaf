// tests/emu/bam_sort_main.cpp -- TEST INFRASTRUCTURE ONLY.  The bodies of the BAM coordinate sort (csrc/bam_sort_body.hpp, through
// bam_sort_emu.cpp) as a stand-alone program for AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_bam_sort_asan.py):
//
//     bam_sort_main SIZE [SIZE ...]
//
// Keys: a record of 36 bytes with tid in {-1, 0, 1, 2^31 - 1} x pos in {-1, 0, 1, 2^31 - 2} at every byte offset 0..15 of a heap buffer that
// ends with the record's last byte, against NABWA_BAM_SORT_KEY.  Copies: for every SIZE, every pair of source and destination alignment
// (16 x 16): the source lies in a heap buffer that ends with its last byte, the destination between guard bytes that must survive.
// Exit 0 and "ok <checks>" on stdout, or 3 with the case that failed on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/nabwa.h"

extern "C" uint64_t emu_bsort_key(const uint8_t *rec);
extern "C" void emu_bsort_copy(const uint8_t *src, uint8_t *dst, int64_t n, int backwards);

int main(int argc, char **argv)
{
	long checks = 0;
	const int32_t tids[4] = { -1, 0, 1, 0x7fffffff }, poss[4] = { -1, 0, 1, 0x7ffffffe };
	for (int a = 0; a < 16; ++a)
		for (int32_t tid : tids)
			for (int32_t pos : poss) {
				uint8_t *buf = (uint8_t*)malloc((size_t)a + 36);          /* malloc's blocks start on a 16-byte boundary: the record at residue a */
				memset(buf, 0xee, (size_t)a + 36);
				const uint32_t bs = 32;
				memcpy(buf + a, &bs, 4); memcpy(buf + a + 4, &tid, 4); memcpy(buf + a + 8, &pos, 4);
				const uint64_t got = emu_bsort_key(buf + a), want = NABWA_BAM_SORT_KEY(tid, pos);
				free(buf);
				if (got != want) { fprintf(stderr, "key: offset %d tid %d pos %d: %llx, not %llx\n", a, tid, pos, (unsigned long long)got, (unsigned long long)want); return 3; }
				++checks;
			}
	const int64_t GUARD = 48;
	for (int k = 1; k < argc; ++k) {
		const int64_t n = atoll(argv[k]);
		if (n < 0) { fprintf(stderr, "size %s?\n", argv[k]); return 2; }
		for (int sa = 0; sa < 16; ++sa)
			for (int da = 0; da < 16; ++da) {
				uint8_t *sbuf = (uint8_t*)malloc((size_t)(sa + n));           /* ends with the record's last byte */
				for (int64_t i = 0; i < sa + n; ++i) sbuf[i] = (uint8_t)(i * 131 + n + sa);
				const int64_t dn = (GUARD + da + n + GUARD + 15) / 16 * 16;
				uint8_t *dbuf = (uint8_t*)aligned_alloc(16, (size_t)dn);
				memset(dbuf, 0xa5, (size_t)dn);
				emu_bsort_copy(sbuf + sa, dbuf + GUARD + da, n, (sa + da) & 1);
				bool ok = memcmp(dbuf + GUARD + da, sbuf + sa, (size_t)n) == 0;
				for (int64_t i = 0; i < GUARD + da && ok; ++i) ok = dbuf[i] == 0xa5;
				for (int64_t i = GUARD + da + n; i < dn && ok; ++i) ok = dbuf[i] == 0xa5;
				free(sbuf); free(dbuf);
				if (!ok) { fprintf(stderr, "copy: size %lld source alignment %d destination alignment %d\n", (long long)n, sa, da); return 3; }
				++checks;
			}
	}
	printf("ok %ld\n", checks);
	return 0;
}
