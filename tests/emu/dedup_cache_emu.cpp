// tests/emu/dedup_cache_emu.cpp -- TEST INFRASTRUCTURE ONLY.  The bodies of the cross-batch read cache (csrc/dedup_cache_body.hpp; NABWA_DEDUP_CACHE)
// compiled by g++: the 16 lanes a read has on the GPU are a loop here, their exchange an and, and the atomics plain reads and writes.
//   as a shared library (tests/test_dedup_cache_emu.py)   emu_dcache_* below
//   with -DDCACHE_EMU_MAIN, a program of its own           lookup and insert under -fsanitize=address,undefined on heap blocks of exactly the
//                                                           bytes the table, the arena and the reads have: the last entry ends where the arena ends
#define NABWA_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../network-aware-bwa_amd/csrc/dedup_cache_body.hpp"

static uint64_t hash_of(const uint8_t *seq, const uint8_t *rseq, int64_t o, int L)
{
	uint64_t sum = 0;
	for (int t = 0; t < DEDUP_LANES; ++t) sum += dedup_hash_part(seq, rseq, o, L, t);
	return dedup_hash_finish(sum, L);
}

extern "C" int emu_dcache_probes(void) { return DCACHE_PROBES; }
extern "C" uint32_t emu_dcache_entry_size(int L, int n_aln) { return dcache_entry_size(L, n_aln); }
extern "C" uint64_t emu_dcache_slot_index(uint64_t hash, uint64_t mask, uint32_t n_slots, int p) { return dcache_slot_index(hash, mask, n_slots, p); }
extern "C" uint64_t emu_dcache_hash(const uint8_t *seq, const uint8_t *rseq, int64_t o, int L) { return hash_of(seq, rseq, o, L); }

/* as dcache_insert_kernel does for one read whose search is complete: -> the entry's arena offset, or -1 (not entered; ctr says why) */
extern "C" long long emu_dcache_insert(unsigned long long *slots, uint32_t n_slots, uint8_t *arena, uint64_t arena_bytes, unsigned long long *ctr, uint64_t mask,
									   const uint8_t *seq, const uint8_t *rseq, int64_t o, int L, int md, int mg, int n_aln, int max_ent, const uint4 *rows, int row_cap)
{
	const uint64_t h = hash_of(seq, rseq, o, L);
	int64_t slot = -1;
	const long long where = dcache_insert_claim(slots, n_slots, h, mask, ctr, arena_bytes, L, n_aln, n_aln >= 0 && n_aln <= row_cap, &slot);
	if (where < 0) return -1;
	for (int t = 0; t < DEDUP_LANES; ++t) dcache_write_part(arena + where, h, seq, rseq, o, L, md, mg, n_aln, max_ent, rows, t);
	dcache_store(slots + slot, dcache_slot_value(h, (uint64_t)where >> 4));
	return where;
}

/* as dcache_lookup_kernel does for one read: -> the entry's arena offset, or -1; *n_cand = the candidates it compared */
extern "C" long long emu_dcache_lookup(const unsigned long long *slots, uint32_t n_slots, const uint8_t *arena, uint64_t mask,
									   const uint8_t *seq, const uint8_t *rseq, int64_t o, int L, int md, int mg, int *n_cand)
{
	const uint64_t h = hash_of(seq, rseq, o, L);
	int p = 0, nc = 0;
	long long hit = -1;
	for (;;) {
		const uint64_t cand = dcache_next_candidate(slots, n_slots, h, mask, &p);
		if (!cand) break;
		++nc;
		int same = 1;
		for (int t = 0; t < DEDUP_LANES; ++t) same &= dcache_match_part(arena + (cand - 1) * 16, h, seq, rseq, o, L, md, mg, t) ? 1 : 0;
		if (same) { hit = (long long)(cand - 1) * 16; break; }
	}
	if (n_cand) *n_cand = nc;
	return hit;
}

/* what the read-back takes from the entry at arena + where */
extern "C" int emu_dcache_entry(const uint8_t *arena, long long where, int32_t *n_aln, int32_t *max_ent, uint4 *rows_out)
{
	const uint8_t *e = arena + where;
	*n_aln = dcache_n_aln(e); *max_ent = dcache_max_ent(e);
	const uint4 *r = dcache_rows(e);
	for (int j = 0; j < *n_aln; ++j) rows_out[j] = r[j];
	return 0;
}

#ifdef DCACHE_EMU_MAIN
static uint64_t rng_state = 0x13198a2e03707344ULL;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(rng_state >> 33); }

int main()
{
	int n_cases = 0, n_failed = 0;
	/* one cache per case: a junk read of `lead` bytes in front moves the reads over every byte phase; three reads of length `len` (0..40, 63..65,
	 * 257 in turn) with 0, 1 and 3 rows.  The arena is a heap block of exactly the three entries' bytes, the table of exactly its slots, seq and
	 * rseq of exactly off[n] bytes: the last read and the last entry end where their blocks end.  Then: every read is found with its rows; a read
	 * with one byte of rseq changed, its prefix and the read under another max_gapo are not; a fourth insert finds the arena full. */
	const int lens[] = { 0, 1, 2, 7, 8, 9, 15, 16, 17, 23, 31, 32, 33, 40, 63, 64, 65, 257 };
	for (int len : lens)
		for (int lead = 0; lead < 17; ++lead) {
			const int n = 4, L[n] = { lead, len, len + 1, len ? len : 2 }, na[n] = { 0, 0, 1, 3 };      /* (two empty reads would be one read) */
			int64_t off[n + 1]; off[0] = 0;
			for (int i = 0; i < n; ++i) off[i + 1] = off[i] + L[i];
			uint8_t *seq = (uint8_t*)malloc((size_t)off[n] ? (size_t)off[n] : 1), *rseq = (uint8_t*)malloc((size_t)off[n] ? (size_t)off[n] : 1);
			for (int64_t k = 0; k < off[n]; ++k) { seq[k] = (uint8_t)(rnd() % 5); rseq[k] = (uint8_t)(rnd() % 5); }
			if (len) seq[off[3]] = (uint8_t)(seq[off[1]] ^ 1);      /* reads 1 and 3 have one length and differ */
			uint64_t arena_bytes = 0;
			for (int i = 1; i < n; ++i) arena_bytes += dcache_entry_size(L[i], na[i]);
			const uint32_t n_slots = 8;
			unsigned long long *slots = (unsigned long long*)calloc(n_slots, 8), ctr[DC_WORDS] = { 0 };
			uint8_t *arena = (uint8_t*)malloc(arena_bytes);
			uint4 rows[3];
			for (int j = 0; j < 3; ++j) rows[j] = make_uint4(rnd(), rnd(), rnd(), rnd());
			bool ok = true;
			long long where[n] = { -1, -1, -1, -1 };
			for (int i = 1; i < n; ++i) {
				where[i] = emu_dcache_insert(slots, n_slots, arena, arena_bytes, ctr, ~0ull, seq, rseq, off[i], L[i], 3, 1, na[i], 100 + i, rows, 64);
				ok = ok && where[i] >= 0 && where[i] % 16 == 0;
			}
			ok = ok && ctr[DC_USED] == arena_bytes && ctr[DC_ENTRIES] == 3 && ctr[DC_FULL] == 0;
			ok = ok && emu_dcache_insert(slots, n_slots, arena, arena_bytes, ctr, ~0ull, seq, rseq, off[0], L[0], 3, 1, 0, 1, rows, 64) == -1 && ctr[DC_FULL] == 1 && ctr[DC_USED] == arena_bytes;
			for (int i = 1; i < n; ++i) {
				int32_t a = -1, m = -1; uint4 got[3];
				const long long w = emu_dcache_lookup(slots, n_slots, arena, ~0ull, seq, rseq, off[i], L[i], 3, 1, 0);
				ok = ok && w == where[i];
				if (w >= 0) { emu_dcache_entry(arena, w, &a, &m, got); ok = ok && a == na[i] && m == 100 + i && memcmp(got, rows, 16 * (size_t)na[i]) == 0; }
				ok = ok && emu_dcache_lookup(slots, n_slots, arena, ~0ull, seq, rseq, off[i], L[i], 3, 2, 0) == -1;      /* another max_gapo */
				ok = ok && emu_dcache_lookup(slots, n_slots, arena, ~0ull, seq, rseq, off[i], L[i], 2, 1, 0) == -1;      /* another max_diff */
				if (L[i]) {
					if (len >= 2) ok = ok && emu_dcache_lookup(slots, n_slots, arena, ~0ull, seq, rseq, off[i], L[i] - 1, 3, 1, 0) == -1;      /* its prefix (of the shortest reads it may be another read) */
					rseq[off[i] + L[i] - 1] ^= 2;
					ok = ok && emu_dcache_lookup(slots, n_slots, arena, ~0ull, seq, rseq, off[i], L[i], 3, 1, 0) == -1;          /* the last byte of rseq */
					rseq[off[i] + L[i] - 1] ^= 2;
				}
			}
			++n_cases;
			if (!ok) { ++n_failed; printf("len %d lead %d: wrong\n", len, lead); }
			free(seq); free(rseq); free(slots); free(arena);
		}
	printf("%d cases, %d failed\n", n_cases, n_failed);
	return n_failed ? 1 : 0;
}
#endif
