// tests/emu/dedup_emu.cpp -- TEST INFRASTRUCTURE ONLY.  The bodies of the duplicate-read stage (csrc/dedup_body.hpp) compiled by g++: the
// 16 lanes a read has on the GPU are a loop here, and their exchange (dedup_kernels.hip: an add, an and, over __shfl_xor) a plain sum.
//   as a shared library (tests/dedup_cases.py)     emu_dedup_hash, emu_dedup_hash_batch, emu_dedup_equal
//   with -DDEDUP_EMU_MAIN, a program of its own     the same bodies under -fsanitize=address,undefined on buffers of exactly off[n]
//                                                    bytes whose last read ends where the buffer ends
#define NABWA_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../network-aware-bwa_amd/csrc/dedup_body.hpp"

extern "C" uint64_t emu_dedup_hash(const uint8_t *seq, const uint8_t *rseq, int64_t o, int L)
{
	uint64_t sum = 0;
	for (int t = 0; t < DEDUP_LANES; ++t) sum += dedup_hash_part(seq, rseq, o, L, t);
	return dedup_hash_finish(sum, L);
}

extern "C" void emu_dedup_hash_batch(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, uint64_t *out)
{
	for (int i = 0; i < n; ++i) out[i] = emu_dedup_hash(seq, rseq, off[i], (int)(off[i + 1] - off[i]));
}

/* as dedup_verify_kernel: reads i and f of a batch */
extern "C" int emu_dedup_equal(const uint8_t *seq, const uint8_t *rseq, const int64_t *off, int i, int f)
{
	const int L = (int)(off[i + 1] - off[i]);
	if (L != (int)(off[f + 1] - off[f])) return 0;
	int same = 1;
	for (int t = 0; t < DEDUP_LANES; ++t) same &= dedup_equal_part(seq, rseq, off[i], off[f], L, t) ? 1 : 0;
	return same;
}

#ifdef DEDUP_EMU_MAIN
static uint64_t rng_state = 0x243f6a8885a308d3ULL;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(rng_state >> 33); }

int main()
{
	int n_cases = 0, n_failed = 0;
	/* the batch: `lead` junk reads of lengths that move the later starts over every byte phase, a read, its copy, its copy with the last
	 * byte of rseq changed, and the same three once more at the very end: the last read's length is `tail`, 0..33, and it ends where
	 * the buffers end.  Each buffer is its own heap block of exactly off[n] bytes. */
	for (int tail = 0; tail <= 33; ++tail)
		for (int lead = 0; lead < 17; ++lead) {
			const int n = 7;
			const int lens[n] = { lead, 40 + (int)(rnd() % 30), tail, tail, tail, tail, tail };
			int64_t off[n + 1]; off[0] = 0;
			for (int i = 0; i < n; ++i) off[i + 1] = off[i] + lens[i];
			uint8_t *seq = (uint8_t*)malloc((size_t)off[n]), *rseq = (uint8_t*)malloc((size_t)off[n]);
			for (int64_t k = 0; k < off[n]; ++k) { seq[k] = (uint8_t)(rnd() % 5); rseq[k] = (uint8_t)(rnd() % 5); }
			for (int i = 3; i < n; ++i)
				for (int k = 0; k < tail; ++k) { seq[off[i] + k] = seq[off[2] + k]; rseq[off[i] + k] = rseq[off[2] + k]; }
			if (tail) { rseq[off[4] + tail - 1] ^= 1; seq[off[5]] ^= 2; }      /* read 4: last byte of rseq, read 5: first byte of seq */
			uint64_t h[n];
			emu_dedup_hash_batch(n, seq, rseq, off, h);
			++n_cases;
			bool ok = h[3] == h[2] && h[6] == h[2] && emu_dedup_equal(seq, rseq, off, 3, 2) && emu_dedup_equal(seq, rseq, off, 6, 2) && emu_dedup_equal(seq, rseq, off, 6, 6);
			if (tail) ok = ok && h[4] != h[2] && h[5] != h[2] && !emu_dedup_equal(seq, rseq, off, 4, 2) && !emu_dedup_equal(seq, rseq, off, 5, 2) && !emu_dedup_equal(seq, rseq, off, 6, 5);
			ok = ok && !emu_dedup_equal(seq, rseq, off, 1, 6) && (lens[0] == tail || !emu_dedup_equal(seq, rseq, off, 0, 6));
			if (!ok) { ++n_failed; printf("tail %d lead %d: wrong\n", tail, lead); }
			free(seq); free(rseq);
		}
	printf("%d cases, %d failed\n", n_cases, n_failed);
	return n_failed ? 1 : 0;
}
#endif
