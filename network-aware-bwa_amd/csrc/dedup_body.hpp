// dedup_body.hpp -- the bodies of the duplicate-read stage (dedup_kernels.hip, NABWA_DEDUP=1): a 64-bit hash of a read over its length and
// the bytes of both strands, and the exact comparison of two reads that decides whether they merge.
//
//   dedup_hash_part    lane t of the 16 lanes a read has: the sum, over the 16-byte chunks t, t + 16, ... of both strands, of a mix of the
//                      chunk's bytes with (chunk index, strand).  The group adds its lanes' sums.
//   dedup_hash_finish  the group's sum and the length -> the hash
//   dedup_equal_part   lane t's chunks of two reads of one length, byte for byte on both strands
//
// Why the sum: mix64 is a bijection of 64-bit words, so two reads of one length that differ in bytes of ONE 8-byte half of one chunk have
// different sums whatever the other bytes are -- exactly one term changes.  Reads that share every byte and differ in length by one within
// a chunk whose new byte is the pad value differ in the last step, which is a bijection of the length for a fixed sum.  Everything else is
// a hash: unequal reads may collide, and the stage compares the bytes before it merges (dedup_equal_part), so a collision costs a merge,
// never a row.
//
// No body touches a byte at or beyond off + L of either strand: whole chunks are 16-byte loads, the last, partial chunk goes byte by byte.
// Compiled for gfx950 by dedup_kernels.hip and, with NABWA_EMU (tests/emu/, test infrastructure), by g++, so that every address the bodies
// form can be checked under AddressSanitizer and the hash's properties without a GPU.  No arrays of their own beyond two words: no scratch.
#pragma once
#include <stdint.h>
#ifdef NABWA_EMU
#include "emu_hip.hpp"
#define DEDUP_FN static inline
#else
#include <hip/hip_runtime.h>
#define DEDUP_FN __device__ __forceinline__
#endif

#define DEDUP_LANES 16      /* lanes per read, as pad_reads_kernel (batch_kernels.hip) */

DEDUP_FN uint64_t dedup_mix64(uint64_t x)
{
	x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
	return x;
}

/* the up to 16 bytes of a chunk as two words, the first byte lowest; bytes that do not exist are 0 */
DEDUP_FN void dedup_load_chunk(const uint8_t *src, int have, uint64_t w[2])
{
	w[0] = w[1] = 0;
	if (have >= 16) { __builtin_memcpy(w, src, 16); return; }
#pragma unroll
	for (int k = 0; k < 16; ++k) if (k < have) w[k >> 3] |= (uint64_t)src[k] << (8 * (k & 7));
}

/* o: where the read starts in seq and in rseq, L: its length */
DEDUP_FN uint64_t dedup_hash_part(const uint8_t *seq, const uint8_t *rseq, int64_t o, int L, int t)
{
	uint64_t sum = 0;
	const int NC = (L + 15) >> 4;
	for (int c = t; c < NC; c += DEDUP_LANES) {
#pragma unroll
		for (int st = 0; st < 2; ++st) {
			uint64_t w[2];
			dedup_load_chunk((st ? rseq : seq) + o + 16 * (int64_t)c, L - 16 * c, w);
			const uint64_t where = (uint64_t)(4 * c + 2 * st + 1);      /* odd, one per (chunk, strand, half) with where + 1 */
			sum += dedup_mix64(w[0] ^ where * 0x9e3779b97f4a7c15ULL) + dedup_mix64(w[1] ^ (where + 1) * 0xd6e8feb86659fd93ULL);
		}
	}
	return sum;
}

DEDUP_FN uint64_t dedup_hash_finish(uint64_t sum, int L)
{
	return dedup_mix64(sum ^ dedup_mix64(((uint64_t)(uint32_t)L + 1) * 0xa0761d6478bd642fULL));
}

/* reads of one length L that start at oa and ob: do lane t's chunks agree on both strands? */
DEDUP_FN bool dedup_equal_part(const uint8_t *seq, const uint8_t *rseq, int64_t oa, int64_t ob, int L, int t)
{
	bool same = true;
	const int NC = (L + 15) >> 4;
	for (int c = t; c < NC; c += DEDUP_LANES) {
#pragma unroll
		for (int st = 0; st < 2; ++st) {
			const uint8_t *base = st ? rseq : seq;
			uint64_t a[2], b[2];
			dedup_load_chunk(base + oa + 16 * (int64_t)c, L - 16 * c, a);
			dedup_load_chunk(base + ob + 16 * (int64_t)c, L - 16 * c, b);
			same = same && a[0] == b[0] && a[1] == b[1];
		}
	}
	return same;
}
