// bam_sort_body.hpp -- the per-lane bodies of the coordinate sort of finished BAM records (bam_sort.hip, nabwa_bam_sort*):
//
//   bsort_u32        a little-endian word at any byte address, read byte by byte (a record starts wherever the one before it ended)
//   bsort_key        the sort key of the record at `rec`: NABWA_BAM_SORT_KEY(refID, pos), refID at byte 4 and pos at byte 8
//   bsort_copy_part  lane t of the REC_LANES lanes that copy one record of n bytes from src to dst, both at any byte alignment
//
// The copy: the bytes up to dst's first 16-byte boundary go singly (lane t takes byte t), then whole 16-byte chunks, chunk c by lane
// c mod 16 -- the store is a 16-byte aligned one, the load takes its 16 bytes from wherever the source has them (the hardware reads a
// global dwordx4 at any byte address; the words arrive realigned in the lane's registers) -- and the bytes behind the last whole chunk go
// singly again.  Every load lies in [src, src + n) and every store in [dst, dst + n): no neighbour's byte is read, none is written, so a
// record at the very end of the input buffer and one at the very end of the output buffer are copied like any other.
//
// Compiled for gfx950 by bam_sort.hip and, with NABWA_EMU (tests/emu/, test infrastructure), by g++, so that every address the bodies form
// can be checked under AddressSanitizer without a GPU.  No arrays beyond four words: no scratch.
#pragma once
#include <stdint.h>
#ifdef NABWA_EMU
#include "emu_hip.hpp"
#define BSORT_FN static inline
#else
#include <hip/hip_runtime.h>
#define BSORT_FN __device__ __forceinline__
#endif
#include "rec_body.hpp"        /* REC_LANES, the lanes per record in the gather, and REC_MIN_REC; nothing else of it */
#ifdef NABWA_EMU
#define BSORT_LANES REC_LANES      /* (tests/emu/bam_sort_emu.cpp counts its lanes by this name) */
#endif

BSORT_FN uint32_t bsort_u32(const uint8_t *p)
{
	return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

BSORT_FN uint64_t bsort_key(const uint8_t *rec)
{
	return (uint64_t)bsort_u32(rec + 4) << 32 | (uint32_t)(bsort_u32(rec + 8) + 1u);
}

BSORT_FN void bsort_copy_part(const uint8_t *src, uint8_t *dst, int64_t n, int t)
{
	int64_t head = (int64_t)((16u - ((uint32_t)(uintptr_t)dst & 15u)) & 15u);
	if (head > n) head = n;
	if (t < head) dst[t] = src[t];
	const int64_t n_chunks = (n - head) >> 4;
	for (int64_t c = t; c < n_chunks; c += REC_LANES) {
		uint32_t w[4];
		__builtin_memcpy(w, src + head + 16 * c, 16);
		__builtin_memcpy(__builtin_assume_aligned(dst + head + 16 * c, 16), w, 16);
	}
	const int64_t done = head + 16 * n_chunks;
	if (done + t < n) dst[done + t] = src[done + t];
}
