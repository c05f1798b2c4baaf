// bai_body.hpp -- the bodies of the BAM index (.bai, SAM specification 5.2) of finished, coordinate-sorted BAM records (bai_kernels.hip,
// nabwa_bai*; the semantics: include/nabwa.h):
//
//   bai_record_part  lane t of the REC_LANES lanes that take one record: its fields checked, its key against the record's in front of it,
//                    CIGAR operations t, t + 16, ... summed into the group's word of LDS (the cross-lane sum of the reference length)
//   bai_block        one workgroup of the persistent grid: REC_GROUPS records per trip; lane 0 of a group writes the record's tuple
//   bai_ref_block    a workgroup of REC_BLOCK tuples in stream order: both virtual offsets of each (binary search in the block table), and
//                    per reference the highest window, the records with flag 0x4, the first and the last ordinal -- one atomic per run of
//                    equal references in the workgroup, not one per record
//   bai_head_one     position j of the tuples sorted by (tid, bin): does a bin start here, does a chunk
//   bai_place_one    the same position once the heads are scanned: where its bin's chunks start, where its reference's bins and chunks do
//   bai_refsize_one  reference r: the bytes of its part of the file and its windows
//   bai_lin_one      tuple o: its virtual start into every window it touches (64-bit atomic minimum; the table lies reversed)
//   BaiNextTouched   the scan operator of the backward fill: an untouched window takes the next touched one's value
//   bai_write_ref, bai_write_tuple, bai_write_lin    the file: header, bin counts, pseudo-bins and trailer; bins and chunks; windows
//
// A record starts at any byte, so nothing in it is aligned; the hardware reads a global word at any byte address.  No byte outside
// [rec, rec + size) is read, except bytes 4 .. 11 of the record in front of it.  The file is written as 32-bit words: every field of a .bai
// lies at a multiple of 4.
//
// A tuple is four 64-bit words, one array each, indexed by the record's ordinal (records without a reference get a slot too: in coordinate
// order they are the last, so the placed ones are the first n):
//   key  tid << 16 | bin                 (BAI_KEY_NONE for a record without a reference)
//   be   end << 32 | beg
//   us   where the record starts in the uncompressed stream
//   ue   where it ends, and flag 0x4 in bit 63
//
// Compiled for gfx950 by bai_kernels.hip and, with NABWA_EMU (tests/emu/, test infrastructure), by g++: there the threads of a workgroup
// run one after the other between the barriers, so that every address the bodies form can be checked under AddressSanitizer without a GPU.
// No arrays: no scratch.
#pragma once
#include <stdint.h>
#include "../../include/nabwa.h"
#include "rec_body.hpp"        /* the macro layer, REC_LANES ... REC_MIN_REC, rec_u32, rec_op_ref, REC_HEAD */
#ifdef NABWA_EMU
#define BAI_MEMBER inline
#define BAI_GROUPS REC_GROUPS      /* (tests/emu/bai_emu.cpp sizes its arrays by these names) */
#define BAI_BLOCK  REC_BLOCK
#else
#define BAI_MEMBER __host__ __device__ __forceinline__
#endif

#define BAI_MAX_END    ((int64_t)1 << 29)       /* the last coordinate a .bai addresses */
#define BAI_PSEUDO_BIN 37450u
#define BAI_KEY_NONE   (~(uint64_t)0)
#define BAI_UNMAPPED   ((uint64_t)1 << 63)
#define BAI_UNTOUCHED  (~(unsigned long long)0)
#define BAI_OK  0
#define BAI_BAD 1
/* a group's state word in LDS */
#define BAI_ST_IDLE 0u
#define BAI_ST_OK   1u
#define BAI_ST_BAD  2u

/* what an add works on.  off[] are the caller's offsets, base = off[0]: record i lies at in + (off[i] - base) and at stream_off +
 * (off[i] - base) of the uncompressed stream.  last_key: the key of the record in front of the call's first (0 where there is none).
 * key, be, us, ue: the arena at the call's first ordinal.  cnt[0]: the lowest damaged record (0xffffffff before), cnt[1]: the call's records
 * without a reference (0 before) */
struct BaiParams {
	const uint8_t *in; const int64_t *off; int64_t base, stream_off; uint64_t last_key; int32_t n_rec, n_ref;
	uint64_t *key, *be; int64_t *us; uint64_t *ue; unsigned int *cnt;
};
/* what a finish works on.  n: the placed records; the block table has n_blk + 1 entries.  Per reference: maxwin (-1 before), unm (0 before),
 * o0 / o1 the first and last ordinal, b0 / b1 and c0 / c1 the first and one past the last bin and chunk (counted over all references).
 * skey, sidx: the keys sorted and the ordinals beside them; heads: bin head << 32 | chunk head, sc: its inclusive sum; bin_c0[b]: the first
 * chunk of bin b (n + 1 words).  ref_size -> ref_off and ref_nintv -> lin_off by an exclusive sum over n_ref + 1 entries.  lin: the n_lin
 * windows of all references back to back, reversed.  out: the file */
struct BaiFin {
	int64_t n, n_blk, n_lin; int32_t n_ref; uint64_t n_no_coor;
	const uint64_t *key, *be; const int64_t *us; const uint64_t *ue;
	const int64_t *blk_u, *blk_c;
	uint64_t *vb, *ve;
	int *maxwin; unsigned int *unm, *o0, *o1, *b0, *b1, *c0, *c1;
	const uint64_t *skey; const uint32_t *sidx;
	unsigned long long *heads, *sc; uint32_t *bin_c0;
	unsigned long long *ref_size, *ref_nintv, *ref_off, *lin_off;
	unsigned long long *lin;
	uint32_t *out;
};

/* reg2bin of the specification, for [beg, end) with 0 <= beg < end <= 2^29 */
REC_HD uint32_t bai_reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}
/* a record's end from its fields and the reference length of its CIGAR */
REC_HD int64_t bai_end(int32_t pos, uint32_t flag, uint32_t n_cig, uint64_t ref_len)
{
	return (flag & 4u) || n_cig == 0 || ref_len == 0 ? (int64_t)pos + 1 : (int64_t)pos + (int64_t)ref_len;
}

/* lane t of the group of record i, `rec` of `size` >= REC_MIN_REC bytes; prev: the record in front of it, or null for the call's first.
 * sum: the group's word of LDS (zero).  BAI_BAD for a record that is damaged whatever its CIGAR says (every lane says so, before any lane
 * has touched sum), else BAI_OK */
REC_FN int bai_record_part(const BaiParams &P, const uint8_t *rec, int64_t size, const uint8_t *prev, int t, unsigned long long *sum)
{
	REC_HEAD(rec, size, BAI_BAD);
	if (ref_id >= P.n_ref || (ref_id >= 0 && pos < 0)) return BAI_BAD;
	const uint64_t before = prev ? NABWA_BAM_SORT_KEY((int32_t)rec_u32(prev + 4), (int32_t)rec_u32(prev + 8)) : P.last_key;
	if (NABWA_BAM_SORT_KEY(ref_id, pos) < before) return BAI_BAD;
	if (ref_id >= 0 && !(flag & 4u)) {
		const uint8_t *cig = rec + REC_MIN_REC + l_name;
		uint64_t s = 0;                         /* (operations of 28 bits, at most 65535 of them: no sum leaves 64 bits) */
		for (uint32_t c = (uint32_t)t; c < n_cig; c += REC_LANES) { const uint32_t w = rec_u32(cig + 4 * c); if (rec_op_ref(w & 15u)) s += w >> 4; }
		if (s) REC_ADD64(sum, (unsigned long long)s);
	}
	return BAI_OK;
}

/* workgroup `block` of `n_blocks`: trips block, block + n_blocks, ... of REC_GROUPS records each.  sum, state: REC_GROUPS words of LDS each */
REC_FN void bai_block(const BaiParams &P, unsigned long long *sum, uint32_t *state, int block, int n_blocks)
{
	REC_THREADS { if (tid < REC_GROUPS) { sum[tid] = 0; state[tid] = BAI_ST_IDLE; } }
	REC_SYNC;
	for (int64_t first = (int64_t)block * REC_GROUPS; first < P.n_rec; first += (int64_t)n_blocks * REC_GROUPS) {
		REC_THREADS {
			const int g = tid / REC_LANES, t = tid % REC_LANES;
			const int64_t i = first + g;
			if (i < P.n_rec) {
				const int64_t o = P.off[i];
				const int r = bai_record_part(P, P.in + (o - P.base), P.off[i + 1] - o, i ? P.in + (P.off[i - 1] - P.base) : (const uint8_t*)0, t, sum + g);
				if (t == 0) { state[g] = r == BAI_OK ? BAI_ST_OK : BAI_ST_BAD; if (r != BAI_OK) REC_MIN32(P.cnt, (unsigned int)i); }
			}
		}
		REC_SYNC;
		REC_THREADS {                                   /* the group's sum is whole: the record's end, bin and tuple, and the words as they were */
			const int g = tid / REC_LANES;
			const int64_t i = first + g;
			if (tid % REC_LANES == 0 && i < P.n_rec) {
				if (state[g] == BAI_ST_OK) {
					const int64_t o = P.off[i];
					const uint8_t *rec = P.in + (o - P.base);
					REC_FIELDS(rec);                    /* (it has passed REC_HEAD: the fields alone) */
					const int64_t end = bai_end(pos, flag, n_cig, sum[g]);
					const int64_t us = P.stream_off + (o - P.base);
					if (ref_id < 0) { P.key[i] = BAI_KEY_NONE; P.be[i] = 0; REC_ADD32(P.cnt + 1, 1u); }
					else if (end > BAI_MAX_END) REC_MIN32(P.cnt, (unsigned int)i);
					else { P.key[i] = (uint64_t)(uint32_t)ref_id << 16 | bai_reg2bin(pos, end); P.be[i] = (uint64_t)end << 32 | (uint32_t)pos; }
					P.us[i] = us;
					P.ue[i] = (uint64_t)(us + (P.off[i + 1] - o)) | ((flag & 4u) ? BAI_UNMAPPED : 0);
				}
				sum[g] = 0; state[g] = BAI_ST_IDLE;
			}
		}
		REC_SYNC;
	}
}

/* the virtual offset of stream offset u, blk_u[0] <= u <= blk_u[n_blk]: the last block that starts at or before u */
REC_FN uint64_t bai_voff(const BaiFin &F, int64_t u)
{
	int64_t lo = 0, hi = F.n_blk + 1;
	while (hi - lo > 1) { const int64_t mid = lo + (hi - lo) / 2; if (F.blk_u[mid] <= u) lo = mid; else hi = mid; }
	return (uint64_t)F.blk_c[lo] << 16 | (uint64_t)(u - F.blk_u[lo]);
}

/* workgroup `block`: tuples block * REC_BLOCK ... in stream order.  l_tid, l_win, l_unm: REC_BLOCK words of LDS each */
REC_FN void bai_ref_block(const BaiFin &F, int *l_tid, int *l_win, unsigned int *l_unm, int64_t block)
{
	REC_THREADS {
		const int64_t o = block * REC_BLOCK + tid;
		l_tid[tid] = -1;
		if (o < F.n) {
			const uint64_t ue = F.ue[o];
			F.vb[o] = bai_voff(F, F.us[o]);
			F.ve[o] = bai_voff(F, (int64_t)(ue & ~BAI_UNMAPPED));
			l_tid[tid] = (int)(F.key[o] >> 16);
			l_win[tid] = (int)(((F.be[o] >> 32) - 1) >> 14);
			l_unm[tid] = (unsigned int)(ue >> 63);
		}
	}
	REC_SYNC;
	REC_THREADS {
		const int64_t o = block * REC_BLOCK + tid;
		const int r = l_tid[tid];
		if (r >= 0 && (tid == 0 || l_tid[tid - 1] != r)) {     /* the first of a run of one reference in this workgroup: the run's maximum and count */
			int win = l_win[tid]; unsigned int unm = l_unm[tid];
			int k = tid + 1;
			for (; k < REC_BLOCK && l_tid[k] == r; ++k) { win = l_win[k] > win ? l_win[k] : win; unm += l_unm[k]; }
			REC_MAX32(F.maxwin + r, win);
			if (unm) REC_ADD32(F.unm + r, unm);
			if (o == 0 || (int)(F.key[o - 1] >> 16) != r) F.o0[r] = (unsigned int)o;
			const int64_t last = o + (k - tid) - 1;
			if (last == F.n - 1 || (int)(F.key[last + 1] >> 16) != r) F.o1[r] = (unsigned int)last;
		}
	}
}

REC_FN void bai_head_one(const BaiFin &F, int64_t j)
{
	const bool hb = j == 0 || F.skey[j - 1] != F.skey[j];
	const bool hc = hb || (F.ve[F.sidx[j - 1]] >> 16) != (F.vb[F.sidx[j]] >> 16);
	F.heads[j] = (unsigned long long)hb << 32 | (unsigned long long)hc;
}

REC_FN void bai_place_one(const BaiFin &F, int64_t j)
{
	const unsigned long long sc = F.sc[j];
	const unsigned int b = (unsigned int)(sc >> 32) - 1, c = (unsigned int)sc - 1;
	const uint64_t k = F.skey[j];
	const uint64_t r = k >> 16;
	if (j == 0 || F.skey[j - 1] != k) F.bin_c0[b] = c;
	if (j == 0 || F.skey[j - 1] >> 16 != r) { F.b0[r] = b; F.c0[r] = c; }
	if (j == F.n - 1 || F.skey[j + 1] >> 16 != r) { F.b1[r] = b + 1; F.c1[r] = c + 1; }
	if (j == F.n - 1) F.bin_c0[b + 1] = c + 1;
}

/* reference r of n_ref + 1: the last is the end of both sums */
REC_FN void bai_refsize_one(const BaiFin &F, int64_t r)
{
	unsigned long long size = 0, nintv = 0;
	if (r < F.n_ref) {
		size = 8;                                       /* n_bin, n_intv */
		if (F.maxwin[r] >= 0) {
			nintv = (unsigned long long)F.maxwin[r] + 1;
			size += 8ull * (F.b1[r] - F.b0[r]) + 16ull * (F.c1[r] - F.c0[r]) + 40 + 8 * nintv;
		}
	}
	F.ref_size[r] = size; F.ref_nintv[r] = nintv;
}

REC_FN void bai_lin_one(const BaiFin &F, int64_t o)
{
	const uint64_t be = F.be[o];
	const int64_t beg = (int64_t)(uint32_t)be, end = (int64_t)(be >> 32);
	const unsigned long long base = F.lin_off[F.key[o] >> 16], v = F.vb[o];
	for (int64_t w = beg >> 14; w <= (end - 1) >> 14; ++w) REC_MIN64(F.lin + (F.n_lin - 1 - (int64_t)(base + (unsigned long long)w)), v);
}

/* over the reversed table, front to back: an untouched window takes what the window before it (the next one of the file) came to.  The
 * last window of a reference is touched, so nothing crosses from one reference into another */
struct BaiNextTouched {
	BAI_MEMBER unsigned long long operator()(unsigned long long a, unsigned long long b) const { return b != BAI_UNTOUCHED ? b : a; }
};

REC_FN void bai_put64(uint32_t *out, unsigned long long at, unsigned long long v) { out[at / 4] = (uint32_t)v; out[at / 4 + 1] = (uint32_t)(v >> 32); }

/* reference r of n_ref + 1: its bin count, its pseudo-bin, its window count; the last writes the header and the trailer */
REC_FN void bai_write_ref(const BaiFin &F, int64_t r)
{
	if (r == F.n_ref) {
		F.out[0] = 0x01494142u; F.out[1] = (uint32_t)F.n_ref;       /* "BAI\1" */
		bai_put64(F.out, 8 + F.ref_off[r], F.n_no_coor);
		return;
	}
	unsigned long long at = 8 + F.ref_off[r];
	if (F.maxwin[r] < 0) { F.out[at / 4] = 0; F.out[at / 4 + 1] = 0; return; }
	const unsigned int nb = F.b1[r] - F.b0[r], nc = F.c1[r] - F.c0[r], n_rec = F.o1[r] - F.o0[r] + 1, unm = F.unm[r];
	F.out[at / 4] = nb + 1;
	at += 4 + 8ull * nb + 16ull * nc;
	F.out[at / 4] = BAI_PSEUDO_BIN; F.out[at / 4 + 1] = 2;
	bai_put64(F.out, at + 8, F.vb[F.o0[r]]); bai_put64(F.out, at + 16, F.ve[F.o1[r]]);
	bai_put64(F.out, at + 24, n_rec - unm); bai_put64(F.out, at + 32, unm);
	F.out[(at + 40) / 4] = (uint32_t)F.maxwin[r] + 1;
}

/* position j of the sorted tuples: the head of a bin writes the bin's number and chunk count, the head of a chunk its start, its last its end */
REC_FN void bai_write_tuple(const BaiFin &F, int64_t j)
{
	const unsigned long long sc = F.sc[j], h = F.heads[j];
	const unsigned int b = (unsigned int)(sc >> 32) - 1, c = (unsigned int)sc - 1;
	const uint64_t k = F.skey[j], r = k >> 16;
	const unsigned long long ref_at = 8 + F.ref_off[r] + 4;
	if (h >> 32) {
		const unsigned long long at = ref_at + 8ull * (b - F.b0[r]) + 16ull * (F.bin_c0[b] - F.c0[r]);
		F.out[at / 4] = (uint32_t)(k & 0xffffu); F.out[at / 4 + 1] = F.bin_c0[b + 1] - F.bin_c0[b];
	}
	const unsigned long long at = ref_at + 8ull * (b - F.b0[r] + 1) + 16ull * (c - F.c0[r]);
	if (h & 1u) bai_put64(F.out, at, F.vb[F.sidx[j]]);
	if (j == F.n - 1 || (unsigned int)F.sc[j + 1] - 1 != c) bai_put64(F.out, at + 8, F.ve[F.sidx[j]]);
}

/* window g of all references' windows back to back */
REC_FN void bai_write_lin(const BaiFin &F, int64_t g)
{
	int64_t lo = 0, hi = F.n_ref;                       /* the last reference whose windows start at or before g */
	while (hi - lo > 1) { const int64_t mid = lo + (hi - lo) / 2; if (F.lin_off[mid] <= (unsigned long long)g) lo = mid; else hi = mid; }
	const int64_t r = lo;
	const unsigned long long at = 8 + F.ref_off[r] + 4 + 8ull * (F.b1[r] - F.b0[r]) + 16ull * (F.c1[r] - F.c0[r]) + 40 + 4 + 8 * ((unsigned long long)g - F.lin_off[r]);
	bai_put64(F.out, at, F.lin[F.n_lin - 1 - g]);
}
