// markdup_body.hpp -- the bodies of duplicate marking of finished BAM records (markdup_kernels.hip, nabwa_markdup*; the
// semantics: include/nabwa.h):
//
//   md_record_part   lane t of the REC_LANES lanes that take one record: its fields, its class, the CIGAR walked for its two unclipped ends,
//                    its piece of the base qualities and of the read-name comparison with the record behind it
//   md_block         one workgroup of the persistent grid: REC_GROUPS records per trip; what a record came to goes into the call's scratch
//   md_emit_record   one record of a call whose records were all sound: mates found from the neighbours' scratch, the record's tuples appended
//                    to the handle's arena, its class counted
//   md_mark_one      position j of the sorted tuples: not the head of its group and not a shadow -> dup[ordinal] (a pair's: both mates)
//   md_prop_one      ordinal o: the unmapped mate of a half pair takes its mate's mark; the marked records are counted
//
// A record starts at any byte, so nothing in it is aligned; the hardware reads a global word at any byte address.  Every lane walks the
// CIGAR itself, as the damage kernel's lanes do (the operations are few and the lanes of a group run in step), so a CIGAR of any length
// needs no exchange.  The qualities and the read name go to the lanes in pieces of 8 bytes, lane t taking pieces t, t + 16, ...: one load
// of 8 bytes, or byte by byte where fewer than 8 remain in the record.  The lanes' partial sums meet in a 64-bit word of LDS per group (the
// lane-group reduction), the name's unequal pieces in a flag word beside it.  No byte outside [rec, rec + size) is read, except the name of
// the record behind it, and of that none outside its own extent.
//
// A tuple is three 64-bit words (the arena holds them as three arrays):
//   hi   the end (refID << 33 | strand << 32 | c5 + 2^30) of a fragment or shadow; of a pair the lower of its two ends
//   lo   0 (NABWA_MARKDUP_ENDS_5P) or c3 + 2^30 (ENDS_BOTH) of a fragment; 0 of a shadow; of a pair the higher of its two ends
//   k3   pair << 63 | ~score << 31 | ordinal: sorted by (hi, lo, k3) a group's fragments come before its pairs, each by falling score, then
//        by rising ordinal.  A shadow is a fragment tuple of score 0xffffffff, which no record reaches (MD_SCORE_CAP).
//
// Compiled for gfx950 by markdup_kernels.hip and, with NABWA_EMU (tests/emu/, test infrastructure), by g++: there the threads of a workgroup
// run one after the other between the barriers, so that every address the bodies form can be checked under AddressSanitizer without a GPU.
// No arrays: no scratch.
#pragma once
#include <stdint.h>
#include "../../include/nabwa.h"
#include "rec_body.hpp"        /* the macro layer, REC_LANES ... REC_MIN_REC, rec_u32, rec_op_read / rec_op_ref, REC_HEAD */
#ifdef NABWA_EMU
#define MD_GROUPS REC_GROUPS       /* (tests/emu/markdup_emu.cpp sizes its arrays by this name) */
#endif

#define MD_SCORE_CAP 0xfffffffeu                /* the highest score of a record or pair; 0xffffffff is a shadow's */
#define MD_COORD_LO  (-((int64_t)1 << 30))      /* a coordinate lies in [MD_COORD_LO, MD_COORD_HI): 32 bits once MD_COORD_LO is taken off */
#define MD_COORD_HI  (((int64_t)1 << 31) + ((int64_t)1 << 30))
#define MD_OK  0
#define MD_BAD 1

/* a record's word of the call's scratch: its class so far, and what the mate search asks of it */
#define MD_CLS_SKIPPED  0u
#define MD_CLS_ALREADY  1u
#define MD_CLS_UNMAPPED 2u
#define MD_CLS_MAPPED   3u
#define MD_CLS_MASK     3u
#define MD_M_FIRST      4u                      /* flags 0x1 and 0x40 without 0x80 */
#define MD_M_SECOND     8u                      /* flags 0x1 and 0x80 without 0x40 */
#define MD_M_PAIRED     16u                     /* flag 0x1 */
#define MD_M_COMPARED   32u                     /* its name was compared with the next record's (workgroup-local) */
#define MD_M_SAME_NEXT  64u                     /* ... and is the same, length and bytes */
/* link[ordinal]: whose mark an unmapped mate takes */
#define MD_LINK_NONE 0
#define MD_LINK_NEXT 1
#define MD_LINK_PREV 2

#define MD_K3_PAIR ((uint64_t)1 << 63)
#define MD_K3(pair, score, ord) (((pair) ? MD_K3_PAIR : 0) | (uint64_t)(uint32_t)~(uint32_t)(score) << 31 | (uint64_t)(ord))
#define MD_K3_ORD(k) ((uint32_t)((k) & 0x7fffffffu))
#define MD_K3_NSCORE(k) ((uint32_t)((k) >> 31))

/* what a call works on.  off[] are the caller's offsets, base = off[0]: record i lies at in + (off[i] - base).  end, c3, score, meta: the
 * call's scratch, a word per record each */
struct MdParams {
	const uint8_t *in; const int64_t *off; int64_t base; int32_t n_rec;
	int32_t min_qual, single_ends; uint32_t exclude_flags;
	uint64_t *end; uint32_t *c3, *score, *meta;
};
/* the handle's arena: n_tup tuples so far (room for two more per record of the call), link[] per ordinal, the class counters; the call's
 * records get the ordinals ord_base, ord_base + 1, ... */
struct MdArena { uint64_t *hi, *lo, *k3; uint8_t *link; unsigned int *n_tup; unsigned long long *stats; uint32_t ord_base; };

/* the `need` (1..8) bytes at p, little-endian, of which `avail` >= need exist; the bytes above them read as 0.  One 8-byte load where 8 exist */
REC_FN uint64_t md_load(const uint8_t *p, int64_t avail, int need)
{
	uint64_t w = 0;
	if (avail >= 8) { __builtin_memcpy(&w, p, 8); return need < 8 ? w & ((((uint64_t)1) << (8 * need)) - 1) : w; }
	for (int b = 0; b < need; ++b) w |= (uint64_t)p[b] << (8 * b);
	return w;
}

/* lane t of the group of record i, `rec` of `size` >= REC_MIN_REC bytes; nsize: the size of record i + 1, which lies at rec + size, or 0 where
 * there is none.  sum, diff, meta: the group's words of LDS (sum and diff zero).  MD_BAD for a damaged record (every lane says so, before any
 * lane has touched sum or diff), else MD_OK */
REC_FN int md_record_part(const MdParams &P, int64_t i, const uint8_t *rec, int64_t size, int64_t nsize, int t, unsigned long long *sum, uint32_t *diff, uint32_t *meta)
{
	REC_HEAD(rec, size, MD_BAD);
	uint32_t m = MD_CLS_MAPPED;
	if (flag & P.exclude_flags) m = MD_CLS_SKIPPED;
	else if (flag & 0x400u) m = MD_CLS_ALREADY;
	else if ((flag & 0x4u) || ref_id < 0 || pos < 0 || n_cig == 0) m = MD_CLS_UNMAPPED;
	const uint8_t *cig = rec + REC_MIN_REC + l_name, *end = rec + size;
	uint64_t e5 = 0; uint32_t c3w = 0;
	if (m == MD_CLS_MAPPED) {
		/* what the CIGAR consumes, and the clips outside its reference span (operations of 28 bits, at most 65535 of them: no sum leaves 64 bits) */
		uint64_t n_read = 0, n_ref = 0, lead = 0, trail = 0;
		bool seen = false;
		for (uint32_t c = 0; c < n_cig; ++c) {
			const uint32_t w = rec_u32(cig + 4 * c), op = w & 15u, len = w >> 4;
			if (rec_op_read(op)) n_read += len;
			if (rec_op_ref(op)) { n_ref += len; seen = true; trail = 0; }
			else if (op == 4 || op == 5) { if (seen) trail += len; else lead += len; }
		}
		if (L > 0 && n_read != L) return MD_BAD;
		const int64_t left = (int64_t)pos - (int64_t)lead, right = (int64_t)pos + (int64_t)n_ref - 1 + (int64_t)trail;
		if (left < MD_COORD_LO || right >= MD_COORD_HI) return MD_BAD;
		const bool rev = (flag & 0x10u) != 0;
		e5 = (uint64_t)(uint32_t)ref_id << 33 | (uint64_t)rev << 32 | (uint32_t)((rev ? right : left) - MD_COORD_LO);
		c3w = (uint32_t)((rev ? left : right) - MD_COORD_LO);
		/* the qualities that count, this lane's pieces */
		const uint8_t *q = cig + 4 * (uint64_t)n_cig + (L + 1) / 2;
		uint64_t s = 0;
		for (int64_t at = 8 * (int64_t)t; at < (int64_t)L; at += 8 * REC_LANES) {
			const int nb = (int64_t)L - at < 8 ? (int)((int64_t)L - at) : 8;
			const uint64_t w = md_load(q + at, end - (q + at), nb);
			for (int b = 0; b < nb; ++b) { const uint32_t v = (uint32_t)(w >> (8 * b)) & 0xffu; if (v != 0xffu && (int32_t)v >= P.min_qual) s += v; }
		}
		if (s) REC_ADD64(sum, (unsigned long long)s);
	}
	if ((flag & 0xC1u) == 0x41u) m |= MD_M_FIRST;
	if ((flag & 0xC1u) == 0x81u) m |= MD_M_SECOND;
	if (flag & 1u) m |= MD_M_PAIRED;
	if ((m & MD_M_FIRST) && (m & MD_CLS_MASK) >= MD_CLS_UNMAPPED && nsize) {      /* a first mate that can have one: is the next record's name this one's? */
		m |= MD_M_COMPARED;
		const uint8_t *nxt = rec + size;
		if ((nxt[12] != l_name || (int64_t)REC_MIN_REC + l_name > nsize)) { if (t == 0) REC_OR(diff, 1u); }
		else
			for (int at = 8 * t; at < (int)l_name; at += 8 * REC_LANES) {
				const int nb = (int)l_name - at < 8 ? (int)l_name - at : 8;
				const uint8_t *a = rec + REC_MIN_REC + at, *b = nxt + REC_MIN_REC + at;
				if (md_load(a, end - a, nb) != md_load(b, nxt + nsize - b, nb)) REC_OR(diff, 1u);
			}
	}
	if (t == 0) { P.end[i] = e5; P.c3[i] = c3w; *meta = m; }
	return MD_OK;
}

/* workgroup `block` of `n_blocks`: trips block, block + n_blocks, ... of REC_GROUPS records each.  sum, diff, meta: REC_GROUPS words of LDS
 * each; *bad: 0xffffffff before the kernel, the lowest damaged record after it */
REC_FN void md_block(const MdParams &P, unsigned long long *sum, uint32_t *diff, uint32_t *meta, unsigned int *bad, int block, int n_blocks)
{
	REC_THREADS { if (tid < REC_GROUPS) { sum[tid] = 0; diff[tid] = 0; meta[tid] = 0; } }
	REC_SYNC;
	for (int64_t first = (int64_t)block * REC_GROUPS; first < P.n_rec; first += (int64_t)n_blocks * REC_GROUPS) {
		REC_THREADS {
			const int g = tid / REC_LANES, t = tid % REC_LANES;
			const int64_t i = first + g;
			if (i < P.n_rec) {
				const int64_t o = P.off[i], o1 = P.off[i + 1];
				const int64_t nsize = i + 1 < P.n_rec ? P.off[i + 2] - o1 : 0;
				if (md_record_part(P, i, P.in + (o - P.base), o1 - o, nsize, t, sum + g, diff + g, meta + g) != MD_OK && t == 0) { REC_MIN32(bad, (unsigned int)i); meta[g] = MD_CLS_SKIPPED; }
			}
		}
		REC_SYNC;
		REC_THREADS {                                    /* the group's sums are whole: the record's score and the name's verdict, and the words zero again */
			const int g = tid / REC_LANES;
			const int64_t i = first + g;
			if (tid % REC_LANES == 0 && i < P.n_rec) {
				const unsigned long long s = sum[g];
				uint32_t m = meta[g];
				if ((m & MD_M_COMPARED) && diff[g] == 0) m |= MD_M_SAME_NEXT;
				P.score[i] = s > MD_SCORE_CAP ? MD_SCORE_CAP : (uint32_t)s;
				P.meta[i] = m & ~MD_M_COMPARED;
				sum[g] = 0; diff[g] = 0;
			}
		}
		REC_SYNC;
	}
}

/* record i of a sound call.  Records i and i + 1 are mates when i is a first and i + 1 a second mate of the same name and neither is
 * skipped or already marked; a record is in at most one such couple, since none is both first and second */
REC_FN void md_emit_record(const MdParams &P, const MdArena &A, int64_t i)
{
	const uint32_t m = P.meta[i], cls = m & MD_CLS_MASK;
	const uint32_t ord = A.ord_base + (uint32_t)i;
	uint8_t link = MD_LINK_NONE;
	int64_t mate = -1;
	if (cls >= MD_CLS_UNMAPPED) {
		if ((m & MD_M_FIRST) && (m & MD_M_SAME_NEXT) && i + 1 < P.n_rec) { const uint32_t x = P.meta[i + 1]; if ((x & MD_M_SECOND) && (x & MD_CLS_MASK) >= MD_CLS_UNMAPPED) mate = i + 1; }
		if ((m & MD_M_SECOND) && i > 0) { const uint32_t x = P.meta[i - 1]; if ((x & MD_M_FIRST) && (x & MD_M_SAME_NEXT) && (x & MD_CLS_MASK) >= MD_CLS_UNMAPPED) mate = i - 1; }
	}
	REC_ADD64(A.stats + NABWA_MARKDUP_STAT_SEEN, 1ull);
	const bool mate_mapped = mate >= 0 && (P.meta[mate] & MD_CLS_MASK) == MD_CLS_MAPPED;
	if (cls == MD_CLS_SKIPPED) REC_ADD64(A.stats + NABWA_MARKDUP_STAT_SKIPPED_FLAGS, 1ull);
	else if (cls == MD_CLS_ALREADY) REC_ADD64(A.stats + NABWA_MARKDUP_STAT_ALREADY, 1ull);
	else if (cls == MD_CLS_UNMAPPED) {
		REC_ADD64(A.stats + NABWA_MARKDUP_STAT_UNMAPPED, 1ull);
		if (mate_mapped) link = mate > i ? MD_LINK_NEXT : MD_LINK_PREV;       /* a half pair's unmapped mate */
	} else if (mate_mapped) {                                                  /* a pair: its tuple with the first mate, a shadow at either end */
		const bool first = mate > i, shadow = P.single_ends == NABWA_MARKDUP_ENDS_5P;
		const unsigned int at = rec_fetch_add(A.n_tup, (first ? 1u : 0u) + (shadow ? 1u : 0u));
		unsigned int w = at;
		if (first) {
			const uint64_t a = P.end[i], b = P.end[mate];
			const uint64_t s = (uint64_t)P.score[i] + P.score[mate];
			A.hi[w] = a < b ? a : b; A.lo[w] = a < b ? b : a; A.k3[w] = MD_K3(true, s > MD_SCORE_CAP ? MD_SCORE_CAP : (uint32_t)s, ord);
			++w;
			REC_ADD64(A.stats + NABWA_MARKDUP_STAT_PAIRS, 1ull);
		}
		if (shadow) { A.hi[w] = P.end[i]; A.lo[w] = 0; A.k3[w] = MD_K3(false, 0xffffffffu, ord); }
	} else {                                                                   /* a fragment: a single read, a half pair's mapped mate, an orphan */
		const unsigned int w = rec_fetch_add(A.n_tup, 1u);
		A.hi[w] = P.end[i]; A.lo[w] = P.single_ends == NABWA_MARKDUP_ENDS_BOTH ? (uint64_t)P.c3[i] : 0; A.k3[w] = MD_K3(false, P.score[i], ord);
		REC_ADD64(A.stats + NABWA_MARKDUP_STAT_FRAGMENTS, 1ull);
		if ((m & MD_M_PAIRED) && mate < 0) REC_ADD64(A.stats + NABWA_MARKDUP_STAT_ORPHANS, 1ull);
	}
	A.link[ord] = link;
}

/* position j of the n tuples in (hi, lo, k3) order, idx[j] being the tuple there.  The first of a group wins; every other real member is marked */
REC_FN void md_mark_one(int64_t j, const uint32_t *idx, const uint64_t *hi, const uint64_t *lo, const uint64_t *k3, uint8_t *dup, unsigned long long *stats)
{
	if (j == 0) return;
	const uint32_t t = idx[j], u = idx[j - 1];
	const uint64_t k = k3[t];
	const bool pair = (k & MD_K3_PAIR) != 0;
	if (!pair && MD_K3_NSCORE(k) == 0) return;                                 /* a shadow */
	if (hi[t] != hi[u] || lo[t] != lo[u] || ((k ^ k3[u]) & MD_K3_PAIR)) return;  /* the head of its group */
	const uint32_t ord = MD_K3_ORD(k);
	dup[ord] = 1;
	if (pair) dup[ord + 1] = 1;
	REC_ADD64(stats + (pair ? NABWA_MARKDUP_STAT_DUP_PAIRS : NABWA_MARKDUP_STAT_DUP_FRAGMENTS), 1ull);
}

/* ordinal o of the n records added: a half pair's unmapped mate (which no tuple names, so nobody else writes dup[o]) takes the mark of its
 * mate (a fragment, which this pass does not write) */
REC_FN void md_prop_one(int64_t o, const uint8_t *link, uint8_t *dup, unsigned long long *stats)
{
	const uint8_t l = link[o];
	uint8_t d = dup[o];
	if (l == MD_LINK_NEXT) d = dup[o + 1];
	else if (l == MD_LINK_PREV) d = dup[o - 1];
	if (l != MD_LINK_NONE) dup[o] = d;
	if (d) REC_ADD64(stats + NABWA_MARKDUP_STAT_DUP_RECORDS, 1ull);
}
