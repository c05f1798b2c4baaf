// damage_body.hpp -- the bodies of the damage profile of finished BAM records (damage_kernels.hip, nabwa_damage*; the
// semantics: include/nabwa.h):
//
//   dmg_record_part  lane t of the REC_LANES lanes that take one record: its fields, its class, the CIGAR walked twice -- once for what it
//                    consumes (a CIGAR that does not consume l_seq read bases is damage) and for the holes under its reference span, once
//                    for the columns -- and the counts into the workgroup's table
//   dmg_block        one workgroup of the persistent grid: REC_GROUPS records per trip, the table flushed into the call's 64-bit table
//
// A record starts at any byte, so nothing in it is aligned; the hardware reads a global word at any byte address.  The fields come as 32-bit
// words.  An M run's columns go to the lanes in pieces of DMG_COLS = 8: lane t takes pieces t, t + 16, ...; a piece's read bases (2 per byte, at
// most 5 bytes) and its reference bases (4 per byte, at most 3) each come with ONE load of 8 bytes, or byte by byte where fewer than 8 remain
// in the record or in the .pac: no byte outside [rec, rec + size) and none outside pac[0, l_pac / 4 + 1) is read.  Every lane walks the
// operations itself (they are few, and the lanes of a group run in step: sixteen walks cost what one costs), so no lane waits for another
// and the group needs no exchange.  The holes under a record's reference span are found once per record by a binary search over the sorted
// list -- most records have none, and then no column looks at the list.
//
// The table: 32-bit words in LDS, DmgTab below -- sub5, sub3, the length bins, the stats.  Why no word wraps between two flushes: a word
// rises by at most one per column (the two substitution tables are apart; the column stats) or one per record (classes, length bins).  A
// record of `size` bytes holds (l_seq + 1) / 2 + l_seq <= size - 36 bytes of bases and qualities, so its columns, at most l_seq, are fewer
// than 2/3 size, and it is one record.  Between two flushes a workgroup takes either trips whose records together have fewer than
// DMG_FLUSH_BYTES = 2^32 bytes -- fewer than 2/3 2^32 columns -- or one single record, whose block_size is a 32-bit word: at most 2^32 + 3
// bytes, again fewer than 2^32 columns.
//
// Compiled for gfx950 by damage_kernels.hip and, with NABWA_EMU (tests/emu/, test infrastructure, and the host comparison of
// profiles/damage_rate.py), by g++: there the threads of a workgroup run one after the other between the barriers, so that every address
// the bodies form can be checked under AddressSanitizer without a GPU.  No arrays: no scratch.
#pragma once
#include <stdint.h>
#include "../../include/nabwa.h"
#include "finish_body.hpp"          /* FinRef, FinHole, fin_pac_at */
#include "rec_body.hpp"        /* the macro layer, REC_LANES ... REC_MIN_REC, rec_u32, rec_op_read / rec_op_ref, REC_HEAD */

#define DMG_COLS    8                           /* columns per lane and piece */
#ifndef DMG_FLUSH_BYTES
#define DMG_FLUSH_BYTES 0x100000000ull          /* (the emulation also runs with a small value, to take every path of dmg_block) */
#endif
#define DMG_OK  0
#define DMG_BAD 1

/* the table of n_pos, in words: sub5 at 0, sub3 at sub3, the length bins at len, the stats at stats; `words` in all.  The workgroup's table
 * (32-bit), the call's and the handle's (64-bit) share it. */
struct DmgTab { int32_t sub3, len, stats, words; };
REC_HD DmgTab dmg_tab(int n_pos)
{
	DmgTab t; t.sub3 = (n_pos + 1) * 16; t.len = 2 * t.sub3; t.stats = t.len + NABWA_DAMAGE_LEN_BINS; t.words = t.stats + NABWA_DAMAGE_N_STATS;
	return t;
}

/* what a call works on.  off[] are the caller's offsets, base = off[0]: record i lies at in + (off[i] - base) */
struct DmgParams {
	const uint8_t *in; const int64_t *off; int64_t base; int32_t n_rec;
	int32_t n_contigs; const int64_t *contig_off;
	FinRef R;
	int32_t n_pos, min_mapq; uint32_t exclude_flags, require_flags;
};

/* the `need` (1..8) bytes at p, little-endian, of which `avail` exist (the rest reads as 0): one 8-byte load where 8 exist */
REC_FN uint64_t dmg_load(const uint8_t *p, int64_t avail, int need)
{
	uint64_t w = 0;
	if (avail >= 8) { __builtin_memcpy(&w, p, 8); return w; }
	const int n = avail < need ? (int)avail : need;
	for (int b = 0; b < n; ++b) w |= (uint64_t)p[b] << (8 * b);
	return w;
}
REC_FN bool dmg_op_col(uint32_t op) { return op == 0 || op == 7 || op == 8; }                            /* M = X */

/* lane t of the group of record `rec` of `size` >= REC_MIN_REC bytes; tab: the workgroup's table.  DMG_BAD for a damaged record (every lane
 * says so, nothing is counted), else DMG_OK */
REC_FN int dmg_record_part(const DmgParams &P, const DmgTab &T, const uint8_t *rec, int64_t size, int t, uint32_t *tab)
{
	REC_HEAD(rec, size, DMG_BAD);
	int cls = NABWA_DAMAGE_STAT_COUNTED;
	if ((flag & P.exclude_flags) || (flag & P.require_flags) != P.require_flags) cls = NABWA_DAMAGE_STAT_SKIPPED_FLAGS;
	else if (ref_id < 0 || ref_id >= P.n_contigs || pos < 0) cls = NABWA_DAMAGE_STAT_SKIPPED_PLACE;
	else if ((int32_t)mapq < P.min_mapq) cls = NABWA_DAMAGE_STAT_SKIPPED_MAPQ;
	else if (L == 0 || n_cig == 0) cls = NABWA_DAMAGE_STAT_SKIPPED_EMPTY;
	if (cls != NABWA_DAMAGE_STAT_COUNTED) {
		if (t == 0) { REC_INC(tab + T.stats + NABWA_DAMAGE_STAT_SEEN); REC_INC(tab + T.stats + cls); }
		return DMG_OK;
	}
	const uint8_t *cig = rec + REC_MIN_REC + l_name, *seq = cig + 4 * n_cig, *end = rec + size;
	/* what the CIGAR consumes (operations of 28 bits, at most 65535 of them: no sum leaves 64 bits) */
	uint64_t n_read = 0, n_ref = 0;
	for (uint32_t c = 0; c < n_cig; ++c) {
		const uint32_t w = rec_u32(cig + 4 * c), op = w & 15u, len = w >> 4;
		if (rec_op_read(op)) n_read += len;
		if (rec_op_ref(op)) n_ref += len;
	}
	if (n_read != L) return DMG_BAD;
	const int64_t rp = P.contig_off[ref_id] + pos, rp_end = rp + (int64_t)n_ref, l_pac = P.R.l_pac, pac_bytes = l_pac / 4 + 1;
	/* the holes that overlap [rp, rp_end): h0 is the first that ends behind rp, n_h of them start before rp_end */
	int h0 = 0, n_h = 0;
	if (P.R.n_holes) {
		int hi = P.R.n_holes;
		while (h0 < hi) { const int mid = (h0 + hi) >> 1; if (P.R.holes[mid].offset + P.R.holes[mid].len <= rp) h0 = mid + 1; else hi = mid; }
		while (h0 + n_h < P.R.n_holes && P.R.holes[h0 + n_h].offset < rp_end) ++n_h;
	}
	const bool rev = (flag & 0x10u) != 0;
	uint32_t n_cols = 0, n_skip_read = 0, n_skip_ref = 0;
	int64_t qi = 0, k = rp;
	for (uint32_t c = 0; c < n_cig; ++c) {
		const uint32_t w = rec_u32(cig + 4 * c), op = w & 15u;
		const int64_t len = (int64_t)(w >> 4);
		if (dmg_op_col(op)) {
			for (int64_t at = (int64_t)DMG_COLS * t; at < len; at += DMG_COLS * REC_LANES) {
				const int64_t qs = qi + at, ks = k + at;
				const int nc = len - at < DMG_COLS ? (int)(len - at) : DMG_COLS;
				const uint8_t *sp = seq + (qs >> 1);
				const uint64_t sw = dmg_load(sp, end - sp, (int)(((qs & 1) + nc + 1) >> 1));
				const uint64_t pw = ks < l_pac ? dmg_load(P.R.pac + (ks >> 2), pac_bytes - (ks >> 2), (int)(((ks & 3) + nc + 3) >> 2)) : 0;
				for (int j = 0; j < nc; ++j) {
					const int n = (int)(qs & 1) + j;
					const uint32_t code = (uint32_t)(sw >> (8 * (n >> 1) + ((n & 1) ? 0 : 4))) & 15u;
					if (code != 1 && code != 2 && code != 4 && code != 8) { ++n_skip_read; continue; }
					const int64_t kk = ks + j;
					bool hole = kk >= l_pac;
					for (int h = 0; h < n_h && !hole; ++h) hole = kk >= P.R.holes[h0 + h].offset && kk < P.R.holes[h0 + h].offset + P.R.holes[h0 + h].len;
					if (hole) { ++n_skip_ref; continue; }
					const int m = (int)(ks & 3) + j;
					uint32_t r = (uint32_t)(pw >> (8 * (m >> 2) + ((~m & 3) << 1))) & 3u;
					uint32_t q = code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : 3u;
					int64_t d5 = qs + j, d3 = (int64_t)L - 1 - d5;
					if (rev) { r = 3u - r; q = 3u - q; const int64_t x = d5; d5 = d3; d3 = x; }
					const int p5 = d5 < P.n_pos ? (int)d5 : P.n_pos, p3 = d3 < P.n_pos ? (int)d3 : P.n_pos;
					REC_INC(tab + (p5 * 4 + (int)r) * 4 + (int)q);
					REC_INC(tab + T.sub3 + (p3 * 4 + (int)r) * 4 + (int)q);
					++n_cols;
				}
			}
		}
		if (rec_op_read(op)) qi += len;
		if (rec_op_ref(op)) k += len;
	}
	if (n_cols) REC_ADD32(tab + T.stats + NABWA_DAMAGE_STAT_COLUMNS_COUNTED, n_cols);
	if (n_skip_read) REC_ADD32(tab + T.stats + NABWA_DAMAGE_STAT_COLUMNS_SKIPPED_READ, n_skip_read);
	if (n_skip_ref) REC_ADD32(tab + T.stats + NABWA_DAMAGE_STAT_COLUMNS_SKIPPED_REF, n_skip_ref);
	if (t == 0) {
		REC_INC(tab + T.stats + NABWA_DAMAGE_STAT_SEEN); REC_INC(tab + T.stats + NABWA_DAMAGE_STAT_COUNTED);
		REC_INC(tab + T.len + (int)(L < NABWA_DAMAGE_LEN_BINS - 1 ? L : NABWA_DAMAGE_LEN_BINS - 1));
	}
	return DMG_OK;
}

/* the workgroup's non-zero words into the call's table, and zero again; a barrier on either side */
#define DMG_FLUSH() do { \
	REC_SYNC; \
	REC_THREADS { for (int w = tid; w < T.words; w += REC_BLOCK) { const uint32_t v = tab[w]; if (v) { REC_ADD64(call + w, (unsigned long long)v); tab[w] = 0; } } } \
	REC_SYNC; \
} while (0)

/* workgroup `block` of `n_blocks`: trips block, block + n_blocks, ... of REC_GROUPS records each.  tab: T.words words of LDS; call: the call's
 * table, zero before the kernel; *bad: 0xffffffff before it, the lowest damaged record after it.  Everything that decides a flush is the same
 * in every thread of the workgroup. */
REC_FN void dmg_block(const DmgParams &P, uint32_t *tab, unsigned long long *call, unsigned int *bad, int block, int n_blocks)
{
	const DmgTab T = dmg_tab(P.n_pos);
	REC_THREADS { for (int w = tid; w < T.words; w += REC_BLOCK) tab[w] = 0; }
	REC_SYNC;
	uint64_t held = 0;                                  /* bytes of the records taken since the last flush */
	for (int64_t first = (int64_t)block * REC_GROUPS; first < P.n_rec; first += (int64_t)n_blocks * REC_GROUPS) {
		const int64_t last = first + REC_GROUPS < P.n_rec ? first + REC_GROUPS : P.n_rec;
		const uint64_t bytes = (uint64_t)(P.off[last] - P.off[first]);
		if (bytes >= DMG_FLUSH_BYTES) {                 /* records of gigabytes: one at a time, a flush around each */
			for (int64_t i = first; i < last; ++i) {
				DMG_FLUSH();
				REC_THREADS {
					if (tid < REC_LANES) {
						const int64_t o = P.off[i];
						if (dmg_record_part(P, T, P.in + (o - P.base), P.off[i + 1] - o, tid, tab) != DMG_OK && tid == 0) REC_MIN32(bad, (unsigned int)i);
					}
				}
			}
			DMG_FLUSH();
			held = 0;
			continue;
		}
		if (held + bytes >= DMG_FLUSH_BYTES) { DMG_FLUSH(); held = 0; }
		held += bytes;
		REC_THREADS {
			const int64_t i = first + tid / REC_LANES;
			if (i < last) {
				const int64_t o = P.off[i];
				if (dmg_record_part(P, T, P.in + (o - P.base), P.off[i + 1] - o, tid % REC_LANES, tab) != DMG_OK && tid % REC_LANES == 0) REC_MIN32(bad, (unsigned int)i);
			}
		}
	}
	DMG_FLUSH();
}
