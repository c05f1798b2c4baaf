// finish_body.hpp -- the bodies of the finishing kernels (finish_kernels.hip): what refine_gapped_core (bwase.c:189-237) does around its
// alignment, and bwa_cal_md1 (bwase.c:253-315), on the 2-bit reference held in HBM.
//
//   fin_window_wave   one wavefront per job: the job's reference window out of the .pac, one code per byte, and its query in
//                     alignment orientation, both straight into the alignment kernel's input arrays
//   fin_cigar_job     one job per lane: the alignment kernel's 32-bit operations (slot-major) -> bwa_cigar_t with the end rules of
//                     bwase.c:213-234 and the position shift
//   fin_md_wave       one wavefront per record: the MD string and NM.  Over an M stretch the lanes compare 64 bases at a time; the
//                     mismatches are a ballot, every mismatching lane forms its own token -- decimal(run since the previous difference)
//                     and the reference character -- and an exclusive scan of the token lengths says where it goes.  WRITE = false
//                     only counts (string length, NM), WRITE = true fills the string: the caller sizes the packed buffer in between.
//
// Written in the wave operations of wave_spmd.hpp: compiled for gfx950 by finish_kernels.hip and, with NABWA_EMU (tests/emu/, test
// infrastructure), by g++ as a sequential emulation of one wave, so that every index it forms can be checked under AddressSanitizer.
// No body reads a .pac byte at or past (l_pac + 3) / 4, and none holds an array of its own: no scratch.
#pragma once
#include <stdint.h>
#ifdef NABWA_EMU
#include "emu_hip.hpp"
#define FIN_FN static inline
#else
#include <hip/hip_runtime.h>
#define FIN_FN __device__ __forceinline__
#endif
#include "wave_spmd.hpp"

struct FinHole { int64_t offset; int32_t len; int32_t amb; };       /* bntamb1_t as the kernels read it, 16 bytes */
struct FinRef { const uint8_t *pac; int64_t l_pac; const FinHole *holes; int32_t n_holes; int32_t pad; };

/* one refinement job.  pos is the signed position of bwase.c:197; src_off is where the record's read starts in the uploaded reads;
 * copy != 0: the query is reads1[src_off ..) as it stands (rseq, or a caller's query in alignment orientation), else reads0[src_off ..)
 * reversed (seq is held reversed) */
struct FinJob { int64_t win_lo, src_off, pos; int32_t win_n, len, ext, copy; };
/* one record for MD / NM: the read as above, its position and where its CIGAR row starts (n_cigar 0: the ungapped branch) */
struct FinRec { int64_t src_off, cig_off; uint32_t pos; int32_t len, n_cigar, copy; };

FIN_FN uint32_t fin_pac_at(const uint8_t *pac, int64_t k) { return (uint32_t)(pac[k >> 2] >> ((~k & 3) << 1)) & 3u; }
/* the four bases of a .pac byte as four bytes, the first base lowest */
FIN_FN uint32_t fin_pac_expand(uint32_t b) { return (b >> 6 & 3u) | (b >> 4 & 3u) << 8 | (b >> 2 & 3u) << 16 | (b & 3u) << 24; }

/* ------------------------------------------------------------------ window and query */

/* ref[0, win_n) = bases win_lo .. win_lo + win_n of the reference (win_lo >= 0, win_lo + win_n <= l_pac: the host clipped);
 * qry[0, len) = the read in alignment orientation.  A lane takes one .pac byte and stores its four codes with one 32-bit store; the
 * bases in front of the first whole byte and behind the last one go byte-wise. */
FIN_FN void fin_window_wave(const uint8_t *pac, const FinJob &J, const uint8_t *reads0, const uint8_t *reads1, uint8_t *ref, uint8_t *qry)
{
#ifndef NABWA_EMU
	const int ln = (int)(threadIdx.x & 63u);
#endif
	const int head0 = (int)((4 - (J.win_lo & 3)) & 3), head = head0 < J.win_n ? head0 : J.win_n;
	const int n_bytes = (J.win_n - head) >> 2, tail0 = head + 4 * n_bytes, tail = J.win_n - tail0;
	const int64_t byte0 = (J.win_lo + head) >> 2;
	LANES { if (ln < head) ref[ln] = (uint8_t)fin_pac_at(pac, J.win_lo + ln); }
	for (int b = 0; b < n_bytes; b += 64) {
		LANES {
			const int i = b + ln;
			if (i < n_bytes) { const uint32_t v = fin_pac_expand(pac[byte0 + i]); __builtin_memcpy(ref + head + 4 * i, &v, 4); }
		}
	}
	LANES { if (ln < tail) ref[tail0 + ln] = (uint8_t)fin_pac_at(pac, J.win_lo + tail0 + ln); }
	const uint8_t *src = (J.copy ? reads1 : reads0) + J.src_off;
	for (int b = 0; b < J.len; b += 64) {
		LANES { const int k = b + ln; if (k < J.len) qry[k] = J.copy ? src[k] : src[J.len - 1 - k]; }
	}
}

/* ------------------------------------------------------------------ CIGAR end rules */

#define FIN_COP(c) ((c) >> 14)
#define FIN_CLEN(c) ((c) & 0x3fff)
#define FIN_CMAKE(op, len) ((uint16_t)((op) << 14 | (len)))

/* c32[k * stride]: operation k of this job, len << 4 | op.  Writes row[0, n) and returns n, or -1 for a path of more than max_cigar
 * operations or of none (row is then untouched).  bwase.c:213-234, in that order. */
FIN_FN int fin_cigar_job(const uint32_t *c32, size_t stride, int nc, int max_cigar, int ext, int end_correct, int64_t pos, uint16_t *row,
						 uint32_t *pos_out)
{
	if (nc > max_cigar || nc < 1) return -1;
	int m = nc; int64_t p = pos; int d = 0;
	for (int k = 0; k < m; ++k) {
		const uint32_t w = c32[(size_t)k * stride];
		const uint32_t op = w & 0xfu, len = w >> 4;
		row[k] = FIN_CMAKE(op, len);
		if (op == 2) d -= (int)(len & 0x3fffu); else if (op == 1) d += (int)(len & 0x3fffu);
	}
	if (ext < 0 && end_correct) p += d;                /* forward strand: the end was anchored, the start moves by the net indel */
	if (FIN_COP(row[0]) == 2) { p += FIN_CLEN(row[0]); for (int k = 0; k + 1 < m; ++k) row[k] = row[k + 1]; --m; }
	if (m >= 1 && FIN_COP(row[m - 1]) == 2) --m;
	if (m < 1) return -1;                              /* a path of deletions only: no query base, cannot happen */
	if (FIN_COP(row[m - 1]) == 1) row[m - 1] = FIN_CMAKE(3, FIN_CLEN(row[m - 1]));
	if (FIN_COP(row[0]) == 1) row[0] = FIN_CMAKE(3, FIN_CLEN(row[0]));
	*pos_out = (uint32_t)p;
	return m;
}

/* ------------------------------------------------------------------ MD / NM */

/* base of the reference at p < l_pac with the ambiguity codes of the .amb holes restored (bwase.c:239-251): 0-3, or the hole's letter */
FIN_FN uint32_t fin_ref_char(const FinRef &R, bool plain, int64_t p)
{
	if (!plain) {
		int lo = 0, hi = R.n_holes;
		while (lo < hi) {
			const int mid = (lo + hi) >> 1;
			const int64_t ho = R.holes[mid].offset;
			if (p >= ho + R.holes[mid].len) lo = mid + 1;
			else if (p < ho) hi = mid;
			else return (uint32_t)(uint8_t)R.holes[mid].amb;
		}
	}
	return fin_pac_at(R.pac, p);
}
FIN_FN uint32_t fin_digits(uint32_t v) { uint32_t n = 1; while (v >= 10u) { v /= 10u; ++n; } return n; }
/* decimal(v) at dst[0, fin_digits(v)) */
FIN_FN void fin_put_num(char *dst, uint32_t v) { uint32_t n = fin_digits(v); do { dst[--n] = (char)('0' + v % 10u); v /= 10u; } while (n); }
FIN_FN char fin_base_chr(uint32_t c) { return c > 3u ? (char)c : (char)(0x54474341u >> (8u * c) & 0xffu); }      /* "ACGT"[c] */

/* MD and NM of one record.  reads0 / reads1 as for FinJob; cigar: the record's row (unused when n_cigar is 0).  Returns the string's length
 * without its NUL; WRITE: md[0, length] is filled, NUL included.  The wave-uniform state -- position, read offset, run, NM, characters
 * so far -- is the same in every lane. */
template <bool WRITE>
FIN_FN uint32_t fin_md_wave(const FinRef &R, const FinRec &Q, const uint8_t *reads0, const uint8_t *reads1, const uint16_t *cigar, char *md,
							int32_t *nm_out)
{
#ifndef NABWA_EMU
	const int ln = (int)(threadIdx.x & 63u);
#endif
	const uint8_t *src = (Q.copy ? reads1 : reads0) + Q.src_off;
	const int len = Q.len;
#define FIN_Q(y_) ((uint32_t)(Q.copy ? src[(y_)] : src[len - 1 - (y_)]))
	int64_t pos = (int64_t)Q.pos;
	int y = 0;
	uint32_t u = 0, nm = 0, o = 0;
	/* the stretch of the reference this alignment can touch, and whether a hole lies under it */
	int64_t span = len;
	if (Q.n_cigar) { span = 0; for (int k = 0; k < Q.n_cigar; ++k) { const uint32_t op = FIN_COP(cigar[k]); if (op == 0 || op == 2) span += FIN_CLEN(cigar[k]); } }
	bool plain = true;
	{
		int lo = 0, hi = R.n_holes;
		while (lo < hi) { const int mid = (lo + hi) >> 1; if (R.holes[mid].offset + R.holes[mid].len <= pos) lo = mid + 1; else hi = mid; }
		if (lo < R.n_holes && R.holes[lo].offset < pos + span) plain = false;
	}
	const int n_ops = Q.n_cigar ? Q.n_cigar : 1;
	for (int k = 0; k < n_ops; ++k) {
		const int l = Q.n_cigar ? (int)FIN_CLEN(cigar[k]) : len, op = Q.n_cigar ? (int)FIN_COP(cigar[k]) : 0;
		const int64_t left = R.l_pac - pos;
		const int lim = left <= 0 ? 0 : ((int64_t)l < left ? l : (int)left);     /* M and D stop at l_pac (bwase.c:275, 291) */
		if (op == 0) {
			for (int z = 0; z < lim; z += 64) {
				const int n_act = lim - z < 64 ? lim - z : 64;
				LANE(uint32_t, c); LANE(uint32_t, mis); LANE(uint32_t, tlen); LANE(uint32_t, toff);
				LANES {
					L(mis) = 0; L(c) = 0;
					if (ln < n_act) {
						L(c) = fin_ref_char(R, plain, pos + z + ln);
						const uint32_t q = FIN_Q(y + z + ln);
						L(mis) = (L(c) > 3u || q > 3u || L(c) != q) ? 1u : 0u;
					}
				}
				const uint64_t mask = WBALLOT(L(mis) != 0u);
				if (mask) {
					LANE(uint32_t, run);
					LANES {
						const uint64_t below = mask & ((1ull << ln) - 1ull);
						L(run) = below ? (uint32_t)(ln - (63 - __builtin_clzll(below)) - 1) : u + (uint32_t)ln;
						L(tlen) = L(mis) ? fin_digits(L(run)) + 1u : 0u;
					}
					uint32_t total;
					WEXSCAN_U32(L(toff), L(tlen), total);
					if (WRITE) {
						LANES { if (L(mis)) { char *t = md + o + L(toff); fin_put_num(t, L(run)); t[L(tlen) - 1u] = fin_base_chr(L(c)); } }
					}
					o += total; nm += (uint32_t)__popcll(mask);
					u = (uint32_t)(n_act - 1 - (63 - __builtin_clzll(mask)));
				} else u += (uint32_t)n_act;
			}
			y += lim; pos += lim;
		} else if (op == 1 || op == 3) { y += l; if (op == 1) nm += (uint32_t)l; }
		else {
			const uint32_t nd = fin_digits(u);
			if (WRITE) { ONE_LANE { fin_put_num(md + o, u); md[o + nd] = '^'; } }
			o += nd + 1u;
			if (WRITE) {
				for (int z = 0; z < lim; z += 64) {
					LANES { if (z + ln < lim) md[o + (uint32_t)(z + ln)] = fin_base_chr(fin_ref_char(R, plain, pos + z + ln)); }
				}
			}
			o += (uint32_t)lim; pos += lim;
			u = 0; nm += (uint32_t)l;
		}
	}
	const uint32_t nd = fin_digits(u);                  /* the closing number is always written */
	if (WRITE) { ONE_LANE { fin_put_num(md + o, u); md[o + nd] = 0; } }
	o += nd;
	*nm_out = (int32_t)nm;
#undef FIN_Q
	return o;
}
