// bgzf_inflate_body.hpp -- the per-member body of the BGZF decompressor (bgzf_inflate.hip): the RFC 1951 payload of one BGZF member
// becomes its <= 0x10000 inflated bytes at the member's destination, with one status word.
//
// One wavefront (a workgroup of 64 lanes) per member.  Huffman decoding of one stream is serial, so lane 0 decodes; what the wave
// shares is the writing.  The output window is the destination itself, in global memory: LDS holds only the code tables, the CRC
// table and one batch of tokens (5.4 KB), so many waves fit a CU and hide each other's latency; a back-reference reads bytes this
// wave wrote earlier, out of L2.  The body is a sequence of phases; a phase is a function of the lane number, and BGZI_PHASE puts
// a barrier behind it.  With BGZF_EMU defined (tests only, never part of libnabwa.so) g++ compiles the same phases and BGZI_PHASE
// runs the lanes one after the other: the kernel's indexing under AddressSanitizer.
//
//   init     the CRC table, the decoder's state
//   decode   lane 0: deflate block headers, code tables and symbols, until the batch is full (BGZI_NLIT literals or BGZI_NCOPY
//            copies), the final block has ended or the stream is found damaged.  Every token is checked here: its bytes lie inside
//            [0, ISIZE), a distance does not reach before byte 0, a stored block's bytes lie inside the payload.
//   lits     the batch's literals, one per lane and round
//   copy(i)  the batch's i-th copy, its bytes dealt over the lanes: a back-reference (for distance < length byte j is source byte
//            j mod distance, so the source never overlaps the destination) or the bytes of a stored block.  Copies run in stream
//            order; one whose source may hold bytes of an earlier copy of the same batch has a barrier in front of it.
//   crc      lane t: the CRC-32 of its share of the output, moved to the end (bgzf_mulmod of bgzf_deflate_body.hpp) and XOR-ed
//   finish   lane 0: length and CRC against the trailer, the status word
//
// Damaged input is a status, never a fault.  Every payload read is checked against the payload's end (bgzi_need), every write
// against ISIZE, every back-reference against byte 0, every table index against its table; every loop is bounded by the payload's
// bits, ISIZE, 258, 320 code lengths or 15; no lane waits for another outside a barrier.
#pragma once
#include <stdint.h>
#include "bgzf_deflate_body.hpp"                   /* BGZF_LANES, BGZF_FN, BGZF_XOR, bgzf_mulmod, bgzf_shift_op */

#define BGZI_NLIT   512u                           /* literals of a batch */
#define BGZI_NCOPY  128u                           /* copies of a batch */
#define BGZI_MAXOUT 0x10000u

enum {                                             /* the status word of a member */
	BGZI_OK = 0,
	BGZI_BTYPE3 = 1,                               /* block type 11 */
	BGZI_STORED_LEN = 2,                           /* stored block: LEN is not the complement of NLEN */
	BGZI_TRUNCATED = 3,                            /* the payload ends before the final block does */
	BGZI_OVERSUBSCRIBED = 4,                       /* a set of code lengths that is over-subscribed */
	BGZI_INCOMPLETE = 5,                           /* ... or incomplete (other than a single code of one bit, or no distance code) */
	BGZI_REPEAT_FIRST = 6,                         /* repeat code 16 with no length before it */
	BGZI_LENGTHS_OVERRUN = 7,                      /* a repeat runs past HLIT + HDIST */
	BGZI_NO_EOB = 8,                               /* the end-of-block symbol has no code */
	BGZI_BAD_SYMBOL = 9,                           /* literal/length symbol 286 or 287, distance symbol 30 or 31 */
	BGZI_DIST_TOO_FAR = 10,                        /* a distance that reaches before the member's first byte */
	BGZI_OUTPUT_LONG = 11,                         /* more output than ISIZE */
	BGZI_OUTPUT_SHORT = 12,                        /* the final block ends with less output than ISIZE */
	BGZI_CRC = 13,                                 /* the output's CRC-32 is not the trailer's */
	BGZI_TOO_MANY_CODES = 14,                      /* HLIT > 29 or HDIST > 29 */
	BGZI_INVALID_CODE = 15,                        /* bits that are no code of an incomplete set */
	BGZI_INTERNAL = 16,                            /* the batch loop's bound was reached: cannot happen */
	BGZI_N_STATUS = 17
};

struct BgzfInBlk {                                 /* one member, as the host reads it from the header and the trailer */
	uint64_t src, dst;                             /* the payload's offset in the compressed bytes, the output's in the inflated ones */
	uint32_t n_src, isize, crc, pad;
};

struct BgziCode { uint16_t cnt[16]; uint16_t sym[288]; };      /* canonical code: symbols per length, symbols in code order */

struct BgziShared {                                /* 5 424 bytes */
	uint32_t crc_tab[256];
	uint32_t lit[BGZI_NLIT];                       /* output offset << 8 | byte */
	uint32_t cp_a[BGZI_NCOPY];                     /* output offset | (length - 1) << 16 */
	uint32_t cp_b[BGZI_NCOPY];                     /* distance - 1, or a stored block's payload offset; bit 17: stored; bit 18: barrier first */
	BgziCode lcode, dcode;
	uint8_t lens[320];
	uint64_t bitbuf;
	uint32_t bitcnt, in_pos, out_pos, state, bfinal, status, done, n_lit, n_copy, crc;
};

enum { BGZI_ST_HEADER = 0, BGZI_ST_CODES = 1 };

#ifndef BGZF_EMU
#define BGZI_LANES(t, call) do { call; } while (0)
#define BGZI_BARRIER()      __syncthreads()
#else
#define BGZI_LANES(t, call) do { for (uint32_t t = 0; t < BGZF_LANES; ++t) { call; } } while (0)
#define BGZI_BARRIER()      ((void)0)
#endif
#define BGZI_PHASE(t, call) do { BGZI_LANES(t, call); BGZI_BARRIER(); } while (0)

/* ------------------------------------------------------------------ bits (lane 0) */
struct BgziBits { const uint8_t *p; uint32_t n, pos, cnt; uint64_t buf; };
/* at least k <= 32 bits in the buffer, or false: the payload has no more */
BGZF_FN bool bgzi_need(BgziBits &b, uint32_t k)
{
	if (b.cnt >= k) return true;
	while (b.cnt <= 56 && b.pos < b.n) { b.buf |= (uint64_t)b.p[b.pos++] << b.cnt; b.cnt += 8; }
	return b.cnt >= k;
}
BGZF_FN uint32_t bgzi_take(BgziBits &b, uint32_t k)            /* after bgzi_need(k); k <= 32 */
{
	const uint32_t v = (uint32_t)(b.buf & ((1ull << k) - 1));
	b.buf >>= k; b.cnt -= k;
	return v;
}

/* lens[0, n) -> the canonical code; 0, or the status of a set that cannot be used.  An incomplete set passes only as zlib lets it:
 * no code at all, or nothing longer than one bit */
BGZF_FN uint32_t bgzi_construct(BgziCode &c, const uint8_t *lens, uint32_t n, bool may_lack)
{
	uint16_t offs[16];
	for (uint32_t l = 0; l < 16; ++l) c.cnt[l] = 0;
	for (uint32_t i = 0; i < n; ++i) c.cnt[lens[i] & 15u]++;
	uint32_t max = 15;
	while (max > 0 && c.cnt[max] == 0) --max;
	int32_t left = 1;
	for (uint32_t l = 1; l < 16; ++l) {
		left = left * 2 - (int32_t)c.cnt[l];
		if (left < 0) return BGZI_OVERSUBSCRIBED;
	}
	if (left > 0 && max != 0 && !(may_lack && max == 1)) return BGZI_INCOMPLETE;
	offs[0] = 0; offs[1] = 0;
	for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + c.cnt[l]);
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t l = lens[i] & 15u;
		if (l) { const uint32_t at = offs[l]++; if (at < 288) c.sym[at] = (uint16_t)i; }
	}
	return BGZI_OK;
}

/* the next symbol of code c, bit by bit (at most 15); false with st set when the payload ends or the bits are no code */
BGZF_FN bool bgzi_symbol(BgziBits &b, const BgziCode &c, uint32_t &sym, uint32_t &st)
{
	(void)bgzi_need(b, 15);
	uint32_t code = 0, first = 0, index = 0;
	uint64_t bits = b.buf;
	for (uint32_t l = 1; l < 16; ++l) {
		if (l > b.cnt) { st = BGZI_TRUNCATED; return false; }
		code |= (uint32_t)(bits & 1u); bits >>= 1;
		const uint32_t count = c.cnt[l];
		if (code < first + count) {
			const uint32_t at = index + (code - first);
			if (at >= 288) break;
			sym = c.sym[at];
			b.buf >>= l; b.cnt -= l;
			return true;
		}
		index += count; first = (first + count) << 1; code <<= 1;
	}
	st = BGZI_INVALID_CODE;
	return false;
}

/* the code tables of a dynamic block (RFC 1951 3.2.7) */
BGZF_FN uint32_t bgzi_dynamic(BgziShared &Sh, BgziBits &b)
{
	const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
	if (!bgzi_need(b, 14)) return BGZI_TRUNCATED;
	const uint32_t nlen = bgzi_take(b, 5) + 257, ndist = bgzi_take(b, 5) + 1, ncode = bgzi_take(b, 4) + 4;
	if (nlen > 286 || ndist > 30) return BGZI_TOO_MANY_CODES;
	for (uint32_t i = 0; i < 19; ++i) Sh.lens[i] = 0;
	for (uint32_t i = 0; i < ncode; ++i) {
		if (!bgzi_need(b, 3)) return BGZI_TRUNCATED;
		Sh.lens[order[i]] = (uint8_t)bgzi_take(b, 3);
	}
	if (uint32_t st = bgzi_construct(Sh.dcode, Sh.lens, 19, false)) return st;      /* the code-length code borrows the distance table */
	uint32_t idx = 0;
	while (idx < nlen + ndist) {                       /* every turn adds at least one length: at most 316 turns */
		uint32_t sym, st = 0;
		if (!bgzi_symbol(b, Sh.dcode, sym, st)) return st;
		if (sym < 16) { Sh.lens[idx++] = (uint8_t)sym; continue; }
		uint32_t prev = 0, rep;
		if (sym == 16) {
			if (idx == 0) return BGZI_REPEAT_FIRST;
			prev = Sh.lens[idx - 1];
			if (!bgzi_need(b, 2)) return BGZI_TRUNCATED;
			rep = 3 + bgzi_take(b, 2);
		} else if (sym == 17) {
			if (!bgzi_need(b, 3)) return BGZI_TRUNCATED;
			rep = 3 + bgzi_take(b, 3);
		} else {
			if (!bgzi_need(b, 7)) return BGZI_TRUNCATED;
			rep = 11 + bgzi_take(b, 7);
		}
		if (idx + rep > nlen + ndist) return BGZI_LENGTHS_OVERRUN;
		for (uint32_t k = 0; k < rep; ++k) Sh.lens[idx++] = (uint8_t)prev;
	}
	if (Sh.lens[256] == 0) return BGZI_NO_EOB;
	if (uint32_t st = bgzi_construct(Sh.lcode, Sh.lens, nlen, true)) return st;
	return bgzi_construct(Sh.dcode, Sh.lens + nlen, ndist, true);
}

BGZF_FN void bgzi_fixed(BgziShared &Sh)
{
	for (uint32_t i = 0; i < 288; ++i) Sh.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
	(void)bgzi_construct(Sh.lcode, Sh.lens, 288, true);
	for (uint32_t i = 0; i < 32; ++i) Sh.lens[i] = 5;           /* symbols 30 and 31 have codes and no meaning: BGZI_BAD_SYMBOL in the decode phase */
	(void)bgzi_construct(Sh.dcode, Sh.lens, 32, true);
}

/* ------------------------------------------------------------------ init */
BGZF_FN void bgzi_phase_init(BgziShared &Sh, uint32_t t)
{
	for (uint32_t i = t; i < 256; i += BGZF_LANES) {
		uint32_t c = i;
		for (int j = 0; j < 8; ++j) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1;
		Sh.crc_tab[i] = c;
	}
	if (t == 0) {
		Sh.bitbuf = 0; Sh.bitcnt = 0; Sh.in_pos = 0; Sh.out_pos = 0; Sh.state = BGZI_ST_HEADER; Sh.bfinal = 0;
		Sh.status = BGZI_OK; Sh.done = 0; Sh.n_lit = 0; Sh.n_copy = 0; Sh.crc = 0;
	}
}

/* ------------------------------------------------------------------ decode (lane 0) */
BGZF_FN void bgzi_put_copy(BgziShared &Sh, uint32_t out, uint32_t len, uint32_t b_word, uint32_t src_end, uint32_t &dirty_lo)
{
	/* bytes [dirty_lo, out) may hold what an earlier copy of this batch wrote with no barrier since */
	if (src_end > dirty_lo) { b_word |= 1u << 18; dirty_lo = out; }
	else if (dirty_lo == 0xffffffffu) dirty_lo = out;
	Sh.cp_a[Sh.n_copy] = out | ((len - 1) << 16);
	Sh.cp_b[Sh.n_copy] = b_word;
	++Sh.n_copy;
}

BGZF_FN void bgzi_phase_decode(BgziShared &Sh, uint32_t t, const uint8_t *pay, uint32_t n_src, uint32_t isize)
{
	const uint16_t lbase[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
	const uint8_t lext[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
	const uint16_t dbase[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
	const uint8_t dext[30] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };
	if (t != 0) return;
	Sh.n_lit = 0; Sh.n_copy = 0;
	if (Sh.done) return;
	BgziBits b; b.p = pay; b.n = n_src; b.pos = Sh.in_pos; b.cnt = Sh.bitcnt; b.buf = Sh.bitbuf;
	uint32_t out = Sh.out_pos, st = BGZI_OK, dirty_lo = 0xffffffffu;
	bool done = false;
	/* every turn takes at least one bit of the payload or ends the loop, and a full batch ends it */
	while (!done && Sh.n_lit < BGZI_NLIT && Sh.n_copy < BGZI_NCOPY) {
		if (Sh.state == BGZI_ST_HEADER) {
			if (!bgzi_need(b, 3)) { st = BGZI_TRUNCATED; break; }
			Sh.bfinal = bgzi_take(b, 1);
			const uint32_t btype = bgzi_take(b, 2);
			if (btype == 3) { st = BGZI_BTYPE3; break; }
			if (btype == 0) {
				bgzi_take(b, b.cnt & 7u);                          /* to the byte boundary; the buffer's whole bytes go back to the payload */
				b.pos -= b.cnt >> 3; b.cnt = 0; b.buf = 0;
				if (b.pos > n_src || n_src - b.pos < 4) { st = BGZI_TRUNCATED; break; }
				const uint32_t len = pay[b.pos] | (uint32_t)pay[b.pos + 1] << 8, nlen = pay[b.pos + 2] | (uint32_t)pay[b.pos + 3] << 8;
				b.pos += 4;
				if (len != (nlen ^ 0xffffu)) { st = BGZI_STORED_LEN; break; }
				if (n_src - b.pos < len) { st = BGZI_TRUNCATED; break; }
				if (len > isize - out) { st = BGZI_OUTPUT_LONG; break; }
				if (len) bgzi_put_copy(Sh, out, len, b.pos | (1u << 17), 0, dirty_lo);
				out += len; b.pos += len;
				if (Sh.bfinal) done = true;
				continue;
			}
			if (btype == 1) bgzi_fixed(Sh);
			else if ((st = bgzi_dynamic(Sh, b)) != BGZI_OK) break;
			Sh.state = BGZI_ST_CODES;
			continue;
		}
		uint32_t sym;
		if (!bgzi_symbol(b, Sh.lcode, sym, st)) break;
		if (sym < 256) {
			if (out >= isize) { st = BGZI_OUTPUT_LONG; break; }
			Sh.lit[Sh.n_lit++] = (out << 8) | sym;
			++out;
			continue;
		}
		if (sym == 256) {
			Sh.state = BGZI_ST_HEADER;
			if (Sh.bfinal) done = true;
			continue;
		}
		sym -= 257;
		if (sym >= 29) { st = BGZI_BAD_SYMBOL; break; }
		if (!bgzi_need(b, lext[sym])) { st = BGZI_TRUNCATED; break; }
		const uint32_t len = lbase[sym] + bgzi_take(b, lext[sym]);
		uint32_t ds;
		if (!bgzi_symbol(b, Sh.dcode, ds, st)) break;
		if (ds >= 30) { st = BGZI_BAD_SYMBOL; break; }
		if (!bgzi_need(b, dext[ds])) { st = BGZI_TRUNCATED; break; }
		const uint32_t dist = dbase[ds] + bgzi_take(b, dext[ds]);
		if (dist > out) { st = BGZI_DIST_TOO_FAR; break; }
		if (len > isize - out) { st = BGZI_OUTPUT_LONG; break; }
		bgzi_put_copy(Sh, out, len, dist - 1, out - dist + (len < dist ? len : dist), dirty_lo);
		out += len;
	}
	if (st == BGZI_OK && done && out != isize) st = BGZI_OUTPUT_SHORT;
	if (st != BGZI_OK) { Sh.status = st; done = true; }
	Sh.done = done;
	Sh.out_pos = out; Sh.in_pos = b.pos; Sh.bitcnt = b.cnt; Sh.bitbuf = b.buf;
}

/* ------------------------------------------------------------------ lits */
BGZF_FN void bgzi_phase_lits(const BgziShared &Sh, uint32_t t, uint8_t *dst, uint32_t isize)
{
	const uint32_t n = Sh.n_lit < BGZI_NLIT ? Sh.n_lit : BGZI_NLIT;
	for (uint32_t i = t; i < n; i += BGZF_LANES) {
		const uint32_t v = Sh.lit[i], o = v >> 8;
		if (o < isize) dst[o] = (uint8_t)v;
	}
}

/* ------------------------------------------------------------------ copy i */
BGZF_FN bool bgzi_copy_waits(const BgziShared &Sh, uint32_t i) { return (Sh.cp_b[i] >> 18) & 1u; }
BGZF_FN void bgzi_phase_copy(const BgziShared &Sh, uint32_t t, uint32_t i, const uint8_t *pay, uint32_t n_src, uint8_t *dst, uint32_t isize)
{
	const uint32_t a = Sh.cp_a[i], bw = Sh.cp_b[i];
	const uint32_t out = a & 0xffffu, len = (a >> 16) + 1;
	if (out + len > isize) return;                         /* the decode phase has checked it; once more where the bytes are written */
	if (bw & (1u << 17)) {
		const uint32_t src = bw & 0xffffu;
		if (src + len > n_src) return;
		for (uint32_t j = t; j < len; j += BGZF_LANES) dst[out + j] = pay[src + j];
		return;
	}
	const uint32_t dist = (bw & 0xffffu) + 1;
	if (dist > out) return;
	const uint8_t *s = dst + (out - dist);
	if (dist >= len) for (uint32_t j = t; j < len; j += BGZF_LANES) dst[out + j] = s[j];
	else for (uint32_t j = t; j < len; j += BGZF_LANES) dst[out + j] = s[j % dist];
}

/* ------------------------------------------------------------------ crc */
BGZF_FN void bgzi_phase_crc(BgziShared &Sh, uint32_t t, const uint8_t *dst, uint32_t isize)
{
	if (Sh.status != BGZI_OK) return;
	const uint32_t S = (isize + BGZF_LANES - 1) / BGZF_LANES;
	uint32_t s0 = t * S, s1 = s0 + S;
	if (s0 > isize) s0 = isize;
	if (s1 > isize) s1 = isize;
	if (s1 <= s0) return;
	uint32_t c = 0xffffffffu;
	for (uint32_t p = s0; p < s1; ++p) c = Sh.crc_tab[(c ^ dst[p]) & 0xffu] ^ (c >> 8);
	BGZF_XOR(&Sh.crc, bgzf_mulmod(bgzf_shift_op(isize - s1), ~c));
}

/* ------------------------------------------------------------------ finish (lane 0) */
BGZF_FN void bgzi_phase_finish(const BgziShared &Sh, uint32_t t, uint32_t crc, uint32_t *status)
{
	if (t != 0) return;
	*status = Sh.status != BGZI_OK ? Sh.status : Sh.crc != crc ? (uint32_t)BGZI_CRC : (uint32_t)BGZI_OK;
}

/* ------------------------------------------------------------------ one member */
BGZF_FN void bgzf_inflate_member(BgziShared &Sh, uint32_t t, const uint8_t *pay, uint32_t n_src, uint8_t *dst, uint32_t isize, uint32_t crc, uint32_t *status)
{
	if (isize > BGZI_MAXOUT || n_src > BGZI_MAXOUT) {          /* the host does not build such an entry; offsets here have 16 bits */
		if (t == 0) *status = BGZI_INTERNAL;
		return;
	}
	BGZI_PHASE(t, bgzi_phase_init(Sh, t));
	/* a batch that ends neither the stream nor in a status took at least one bit */
	const uint32_t max_batches = n_src * 8u + 2u;
	for (uint32_t k = 0; ; ++k) {
		BGZI_PHASE(t, bgzi_phase_decode(Sh, t, pay, n_src, isize));
		BGZI_PHASE(t, bgzi_phase_lits(Sh, t, dst, isize));
		const uint32_t nc = Sh.n_copy < BGZI_NCOPY ? Sh.n_copy : BGZI_NCOPY;
		for (uint32_t i = 0; i < nc; ++i) {
			if (bgzi_copy_waits(Sh, i)) BGZI_BARRIER();
			BGZI_LANES(t, bgzi_phase_copy(Sh, t, i, pay, n_src, dst, isize));
		}
		BGZI_BARRIER();
		const uint32_t done = Sh.done;
		BGZI_BARRIER();                                    /* every lane has read the batch's state before lane 0 starts the next */
		if (done) break;
		if (k >= max_batches) { BGZI_LANES(t, if (t == 0) Sh.status = BGZI_INTERNAL); BGZI_BARRIER(); break; }
	}
	BGZI_PHASE(t, bgzi_phase_crc(Sh, t, dst, isize));
	BGZI_PHASE(t, bgzi_phase_finish(Sh, t, crc, status));
}
