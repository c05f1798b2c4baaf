// bgzf_deflate_body.hpp -- the per-slice body of the BGZF compressor (bgzf_deflate.hip): one slice of <= 0xff00 bytes becomes one
// BGZF block (RFC 1952 member with the BC field, RFC 1951 payload) in the block's 0x10000-byte slot of the staging area.
//
// One wavefront (a workgroup of 64 lanes) per slice: the lanes of one wave run in lockstep, so the order in which they enter and
// find positions in the shared hash table -- and with it every byte of the output -- is the same in every run; waves that raced for
// the table would make valid blocks that differ from call to call.  The body is a sequence of phases; a phase is a function of the
// lane number, and the kernel puts a barrier between two phases.  No phase waits for another lane, and every loop is bounded by the
// slice length, 258, the four candidates of a position or 32.  With BGZF_EMU defined (tests only, never part of libnabwa.so) g++ compiles the
// same phases, and a host loop over the lanes runs them one after the other: the kernel's indexing under AddressSanitizer.
//
//   load   the slice into LDS; hash heads, match bitmap and the CRC table are set up
//   parse  lane t owns the bytes [t * S, (t + 1) * S), S = max(ceil(n / 64), 272), 1020 for a full slice: their CRC-32, shifted to the slice's end and
//          folded into one word, then a greedy parse against the one hash table all lanes share (buckets of the two newest
//          positions of a 3-byte hash; the byte before and the last match's distance are tried as well, since the lanes' entries
//          crowd each other out of the table).  A candidate counts only if it lies before the position, within 32768, and its bytes
//          compare equal; a match ends with its lane's bytes, so the lanes' tokens concatenate into one stream.  The matches
//          are kept (a bitmap of their starts, length and distance in the three token bytes at the start), the bits counted.
//   scan   lane 0: the lanes' bit offsets; fixed Huffman if that is shorter than one stored block, else stored
//   zero   the words of the slot the block will cover (the emit phase ORs into them)
//   emit   the header, each lane's codes at its bit offset (words it owns alone are stored, shared ones ORed atomically),
//          CRC-32 and ISIZE; or the stored block, byte by byte
#pragma once
#include <stdint.h>

#define BGZF_SLICE    0xff00u
#define BGZF_STRIDE   0x10000u
#define BGZF_LANES    64u
#define BGZF_MINSEG   272u        /* a lane's bytes: at least 259, so that a match of 258 fits behind one literal */
#define BGZF_BUCKETS  4096u
#define BGZF_MAXLEN   258u
#define BGZF_MAXDIST  32768u
#define BGZF_FAR3     4096u       /* a match of 3 bytes further back than this costs more bits than its literals */

#ifndef BGZF_EMU
#define BGZF_FN                __device__ __forceinline__
#define BGZF_OR(p, v)          atomicOr((p), (v))
#define BGZF_XOR(p, v)         atomicXor((p), (v))
#define BGZF_LOG2(x)           (31u - (uint32_t)__clz((int)(x)))
#define BGZF_BREV(x)           __brev(x)
#else
#define BGZF_FN                static inline
#define BGZF_OR(p, v)          (*(p) |= (v))
#define BGZF_XOR(p, v)         (*(p) ^= (v))
#define BGZF_LOG2(x)           (31u - (uint32_t)__builtin_clz(x))
static inline uint32_t bgzf_emu_brev(uint32_t x) { uint32_t r = 0; for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i); return r; }
#define BGZF_BREV(x)           bgzf_emu_brev(x)
#endif

struct BgzfShared {                                    /* 156 400 bytes of the CU's 163 840 */
	uint32_t in[BGZF_SLICE / 4];                       /* the slice */
	uint8_t tok[BGZF_SLICE];                           /* at a match's start: length - 3, distance - 1 (two bytes) */
	uint32_t mstart[BGZF_SLICE / 32];                  /* bit p: a match starts at byte p */
	uint32_t head[BGZF_BUCKETS];                       /* the two newest positions of a hash, the newer in the low half; 0xffff: none */
	uint32_t crc_tab[256];
	uint32_t bits[BGZF_LANES];                         /* a lane's bit count, after the scan its bit offset */
	uint32_t crc, fixed, payload, total_bits;
};

BGZF_FN void bgzf_segment(uint32_t n, uint32_t t, uint32_t &s0, uint32_t &s1)
{
	uint32_t S = (n + BGZF_LANES - 1) / BGZF_LANES;
	if (S < BGZF_MINSEG) S = BGZF_MINSEG;
	s0 = t * S; if (s0 > n) s0 = n;
	s1 = s0 + S; if (s1 > n) s1 = n;
}

/* a * b modulo the CRC-32 polynomial, bit 31 the coefficient of x^0 (the CRC's reflected order) */
BGZF_FN uint32_t bgzf_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) {
		if (a & (0x80000000u >> i)) p ^= b;
		b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
	}
	return p;
}
/* x^(8 k) modulo the polynomial, k < 65536: the operator that moves a CRC over k bytes that follow it */
BGZF_FN uint32_t bgzf_shift_op(uint32_t k)
{
	uint32_t p = 0x80000000u, sq = 0x00800000u;        /* x^0, x^8 */
	for (int i = 0; i < 16; ++i) {
		if (k & 1u) p = bgzf_mulmod(sq, p);
		sq = bgzf_mulmod(sq, sq);
		k >>= 1;
	}
	return p;
}

/* deflate's length symbol for l = length - 3 (0..255): symbol - 257 (its fixed code: sym + 1 in 7 bits up to 279, then 0xc0 + sym - 23 in 8), and the number of extra bits */
BGZF_FN void bgzf_len_sym(uint32_t l, uint32_t &sym, uint32_t &e)
{
	if (l < 8) { sym = l; e = 0; return; }
	if (l == 255) { sym = 28; e = 0; return; }
	e = BGZF_LOG2(l) - 2;
	sym = 4 + (e << 2) + ((l >> e) & 3u);
}
/* the distance symbol for d = distance - 1 (0..32767) */
BGZF_FN void bgzf_dist_sym(uint32_t d, uint32_t &sym, uint32_t &e)
{
	if (d < 4) { sym = d; e = 0; return; }
	const uint32_t nb = BGZF_LOG2(d);
	e = nb - 1;
	sym = 2 * nb + ((d >> e) & 1u);
}
BGZF_FN uint32_t bgzf_match_bits(uint32_t l, uint32_t d)
{
	uint32_t ls, le, ds, de;
	bgzf_len_sym(l, ls, le); bgzf_dist_sym(d, ds, de);
	return (ls < 23 ? 7u : 8u) + le + 5u + de;          /* symbols 257..279 have 7 bits, 280..287 have 8 */
}

/* ------------------------------------------------------------------ load */
BGZF_FN void bgzf_phase_load(BgzfShared &Sh, uint32_t t, const uint32_t *src, uint32_t n)
{
	for (uint32_t i = t; i < (n + 3) / 4; i += BGZF_LANES) Sh.in[i] = src[i];
	for (uint32_t i = t; i < BGZF_BUCKETS; i += BGZF_LANES) Sh.head[i] = 0xffffffffu;
	for (uint32_t i = t; i < BGZF_SLICE / 32; i += BGZF_LANES) Sh.mstart[i] = 0;
	for (uint32_t i = t; i < 256; i += BGZF_LANES) {
		uint32_t c = i;
		for (int j = 0; j < 8; ++j) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1;
		Sh.crc_tab[i] = c;
	}
	if (t == 0) Sh.crc = 0;
}

/* ------------------------------------------------------------------ parse */
BGZF_FN void bgzf_phase_parse(BgzfShared &Sh, uint32_t t, uint32_t n)
{
	const uint8_t *b = (const uint8_t*)Sh.in;
	uint32_t s0, s1; bgzf_segment(n, t, s0, s1);
	/* crc(A B) = crc(A) * x^(8 |B|) + crc(B) on finished CRCs: each lane's moved to the end of the slice, the sum is the slice's */
	if (s1 > s0) {
		uint32_t c = 0xffffffffu;
		for (uint32_t p = s0; p < s1; ++p) c = Sh.crc_tab[(c ^ b[p]) & 0xffu] ^ (c >> 8);
		BGZF_XOR(&Sh.crc, bgzf_mulmod(bgzf_shift_op(n - s1), ~c));
	}
	uint32_t nbits = 0, p = s0, last = 1;
	while (p < s1) {
		uint32_t best = 0, bdist = 0;
		if (p + 3 <= s1) {
			const uint32_t h = ((((uint32_t)b[p] << 16) | ((uint32_t)b[p + 1] << 8) | b[p + 2]) * 0x9e3779b1u) >> 20;      /* 12 bits */
			const uint32_t e = Sh.head[h];
			Sh.head[h] = (e << 16) | p;
			const uint32_t lim = s1 - p < BGZF_MAXLEN ? s1 - p : BGZF_MAXLEN;
			for (int w = 0; w < 4; ++w) {                        /* the bucket's two, then the byte before (a run) and the last match's distance again */
				const uint32_t cand = w < 2 ? (e >> (16 * w)) & 0xffffu : w == 2 ? p - 1 : p - last;      /* p = 0: p - 1 wraps and fails the test below */
				if (cand < p && p - cand <= BGZF_MAXDIST) {      /* another lane may have entered a later position, or none is there (0xffff) */
					uint32_t l = 0;
					while (l < lim && b[cand + l] == b[p + l]) ++l;
					if (l > best) { best = l; bdist = p - cand; }
				}
			}
			if (best == 3 && bdist > BGZF_FAR3) best = 0;
		}
		if (best >= 3) {
			BGZF_OR(&Sh.mstart[p >> 5], 1u << (p & 31u));
			Sh.tok[p] = (uint8_t)(best - 3); Sh.tok[p + 1] = (uint8_t)(bdist - 1); Sh.tok[p + 2] = (uint8_t)((bdist - 1) >> 8);
			nbits += bgzf_match_bits(best - 3, bdist - 1);
			last = bdist;
			p += best;
		} else {
			nbits += b[p] < 144 ? 8u : 9u;
			++p;
		}
	}
	Sh.bits[t] = nbits;
}

/* ------------------------------------------------------------------ scan (lane 0) */
BGZF_FN void bgzf_phase_scan(BgzfShared &Sh, uint32_t t, uint32_t n)
{
	if (t != 0) return;
	uint32_t acc = 0;
	for (uint32_t i = 0; i < BGZF_LANES; ++i) { const uint32_t v = Sh.bits[i]; Sh.bits[i] = acc; acc += v; }
	const uint32_t fixed = (3 + acc + 7 + 7) >> 3, stored = n + 5;      /* BFINAL + BTYPE, the codes, end of block; or 00, LEN, NLEN, the bytes */
	Sh.total_bits = acc;
	Sh.fixed = fixed < stored;
	Sh.payload = fixed < stored ? fixed : stored;
}

/* ------------------------------------------------------------------ zero */
BGZF_FN void bgzf_phase_zero(BgzfShared &Sh, uint32_t t, uint32_t *ow)
{
	if (!Sh.fixed) return;
	const uint32_t words = (18 + Sh.payload + 8 + 3) / 4;
	for (uint32_t i = t; i < words; i += BGZF_LANES) ow[i] = 0;
}

/* ------------------------------------------------------------------ emit */
struct BgzfBits {                                      /* a lane's bits [b0, b1) of the slot: the words inside are its own */
	uint32_t *ow; uint32_t b0, b1, wi, cnt; uint64_t acc;
};
BGZF_FN void bgzf_put(BgzfBits &w, uint32_t v, uint32_t nb)      /* nb <= 18, cnt < 32 */
{
	w.acc |= (uint64_t)v << w.cnt; w.cnt += nb;
	if (w.cnt >= 32) {
		const uint32_t x = (uint32_t)w.acc;
		if (w.wi * 32 >= w.b0 && w.wi * 32 + 32 <= w.b1) w.ow[w.wi] = x; else BGZF_OR(&w.ow[w.wi], x);
		w.acc >>= 32; w.cnt -= 32; ++w.wi;
	}
}
BGZF_FN void bgzf_or32(uint32_t *ow, uint32_t bit, uint32_t v)      /* 32 bits at any bit position */
{
	const uint32_t sh = bit & 31u;
	BGZF_OR(&ow[bit >> 5], v << sh);
	if (sh) BGZF_OR(&ow[(bit >> 5) + 1], v >> (32 - sh));
}
BGZF_FN void bgzf_phase_emit(BgzfShared &Sh, uint32_t t, uint32_t n, uint32_t *ow, uint32_t *size_out)
{
	const uint8_t *b = (const uint8_t*)Sh.in;
	const uint32_t payload = Sh.payload, bsize = 18 + payload + 8 - 1, crc = Sh.crc;
	if (t == 0) *size_out = bsize + 1;
	if (!Sh.fixed) {                                   /* one stored block; every byte of the slot's block is stored once, none ORed */
		uint8_t *ob = (uint8_t*)ow;
		if (t == 0) {
			const uint8_t hdr[23] = { 31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8),
									  1, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8) };
			for (int i = 0; i < 23; ++i) ob[i] = hdr[i];
			for (int i = 0; i < 4; ++i) { ob[23 + n + i] = (uint8_t)(crc >> (8 * i)); ob[27 + n + i] = (uint8_t)(n >> (8 * i)); }
		}
		for (uint32_t i = t; i < n; i += BGZF_LANES) ob[23 + i] = b[i];
		return;
	}
	if (t == 0) {
		ow[0] = 0x04088b1fu; ow[1] = 0; ow[2] = 0x0006ff00u; ow[3] = 0x00024342u;
		BGZF_OR(&ow[4], bsize | (3u << 16));           /* BSIZE; BFINAL = 1, BTYPE = 01.  The end-of-block code is seven zero bits */
		bgzf_or32(ow, (18 + payload) * 8, crc);
		bgzf_or32(ow, (18 + payload) * 8 + 32, n);
	}
	uint32_t s0, s1; bgzf_segment(n, t, s0, s1);
	BgzfBits w;
	w.ow = ow; w.b0 = 147 + Sh.bits[t]; w.b1 = 147 + (t + 1 < BGZF_LANES ? Sh.bits[t + 1] : Sh.total_bits);
	w.wi = w.b0 >> 5; w.cnt = w.b0 & 31u; w.acc = 0;
	uint32_t p = s0;
	while (p < s1) {
		if ((Sh.mstart[p >> 5] >> (p & 31u)) & 1u) {
			const uint32_t l = Sh.tok[p], d = (uint32_t)Sh.tok[p + 1] | ((uint32_t)Sh.tok[p + 2] << 8);
			uint32_t sym, e;
			bgzf_len_sym(l, sym, e);
			if (sym < 23) bgzf_put(w, BGZF_BREV(sym + 1) >> 25, 7); else bgzf_put(w, BGZF_BREV(0xc0u + sym - 23) >> 24, 8);
			if (e) bgzf_put(w, l & ((1u << e) - 1), e);      /* a symbol's base is a multiple of 2^e above 3 */
			bgzf_dist_sym(d, sym, e);
			bgzf_put(w, BGZF_BREV(sym) >> 27, 5);
			if (e) bgzf_put(w, d & ((1u << e) - 1), e);
			p += l + 3;
		} else {
			const uint32_t v = b[p];
			if (v < 144) bgzf_put(w, BGZF_BREV(0x30u + v) >> 24, 8); else bgzf_put(w, BGZF_BREV(0x190u + v - 144) >> 23, 9);
			++p;
		}
	}
	if (w.acc) BGZF_OR(&ow[w.wi], (uint32_t)w.acc);
}
