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
//
// The dynamic mode (bgzf_deflate_dyn_kernel) runs the same load, parse and scan, so a slice has the same tokens in both modes, and then
//   count    the tokens' histogram of the 286 literal/length and the 30 distance symbols (LDS atomics), the extra bits summed
//   sort     the used symbols of both alphabets ranked by (frequency, symbol): all lanes, n^2 / 64 comparisons each
//   header   lane 0: the two length-limited codes (a two-queue merge of <= 2 * 286 steps, the 15-bit limit enforced on the counts per
//            length), their lengths run-length coded as zlib's scan_tree does, the 7-bit code of that sequence, the block's exact size;
//            the block is dynamic only if its payload is strictly smaller than what the scan chose, else the fixed mode's block is
//            written byte for byte
//   measure  each lane's bits under the new codes; the slot zeroed up to the new payload
//   offsets  lane 0: the lanes' bit offsets behind the header
//   emit     lane 0 the block header, the tables and the end-of-block code, every lane its codes
// Its tables (BgzfDyn) live where the hash table was: the parse is over.  Its loops are bounded by the alphabet's size, twice that, or the slice.
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
#define BGZF_ADD(p, v)         atomicAdd((p), (v))
#define BGZF_LOG2(x)           (31u - (uint32_t)__clz((int)(x)))
#define BGZF_BREV(x)           __brev(x)
#else
#define BGZF_FN                static inline
#define BGZF_OR(p, v)          (*(p) |= (v))
#define BGZF_XOR(p, v)         (*(p) ^= (v))
#define BGZF_ADD(p, v)         (*(p) += (v))
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

/* ================================================================== dynamic Huffman blocks (BTYPE 10) */
#define BGZF_NLL      286u
#define BGZF_ND       30u
#define BGZF_NCL      19u
#define BGZF_EOB      256u

struct __attribute__((may_alias)) BgzfDyn {            /* 7 316 bytes in place of BgzfShared::head, which is dead once the parse is over */
	uint32_t ll_freq[288], d_freq[32], cl_freq[20];
	uint32_t nf[2 * 288];                              /* the merge: leaves in rising order, then the nodes made of them */
	uint32_t blc[16], next[16];                        /* symbols per length, the first code of a length */
	uint32_t extra, dynamic, hdr_bits, hlit, hdist, hclen, n_seq, pad;
	uint16_t par[2 * 288];                             /* a node's parent, then its depth */
	uint16_t ll_ord[288], d_ord[32], cl_ord[20];       /* the used symbols by rising (frequency, symbol) */
	uint16_t ll_code[288], d_code[32], cl_code[20];    /* bit-reversed, as they are sent */
	uint16_t seq[320];                                 /* the coded length sequence: symbol | extra value << 5 */
	uint8_t ll_len[288], d_len[32], cl_len[20];
};
static_assert(sizeof(BgzfDyn) <= sizeof(((BgzfShared*)0)->head), "the dynamic mode's tables live in the hash table's place");

BGZF_FN BgzfDyn &bgzf_dyn(BgzfShared &Sh) { return *(BgzfDyn*)Sh.head; }

/* the order in which the code-length code's lengths are sent: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 */
BGZF_FN uint32_t bgzf_cl_perm(uint32_t i)
{
	if (i < 3) return 16 + i;
	if (i == 3) return 0;
	const uint32_t j = i - 4;
	return (j & 1u) ? 7 - (j >> 1) : 8 + (j >> 1);
}

/* ord[r] = the used symbol with r used symbols before it in the order of (frequency, symbol); lanes t, t + step, ... take a symbol each */
BGZF_FN void bgzf_rank_sort(const uint32_t *f, uint32_t n, uint16_t *ord, uint32_t t, uint32_t step)
{
	for (uint32_t s = t; s < n; s += step) {
		const uint32_t fs = f[s];
		if (!fs) continue;
		uint32_t r = 0;
		for (uint32_t j = 0; j < n; ++j) { const uint32_t fj = f[j]; r += (uint32_t)((fj != 0) & ((fj < fs) | ((fj == fs) & (j < s)))); }
		ord[r] = (uint16_t)s;                          /* r < the number of used symbols <= n */
	}
}

/* one lane.  Code lengths of at most `limit` bits for the n <= 286 symbols of frequencies f (ord: bgzf_rank_sort's), a complete code
 * (Kraft sum 1) with at least two symbols: no used symbol -> symbols 0 and 1 get one bit, one -> it and a neighbour.  len is all zero
 * on entry.  2^limit >= n.  A function of f alone. */
BGZF_FN void bgzf_build_lengths(BgzfDyn &D, const uint32_t *f, uint32_t n, uint32_t limit, const uint16_t *ord, uint8_t *len)
{
	uint32_t m = 0;
	for (uint32_t j = 0; j < n; ++j) m += f[j] != 0;
	if (m == 0) { len[0] = len[1] = 1; return; }
	if (m == 1) { const uint32_t s = ord[0]; len[s] = 1; len[s ? s - 1 : 1] = 1; return; }
	/* Huffman's merge on two queues: the leaves 0 .. m - 1 in rising order, the nodes m .. 2 m - 2 in the order they are made, which is
	 * rising too.  m - 1 steps; a node's parent has the larger index */
	for (uint32_t i = 0; i < m; ++i) D.nf[i] = f[ord[i]];
	uint32_t li = 0, ii = m, ni = m;
	for (uint32_t k = 0; k + 1 < m; ++k) {
		uint32_t sum = 0;
		for (int w = 0; w < 2; ++w) {
			uint32_t x;
			if (li < m && (ii >= ni || D.nf[li] <= D.nf[ii])) x = li++; else x = ii++;
			const uint32_t v = D.nf[x];
			sum = sum + v < sum ? 0xffffffffu : sum + v;      /* saturated: any merge order is a prefix code */
			D.par[x] = (uint16_t)ni;
		}
		D.nf[ni++] = sum;
	}
	D.par[2 * m - 2] = 0;                              /* the root's depth; below it a parent's entry is its depth already */
	for (uint32_t i = 2 * m - 2; i-- > 0; ) D.par[i] = (uint16_t)(D.par[D.par[i]] + 1);
	for (uint32_t l = 0; l <= limit; ++l) D.blc[l] = 0;
	for (uint32_t i = 0; i < m; ++i) { const uint32_t d = D.par[i]; ++D.blc[d < limit ? d : limit]; }
	/* the Kraft sum in units of 2^-limit is 2^limit + over, over < the number of leaves that were cut short.  zlib's step takes one
	 * unit off: a leaf of the longest length below the limit goes down one, and a leaf from the limit comes up to be its sibling */
	uint32_t kraft = 0;
	for (uint32_t l = 1; l <= limit; ++l) kraft += D.blc[l] << (limit - l);
	uint32_t over = kraft > (1u << limit) ? kraft - (1u << limit) : 0;
	if (over > m) over = m;                            /* cannot be; the loop's bound */
	for (; over > 0; --over) {
		uint32_t l = limit - 1;
		while (l > 1 && D.blc[l] == 0) --l;
		if (D.blc[l] == 0 || D.blc[limit] == 0) break;  /* cannot be */
		--D.blc[l]; D.blc[l + 1] += 2; --D.blc[limit];
	}
	uint32_t at = 0;                                   /* the longest codes to the rarest symbols */
	for (uint32_t l = limit; l >= 1; --l)
		for (uint32_t c = D.blc[l]; c > 0 && at < m; --c) len[ord[at++]] = (uint8_t)l;
}

/* one lane.  RFC 1951 3.2.2: codes of one length are consecutive, a shorter length's come first; sent from the top bit */
BGZF_FN void bgzf_assign_codes(BgzfDyn &D, const uint8_t *len, uint32_t n, uint16_t *code)
{
	for (uint32_t l = 0; l < 16; ++l) D.blc[l] = 0;
	for (uint32_t s = 0; s < n; ++s) ++D.blc[len[s]];
	uint32_t c = 0;
	D.blc[0] = 0;
	for (uint32_t l = 1; l < 16; ++l) { c = (c + D.blc[l - 1]) << 1; D.next[l] = c; }
	for (uint32_t s = 0; s < n; ++s) {
		const uint32_t l = len[s];
		code[s] = l ? (uint16_t)(BGZF_BREV(D.next[l]++) >> (32 - l)) : 0;
	}
}

/* one lane.  The lengths len[0, n) run-length coded as zlib's scan_tree and send_tree do, appended to D.seq at `at`; -> the new end.
 * At most n entries */
BGZF_FN uint32_t bgzf_rle(BgzfDyn &D, const uint8_t *len, uint32_t n, uint32_t at)
{
	uint32_t prev = 0xffffu, next = len[0], count = 0, maxc = next ? 7 : 138, minc = next ? 4 : 3;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t cur = next;
		next = i + 1 < n ? len[i + 1] : 0xffffu;
		if (++count < maxc && cur == next) continue;
		if (count < minc) {
			for (; count > 0; --count) { D.seq[at++] = (uint16_t)cur; ++D.cl_freq[cur]; }
		} else if (cur != 0) {
			if (cur != prev) { D.seq[at++] = (uint16_t)cur; ++D.cl_freq[cur]; --count; }
			D.seq[at++] = (uint16_t)(16u | (count - 3) << 5); ++D.cl_freq[16];
		} else if (count <= 10) {
			D.seq[at++] = (uint16_t)(17u | (count - 3) << 5); ++D.cl_freq[17];
		} else {
			D.seq[at++] = (uint16_t)(18u | (count - 11) << 5); ++D.cl_freq[18];
		}
		count = 0; prev = cur;
		if (next == 0) { maxc = 138; minc = 3; } else if (cur == next) { maxc = 6; minc = 3; } else { maxc = 7; minc = 4; }
	}
	return at;
}

/* ------------------------------------------------------------------ clear (beside the scan: the hash table is dead) */
BGZF_FN void bgzf_dyn_phase_clear(BgzfShared &Sh, uint32_t t)
{
	uint32_t *w = (uint32_t*)&bgzf_dyn(Sh);
	for (uint32_t i = t; i < sizeof(BgzfDyn) / 4; i += BGZF_LANES) w[i] = 0;
}

/* ------------------------------------------------------------------ count */
BGZF_FN void bgzf_dyn_phase_count(BgzfShared &Sh, uint32_t t, uint32_t n)
{
	BgzfDyn &D = bgzf_dyn(Sh);
	const uint8_t *b = (const uint8_t*)Sh.in;
	uint32_t s0, s1; bgzf_segment(n, t, s0, s1);
	uint32_t p = s0, extra = 0;
	while (p < s1) {
		if ((Sh.mstart[p >> 5] >> (p & 31u)) & 1u) {
			const uint32_t l = Sh.tok[p], d = (uint32_t)Sh.tok[p + 1] | ((uint32_t)Sh.tok[p + 2] << 8);
			uint32_t sym, e;
			bgzf_len_sym(l, sym, e); extra += e;
			BGZF_ADD(&D.ll_freq[257 + sym], 1u);
			bgzf_dist_sym(d, sym, e); extra += e;
			BGZF_ADD(&D.d_freq[sym], 1u);
			p += l + 3;
		} else {
			BGZF_ADD(&D.ll_freq[b[p]], 1u);
			++p;
		}
	}
	if (extra) BGZF_ADD(&D.extra, extra);
	if (t == 0) BGZF_ADD(&D.ll_freq[BGZF_EOB], 1u);
}

/* ------------------------------------------------------------------ sort */
BGZF_FN void bgzf_dyn_phase_sort(BgzfShared &Sh, uint32_t t)
{
	BgzfDyn &D = bgzf_dyn(Sh);
	bgzf_rank_sort(D.ll_freq, BGZF_NLL, D.ll_ord, t, BGZF_LANES);
	bgzf_rank_sort(D.d_freq, BGZF_ND, D.d_ord, t, BGZF_LANES);
}

/* ------------------------------------------------------------------ header (lane 0): the codes, the coded lengths, the size, the choice */
BGZF_FN void bgzf_dyn_phase_header(BgzfShared &Sh, uint32_t t)
{
	if (t != 0) return;
	BgzfDyn &D = bgzf_dyn(Sh);
	bgzf_build_lengths(D, D.ll_freq, BGZF_NLL, 15, D.ll_ord, D.ll_len);
	bgzf_build_lengths(D, D.d_freq, BGZF_ND, 15, D.d_ord, D.d_len);
	uint32_t hlit = BGZF_NLL, hdist = BGZF_ND;
	while (hlit > 257 && D.ll_len[hlit - 1] == 0) --hlit;
	while (hdist > 1 && D.d_len[hdist - 1] == 0) --hdist;
	uint32_t n_seq = bgzf_rle(D, D.ll_len, hlit, 0);      /* a run ends with the literal/length lengths */
	n_seq = bgzf_rle(D, D.d_len, hdist, n_seq);
	bgzf_rank_sort(D.cl_freq, BGZF_NCL, D.cl_ord, 0, 1);
	bgzf_build_lengths(D, D.cl_freq, BGZF_NCL, 7, D.cl_ord, D.cl_len);
	uint32_t hclen = BGZF_NCL;
	while (hclen > 4 && D.cl_len[bgzf_cl_perm(hclen - 1)] == 0) --hclen;
	uint32_t hdr = 3 + 14 + 3 * hclen + 2 * D.cl_freq[16] + 3 * D.cl_freq[17] + 7 * D.cl_freq[18];
	for (uint32_t s = 0; s < BGZF_NCL; ++s) hdr += D.cl_freq[s] * D.cl_len[s];
	uint32_t body = D.extra;                           /* the codes, the end of block among them, and the extra bits */
	for (uint32_t s = 0; s < BGZF_NLL; ++s) body += D.ll_freq[s] * D.ll_len[s];
	for (uint32_t s = 0; s < BGZF_ND; ++s) body += D.d_freq[s] * D.d_len[s];
	const uint32_t payload = (hdr + body + 7) >> 3;
	D.hlit = hlit; D.hdist = hdist; D.hclen = hclen; D.n_seq = n_seq; D.hdr_bits = hdr;
	D.dynamic = payload < Sh.payload;
	if (!D.dynamic) return;                            /* the scan's block stands: Sh.bits, Sh.fixed and Sh.payload are the fixed mode's */
	Sh.payload = payload;
	bgzf_assign_codes(D, D.ll_len, BGZF_NLL, D.ll_code);
	bgzf_assign_codes(D, D.d_len, BGZF_ND, D.d_code);
	bgzf_assign_codes(D, D.cl_len, BGZF_NCL, D.cl_code);
}

/* ------------------------------------------------------------------ measure, and the slot's words zeroed */
BGZF_FN void bgzf_dyn_phase_measure(BgzfShared &Sh, uint32_t t, uint32_t n, uint32_t *ow)
{
	BgzfDyn &D = bgzf_dyn(Sh);
	if (!D.dynamic) { bgzf_phase_zero(Sh, t, ow); return; }
	const uint32_t words = (18 + Sh.payload + 8 + 3) / 4;
	for (uint32_t i = t; i < words; i += BGZF_LANES) ow[i] = 0;
	const uint8_t *b = (const uint8_t*)Sh.in;
	uint32_t s0, s1; bgzf_segment(n, t, s0, s1);
	uint32_t p = s0, nbits = 0;
	while (p < s1) {
		if ((Sh.mstart[p >> 5] >> (p & 31u)) & 1u) {
			const uint32_t l = Sh.tok[p], d = (uint32_t)Sh.tok[p + 1] | ((uint32_t)Sh.tok[p + 2] << 8);
			uint32_t sym, e;
			bgzf_len_sym(l, sym, e); nbits += D.ll_len[257 + sym] + e;
			bgzf_dist_sym(d, sym, e); nbits += D.d_len[sym] + e;
			p += l + 3;
		} else {
			nbits += D.ll_len[b[p]];
			++p;
		}
	}
	Sh.bits[t] = nbits;
}

/* ------------------------------------------------------------------ offsets (lane 0) */
BGZF_FN void bgzf_dyn_phase_offsets(BgzfShared &Sh, uint32_t t)
{
	if (t != 0 || !bgzf_dyn(Sh).dynamic) return;
	uint32_t acc = 0;
	for (uint32_t i = 0; i < BGZF_LANES; ++i) { const uint32_t v = Sh.bits[i]; Sh.bits[i] = acc; acc += v; }
	Sh.total_bits = acc;
}

/* ------------------------------------------------------------------ emit */
BGZF_FN void bgzf_dyn_phase_emit(BgzfShared &Sh, uint32_t t, uint32_t n, uint32_t *ow, uint32_t *size_out)
{
	BgzfDyn &D = bgzf_dyn(Sh);
	if (!D.dynamic) { bgzf_phase_emit(Sh, t, n, ow, size_out); return; }
	const uint8_t *b = (const uint8_t*)Sh.in;
	const uint32_t payload = Sh.payload, bsize = 18 + payload + 8 - 1, first = 144 + D.hdr_bits;      /* the first token's bit */
	BgzfBits w;
	w.ow = ow; w.b0 = t ? first + Sh.bits[t] : 144; w.b1 = first + (t + 1 < BGZF_LANES ? Sh.bits[t + 1] : Sh.total_bits);
	w.wi = w.b0 >> 5; w.cnt = w.b0 & 31u; w.acc = 0;
	if (t == 0) {
		*size_out = bsize + 1;
		ow[0] = 0x04088b1fu; ow[1] = 0; ow[2] = 0x0006ff00u; ow[3] = 0x00024342u;
		BGZF_OR(&ow[4], bsize);
		bgzf_or32(ow, (18 + payload) * 8, Sh.crc);
		bgzf_or32(ow, (18 + payload) * 8 + 32, n);
		bgzf_or32(ow, first + Sh.total_bits, D.ll_code[BGZF_EOB]);      /* ends before the CRC's bytes: both words are the slot's */
		bgzf_put(w, 5, 3);                             /* BFINAL = 1, BTYPE = 10 */
		bgzf_put(w, D.hlit - 257, 5); bgzf_put(w, D.hdist - 1, 5); bgzf_put(w, D.hclen - 4, 4);
		for (uint32_t i = 0; i < D.hclen; ++i) bgzf_put(w, D.cl_len[bgzf_cl_perm(i)], 3);
		for (uint32_t i = 0; i < D.n_seq; ++i) {
			const uint32_t s = D.seq[i] & 31u, x = D.seq[i] >> 5;
			bgzf_put(w, D.cl_code[s], D.cl_len[s]);
			if (s >= 16) bgzf_put(w, x, s == 16 ? 2 : s == 17 ? 3 : 7);
		}
	}
	uint32_t s0, s1; bgzf_segment(n, t, s0, s1);
	uint32_t p = s0;
	while (p < s1) {
		if ((Sh.mstart[p >> 5] >> (p & 31u)) & 1u) {
			const uint32_t l = Sh.tok[p], d = (uint32_t)Sh.tok[p + 1] | ((uint32_t)Sh.tok[p + 2] << 8);
			uint32_t sym, e;
			bgzf_len_sym(l, sym, e);
			bgzf_put(w, D.ll_code[257 + sym], D.ll_len[257 + sym]);
			if (e) bgzf_put(w, l & ((1u << e) - 1), e);
			bgzf_dist_sym(d, sym, e);
			bgzf_put(w, D.d_code[sym], D.d_len[sym]);
			if (e) bgzf_put(w, d & ((1u << e) - 1), e);
			p += l + 3;
		} else {
			const uint32_t v = b[p];
			bgzf_put(w, D.ll_code[v], D.ll_len[v]);
			++p;
		}
	}
	if (w.acc) BGZF_OR(&ow[w.wi], (uint32_t)w.acc);
}
