// bam_rec.hpp -- one BAM record of the bam2bam front-end: its bytes, parsing, the two tag walkers, the edits pass 2 makes and the read
// it encodes for the search.  Host only and free of the library's other headers: the records come from a socket as well as from files
// (nabwa_worker_process), so everything here runs on the CPU, under sanitizers, in tests/emu/bam_front_main.cpp.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <utility>
#include <vector>
#include "read_trim.hpp"

#define F_PD 1
#define F_PP 2
#define F_SU 4
#define F_MU 8
#define F_SR 16
#define F_MR 32
#define F_R1 64
#define F_R2 128
#define F_SC 256
#define F_QC 512
#define F_DP 1024

/* The bytes of one record.  They start out in the batch's arena, with room for what pass 2 adds (a million records = one
 * allocation, not a million), and move to the heap only if they outgrow that room. */
struct RecBuf {
	uint8_t *p; uint32_t n, cap; bool heap;
	RecBuf() : p(0), n(0), cap(0), heap(false) {}
	~RecBuf() { if (heap) free(p); }
	RecBuf(const RecBuf&) = delete;
	RecBuf &operator=(const RecBuf&) = delete;
	RecBuf(RecBuf &&o) noexcept : p(o.p), n(o.n), cap(o.cap), heap(o.heap) { o.p = 0; o.n = o.cap = 0; o.heap = false; }
	RecBuf &operator=(RecBuf &&o) noexcept
	{
		if (this != &o) { if (heap) free(p); p = o.p; n = o.n; cap = o.cap; heap = o.heap; o.p = 0; o.n = o.cap = 0; o.heap = false; }
		return *this;
	}
	uint8_t *data() { return p; }
	const uint8_t *data() const { return p; }
	size_t size() const { return n; }
	bool empty() const { return n == 0; }
	void place(uint8_t *at, size_t room, const uint8_t *src, size_t len) { if (heap) free(p); p = at; cap = (uint32_t)room; heap = false; n = (uint32_t)len; if (len) memcpy(p, src, len); }
	void grow(size_t need)
	{
		const size_t nc = need > 2 * (size_t)cap + 64 ? need : 2 * (size_t)cap + 64;
		uint8_t *q = (uint8_t*)malloc(nc);
		if (!q) throw std::bad_alloc();
		if (n) memcpy(q, p, n);
		if (heap) free(p);
		p = q; cap = (uint32_t)nc; heap = true;
	}
	void resize(size_t m) { if (m > cap) grow(m); n = (uint32_t)m; }
	void append(const void *b, size_t len) { if ((size_t)n + len > cap) grow((size_t)n + len); memcpy(p + n, b, len); n += (uint32_t)len; }
};
#define REC_ROOM 160u              /* bytes of room behind a record for the tags and the CIGAR pass 2 adds */

struct BamRec {                    /* one record, parsed: offsets are into `data` (everything after the 32 bytes of core) */
	int32_t tid, pos; uint32_t bin, mapq, l_qname, flag, n_cigar; int32_t l_qseq, mtid, mpos, isize;
	RecBuf data;                   /* qname, cigar, seq, qual, tags */
	const uint8_t *rg_p; uint32_t rg_n;      /* its read group (bam_get_rg), a view into data: found while the record is being parsed */
	size_t off_cigar() const { return l_qname; }
	size_t off_seq() const { return l_qname + 4 * (size_t)n_cigar; }
	size_t off_qual() const { return off_seq() + ((size_t)l_qseq + 1) / 2; }
	size_t off_aux() const { return off_qual() + (size_t)l_qseq; }
};

static inline bool parse_rec(const uint8_t *p, int64_t len, BamRec &r, uint8_t *room)       /* room: len - 36 + REC_ROOM bytes of the arena */
{
	if (len < 36) return false;
	uint32_t bs; memcpy(&bs, p, 4);
	if ((int64_t)bs + 4 != len || bs < 32) return false;
	uint32_t y, z;
	memcpy(&r.tid, p + 4, 4); memcpy(&r.pos, p + 8, 4); memcpy(&y, p + 12, 4); memcpy(&z, p + 16, 4);
	memcpy(&r.l_qseq, p + 20, 4); memcpy(&r.mtid, p + 24, 4); memcpy(&r.mpos, p + 28, 4); memcpy(&r.isize, p + 32, 4);
	r.bin = y >> 16; r.mapq = y >> 8 & 0xff; r.l_qname = y & 0xff; r.flag = z >> 16; r.n_cigar = z & 0xffff;
	r.data.place(room, (size_t)(len - 36) + REC_ROOM, p + 36, (size_t)(len - 36));
	if (r.l_qseq < 0 || r.off_aux() > r.data.size() || r.l_qname == 0) return false;
	if (r.data.data()[r.l_qname - 1] != 0) return false;        /* the name is compared as a C string (mates, bwaseqio.c:366): it must end inside l_qname */
	return true;
}

/* erase_unwanted_tags (bwaseqio.c:413-464): AM NM CM SM MD X0 X1 XA XC XG XM XN XO XT YQ go, everything else stays */
static inline bool erase_tags(BamRec &r)
{
	size_t p = r.off_aux(), q = p; const size_t end = r.data.size();
	uint8_t *d = r.data.data();
	while (p < end) {
		if (p + 3 > end) return false;
		bool keep = true;
		switch (d[p]) {
			case 'A': case 'S': case 'C': case 'N': keep = d[p + 1] != 'M'; break;
			case 'M': keep = d[p + 1] != 'D'; break;
			case 'X': keep = !(d[p + 1] && strchr("01ACGMNOT", d[p + 1])); break;
			case 'Y': keep = d[p + 1] != 'Q'; break;
		}
		size_t len = 3;
		switch (d[p + 2] & ~32) {
			case 'C': case 'A': len += 1; break;
			case 'S': len += 2; break;
			case 'I': case 'F': len += 4; break;
			case 'D': len += 8; break;
			case 'Z': case 'H': while (p + len < end && d[p + len]) ++len; ++len; break;
			case 'B': {
				if (p + 8 > end) return false;
				const size_t count = (size_t)d[p + 4] | (size_t)d[p + 5] << 8 | (size_t)d[p + 6] << 16 | (size_t)d[p + 7] << 24;
				len += 5;
				switch (d[p + 3] & ~32) { case 'C': case 'A': len += count; break; case 'S': len += 2 * count; break;
										  case 'I': case 'F': len += 4 * count; break; case 'D': len += 8 * count; break; }
				break;
			}
		}
		if (p + len > end) return false;
		if (keep) { memmove(d + q, d + p, len); q += len; }
		p += len;
	}
	r.data.resize(q);
	return true;
}

/* bam_get_rg (bamlite.c:157-190): the read group of a record, "" when it has none */
static inline std::pair<const uint8_t*, size_t> get_rg(const BamRec &r)       /* a view into the record */
{
	size_t p = r.off_aux(); const size_t end = r.data.size(); const uint8_t *d = r.data.data();
	while (p + 4 < end) {
		if (d[p] == 'R' && d[p + 1] == 'G') {
			if (d[p + 2] == 'Z') return { d + p + 3, strnlen((const char*)d + p + 3, end - p - 3) };
			if (d[p + 2] == 'A') return { d + p + 3, (size_t)1 };
		}
		switch (d[p + 2]) {
			case 'A': case 'C': case 'c': p += 4; break;
			case 'S': case 's': p += 5; break;
			case 'I': case 'i': case 'f': p += 7; break;
			case 'd': p += 11; break;
			case 'Z': case 'H': p += 3; while (p < end && d[p]) ++p; ++p; break;
			case 'B': {
				if (p + 8 > end) return { d, (size_t)0 };
				const size_t count = (size_t)d[p + 4] | (size_t)d[p + 5] << 8 | (size_t)d[p + 6] << 16 | (size_t)d[p + 7] << 24;
				size_t w = 1; switch (d[p + 3]) { case 's': case 'S': w = 2; break; case 'i': case 'I': case 'f': w = 4; break; case 'd': w = 8; break; }
				p += 8 + w * count; break;
			}
			default: return { d, (size_t)0 };
		}
	}
	return { d, (size_t)0 };
}

static constexpr int nib4(int v) { return ((v & 1) << 3) | ((v & 2) << 1) | ((v & 4) >> 1) | ((v & 8) >> 3); }   /* complement of a 4-bit base code = its bits reversed */

/* both nibbles of a byte complemented (nib4), in place and swapped; filled by the compiler: one table in the program, no constructor at start-up */
struct NibComp {
	uint8_t same[256], swap[256];
	constexpr NibComp() : same(), swap()
	{
		for (int x = 0; x < 256; ++x) { const int hi = nib4(x >> 4), lo = nib4(x & 15); same[x] = (uint8_t)(hi << 4 | lo); swap[x] = (uint8_t)(lo << 4 | hi); }
	}
};
inline constexpr NibComp nib_comp{};

/* revcom_bam1 (bam2bam.c:335-362): flip the strand flag, reverse-complement SEQ, reverse QUAL */
static inline void revcom_rec(BamRec &r)
{
	r.flag ^= F_SR;
	const int L = r.l_qseq;
	uint8_t *s = r.data.data() + r.off_seq(), *q = r.data.data() + r.off_qual();
	/* byte by byte: with an even number of bases the bytes change places and their nibbles with them; with an odd number every byte of the
	 * result is put together from two neighbours (base L-1 sits alone in the top of the last byte, and the new last byte ends in a zero nibble) */
	const int nb = (L + 1) / 2;
	if (!(L & 1)) {
		int a = 0, b = nb - 1;
		for (; a < b; ++a, --b) { const uint8_t x = nib_comp.swap[s[a]], y = nib_comp.swap[s[b]]; s[a] = y; s[b] = x; }
		if (a == b) s[a] = nib_comp.swap[s[a]];
	} else if (nb) {
		uint8_t small[256]; std::vector<uint8_t> big;
		uint8_t *c = small;
		if (nb > (int)sizeof(small)) { big.resize((size_t)nb); c = big.data(); }
		for (int j = 0; j < nb; ++j) c[j] = nib_comp.same[s[j]];
		const int m = nb - 1;
		for (int j = 0; j < m; ++j) s[j] = (uint8_t)((c[m - j] & 0xF0) | (c[m - j - 1] & 0x0F));
		s[m] = (uint8_t)(c[0] & 0xF0);
	}
	for (int a = 0, b = L - 1; a < b; ++a, --b) { const uint8_t t = q[a]; q[a] = q[b]; q[b] = t; }
}

static inline uint32_t reg2bin(uint32_t beg, uint32_t end)      /* bam_reg2bin (bam2bam.c:324-333) */
{
	--end;
	if (beg >> 14 == end >> 14) return 4681 + (beg >> 14);
	if (beg >> 17 == end >> 17) return 585 + (beg >> 17);
	if (beg >> 20 == end >> 20) return 73 + (beg >> 20);
	if (beg >> 23 == end >> 23) return 9 + (beg >> 23);
	if (beg >> 26 == end >> 26) return 1 + (beg >> 26);
	return 0;
}

static inline void push_int(BamRec &r, char u, char v, int x) { const uint8_t b[7] = { (uint8_t)u, (uint8_t)v, 'i', (uint8_t)x, (uint8_t)(x >> 8), (uint8_t)(x >> 16), (uint8_t)(x >> 24) }; r.data.append(b, 7); }
static inline void push_char(BamRec &r, char u, char v, char c) { const uint8_t b[4] = { (uint8_t)u, (uint8_t)v, 'A', (uint8_t)c }; r.data.append(b, 4); }
static inline void push_str(BamRec &r, char u, char v, const char *s) { const uint8_t b[3] = { (uint8_t)u, (uint8_t)v, 'Z' }; r.data.append(b, 3); r.data.append(s, strlen(s) + 1); }

static inline void set_cigar(BamRec &r, int n, const uint32_t *c)       /* bam_resize_cigar + the copy (bam2bam.c:411-420,467-477) */
{
	const size_t at = r.off_cigar(), old_b = 4 * (size_t)r.n_cigar, new_b = 4 * (size_t)n, tail = r.data.size() - at - old_b;
	if (new_b > old_b) { r.data.resize(r.data.size() + (new_b - old_b)); memmove(r.data.data() + at + new_b, r.data.data() + at + old_b, tail); }
	else if (new_b < old_b) { memmove(r.data.data() + at + new_b, r.data.data() + at + old_b, tail); r.data.resize(r.data.size() - (old_b - new_b)); }
	if (n) memcpy(r.data.data() + at, c, new_b);
	r.n_cigar = (uint32_t)n;
}

static inline void write_rec(const BamRec &r, uint8_t *o)
{
	const uint32_t bs = 32 + (uint32_t)r.data.size();
	const uint32_t y = r.bin << 16 | (r.mapq & 0xff) << 8 | (r.l_qname & 0xff), z = r.flag << 16 | (r.n_cigar & 0xffff);
	uint8_t h[36];
	memcpy(h, &bs, 4); memcpy(h + 4, &r.tid, 4); memcpy(h + 8, &r.pos, 4); memcpy(h + 12, &y, 4); memcpy(h + 16, &z, 4);
	memcpy(h + 20, &r.l_qseq, 4); memcpy(h + 24, &r.mtid, 4); memcpy(h + 28, &r.mpos, 4); memcpy(h + 32, &r.isize, 4);
	memcpy(o, h, 36); if (!r.data.empty()) memcpy(o + 36, r.data.data(), r.data.size());
}

/* ------------------------------------------------------------------ the read of a record (bam1_to_seq, bwaseqio.c:272-307) */

inline constexpr uint8_t nt16_nt4[16] = { 4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4 };      /* bam_nt16_nt4_table (bwaseqio.c:10) */
/* the two bases of a byte at once, as they lie in a REVERSED read (the later base first), plain and complemented: one 16-bit store per strand for two bases */
struct Nt16Rev {
	uint16_t s[256], r[256];
	constexpr Nt16Rev() : s(), r()
	{
		for (int x = 0; x < 256; ++x) {
			const int a = nt16_nt4[x >> 4], b = nt16_nt4[x & 15];
			s[x] = (uint16_t)(b | a << 8); r[x] = (uint16_t)((b < 4 ? 3 - b : b) | (a < 4 ? 3 - a : a) << 8);
		}
	}
};
inline constexpr Nt16Rev nt16_rev{};

/* bwa_trim_read (bwaseqio.c:110-123) on phred + 33 capped at 126, in the read's own orientation: the length that is searched */
static inline int rec_trimmed_len(const BamRec &x, int trim_qual)
{
	const int L = x.l_qseq;
	if (trim_qual < 1) return L;
	const bool rev = (x.flag & F_SR) != 0;
	const uint8_t *ql = x.data.data() + x.off_qual();
	return bwa_trimmed_len(L, trim_qual, [=](int l) { const int q = ql[rev ? L - 1 - l : l]; return q + 33 < 126 ? q : 93; });
}

/* the first `len` bases of the read in its own orientation -- a record that carries the reverse flag holds the reverse complement
 * (bwaseqio.c:288-291) -- as the search takes them: s = the (trimmed) read reversed, r = its complement (bwaseqio.c:294-297) */
static inline void rec_encode(const BamRec &x, int len, uint8_t *s, uint8_t *r)
{
	const int L = x.l_qseq;
	const uint8_t *sq = x.data.data() + x.off_seq();
	if (!(x.flag & F_SR)) {
		/* s[j] = code of base len-1-j; a byte of the record holds bases 2m (high nibble) and 2m+1: both codes from one table look-up,
		 * written back to front */
		int k = 0;
		for (; k + 1 < len; k += 2) {          /* bases k, k + 1 go to places len-1-k, len-2-k: the two bytes at len-2-k, the later base first */
			const uint8_t b = sq[k >> 1];
			memcpy(s + (len - 2 - k), &nt16_rev.s[b], 2);
			memcpy(r + (len - 2 - k), &nt16_rev.r[b], 2);
		}
		if (k < len) { const uint8_t v = nt16_nt4[sq[k >> 1] >> 4]; s[len - 1 - k] = v; r[len - 1 - k] = v < 4 ? 3 - v : v; }
	} else for (int j = 0; j < len; ++j) {
		const int k = len - 1 - j, jj = L - 1 - k;
		uint8_t v = nt16_nt4[sq[jj >> 1] >> ((~jj & 1) << 2) & 15];
		if (v < 4) v = 3 - v;
		s[j] = v; r[j] = v < 4 ? 3 - v : v;
	}
}
