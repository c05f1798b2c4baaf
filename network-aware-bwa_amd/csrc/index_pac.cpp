// index_pac.cpp -- the host half of `bwa index`: FASTA in, <prefix>.pac / .ann / .amb / .rpac out, byte for byte what
// the reference writes (bns_fasta2bntseq + bns_dump, bntseq.c:58-85,166-256; bwa_pac_rev_core, bwtmisc.c:168-193), and
// the colour-space conversion of `bwa index -c` (bwa_pac2cspac, bwtmisc.c:210-254).  No GPU is involved: the packed
// text these write is what nabwa_index_build (index_build.hip) turns into the FM-indexes.
//
// The reference's quirks are kept, because they are visible in the files:
//  * records are parsed as its kseq.h does (kseq.h:155-193), FASTA or FASTQ, plain or gzip: the name ends at the first
//    white space, the comment is the rest of the header line (a '\r' of a CRLF file included), only isgraph characters
//    enter the sequence, and a '>' '+' or '@' ends it wherever it stands;
//  * a record without a comment gets the comment of the last record that had one (kseq resets comment.l, not
//    comment.s, and bntseq.c:201 strdup()s comment.s), or "(null)" while no record had one;
//  * every base with nst_nt4_table >= 4 (IUPAC codes, 'n', '-', ...) becomes lrand48() & 3 from srand48(11), drawn in
//    input order; a hole (.amb) goes on only while the SAME character repeats, and never across records;
//  * .pac is always l_pac/4 + 2 bytes long: the packed bases, a zero byte when l_pac % 4 == 0, then l_pac % 4.
// Differences: nothing is written until the whole input has been read and accepted, so an empty input (the reference
// aborts in xassert, leaving an empty .pac) or one over 4 Gbp (refused after the .pac was written, bwtindex.c:103)
// leaves no files.  A first record without bases, on which the reference's kseq writes through a null pointer, is read
// as any other empty record.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <string>
#include <vector>
#include "nabwa_internal.hpp"
#include "../../include/nabwa.h"

namespace {

const unsigned char nt4[256] = {     // nst_nt4_table (bntseq.c:39-56): A C G T either case -> 0..3, '-' -> 5, the rest 4
	4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,  4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,
	4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 4, 4,  4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,
	4, 0, 4, 1, 4, 4, 4, 2, 4, 4, 4, 4, 4, 4, 4, 4,  4, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,
	4, 0, 4, 1, 4, 4, 4, 2, 4, 4, 4, 4, 4, 4, 4, 4,  4, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,
	4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,  4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,
	4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,  4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,
	4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,  4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,
	4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4,  4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4 };

// kstream_t over gzread (kseq.h:30-110).  Bytes come back as the reference's `char` does (signed): 0xFF reads as -1,
// which kseq takes for the end of the input exactly as it does there.
struct KStream {
	enum { BUFSIZE = 4096 };          // KSEQ_INIT(gzFile, gzread) -> KSTREAM_INIT(.., 4096); is_eof follows a short read
	gzFile f;
	char buf[BUFSIZE];
	int begin = 0, end = 0, is_eof = 0;
	bool refill()
	{
		begin = 0;
		end = gzread(f, buf, BUFSIZE);
		if (end < 0) end = 0;
		if (end < BUFSIZE) is_eof = 1;
		return end != 0;
	}
	int getc()
	{
		if (is_eof && begin >= end) return -1;
		if (begin >= end && !refill()) return -1;
		return (int)(signed char)buf[begin++];
	}
	// ks_getuntil (kseq.h:70-107): delimiter 0 = any white space.  Returns -1 without touching *s (but clearing the
	// length the caller sees) when the input had already ended; *s is only (re)assigned when the reference's
	// kstring would have been written.
	int getuntil(int delimiter, std::string *s, bool *assigned, int *dret)
	{
		if (dret) *dret = 0;
		if (begin >= end && is_eof) return -1;
		std::string acc;
		for (;;) {
			if (begin >= end) {
				if (!is_eof) { if (!refill()) break; } else break;
			}
			int i;
			if (delimiter) { for (i = begin; i < end; ++i) if (buf[i] == delimiter) break; }
			else { for (i = begin; i < end; ++i) { const unsigned char c = (unsigned char)buf[i]; if (c == ' ' || (c >= '\t' && c <= '\r')) break; } }
			acc.append(buf + begin, buf + i);
			begin = i + 1;
			if (i < end) { if (dret) *dret = buf[i]; break; }
		}
		*s = acc;
		if (assigned) *assigned = true;
		return (int)acc.size();
	}
};

static inline bool graph(int c) { return c >= 33 && c <= 126; }   // isgraph() in the C locale

// kseq_read (kseq.h:155-193): >= 0 the sequence length, -1 end of input, -2 truncated quality (ends the reference's loop)
struct KSeq {
	KStream ks;
	int last_char = 0;
	std::string name, comment, seq;
	bool has_comment = false;         // comment.s != NULL
	int64_t read()
	{
		int c;
		if (last_char == 0) {
			while ((c = ks.getc()) != -1 && c != '>' && c != '@') {}
			if (c == -1) return -1;
			last_char = c;
		}
		seq.clear();
		if (ks.getuntil(0, &name, nullptr, &c) < 0) return -1;
		if (c != '\n') ks.getuntil('\n', &comment, &has_comment, nullptr);
		while ((c = ks.getc()) != -1 && c != '>' && c != '+' && c != '@')
			if (graph(c)) seq.push_back((char)c);
		if (c == '>' || c == '@') last_char = c;
		if (c != '+') return (int64_t)seq.size();
		while ((c = ks.getc()) != -1 && c != '\n') {}
		if (c == -1) return -2;
		size_t ql = 0;
		while ((c = ks.getc()) != -1 && ql < seq.size())
			if (c >= 33 && c <= 127) ++ql;
		last_char = 0;
		if (ql != seq.size()) return -2;
		return (int64_t)seq.size();
	}
};

// lrand48 on a private state (the library's drand48 stream, finish_common.hpp, uses the same recurrence)
static inline int lrand48_on(uint64_t *x)
{
	*x = (*x * 0x5DEECE66DULL + 0xBULL) & 0xFFFFFFFFFFFFULL;
	return (int)(*x >> 17);
}

struct Packed {
	int64_t l_pac = 0;
	std::vector<nabwa_ann> anns;
	std::vector<std::string> annos;
	std::vector<nabwa_hole> holes;
	std::vector<uint8_t> pac;         // l_pac/4 + 2 bytes, the .pac file
};

static int fail_msg(int code, const std::string &m) { return nabwa_fail(code, "%s", m.c_str()); }

// the .pac convention: packed bytes (zero-padded to l_pac/4 + 1), then l_pac % 4 (bntseq.c:235-244, bwtmisc.c:186-191)
static void pac_tail(std::vector<uint8_t> &pac, int64_t l_pac)
{
	pac.resize((size_t)(l_pac / 4 + 1), 0);
	pac.push_back((uint8_t)(l_pac % 4));
}

static int read_fasta(const char *fasta, Packed &P)
{
	gzFile fp = gzopen(fasta, "r");
	if (!fp) return fail_msg(NABWA_EIO, std::string("cannot open '") + fasta + "'");
	KSeq ks; ks.ks.f = fp;
	uint64_t rng = ((uint64_t)11 << 16) | 0x330E;      // srand48(bns->seed = 11), bntseq.c:180-181
	int64_t l;
	P.pac.reserve(1 << 20);
	while ((l = ks.read()) >= 0) {
		if (l > 0x7fffffff) { gzclose(fp); return fail_msg(NABWA_EINVAL, "record '" + ks.name + "' is longer than 2^31 - 1 bases (bntann1_t.len is an int)"); }
		nabwa_ann a;
		a.name = ks.name.c_str();
		a.offset = P.anns.empty() ? 0 : P.anns.back().offset + P.anns.back().len;
		a.len = (int32_t)l; a.n_ambs = 0;
		const std::string anno = ks.has_comment ? std::string(ks.comment.c_str()) : std::string("(null)");
		int lasts = 0;
		for (int64_t i = 0; i < l; ++i) {
			const int ch = (unsigned char)ks.seq[i];
			int c = nt4[ch];
			if (c >= 4) {
				if (lasts == ch) ++P.holes.back().len;
				else { P.holes.push_back(nabwa_hole{ a.offset + i, 1, (char)ch }); ++a.n_ambs; }
				c = lrand48_on(&rng) & 3;
			}
			lasts = ch;
			const int64_t k = P.l_pac + i;
			if ((k & 3) == 0) P.pac.push_back(0);
			P.pac.back() |= (uint8_t)(c << ((3 - (k & 3)) << 1));
		}
		P.l_pac += l;
		P.anns.push_back(a); P.annos.push_back(anno);
	}
	gzclose(fp);
	if (P.l_pac == 0) return fail_msg(NABWA_EINVAL, std::string("'") + fasta + "' holds no bases (the reference aborts: zero length sequence)");
	if (P.l_pac > 0xffffffffLL)
		return fail_msg(NABWA_EINVAL, "the reference is longer than 4 Gbp in total; BWA only works with reference sequences shorter than 4GB (bwtindex.c:103)");
	/* the reference's own builder wraps above this: n_occ = (seq_len + 127)/128 + 1 in 32 bits (bwtmisc.c:131), so there are no
	 * reference files to be identical to (and its SA loader, bwtio.c:175, wraps above 0xffffffdf) */
	if (P.l_pac > 0xffffff80LL)
		return fail_msg(NABWA_EINVAL, "the reference is longer than 4 294 967 168 bases; BWA's Occ count wraps above that (bwtmisc.c:131)");
	pac_tail(P.pac, P.l_pac);
	return 0;
}

static int write_file(const std::string &fn, const void *data, size_t n)
{
	FILE *fp = fopen(fn.c_str(), "wb");
	if (!fp) return fail_msg(NABWA_EIO, "cannot write '" + fn + "'");
	const bool ok = fwrite(data, 1, n, fp) == n;
	if (fclose(fp) != 0 || !ok) return fail_msg(NABWA_EIO, "write to '" + fn + "' failed");
	return 0;
}

// bns_dump (bntseq.c:58-85)
static int dump_ann_amb(const Packed &P, const std::string &prefix)
{
	std::string ann, amb;
	char line[64];
	snprintf(line, sizeof line, "%lld %d %u\n", (long long)P.l_pac, (int)P.anns.size(), 11u); ann += line;
	for (size_t i = 0; i < P.anns.size(); ++i) {
		const nabwa_ann &a = P.anns[i];
		ann += "0 "; ann += a.name;
		if (!P.annos[i].empty()) { ann += ' '; ann += P.annos[i]; }
		ann += '\n';
		snprintf(line, sizeof line, "%lld %d %d\n", (long long)a.offset, a.len, a.n_ambs); ann += line;
	}
	snprintf(line, sizeof line, "%lld %d %u\n", (long long)P.l_pac, (int)P.anns.size(), (unsigned)P.holes.size()); amb += line;
	for (const nabwa_hole &h : P.holes) { snprintf(line, sizeof line, "%lld %d %c\n", (long long)h.offset, h.len, h.amb); amb += line; }
	int rc = write_file(prefix + ".ann", ann.data(), ann.size());
	if (!rc) rc = write_file(prefix + ".amb", amb.data(), amb.size());
	return rc;
}

static inline int base_at(const uint8_t *pac, int64_t i) { return pac[i >> 2] >> ((~i & 3) << 1) & 3; }

// bwa_pac_rev_core (bwtmisc.c:168-193): the text reversed (not complemented), same file convention
static std::vector<uint8_t> pac_reverse(const std::vector<uint8_t> &pac, int64_t l_pac)
{
	std::vector<uint8_t> r((size_t)(l_pac / 4 + 1), 0);
	for (int64_t j = 0; j < l_pac; ++j) r[j >> 2] |= (uint8_t)(base_at(pac.data(), l_pac - 1 - j) << ((~j & 3) << 1));
	r.push_back((uint8_t)(l_pac % 4));
	return r;
}

// bwa_pac2cspac_core (bwtmisc.c:210-229): colour i (i >= 1) encodes bases i-1 and i; the first "colour" is the first base
static std::vector<uint8_t> pac_to_colour(const std::vector<uint8_t> &pac, int64_t l_pac)
{
	static const int cs[16] = { 4, 0, 0, 1, 0, 2, 3, 4, 0, 3, 2, 4, 1, 4, 4, 4 };   // nst_color_space_table
	std::vector<uint8_t> out((size_t)(l_pac / 4 + 1), 0);
	int c1 = pac[0] >> 6;
	out[0] = (uint8_t)(c1 << 6);
	for (int64_t i = 1; i < l_pac; ++i) {
		const int c2 = base_at(pac.data(), i);
		out[i >> 2] |= (uint8_t)(cs[(1 << c1) | (1 << c2)] << ((~i & 3) * 2));
		c1 = c2;
	}
	out.push_back((uint8_t)(l_pac % 4));
	return out;
}

static int write_set(const Packed &P, const std::string &prefix, const std::vector<uint8_t> &pac, bool with_rpac)
{
	int rc = write_file(prefix + ".pac", pac.data(), pac.size());
	if (!rc) rc = dump_ann_amb(P, prefix);
	if (!rc && with_rpac) { const std::vector<uint8_t> r = pac_reverse(pac, P.l_pac); rc = write_file(prefix + ".rpac", r.data(), r.size()); }
	return rc;
}

}  // namespace

extern "C" int64_t nabwa_index_fa2pac(const char *fasta, const char *prefix)
{
	if (!fasta) return nabwa_fail(NABWA_EINVAL, "null argument");
	Packed P;
	const int rc = read_fasta(fasta, P);
	if (rc || !prefix) return rc ? rc : P.l_pac;      // no prefix: read and check only
	const int wc = write_set(P, prefix, P.pac, true);
	return wc ? wc : P.l_pac;
}

// `bwa index -c` up to the BWT (bwtindex.c:84-98): <prefix>.nt.pac/.ann/.amb of the bases, then the colour text as
// <prefix>.pac with the same .ann/.amb (bwa_pac2cspac re-dumps what bns_restore read back from the .nt files), and its
// reverse as <prefix>.rpac
extern "C" int64_t nabwa_index_fa2cspac(const char *fasta, const char *prefix)
{
	if (!fasta || !prefix) return nabwa_fail(NABWA_EINVAL, "null argument");
	Packed P;
	int rc = read_fasta(fasta, P);
	if (rc) return rc;
	const std::string pre(prefix);
	rc = write_set(P, pre + ".nt", P.pac, false);
	if (!rc) rc = write_set(P, pre, pac_to_colour(P.pac, P.l_pac), true);
	return rc ? rc : P.l_pac;
}
