// read_input.hpp -- the read side of bwa_read_seq / bwa_read_bam (bwaseqio.c:125-252), shared by nabwa_aln and
// nabwa_samse / nabwa_sampe: FASTA / FASTQ records as kseq delivers them, and BAM records as bamlite reads them.
// The including file defines TOOL (the tool name of its messages) before including this header; a damaged BGZF block ends the run
// through die(), a read the tools cannot take through fail(), both of tool_common.hpp.  Source is the one place where the records bwa_read_seq keeps are decided: the reads (and the
// .sai records) of nabwa_aln and of nabwa_samse / nabwa_sampe cannot drift apart.
#pragma once
#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>
#include "bgzf_in.hpp"
#include "bam_rec.hpp"

// ---------------------------------------------------------------------------------------------------------------------
// FASTA / FASTQ records the way kseq_read delivers them (kseq.h:155-193): a record starts at the next '>' or '@';
// the name ends at the first white space, the rest of the line is the comment; sequence characters are gathered
// up to the next '>', '+' or '@' WHEREVER it stands; after a '+' line, quality characters (33..127) are gathered
// until there are as many as bases, and one more character is consumed.
struct Fastx {
	gzFile fp = nullptr;
	std::vector<unsigned char> own;    /* gzip / stdin: the read buffer */
	const unsigned char *data = nullptr;   /* what the scans run over: `own`, or the whole file when it is plain and mapped */
	size_t have = 0, at = 0, file_size = 0;
	int pending = 0;
	bool eof = false, mapped = false, hit_limit = false;
	std::string name, comment, seq, qual;
	unsigned char cls[256];            /* sequence bytes: 0 = base character (isgraph), 1 = skipped, 2 = ends the sequence ('>' '+' '@') */

	void tables()
	{
		for (int c = 0; c < 256; ++c) cls[c] = isgraph(c) ? 0 : 1;
		cls['>'] = cls['+'] = cls['@'] = 2;
	}
	bool open(const char *fn)
	{
		tables();
		if (strcmp(fn, "-") != 0 && !getenv("NABWA_ALN_BUF")) {          /* a plain regular file is mapped: no copies, and its parse can be split */
			const int fd = ::open(fn, O_RDONLY);
			struct stat st;
			if (fd >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 2) {
				unsigned char magic[2] = { 0, 0 };
				if (pread(fd, magic, 2, 0) == 2 && !(magic[0] == 0x1f && magic[1] == 0x8b)) {
					void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
					if (m != MAP_FAILED) {
						(void)madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
						data = (const unsigned char*)m; have = file_size = (size_t)st.st_size; at = 0; eof = true; mapped = true;
						::close(fd);
						return true;
					}
				}
			}
			if (fd >= 0) ::close(fd);
		}
		fp = strcmp(fn, "-") == 0 ? gzdopen(fileno(stdin), "r") : gzopen(fn, "r");
		if (fp) gzbuffer(fp, 1 << 20);
		const char *bs = getenv("NABWA_ALN_BUF");             /* (tests: a few bytes, so that every scan meets the end of the buffer) */
		own.resize(bs && atoi(bs) > 0 ? (size_t)atoi(bs) : (size_t)4 << 20);
		data = own.data();
		return fp != nullptr;
	}
	/* a second reader on the same mapped file: bytes [from, limit) */
	void view(const Fastx &whole, size_t from, size_t limit)
	{
		tables();
		data = whole.data; file_size = whole.file_size; have = limit; at = from; eof = true; mapped = true; pending = 0; hit_limit = false;
	}
	void close() { if (fp) gzclose(fp); fp = nullptr; if (mapped && data && have == file_size && !own.size()) { /* the mapping lives until exit */ } }
	/* where the next record starts: the header character of a FASTA record may already have been taken */
	size_t logical_pos() const { return at - (pending ? 1 : 0); }
	/* true when data[at .. have) holds at least one byte */
	bool more()
	{
		if (at < have) return true;
		if (mapped) { if (have < file_size) hit_limit = true; return false; }
		if (eof) return false;
		const int got = gzread(fp, own.data(), (unsigned)own.size());
		at = 0; have = got > 0 ? (size_t)got : 0;
		if (got <= 0) { eof = true; return false; }
		return true;
	}
	/* length of the sequence, -1 at the end of the input, -2 for a truncated quality string.  The scans below run over
	 * what is in the buffer and append whole runs; they consume exactly the bytes the character-at-a-time description
	 * above consumes (tests/test_aln_parser.py holds that description as code). */
	int next()
	{
		int c = -1;
		if (!pending) {
			for (;;) {
				if (!more()) return -1;
				const unsigned char *p = data + at, *e = data + have;
				while (p < e && *p != '>' && *p != '@') ++p;
				at = (size_t)(p - data);
				if (p < e) { ++at; break; }
			}
		}
		pending = 0;
		name.clear(); comment.clear(); seq.clear(); qual.clear();
		for (c = -1;;) {                                     /* name: up to the first white space */
			if (!more()) break;
			const unsigned char *p = data + at, *e = data + have, *q = p;
			while (q < e && !isspace(*q)) ++q;
			name.append((const char*)p, (size_t)(q - p));
			at = (size_t)(q - data);
			if (q < e) { c = *q; ++at; break; }
		}
		if (c == -1 && name.empty()) return -1;
		if (c != '\n' && c != -1)                            /* comment: the rest of the line */
			for (;;) {
				if (!more()) break;
				const unsigned char *p = data + at, *e = data + have;
				const unsigned char *q = (const unsigned char*)memchr(p, '\n', (size_t)(e - p));
				comment.append((const char*)p, (size_t)((q ? q : e) - p));
				at = (size_t)((q ? q + 1 : e) - data);
				if (q) break;
			}
		for (c = -1;;) {                                     /* sequence: runs of base characters up to '>', '+' or '@' */
			if (!more()) break;
			const unsigned char *e = data + have, *q = data + at;
			while (q < e) {
				const unsigned char k = cls[*q];
				if (k == 0) { const unsigned char *r = q; do ++q; while (q < e && cls[*q] == 0); seq.append((const char*)r, (size_t)(q - r)); }
				else if (k == 1) ++q;
				else { c = *q; break; }
			}
			at = (size_t)(q - data);
			if (c != -1) { ++at; break; }
		}
		if (c == '>' || c == '@') pending = c;
		if (c != '+') return (int)seq.size();
		for (;;) {                                           /* the rest of the '+' line */
			if (!more()) return -2;
			const unsigned char *p = data + at, *e = data + have;
			const unsigned char *q = (const unsigned char*)memchr(p, '\n', (size_t)(e - p));
			at = (size_t)((q ? q + 1 : e) - data);
			if (q) break;
		}
		for (;;) {                                           /* quality: characters 33..127 until there is one per base */
			if (qual.size() >= seq.size()) { if (more()) ++at; break; }       /* ... and the character after them goes too */
			if (!more()) break;
			const unsigned char *e = data + have, *q = data + at;
			size_t need = seq.size() - qual.size();
			while (q < e && need) {
				const unsigned char *r = q;
				while (q < e && (size_t)(q - r) < need && *q >= 33 && *q <= 127) ++q;
				qual.append((const char*)r, (size_t)(q - r)); need -= (size_t)(q - r);
				if (need && q < e) ++q;                      /* a character that is not a quality (line break): skipped */
			}
			at = (size_t)(q - data);
		}
		if (qual.size() != seq.size()) return -2;
		return (int)seq.size();
	}
};

static uint8_t NT4[256];               /* nst_nt4_table (bntseq.c:39-56): 5 for '-', which the search and the alignments take as 4 (N) */
static void nt4_init()
{
	memset(NT4, 4, sizeof NT4);
	NT4['A'] = NT4['a'] = 0; NT4['C'] = NT4['c'] = 1; NT4['G'] = NT4['g'] = 2; NT4['T'] = NT4['t'] = 3;
	NT4['-'] = 5;
}

/* BAM records as bwa_read_bam takes them (bwaseqio.c:125-168 over bamlite.c:73-155): any gzip container (BGZF is a
 * series of gzip members; the reference opens BAM with gzopen as well, bamlite.h:7-11), header skipped, then per record the
 * flag, the 4-bit bases and the qualities.  `which`: 1 = first reads of pairs, 2 = second reads, 4 = unpaired (bwtaln.c:167-172). */

struct BamReader {
	FILE *file = nullptr;
	std::unique_ptr<BamIn> fp;              /* BGZF blocks inflated many at a time; any other gzip stream, or none, as gzread takes it */
	int which = 7;
	std::vector<unsigned char> rec;

	bool get(void *dst, size_t n) { return n == 0 || fp->read(dst, n); }
	bool skip(size_t n) { unsigned char tmp[4096]; while (n) { const size_t k = n < sizeof tmp ? n : sizeof tmp; if (!get(tmp, k)) return false; n -= k; } return true; }
	bool open(const char *fn)
	{
		file = strcmp(fn, "-") == 0 ? stdin : fopen(fn, "rb");
		if (!file) return false;
		fp.reset(new BamIn(file, fn));
		char magic[4]; int32_t l_text = 0, n_ref = 0;
		if (!get(magic, 4) || memcmp(magic, "BAM\1", 4) != 0) { fprintf(stderr, "[" TOOL "] invalid BAM binary header (this is not a BAM file).\n"); return false; }
		if (!get(&l_text, 4) || l_text < 0 || !skip((size_t)l_text) || !get(&n_ref, 4) || n_ref < 0) return false;
		for (int32_t i = 0; i < n_ref; ++i) { int32_t l_name = 0; if (!get(&l_name, 4) || l_name < 0 || !skip((size_t)l_name + 4)) return false; }
		return true;
	}
	void close() { fp.reset(); if (file && file != stdin) fclose(file); file = nullptr; }
	/* the next record that passes the selection: flag, number of bases, pointers to 4-bit bases and qualities; false at the end */
	bool next(unsigned *flag, int *l_seq, const unsigned char **bases, const unsigned char **qual)
	{
		for (;;) {
			int32_t block = 0; uint32_t x[8];
			if (!get(&block, 4) || block < 32 || !get(x, 32)) return false;
			rec.resize((size_t)block - 32 + 1);
			if (!get(rec.data(), (size_t)block - 32)) return false;
			const unsigned l_qname = x[2] & 0xffu, n_cigar = x[3] & 0xffffu; *flag = x[3] >> 16; *l_seq = (int)x[4];
			const size_t need = (size_t)l_qname + 4u * n_cigar + ((size_t)*l_seq + 1) / 2 + (size_t)*l_seq;
			if (*l_seq < 0 || need > (size_t)block - 32) return false;
			const bool paired = *flag & 1u;
			if (!(((which & 1) && paired && (*flag & 64u)) || ((which & 2) && paired && (*flag & 128u)) || ((which & 4) && !paired))) continue;
			*bases = rec.data() + l_qname + 4u * n_cigar; *qual = *bases + ((size_t)*l_seq + 1) / 2;
			return true;
		}
	}
};

#define READ_MODE_BAM   0x20                           /* BWA_MODE_* bits of gap_opt_t.mode, bwtaln.h:132-141 */
#define READ_MODE_CFY   0x08
#define READ_MODE_IL13  0x200
#define READ_MIN_RDLEN  35                             /* bwtaln.h:28 */
#define READ_BC_LOW_Q   13                             /* bwaseqio.c:170 */

/* what bwa_read_seq / bwa_read_bam keep of one record; the pointers are valid until the next call */
struct SeqRead {
	const uint8_t *code = nullptr;      /* full_len codes of the read as sequenced (nst_nt4_table: 0-3, 4, 5 for '-') */
	const char *qual = nullptr;         /* full_len quality characters after -I, or nullptr when the record has none */
	int full_len = 0, len = 0;          /* len: after -q (bwa_trim_read) */
	const char *name = nullptr;         /* the name as read; the /1 /2 strip of bwaseqio.c:239 is the caller's (BAM names keep it) */
	std::string bc;                     /* the barcode of -B (l_bc = mode >> 24), lower case below Q13 (bwaseqio.c:196-220) */
};

struct Source {                     /* bwa_read_seq (bwaseqio.c:172-252) and bwa_read_bam (:125-168) */
	Fastx fx;
	int mode = 0, trim_qual = 0;
	long n_trimmed = 0, n_tot = 0;
	BamReader *bam = nullptr;           /* BAM input: records come from here instead of fx */
	std::vector<uint8_t> code;
	std::string qa;

	/* bwa_open_reads (bwtaln.c:164-176): BAM (through b) with the read selection of -0 -1 -2 (none given: all), or FASTA / FASTQ */
	bool open(const char *fn, int mode_, int trim_qual_, BamReader &b)
	{
		mode = mode_; trim_qual = trim_qual_;
		if (!(mode & READ_MODE_BAM)) return fx.open(fn);
		const int which = ((mode & 0x40) ? 4 : 0) | ((mode & 0x80) ? 1 : 0) | ((mode & 0x100) ? 2 : 0);
		b.which = which ? which : 7;
		if (!b.open(fn)) return false;
		bam = &b;
		return true;
	}
	/* bwa_trim_read (bwaseqio.c:110-123) on phred+33 characters q[0..full): the length that is kept */
	static int trimmed_len(const char *q, int full, int trim_qual) { return bwa_trimmed_len(full, trim_qual, [q](int l) { return (int)(unsigned char)q[l] - 33; }); }
	/* the next record that survives the filters, into *r; r null: skip it (nothing decoded, nothing counted).  false at the end. */
	bool next(SeqRead *r)
	{
		if (bam) return next_bam(r);
		const int l_bc = (int)((unsigned)mode >> 24);
		for (;;) {
			if (fx.next() < 0) return false;
			if ((mode & READ_MODE_CFY) && !fx.comment.empty()) {        /* Casava's filter flag: "...:Y..." */
				const size_t p = fx.comment.find(':');
				if (p != std::string::npos && p + 1 < fx.comment.size() && fx.comment[p + 1] == 'Y') continue;
			}
			if ((int)fx.seq.size() <= l_bc) continue;                    /* nothing left after the barcode (also: empty reads) */
			break;
		}
		if (!r) return true;
		const bool hq = !fx.qual.empty();
		if ((mode & READ_MODE_IL13) && hq) for (char &c : fx.qual) c = (char)(c - 31);
		r->bc.clear();
		for (int i = 0; i < l_bc; ++i) {
			const unsigned char c = (unsigned char)fx.seq[i];
			r->bc.push_back((char)((hq && fx.qual[i] - 33 < READ_BC_LOW_Q) ? tolower(c) : toupper(c)));
		}
		const int full = (int)fx.seq.size() - l_bc;
		const char *q = hq ? fx.qual.data() + l_bc : nullptr;
		int len = full;
		if (hq && trim_qual >= 1) { len = trimmed_len(q, full, trim_qual); n_trimmed += full - len; }
		n_tot += full;
		if (len > 65535) fail("read '" + fx.name + "' is longer than 65535 bases");
		code.resize((size_t)full);
		const unsigned char *s = (const unsigned char*)fx.seq.data() + l_bc;
		for (int i = 0; i < full; ++i) code[i] = NT4[s[i]];
		r->code = code.data(); r->qual = q; r->full_len = full; r->len = len; r->name = fx.name.c_str();
		return true;
	}
	/* no barcode, no Casava filter, empty reads kept; qualities are always there (255 -> 126) */
	bool next_bam(SeqRead *r)
	{
		unsigned flag; int l; const unsigned char *s4, *q;
		if (!bam->next(&flag, &l, &s4, &q)) return false;
		if (!r) return true;
		if (l > 65535) fail("a read is longer than 65535 bases");
		code.resize((size_t)l); qa.assign((size_t)l, 0);
		for (int i = 0; i < l; ++i) {
			code[i] = nt16_nt4[s4[i >> 1] >> 4 * (1 - (i & 1)) & 0xf];
			qa[i] = (char)((int)q[i] + 33 < 126 ? q[i] + 33 : 126);
		}
		if (flag & 16u) {                                           /* stored reverse-complemented: back to the read as sequenced */
			std::reverse(code.begin(), code.end()); std::reverse(qa.begin(), qa.end());
			for (auto &c : code) if (c < 4) c = 3 - c;
		}
		int len = l;
		if (trim_qual >= 1) { len = trimmed_len(qa.data(), l, trim_qual); n_trimmed += l - len; }
		n_tot += l;
		r->bc.clear();
		r->code = code.data(); r->qual = qa.data(); r->full_len = l; r->len = len; r->name = (const char*)bam->rec.data();
		return true;
	}
};
