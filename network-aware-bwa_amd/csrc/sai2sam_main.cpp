// sai2sam_main.cpp -- `nabwa_samse` and `nabwa_sampe`: the reference's `bwa samse` (bwase.c:595-750) and `bwa sampe`
// (bwape.c:655-817) on top of libnabwa.so.  One source, two binaries (SAI2SAM_PE = 0 / 1).
//
//   nabwa_samse [-n max_occ] [-f out.sam] [-r RG_line] <prefix> <in.sai> <in.fq|in.bam>
//   nabwa_sampe [-a -o -s -P -n -N -c -f -A -r] <prefix> <in1.sai> <in2.sai> <in1.fq> <in2.fq>
//
// Every byte of the SAM text equals the reference's but the @PG line.  Reads are taken in chunks of 0x40000 (pairs for sampe), as
// the reference takes them: sampe's insert-size estimate is per chunk (bwape.c:340, with last_ii for a chunk without one), one
// drand48 stream seeded from the .ann seed runs across all chunks, and one position cache (g_hash) lives for the whole run.
//
// What runs where: hit choice, mapQ and pairing decisions on host threads in the library; every bwt_sa walk, gap refinement and mate
// rescue alignment on the GPU (nabwa_se_finish, nabwa_pe_posn, nabwa_pe_finish_sampe); parsing and SAM text (bwa_print_sam1,
// bwase.c:458-592) on host threads here.  Chunk k+1 is parsed and chunk k-1 formatted and written while the GPU works on chunk k;
// the output order is the input order.
//
// Colour space (a .sai whose option block lacks BWA_MODE_COMPREAD, from `nabwa_aln -c` on an index built with `nabwa_index -c`): the chains
// are nabwa_se_finish_cs / nabwa_pe_finish_sampe_cs, which also decode every mapped colour read into nucleotides on the GPU; SEQ / QUAL of
// a mapped record are the decoded read, those of an unmapped one the colour letters.  Refused with exit status 1, each because the
// reference crashes or reads outside its arrays there:
//   * nabwa_sampe without -s or -A: bwa_paired_sw hands bwa_paired_sw1 a null pac (bwape.c:651,692-701);
//   * reads without qualities (FASTA input): bwa_cs2nt_core reads p->qual[...] of a null pointer (cs2nt.c:129).
#include <future>

#ifndef SAI2SAM_PE
#define SAI2SAM_PE 0
#endif
#if SAI2SAM_PE
#define TOOL "nabwa_sampe"
#else
#define TOOL "nabwa_samse"
#endif

/* bad input: exit status 1 (thrown, so that the parser thread hands it to the main thread through its future) */
#define TOOL_FAIL_THROWS
#include "read_input.hpp"

#define MODE_BAM       0x20                            /* BWA_MODE_BAM*, bwtaln.h:137-140 */
#define MAX_BCLEN      63                              /* bwtaln.h:30 */
#define CHUNK          0x40000                         /* bwase.c:690, bwape.c:706 */
#define F_PD 1
#define F_PP 2
#define F_SU 4
#define F_MU 8
#define F_SR 16
#define F_MR 32
#define F_R1 64
#define F_R2 128

// ---------------------------------------------------------------------------------------------------------------------
// reads: what bwa_read_seq / bwa_read_bam put into a bwa_seq_t (bwaseqio.c:125-252)
struct Reads {
	std::vector<std::string> name, qual, bc;            /* qual: the whole string after -I, or empty when there is none */
	std::vector<uint8_t> has_qual;
	std::vector<int64_t> foff{0};                       /* fwd[foff[i] .. foff[i+1]): the read's codes as sequenced, full_len of them */
	std::vector<uint8_t> fwd;
	std::vector<int32_t> len, full_len;                 /* len after -q trimming */
	int n() const { return (int)name.size(); }
};

struct Input {                      /* the reader nabwa_aln uses (read_input.hpp), keeping what the SAM text needs of each read */
	Source src; BamReader bam;

	bool open(const char *fn, int mode, int trim_qual) { return src.open(fn, mode, trim_qual, bam); }
	/* the next read that passes the filters, appended to r; false at the end of the input */
	bool next(Reads &r)
	{
		SeqRead x;
		if (!src.next(&x)) return false;
		std::string nm = x.name;
		const size_t t = nm.size();                                      /* trim /[12]$ (FASTA / FASTQ only, bwaseqio.c:239) */
		if (!src.bam && t > 2 && nm[t - 2] == '/' && (nm[t - 1] == '1' || nm[t - 1] == '2')) nm.resize(t - 2);
		r.name.push_back(std::move(nm));
		r.qual.push_back(x.qual ? std::string(x.qual, (size_t)x.full_len) : std::string());
		r.has_qual.push_back(x.qual != nullptr);
		r.bc.push_back(x.bc);
		r.fwd.insert(r.fwd.end(), x.code, x.code + x.full_len);
		r.foff.push_back((int64_t)r.fwd.size());
		r.len.push_back(x.len); r.full_len.push_back(x.full_len);
		return true;
	}
	void close() { if (src.bam) bam.close(); else src.fx.close(); }
};

// ---------------------------------------------------------------------------------------------------------------------
// .sai files: gap_opt_t, then per read i32 n_aln and n_aln bwt_aln1_t (bwtaln.c:236-246)
struct Sai {
	FILE *f = nullptr; std::string fn;
	bool open(const char *path) { fn = path; f = fopen(path, "rb"); if (f) setvbuf(f, nullptr, _IOFBF, 4 << 20); return f != nullptr; }
	bool header(nabwa_gap_opt_t *o) { return fread(o, sizeof *o, 1, f) == 1; }
	void record(std::vector<int32_t> &n_aln, std::vector<nabwa_aln1_t> &rows)
	{
		int32_t n = 0;
		if (fread(&n, 4, 1, f) != 1) fail(fn + " ends before the reads do");
		if (n < 0) fail(fn + " holds a record with a negative number of hits");
		const size_t at = rows.size();
		rows.resize(at + (size_t)n);
		if (n && fread(rows.data() + at, sizeof(nabwa_aln1_t), (size_t)n, f) != (size_t)n) fail(fn + " ends inside a record");
		n_aln.push_back(n);
	}
};

// ---------------------------------------------------------------------------------------------------------------------
// one chunk through the pipeline
struct Chunk {
	int n = 0;                                          /* reads (samse) or pairs (sampe) */
	Reads r[2];
	std::vector<int32_t> n_aln;                         /* per read; sampe: interleaved 2 * pair + end */
	std::vector<nabwa_aln1_t> aln;
	std::vector<int64_t> off{0};
	std::vector<uint8_t> seq, rseq;
	std::vector<int32_t> full_len;
	std::vector<uint8_t> qual, nt_seq, nt_rseq, nt_qual; /* colour space: the qualities in, the decoded reads out (nabwa_se_finish_cs), all at off[] */
	std::vector<nabwa_se_t> se;
	std::vector<nabwa_pe_t> pe;
	std::string log;                                    /* stderr lines of the GPU step, printed in order */
	double t_read = 0, t_gpu = 0, t_fmt = 0, t_write = 0;
};

static void encode(Chunk &c, const Reads &r, int i, bool comp)          /* bwa_seq_t.seq (read reversed) and .rseq (its reverse complement), len bases */
{
	const int len = r.len[i];
	const uint8_t *f = r.fwd.data() + r.foff[i];
	const uint8_t flip = comp ? 3 : 0;
	for (int k = 0; k < len; ++k) { const uint8_t x = f[len - 1 - k]; c.seq.push_back(x < 4 ? x : 4); c.rseq.push_back(x < 4 ? x ^ flip : 4); }   /* '-' (5) as N, as nabwa_aln searched it */
	c.off.push_back((int64_t)c.seq.size());
	c.full_len.push_back(r.full_len[i]);
	if (!comp) {                                                         /* colour space: the qualities bwa_cs2nt_core reads (cs2nt.c:129) */
		if (!r.has_qual[i]) fail("colour-space read " + r.name[i] + " has no qualities: the conversion to nucleotides needs them (the reference reads a null pointer there, cs2nt.c:129)");
		c.qual.insert(c.qual.end(), r.qual[i].begin(), r.qual[i].begin() + len);
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// bwa_print_sam1 (bwase.c:458-592)
struct Printer {
	nabwa_index_t *ix;
	std::vector<std::string> names; std::vector<int64_t> offs; std::vector<int32_t> lens;
	int mode = 0, max_top2 = 0;
	std::string rg_id;
	bool colour() const { return !(mode & NABWA_MODE_COMPREAD); }

	int pac2real(int64_t pos, int len, int *seqid) const { return nabwa_index_pac2real(ix, pos, len, seqid); }
	static int64_t pos_end(const nabwa_se_t &p, int64_t pos)
	{
		if (p.n_cigar == 0) return pos + p.len;
		int64_t x = pos;
		for (int j = 0; j < p.n_cigar; ++j) { const int op = p.cigar[j] >> 14; if (op == 0 || op == 2) x += p.cigar[j] & 0x3fff; }
		return x;
	}
	static void cigar(std::string &o, const uint16_t *c, int n) { char b[16]; for (int j = 0; j < n; ++j) { snprintf(b, sizeof b, "%d%c", c[j] & 0x3fff, "MIDS"[c[j] >> 14]); o += b; } }
	static void put_qual(std::string &o, const Reads &rd, int i, int strand, int len)
	{
		if (!rd.has_qual[i]) { o += '*'; return; }
		const size_t at = o.size();
		o += rd.qual[i];
		if (strand) std::reverse(o.begin() + (long)at, o.begin() + (long)at + std::min<long>(len, (long)rd.qual[i].size()));   /* seq_reverse(p->len, p->qual, 0) */
	}
	/* p: the record; mapQ: its mapping quality; extra_flag: bwa_seq_t.extra_flag; mate: NULL for single-end; bc: the barcode printed */
	/* nt_seq / nt_qual (colour space): the decoded read of a mapped record -- reversed, as the chain leaves it -- and its qualities */
	void print1(std::string &o, const nabwa_se_t &p, int mapQ, int extra_flag, const nabwa_se_t *mate, const Reads &rd, int i, const std::string &bc,
				const uint8_t *nt_seq = nullptr, const uint8_t *nt_qual = nullptr) const
	{
		char b[256];
		const uint8_t *fwd = rd.fwd.data() + rd.foff[i];
		/* bwa_correct_trimmed (bwase.c:320-354) runs on every read, unmapped ones too, while their strand is still 0: a trimmed unmapped
		 * read gets len M + the clip as S, and len = full_len from there on */
		const bool trim0 = p.type == 0 && p.len < rd.full_len[i] && !colour();          /* (not applied in colour space, bwase.c:418-419) */
		const int tag_full = p.type != 0 && colour() ? p.full_len : rd.full_len[i];      /* bwa_seq_t.full_len: the decoded length once a colour read is decoded */
		const int plen = trim0 ? rd.full_len[i] : p.len;
		if (p.type != 0 || (mate && mate->type != 0)) {
			int seqid, m_seqid = -1, am = 0, flag = extra_flag, j;
			int64_t pos = p.pos; int strand = p.strand;
			if (p.type == 0) {                                           /* the mate's position and strand */
				pos = mate->pos; strand = mate->strand;
				flag |= F_SU; flag &= ~F_PP;
				j = 1;
			} else j = (int)(pos_end(p, pos) - pos);
			int nn = pac2real(pos, j, &seqid);
			if (p.type != 0 && pos + j - offs[seqid] > lens[seqid]) { flag |= F_SU; flag &= ~F_PP; mapQ = 0; }   /* bridges two contigs */
			if (strand) flag |= F_SR;
			if (mate) {
				if (mate->type != 0) {
					nn += pac2real(mate->pos, mate->len, &m_seqid);
					const int64_t m_j = pos_end(*mate, mate->pos) - mate->pos;
					if ((int64_t)mate->pos + m_j - offs[m_seqid] > lens[m_seqid]) { flag |= F_MU; flag &= ~F_PP; }
					if (mate->strand) flag |= F_MR;
				} else { flag |= F_MU; flag &= ~F_PP; }
			}
			o += rd.name[i];
			snprintf(b, sizeof b, "\t%d\t", flag); o += b;
			o += names[seqid];
			snprintf(b, sizeof b, "\t%d\t%d\t", (int)(pos - offs[seqid] + 1), mapQ); o += b;
			if (p.n_cigar) cigar(o, p.cigar, p.n_cigar);
			else if (trim0) { snprintf(b, sizeof b, "%dM%dS", p.len, rd.full_len[i] - p.len); o += b; }
			else if (p.type == 0) o += '*';
			else { snprintf(b, sizeof b, "%dM", p.len); o += b; }
			if (mate && mate->type != 0) {
				am = mate->seQ < p.seQ ? mate->seQ : p.seQ;
				o += '\t'; o += seqid == m_seqid ? std::string("=") : names[m_seqid]; o += '\t';
				long long isize = 0;
				if (seqid == m_seqid) {
					const int64_t m5 = mate->strand ? pos_end(*mate, mate->pos) : (int64_t)mate->pos;
					const int64_t p5 = p.type != 0 ? (strand ? pos_end(p, pos) : pos) : -1;
					isize = m5 - p5;
				}
				if (p.type == 0) isize = 0;
				snprintf(b, sizeof b, "%d\t%lld\t", (int)(mate->pos - offs[m_seqid] + 1), isize); o += b;
			} else if (mate) { snprintf(b, sizeof b, "\t=\t%d\t0\t", (int)(pos - offs[seqid] + 1)); o += b; }
			else o += "\t*\t0\t0\t";
			if (p.type != 0 && colour()) {                               /* the decoded read, in the alignment's orientation */
				const int fl = p.full_len;
				const size_t at = o.size();
				o.resize(at + 2 * (size_t)fl + 1);
				if (strand == 0) for (int k = 0; k < fl; ++k) { o[at + k] = "ACGT"[nt_seq[fl - 1 - k] & 3]; o[at + fl + 1 + k] = (char)nt_qual[k]; }
				else for (int k = 0; k < fl; ++k) { o[at + k] = "TGCA"[nt_seq[k] & 3]; o[at + fl + 1 + k] = (char)nt_qual[fl - 1 - k]; }
				o[at + fl] = '\t';
			} else {
				/* (an unmapped colour read beside its mapped mate: bwa_seq_t.full_len is still the untrimmed length; strand and pos are the mate's) */
				const int fl = rd.full_len[i];
				const size_t at = o.size();
				o.resize(at + (size_t)fl);
				/* codes 0-5: "ACGTN"[5] is the literal's terminating NUL, the byte the reference's putchar writes for a '-' */
				if (strand == 0) for (int k = 0; k < fl; ++k) o[at + k] = "ACGTN"[fwd[k]];
				else for (int k = 0; k < fl; ++k) o[at + k] = "TGCAN"[fwd[fl - 1 - k]];
				o += '\t';
				put_qual(o, rd, i, strand, plen);
			}
			tags_head(o, p, bc, tag_full);
			if (p.type != 0) {
				char XT = "NURM"[p.type];
				if (nn > 10) XT = 'N';
				snprintf(b, sizeof b, "\tXT:A:%c\t%s:i:%d", XT, (mode & NABWA_MODE_COMPREAD) ? "NM" : "CM", p.nm); o += b;
				if (nn) { snprintf(b, sizeof b, "\tXN:i:%d", nn); o += b; }
				if (mate) { snprintf(b, sizeof b, "\tSM:i:%d\tAM:i:%d", p.seQ, am); o += b; }
				if (p.type != 3) {
					snprintf(b, sizeof b, "\tX0:i:%d", (int)p.c1); o += b;
					if ((int)p.c1 <= max_top2) { snprintf(b, sizeof b, "\tX1:i:%d", (int)p.c2); o += b; }
				}
				snprintf(b, sizeof b, "\tXM:i:%d\tXO:i:%d\tXG:i:%d", p.n_mm, p.n_gapo, p.n_gapo + p.n_gape); o += b;
				o += "\tMD:Z:"; o += p.md;
				if (p.n_multi) {
					o += "\tXA:Z:";
					for (int k = 0; k < p.n_multi; ++k) {
						const nabwa_multi_t &q = p.multi[k];
						int64_t e = q.pos;
						if (q.n_cigar) { for (int z = 0; z < q.n_cigar; ++z) { const int op = q.cigar[z] >> 14; if (op == 0 || op == 2) e += q.cigar[z] & 0x3fff; } }
						else e += p.len;
						int sid;
						pac2real(q.pos, (int)(e - q.pos), &sid);
						o += names[sid];
						snprintf(b, sizeof b, ",%c%d,", q.strand ? '-' : '+', (int)((int64_t)q.pos - offs[sid] + 1)); o += b;
						if (q.n_cigar) cigar(o, q.cigar, q.n_cigar);
						else { snprintf(b, sizeof b, "%dM", p.len); o += b; }
						snprintf(b, sizeof b, ",%d;", q.gap + q.mm); o += b;
					}
				}
			}
			o += '\n';
		} else {                                                         /* no match, and no mapped mate */
			int flag = extra_flag | F_SU;
			if (mate && mate->type == 0) flag |= F_MU;
			o += rd.name[i];
			snprintf(b, sizeof b, "\t%d\t*\t0\t0\t*\t*\t0\t0\t", flag); o += b;
			const size_t at = o.size();
			o.resize(at + (size_t)plen);
			if (p.strand == 0) for (int k = 0; k < plen; ++k) o[at + k] = "ACGTN"[fwd[k]];
			else for (int k = 0; k < plen; ++k) { const uint8_t c = fwd[plen - 1 - k]; o[at + k] = "ACGTN"[c < 4 ? 3 - c : c]; }
			o += '\t';
			put_qual(o, rd, i, p.strand, plen);
			tags_head(o, p, bc, tag_full);
			if (mate && mate->type != 0) {                               /* the mate's XN (bwase.c:586-590) */
				int m_seqid;
				const int nn = pac2real(mate->pos, mate->len, &m_seqid);
				if (nn) { snprintf(b, sizeof b, "\tXN:i:%d", nn); o += b; }
			}
			o += '\n';
		}
	}
	void tags_head(std::string &o, const nabwa_se_t &p, const std::string &bc, int full_len) const
	{
		char b[64];
		if (!rg_id.empty()) { o += "\tRG:Z:"; o += rg_id; }
		if (!bc.empty()) { o += "\tBC:Z:"; o += bc; }
		if (p.clip_len < full_len) { snprintf(b, sizeof b, "\tXC:i:%d", p.clip_len); o += b; }
	}
};

/* bwa_escape + bwa_set_rg (bwase.c:619-656): -1 for a malformed line */
static int set_rg(const char *s, std::string &line, std::string &id)
{
	if (strstr(s, "@RG") != s) return -1;
	std::string t;
	for (const char *p = s; *p; ++p) {
		if (*p == '\\') {
			++p;
			if (*p == 't') t += '\t'; else if (*p == 'n') t += '\n'; else if (*p == 'r') t += '\r'; else if (*p == '\\') t += '\\';
			if (!*p) break;
		} else t += *p;
	}
	line = t;
	const size_t at = t.find("\tID:");
	if (at == std::string::npos) return -1;
	size_t e = at + 4;
	while (e < t.size() && t[e] != '\t' && t[e] != '\n') ++e;
	id = t.substr(at + 4, e - at - 4);
	return 0;
}

static int usage()
{
#if SAI2SAM_PE
	fprintf(stderr, "\nUsage:   " TOOL " [options] <prefix> <in1.sai> <in2.sai> <in1.fq> <in2.fq>\n\n"
			"Options: -a INT   maximum insert size [500]\n"
			"         -o INT   maximum occurrences for one end [100000]\n"
			"         -n INT   maximum hits to output for paired reads [3]\n"
			"         -N INT   maximum hits to output for discordant pairs [10]\n"
			"         -c FLOAT prior of chimeric rate (lower bound) [1.0e-05]\n"
			"         -f FILE  sam file to output results to [stdout]\n"
			"         -r STR   read group header line such as `@RG\\tID:foo\\tSM:bar' [null]\n"
			"         -P       accepted for compatibility; the index is always resident on the GPU\n"
			"         -s       disable Smith-Waterman for the unmapped mate\n"
			"         -A       disable insert size estimate (force -s)\n\n"
			"Colour space (.sai files from `nabwa_aln -c`): needs <prefix>.nt.ann, .nt.amb and .nt.pac, FASTQ reads (the conversion to\n"
			"nucleotides reads the qualities; the reference reads a null pointer without them, cs2nt.c:129), R3 reads first and -s or -A\n"
			"(the reference's mate rescue crashes in colour space, bwape.c:651).  Anything else is refused with exit status 1.\n\n"
			"Environment: NABWA_DEVICE picks the GPU [0].  Exit status 1: bad input, 2: no usable GPU.\n\n");
#else
	fprintf(stderr, "Usage: " TOOL " [-n max_occ] [-f out.sam] [-r RG_line] <prefix> <in.sai> <in.fq>\n"
			"Colour space (a .sai from `nabwa_aln -c`): needs <prefix>.nt.ann, .nt.amb and .nt.pac, and FASTQ reads (the conversion to\n"
			"nucleotides reads the qualities; the reference reads a null pointer without them, cs2nt.c:129); else exit status 1.\n"
			"Environment: NABWA_DEVICE picks the GPU [0].  Exit status 1: bad input, 2: no usable GPU.\n");
#endif
	return 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// one run: its inputs and options, and what lives across its chunks
static const int N_FILES = SAI2SAM_PE ? 2 : 1;
struct Run {
	const char *fn_rd[2] = { nullptr, nullptr };
	Sai sai[2]; nabwa_gap_opt_t gopt[2]; Input in[2];
	nabwa_pe_opt_t popt; int n_occ = 3;
	bool colour = false;                                /* bwase.c:680, bwape.c:690-692 */
	nabwa_index_t *ix = nullptr; int64_t seq_len = 0;
	Printer pr;
	uint64_t rng48 = 0;                                 /* srand48(bns->seed): one stream across all chunks */
	nabwa_poscache_t *cache = nullptr;
	nabwa_isize_t last_ii;                              /* sampe: the estimate of the last chunk that had one */
	bool inputs_done = false;
	double t_decode[2] = { 0, 0 };                      /* colour space: seconds of the decode stage, milliseconds of its kernels */
	/* sampe reads file 1 with the first .sai's mode and trimming, file 2 with the second's, and prints both with the second's option block (bwape.c:687-690) */
	const nabwa_gap_opt_t &opt() const { return gopt[N_FILES - 1]; }
};

/* ---- parse: one chunk of reads (pairs), their .sai records, the encoded reads; null at the end of the input */
static std::unique_ptr<Chunk> read_chunk(Run &R)
{
	if (R.inputs_done) return nullptr;
	const double ts = now_s();
	std::unique_ptr<Chunk> ch(new Chunk());
	Chunk &k = *ch;
	while (k.n < CHUNK) {
		if (!R.in[0].next(k.r[0])) break;
		if (SAI2SAM_PE && !R.in[1].next(k.r[1])) fail(std::string(R.fn_rd[1]) + " has fewer reads than " + R.fn_rd[0]);
		++k.n;
	}
	if (k.n < CHUNK) {
		R.inputs_done = true;
		if (SAI2SAM_PE && R.in[1].next(k.r[1])) fail(std::string(R.fn_rd[1]) + " has more reads than " + R.fn_rd[0]);
	}
	if (k.n == 0) return nullptr;
	const bool comp = R.opt().mode & NABWA_MODE_COMPREAD;
	for (int i = 0; i < k.n; ++i)
		for (int f = 0; f < N_FILES; ++f) { R.sai[f].record(k.n_aln, k.aln); encode(k, k.r[f], i, comp); }
	for (int f = 0; f < N_FILES; ++f)
		if (R.gopt[f].trim_qual >= 1) {
			char b[128]; snprintf(b, sizeof b, "[bwa_read_seq] %.1f%% bases are trimmed.\n", 100.0f * R.in[f].src.n_trimmed / R.in[f].src.n_tot);
			k.log += b; R.in[f].src.n_trimmed = R.in[f].src.n_tot = 0;
		}
	k.t_read = now_s() - ts;
	return ch;
}

/* a library call of the GPU chain failed: one line, exit status 2 without a usable GPU, else 1 (other threads are working: no exit handlers) */
[[noreturn]] static void gpu_failed(int r, bool say_caps)
{
	fprintf(stderr, "[" TOOL "] %s%s\n", nabwa_last_error(), say_caps && r == NABWA_ECAP ? " -- a record would exceed the library's caps; nothing wrong is written" : "");
	fflush(stderr); _exit(r == NABWA_ENODEV || r == NABWA_ENOMEM ? 2 : 1);
}

/* ---- GPU: the finishing chain of one chunk */
static void gpu_chunk(Run &R, Chunk &k)
{
	const double ts = now_s();
	const nabwa_gap_opt_t &opt = R.opt();
	fputs(k.log.c_str(), stderr);
	int r;
#if SAI2SAM_PE
	const int n = 2 * k.n;
	k.pe.resize((size_t)n);
	r = nabwa_pe_posn(R.ix, &opt, k.n, k.off.data(), k.full_len.data(), k.n_aln.data(), k.aln.data(), &R.rng48, k.pe.data());
	if (r != NABWA_OK) gpu_failed(r, false);
	std::vector<uint32_t> pos((size_t)n); std::vector<int32_t> len((size_t)n), mq((size_t)n);
	for (int i = 0; i < n; ++i) { const nabwa_se_t &s = k.pe[i].se; pos[i] = s.pos; len[i] = s.len; mq[i] = s.type ? s.mapQ : 0; }
	nabwa_isize_t ii; memset(&ii, 0, sizeof ii); char lg[2048];
	nabwa_isize_infer_pairs(k.n, pos.data(), len.data(), mq.data(), R.popt.ap_prior, R.seq_len, &ii, lg, sizeof lg);
	fputs(lg, stderr);
	if (ii.avg < 0.0 && R.last_ii.avg > 0.0) ii = R.last_ii;
	if (R.popt.force_isize) {
		fprintf(stderr, "[bwa_cal_pac_pos_pe] discard insert size estimate as user's request.\n");
		ii.low = ii.high = 0; ii.avg = ii.std = -1.0;
	}
	int cnt_chg = 0;
	if (R.colour) {
		k.nt_seq.assign(k.seq.size(), 0); k.nt_rseq.assign(k.seq.size(), 0); k.nt_qual.assign(k.seq.size(), 0);
		r = nabwa_pe_finish_sampe_cs(R.ix, &opt, &R.popt, &ii, k.n, k.off.data(), k.seq.data(), k.rseq.data(), k.qual.data(), k.n_aln.data(), k.aln.data(),
									 k.pe.data(), R.cache, &cnt_chg, k.nt_seq.data(), k.nt_rseq.data(), k.nt_qual.data(), R.t_decode);
	} else
		r = nabwa_pe_finish_sampe(R.ix, &opt, &R.popt, &ii, k.n, k.off.data(), k.seq.data(), k.rseq.data(), k.n_aln.data(), k.aln.data(), k.pe.data(),
								  R.cache, &cnt_chg, nullptr, nullptr);
	if (r != NABWA_OK) gpu_failed(r, true);
	fprintf(stderr, "[bwa_sai2sam_pe_core] changing coordinates of %d alignments.\n", cnt_chg);
	R.last_ii = ii;
#else
	k.se.resize((size_t)k.n);
	if (R.colour) {
		k.nt_seq.assign(k.seq.size(), 0); k.nt_rseq.assign(k.seq.size(), 0); k.nt_qual.assign(k.seq.size(), 0);
		r = nabwa_se_finish_cs(R.ix, &opt, k.n, k.off.data(), k.seq.data(), k.rseq.data(), k.qual.data(), k.full_len.data(), k.n_aln.data(), k.aln.data(),
							   R.n_occ, &R.rng48, k.se.data(), k.nt_seq.data(), k.nt_rseq.data(), k.nt_qual.data(), R.t_decode);
	} else
		r = nabwa_se_finish(R.ix, &opt, k.n, k.off.data(), k.seq.data(), k.rseq.data(), k.full_len.data(), k.n_aln.data(), k.aln.data(),
							R.n_occ, &R.rng48, k.se.data());
	if (r != NABWA_OK) gpu_failed(r, true);
#endif
	k.t_gpu = now_s() - ts;
}

/* ---- SAM text on host threads, in slices; written in order */
static std::vector<std::string> format_chunk(const Run &R, Chunk &k)
{
	const double ts = now_s();
	const int nt = host_threads((size_t)k.n, 4096);
	const bool colour = R.colour;
	std::vector<std::string> parts((size_t)nt);
	host_parallel(nt, (size_t)k.n, [&](int t, size_t lo, size_t hi) {
		std::string &o = parts[(size_t)t];
		o.reserve((hi - lo) * (SAI2SAM_PE ? 700 : 350));
		for (size_t i = lo; i < hi; ++i) {
#if SAI2SAM_PE
			const nabwa_pe_t &a = k.pe[2 * i], &b = k.pe[2 * i + 1];
			const std::string bc = (k.r[0].bc[i].empty() && k.r[1].bc[i].empty()) ? std::string() : k.r[0].bc[i] + k.r[1].bc[i];   /* bwape.c:734-737 */
			const uint8_t *ns = colour ? k.nt_seq.data() : nullptr, *nq = colour ? k.nt_qual.data() : nullptr;
			const int64_t oa = k.off[2 * i], ob = k.off[2 * i + 1];
			R.pr.print1(o, a.se, a.mapQ_paired, a.extra_flag & (F_PD | F_PP | F_R1 | F_R2), &b.se, k.r[0], (int)i, bc, ns ? ns + oa : ns, nq ? nq + oa : nq);
			R.pr.print1(o, b.se, b.mapQ_paired, b.extra_flag & (F_PD | F_PP | F_R1 | F_R2), &a.se, k.r[1], (int)i, bc, ns ? ns + ob : ns, nq ? nq + ob : nq);
#else
			const nabwa_se_t &s = k.se[i];
			R.pr.print1(o, s, s.mapQ, 0, nullptr, k.r[0], (int)i, k.r[0].bc[i], colour ? k.nt_seq.data() + k.off[i] : nullptr,
						colour ? k.nt_qual.data() + k.off[i] : nullptr);
#endif
		}
	});
	k.t_fmt = now_s() - ts;
	return parts;
}

static int run(int argc, char *argv[]);
int main(int argc, char *argv[])
{
	try { return run(argc, argv); }
	catch (const BadInput &e) { fprintf(stderr, "[" TOOL "] %s\n", e.msg.c_str()); fflush(stderr); return 1; }
}

static int run(int argc, char *argv[])
{
	nt4_init();
	Run R;
	std::string rg_line, rg_id;
	const char *ofile = nullptr;
	int c;
	nabwa_pe_opt_t &popt = R.popt;
	nabwa_pe_opt_default(&popt);
#if SAI2SAM_PE
	const char *optstr = "a:o:sPn:N:c:f:Ar:";
#else
	const char *optstr = "hn:f:r:";
#endif
	while ((c = getopt(argc, argv, optstr)) >= 0) {
		switch (c) {
		case 'h': break;
		case 'r':
			if (set_rg(optarg, rg_line, rg_id) < 0) { fprintf(stderr, "[" TOOL "] malformated @RG line\n"); return 1; }
			break;
		case 'f': ofile = optarg; break;
#if SAI2SAM_PE
		case 'a': popt.max_isize = atoi(optarg); break;
		case 'o': popt.max_occ = atoi(optarg); break;
		case 's': popt.is_sw = 0; break;
		case 'P': popt.is_preload = 1; break;
		case 'n': popt.n_multi = atoi(optarg); break;
		case 'N': popt.N_multi = atoi(optarg); break;
		case 'c': popt.ap_prior = atof(optarg); break;
		case 'A': popt.force_isize = 1; break;
#else
		case 'n': R.n_occ = atoi(optarg); break;
#endif
		default: return 1;
		}
	}
	if (optind + 1 + 2 * N_FILES > argc) return usage();
	/* NABWA_FINISH: where the finishing chains cut reference windows, apply the CIGAR end rules and write MD / NM (the library reads it at
	 * every call); a value it would refuse is refused here, before any file is opened */
	if (const char *e = getenv("NABWA_FINISH")) if (strcmp(e, "gpu") && strcmp(e, "host")) fail(std::string("NABWA_FINISH=") + e + ": host or gpu");
	const char *prefix = argv[optind];
	const char *fn_sai[2] = { argv[optind + 1], SAI2SAM_PE ? argv[optind + 2] : nullptr };
	R.fn_rd[0] = argv[optind + 1 + N_FILES]; R.fn_rd[1] = SAI2SAM_PE ? argv[optind + 2 + N_FILES] : nullptr;
#if SAI2SAM_PE
	if (popt.n_multi < 0 || popt.N_multi < 0 || popt.n_multi > NABWA_MAX_MULTI || popt.N_multi > NABWA_MAX_MULTI)
		fail("-n / -N must be within 0.." + std::to_string(NABWA_MAX_MULTI) + " (the library's multi-hit cap)");
#else
	if (R.n_occ < 0 || R.n_occ > NABWA_MAX_MULTI - 1) fail("-n must be within 0.." + std::to_string(NABWA_MAX_MULTI - 1) + " (the library's multi-hit cap)");
#endif

	// inputs first: a bad one is reported without a GPU, and before anything is written
	for (int f = 0; f < N_FILES; ++f) {
		if (!R.sai[f].open(fn_sai[f])) fail(std::string("cannot open ") + fn_sai[f]);
		if (!R.sai[f].header(&R.gopt[f])) fail(std::string(fn_sai[f]) + " is too short for a .sai header");
	}
	const nabwa_gap_opt_t &opt = R.opt();
	const bool colour = R.colour = !(opt.mode & NABWA_MODE_COMPREAD);
	if (colour) {
		for (const char *ext : { ".nt.ann", ".nt.amb", ".nt.pac" }) {
			const std::string p = std::string(prefix) + ext;
			if (access(p.c_str(), R_OK) != 0) fail(std::string(fn_sai[N_FILES - 1]) + " is a colour-space .sai and " + p + " cannot be read (an index built with `nabwa_index -c` has it)");
		}
#if SAI2SAM_PE
		if (popt.is_sw && !popt.force_isize)
			fail(std::string(fn_sai[1]) + " is a colour-space .sai: give -s or -A (there is no mate rescue in colour space; the reference's crashes there, bwape.c:651)");
		popt.type = 2;                                                   /* BWA_PET_SOLID */
		popt.is_sw = 0;
#endif
	}
	for (int f = 0; f < N_FILES; ++f) {
		if ((unsigned)R.gopt[f].mode >> 24 > MAX_BCLEN) fail("the maximum barcode length is 63");
		if (!R.in[f].open(R.fn_rd[f], R.gopt[f].mode, R.gopt[f].trim_qual)) fail(std::string("cannot open ") + R.fn_rd[f]);
	}
	for (const char *ext : { ".ann", ".amb", ".pac", ".bwt", ".rbwt", ".sa", ".rsa" }) {
		const std::string p = std::string(prefix) + ext;
		if (access(p.c_str(), R_OK) != 0) fail("cannot read " + p);
	}
	int device;
	if (!tool_device(&device, "; nothing was written")) return 2;
	double t0 = now_s();
	nabwa_index_t *&ix = R.ix;
	int rc = nabwa_index_load(prefix, device, 1, 0, &ix);
	if (rc == NABWA_OK) rc = nabwa_index_attach_reference(ix, prefix);
	if (rc == NABWA_OK && colour) rc = nabwa_index_attach_nt_reference(ix, prefix);
	if (rc != NABWA_OK) {
		fprintf(stderr, "[" TOOL "] loading the index failed: %s\n", nabwa_last_error());
		return rc == NABWA_ENODEV || rc == NABWA_ENOMEM ? 2 : 1;
	}
	const double t_load = now_s() - t0;
	Printer &pr = R.pr; pr.ix = ix; pr.mode = opt.mode; pr.max_top2 = opt.max_top2; pr.rg_id = rg_id;
	int64_t l_pac = 0; uint32_t seed = 0;
	nabwa_index_reference_info(ix, &l_pac, &seed);
	for (int i = 0, n = nabwa_index_n_contigs(ix); i < n; ++i) {
		char nm[4096]; int64_t o; int32_t l;
		nabwa_index_contig(ix, i, nm, sizeof nm, &o, &l);
		pr.names.push_back(nm); pr.offs.push_back(o); pr.lens.push_back(l);
	}
	R.seq_len = (int64_t)nabwa_index_seq_len(ix, 0);

	FILE *out = stdout;
	if (ofile && !(out = fopen(ofile, "w"))) fail(std::string("cannot write ") + ofile);
	setvbuf(out, nullptr, _IOFBF, 8 << 20);
	{
		std::string h;
		for (size_t i = 0; i < pr.names.size(); ++i) h += "@SQ\tSN:" + pr.names[i] + "\tLN:" + std::to_string(pr.lens[i]) + "\n";
		if (!rg_line.empty()) h += rg_line + "\n";
		h += std::string("@PG\tID:bwa\tPN:bwa\tVN:") + VERSION + "\n";
		fwrite(h.data(), 1, h.size(), out);
	}

	R.rng48 = (uint64_t)seed << 16 | 0x330E;
	R.cache = SAI2SAM_PE ? nabwa_poscache_create() : nullptr;
	memset(&R.last_ii, 0, sizeof R.last_ii); R.last_ii.avg = -1.0;

	long long tot = 0;
	double t_read = 0, t_gpu = 0, t_fmt = 0, t_write = 0;
	double t_wait_parse = 0, t_wait_write = 0, t_first_parse = 0;    /* the main thread's time is GPU chain + these waits */
	const double t_run0 = now_s();
	std::future<std::unique_ptr<Chunk>> next = std::async(std::launch::async, read_chunk, std::ref(R));
	std::future<void> writing;
	for (;;) {
		std::unique_ptr<Chunk> k;
		const double tw0 = now_s();
		try { k = next.get(); }
		catch (...) { if (writing.valid()) writing.wait(); throw; }      /* bad input in the next chunk: the chunk being written stays alive until then */
		if (tot == 0) t_first_parse = now_s() - tw0; else t_wait_parse += now_s() - tw0;
		if (!k) break;
		t_read += k->t_read;
		next = std::async(std::launch::async, read_chunk, std::ref(R));  /* chunk k+1 is parsed ... */
		gpu_chunk(R, *k);                                                /* ... while chunk k is on the GPU and chunk k-1 is written */
		t_gpu += k->t_gpu;
		const double tw1 = now_s();
		if (writing.valid()) writing.get();
		t_wait_write += now_s() - tw1;
		tot += k->n;
		fprintf(stderr, "[" TOOL "] %lld %s have been processed (GPU chain of the last chunk %.2f sec).\n", tot, SAI2SAM_PE ? "pairs" : "reads", k->t_gpu);
		/* the writer owns the chunk from here and frees it (hundreds of MB of records) off the main thread */
		std::shared_ptr<Chunk> kp(std::move(k));
		writing = std::async(std::launch::async, [&, kp]() mutable {
			std::vector<std::string> parts = format_chunk(R, *kp);
			const double tw = now_s();
			for (const std::string &p : parts) fwrite(p.data(), 1, p.size(), out);
			kp->t_write = now_s() - tw;
			t_fmt += kp->t_fmt; t_write += kp->t_write;
			parts.clear(); kp.reset();
		});
	}
	const double tw2 = now_s();
	if (writing.valid()) writing.get();
	if (fflush(out) != 0 || (out != stdout && fclose(out) != 0)) fail("writing the output failed");
	const double t_drain = now_s() - tw2;
	const double t_run = now_s() - t_run0;
	for (int f = 0; f < N_FILES; ++f) R.in[f].close();
	if (R.cache) nabwa_poscache_destroy(R.cache);
	nabwa_index_destroy(ix);
	final_rename(ofile, false);
	fprintf(stderr, "[" TOOL "] %lld %s in %.2f sec (%.0f %s/s); index load %.2f sec; stage totals: parse %.2f sec, GPU chain %.2f sec, "
			"SAM text %.2f sec, write %.2f sec (parse and text overlap the GPU chain)\n", tot, SAI2SAM_PE ? "pairs" : "reads", t_run,
			t_run > 0 ? tot / t_run : 0.0, SAI2SAM_PE ? "pairs" : "reads", t_load, t_read, t_gpu, t_fmt, t_write);
	fprintf(stderr, "[" TOOL "] main thread: first chunk parsed %.2f sec (fill), GPU chain %.2f sec, waited for the parser %.2f sec and for "
			"the writer %.2f sec, last chunk's text and write %.2f sec (drain), other %.2f sec\n", t_first_parse, t_gpu, t_wait_parse, t_wait_write, t_drain,
			t_run - (t_first_parse + t_gpu + t_wait_parse + t_wait_write + t_drain));
	if (colour)
		fprintf(stderr, "[" TOOL "] colour space: decoding the mapped reads took %.3f sec of the GPU chain (records, copies and kernels; the kernels alone %.2f ms)\n", R.t_decode[0], R.t_decode[1]);
	return 0;
}
