// bam2bam_main.cpp -- `nabwa_bam2bam`: the command line of `bwa bam2bam -t 1` (bam2bam.c:1942-2098) on top of libnabwa.so.
//
//     nabwa_bam2bam -g PREFIX [alignment options of bwa bam2bam] [-f out.bam] in.bam
//
// BAM in (BGZF, any other gzip stream or none, as the reference's bamlite reads it; bgzf_in.hpp) -> both passes of the reference's sequential loop
// (bam2bam.c:1143-1216) through the batch front-end of the library (nabwa_bam_batch_*, bam_batch.hip) -> BGZF BAM out with
// the header bwa_print_bam_header writes (@HD VN:1.4, a new @PG chained to the old one, @SQ from the .ann file, the other old
// lines kept; bam2bam.c:164-301).  Host code only; the GPU work is the library's.  Not provided: the 0MQ master mode
// (-p; the worker side is nabwa_worker, worker_main.cpp) and resuming from .sai files (-0 -1 -2) -- each is refused, none is
// silently ignored.  --only-aligned, --drop-aligned, --skip-duplicates, --broken-input and --debug-bam are the library's NABWA_BAM_* flags.
// --sort (not the reference's): the records leave sorted by coordinate, runs sorted on the GPU or, NABWA_SORT=host, on host threads.
// --damage FILE (not the reference's): the damage profile of the records as they leave, counted on the first GPU.
// --mark-duplicates, --remove-duplicates (not the reference's; with --sort): duplicates found on the first GPU, flagged 0x400 or dropped.
// --index (not the reference's; with --sort and -f): out.bam.bai beside the output, built on the first GPU from the records as they are written.
// -t is accepted and ignored (NABWA_DEVICES=0,1,... names the GPUs: an index replica on each, batches dealt to them in turn, searched as
// they come and passed in input order; default one GPU, NABWA_DEVICE or 0), --temp-dir likewise (the records wait in memory between the passes).
#include <getopt.h>
#include <zlib.h>
#include <memory>
#include <set>
#include <string>
#include <thread>
#include <vector>
#define TOOL "nabwa_bam2bam"
#include "bgzf_in.hpp"
#include "bam_header.hpp"
#include "bam_sort_host.hpp"

/* ---------------------------------------------------------------- BGZF out (bgzf.c: blocks of <= 0xff00 input bytes, level 2) */
static void bgzf_block(const uint8_t *in, size_t n, int level, std::vector<uint8_t> &out)
{
	uint8_t buf[0x10000 + 64];
	z_stream zs; memset(&zs, 0, sizeof(zs));
	zs.next_in = (Bytef*)in; zs.avail_in = (uInt)n; zs.next_out = buf + 18; zs.avail_out = sizeof(buf) - 18 - 8;
	if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK || deflate(&zs, Z_FINISH) != Z_STREAM_END) die("BGZF", "deflate failed");
	const size_t clen = zs.total_out; deflateEnd(&zs);
	static const uint8_t hdr[16] = { 31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0 };
	memcpy(buf, hdr, 16);
	const uint16_t bsize = (uint16_t)(clen + 25);
	buf[16] = (uint8_t)bsize; buf[17] = (uint8_t)(bsize >> 8);
	const uint32_t crc = (uint32_t)crc32(crc32(0, 0, 0), in, (uInt)n), isz = (uint32_t)n;
	uint8_t *t = buf + 18 + clen;
	memcpy(t, &crc, 4); memcpy(t + 4, &isz, 4);
	out.insert(out.end(), buf, buf + 18 + clen + 8);
}

struct BgzfOut {
	FILE *f; std::vector<uint8_t> pend; int level;
	nabwa_bgzf_t *gpu;                                 /* NABWA_BGZF=gpu, gpu-dynamic: the blocks are made by the library's compressor; null: zlib on host threads */
	std::vector<uint8_t> packed;
	int codes = NABWA_BGZF_CODES_FIXED;                /* gpu-dynamic: NABWA_BGZF_CODES_DYNAMIC */
	uint64_t n_taken = 0;                              /* the uncompressed bytes taken so far, the header's first */
	bool track = false;                                /* --index: where every block written starts, uncompressed and in the file */
	std::vector<int64_t> blk_u, blk_c;
	int64_t u_at = 0, c_at = 0;
	void write(const void *p, size_t n) { const uint8_t *b = (const uint8_t*)p; pend.insert(pend.end(), b, b + n); n_taken += n; if (pend.size() >= (64u << 20)) flush(false); }
	/* the members just written, whoever made them: BSIZE at +16, ISIZE in the trailer */
	void note(const uint8_t *p, size_t n)
	{
		if (!track) return;
		for (size_t q = 0; q < n; ) {
			if (n - q < 26) die("output", "a BGZF block cut short");
			const size_t bsize = (size_t)(p[q + 16] | p[q + 17] << 8) + 1;
			if (bsize < 26 || bsize > n - q) die("output", "a BGZF block cut short");
			uint32_t isize; memcpy(&isize, p + q + bsize - 4, 4);
			blk_u.push_back(u_at); blk_c.push_back(c_at);
			u_at += isize; c_at += (int64_t)bsize; q += bsize;
		}
	}
	void flush(bool all)
	{
		const size_t BS = 0xff00;
		const size_t n_full = pend.size() / BS, n_blocks = all ? (pend.size() + BS - 1) / BS : n_full;
		if (!n_blocks) return;
		const size_t take = n_blocks * BS < pend.size() ? n_blocks * BS : pend.size();
		if (gpu) {
			const size_t bound = (size_t)nabwa_bgzf_bound((int64_t)take);
			if (packed.size() < bound) packed.resize(bound);
			int64_t n_out = 0, nb = 0;
			if (nabwa_bgzf_handle_compress_ex(gpu, codes, pend.data(), (int64_t)take, packed.data(), (int64_t)packed.size(), &n_out, &nb) != NABWA_OK) { fprintf(stderr, "[nabwa_bam2bam] BGZF on the GPU: %s\n", nabwa_last_error()); fflush(stderr); _exit(2); }
			if (fwrite(packed.data(), 1, (size_t)n_out, f) != (size_t)n_out) die("output", "write failed");
			note(packed.data(), (size_t)n_out);
			pend.erase(pend.begin(), pend.begin() + take);
			return;
		}
		int nt = io_threads(); if ((size_t)nt > n_blocks) nt = (int)n_blocks;
		std::vector<std::vector<uint8_t>> parts(nt);
		std::vector<std::thread> th;
		for (int t = 0; t < nt; ++t) th.emplace_back([&, t]() {
			for (size_t k = n_blocks * t / nt; k < n_blocks * (t + 1) / nt; ++k) {
				const size_t o = k * BS, m = pend.size() - o < BS ? pend.size() - o : BS;
				bgzf_block(pend.data() + o, m, level, parts[t]);
			}
		});
		for (auto &x : th) x.join();
		for (auto &p : parts) if (!p.empty() && fwrite(p.data(), 1, p.size(), f) != p.size()) die("output", "write failed");
		for (auto &p : parts) note(p.data(), p.size());
		pend.erase(pend.begin(), pend.begin() + take);
	}
	void close()
	{
		flush(true);
		static const uint8_t eof[28] = { 31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
		if (fwrite(eof, 1, 28, f) != 28 || fflush(f) != 0) die("output", "write failed");
		note(eof, 28);
		if (f != stdout) fclose(f);
	}
};

/* ---------------------------------------------------------------- the header (bam2bam.c:164-301); find_pp_tag: bam_header.hpp */
/* f(name, length) for the contigs of the index, in order */
template <class F> static void each_contig(nabwa_index_t *ix, F f)
{
	const int ns = nabwa_index_n_contigs(ix);
	for (int i = 0; i < ns; ++i) { char name[1024]; int64_t off; int32_t len; nabwa_index_contig(ix, i, name, sizeof name, &off, &len); f(name, len); }
}
/* ---------------------------------------------------------------- the temporary file between the passes (bam2bam.c:1099-1135, 1733-1758)
 * With --temp-dir a batch that has to wait for the insert-size estimates does not wait in memory: its records leave as the reference's
 * temporary file holds them -- u32 length + the message of msg_init_from_pair, positioned (or finished, for a batch of single reads
 * that only waits for its turn) -- and come back batch by batch for pass 2.  (Plain, not gzip: one core of deflate would pace the file.) */
struct Spilled { long at; int n_logical, n_records; bool finished; size_t dev; };
/* (Known and left as it is here: with --only-aligned a finished batch's nabwa_bam_batch_output has dropped the unmapped records already,
 * while the loop below still sizes one record per logical read from it -- the run then ends with "temporary file: cannot write".  Its fix
 * comes with its own test.) */
static void spill_batch(FILE *f, nabwa_bam_batch_t *b, bool finished, Spilled &S)
{
	int nr = 0, nl = 0; nabwa_bam_batch_counts(b, &nr, &nl);
	std::vector<uint8_t> kinds((size_t)(nl ? nl : 1));
	nabwa_bam_batch_kinds(b, kinds.data());
	int64_t nb = 0; std::vector<int64_t> oo((size_t)nr + 1, 0);
	nabwa_bam_batch_output(b, 0, 0, oo.data(), &nb);
	std::vector<uint8_t> ob((size_t)(nb ? nb : 1));
	if (nabwa_bam_batch_output(b, ob.data(), nb, oo.data(), &nb) != NABWA_OK) die("temporary file", nabwa_last_error());
	std::vector<nabwa_wire_read_t> st((size_t)(nr ? nr : 1));
	memset(st.data(), 0, sizeof(nabwa_wire_read_t) * st.size());
	if (!finished && nabwa_bam_batch_positioned(b, st.data()) != NABWA_OK) die("temporary file", nabwa_last_error());
	S.at = ftell(f); S.n_logical = nl; S.n_records = nr; S.finished = finished;
	std::vector<uint8_t> msg;
	int at = 0;
	for (int k = 0; k < nl; ++k) {
		nabwa_wire_rec_t r; memset(&r, 0, sizeof r);
		r.recno = (uint64_t)k; r.kind = kinds[(size_t)k]; r.phase = finished ? NABWA_PHASE_FINISHED : NABWA_PHASE_POSITIONED;
		for (int e = 0; e < r.kind; ++e, ++at) {
			r.read[e] = st[(size_t)at];
			const uint8_t *rec = ob.data() + oo[(size_t)at];
			nabwa_wire_core_from_bam(rec + 4, r.read[e].core);
			r.read[e].data = rec + 36; r.read[e].data_len = (int32_t)(oo[(size_t)at + 1] - oo[(size_t)at] - 36);
		}
		const int64_t need = nabwa_wire_size(&r);
		msg.resize((size_t)need + 4);
		const uint32_t len = (uint32_t)need;
		memcpy(msg.data(), &len, 4);
		if (nabwa_wire_encode(&r, msg.data() + 4, need) != need || fwrite(msg.data(), 1, msg.size(), f) != msg.size()) die("temporary file", "cannot write");
	}
}
/* one batch back: its records as a BAM stream and, unless it was finished, the state pass 1 left */
static void unspill_batch(FILE *f, const Spilled &S, std::vector<uint8_t> &stream, std::vector<int64_t> &off, std::vector<nabwa_wire_read_t> &st, std::vector<std::vector<uint8_t>> &keep)
{
	if (fseek(f, S.at, SEEK_SET) != 0) die("temporary file", "cannot seek");
	stream.clear(); off.assign(1, 0); st.clear(); keep.clear();
	for (int k = 0; k < S.n_logical; ++k) {
		uint32_t len = 0;
		if (fread(&len, 4, 1, f) != 1) die("temporary file", "truncated");
		keep.emplace_back((size_t)len);
		if (len && fread(keep.back().data(), 1, len, f) != len) die("temporary file", "truncated");
		nabwa_wire_rec_t r;
		if (nabwa_wire_decode(keep.back().data(), (int64_t)len, &r) != NABWA_OK) die("temporary file", nabwa_last_error());
		for (int e = 0; e < r.kind; ++e) {
			const nabwa_wire_read_t &x = r.read[e];
			const uint32_t bs = 32u + (uint32_t)x.data_len;
			const size_t at = stream.size();
			stream.resize(at + 4 + bs);
			memcpy(&stream[at], &bs, 4);
			nabwa_wire_core_to_bam(x.core, &stream[at + 4]);
			if (x.data_len) memcpy(&stream[at + 36], x.data, (size_t)x.data_len);
			off.push_back((int64_t)stream.size());
			st.push_back(x);
		}
	}
	if ((int)st.size() != S.n_records) die("temporary file", "a batch came back with another number of records");
}

/* ---------------------------------------------------------------- the command line (bam2bam.c:40-75, 1942-2098) */
struct Options {
	nabwa_gap_opt_t go; nabwa_pe_opt_t po;
	uint32_t rec_flags = 0;                                    /* NABWA_BAM_*: --only-aligned, --drop-aligned, --debug-bam, --broken-input, --skip-duplicates */
	const char *prefix = 0, *ofile = 0, *temp_dir = 0, *input = 0;
	bool bgzf_gpu = false;                                     /* NABWA_BGZF=gpu or gpu-dynamic */
	bool bgzf_dynamic = false;                                 /* NABWA_BGZF=gpu-dynamic */
	bool bgzf_in_gpu = false;                                  /* NABWA_BGZF_IN=gpu */
	bool sort = false;                                         /* --sort: coordinate order */
	bool sort_host = false;                                    /* NABWA_SORT=host: the runs are sorted on host threads, not on the GPU */
	long sort_run_mib = 1024;                                  /* NABWA_SORT_RUN_MIB: record bytes of a run */
	const char *damage_file = 0;                               /* --damage FILE: the damage profile of the records goes there */
	nabwa_damage_opt_t damage;                                 /* NABWA_DAMAGE_POS, NABWA_DAMAGE_MAPQ */
	bool mark_dups = false, remove_dups = false;               /* --mark-duplicates, --remove-duplicates */
	nabwa_markdup_opt_t markdup;                               /* NABWA_MARKDUP_ENDS, NABWA_MARKDUP_QUAL */
	bool dups() const { return mark_dups || remove_dups; }
	bool index = false;                                        /* --index: out.bam.bai beside the output */
};
/* -1: go on; else the exit status, after the line that says why */
static int parse_options(int argc, char **argv, Options &o)
{
	static struct option longopts[] = {
		{ "num-diff", 1, 0, 'n' }, { "max-gap-open", 1, 0, 'o' }, { "max-gap-extensions", 1, 0, 'e' }, { "indel-near-end", 1, 0, 'i' },
		{ "deletion-occurences", 1, 0, 'd' }, { "seed-length", 1, 0, 'l' }, { "seed-mismatches", 1, 0, 'k' }, { "queue-size", 1, 0, 'm' },
		{ "num-threads", 1, 0, 't' }, { "mismatch-penalty", 1, 0, 'M' }, { "gap-open-penalty", 1, 0, 'O' }, { "gap-extension-penalty", 1, 0, 'E' },
		{ "max-best-hits", 1, 0, 'R' }, { "trim-quality", 1, 0, 'q' }, { "log-gap-penalty", 0, 0, 'L' }, { "non-iterative", 0, 0, 'N' },
		{ "output", 1, 0, 'f' }, { "genome", 1, 0, 'g' }, { "only-aligned", 0, 0, 128 }, { "drop-aligned", 0, 0, 133 }, { "debug-bam", 0, 0, 129 },
		{ "broken-input", 0, 0, 130 }, { "skip-duplicates", 0, 0, 131 }, { "temp-dir", 1, 0, 132 }, { "max-insert-size", 1, 0, 'a' },
		{ "max-occurences", 1, 0, 'C' }, { "max-occurences-se", 1, 0, 'D' }, { "max-hits", 1, 0, 'h' }, { "max-discordant-hits", 1, 0, 'H' },
		{ "chimeric-rate", 1, 0, 'c' }, { "disable-sw", 0, 0, 's' }, { "disable-isize-estimate", 0, 0, 'A' }, { "listen-port", 1, 0, 'p' }, { "sort", 0, 0, 134 }, { "damage", 1, 0, 135 },
		{ "mark-duplicates", 0, 0, 136 }, { "remove-duplicates", 0, 0, 137 }, { "index", 0, 0, 138 }, { 0, 0, 0, 0 } };
	nabwa_gap_opt_t &go = o.go; nabwa_pe_opt_t &po = o.po;
	nabwa_gap_init_opt(&go);
	nabwa_pe_opt_default(&po);
	const struct { int c; int *v; } ints[] = {                  /* options that set one integer ... */
		{ 'o', &go.max_gapo }, { 'M', &go.s_mm }, { 'O', &go.s_gapo }, { 'E', &go.s_gape }, { 'd', &go.max_del_occ }, { 'i', &go.indel_end_skip },
		{ 'l', &go.seed_len }, { 'k', &go.max_seed_diff }, { 'm', &go.max_entries }, { 't', &go.n_threads }, { 'R', &go.max_top2 }, { 'q', &go.trim_qual },
		{ 'C', &po.max_occ }, { 'D', &po.max_occ_se }, { 'a', &po.max_isize }, { 'h', &po.n_multi }, { 'H', &po.N_multi } };
	const struct { int c; uint32_t flag; } flags[] = {          /* ... and those that are a flag of the library */
		{ 128, NABWA_BAM_ONLY_ALIGNED }, { 129, NABWA_BAM_DEBUG }, { 130, NABWA_BAM_BROKEN_INPUT }, { 131, NABWA_BAM_SKIP_DUPLICATES }, { 133, NABWA_BAM_DROP_ALIGNED } };
	int c, opte = -1;
	while ((c = getopt_long(argc, argv, "g:n:o:e:i:d:l:k:LR:m:t:NM:O:E:q:f:C:D:a:sc:h:H:Ap:0:1:2:", longopts, 0)) >= 0) {
		bool in_table = false;
		for (const auto &x : ints) if (x.c == c) { *x.v = atoi(optarg); in_table = true; }
		for (const auto &x : flags) if (x.c == c) { o.rec_flags |= x.flag; in_table = true; }
		switch (c) {
			case 'g': o.prefix = optarg; break;
			case 'n': if (strstr(optarg, ".")) { go.fnr = (float)atof(optarg); go.max_diff = -1; } else { go.max_diff = atoi(optarg); go.fnr = -1.0f; } break;
			case 'e': opte = atoi(optarg); break;
			case 'L': go.mode |= NABWA_MODE_LOGGAP; break;
			case 'N': go.mode |= NABWA_MODE_NONSTOP; go.max_top2 = 0x7fffffff; break;
			case 'f': o.ofile = optarg; break;
			case 's': po.is_sw = 0; break;
			case 'c': po.ap_prior = atof(optarg); break;
			case 'A': po.force_isize = 1; break;
			case 132: o.temp_dir = optarg; break;
			case 134: o.sort = true; break;
			case 135: o.damage_file = optarg; break;
			case 136: o.mark_dups = true; break;
			case 137: o.remove_dups = true; break;
			case 138: o.index = true; break;
			case 'p': case '0': case '1': case '2':
				fprintf(stderr, "[nabwa_bam2bam] this option of bwa bam2bam is not provided (0MQ modes, .sai resume)\n");
				return 1;
			default: if (!in_table) return 1;
		}
	}
	if (opte > 0) { go.max_gape = opte; go.mode &= ~NABWA_MODE_GAPE; }
	/* the library's limits, said before the index is loaded */
	if (po.max_occ_se < 0 || po.max_occ_se > NABWA_MAX_MULTI - 1) { fprintf(stderr, "[nabwa_bam2bam] -D %d: at most %d other hits of a single read are listed\n", po.max_occ_se, NABWA_MAX_MULTI - 1); return 1; }
	if (po.n_multi < 0 || po.n_multi > NABWA_MAX_MULTI || po.N_multi < 0 || po.N_multi > NABWA_MAX_MULTI) { fprintf(stderr, "[nabwa_bam2bam] -h / -H: 0..%d\n", NABWA_MAX_MULTI); return 1; }
	if (go.s_mm < 1 || go.s_gapo < 1 || go.s_gape < 1) { fprintf(stderr, "[nabwa_bam2bam] -M / -O / -E must be at least 1\n"); return 1; }
	if (optind + 1 > argc || !o.prefix) {
		fprintf(stderr, "\nUsage:   nabwa_bam2bam -g PREFIX [options of bwa bam2bam] [--sort [--mark-duplicates | --remove-duplicates] [--index]] [--damage FILE] [-f out.bam] <in.bam>\n\n"
						"         --sort   write the records sorted by coordinate (@HD SO:coordinate; ties keep the input order).\n"
						"                  NABWA_SORT=gpu|host: who sorts a run (default gpu); NABWA_SORT_RUN_MIB: record bytes per run (default 1024)\n"
						"         --damage FILE   write the damage profile of the records to FILE: substitutions against the reference by distance from\n"
						"                  the read's ends, read lengths.  NABWA_DAMAGE_POS: positions per end, 1..256 (default 25); NABWA_DAMAGE_MAPQ:\n"
						"                  the lowest mapping quality counted (default 0)\n"
						"         --mark-duplicates   with --sort: set flag 0x400 on every record but the best of those that share their unclipped 5' end and\n"
						"                  strand (pairs: both ends); the best has the highest sum of base qualities.  Marked on the gpu; there is no host\n"
						"                  path, also under NABWA_SORT=host.  With --damage the profile then leaves the duplicates out\n"
						"         --remove-duplicates   the same, but the duplicates are dropped\n"
						"                  NABWA_MARKDUP_ENDS=5p|both: single reads are equal on their 5' end (default) or on both ends (merged reads);\n"
						"                  NABWA_MARKDUP_QUAL: the lowest base quality that counts, 0..93 (default 15)\n"
						"         --index   with --sort and -f: write the BAM index of the output to <out.bam>.bai, from the records as they are written.\n"
						"                  Built on the gpu; there is no host path, also under NABWA_SORT=host.  No reference sequence may be longer than 2^29\n\n");
		return 1;
	}
	o.input = argv[optind];
	/* NABWA_BGZF: who deflates the output -- host (default: zlib level 2 on host threads) or gpu (the library's compressor on the first
	 * GPU; other compressed bytes, the same inflated ones) or gpu-dynamic (the same with dynamic Huffman blocks where they are shorter) */
	const char *bgzf_env = getenv("NABWA_BGZF");
	o.bgzf_dynamic = bgzf_env && !strcmp(bgzf_env, "gpu-dynamic");
	o.bgzf_gpu = o.bgzf_dynamic || (bgzf_env && !strcmp(bgzf_env, "gpu"));
	if (bgzf_env && !o.bgzf_gpu && strcmp(bgzf_env, "host")) { fprintf(stderr, "[nabwa_bam2bam] NABWA_BGZF=%s: host, gpu or gpu-dynamic\n", bgzf_env); return 1; }
	/* NABWA_BGZF_IN: who inflates a BGZF input -- host (default: zlib on host threads) or gpu (the library's decompressor on the first
	 * GPU); any other gzip stream and a plain file are read on the host under either */
	const char *bgzf_in_env = getenv("NABWA_BGZF_IN");
	o.bgzf_in_gpu = bgzf_in_env && !strcmp(bgzf_in_env, "gpu");
	if (bgzf_in_env && !o.bgzf_in_gpu && strcmp(bgzf_in_env, "host")) { fprintf(stderr, "[nabwa_bam2bam] NABWA_BGZF_IN=%s: host or gpu\n", bgzf_in_env); return 1; }
	/* NABWA_FINISH: where the finishing chains cut reference windows, apply the CIGAR end rules and write MD / NM (the library reads it at
	 * every call); a value it would refuse is refused here, before the index is loaded */
	const char *finish_env = getenv("NABWA_FINISH");
	if (finish_env && strcmp(finish_env, "gpu") && strcmp(finish_env, "host")) { fprintf(stderr, "[nabwa_bam2bam] NABWA_FINISH=%s: host or gpu\n", finish_env); return 1; }
	if (!tool_dedup_ok()) return 1;      /* NABWA_DEDUP: the search batches read it (include/nabwa.h) */
	/* --sort only: NABWA_SORT, who sorts a run -- gpu (default: nabwa_bam_sort_run on the first GPU) or host (bam_sort_host.hpp; the same bytes) --
	 * and NABWA_SORT_RUN_MIB, the record bytes a run holds */
	if (o.sort) {
		const char *sort_env = getenv("NABWA_SORT");
		o.sort_host = sort_env && !strcmp(sort_env, "host");
		if (sort_env && !o.sort_host && strcmp(sort_env, "gpu")) { fprintf(stderr, "[nabwa_bam2bam] NABWA_SORT=%s: gpu or host\n", sort_env); return 1; }
		if (const char *k = getenv("NABWA_SORT_RUN_MIB")) {
			char *end = 0;
			const long v = strtol(k, &end, 10);
			if (end == k || *end || v < 1 || v > (1L << 20)) { fprintf(stderr, "[nabwa_bam2bam] NABWA_SORT_RUN_MIB=%s: a positive number of MiB\n", k); return 1; }
			o.sort_run_mib = v;
		}
	}
	/* --mark-duplicates, --remove-duplicates: one of them, with --sort; NABWA_MARKDUP_ENDS, which ends make single reads equal, and
	 * NABWA_MARKDUP_QUAL, the lowest base quality that counts */
	if (o.mark_dups && o.remove_dups) { fprintf(stderr, "[nabwa_bam2bam] --mark-duplicates and --remove-duplicates: one of the two\n"); return 1; }
	if (o.dups() && !o.sort) { fprintf(stderr, "[nabwa_bam2bam] %s needs --sort: the duplicates are known once the whole input is in\n", o.mark_dups ? "--mark-duplicates" : "--remove-duplicates"); return 1; }
	if (o.dups()) {
		nabwa_markdup_default_opt(&o.markdup);
		if (const char *k = getenv("NABWA_MARKDUP_ENDS")) {
			if (!strcmp(k, "5p")) o.markdup.single_ends = NABWA_MARKDUP_ENDS_5P;
			else if (!strcmp(k, "both")) o.markdup.single_ends = NABWA_MARKDUP_ENDS_BOTH;
			else { fprintf(stderr, "[nabwa_bam2bam] NABWA_MARKDUP_ENDS=%s: 5p or both\n", k); return 1; }
		}
		if (const char *k = getenv("NABWA_MARKDUP_QUAL")) {
			char *end = 0;
			const long v = strtol(k, &end, 10);
			if (end == k || *end || v < 0 || v > 93) { fprintf(stderr, "[nabwa_bam2bam] NABWA_MARKDUP_QUAL=%s: a base quality, 0 .. 93\n", k); return 1; }
			o.markdup.min_qual = (int32_t)v;
		}
	}
	/* --index: the index of a file in coordinate order, which has a name */
	if (o.index && !o.sort) { fprintf(stderr, "[nabwa_bam2bam] --index needs --sort: a BAM index is one of a file in coordinate order\n"); return 1; }
	if (o.index && !o.ofile) { fprintf(stderr, "[nabwa_bam2bam] --index needs -f out.bam: the index goes to out.bam.bai, and standard output has no name\n"); return 1; }
	/* --damage only: NABWA_DAMAGE_POS, the positions counted from either end, and NABWA_DAMAGE_MAPQ, the lowest mapping quality counted */
	if (o.damage_file) {
		nabwa_damage_default_opt(&o.damage);
		const struct { const char *name; int32_t *v; long lo, hi; const char *what; } vars[] = {
			{ "NABWA_DAMAGE_POS", &o.damage.n_pos, 1, NABWA_DAMAGE_MAX_POS, "1 .. 256 positions" }, { "NABWA_DAMAGE_MAPQ", &o.damage.min_mapq, 0, 255, "a mapping quality, 0 .. 255" } };
		for (const auto &x : vars)
			if (const char *k = getenv(x.name)) {
				char *end = 0;
				const long v = strtol(k, &end, 10);
				if (end == k || *end || v < x.lo || v > x.hi) { fprintf(stderr, "[nabwa_bam2bam] %s=%s: %s\n", x.name, k, x.what); return 1; }
				*x.v = (int32_t)v;
			}
	}
	return -1;
}

/* the input up to its first record: magic, header text, reference list (bamlite.c: bam_header_read).  Returns the text */
static std::string read_input_header(BamIn &in, const char *name)
{
	char magic[4]; int32_t l_text = 0, n_ref = 0;
	if (!in.read(magic, 4) || memcmp(magic, "BAM\1", 4) || !in.read(&l_text, 4) || l_text < 0) die(name, "not a BAM file");
	std::string old(l_text, '\0');
	if (l_text && !in.read(&old[0], l_text)) die(name, "truncated header");
	old.resize(strlen(old.c_str()));
	if (!in.read(&n_ref, 4)) die(name, "truncated header");
	for (int i = 0; i < n_ref; ++i) { int32_t ln, tl; if (!in.read(&ln, 4) || ln < 0) die(name, "truncated header"); std::vector<char> nm(ln); if (!in.read(nm.data(), ln) || !in.read(&tl, 4)) die(name, "truncated header"); }
	return old;
}
static void write_output_header(BgzfOut &out, nabwa_index_t *ix, const std::string &old, int argc, char **argv, bool coordinate)
{
	const std::string text = header_text([&](auto f) { each_contig(ix, f); }, old, argc, argv, VERSION, coordinate);
	const int32_t hl = (int32_t)text.size(), ns = nabwa_index_n_contigs(ix);
	out.write("BAM\1", 4); out.write(&hl, 4); out.write(text.data(), text.size()); out.write(&ns, 4);
	each_contig(ix, [&](const char *name, int32_t len) { const int32_t nl = (int32_t)strlen(name) + 1; out.write(&nl, 4); out.write(name, nl); out.write(&len, 4); });
}

/* ---------------------------------------------------------------- the records: a pipeline of threads, one stage each (DESIGN.md has the picture)
 *
 *   read_batches -in_ch-> create_batches -made_ch[g]-> search_on(g) -found_ch[g]-> pass1_loop, pass2_* -done_ch-> emit -out_ch-> write_out
 *                                                                                      with --sort:  emit -out_ch-> sort_runs -sorted_ch-> write_out
 *                                                                                      with --damage: emit -out_ch-> count_damage -counted_ch-> sort_runs or write_out
 *                                                             with --mark-duplicates:  emit -out_ch-> mark_duplicates -marked_ch-> sort_runs -sorted_ch-> write_out
 *                                                                     and --damage:    ... sort_runs -sorted_ch-> count_damage -counted_ch-> write_out
 *
 * read_batches inflates the input and cuts it into batches of records (mates stay together); create_batches parses them (host work only)
 * and deals them to the GPUs in turn; search_on(g), one thread per GPU, searches that GPU's batches as they come (no random numbers, no
 * order: the kernels of batch k + 1 run while batch k is positioned and finished).  The main thread takes the searched batches in input
 * order: everything that draws random numbers or fills the insert-size table happens there -- pass 1 for every batch (and pass 2 at once
 * for a batch of single reads), then, behind the barrier, pass 2 for what waited in memory or in the temporary file.  emit collects a
 * batch's output records and destroys it (host work only), a batch behind; write_out deflates and writes.
 * One path into the writer: whatever is written goes through done_ch, in the order the main thread put it there.
 * --sort puts one stage between emit and write_out: sort_runs collects records into runs of NABWA_SORT_RUN_MIB MiB, sorts each run by coordinate
 * (nabwa_bam_sort_run on the first GPU, or bam_sort_host under NABWA_SORT=host), keeps the sorted runs and their keys -- in memory, or with
 * --temp-dir in a second unlinked file there -- and at the end of the input hands the writer one run as it is or the merge of several, made
 * from the key arrays alone.  The writer still takes bytes from one thread in one order.
 * --damage puts one stage right behind emit: count_damage hands every piece of records to nabwa_damage_add on the first GPU and passes the bytes
 * on untouched; the tables add up in the handle, in any order, and main writes them at the end.
 * --mark-duplicates / --remove-duplicates put one stage in front of sort_runs: mark_duplicates hands every piece to nabwa_markdup_add on the
 * first GPU and passes it on untouched; a piece is a whole batch, and read_batches keeps mates in one batch, so mates reach the library next
 * to each other.  The records' ordinals are their places in the stream sort_runs takes; each run keeps them beside its keys (run base + the
 * sort's permutation).  When the input ends the stage resolves once, and sort_runs, as it hands over or merges, sets 0x400 on a duplicate
 * or leaves it out.  --damage then counts behind the sort, on what leaves.
 * --index puts one stage right in front of write_out (behind count_damage where that one is there too): index_records hands every piece to
 * nabwa_bai_add on the first GPU with the offset the writer will give it in the uncompressed stream -- the header's length, then what went
 * before -- and passes it on untouched; it sees exactly the records that are written.  BgzfOut notes where each block it writes starts, and
 * main finishes the index from that table once the file is closed. */
struct InBatch { std::vector<uint8_t> buf; std::vector<int64_t> off; };
struct OutBytes { std::unique_ptr<uint8_t[]> p; size_t n = 0; std::vector<int64_t> off; };      /* no zero fill: the library writes every byte.  off: --sort and --damage, the records' offsets where emit has them */
/* a sorted run of --sort: its records in key order (in memory, or n bytes from `at` in the run file), their offsets and their keys */
struct SortedRun { std::unique_ptr<uint8_t[]> p; size_t n = 0; long at = 0; std::vector<int64_t> off; std::vector<uint64_t> keys; std::vector<uint64_t> ords; };      /* ords: --mark-duplicates, the records' ordinals */
struct Finished { nabwa_bam_batch_t *batch = 0; OutBytes bytes; };     /* what emit takes: a batch whose records it collects, or (no batch) records already made */
typedef Chan<nabwa_bam_batch_t*> BatchChan;

struct Pipeline {
	const Options &opt; const std::vector<nabwa_index_t*> &ixs; BamIn &in; BgzfOut &out;
	const size_t n_dev; const long batch_records;             /* NABWA_BAM_BATCH */
	Chan<InBatch> in_ch{2};
	std::vector<std::unique_ptr<BatchChan>> made_ch, found_ch; /* per GPU: parsed batches, searched batches */
	Chan<Finished> done_ch{1};
	Chan<OutBytes> out_ch{2};
	/* --sort */
	Chan<OutBytes> sorted_ch{2};
	nabwa_bam_sort_t *sorter = 0;                             /* null under NABWA_SORT=host */
	std::vector<SortedRun> runs;
	FILE *run_file = 0;                                       /* --temp-dir: the sorted runs wait there */
	uint64_t n_sorted = 0; double t_sort = 0;
	/* --damage */
	Chan<OutBytes> counted_ch{2};
	nabwa_damage_t *damage = 0;
	double t_damage = 0;
	/* --mark-duplicates, --remove-duplicates */
	Chan<OutBytes> marked_ch{2};
	nabwa_markdup_t *markdup = 0;
	std::vector<uint8_t> dup;                                 /* by ordinal, once mark_duplicates has closed marked_ch */
	uint64_t dup_stats[NABWA_MARKDUP_N_STATS] = {};
	uint64_t n_run_base = 0, n_marked_in = 0;                 /* records in the runs sorted so far; records the marker has taken */
	double t_markdup = 0;
	/* --index */
	Chan<OutBytes> indexed_ch{2};
	nabwa_bai_t *bai = 0;
	int64_t index_at = 0;                                     /* where the next piece lies in the uncompressed stream: behind the header, then behind what was passed on */
	double t_index = 0;
	/* the main thread's: the insert-size table, the random numbers (srand48(bns->seed), bam2bam.c:1745), what waits for pass 2 */
	nabwa_isize_table_t *tab; uint64_t rng;
	std::vector<nabwa_bam_batch_t*> waiting;
	FILE *spill = 0; std::vector<Spilled> spilled;            /* --temp-dir: it waits in a file there instead */
	uint64_t n_tot[2] = { 0, 0 }, n_mapped[2] = { 0, 0 };
	long tot_seqs = 0; bool any_pairs = false;
	/* NABWA_TIMING, each written by one stage */
	double t_read = 0, t_write = 0, t_wait_in = 0, t_lib = 0, t_wait_out = 0, t_call[5] = { 0, 0, 0, 0, 0 };      /* create, pass 1, pass 2, output, destroy */
	std::vector<double> t_search;

	Pipeline(const Options &opt_, const std::vector<nabwa_index_t*> &ixs_, BamIn &in_, BgzfOut &out_, int64_t genome_len, uint32_t seed)
		: opt(opt_), ixs(ixs_), in(in_), out(out_), n_dev(ixs_.size()), batch_records(getenv("NABWA_BAM_BATCH") ? atol(getenv("NABWA_BAM_BATCH")) : (1L << 20)),
		  tab(nabwa_isize_table_create(opt_.po.ap_prior, genome_len)), rng(((uint64_t)seed << 16) | 0x330E), t_search(ixs_.size(), 0.0)
	{
		for (size_t g = 0; g < n_dev; ++g) { made_ch.emplace_back(new BatchChan(1)); found_ch.emplace_back(new BatchChan(1)); }
		if (opt.temp_dir) {                                   /* made with mkstemp and unlinked at once, as the reference's is at exit */
			std::string tn = std::string(opt.temp_dir) + "/nabwa_bam2bam_XXXXXX";
			const int fd = mkstemp(&tn[0]);
			if (fd < 0 || !(spill = fdopen(fd, "w+b"))) die(opt.temp_dir, "cannot create a temporary file there");
			unlink(tn.c_str());
			if (opt.sort) {
				std::string rn = std::string(opt.temp_dir) + "/nabwa_bam2bam_runs_XXXXXX";
				const int rfd = mkstemp(&rn[0]);
				if (rfd < 0 || !(run_file = fdopen(rfd, "w+b"))) die(opt.temp_dir, "cannot create a temporary file there");
				unlink(rn.c_str());
			}
		}
	}

	void read_batches()
	{
		const double t0 = now_s();
		InBatch cur; cur.off.assign(1, 0);
		bool hold_mate = false;                                   /* the last record is a paired read that waits for the record after it */
		size_t held_at = 0;                                       /* where it starts in buf */
		double t_blocked = 0;
		auto hand_over = [&]() {
			if (cur.off.size() > 1) { const double tb = now_s(); in_ch.put(std::move(cur)); t_blocked += now_s() - tb; }
			cur = InBatch(); cur.off.assign(1, 0);
		};
		for (;;) {
			if (in.need(4) == 0) break;
			uint32_t bs = 0;
			if (!in.read(&bs, 4) || bs < 32) die(opt.input, "truncated record");
			std::vector<uint8_t> &buf = cur.buf;
			const size_t at = buf.size();
			if (buf.capacity() < at + 4 + bs) buf.reserve(buf.capacity() ? 2 * buf.capacity() + 4 + bs : (size_t)256 << 20);
			buf.resize(at + 4 + bs); memcpy(&buf[at], &bs, 4);
			if (!in.read(&buf[at + 4], bs)) die(opt.input, "truncated record");
			uint32_t z; memcpy(&z, &buf[at + 16], 4);
			const bool paired = (z >> 16) & 1;
			{	/* the name is read as a C string below and by the library: it must lie, terminated, inside the record */
				const uint32_t l_qname = buf[at + 12];
				if (l_qname == 0 || bs < 32 + l_qname || buf[at + 36 + l_qname - 1] != 0) die(opt.input, "damaged record (read name not terminated inside the record)");
			}
			cur.off.push_back((int64_t)buf.size());
			/* read_bam_pair_core's view of the stream (bwaseqio.c:345-410): a paired read takes the next record as its mate if the names
			 * agree; if they do not it is a lone mate (an error, or dropped with --broken-input) and the next record starts afresh */
			const bool mates = hold_mate && !strcmp((const char*)&buf[held_at + 36], (const char*)&buf[at + 36]);
			hold_mate = mates ? false : paired;
			held_at = at;
			if ((long)cur.off.size() - 1 >= batch_records && !hold_mate) hand_over();
		}
		hand_over();
		in_ch.close();
		t_read = now_s() - t0 - t_blocked;
	}
	void create_batches()
	{
		InBatch ib;
		for (size_t k = 0; in_ch.get(ib); ++k) {
			const double t0 = now_s();
			nabwa_bam_batch_t *b = 0;
			if (nabwa_bam_batch_create_ex(ixs[k % n_dev], &opt.go, &opt.po, opt.rec_flags, (int)ib.off.size() - 1, ib.buf.data(), ib.off.data(), &b) != NABWA_OK) die("input records", nabwa_last_error());
			std::vector<uint8_t>().swap(ib.buf);
			t_call[0] += now_s() - t0;
			made_ch[k % n_dev]->put(std::move(b));
		}
		for (auto &c : made_ch) c->close();
	}
	void search_on(size_t g)
	{
		nabwa_bam_batch_t *b;
		while (made_ch[g]->get(b)) {
			const double t0 = now_s();
			if (nabwa_bam_batch_search(b) != NABWA_OK) die("search", nabwa_last_error());
			t_search[g] += now_s() - t0;
			found_ch[g]->put(std::move(b));
		}
		found_ch[g]->close();
	}
	void finished(nabwa_bam_batch_t *b) { Finished f; f.batch = b; done_ch.put(std::move(f)); }
	/* pass 1 over the batches in input order.  A batch of single reads needs no insert-size estimate: it gets pass 2 now, and is
	 * written now unless pairs came before it */
	void pass1_loop()
	{
		for (size_t k = 0; ; ++k) {
			nabwa_bam_batch_t *b = 0;
			const double t0 = now_s();
			if (!found_ch[k % n_dev]->get(b)) break;
			const double t1 = now_s();
			t_wait_in += t1 - t0;
			if (nabwa_bam_batch_pass1(b, &rng, tab) != NABWA_OK) die("pass 1", nabwa_last_error());
			const double td = now_s();
			t_call[1] += td - t1;
			int nr = 0, nl = 0; nabwa_bam_batch_counts(b, &nr, &nl);
			any_pairs |= nr != nl;
			tot_seqs += nr;
			fprintf(stderr, "[nabwa_bam2bam] pass 1: %ld sequences processed\n", tot_seqs);
			if (nr == nl && nabwa_bam_batch_pass2(b, tab, n_tot, n_mapped) != NABWA_OK) die("pass 2", nabwa_last_error());
			const double t2 = now_s();
			if (nr == nl) t_call[2] += t2 - td;
			if (nr == nl && !any_pairs) finished(b);
			else if (spill) { Spilled S; S.dev = k % n_dev; spill_batch(spill, b, nr == nl, S); spilled.push_back(S); nabwa_bam_batch_destroy(b); }
			else waiting.push_back(b);
			t_lib += t2 - t1;
		}
	}
	/* behind the barrier: pass 2 in input order; emit collects a batch while the next is finished */
	void pass2_waiting()
	{
		for (nabwa_bam_batch_t *b : waiting) {
			const double t1 = now_s();
			int nr = 0, nl = 0; nabwa_bam_batch_counts(b, &nr, &nl);
			if (nr != nl && nabwa_bam_batch_pass2(b, tab, n_tot, n_mapped) != NABWA_OK) die("pass 2", nabwa_last_error());
			t_lib += now_s() - t1; t_call[2] += now_s() - t1;
			finished(b);
		}
	}
	void pass2_spilled()
	{
		std::vector<uint8_t> stream; std::vector<int64_t> off; std::vector<nabwa_wire_read_t> st; std::vector<std::vector<uint8_t>> keep;
		for (const Spilled &S : spilled) {
			const double t1 = now_s();
			unspill_batch(spill, S, stream, off, st, keep);
			if (S.finished) {                                     /* single reads that only waited for their turn: their records as they are */
				std::vector<int64_t> pick;
				size_t nb = 0;
				for (size_t i = 0; i + 1 < off.size(); ++i) {     /* --only-aligned (pair_print_bam, bam2bam.c:911-925) on the finished records */
					uint32_t z; memcpy(&z, &stream[(size_t)off[i] + 16], 4);
					if ((opt.rec_flags & NABWA_BAM_ONLY_ALIGNED) && ((z >> 16) & 4)) continue;
					pick.push_back((int64_t)i); nb += (size_t)(off[i + 1] - off[i]);
				}
				Finished f; f.bytes.p.reset(new uint8_t[nb ? nb : 1]); f.bytes.n = nb;
				size_t w = 0;
				for (int64_t i : pick) { memcpy(f.bytes.p.get() + w, &stream[(size_t)off[(size_t)i]], (size_t)(off[(size_t)i + 1] - off[(size_t)i])); w += (size_t)(off[(size_t)i + 1] - off[(size_t)i]); }
				done_ch.put(std::move(f));
				continue;
			}
			nabwa_bam_batch_t *b = 0;
			if (nabwa_bam_batch_create_ex(ixs[S.dev], &opt.go, &opt.po, opt.rec_flags & ~(uint32_t)(NABWA_BAM_BROKEN_INPUT | NABWA_BAM_DROP_ALIGNED), S.n_records, stream.data(), off.data(), &b) != NABWA_OK
				|| nabwa_bam_batch_restore(b, st.data()) != NABWA_OK || nabwa_bam_batch_pass2(b, tab, n_tot, n_mapped) != NABWA_OK) die("pass 2", nabwa_last_error());
			t_lib += now_s() - t1; t_call[2] += now_s() - t1;
			finished(b);
		}
		if (spill) fclose(spill);
	}
	void emit()
	{
		Finished f;
		while (done_ch.get(f)) {
			if (nabwa_bam_batch_t *b = f.batch) {
				int64_t nb = 0;
				const double ta = now_s();
				std::vector<int64_t> &oo = f.bytes.off;               /* --sort, --damage: the offsets too */
				const bool want_off = opt.sort || opt.damage_file;
				if (want_off) { int nr = 0, nl = 0; nabwa_bam_batch_counts(b, &nr, &nl); oo.assign((size_t)nr + 1, 0); }
				nabwa_bam_batch_output(b, 0, 0, 0, &nb);
				f.bytes.p.reset(new uint8_t[(size_t)(nb ? nb : 1)]); f.bytes.n = (size_t)nb;
				if (nabwa_bam_batch_output(b, f.bytes.p.get(), nb, want_off ? oo.data() : 0, &nb) != NABWA_OK) die("output", nabwa_last_error());
				while (oo.size() > 1 && oo[oo.size() - 1] == oo[oo.size() - 2]) oo.pop_back();      /* --only-aligned: the records that are there */
				const double tb = now_s();
				nabwa_bam_batch_destroy(b);
				t_call[3] += tb - ta; t_call[4] += now_s() - tb;
			}
			const double t0 = now_s();
			out_ch.put(std::move(f.bytes));
			t_wait_out += now_s() - t0;
		}
		out_ch.close();
	}
	/* records that came ready-made from the temporary file: their offsets, from the block_size words */
	static void walk_records(const OutBytes &o, std::vector<int64_t> &walked, const char *who)
	{
		walked.assign(1, 0);
		for (size_t q = 0; q < o.n; ) { uint32_t bs; if (o.n - q < 4) die(who, "a record cut short"); memcpy(&bs, o.p.get() + q, 4); q += 4 + (size_t)bs; if (q > o.n) die(who, "a record cut short"); walked.push_back((int64_t)q); }
	}
	/* what emit made, for the stage behind the optional ones */
	Chan<OutBytes> &emitted() { return opt.dups() ? marked_ch : opt.damage_file ? counted_ch : out_ch; }
	/* --mark-duplicates: every piece of records through nabwa_markdup_add, then on as it is; the marks once the input has ended */
	void mark_duplicates()
	{
		OutBytes o;
		while (out_ch.get(o)) {
			const double t0 = now_s();
			if (o.off.empty()) walk_records(o, o.off, "duplicates");
			if (nabwa_markdup_add(markdup, (int64_t)o.off.size() - 1, o.p.get(), o.off.data()) != NABWA_OK) die("duplicates", nabwa_last_error());
			n_marked_in += (uint64_t)o.off.size() - 1;
			t_markdup += now_s() - t0;
			marked_ch.put(std::move(o));
		}
		const double t0 = now_s();
		dup.assign((size_t)(n_marked_in ? n_marked_in : 1), 0);
		if (nabwa_markdup_resolve(markdup, dup.data(), (int64_t)n_marked_in, dup_stats) != NABWA_OK) die("duplicates", nabwa_last_error());
		t_markdup += now_s() - t0;
		marked_ch.close();
	}
	/* --damage: every piece of records through nabwa_damage_add, then on as it is (with its offsets, which --sort takes as emit's) */
	void count_damage()
	{
		OutBytes o;
		Chan<OutBytes> &from = opt.dups() ? sorted_ch : out_ch;      /* behind the marker: the duplicates are flagged or gone */
		while (from.get(o)) {
			const double t0 = now_s();
			if (o.off.empty()) walk_records(o, o.off, "damage");
			if (nabwa_damage_add(damage, (int64_t)o.off.size() - 1, o.p.get(), o.off.data()) != NABWA_OK) die("damage", nabwa_last_error());
			t_damage += now_s() - t0;
			counted_ch.put(std::move(o));
		}
		counted_ch.close();
	}
	/* --sort: one run, in[off[0] .. off[n]) -> sorted, kept */
	void sort_run(const std::vector<uint8_t> &in, const std::vector<int64_t> &off)
	{
		const int64_t n = (int64_t)off.size() - 1;
		if (n <= 0) return;
		SortedRun r;
		r.n = in.size(); r.p.reset(new uint8_t[r.n]); r.off.resize((size_t)n + 1); r.keys.resize((size_t)n);
		std::vector<uint32_t> perm(opt.dups() ? (size_t)n : 0);
		uint32_t *perm_out = opt.dups() ? perm.data() : 0;
		if (sorter) {
			if (nabwa_bam_sort_run_ex(sorter, n, in.data(), off.data(), r.p.get(), (int64_t)r.n, r.off.data(), r.keys.data(), perm_out) != NABWA_OK) die("sort", nabwa_last_error());
		} else {
			const int64_t bad = bam_sort_host(io_threads(), n, in.data(), off.data(), r.p.get(), r.off.data(), r.keys.data(), perm_out);
			if (bad >= 0) die("sort", ("record " + std::to_string(bad) + " of a run: its block_size is not what its offsets say").c_str());
		}
		if (opt.dups()) { r.ords.resize((size_t)n); for (int64_t i = 0; i < n; ++i) r.ords[(size_t)i] = n_run_base + perm[(size_t)i]; }
		n_run_base += (uint64_t)n;
		if (run_file) {
			r.at = ftell(run_file);
			if (fwrite(r.p.get(), 1, r.n, run_file) != r.n) die("temporary file", "cannot write");
			r.p.reset();
		}
		n_sorted += (uint64_t)n;
		runs.push_back(std::move(r));
	}
	/* bytes [o, o + n) of run r for the merge: where they lie in memory, or read from the run file through the run's window */
	struct RunWindow { std::vector<uint8_t> buf; int64_t lo = 0, hi = 0; };
	const uint8_t *run_bytes(size_t r, int64_t o, int64_t n, std::vector<RunWindow> &win)
	{
		const SortedRun &R = runs[r];
		if (R.p) return R.p.get() + o;
		RunWindow &w = win[r];
		if (o < w.lo || o + n > w.hi) {
			int64_t len = n > (8 << 20) ? n : (8 << 20);
			if (len > (int64_t)R.n - o) len = (int64_t)R.n - o;
			w.buf.resize((size_t)len);
			if (pread(fileno(run_file), w.buf.data(), (size_t)len, (off_t)(R.at + o)) != (ssize_t)len) die("temporary file", "truncated");
			w.lo = o; w.hi = o + len;
		}
		return w.buf.data() + (o - w.lo);
	}
	void sort_runs()
	{
		const size_t limit = (size_t)opt.sort_run_mib << 20, CHUNK = (size_t)64 << 20;
		std::vector<uint8_t> cur; std::vector<int64_t> cur_off(1, 0), walked;
		OutBytes o;
		while (emitted().get(o)) {
			const double t0 = now_s();
			if (o.off.empty()) walk_records(o, walked, "sort");
			const std::vector<int64_t> &off = o.off.empty() ? walked : o.off;
			const size_t nrec = off.size() - 1;
			for (size_t i = 0; i < nrec; ) {
				/* records i .. j - 1 go into the run: up to and including the one that fills it */
				const int64_t room = (int64_t)(limit - cur.size());
				size_t j = (size_t)(std::lower_bound(off.begin() + i + 1, off.end(), off[i] + room) - off.begin());
				j = j < nrec ? j : nrec;
				if (cur.capacity() < cur.size() + (size_t)(off[j] - off[i])) cur.reserve(std::max(2 * cur.capacity(), cur.size() + (size_t)(off[j] - off[i])));
				const int64_t shift = (int64_t)cur.size() - off[i];
				cur.insert(cur.end(), o.p.get() + off[i], o.p.get() + off[j]);
				for (size_t k = i + 1; k <= j; ++k) cur_off.push_back(off[k] + shift);
				i = j;
				if (cur.size() >= limit) { sort_run(cur, cur_off); cur.clear(); cur_off.assign(1, 0); }
			}
			o.p.reset();
			t_sort += now_s() - t0;
		}
		const double t0 = now_s();
		sort_run(cur, cur_off);
		std::vector<uint8_t>().swap(cur);
		if (run_file && fflush(run_file) != 0) die("temporary file", "cannot write");
		double t_blocked = 0;
		auto hand_over = [&](OutBytes &&x) { const double tb = now_s(); sorted_ch.put(std::move(x)); t_blocked += now_s() - tb; };
		auto is_dup = [&](size_t r, size_t i) { return opt.dups() && dup[(size_t)runs[r].ords[i]] != 0; };
		if (runs.size() == 1 && runs[0].p) {                      /* one run: as it is, but for the duplicates -- flagged where they lie, or the rest moved up over them */
			OutBytes x; x.p = std::move(runs[0].p); x.n = runs[0].n;
			if (opt.dups()) {
				const SortedRun &R = runs[0];
				size_t w = 0;
				for (size_t i = 0; i + 1 < R.off.size(); ++i) {
					const size_t at = (size_t)R.off[i], n = (size_t)(R.off[i + 1] - R.off[i]);
					const bool d = is_dup(0, i);
					if (d && opt.remove_dups) continue;
					if (d) x.p[at + 19] |= 0x04;                      /* flag 0x400: bytes 18 .. 19 of the record */
					if (w != at) memmove(x.p.get() + w, x.p.get() + at, n);
					w += n;
				}
				x.n = w;
			}
			hand_over(std::move(x));
		} else if (!runs.empty()) {                               /* several: merged by their keys alone, ties to the earlier run (one run in the file: read back in order) */
			std::vector<const std::vector<uint64_t>*> keys;
			for (const SortedRun &r : runs) keys.push_back(&r.keys);
			std::vector<RunWindow> win(runs.size());
			OutBytes x; size_t x_cap = 0;
			bam_sort_merge(keys, [&](size_t r, size_t i) {
				const int64_t at = runs[r].off[i], n = runs[r].off[i + 1] - at;
				const bool d = is_dup(r, i);
				if (d && opt.remove_dups) return;
				if (x.n + (size_t)n > x_cap) {
					if (x.n) hand_over(std::move(x));
					x = OutBytes(); x_cap = (size_t)n > CHUNK ? (size_t)n : CHUNK; x.p.reset(new uint8_t[x_cap]);
				}
				memcpy(x.p.get() + x.n, run_bytes(r, at, n, win), (size_t)n);
				if (d) x.p[x.n + 19] |= 0x04;
				x.n += (size_t)n;
			});
			if (x.n) hand_over(std::move(x));
		}
		if (run_file) fclose(run_file);
		sorted_ch.close();
		t_sort += now_s() - t0 - t_blocked;
	}
	/* what leaves for the file, in the file's order */
	Chan<OutBytes> &leaving() { return opt.dups() && opt.damage_file ? counted_ch : opt.sort ? sorted_ch : emitted(); }
	/* --index: every piece through nabwa_bai_add with the stream offset it is written at, then on as it is */
	void index_records()
	{
		OutBytes o;
		std::vector<int64_t> walked;
		while (leaving().get(o)) {
			const double t0 = now_s();
			if (o.off.empty()) walk_records(o, walked, "index");
			const std::vector<int64_t> &off = o.off.empty() ? walked : o.off;
			if (nabwa_bai_add(bai, (int64_t)off.size() - 1, o.p.get(), off.data(), index_at) != NABWA_OK) die("index", nabwa_last_error());
			index_at += (int64_t)o.n;
			t_index += now_s() - t0;
			indexed_ch.put(std::move(o));
		}
		indexed_ch.close();
	}
	void write_out()
	{
		Chan<OutBytes> &from = opt.index ? indexed_ch : leaving();
		OutBytes o;
		while (from.get(o)) { const double t0 = now_s(); out.write(o.p.get(), o.n); o.p.reset(); t_write += now_s() - t0; }
	}
};

/* --damage: the handle's tables as text into `path`, made to be diffed: the stats by name, a row per end and position (the row behind the
 * last position: everything further in), the read lengths that occur.  Returns the summary line for stderr: the records counted and the two
 * frequencies ancient DNA is known by -- C>T at the first 5' base and G>A at the first 3' base, each among the reference's C resp. G there */
static std::string write_damage_profile(nabwa_damage_t *d, int n_pos, const char *path)
{
	static const char *const stat_names[NABWA_DAMAGE_N_STATS] = { "seen", "counted", "skipped_flags", "skipped_place", "skipped_mapq", "skipped_empty",
																   "columns_counted", "columns_skipped_read", "columns_skipped_ref" };
	std::vector<uint64_t> sub[2] = { std::vector<uint64_t>((size_t)(n_pos + 1) * 16), std::vector<uint64_t>((size_t)(n_pos + 1) * 16) }, len(NABWA_DAMAGE_LEN_BINS), stats(NABWA_DAMAGE_N_STATS);
	if (nabwa_damage_fetch(d, sub[0].data(), sub[1].data(), len.data(), stats.data()) != NABWA_OK) die("damage", nabwa_last_error());
	FILE *f = fopen(path, "w");
	if (!f) die(path, "cannot create");
	fprintf(f, "# nabwa damage profile v1\n");
	for (int k = 0; k < NABWA_DAMAGE_N_STATS; ++k) fprintf(f, "# %s %llu\n", stat_names[k], (unsigned long long)stats[(size_t)k]);
	fprintf(f, "end\tpos");
	for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) fprintf(f, "\t%c>%c", "ACGT"[r], "ACGT"[q]);
	fprintf(f, "\n");
	for (int e = 0; e < 2; ++e)
		for (int p = 0; p <= n_pos; ++p) {
			if (p < n_pos) fprintf(f, "%s\t%d", e ? "3p" : "5p", p + 1); else fprintf(f, "%s\t>%d", e ? "3p" : "5p", n_pos);
			for (int k = 0; k < 16; ++k) fprintf(f, "\t%llu", (unsigned long long)sub[e][(size_t)p * 16 + (size_t)k]);
			fprintf(f, "\n");
		}
	for (int L = 0; L < NABWA_DAMAGE_LEN_BINS; ++L) if (len[(size_t)L]) fprintf(f, "len\t%d\t%llu\n", L, (unsigned long long)len[(size_t)L]);
	if (fclose(f) != 0) die(path, "cannot write");
	auto freq = [&](int e, int r, int q) {
		uint64_t tot = 0;
		for (int k = 0; k < 4; ++k) tot += sub[e][(size_t)(r * 4 + k)];
		char b[32];
		if (tot) snprintf(b, sizeof b, "%.4f", (double)sub[e][(size_t)(r * 4 + q)] / (double)tot); else snprintf(b, sizeof b, "nan");
		return std::string(b);
	};
	return "[nabwa_bam2bam] damage profile of " + std::to_string((unsigned long long)stats[NABWA_DAMAGE_STAT_COUNTED]) + " records: 5' C>T at position 1 " + freq(0, 1, 3)
		   + ", 3' G>A at position 1 " + freq(1, 2, 0) + "\n";
}

int main(int argc, char **argv)
{
	const double t_main = now_s();
	Options opt;
	const int bad = parse_options(argc, argv, opt);
	if (bad >= 0) return bad;
	/* one index replica per GPU of NABWA_DEVICES ("0,1,2,3"; default: NABWA_DEVICE or 0); batches are dealt to them in turn */
	const std::vector<int> devices = tool_devices();
	nabwa_bgzf_t *bgzf = 0;
	if (opt.bgzf_gpu && nabwa_bgzf_create(devices[0], &bgzf) != NABWA_OK) { fprintf(stderr, "[nabwa_bam2bam] BGZF on the GPU: %s\n", nabwa_last_error()); return 2; }
	/* the reader's handle is its own: a handle takes one call at a time, and reader and writer are two threads */
	nabwa_bgzf_t *bgzf_in = 0;
	if (opt.bgzf_in_gpu && nabwa_bgzf_create(devices[0], &bgzf_in) != NABWA_OK) { fprintf(stderr, "[nabwa_bam2bam] BGZF on the GPU: %s\n", nabwa_last_error()); return 2; }
	/* --sort on the GPU: its handle now, so that a run without a usable device ends before anything is written */
	nabwa_bam_sort_t *sorter = 0;
	if (opt.sort && !opt.sort_host && nabwa_bam_sort_create(devices[0], &sorter) != NABWA_OK) { fprintf(stderr, "[nabwa_bam2bam] --sort on the GPU: %s\n", nabwa_last_error()); return 2; }
	/* --mark-duplicates, --remove-duplicates: the handle on the first GPU now, for the same reason; there is no host path, whatever NABWA_SORT says */
	nabwa_markdup_t *markdup = 0;
	if (opt.dups() && nabwa_markdup_create(devices[0], &opt.markdup, &markdup) != NABWA_OK) { fprintf(stderr, "[nabwa_bam2bam] %s on the GPU: %s\n", opt.mark_dups ? "--mark-duplicates" : "--remove-duplicates", nabwa_last_error()); return 2; }
	/* --index builds on the first GPU, through a handle made below, once the index says how many reference sequences there are */
	if (opt.index && nabwa_device_count() <= devices[0]) { fprintf(stderr, "[nabwa_bam2bam] --index on the GPU: no HIP device %d\n", devices[0]); return 2; }
	/* --damage counts on the first GPU, through a handle on that GPU's index (made below, once the index is there): no such device ends the run here */
	if (opt.damage_file && nabwa_device_count() <= devices[0]) { fprintf(stderr, "[nabwa_bam2bam] --damage on the GPU: no HIP device %d\n", devices[0]); return 2; }
	std::vector<nabwa_index_t*> ixs;
	{
		std::string err;
		if (load_replicas(opt.prefix, devices, 1, 1, ixs, err) >= 0) die("genome index", err.c_str());
	}
	int64_t genome_len = 0; uint32_t seed = 0;
	nabwa_index_reference_info(ixs[0], &genome_len, &seed);
	fprintf(stderr, "[nabwa_bam2bam] genome length is %ld\n", (long)genome_len);
	/* --damage: its handle on the first GPU's index now, so that a run that cannot count ends before anything is written */
	nabwa_damage_t *damage = 0;
	if (opt.damage_file && nabwa_damage_create(ixs[0], &opt.damage, &damage) != NABWA_OK) { fprintf(stderr, "[nabwa_bam2bam] --damage on the GPU: %s\n", nabwa_last_error()); return 2; }

	/* --index: a .bai addresses 2^29 bases of a reference sequence; its handle now, so that a run that cannot index ends before anything is written */
	nabwa_bai_t *bai = 0;
	if (opt.index) {
		each_contig(ixs[0], [&](const char *name, int32_t len) {
			if ((int64_t)len > ((int64_t)1 << 29)) { fprintf(stderr, "[nabwa_bam2bam] --index: reference sequence %s has %ld bases, a BAM index addresses 536870912\n", name, (long)len); exit(1); }
		});
		if (nabwa_bai_create(devices[0], nabwa_index_n_contigs(ixs[0]), &bai) != NABWA_OK) { fprintf(stderr, "[nabwa_bam2bam] --index on the GPU: %s\n", nabwa_last_error()); return 2; }
	}

	FILE *inf = strcmp(opt.input, "-") ? fopen(opt.input, "rb") : stdin;
	if (!inf) die(opt.input, "cannot open");
	BamIn in(inf, opt.input);
	if (bgzf_in) in.inflater = [bgzf_in](const uint8_t *cmp, size_t from, size_t to, const std::vector<BamIn::Blk> &blk, uint8_t *plain, std::string &why) {
		const size_t first = blk.front().dst, end = blk.back().dst + blk.back().isize;
		int64_t n_out = 0, nb = 0;
		if (nabwa_bgzf_handle_decompress(bgzf_in, cmp + from, (int64_t)(to - from), plain + first, (int64_t)(end - first), &n_out, &nb) == NABWA_OK) return true;
		why = nabwa_last_error();
		return false;
	};
	const std::string old = read_input_header(in, opt.input);
	FILE *of = opt.ofile ? fopen(opt.ofile, "wb") : stdout;
	if (!of) die(opt.ofile, "cannot create");
	BgzfOut out{ of, {}, 2, bgzf, {} };
	if (opt.bgzf_dynamic) out.codes = NABWA_BGZF_CODES_DYNAMIC;
	out.track = opt.index;
	write_output_header(out, ixs[0], old, argc, argv, opt.sort);

	const bool timing = getenv("NABWA_TIMING") != 0;
	const double t_loop = now_s();
	Pipeline P(opt, ixs, in, out, genome_len, seed);
	P.sorter = sorter;
	P.damage = damage;
	P.markdup = markdup;
	P.bai = bai; P.index_at = (int64_t)out.n_taken;
	std::thread sort_thread, damage_thread, markdup_thread, index_thread;
	if (bai) index_thread = std::thread(&Pipeline::index_records, &P);
	if (markdup) markdup_thread = std::thread(&Pipeline::mark_duplicates, &P);
	if (damage) damage_thread = std::thread(&Pipeline::count_damage, &P);
	if (opt.sort) sort_thread = std::thread(&Pipeline::sort_runs, &P);
	std::thread reader(&Pipeline::read_batches, &P), creator(&Pipeline::create_batches, &P), finisher(&Pipeline::emit, &P), writer(&Pipeline::write_out, &P);
	std::vector<std::thread> searchers;
	for (size_t g = 0; g < P.n_dev; ++g) searchers.emplace_back(&Pipeline::search_on, &P, g);
	P.pass1_loop();
	reader.join(); creator.join();
	for (auto &x : searchers) x.join();
	if (inf != stdin) fclose(inf);
	nabwa_isize_table_infer_all(P.tab);                        /* the barrier (infer_all_isizes) */
	P.pass2_waiting();
	P.pass2_spilled();
	P.done_ch.close();
	finisher.join();
	if (markdup) markdup_thread.join();
	if (damage && !markdup) damage_thread.join();
	if (opt.sort) sort_thread.join();
	if (damage && markdup) damage_thread.join();
	if (bai) index_thread.join();
	writer.join();

	if (timing) fprintf(stderr, "[nabwa_bam2bam] timing: start-up (device, index, headers) %.3f s, records %.3f s\n", t_loop - t_main, now_s() - t_loop);
	if (timing) { double ts = 0; for (double x : P.t_search) ts += x; fprintf(stderr, "[nabwa_bam2bam] timing: search threads (%zu GPU%s) %.3f s busy\n", P.n_dev, P.n_dev > 1 ? "s" : "", ts); }
	if (timing) fprintf(stderr, "[nabwa_bam2bam] timing: library calls: create %.3f s, pass 1 %.3f s, pass 2 %.3f s, output %.3f s, destroy %.3f s\n", P.t_call[0], P.t_call[1], P.t_call[2], P.t_call[3], P.t_call[4]);
	if (timing && damage) fprintf(stderr, "[nabwa_bam2bam] timing: damage thread %.3f s busy (upload and count on the gpu)\n", P.t_damage);
	if (timing && markdup) fprintf(stderr, "[nabwa_bam2bam] timing: duplicates thread %.3f s busy (upload, signatures and the resolve on the gpu)\n", P.t_markdup);
	if (timing && bai) fprintf(stderr, "[nabwa_bam2bam] timing: index thread %.3f s busy (upload and tuples on the gpu)\n", P.t_index);
	if (timing && opt.sort) fprintf(stderr, "[nabwa_bam2bam] timing: sort thread %.3f s busy (%zu run(s) sorted on the %s, then handed on or merged)\n", P.t_sort, P.runs.size(), sorter ? "gpu" : "host");
	if (timing) fprintf(stderr, "[nabwa_bam2bam] timing: reader thread %.3f s busy (%.3f s of it inflate, %s), passes 1 and 2 on this thread %.3f s (+ %.3f s waiting for input; the output thread waited %.3f s for the writer), writer thread %.3f s busy (deflate + write; %s)\n",
						P.t_read, in.t_inflate, in.bgzf ? (bgzf_in ? "BGZF blocks on the GPU" : "BGZF blocks in parallel") : in.raw ? "not compressed" : "one gzip stream", P.t_lib, P.t_wait_in, P.t_wait_out, P.t_write,
						opt.bgzf_dynamic ? "BGZF on the GPU, dynamic Huffman codes" : opt.bgzf_gpu ? "BGZF on the GPU" : "zlib level 2 on host threads");
	fprintf(stderr, "[nabwa_bam2bam] %ld sequences processed\n[nabwa_bam2bam] finished cleanly, shutting down.\n"
			"[bwa_paired_sw] %lld out of %lld Q%d singletons are mated.\n[bwa_paired_sw] %lld out of %lld Q%d discordant pairs are fixed.\n",
			P.tot_seqs, (long long)P.n_mapped[1], (long long)P.n_tot[1], 17, (long long)P.n_mapped[0], (long long)P.n_tot[0], 17);
	out.close();
	if (bgzf) nabwa_bgzf_destroy(bgzf);
	if (bgzf_in) nabwa_bgzf_destroy(bgzf_in);
	if (sorter) nabwa_bam_sort_destroy(sorter);
	if (markdup) nabwa_markdup_destroy(markdup);
	std::string damage_line;
	if (damage) { damage_line = write_damage_profile(damage, opt.damage.n_pos, opt.damage_file); nabwa_damage_destroy(damage); }
	nabwa_isize_table_destroy(P.tab);
	tool_dedup_cache_summary(ixs);
	for (nabwa_index_t *p : ixs) nabwa_index_destroy(p);
	final_rename(opt.ofile, true);
	uint64_t bai_stats[NABWA_BAI_N_STATS] = {};
	if (bai) {                                                  /* the file is whole: its block table is, and the index goes beside the name it ends up with */
		const double t0 = now_s();
		int64_t n_bai = 0;
		if (nabwa_bai_finish(bai, (int64_t)out.blk_u.size() - 1, out.blk_u.data(), out.blk_c.data(), 0, 0, &n_bai, 0) != NABWA_OK) die("index", nabwa_last_error());
		std::vector<uint8_t> file((size_t)n_bai);
		if (nabwa_bai_finish(bai, (int64_t)out.blk_u.size() - 1, out.blk_u.data(), out.blk_c.data(), file.data(), n_bai, &n_bai, bai_stats) != NABWA_OK) die("index", nabwa_last_error());
		nabwa_bai_destroy(bai);
		std::string name(opt.ofile);
		size_t e = name.size();
		while (e > 0 && name[e - 1] == '_') --e;                /* final_rename's rule */
		if (e != 0 && name[e - 1] != '/') name.resize(e);
		name += ".bai";
		FILE *bf = fopen(name.c_str(), "wb");
		if (!bf || fwrite(file.data(), 1, file.size(), bf) != file.size() || fclose(bf) != 0) die(name.c_str(), "cannot write");
		if (timing) fprintf(stderr, "[nabwa_bam2bam] timing: index finished and written in %.3f s\n", now_s() - t0);
	}
	if (opt.sort) fprintf(stderr, "[nabwa_bam2bam] sorted %llu records in %zu run(s) on the %s\n", (unsigned long long)P.n_sorted, P.runs.size(), opt.sort_host ? "host" : "gpu");
	if (damage) fprintf(stderr, "%s", damage_line.c_str());
	if (opt.dups()) fprintf(stderr, "[nabwa_bam2bam] %s %llu of %llu records as duplicates (%llu pairs, %llu single reads) on the gpu\n", opt.remove_dups ? "removed" : "marked",
							(unsigned long long)P.dup_stats[NABWA_MARKDUP_STAT_DUP_RECORDS], (unsigned long long)P.dup_stats[NABWA_MARKDUP_STAT_SEEN],
							(unsigned long long)P.dup_stats[NABWA_MARKDUP_STAT_DUP_PAIRS], (unsigned long long)P.dup_stats[NABWA_MARKDUP_STAT_DUP_FRAGMENTS]);
	if (opt.index) fprintf(stderr, "[nabwa_bam2bam] indexed %llu records, %llu chunks in %llu bins on the gpu\n", (unsigned long long)bai_stats[NABWA_BAI_STAT_RECORDS],
							(unsigned long long)bai_stats[NABWA_BAI_STAT_CHUNKS], (unsigned long long)bai_stats[NABWA_BAI_STAT_BINS]);
	return 0;
}
