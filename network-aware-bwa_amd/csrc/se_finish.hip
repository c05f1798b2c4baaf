// se_finish.hip -- host side of the single-end finishing chain, and the reference annotations it reads.
//
// What the reference does per record between the FM search and the BAM record (bam2bam.c:622-657):
//   posn_singleton : bwa_aln2seq_core (bwase.c:19-95, consumes drand48 in record order),
//                    bwa_cal_pac_pos_core + multi-hit positions (bwase.c:139-154, bam2bam.c:633-637)
//   finish_singleton: bwa_refine_gapped (bwase.c:356-423): refine_gapped_core -> aln_global_core,
//                    bwa_cal_md1, bwa_correct_trimmed; then the flag / XT logic of bwa_update_bam1
//                    (bam2bam.c:430-593), which mirrors bwa_print_sam1 (bwase.c:458-571).
// Here the same chain runs over a whole batch: phase 1 on the host in record order (it is O(ns) per read
// and owns the RNG stream), all bwt_sa walks as ONE GPU batch, all gap refinements as ONE GPU batch of
// banded global alignments, the rest (CIGAR fix-ups, MD/NM, flags) on the host.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "../../include/nabwa.h"
#include "nabwa_internal.hpp"
#include "finish_common.hpp"
#include "finish_gpu.hpp"

/* ------------------------------------------------------------------ reference annotations */

int nabwa_reference_read(const char *prefix, nabwa_reference **out)
{
	nabwa_reference *R = new nabwa_reference();
	std::string p(prefix);
	FILE *f = fopen((p + ".ann").c_str(), "r");                       /* format: bns_dump / bns_restore_core, bntseq.c:63-117 */
	long long xx; int n_seqs = 0; unsigned seed = 0;
	if (!f || fscanf(f, "%lld%d%u", &xx, &n_seqs, &seed) != 3) { if (f) fclose(f); delete R; return nabwa_fail(NABWA_EIO, "cannot read %s.ann", prefix); }
	R->l_pac = xx; R->seed = seed;
	for (int i = 0; i < n_seqs; ++i) {
		unsigned gi; char name[1024]; int c; nabwa_ann a;
		if (fscanf(f, "%u%1023s", &gi, name) != 2) { fclose(f); delete R; return nabwa_fail(NABWA_EIO, "malformed %s.ann", prefix); }
		while ((c = fgetc(f)) != '\n' && c != EOF) {}
		if (fscanf(f, "%lld%d%d", &xx, &a.len, &a.n_ambs) != 3) { fclose(f); delete R; return nabwa_fail(NABWA_EIO, "malformed %s.ann", prefix); }
		a.offset = xx; a.name = name;
		R->anns.push_back(a);
	}
	fclose(f);
	f = fopen((p + ".amb").c_str(), "r");
	int ns = 0, nh = 0;
	if (!f || fscanf(f, "%lld%d%d", &xx, &ns, &nh) != 3) { if (f) fclose(f); delete R; return nabwa_fail(NABWA_EIO, "cannot read %s.amb", prefix); }
	for (int i = 0; i < nh; ++i) {
		char s[64]; nabwa_hole h;
		if (fscanf(f, "%lld%d%63s", &xx, &h.len, s) != 3) { fclose(f); delete R; return nabwa_fail(NABWA_EIO, "malformed %s.amb", prefix); }
		h.offset = xx; h.amb = s[0];
		R->holes.push_back(h);
	}
	fclose(f);
	f = fopen((p + ".pac").c_str(), "rb");
	if (!f) { delete R; return nabwa_fail(NABWA_EIO, "cannot read %s.pac", prefix); }
	fseek(f, 0, SEEK_END); long sz = ftell(f); fseek(f, 0, SEEK_SET);
	R->pac.resize(sz + 8);
	if (fread(R->pac.data(), 1, sz, f) != (size_t)sz || sz < R->l_pac / 4) { fclose(f); delete R; return nabwa_fail(NABWA_EIO, "short %s.pac", prefix); }
	fclose(f);
	*out = R;
	return NABWA_OK;
}

extern "C" int nabwa_index_attach_reference(nabwa_index_t *ix, const char *prefix)
{
	if (!ix || !prefix) return nabwa_fail(NABWA_EINVAL, "null argument");
	nabwa_reference *R = nullptr;
	if (const int r = nabwa_reference_read(prefix, &R)) return r;
	nabwa_finish_drop_reference(ix);      /* the device path's copies of the old one (finish_gpu.hip) */
	delete ix->ref;
	ix->ref = R;
	return NABWA_OK;
}

/* The same from memory: one or more contigs (names, offsets, lengths), ambiguity holes, the packed bases (.pac layout: 4 per
 * byte, first base in the top bits).  bench.py attaches its synthetic genome this way. */
extern "C" int nabwa_index_set_reference(nabwa_index_t *ix, int64_t l_pac, uint32_t seed, int n_seqs, const char *const *names,
										  const int64_t *offsets, const int32_t *lens, int n_holes, const int64_t *hole_off,
										  const int32_t *hole_len, const char *hole_amb, const uint8_t *pac)
{
	if (!ix || l_pac < 0 || n_seqs < 1 || !offsets || !lens || !pac || (n_holes && (!hole_off || !hole_len || !hole_amb))) return nabwa_fail(NABWA_EINVAL, "bad argument");
	nabwa_reference *R = new nabwa_reference();
	R->l_pac = l_pac; R->seed = seed;
	for (int i = 0; i < n_seqs; ++i) { nabwa_ann a; a.offset = offsets[i]; a.len = lens[i]; a.n_ambs = 0; a.name = names && names[i] ? names[i] : "seq"; R->anns.push_back(a); }
	for (int i = 0; i < n_holes; ++i) { nabwa_hole h; h.offset = hole_off[i]; h.len = hole_len[i]; h.amb = hole_amb[i]; R->holes.push_back(h); }
	R->pac.assign(pac, pac + (l_pac + 3) / 4);
	R->pac.resize(R->pac.size() + 8);
	nabwa_finish_drop_reference(ix);      /* the device path's copies of the old one (finish_gpu.hip) */
	delete ix->ref;
	ix->ref = R;
	return NABWA_OK;
}

extern "C" int nabwa_index_n_contigs(const nabwa_index_t *ix) { return ix && ix->ref ? (int)ix->ref->anns.size() : 0; }
extern "C" int nabwa_index_contig(const nabwa_index_t *ix, int i, char *name, int name_cap, int64_t *offset, int32_t *len)
{
	if (!ix || !ix->ref || i < 0 || i >= (int)ix->ref->anns.size()) return nabwa_fail(NABWA_EINVAL, "no such contig");
	const nabwa_ann &a = ix->ref->anns[i];
	if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s", a.name.c_str());
	if (offset) *offset = a.offset;
	if (len) *len = a.len;
	return NABWA_OK;
}
extern "C" int nabwa_index_reference_info(const nabwa_index_t *ix, int64_t *l_pac, uint32_t *seed)
{
	if (!ix || !ix->ref) return nabwa_fail(NABWA_EINVAL, "index has no reference attached");
	if (l_pac) *l_pac = ix->ref->l_pac;
	if (seed) *seed = ix->ref->seed;
	return NABWA_OK;
}

/* ------------------------------------------------------------------ the chain */

/* posn_singleton (bam2bam.c:622-641) for n reads in record order: bwa_aln2seq_core with the caller's drand48 stream, all
 * bwt_sa walks of the batch (main hits and multi hits) as one GPU batch, bwa_approx_mapQ */
static int se_posn_impl(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const int32_t *full_len,
						const int32_t *n_aln, const nabwa_aln1_t *aln, int n_occ, const uint8_t *n_occ_v, uint64_t *rng48, void *out_base, size_t stride);

extern "C" int nabwa_se_posn(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const int32_t *full_len,
							 const int32_t *n_aln, const nabwa_aln1_t *aln, int n_occ, uint64_t *rng48, nabwa_se_t *out)
{
	return se_posn_impl(ix, opt, n, off, full_len, n_aln, aln, n_occ, 0, rng48, out, sizeof(nabwa_se_t));
}

/* the same with a bound per read: a file that mixes singletons (max_occ_se other hits listed, bam2bam.c:629) and ends of pairs
 * (none, bam2bam.c:692-694) is still ONE drand48 stream in record order */
extern "C" int nabwa_se_posn_v(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const int32_t *full_len,
							   const int32_t *n_aln, const nabwa_aln1_t *aln, const uint8_t *n_occ_v, uint64_t *rng48, nabwa_se_t *out)
{
	if (n && !n_occ_v) return nabwa_fail(NABWA_EINVAL, "null argument");
	return se_posn_impl(ix, opt, n, off, full_len, n_aln, aln, 0, n_occ_v, rng48, out, sizeof(nabwa_se_t));
}

/* records of any stride whose head is a nabwa_se_t (nabwa_pe_t starts with one): the batch front-end works in place */
int nabwa_se_posn_strided(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const int32_t *full_len,
						  const int32_t *n_aln, const nabwa_aln1_t *aln, const uint8_t *n_occ_v, uint64_t *rng48, void *out_base, size_t stride)
{
	return se_posn_impl(ix, opt, n, off, full_len, n_aln, aln, 0, n_occ_v, rng48, out_base, stride);
}

static int se_posn_impl(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const int32_t *full_len,
						const int32_t *n_aln, const nabwa_aln1_t *aln, int n_occ, const uint8_t *n_occ_v, uint64_t *rng48, void *out_base, size_t stride)
{
	if (!ix || !opt || !rng48 || n < 0 || (n && (!off || !n_aln || !out_base))) return nabwa_fail(NABWA_EINVAL, "null argument");
#define out_at(i_) (*rec_at(out_base, stride, (int)(i_)))
	if (n_occ < 0 || n_occ + 1 > NABWA_MAX_MULTI) return nabwa_fail(NABWA_EINVAL, "n_occ outside 0..15");
	if (n_occ_v) for (int i = 0; i < n; ++i) if (n_occ_v[i] + 1 > NABWA_MAX_MULTI) return nabwa_fail(NABWA_EINVAL, "n_occ outside 0..15");
	const uint32_t rlen = ix->bwt[1].seq_len;
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double t0 = now_s();
	/* ---- host: hit choice with the caller's RNG stream (bwase.c:19-95).  The stream is consumed in record order and how many
	 * numbers a read takes depends on the numbers themselves (a second draw follows every accepted row), so ONE light serial pass
	 * runs the generator alone over the batch -- two multiplications per draw, no record touched -- and notes its state at the slice
	 * boundaries; the slices then do the whole choice in threads, each from its own state, and draw exactly what that pass drew. */
	const int nt0 = host_threads((size_t)n, 4096);
	std::vector<uint64_t> slice_state((size_t)nt0 + 1, 0); std::vector<size_t> slice_a0((size_t)nt0 + 1, 0);
	{
		uint64_t st = *rng48; size_t a0 = 0; int next = 0;
		for (int i = 0; i <= n; ++i) {
			while (next <= nt0 && (size_t)i == (size_t)n * next / nt0) { slice_state[next] = st; slice_a0[next] = a0; ++next; }
			if (i == n) break;
			const int na = n_aln[i]; const nabwa_aln1_t *A = aln + a0;
			a0 += na;
			if (na == 0) continue;
			int cnt = 0; const int best = A[0].score;
			for (int j = 0; j < na; ++j) {                       /* choose_main's draws, nothing else */
				if (A[j].score > best) break;
				const uint32_t w = A[j].l - A[j].k + 1;
				if (rng48_next(&st) * (double)(w + cnt) > (double)cnt) (void)rng48_next(&st);
				cnt += w;
			}
		}
		*rng48 = st;
	}
	struct Part { std::vector<uint8_t> which; std::vector<uint32_t> rows; std::vector<int> look_rec, look_multi; };
	std::vector<Part> parts((size_t)nt0);
	{
		host_parallel(nt0, (size_t)n, [&](int t, size_t lo, size_t hi) {
			Part &Q = parts[(size_t)t];
			Q.which.reserve((hi - lo) + (hi - lo) / 4); Q.rows.reserve((hi - lo) + (hi - lo) / 4); Q.look_rec.reserve((hi - lo) + (hi - lo) / 4); Q.look_multi.reserve((hi - lo) + (hi - lo) / 4);
			uint64_t st = slice_state[(size_t)t]; size_t a0 = slice_a0[(size_t)t];
			for (size_t i = lo; i < hi; ++i) {
				if (i + 8 < hi) { nabwa_se_t *const f = &out_at(i + 8); __builtin_prefetch(f, 1); __builtin_prefetch(&f->nm, 1); __builtin_prefetch(&f->n_multi, 1); __builtin_prefetch(&f->flag, 1); }      /* (the fields written below, in a 3 KB record) */
				nabwa_se_t &s = out_at(i);
				memset(&s, 0, offsetof(nabwa_se_t, cigar));          /* the scalar head; arrays are only valid up to their counts */
				s.n_cigar = 0; s.nm = 0; s.md[0] = 0; s.n_multi = 0; s.flag = 0; s.seqid = 0; s.nn = 0; s.rpos = 0; s.xt = 0;
				const int len = (int)(off[i + 1] - off[i]);
				s.len = len; s.clip_len = len; s.full_len = full_len ? full_len[i] : len;
				const nabwa_aln1_t *A = aln + a0; const int na = n_aln[i];
				a0 += na;
				if (na == 0) continue;
				choose_main(s, na, A, &st);
				list_multi(s, na, A, n_occ_v ? (int)n_occ_v[i] : n_occ);
				Q.which.push_back(s.strand ? 0 : 1); Q.rows.push_back(s.sa); Q.look_rec.push_back((int)i); Q.look_multi.push_back(-1);
				for (int j = 0; j < s.n_multi; ++j) {
					Q.which.push_back(s.multi[j].strand ? 0 : 1); Q.rows.push_back(s.multi[j].pos); Q.look_rec.push_back((int)i); Q.look_multi.push_back(j);
				}
			}
		});
	}
	std::vector<uint8_t> which; std::vector<uint32_t> rows;           /* SA lookups: [main of each mapped read][multi...] */
	std::vector<int> look_rec, look_multi;
	{
		size_t tot = 0; for (Part &Q : parts) tot += Q.rows.size();
		which.reserve(tot); rows.reserve(tot); look_rec.reserve(tot); look_multi.reserve(tot);
		for (Part &Q : parts) {
			which.insert(which.end(), Q.which.begin(), Q.which.end()); rows.insert(rows.end(), Q.rows.begin(), Q.rows.end());
			look_rec.insert(look_rec.end(), Q.look_rec.begin(), Q.look_rec.end()); look_multi.insert(look_multi.end(), Q.look_multi.begin(), Q.look_multi.end());
		}
	}
	const double t1 = now_s();
	/* ---- GPU: all bwt_sa walks of the batch (bwt.c:72-81) */
	std::vector<uint32_t> sa(rows.size());
	if (!rows.empty()) {
		int r = nabwa_sa_lookup(ix, (int)rows.size(), which.data(), rows.data(), sa.data());
		if (r != NABWA_OK) return r;
	}
	const int nt = host_threads((size_t)n, 4096);
	/* positions (bwase.c:146-151, bam2bam.c:635-636): every looked-up row belongs to one record field, so slices are independent */
	host_parallel(nt, rows.size(), [&](int, size_t lo, size_t hi) {
		for (size_t t = lo; t < hi; ++t) {
			nabwa_se_t &s = out_at(look_rec[t]);
			const uint32_t p = which[t] == 0 ? sa[t] : rlen - (sa[t] + (uint32_t)s.len);
			if (look_multi[t] < 0) s.pos = p; else s.multi[look_multi[t]].pos = p;
		}
	});
	/* bwa_approx_mapQ (bwase.c:113-122); max_diff of a read follows from its length: one table instead of a Poisson sum per read */
	int longest = 0;
	for (int i = 0; i < n; ++i) if ((int)(off[i + 1] - off[i]) > longest) longest = (int)(off[i + 1] - off[i]);      /* (= the records' len, without touching a million records on one thread) */
	std::vector<int> md_of(longest + 1, opt->max_diff);
	if (opt->fnr > 0.0f) for (int L = 0; L <= longest; ++L) md_of[L] = nabwa_cal_maxdiff(L, 0.02, opt->fnr);
	host_parallel(nt, (size_t)n, [&](int, size_t lo, size_t hi) {
		for (size_t i = lo; i < hi; ++i) {
			if (i + 8 < hi) __builtin_prefetch(&out_at(i + 8), 1);
			nabwa_se_t &s = out_at(i);
			if (s.type == 0) continue;
			const int q = approx_mapq(s, md_of[s.len]);
			s.mapQ = s.seQ = q;
		}
	});
	if (timing) fprintf(stderr, "[nabwa] se_posn %d reads: hit choice %.3f s, bwt_sa batch (%zu rows) + positions + mapQ %.3f s\n", n, t1 - t0, rows.size(), now_s() - t1);
	return NABWA_OK;
}
#undef out_at

/* The non-BAM part of finish_singleton (bam2bam.c:643-651) for n positioned records: bwa_refine_gapped (bwase.c:356-423 --
 * refine_gapped_core of every gapped hit as ONE GPU batch of banded global alignments, bwa_cal_md1, bwa_correct_trimmed), then
 * the flag / contig / XT logic bwa_update_bam1 applies to a single-end record (bam2bam.c:430-525). */
extern "C" int nabwa_se_refine(nabwa_index_t *ix, int n, const int64_t *off, const uint8_t *seq, const uint8_t *rseq, nabwa_se_t *out)
{
	return nabwa_se_refine_strided(ix, n, off, seq, rseq, out, sizeof(nabwa_se_t));
}

int nabwa_se_refine_strided(nabwa_index_t *ix, int n, const int64_t *off, const uint8_t *seq, const uint8_t *rseq, void *out_base, size_t stride)
{
	if (!ix || n < 0 || (n && (!off || !seq || !rseq || !out_base))) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (!ix->ref) return nabwa_fail(NABWA_EINVAL, "index has no reference attached (nabwa_index_attach_reference)");
	const nabwa_reference *R = ix->ref;
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double t2 = now_s();
	size_t n_jobs = 0;
	/* NABWA_FINISH=gpu: windows, CIGAR rules and MD / NM on the device (finish_gpu.hip), the reads uploaded once for both */
	const int fin_mode = nabwa_finish_mode();
	if (fin_mode < 0) return nabwa_fail(NABWA_EINVAL, "NABWA_FINISH: host or gpu");
	std::unique_ptr<FinGpu> gpu;
	if (fin_mode == 1) {
		nabwa_finish_count_chain_call();
		gpu.reset(new FinGpu(ix));
		if (n) if (const int r = gpu->set_reads(off[n], seq, rseq)) return r;
	}
	{
		int r = refine_batch(ix, out_base, stride, n, off, seq, rseq, &n_jobs, nullptr, gpu.get());
		if (r != NABWA_OK) return r;
	}
	const double t3 = now_s();
	if (gpu && n) if (const int r = gpu->md_records(0, out_base, stride, n, off)) return r;
	/* host threads: MD / NM, trimmed tail, flags (bwase.c:253-354, :458-571); records are independent */
	int md_over = 0;
	auto phase4 = [&](int lo, int hi) {
		std::vector<uint8_t> fwd;
		for (int i = lo; i < hi; ++i) {
			/* what a record needs lies far apart -- its head and its MD field in a 3 KB record, its window in 775 MB of packed reference --, and
			 * every piece was a cache miss in turn: the record 16 ahead and the window of the record 8 ahead are asked for now */
			if (i + 16 < hi) { const nabwa_se_t *const f = rec_at(out_base, stride, i + 16); __builtin_prefetch(f); __builtin_prefetch(f->md, 1); __builtin_prefetch(&f->flag, 1); }
			if (!gpu && i + 8 < hi) { const nabwa_se_t *const f = rec_at(out_base, stride, i + 8); if (f->type) { const uint8_t *const w = R->pac.data() + (f->pos >> 2); __builtin_prefetch(w); __builtin_prefetch(w + 32); } }
			nabwa_se_t &s = *rec_at(out_base, stride, i);
			if (s.type == 0) { s.flag = 4; continue; }
			if (gpu) { if (!gpu->take_md(i, s)) md_over = 1; correct_trimmed(s); }      /* MD / NM came from the device */
			else if (!md_and_trim(R, s, seq + off[i], rseq + off[i], fwd)) md_over = 1;
			se_flags(R, s);
		}
	};
	host_parallel(host_threads((size_t)n, 4096), (size_t)n, [&](int, size_t lo, size_t hi) { phase4((int)lo, (int)hi); });
	if (md_over) return nabwa_fail(NABWA_ECAP, "MD string longer than NABWA_MAX_MD");
	if (timing) fprintf(stderr, "[nabwa] se_refine %d reads: refinement (%zu jobs) %.3f s, md/flags %.3f s\n", n, n_jobs, t3 - t2, now_s() - t3);
	if (gpu) gpu->report("se_refine");
	return NABWA_OK;
}

extern "C" int nabwa_se_finish(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const uint8_t *seq,
							   const uint8_t *rseq, const int32_t *full_len, const int32_t *n_aln, const nabwa_aln1_t *aln,
							   int n_occ, uint64_t *rng48, nabwa_se_t *out)
{
	if (!ix || !opt || !rng48 || n < 0 || (n && (!off || !seq || !rseq || !n_aln || !out))) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (!ix->ref) return nabwa_fail(NABWA_EINVAL, "index has no reference attached (nabwa_index_attach_reference)");
	int r = nabwa_se_posn(ix, opt, n, off, full_len, n_aln, aln, n_occ, rng48, out);
	if (r == NABWA_OK) r = nabwa_se_refine(ix, n, off, seq, rseq, out);
	return r;
}
