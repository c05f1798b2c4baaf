// bam_batch.hip -- the passes of the batching front-end behind `bwa bam2bam` / `bwa worker`: BAM records in, BAM records out.
//
// The reference handles one logical record (a singleton or a pair) at a time: read_bam_pair -> pair_aln -> pair_posn ->
// improve_isize_est -> [all records] -> infer_all_isizes -> pair_finish -> bwa_update_bam1 (bam2bam.c:1143-1216, 608-811,
// 430-593; bwaseqio.c:340-494; insert_size.c:141-213).  Here the same steps run over a BATCH of records:
//   create : split the records into singletons and pairs (read_bam_pair_core's rules), OR the QC flag over mates, erase the
//            tags the aligner regenerates (erase_unwanted_tags), encode the reads (bam1_to_seq incl. reverse flag and trimming):
//            the stages of bam_front.cpp over the records of bam_rec.hpp, host code that needs no index
//   pass 1 : bwa_cal_sa_reg_gap of every read [GPU, kernels W / S / D], the hit choice IN RECORD ORDER on the caller's drand48
//            stream (posn_singleton: bwa_aln2seq_core(.., 1, max_occ_se); posn_pair: bwa_aln2seq), all bwt_sa walks as one
//            GPU batch, mapQ, and the per-@RG insert-size histograms (improve_isize_est; the table is isize_table.cpp)
//   pass 2 : finish_singleton / finish_pair per read group with that group's estimate (pairing, mate rescue and gap
//            refinement as GPU batches inside nabwa_pe_finish / nabwa_se_refine), then bwa_update_bam1: flags, coordinates,
//            bin, CIGAR, reverse-complemented SEQ/QUAL, mate fields, tags in the reference's order and types
// All host code; the GPU work is what the entry points it calls do.  bam2bam.c itself cannot be compiled in the build
// container (<zmq.h>), so what pass 2 writes is checked through every field the reference's samse / sampe SAM exposes
// (tests/test_gpu_bam.py), not against a bam2bam run; the create stage is held against bwaseqio.c / bamlite.c themselves
// (tests/test_bam_front.py): DESIGN.md says so.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../include/nabwa.h"
#include "nabwa_internal.hpp"
#include "finish_common.hpp"
#include "isize_table.hpp"
#include "bam_batch.hpp"
#include "bam_front.hpp"

/* bwa_update_bam1 (bam2bam.c:430-593).  p: this end's finished record; mate: the other end's (null for a singleton); pe: this
 * end's pair fields.  p / mate are in the state nabwa_se_refine / nabwa_pe_finish leave them in, i.e. with the side effects the
 * reference's calls have on them (an unmapped end takes its mate's place, a contig-bridging hit loses its mapQ) already applied. */
static void update_bam(BamRec &out, const nabwa_reference *R, const nabwa_se_t &p, const nabwa_se_t *mate, const nabwa_pe_t *pe,
					   int mode, int max_top2, int yq)
{
	if (p.clip_len < p.full_len) push_int(out, 'X', 'C', p.clip_len);
	if (yq) push_int(out, 'Y', 'Q', yq);                  /* --debug-bam: the most entries the search held (bam2bam.c:433) */
	if (p.type != 0 || (mate && mate->type != 0)) {
		if ((p.strand != 0) != ((out.flag & F_SR) != 0)) revcom_rec(out);
		out.flag &= ~(uint32_t)(F_PP | F_SU | F_MU | F_SC | F_MR);
		const int fl = p.flag;                 /* what the chain derived: proper pair, self / mate unmapped, mate strand */
		out.flag |= (uint32_t)(fl & (F_PP | F_SU | F_MU | F_MR));
		const int seqid = p.seqid;
		const int64_t off = R->anns[seqid].offset;
		out.tid = seqid; out.pos = (int32_t)((int64_t)p.pos - off);
		out.bin = reg2bin((uint32_t)((int64_t)p.pos - off), (uint32_t)(rec_pos_end(p) - off));
		out.mapq = (uint32_t)p.mapQ & 0xff;
		if (p.n_cigar) {
			uint32_t c[NABWA_MAX_CIGAR];
			for (int j = 0; j < p.n_cigar; ++j) c[j] = (uint32_t)CLEN(p.cigar[j]) << 4 | (uint32_t)"\000\001\002\004"[COP(p.cigar[j])];
			set_cigar(out, p.n_cigar, c);
		} else if (p.type == 0) set_cigar(out, 0, 0);
		else { const uint32_t c = (uint32_t)p.len << 4; set_cigar(out, 1, &c); }
		if (mate && mate->type != 0) { out.mtid = pe->m_seqid; out.mpos = (int32_t)(pe->m_rpos - 1); out.isize = (int32_t)pe->isize; }
		else if (mate) { out.mtid = seqid; out.mpos = (int32_t)((int64_t)p.pos - off); out.isize = 0; }
		else { out.mtid = -1; out.mpos = -1; out.isize = 0; }
		if (p.type != 0) {
			push_char(out, 'X', 'T', p.xt);
			push_int(out, (mode & NABWA_MODE_COMPREAD) ? 'N' : 'C', 'M', p.nm);
			if (p.nn) push_int(out, 'X', 'N', p.nn);
			if (mate) { push_int(out, 'S', 'M', p.seQ); push_int(out, 'A', 'M', pe->am); }
			if (p.type != 3) {                                     /* X0 / X1 do not exist for a mate-rescued alignment */
				push_int(out, 'X', '0', (int)p.c1);
				if ((int64_t)p.c1 <= (int64_t)max_top2) push_int(out, 'X', '1', (int)p.c2);
			}
			push_int(out, 'X', 'M', p.n_mm); push_int(out, 'X', 'O', p.n_gapo); push_int(out, 'X', 'G', p.n_gapo + p.n_gape);
			push_str(out, 'M', 'D', p.md);
			if (p.n_multi) {
				std::string xa; char buf[128];
				for (int i = 0; i < p.n_multi; ++i) {
					const nabwa_multi_t &q = p.multi[i];
					int64_t e = q.pos;
					if (q.n_cigar) { for (int k = 0; k < q.n_cigar; ++k) { const int op = COP(q.cigar[k]); if (op == 0 || op == 2) e += CLEN(q.cigar[k]); } } else e += p.len;
					int sid; pac2real(R, q.pos, (int)(e - q.pos), &sid);
					snprintf(buf, sizeof buf, "%s,%c%d,", R->anns[sid].name.c_str(), q.strand ? '-' : '+', (int)((int64_t)q.pos - R->anns[sid].offset + 1)); xa += buf;
					if (q.n_cigar) for (int k = 0; k < q.n_cigar; ++k) { snprintf(buf, sizeof buf, "%d%c", CLEN(q.cigar[k]), "MIDS"[COP(q.cigar[k])]); xa += buf; }
					else { snprintf(buf, sizeof buf, "%dM", p.len); xa += buf; }
					snprintf(buf, sizeof buf, ",%d;", q.gap + q.mm); xa += buf;
				}
				push_str(out, 'X', 'A', xa.c_str());
			}
		}
	} else {                       /* neither this read nor its mate has a match */
		out.tid = -1; out.pos = -1; out.bin = 0; out.mapq = 0; out.mtid = -1; out.mpos = -1; out.isize = 0;
		out.flag &= ~(uint32_t)(F_PP | F_MU | F_SC);
		out.flag |= F_SU;
		if (mate && mate->type == 0) out.flag |= F_MU;
		set_cigar(out, 0, 0);
	}
}

/* ------------------------------------------------------------------ the batch */

extern "C" int nabwa_bam_batch_create(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, int n_rec,
									  const uint8_t *in, const int64_t *in_off, nabwa_bam_batch_t **out)
{
	return nabwa_bam_batch_create_ex(ix, opt, popt, 0, n_rec, in, in_off, out);
}

extern "C" int nabwa_bam_batch_create_ex(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, uint32_t flags, int n_rec,
										 const uint8_t *in, const int64_t *in_off, nabwa_bam_batch_t **out)
{
	if (!ix || !opt || !popt || !out || n_rec < 0 || (n_rec && (!in || !in_off))) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (flags & ~(uint32_t)NABWA_BAM_ALL_FLAGS) return nabwa_fail(NABWA_EINVAL, "unknown NABWA_BAM_* flag");
	if (!ix->ref) return nabwa_fail(NABWA_EINVAL, "index has no reference attached (nabwa_index_attach_reference)");
	/* limits of the record format, refused here and not after the search: the other hits of a singleton (bam2bam.c:629) fill a fixed list */
	if (popt->max_occ_se < 0 || popt->max_occ_se + 1 > NABWA_MAX_MULTI) return nabwa_fail(NABWA_EINVAL, "max_occ_se (-D) outside 0..15");
	if (popt->n_multi < 0 || popt->N_multi < 0 || popt->n_multi > NABWA_MAX_MULTI || popt->N_multi > NABWA_MAX_MULTI) return nabwa_fail(NABWA_EINVAL, "n_multi / N_multi outside 0..16");
	if (opt->s_mm < 1 || opt->s_gapo < 1 || opt->s_gape < 1) return nabwa_fail(NABWA_EINVAL, "s_mm, s_gapo and s_gape must be >= 1 (-M / -O / -E 0 are not supported)");
	std::unique_ptr<nabwa_bam_batch> b(new nabwa_bam_batch());
	b->ix = ix; b->opt = *opt; b->popt = *popt; b->phase = 0; b->flags = flags;
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double tc0 = now_s();
	uint32_t any_flag = 0;
	int rc = bam_front_parse(b.get(), n_rec, in, in_off, &any_flag);
	if (rc != NABWA_OK) return rc;
	const double tc1 = now_s();
	rc = bam_front_pair(b.get(), any_flag);
	if (rc != NABWA_OK) return rc;
	const double tc1a = now_s();          /* (the tags are erased while the records are parsed: the line keeps its column) */
	bam_front_read_groups(b.get());
	const double tc2 = now_s();
	rc = bam_front_encode(b.get());
	if (rc != NABWA_OK) return rc;
	n_rec = (int)b->rec.size();
	if (timing) fprintf(stderr, "[nabwa] bam_batch_create %d records: parse %.3f s, pairing %.3f s, tag erase %.3f s, read groups %.3f s, bam1_to_seq %.3f s (%d threads)\n",
						n_rec, tc1 - tc0, tc1a - tc1, 0.0, tc2 - tc1a, now_s() - tc2, host_threads((size_t)n_rec, BAM_MIN_N));
	*out = b.release();
	return NABWA_OK;
}

extern "C" void nabwa_bam_batch_destroy(nabwa_bam_batch_t *b) { delete b; }

/* what the passes write again and again into a working record */
static inline void pe_tail_reset(nabwa_pe_t &r) { r.extra_flag = 0; r.m_seqid = 0; r.am = 0; r.mapQ_paired = 0; r.m_rpos = 0; r.isize = 0; }
static inline void se_posn_reset(nabwa_se_t &s) { s.nm = 0; s.md[0] = 0; s.flag = 0; s.seqid = 0; s.nn = 0; s.rpos = 0; s.xt = 0; }          /* as nabwa_se_posn leaves them */
/* bwt_multi1_t (bwtaln.h:58-62) on the wire: pos, then n_cigar:15 | gap:8 | mm:8 | strand:1, then a pointer that means nothing outside its process */
static inline void multi_to_wire(const nabwa_multi_t &m, uint8_t *o)
{
	const uint32_t pos = m.pos, bits = ((uint32_t)m.gap & 0xff) << 15 | ((uint32_t)m.mm & 0xff) << 23 | ((uint32_t)m.strand & 1) << 31;
	memcpy(o, &pos, 4); memcpy(o + 4, &bits, 4);
}
static inline void multi_from_wire(const uint8_t *o, nabwa_multi_t &m)
{
	uint32_t pos, bits; memcpy(&pos, o, 4); memcpy(&bits, o + 4, 4);
	m.pos = pos; m.gap = bits >> 15 & 0xff; m.mm = bits >> 23 & 0xff; m.strand = bits >> 31; m.n_cigar = 0;
}
/* the block of working records, one per read, from the pool (what a batch held before goes back first) */
static bool take_res(nabwa_bam_batch *b) { const size_t n = b->rec.size(); return b->res.take(sizeof(nabwa_pe_t) * (n ? n : 1)); }

/* A batch with pairs waits between the passes for the insert-size estimates of the whole input, and of its 3 KB per read pass 1
 * has filled some 70 bytes (the scalar head and, for singletons, the heads of the other hits).  These are packed and the block
 * goes back to the pool until pass 2 asks for it again: a file of 20 M paired reads waits in 1.4 GB instead of 64 GB. */
#define PARK_HEAD offsetof(nabwa_se_t, cigar)
#define PARK_MULTI offsetof(nabwa_multi_t, cigar)
static void park(nabwa_bam_batch *b)
{
	const size_t n = b->rec.size();
	b->parked_at.assign(n + 1, 0);
	for (size_t i = 0; i < n; ++i) b->parked_at[i + 1] = b->parked_at[i] + PARK_HEAD + 4 + PARK_MULTI * (size_t)b->res[i].se.n_multi;
	b->parked.resize(b->parked_at[n] ? b->parked_at[n] : 1);
	host_parallel(host_threads(n, BAM_MIN_N), n, [&](int, size_t lo, size_t hi) {
		for (size_t i = lo; i < hi; ++i) {
			const nabwa_se_t &s = b->res[i].se;
			uint8_t *o = b->parked.data() + b->parked_at[i];
			memcpy(o, &s, PARK_HEAD); memcpy(o + PARK_HEAD, &s.n_multi, 4);
			for (int j = 0; j < s.n_multi; ++j) memcpy(o + PARK_HEAD + 4 + PARK_MULTI * (size_t)j, &s.multi[j], PARK_MULTI);
		}
	});
	b->res.give();
}
static bool unpark(nabwa_bam_batch *b)
{
	const size_t n = b->rec.size();
	if (!take_res(b)) return false;
	host_parallel(host_threads(n, BAM_MIN_N), n, [&](int, size_t lo, size_t hi) {
		for (size_t i = lo; i < hi; ++i) {
			nabwa_pe_t &r = b->res[i]; nabwa_se_t &s = r.se;
			const uint8_t *o = b->parked.data() + b->parked_at[i];
			memcpy(&s, o, PARK_HEAD); memcpy(&s.n_multi, o + PARK_HEAD, 4);
			for (int j = 0; j < s.n_multi; ++j) memcpy(&s.multi[j], o + PARK_HEAD + 4 + PARK_MULTI * (size_t)j, PARK_MULTI);
			se_posn_reset(s); pe_tail_reset(r);
		}
	});
	std::vector<uint8_t>().swap(b->parked); std::vector<uint64_t>().swap(b->parked_at);
	return true;
}

/* the FM search of the batch's reads: the part of pass 1 that needs neither the random stream nor the other batches, so a caller
 * may run it ahead, from another thread and on the batch's own GPU, while pass 1 and pass 2 of earlier batches go on
 * (bwa_cal_sa_reg_gap is called with one read at a time in the reference, bam2bam.c:616,676 -> per_read = 1) */
extern "C" int nabwa_bam_batch_search(nabwa_bam_batch_t *b)
{
	if (!b) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (b->phase != 0 || b->searched) return nabwa_fail(NABWA_EINVAL, "the batch has been searched already");
	const int n = (int)b->rec.size();
	b->n_aln.assign(n ? n : 1, 0); b->max_ent.assign(n ? n : 1, 0); b->row0.assign(n + 1, 0);
	int64_t n_rows = 0;
	nabwa_batch_t *sb = 0;
	int rc = nabwa_batch_create(b->ix, &b->opt, n, b->off.data(), b->seq.data(), b->rseq.data(), 1, &sb);
	if (rc != NABWA_OK) return rc;
	rc = nabwa_batch_run(sb);
	if (rc == NABWA_OK) rc = nabwa_batch_sync(sb, 0);
	if (rc == NABWA_OK) {
		/* one fetch where the rows fit a guess (most reads bring one row), a second one where they do not */
		if (!b->rows.resize((size_t)n + (size_t)n / 4 + 1024)) { nabwa_batch_destroy(sb); return nabwa_fail(NABWA_ENOMEM, "out of memory for the hit rows"); }
		rc = nabwa_batch_fetch(sb, b->n_aln.data(), b->rows.data(), (int64_t)b->rows.size(), &n_rows, b->max_ent.data());
		if (rc == NABWA_ECAP && n_rows > (int64_t)b->rows.size()) {
			if (!b->rows.resize((size_t)n_rows)) { nabwa_batch_destroy(sb); return nabwa_fail(NABWA_ENOMEM, "out of memory for the hit rows"); }
			rc = nabwa_batch_fetch(sb, b->n_aln.data(), b->rows.data(), n_rows, &n_rows, b->max_ent.data());
		}
		if (rc == NABWA_OK) (void)b->rows.resize(n_rows ? (size_t)n_rows : 1);
	}
	nabwa_batch_destroy(sb);
	if (rc == NABWA_OK) b->searched = true;
	return rc;
}

/* pass 1: pair_aln + pair_posn + improve_isize_est of every logical record (bam2bam.c:1143-1176) */
extern "C" int nabwa_bam_batch_pass1(nabwa_bam_batch_t *b, uint64_t *rng48, nabwa_isize_table_t *tab)
{
	if (!b || !rng48 || !tab) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (b->phase != 0) return nabwa_fail(NABWA_EINVAL, "pass 1 already ran on this batch");
	const int n = (int)b->rec.size();
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double tp0 = now_s();
	int rc = b->searched ? NABWA_OK : nabwa_bam_batch_search(b);
	if (rc != NABWA_OK) return rc;
	for (int i = 0; i < n; ++i) b->row0[i + 1] = b->row0[i] + b->n_aln[i];
	for (size_t k = 0; k < b->kind.size(); ++k) if (b->skip[k]) for (int e = 0; e < b->kind[k]; ++e)
		if (b->n_aln[b->first[k] + e]) return nabwa_fail(NABWA_EINVAL, "internal: a read without bases came back with hits");
	/* posn_singleton / posn_pair in record order: singletons list up to max_occ_se other hits, ends of pairs none */
	std::vector<uint8_t> n_occ(n ? n : 1, 0);
	for (size_t k = 0; k < b->kind.size(); ++k) if (b->kind[k] == 1) n_occ[b->first[k]] = (uint8_t)b->popt.max_occ_se;
	if (!take_res(b)) return nabwa_fail(NABWA_ENOMEM, "out of memory for the batch's records");
	const double tp1 = now_s();
	rc = nabwa_se_posn_strided(b->ix, &b->opt, n, b->off.data(), b->full_len.data(), b->n_aln.data(), b->rows.data(), n_occ.data(), rng48, b->res.get(), sizeof(nabwa_pe_t));
	if (rc != NABWA_OK) return rc;
	host_parallel(host_threads((size_t)n, BAM_MIN_N), (size_t)n, [&](int, size_t lo, size_t hi) {
		for (size_t i = lo; i < hi; ++i) pe_tail_reset(b->res[i]);
	});
	/* improve_isize_est (insert_size.c:141-165): the bins by many threads, the counts in record order */
	{
		const size_t nk = b->kind.size();
		std::vector<int> bin(nk ? nk : 1, -1);
		host_parallel(host_threads(nk, BAM_MIN_N), nk, [&](int, size_t lo, size_t hi) {
			for (size_t k = lo; k < hi; ++k) {
				if (b->skip[k]) continue;
				const int i = b->first[k];
				const nabwa_se_t &s0 = b->res[i].se;
				const nabwa_se_t &s1 = b->kind[k] == 2 ? b->res[i + 1].se : s0;
				bin[k] = nabwa_isize_bin(b->kind[k], s0.mapQ, s1.mapQ, s0.pos, s0.len, s1.pos, s1.len);
			}
		});
		std::vector<nabwa_isize_table::Rg*> slot(b->rg_names.size(), (nabwa_isize_table::Rg*)0);
		for (size_t k = 0; k < nk; ++k) {
			if (bin[k] < 0) continue;
			nabwa_isize_table::Rg *&r = slot[b->rg[k]];
			if (!r) r = isize_slot(tab, b->rg_names[b->rg[k]]);
			if (r->has_hist) r->hist[bin[k]] = (uint16_t)(r->hist[bin[k]] + 1);
		}
	}
	if (b->kind.size() != b->rec.size()) park(b);
	b->phase = 1;
	if (timing) fprintf(stderr, "[nabwa] bam_batch_pass1 %d records: search (upload, kernels, rows back) %.3f s, posn + insert-size bins %.3f s\n", n, tp1 - tp0, now_s() - tp1);
	return NABWA_OK;
}

/* ---- the state pass 1 leaves, out of the batch and back into a fresh one (the wire record's positioned / aligned parts) */
extern "C" int nabwa_bam_batch_positioned(nabwa_bam_batch_t *b, nabwa_wire_read_t *out)
{
	if (!b || !out) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (b->phase != 1) return nabwa_fail(NABWA_EINVAL, "the batch is not between the passes");
	if (!b->res && !unpark(b)) return nabwa_fail(NABWA_ENOMEM, "out of memory for the batch's records");
	const size_t n = b->rec.size();
	std::vector<size_t> m0(n + 1, 0);
	for (size_t i = 0; i < n; ++i) m0[i + 1] = m0[i] + (size_t)b->res[i].se.n_multi;
	b->wire_multi.assign(16 * (m0[n] ? m0[n] : 1), 0);
	for (size_t i = 0; i < n; ++i) {
		const nabwa_se_t &s = b->res[i].se; nabwa_wire_read_t &w = out[i];
		w.strand = (uint8_t)s.strand; w.type = (uint8_t)s.type; w.n_mm = (uint8_t)s.n_mm; w.n_gapo = (uint8_t)s.n_gapo; w.n_gape = (uint8_t)s.n_gape;
		w.seQ = (uint8_t)s.seQ; w.mapQ = (uint8_t)s.mapQ; w.len = s.len; w.clip_len = s.clip_len; w.score = s.score; w.sa = s.sa; w.c1 = s.c1; w.c2 = s.c2; w.pos = s.pos;
		w.n_multi = s.n_multi; w.multi = b->wire_multi.data() + 16 * m0[i];
		for (int j = 0; j < s.n_multi; ++j) multi_to_wire(s.multi[j], b->wire_multi.data() + 16 * (m0[i] + (size_t)j));
		w.max_entries = b->max_ent[i]; w.n_aln = b->n_aln[i]; w.aln = (const uint8_t*)(b->rows.data() + b->row0[i]);
	}
	return NABWA_OK;
}

extern "C" int nabwa_bam_batch_restore(nabwa_bam_batch_t *b, const nabwa_wire_read_t *in)
{
	if (!b || !in) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (b->phase != 0 || b->searched) return nabwa_fail(NABWA_EINVAL, "restore needs a batch that was just created");
	const int n = (int)b->rec.size();
	b->n_aln.assign(n ? n : 1, 0); b->max_ent.assign(n ? n : 1, 0); b->row0.assign(n + 1, 0);
	/* the state may come from a socket (nabwa_worker_process): rows and positions index the SA and the reference on the GPU in pass 2, so
	 * what cannot come from this index stops here.  Rows run 0 .. seq_len, positions 0 .. l_pac; the two BWTs are of one text and its reverse */
	const uint32_t max_row = b->ix->bwt[0].seq_len < b->ix->bwt[1].seq_len ? b->ix->bwt[0].seq_len : b->ix->bwt[1].seq_len;
	const int64_t l_pac = b->ix->ref ? b->ix->ref->l_pac : (int64_t)max_row;
	/* (a hit with insertions at the very start of the text is positioned at rlen - (sa + len) < 0, kept as the u32 it wraps to and read
	 * back as negative, bwase.c:197: the last `len` values of the u32 range are positions of the library's own making) */
	auto pos_inside = [&](uint32_t pos, int32_t len) { return (int64_t)pos <= l_pac || (len > 0 && pos >= 0u - (uint32_t)len); };
	for (int i = 0; i < n; ++i) {
		const nabwa_wire_read_t &w = in[i];
		if (w.n_aln < 0 || w.n_multi < 0 || w.n_multi > NABWA_MAX_MULTI || (w.n_aln && !w.aln) || (w.n_multi && !w.multi)) { char m[96]; snprintf(m, sizeof m, "record %d: counts out of range", i); return nabwa_fail(NABWA_EINVAL, "%s", m); }
		if ((int64_t)w.len != b->off[i + 1] - b->off[i]) { char m[160]; snprintf(m, sizeof m, "record %d: positioned with a length of %d, the batch has %lld (other trimming options?)", i, w.len, (long long)(b->off[i + 1] - b->off[i])); return nabwa_fail(NABWA_EINVAL, "%s", m); }
		bool inside = w.sa <= max_row && pos_inside(w.pos, w.len);
		for (int j = 0; j < w.n_aln && inside; ++j) {
			uint32_t kl[2]; memcpy(kl, w.aln + 16 * (size_t)j + 4, 8);
			inside = kl[0] <= kl[1] && kl[1] <= max_row;
		}
		for (int j = 0; j < w.n_multi && inside; ++j) { uint32_t pos; memcpy(&pos, w.multi + 16 * (size_t)j, 4); inside = pos_inside(pos, w.len); }
		if (!inside) { char m[96]; snprintf(m, sizeof m, "record %d: hit row outside the index", i); return nabwa_fail(NABWA_EINVAL, "%s", m); }
		b->n_aln[i] = w.n_aln; b->max_ent[i] = w.max_entries; b->row0[i + 1] = b->row0[i] + w.n_aln;
	}
	if (!b->rows.resize(b->row0[n] ? (size_t)b->row0[n] : 1)) return nabwa_fail(NABWA_ENOMEM, "out of memory for the hit rows");
	if (!take_res(b)) return nabwa_fail(NABWA_ENOMEM, "out of memory for the batch's records");
	host_parallel(host_threads((size_t)n, BAM_MIN_N), (size_t)n, [&](int, size_t lo, size_t hi) {
		for (size_t i = lo; i < hi; ++i) {
			const nabwa_wire_read_t &w = in[i]; nabwa_pe_t &r = b->res[i]; nabwa_se_t &s = r.se;
			if (w.n_aln) memcpy(b->rows.data() + b->row0[i], w.aln, 16 * (size_t)w.n_aln);
			memset(&s, 0, offsetof(nabwa_se_t, cigar));                            /* as nabwa_se_posn leaves a record */
			s.n_cigar = 0; se_posn_reset(s);
			s.type = w.type & 3; s.strand = w.strand & 1; s.n_mm = w.n_mm; s.n_gapo = w.n_gapo; s.n_gape = w.n_gape; s.score = w.score; s.sa = w.sa; s.pos = w.pos;
			s.c1 = w.c1 & 0xfffffff; s.c2 = w.c2 & 0xfffffff; s.mapQ = w.mapQ; s.seQ = w.seQ; s.len = w.len; s.clip_len = w.clip_len; s.full_len = b->full_len[i];
			s.n_multi = w.n_multi;
			for (int j = 0; j < w.n_multi; ++j) multi_from_wire(w.multi + 16 * (size_t)j, s.multi[j]);
			pe_tail_reset(r);
		}
	});
	b->searched = true; b->phase = 1;
	return NABWA_OK;
}

/* one working record to another: the scalars, and of the arrays what their counts say is filled */
static void copy_filled(nabwa_pe_t &d, const nabwa_pe_t &r)
{
	const nabwa_se_t &s = r.se; nabwa_se_t &o = d.se;
	memcpy(&o, &s, offsetof(nabwa_se_t, cigar));
	if (s.n_cigar > 0) memcpy(o.cigar, s.cigar, sizeof(uint16_t) * (size_t)(s.n_cigar < NABWA_MAX_CIGAR ? s.n_cigar : NABWA_MAX_CIGAR));
	o.nm = s.nm;
	memcpy(o.md, s.md, strnlen(s.md, NABWA_MAX_MD - 1) + 1);
	o.n_multi = s.n_multi;
	for (int j = 0; j < s.n_multi && j < NABWA_MAX_MULTI; ++j) {
		memcpy(&o.multi[j], &s.multi[j], offsetof(nabwa_multi_t, cigar));
		if (s.multi[j].n_cigar > 0) memcpy(o.multi[j].cigar, s.multi[j].cigar, sizeof(uint16_t) * (size_t)(s.multi[j].n_cigar < NABWA_MAX_CIGAR ? s.multi[j].n_cigar : NABWA_MAX_CIGAR));
	}
	o.flag = s.flag; o.seqid = s.seqid; o.nn = s.nn; o.rpos = s.rpos; o.xt = s.xt;
	d.extra_flag = r.extra_flag; d.m_seqid = r.m_seqid; d.am = r.am; d.mapQ_paired = r.mapQ_paired; d.m_rpos = r.m_rpos; d.isize = r.isize;
}

/* ---- pass 2, singletons: bwa_refine_gapped + what bwa_update_bam1 derives */
static int finish_singletons(nabwa_bam_batch *b)
{
	std::vector<int> idx;
	for (size_t k = 0; k < b->kind.size(); ++k) if (b->kind[k] == 1 && !b->skip[k]) idx.push_back(b->first[k]);
	if (idx.size() == b->rec.size() && !idx.empty()) {       /* a batch of singletons only: in place, no gathering */
		int rc = nabwa_se_refine_strided(b->ix, (int)idx.size(), b->off.data(), b->seq.data(), b->rseq.data(), b->res.get(), sizeof(nabwa_pe_t));
		if (rc != NABWA_OK) return rc;
	} else if (!idx.empty()) {
		std::vector<int64_t> off(idx.size() + 1, 0); std::vector<uint8_t> sq, rq; std::vector<nabwa_se_t> se(idx.size());
		for (size_t t = 0; t < idx.size(); ++t) {
			const int i = idx[t]; const int64_t L = b->off[i + 1] - b->off[i];
			sq.insert(sq.end(), b->seq.begin() + b->off[i], b->seq.begin() + b->off[i] + L);
			rq.insert(rq.end(), b->rseq.begin() + b->off[i], b->rseq.begin() + b->off[i] + L);
			off[t + 1] = off[t] + L; memcpy(&se[t], &b->res[i].se, sizeof(nabwa_se_t));
		}
		sq.push_back(0); rq.push_back(0);
		int rc = nabwa_se_refine(b->ix, (int)idx.size(), off.data(), sq.data(), rq.data(), se.data());
		if (rc != NABWA_OK) return rc;
		for (size_t t = 0; t < idx.size(); ++t) memcpy(&b->res[idx[t]].se, &se[t], sizeof(nabwa_se_t));
	}
	return NABWA_OK;
}

/* the pairs of one read group that is not the whole batch: its reads are gathered, by all threads, finished and put back; of a 3 KB record
 * only what is filled travels */
static int finish_gathered(nabwa_bam_batch *b, const nabwa_isize_table *tab, const nabwa_isize_t &ii, const std::vector<int> &idx, uint64_t n_tot[2], uint64_t n_mapped[2])
{
	const int np = (int)idx.size();
	const size_t nr = 2 * (size_t)np;
	std::vector<int64_t> off(nr + 1, 0), r0(nr + 1, 0); std::vector<int32_t> na(nr);
	for (int t = 0; t < np; ++t) for (int e = 0; e < 2; ++e) {
		const int i = idx[t] + e; const size_t q = 2 * (size_t)t + e;
		off[q + 1] = off[q] + (b->off[i + 1] - b->off[i]); na[q] = b->n_aln[i]; r0[q + 1] = r0[q] + b->n_aln[i];
	}
	RawBytes sq, rq, rowb;
	Pooled<nabwa_pe_t> pe;          /* (declared last: it goes back to the pool first) */
	if (!pe.take(sizeof(nabwa_pe_t) * nr) || !sq.alloc((size_t)off[nr] + 1) || !rq.alloc((size_t)off[nr] + 1) || !rowb.alloc(sizeof(nabwa_aln1_t) * ((size_t)r0[nr] + 1)))
		return nabwa_fail(NABWA_ENOMEM, "out of memory for a read group's pairs");
	nabwa_aln1_t *rows = (nabwa_aln1_t*)rowb.data();
	host_parallel(host_threads(nr, BAM_MIN_N), nr, [&](int, size_t lo, size_t hi) {
		for (size_t q = lo; q < hi; ++q) {
			const int i = idx[q >> 1] + (int)(q & 1);
			memcpy(sq.data() + off[q], b->seq.data() + b->off[i], (size_t)(off[q + 1] - off[q]));
			memcpy(rq.data() + off[q], b->rseq.data() + b->off[i], (size_t)(off[q + 1] - off[q]));
			if (na[q]) memcpy(rows + r0[q], b->rows.data() + b->row0[i], sizeof(nabwa_aln1_t) * (size_t)na[q]);
			copy_filled(pe[q], b->res[i]);
		}
	});
	sq.data()[off[nr]] = 0; rq.data()[off[nr]] = 0; memset(&rows[r0[nr]], 0, sizeof(nabwa_aln1_t));
	int rc = nabwa_pe_finish_cached(b->ix, &b->opt, &b->popt, &ii, np, off.data(), sq.data(), rq.data(), na.data(), rows, pe.get(), n_tot, n_mapped, tab->poscache);
	if (rc == NABWA_OK) host_parallel(host_threads(nr, BAM_MIN_N), nr, [&](int, size_t lo, size_t hi) { for (size_t q = lo; q < hi; ++q) copy_filled(b->res[idx[q >> 1] + (int)(q & 1)], pe[q]); });
	return rc;
}

/* ---- pass 2, pairs: one read group at a time with that group's estimate (pass 2 draws no random numbers: its order is free) */
static int finish_pairs(nabwa_bam_batch *b, const nabwa_isize_table *tab, uint64_t n_tot[2], uint64_t n_mapped[2])
{
	std::map<std::string, std::vector<int>> groups;
	std::vector<int> in_order;
	for (size_t k = 0; k < b->kind.size(); ++k) if (b->kind[k] == 2 && !b->skip[k]) { groups[b->rg_names[b->rg[k]]].push_back(b->first[k]); in_order.push_back(b->first[k]); }
	/* who is first with a wide hit row is settled in record order (finish_pair's cache of positions, pe_finish.hip), not in group order */
	if (groups.size() > 1) nabwa_poscache_register(tab->poscache, b->popt.max_occ, (int)in_order.size(), in_order.data(), b->n_aln.data(), b->row0.data(), b->rows.data(), b->res.get());
	for (auto &g : groups) {
		nabwa_isize_t ii;
		nabwa_isize_table_get(tab, g.first.c_str(), &ii);
		const std::vector<int> &idx = g.second;
		int rc;
		if (2 * idx.size() == b->rec.size())           /* the whole batch is pairs of this one group: in place */
			rc = nabwa_pe_finish_cached(b->ix, &b->opt, &b->popt, &ii, (int)idx.size(), b->off.data(), b->seq.data(), b->rseq.data(), b->n_aln.data(), b->rows.data(), b->res.get(), n_tot, n_mapped, tab->poscache);
		else rc = finish_gathered(b, tab, ii, idx, n_tot, n_mapped);
		if (rc != NABWA_OK) return rc;
	}
	return NABWA_OK;
}

/* ---- pass 2, bwa_update_bam1 of every record */
static void update_all(nabwa_bam_batch *b)
{
	const nabwa_reference *R = b->ix->ref;
	host_parallel(host_threads(b->kind.size(), BAM_MIN_N), b->kind.size(), [&](int, size_t lo, size_t hi) {
		for (size_t k = lo; k < hi; ++k) {
			/* (a record's pieces lie far apart -- its parsed head, the end of its bytes in the arena where the tags go, the head and the MD field of
			 * its 3 KB working record: asked for ahead, the ones behind a pointer once that pointer is at hand) */
			if (k + 16 < hi) { const int f = b->first[k + 16]; __builtin_prefetch(&b->rec[f], 1); __builtin_prefetch(&b->res[f].se); __builtin_prefetch(b->res[f].se.md); __builtin_prefetch(&b->res[f].se.flag); }
			if (k + 8 < hi) { const BamRec &fr = b->rec[b->first[k + 8]]; __builtin_prefetch(fr.data.p + fr.data.n, 1); __builtin_prefetch(fr.data.p + fr.l_qname, 1); }
			const int i = b->first[k];
			if (b->skip[k]) continue;
			const bool dbg = (b->flags & NABWA_BAM_DEBUG) != 0;
			if (b->kind[k] == 1) update_bam(b->rec[i], R, b->res[i].se, 0, 0, b->opt.mode, b->opt.max_top2, dbg ? b->max_ent[i] : 0);
			else {
				update_bam(b->rec[i], R, b->res[i].se, &b->res[i + 1].se, &b->res[i], b->opt.mode, b->opt.max_top2, dbg ? b->max_ent[i] : 0);
				update_bam(b->rec[i + 1], R, b->res[i + 1].se, &b->res[i].se, &b->res[i + 1], b->opt.mode, b->opt.max_top2, dbg ? b->max_ent[i + 1] : 0);
			}
		}
	});
}

/* pass 2: pair_finish of every logical record (bam2bam.c:1178-1216, 643-658, 705-811) */
extern "C" int nabwa_bam_batch_pass2(nabwa_bam_batch_t *b, const nabwa_isize_table_t *tab, uint64_t n_tot[2], uint64_t n_mapped[2])
{
	if (!b || !tab) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (b->phase != 1) return nabwa_fail(NABWA_EINVAL, "pass 2 needs a batch that went through pass 1 once");
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double tq0 = now_s();
	if (!b->res && !unpark(b)) return nabwa_fail(NABWA_ENOMEM, "out of memory for the batch's records");
	int rc = finish_singletons(b);
	if (rc == NABWA_OK) rc = finish_pairs(b, tab, n_tot, n_mapped);
	if (rc != NABWA_OK) return rc;
	const double tq1 = now_s();
	update_all(b);
	b->phase = 2;
	/* the records are complete: the 3 KB per read that led to them go back to the pool (a batch may wait long for its turn to be written) */
	b->res.give();
	if (timing) fprintf(stderr, "[nabwa] bam_batch_pass2 %zu records: finishing chains %.3f s, bwa_update_bam1 %.3f s\n", b->rec.size(), tq1 - tq0, now_s() - tq1);
	return NABWA_OK;
}

/* the records as they now are (after create: cleaned; after pass 2: aligned), in logical-record order; with NABWA_BAM_ONLY_ALIGNED
 * without the logical records a read of which is flagged unmapped (pair_print_bam, bam2bam.c:911-925); out_off then has one more
 * entry than records were written, and the rest of its n_rec + 1 entries repeat the end */
extern "C" int nabwa_bam_batch_output(const nabwa_bam_batch_t *b, uint8_t *out, int64_t cap, int64_t *out_off, int64_t *n_bytes)
{
	if (!b || !n_bytes) return nabwa_fail(NABWA_EINVAL, "null argument");
	const size_t n = b->rec.size();
	std::vector<int> pick;
	if ((b->flags & NABWA_BAM_ONLY_ALIGNED) && b->phase == 2) {
		pick.reserve(n);
		for (size_t k = 0; k < b->kind.size(); ++k) {
			const int i = b->first[k];
			bool keep = true;
			for (int e = 0; e < b->kind[k]; ++e) if (b->rec[i + e].flag & F_SU) keep = false;      /* (before pass 2 the flag is the input's) */
			if (keep) for (int e = 0; e < b->kind[k]; ++e) pick.push_back(i + e);
		}
	} else {       /* every record, in the order they lie in (logical records are consecutive) */
		pick.resize(n);
		int *const pp = pick.data();
		host_parallel(host_threads(n, BAM_MIN_N), n, [pp](int, size_t lo, size_t hi) { for (size_t t = lo; t < hi; ++t) pp[t] = (int)t; });
	}
	const size_t m = pick.size();
	std::vector<int64_t> at(n + 1, 0);
	host_parallel(host_threads(m, BAM_MIN_N), m, [&](int, size_t lo, size_t hi) { for (size_t t = lo; t < hi; ++t) at[t + 1] = 36 + (int64_t)b->rec[pick[t]].data.size(); });      /* the sizes by all threads ... */
	for (size_t t = 0; t < m; ++t) at[t + 1] += at[t];                                                                                                     /* ... their sums by one */
	for (size_t t = m; t < n; ++t) at[t + 1] = at[m];
	if (out_off) memcpy(out_off, at.data(), sizeof(int64_t) * (n + 1));
	*n_bytes = at[m];
	if (!out || cap < at[m]) return nabwa_fail(NABWA_ECAP, "output buffer too small");
	host_parallel(host_threads(m, BAM_MIN_N), m, [&](int, size_t lo, size_t hi) {
		for (size_t t = lo; t < hi; ++t) {
			if (t + 8 < hi) { const BamRec &fr = b->rec[pick[t + 8]]; __builtin_prefetch(fr.data.p); __builtin_prefetch(fr.data.p + 64); __builtin_prefetch(fr.data.p + 128); __builtin_prefetch(fr.data.p + 192); }
			if (t + 16 < hi) __builtin_prefetch(&b->rec[pick[t + 16]]);
			write_rec(b->rec[pick[t]], out + at[t]);
		}
	});
	return NABWA_OK;
}

extern "C" int nabwa_bam_batch_kinds(const nabwa_bam_batch_t *b, uint8_t *kind_out)
{
	if (!b || !kind_out) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (size_t k = 0; k < b->kind.size(); ++k) kind_out[k] = (uint8_t)b->kind[k];
	return NABWA_OK;
}

extern "C" int nabwa_bam_batch_counts(const nabwa_bam_batch_t *b, int *n_records, int *n_logical)
{
	if (!b) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (n_records) *n_records = (int)b->rec.size();
	if (n_logical) *n_logical = (int)b->kind.size();
	return NABWA_OK;
}
