// finish_gpu.hpp -- the device path of the finishing chains (finish_gpu.hip): refinement of gapped hits and MD / NM with the reference
// held in HBM.  The chains take it when NABWA_FINISH=gpu; nabwa_refine_gapped_core and nabwa_cal_md are built on the same pieces.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "nabwa_internal.hpp"
#include "dev_pool.hpp"
#include "finish_body.hpp"

#pragma GCC visibility push(hidden)

/* NABWA_FINISH, read at every call: 0 = host (unset or "host"), 1 = gpu, -1 = anything else */
static inline int nabwa_finish_mode()
{
	const char *e = getenv("NABWA_FINISH");
	if (!e || !strcmp(e, "host")) return 0;
	return strcmp(e, "gpu") ? -1 : 1;
}

/* the extent of a job's window (bwase.c:197-209) from its 32-bit position, length and ext: arithmetic only, no access to the pac.
 * Sets pos (signed, bwase.c:197), win_lo and win_n; 0 <= win_lo and win_lo + win_n <= l_pac. */
static inline void fin_job_extent(int64_t l_pac, bool end_correct, uint32_t pos, FinJob &J)
{
	const int64_t ref_len = (int64_t)J.len + (J.ext < 0 ? -(int64_t)J.ext : (int64_t)J.ext);
	const int64_t p = (int64_t)pos > l_pac ? (int64_t)(int32_t)pos : (int64_t)pos;
	int64_t lo, hi;
	if (J.ext > 0) { lo = p > 0 ? p : 0; hi = p + ref_len < l_pac ? p + ref_len : l_pac; }
	else { const int64_t x = p + (end_correct ? J.len : ref_len); lo = x - ref_len > 0 ? x - ref_len : 0; hi = x < l_pac ? x : l_pac; }
	J.pos = p; J.win_lo = lo; J.win_n = hi > lo ? (int32_t)(hi - lo) : 0;
	if (J.win_n == 0) J.win_lo = 0;
}

/* the copies of the reference the kernels read: made by the first call that needs them, under the index's lock, and kept with it;
 * which_ref 0 = ix->ref, 1 = the nucleotide bases of a colour index (d_ntpac) under the colour annotations' holes */
int nabwa_finish_reference(nabwa_index_t *ix, int which_ref, FinRef *out);
/* a new reference is attached, or the index goes: the copies are freed */
void nabwa_finish_drop_reference(nabwa_index_t *ix);

/* One batch on the device path.  The reads are uploaded once (set_reads; again only when a chain changes them, as the colour chain does
 * with its decoded reads) and serve the refinement and the MD strings. */
struct FinGpu {
	nabwa_index_t *ix = nullptr;
	PoolBuf<uint8_t> d_seq, d_rseq;             /* reads0 = seq (the reads reversed), reads1 = rseq (or queries in alignment orientation) */
	bool timing = false;
	double t_desc = 0, t_up = 0, t_down = 0; float ms_kernels = 0;       /* NABWA_TIMING: descriptors, upload, download (s); kernels by HIP events (ms) */
	explicit FinGpu(nabwa_index_t *ix_);
	~FinGpu();
	/* seq may be null (nabwa_refine_gapped_core / nabwa_cal_md: every query is a copy of reads1) */
	int set_reads(int64_t n_bytes, const uint8_t *seq, const uint8_t *rseq);
	/* jobs with their extents set (win_lo, win_n, pos signed, src_off, len, ext, copy): pos_out / n_cigar per job, rows max_cigar wide.
	 * NABWA_ECAP when a path has more than max_cigar operations. */
	int refine(int which_ref, int end_correct, size_t nj, const FinJob *jobs, uint32_t *pos_out, int32_t *n_cigar, uint16_t *rows, int max_cigar);
	/* records with cig_off into cig[0, n_cig): nm per record, md_off[0 .. n] and the strings back to back, NUL-terminated */
	int md(int which_ref, size_t n, const FinRec *recs, const uint16_t *cig, size_t n_cig, int32_t *nm, int64_t *md_off, std::vector<char> &md_out);
	/* MD / NM of every mapped record (type != 0) of a batch of nabwa_se_t-headed records, kept here; the chain's own loop over the
	 * records then takes record i's with take_md (false: the string does not fit NABWA_MAX_MD -- the field holds its cut-off head and the
	 * chain reports NABWA_ECAP, as the host path does) */
	int md_records(int which_ref, void *base, size_t stride, int n, const int64_t *off);
	bool take_md(int i, nabwa_se_t &s) const
	{
		const int32_t k = rec_k[(size_t)i];
		if (k < 0) return true;
		const int64_t l = rec_md_off[(size_t)k + 1] - rec_md_off[(size_t)k];             /* with the NUL */
		s.nm = rec_nm[(size_t)k];
		if (l > NABWA_MAX_MD) { memcpy(s.md, rec_md.data() + rec_md_off[(size_t)k], NABWA_MAX_MD - 1); s.md[NABWA_MAX_MD - 1] = 0; return false; }
		memcpy(s.md, rec_md.data() + rec_md_off[(size_t)k], (size_t)l);
		return true;
	}
	std::vector<int32_t> rec_k, rec_nm; std::vector<int64_t> rec_md_off; std::vector<char> rec_md;      /* md_records' results: record -> slot, NM, strings */
	void report(const char *what) const;
};

/* counters of nabwa_finish_counts */
void nabwa_finish_count_chain_call();

#pragma GCC visibility pop
