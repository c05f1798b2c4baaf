// finish_gpu.hip -- host side of the finishing chains' device path: the reference in HBM, the launches of finish_kernels.hip around the
// global alignment kernel, and the entry points nabwa_refine_gapped_core / nabwa_cal_md / nabwa_finish_counts built on them.
//
// What travels per batch: the reads once (2 x off[n] bytes), 40 bytes per refinement job and 32 per mapped record down; per job its
// position, its operation count and the CIGAR slots in use, per record NM, the string's length and the string up.  The windows, the
// queries in alignment orientation and the alignment kernel's 32-bit rows never leave the device.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <memory>
#include <vector>
#include "../../include/nabwa.h"
#include "launchers.hpp"
#include "nabwa_internal.hpp"
#include "dev_pool.hpp"
#include "dp_params.hpp"
#include "finish_gpu.hpp"

namespace {
std::atomic<uint64_t> g_fin_jobs(0), g_fin_md(0), g_fin_calls(0), g_fin_ref_bytes(0);
}

extern "C" void nabwa_finish_counts(uint64_t out[4])
{
	if (!out) return;
	out[0] = g_fin_jobs.load(); out[1] = g_fin_md.load(); out[2] = g_fin_calls.load(); out[3] = g_fin_ref_bytes.load();
}
void nabwa_finish_count_chain_call() { ++g_fin_calls; }

/* ------------------------------------------------------------------ the reference in HBM */

int nabwa_finish_reference(nabwa_index_t *ix, int which_ref, FinRef *out)
{
	const nabwa_reference *R = which_ref ? ix->ref_nt : ix->ref;
	if (!R) return nabwa_fail(NABWA_EINVAL, which_ref ? "index has no nucleotide reference attached (nabwa_index_attach_nt_reference)"
													  : "index has no reference attached (nabwa_index_attach_reference)");
	if (which_ref && !ix->d_ntpac) return nabwa_fail(NABWA_EINVAL, "index has no nucleotide reference attached (nabwa_index_attach_nt_reference)");
	std::lock_guard<std::mutex> lk(ix->fin_mu);
	if (!ix->fin_ready[which_ref]) {
		HIP_CHECK(hipSetDevice(ix->device));
		if (!which_ref) {
			const uint64_t nb = (uint64_t)(R->l_pac / 4 + 1);       /* (the host copy is at least 8 bytes longer) */
			uint8_t *d = nullptr;
			HIP_CHECK(hipMalloc((void**)&d, nb));
			const hipError_t e = hipMemcpy(d, R->pac.data(), nb, hipMemcpyHostToDevice);
			if (e != hipSuccess) { (void)hipFree(d); return nabwa_hip_fail(e, "uploading the pac", __FILE__, __LINE__); }
			ix->d_pac = d; ix->pac_bytes = nb; ix->bytes += nb; g_fin_ref_bytes += nb;
		}
		std::vector<FinHole> h(R->holes.size());
		for (size_t i = 0; i < h.size(); ++i) h[i] = FinHole{ R->holes[i].offset, R->holes[i].len, (int32_t)(uint8_t)R->holes[i].amb };
		const uint64_t hb = (uint64_t)(h.size() ? h.size() : 1) * sizeof(FinHole);
		void *dh = nullptr;
		HIP_CHECK(hipMalloc(&dh, hb));
		if (!h.empty()) {
			const hipError_t e = hipMemcpy(dh, h.data(), h.size() * sizeof(FinHole), hipMemcpyHostToDevice);
			if (e != hipSuccess) { (void)hipFree(dh); return nabwa_hip_fail(e, "uploading the hole table", __FILE__, __LINE__); }
		}
		ix->d_holes[which_ref] = dh; ix->holes_bytes[which_ref] = hb; ix->n_holes_dev[which_ref] = (int)h.size();
		ix->bytes += hb; g_fin_ref_bytes += hb;
		ix->fin_ready[which_ref] = true;
	}
	out->pac = which_ref ? ix->d_ntpac : ix->d_pac;
	out->l_pac = R->l_pac;
	out->holes = (const FinHole*)ix->d_holes[which_ref];
	out->n_holes = ix->n_holes_dev[which_ref];
	out->pad = 0;
	return NABWA_OK;
}

void nabwa_finish_drop_reference(nabwa_index_t *ix)
{
	std::lock_guard<std::mutex> lk(ix->fin_mu);
	(void)hipSetDevice(ix->device);
	if (ix->d_pac) { (void)hipFree(ix->d_pac); ix->bytes -= ix->pac_bytes; g_fin_ref_bytes -= ix->pac_bytes; ix->d_pac = nullptr; ix->pac_bytes = 0; }
	for (int w = 0; w < 2; ++w) {
		if (ix->d_holes[w]) { (void)hipFree(ix->d_holes[w]); ix->bytes -= ix->holes_bytes[w]; g_fin_ref_bytes -= ix->holes_bytes[w]; }
		ix->d_holes[w] = nullptr; ix->holes_bytes[w] = 0; ix->n_holes_dev[w] = 0; ix->fin_ready[w] = false;
	}
}

/* ------------------------------------------------------------------ one batch on the device */

FinGpu::FinGpu(nabwa_index_t *ix_) : ix(ix_), timing(getenv("NABWA_TIMING") != 0) {}
FinGpu::~FinGpu() { (void)hipStreamSynchronize(0); }

int FinGpu::set_reads(int64_t n_bytes, const uint8_t *seq, const uint8_t *rseq)
{
	const double t0 = now_s();
	HIP_CHECK(hipSetDevice(ix->device));
	HIP_CHECK(hipStreamSynchronize(0));               /* (a chain that changes its reads: nothing may still read the old ones) */
	const size_t nb = (size_t)(n_bytes > 0 ? n_bytes : 1);
	if (seq) { HIP_CHECK(d_seq.get(ix, nb)); if (n_bytes > 0) HIP_CHECK(hipMemcpy(d_seq, seq, (size_t)n_bytes, hipMemcpyHostToDevice)); }
	HIP_CHECK(d_rseq.get(ix, nb));
	if (n_bytes > 0) HIP_CHECK(hipMemcpy(d_rseq, rseq, (size_t)n_bytes, hipMemcpyHostToDevice));
	t_up += now_s() - t0;
	return NABWA_OK;
}

namespace {
/* HIP events around a stretch of stream 0 when NABWA_TIMING asks for them */
struct KernelClock {
	DevEvent a, b; bool on;
	explicit KernelClock(bool on_) : on(on_) { if (on) { on = hipEventCreate(&a.e) == hipSuccess && hipEventCreate(&b.e) == hipSuccess; } }
	void start() { if (on) (void)hipEventRecord(a, 0); }
	void stop() { if (on) (void)hipEventRecord(b, 0); }
	float ms() { float v = 0; if (on && hipEventSynchronize(b) == hipSuccess) (void)hipEventElapsedTime(&v, a, b); return v; }
};
}

int FinGpu::refine(int which_ref, int end_correct, size_t nj, const FinJob *jobs, uint32_t *pos_out, int32_t *n_cigar, uint16_t *rows, int max_cigar)
{
	if (nj == 0) return NABWA_OK;
	FinRef R;
	if (const int r = nabwa_finish_reference(ix, which_ref, &R)) return r;
	HIP_CHECK(hipSetDevice(ix->device));
	static const int maq[25] = { 11,-19,-19,-19,-13, -19,11,-19,-19,-13, -19,-19,11,-19,-13, -19,-19,-19,11,-13, -13,-13,-13,-13,-13 };  /* aln_sm_maq */
	const size_t CHUNK = 1u << 16;                  /* tasks per launch of the alignment kernel: bounds its traceback scratch */
	bool bad = false;
	for (size_t c0 = 0; c0 < nj; c0 += CHUNK) {
		const double t0 = now_s();
		const int m = (int)std::min(CHUNK, nj - c0);
		std::vector<int64_t> ro((size_t)m + 1, 0), qo((size_t)m + 1, 0);
		for (int i = 0; i < m; ++i) { ro[i + 1] = ro[i] + jobs[c0 + i].win_n; qo[i + 1] = qo[i] + jobs[c0 + i].len; }
		PoolBuf<FinJob> d_jobs; PoolBuf<uint32_t> d_pos; PoolBuf<int32_t> d_nc; PoolBuf<uint16_t> d_rows; PoolBuf<unsigned int> d_bad;
		StreamDrain drain{ 0 };
		HIP_CHECK(d_jobs.get(ix, (size_t)m * sizeof(FinJob))); HIP_CHECK(d_pos.get(ix, (size_t)m * 4)); HIP_CHECK(d_nc.get(ix, (size_t)m * 4));
		HIP_CHECK(d_rows.get(ix, (size_t)m * max_cigar * 2)); HIP_CHECK(d_bad.get(ix, 4));
		const double t1 = now_s();
		HIP_CHECK(hipMemcpy(d_jobs, jobs + c0, (size_t)m * sizeof(FinJob), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemset(d_bad, 0, 4));
		const double t2 = now_s();
		KernelClock clk(timing);
		double t3 = t2;
		const int r = nabwa_dp_global_device(ix->device, m, ro.data(), qo.data(), 26, 9, 5, maq, 50, max_cigar,        /* aln_param_bwa, stdaln.c:227 */
			[&](const DpDeviceIO &D) -> int {
				clk.start();
				nabwa_launch_refine_window(R.pac, d_jobs, m, d_seq, d_rseq, D.d_ro, D.d_qo, D.d_ref, D.d_qry, 0);
				HIP_CHECK(hipGetLastError());
				return NABWA_OK;
			},
			[&](const DpParams &P) -> int {
				nabwa_launch_refine_cigar(d_jobs, m, end_correct, P.n_cigar, P.cigar, max_cigar, d_pos, d_nc, d_rows, d_bad, 0);
				HIP_CHECK(hipGetLastError());
				clk.stop();
				ms_kernels += clk.ms();
				t3 = now_s();
				unsigned int nb = 0;
				HIP_CHECK(hipMemcpy(&nb, d_bad, 4, hipMemcpyDeviceToHost));
				if (nb) bad = true;
				HIP_CHECK(hipMemcpy(pos_out + c0, d_pos, (size_t)m * 4, hipMemcpyDeviceToHost));
				HIP_CHECK(hipMemcpy(n_cigar + c0, d_nc, (size_t)m * 4, hipMemcpyDeviceToHost));
				int slots = 0;                            /* only the CIGAR slots in use travel */
				for (int i = 0; i < m; ++i) slots = std::max(slots, n_cigar[c0 + i]);
				if (slots) HIP_CHECK(hipMemcpy2D(rows + c0 * (size_t)max_cigar, (size_t)max_cigar * 2, d_rows, (size_t)max_cigar * 2, (size_t)slots * 2, (size_t)m,
												 hipMemcpyDeviceToHost));
				return NABWA_OK;
			}, nullptr);
		if (r != NABWA_OK) return r;
		t_desc += t1 - t0; t_up += t2 - t1; t_down += now_s() - t3;
	}
	g_fin_jobs += nj;
	if (bad) return nabwa_fail(NABWA_ECAP, "refined CIGAR longer than NABWA_MAX_CIGAR");
	return NABWA_OK;
}

int FinGpu::md(int which_ref, size_t n, const FinRec *recs, const uint16_t *cig, size_t n_cig, int32_t *nm, int64_t *md_off, std::vector<char> &md_out)
{
	md_off[0] = 0;
	md_out.clear();
	if (n == 0) return NABWA_OK;
	FinRef R;
	if (const int r = nabwa_finish_reference(ix, which_ref, &R)) return r;
	HIP_CHECK(hipSetDevice(ix->device));
	const double t0 = now_s();
	PoolBuf<FinRec> d_recs; PoolBuf<uint16_t> d_cig; PoolBuf<int32_t> d_nm, d_len; PoolBuf<int64_t> d_off; PoolBuf<char> d_md;
	StreamDrain drain{ 0 };
	HIP_CHECK(d_recs.get(ix, n * sizeof(FinRec))); HIP_CHECK(d_cig.get(ix, (n_cig ? n_cig : 1) * 2)); HIP_CHECK(d_nm.get(ix, n * 4)); HIP_CHECK(d_len.get(ix, n * 4));
	HIP_CHECK(d_off.get(ix, n * 8));
	HIP_CHECK(hipMemcpy(d_recs, recs, n * sizeof(FinRec), hipMemcpyHostToDevice));
	if (n_cig) HIP_CHECK(hipMemcpy(d_cig, cig, n_cig * 2, hipMemcpyHostToDevice));
	const double t1 = now_s();
	KernelClock c1(timing);
	c1.start();
	nabwa_launch_md_count(&R, d_recs, (int)n, d_seq, d_rseq, d_cig, d_nm, d_len, 0);
	HIP_CHECK(hipGetLastError());
	c1.stop();
	ms_kernels += c1.ms();
	const double t2 = now_s();
	std::vector<int32_t> len(n);
	HIP_CHECK(hipMemcpy(nm, d_nm, n * 4, hipMemcpyDeviceToHost));
	HIP_CHECK(hipMemcpy(len.data(), d_len, n * 4, hipMemcpyDeviceToHost));
	for (size_t i = 0; i < n; ++i) md_off[i + 1] = md_off[i] + len[i] + 1;
	const double t3 = now_s();
	HIP_CHECK(d_md.get(ix, (size_t)md_off[n]));
	HIP_CHECK(hipMemcpy(d_off, md_off, n * 8, hipMemcpyHostToDevice));
	const double t4 = now_s();
	KernelClock c2(timing);
	c2.start();
	nabwa_launch_md_write(&R, d_recs, (int)n, d_seq, d_rseq, d_cig, d_off, d_md, 0);
	HIP_CHECK(hipGetLastError());
	c2.stop();
	ms_kernels += c2.ms();
	const double t5 = now_s();
	md_out.resize((size_t)md_off[n]);
	HIP_CHECK(hipMemcpy(md_out.data(), d_md, (size_t)md_off[n], hipMemcpyDeviceToHost));
	t_up += (t1 - t0) + (t4 - t3); t_down += (t3 - t2) + (now_s() - t5);
	g_fin_md += n;
	return NABWA_OK;
}

int FinGpu::md_records(int which_ref, void *base, size_t stride, int n, const int64_t *off)
{
	const double t0 = now_s();
	auto rec = [&](size_t i) -> nabwa_se_t& { return *(nabwa_se_t*)((char*)base + i * stride); };
	const int nt = host_threads((size_t)n, 4096);
	/* the records' descriptors, slice by slice in threads, then the slices side by side in one array each (copied in threads too: two
	 * million descriptors through one thread's push_back cost more than the kernels) */
	struct Part { std::vector<FinRec> recs; std::vector<uint16_t> cig; size_t r0 = 0, c0 = 0; };
	std::vector<Part> part((size_t)nt);
	rec_k.assign((size_t)n, -1);
	host_parallel(nt, (size_t)n, [&](int t, size_t lo, size_t hi) {
		Part &P = part[(size_t)t];
		P.recs.reserve(hi - lo); P.cig.reserve((hi - lo) / 2);
		for (size_t i = lo; i < hi; ++i) {
			if (i + 8 < hi) __builtin_prefetch(&rec(i + 8));
			const nabwa_se_t &s = rec(i);
			if (s.type == 0) continue;
			FinRec Q; memset(&Q, 0, sizeof Q);
			Q.src_off = off[i]; Q.cig_off = (int64_t)P.cig.size(); Q.pos = s.pos; Q.len = s.len; Q.n_cigar = s.n_cigar; Q.copy = s.strand ? 1 : 0;
			if (s.n_cigar) P.cig.insert(P.cig.end(), s.cigar, s.cigar + s.n_cigar);
			rec_k[i] = (int32_t)P.recs.size();                          /* within the slice; its base is added below */
			P.recs.push_back(Q);
		}
	});
	size_t nr = 0, nc = 0;
	for (Part &P : part) { P.r0 = nr; P.c0 = nc; nr += P.recs.size(); nc += P.cig.size(); }
	std::unique_ptr<FinRec[]> recs(new FinRec[nr ? nr : 1]); std::unique_ptr<uint16_t[]> cig(new uint16_t[nc ? nc : 1]);
	host_parallel(nt, (size_t)n, [&](int t, size_t lo, size_t hi) {
		Part &P = part[(size_t)t];
		for (FinRec &Q : P.recs) Q.cig_off += (int64_t)P.c0;
		if (!P.recs.empty()) memcpy(recs.get() + P.r0, P.recs.data(), P.recs.size() * sizeof(FinRec));
		if (!P.cig.empty()) memcpy(cig.get() + P.c0, P.cig.data(), P.cig.size() * 2);
		if (P.r0) for (size_t i = lo; i < hi; ++i) if (rec_k[i] >= 0) rec_k[i] += (int32_t)P.r0;
	});
	t_desc += now_s() - t0;
	rec_nm.resize(nr ? nr : 1); rec_md_off.assign(nr + 1, 0);
	return md(which_ref, nr, recs.get(), cig.get(), nc, rec_nm.data(), rec_md_off.data(), rec_md);
}

void FinGpu::report(const char *what) const
{
	if (timing) fprintf(stderr, "[nabwa] %s device path: descriptors %.3f s, upload %.3f s, kernels %.3f ms (HIP events), download %.3f s\n", what, t_desc, t_up,
						(double)ms_kernels, t_down);
}

/* ------------------------------------------------------------------ the entry points */

static int check_queries(int n, const int64_t *qry_off)
{
	for (int i = 0; i < n; ++i) {
		const int64_t l = qry_off[i + 1] - qry_off[i];
		if (l < 1 || l > 0x3fff) return nabwa_fail(NABWA_EINVAL, "query length outside 1 .. 0x3fff");
	}
	if (n && qry_off[0] < 0) return nabwa_fail(NABWA_EINVAL, "negative offset");
	return NABWA_OK;
}

extern "C" int nabwa_refine_gapped_core(nabwa_index_t *ix, int which_ref, int is_end_correct, int n, const int64_t *qry_off, const uint8_t *qry,
										const int32_t *ext, uint32_t *pos, int32_t *n_cigar, uint16_t *cigar, int max_cigar)
{
	if (!ix || n < 0 || which_ref < 0 || which_ref > 1 || max_cigar < 1 || (n && (!qry_off || !qry || !ext || !pos || !n_cigar || !cigar)))
		return nabwa_fail(NABWA_EINVAL, "bad argument");
	if (const int r = check_queries(n, qry_off)) return r;
	for (int i = 0; i < n; ++i) if (ext[i] > 0xffff || ext[i] < -0xffff) return nabwa_fail(NABWA_EINVAL, "ext outside -0xffff .. 0xffff");
	if (n) for (int64_t k = qry_off[0]; k < qry_off[n]; ++k) if (qry[k] > 4) return nabwa_fail(NABWA_EINVAL, "query code above 4");      /* (the alignment kernel indexes its 5 x 5 matrix with it) */
	if (nabwa_device_count() <= 0) return nabwa_fail(NABWA_ENODEV, "no HIP device");
	const nabwa_reference *R = which_ref ? ix->ref_nt : ix->ref;
	if (!R) return nabwa_fail(NABWA_EINVAL, which_ref ? "index has no nucleotide reference attached (nabwa_index_attach_nt_reference)"
													  : "index has no reference attached (nabwa_index_attach_reference)");
	if (nabwa_device_count() <= ix->device) return nabwa_fail(NABWA_ENODEV, "no such HIP device");
	if (n == 0) return NABWA_OK;
	std::vector<FinJob> jobs((size_t)n);
	for (int i = 0; i < n; ++i) {
		FinJob &J = jobs[(size_t)i]; memset(&J, 0, sizeof J);
		J.src_off = qry_off[i]; J.len = (int32_t)(qry_off[i + 1] - qry_off[i]); J.ext = ext[i]; J.copy = 1;
		fin_job_extent(R->l_pac, is_end_correct != 0, pos[i], J);
	}
	FinGpu G(ix);
	if (const int r = G.set_reads(qry_off[n], nullptr, qry)) return r;
	std::vector<uint32_t> p((size_t)n);
	const int r = G.refine(which_ref, is_end_correct != 0, (size_t)n, jobs.data(), p.data(), n_cigar, cigar, max_cigar);
	if (r != NABWA_OK && r != NABWA_ECAP) return r;
	memcpy(pos, p.data(), (size_t)n * 4);
	G.report("nabwa_refine_gapped_core");
	return r;
}

extern "C" int nabwa_cal_md(nabwa_index_t *ix, int which_ref, int n, const int64_t *qry_off, const uint8_t *qry, const uint32_t *pos,
							const int32_t *n_cigar, const uint16_t *cigar, int max_cigar, int32_t *nm, int64_t *md_off, char *md, int64_t md_cap)
{
	if (!ix || n < 0 || which_ref < 0 || which_ref > 1 || max_cigar < 0 || md_cap < 0 || !md_off || (n && (!qry_off || !qry || !pos || !n_cigar || !nm)) || (md_cap && !md))
		return nabwa_fail(NABWA_EINVAL, "bad argument");
	if (const int r = check_queries(n, qry_off)) return r;
	size_t n_cig = 0;
	for (int i = 0; i < n; ++i) {
		if (n_cigar[i] < 0 || n_cigar[i] > max_cigar || (n_cigar[i] && !cigar)) return nabwa_fail(NABWA_EINVAL, "n_cigar outside 0 .. max_cigar");
		if (n_cigar[i]) {                              /* the CIGAR must consume the query exactly: the kernel reads the read through it */
			int64_t used = 0;
			for (int k = 0; k < n_cigar[i]; ++k) { const uint16_t c = cigar[(size_t)i * max_cigar + k]; if (FIN_COP(c) != 2) used += FIN_CLEN(c); }
			if (used != qry_off[i + 1] - qry_off[i]) return nabwa_fail(NABWA_EINVAL, "a CIGAR does not consume its query");
		}
		n_cig += (size_t)n_cigar[i];
	}
	if (nabwa_device_count() <= 0) return nabwa_fail(NABWA_ENODEV, "no HIP device");
	const nabwa_reference *R = which_ref ? ix->ref_nt : ix->ref;
	if (!R) return nabwa_fail(NABWA_EINVAL, which_ref ? "index has no nucleotide reference attached (nabwa_index_attach_nt_reference)"
													  : "index has no reference attached (nabwa_index_attach_reference)");
	for (int i = 0; i < n; ++i)
		if (!n_cigar[i] && (int64_t)pos[i] + (qry_off[i + 1] - qry_off[i]) > R->l_pac)
			return nabwa_fail(NABWA_EINVAL, "an ungapped record runs past the end of the reference");
	if (nabwa_device_count() <= ix->device) return nabwa_fail(NABWA_ENODEV, "no such HIP device");
	md_off[0] = 0;
	if (n == 0) return NABWA_OK;
	std::vector<FinRec> recs((size_t)n); std::vector<uint16_t> cig; cig.reserve(n_cig);
	for (int i = 0; i < n; ++i) {
		FinRec &Q = recs[(size_t)i]; memset(&Q, 0, sizeof Q);
		Q.src_off = qry_off[i]; Q.cig_off = (int64_t)cig.size(); Q.pos = pos[i]; Q.len = (int32_t)(qry_off[i + 1] - qry_off[i]); Q.n_cigar = n_cigar[i]; Q.copy = 1;
		if (n_cigar[i]) cig.insert(cig.end(), cigar + (size_t)i * max_cigar, cigar + (size_t)i * max_cigar + n_cigar[i]);
	}
	FinGpu G(ix);
	if (const int r = G.set_reads(qry_off[n], nullptr, qry)) return r;
	std::vector<char> out;
	if (const int r = G.md(which_ref, (size_t)n, recs.data(), cig.data(), cig.size(), nm, md_off, out)) return r;
	G.report("nabwa_cal_md");
	if (md_off[n] > md_cap) return nabwa_fail(NABWA_ECAP, "md_cap too small: md_off[n] bytes are needed");
	memcpy(md, out.data(), out.size());
	return NABWA_OK;
}
