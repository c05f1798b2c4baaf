// dp_align.hip -- host side of the batched alignment entry points (aln_global_core, aln_extend_core, aln_local_core of stdaln.c):
// the device working memory, the upload of the tasks, the kernel launches (dp_global.hip, dp_wave.hip) and the paths.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <vector>
#include "../../include/nabwa.h"
#include "nabwa_internal.hpp"
#include "host_util.hpp"
#include "dp_params.hpp"

/* Working memory of the alignment entry points: one grow-only block per device, kept between calls (hipMalloc / hipFree of the
 * traceback matrices -- 1.5 GB for 64 k pairs of 150 bases -- cost more than the kernels), handed out under a lock for the length
 * of one launch.  nabwa_dp_scratch_release gives it back. */
namespace {
struct DevArena { std::mutex mu; void *base = 0; size_t cap = 0; };
DevArena g_arena[16];
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

/* One launch's share of the arena: first the n tasks' offsets and sequences (ref_off / qry_off with ref / qry, as the entry points
 * take them), then the kernel's own buffers in the order reserve() listed them, handed out by next(). */
struct ArenaUse {                 /* at most 8 kernel buffers */
	DevArena &A; std::unique_lock<std::mutex> lk;
	size_t used = 0, buf_sz[8], n_buf = 0, buf_i = 0;
	int64_t *d_ro = 0, *d_qo = 0; uint8_t *d_ref = 0, *d_qry = 0;
	explicit ArenaUse(int dev) : A(g_arena[dev & 15]), lk(A.mu) {}
	int reserve(int n, const int64_t *ro, const int64_t *qo, std::initializer_list<size_t> bufs)
	{
		const size_t sz[4] = { (size_t)(n + 1) * 8, (size_t)(n + 1) * 8, (size_t)ro[n] + 16, (size_t)qo[n] + 16 };
		n_buf = 0; buf_i = 0;
		for (size_t z : bufs) buf_sz[n_buf++] = z;
		size_t need = 0; for (size_t z : sz) need += up256(z); for (size_t z : bufs) need += up256(z);
		used = 0;
		if (need > A.cap) {
			if (A.base) { (void)hipFree(A.base); A.base = 0; A.cap = 0; }
			const size_t c = need + need / 4;
			HIP_CHECK(hipMalloc(&A.base, c));
			A.cap = c;
		}
		d_ro = take<int64_t>(sz[0]); d_qo = take<int64_t>(sz[1]); d_ref = take<uint8_t>(sz[2]); d_qry = take<uint8_t>(sz[3]);
		return NABWA_OK;
	}
	int upload_offsets(int n, const int64_t *ro, const int64_t *qo)
	{
		HIP_CHECK(hipMemcpy(d_ro, ro, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(d_qo, qo, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
		return NABWA_OK;
	}
	int upload(int n, const int64_t *ro, const uint8_t *ref, const int64_t *qo, const uint8_t *qry)
	{
		if (const int r = upload_offsets(n, ro, qo)) return r;
		if (ro[n]) HIP_CHECK(hipMemcpy(d_ref, ref, ro[n], hipMemcpyHostToDevice));
		if (qo[n]) HIP_CHECK(hipMemcpy(d_qry, qry, qo[n], hipMemcpyHostToDevice));
		return NABWA_OK;
	}
	template <class T> T *next() { return buf_i < n_buf ? take<T>(buf_sz[buf_i++]) : nullptr; }
	template <class T> T *take(size_t bytes) { T *p = (T*)((char*)A.base + used); used += up256(bytes); return p; }
};
}

extern "C" void nabwa_dp_scratch_release(int device)
{
	DevArena &A = g_arena[device & 15];
	std::lock_guard<std::mutex> lk(A.mu);
	if (A.base) { (void)hipFree(A.base); A.base = 0; A.cap = 0; }
}

/* ------------------------------------------------------------------ batched aln_global_core */

/* One launch of the global alignment kernel on tasks that are, or are about to be, on the device: the arena is reserved and the offsets
 * uploaded here; `fill` puts the m tasks' sequences at d_ref / d_qry (an upload, or a kernel that writes them there); the kernel is
 * launched; `take` gets the launch's parameters while the arena is still held -- score, n_cigar and the slot-major operations are device
 * memory -- and does what it likes with them.  ro / qo start at 0.  tg (may be null): += set-up, fill, kernel, take seconds. */
int nabwa_dp_global_device(int device, int m, const int64_t *ro, const int64_t *qo, int gap_open, int gap_ext, int gap_end, const int *matrix25,
						   int band, int max_cigar, const std::function<int(const DpDeviceIO&)> &fill,
						   const std::function<int(const DpParams&)> &take, double *tg)
{
	const bool timing = tg != nullptr;
	const double tg0 = now_s();
	int W = 1, H = 1; int64_t maxdiff = 0;
	for (int i = 0; i < m; ++i) {
		const int64_t a1 = ro[i + 1] - ro[i], a2 = qo[i + 1] - qo[i];
		W = std::max<int64_t>(W, a1 + 1);
		H = std::max<int64_t>(H, a2 + 1);
		maxdiff = std::max<int64_t>(maxdiff, a1 > a2 ? a1 - a2 : a2 - a1);
	}
	const size_t waves = (size_t)((m + 255) / 256) * 4;
	DpParams P; memset(&P, 0, sizeof(P));
	ArenaUse A(device);
	if (const int r = A.reserve(m, ro, qo, { waves * 6 * (size_t)W * 64 * 4, waves * (size_t)H * W * 64, waves * (size_t)(W + H) * 64,
											 (size_t)m * 4, (size_t)m * 4, (size_t)m * max_cigar * 4 })) return r;
	P.rows = A.next<int32_t>(); P.tb = A.next<uint8_t>(); P.path = A.next<uint8_t>();
	P.score = A.next<int32_t>(); P.n_cigar = A.next<int32_t>(); P.cigar = A.next<uint32_t>();
	const double tg1 = now_s();
	if (const int r = A.upload_offsets(m, ro, qo)) return r;
	if (const int r = fill(DpDeviceIO{ A.d_ro, A.d_qo, A.d_ref, A.d_qry })) return r;
	P.n = m; P.ref_off = A.d_ro; P.qry_off = A.d_qo; P.ref = A.d_ref; P.qry = A.d_qry;
	P.gap_open = gap_open; P.gap_ext = gap_ext; P.gap_end = gap_end; P.band = band;
	memcpy(P.matrix, matrix25, sizeof(P.matrix));
	P.W = W; P.H = H; P.max_cigar = max_cigar;
	P.wb = (int)std::min<int64_t>(W, 2 * (int64_t)band + maxdiff + 1);
	const double tg2 = now_s();
	nabwa_launch_dp_global(&P, 0);
	HIP_CHECK(hipGetLastError());
	if (timing) HIP_CHECK(hipDeviceSynchronize());
	const double tg3 = now_s();
	if (const int r = take(P)) return r;
	if (tg) { tg[0] += tg1 - tg0; tg[1] += tg2 - tg1; tg[2] += tg3 - tg2; tg[3] += now_s() - tg3; }
	return NABWA_OK;
}

extern "C" int nabwa_global_align(int device, int n, const int64_t *ref_off, const uint8_t *ref, const int64_t *qry_off,
								  const uint8_t *qry, int gap_open, int gap_ext, int gap_end, const int *matrix25, int band,
								  int32_t *score, int32_t *n_cigar, uint32_t *cigar32, int max_cigar)
{
	if (n < 0 || (n && (!ref_off || !qry_off || !ref || !qry || !matrix25 || !score || !n_cigar || !cigar32)) || max_cigar < 1)
		return nabwa_fail(NABWA_EINVAL, "bad argument");
	if (n == 0) return NABWA_OK;
	if (nabwa_device_count() <= device) return nabwa_fail(NABWA_ENODEV, "no such HIP device");
	HIP_CHECK(hipSetDevice(device));
	const int CHUNK = 1 << 16;                     // tasks per launch: bounds the traceback scratch
	const bool timing = getenv("NABWA_TIMING") != 0 && n >= 1024;
	double tg[4] = { 0, 0, 0, 0 };              // set-up, upload, kernel, download
	for (int c0 = 0; c0 < n; c0 += CHUNK) {
		const int m = std::min(CHUNK, n - c0);
		std::vector<int64_t> ro(m + 1), qo(m + 1);
		for (int i = 0; i <= m; ++i) { ro[i] = ref_off[c0 + i] - ref_off[c0]; qo[i] = qry_off[c0 + i] - qry_off[c0]; }
		const int r = nabwa_dp_global_device(device, m, ro.data(), qo.data(), gap_open, gap_ext, gap_end, matrix25, band, max_cigar,
			[&](const DpDeviceIO &D) -> int {
				if (ro[m]) HIP_CHECK(hipMemcpy(D.d_ref, ref + ref_off[c0], ro[m], hipMemcpyHostToDevice));
				if (qo[m]) HIP_CHECK(hipMemcpy(D.d_qry, qry + qry_off[c0], qo[m], hipMemcpyHostToDevice));
				return NABWA_OK;
			},
			[&](const DpParams &P) -> int {
				HIP_CHECK(hipMemcpy(score + c0, P.score, (size_t)m * 4, hipMemcpyDeviceToHost));
				HIP_CHECK(hipMemcpy(n_cigar + c0, P.n_cigar, (size_t)m * 4, hipMemcpyDeviceToHost));
				/* the operations come slot by slot (dp_global_kernel): only the slots in use travel */
				int slots = 0;
				for (int i = 0; i < m; ++i) slots = std::max(slots, std::min(n_cigar[c0 + i], max_cigar));
				if (slots) {
					std::vector<uint32_t> cs((size_t)slots * m);
					HIP_CHECK(hipMemcpy(cs.data(), P.cigar, cs.size() * 4, hipMemcpyDeviceToHost));
					for (int i = 0; i < m; ++i) {
						uint32_t *dst = cigar32 + (size_t)(c0 + i) * max_cigar;
						const int k_n = std::min(n_cigar[c0 + i], max_cigar);
						for (int k = 0; k < k_n; ++k) dst[k] = cs[(size_t)k * m + i];
					}
				}
				return NABWA_OK;
			}, timing ? tg : nullptr);
		if (r != NABWA_OK) return r;
	}
	if (timing) fprintf(stderr, "[nabwa] global_align %d tasks: set-up %.4f s, upload %.4f s, kernel %.4f s, download %.4f s\n", n, tg[0], tg[1], tg[2], tg[3]);
	return NABWA_OK;
}

/* ------------------------------------------------------------------ the path of an extension / local hit */

/* The path behind a score the forward pass found: global alignment of a sub-window of each task with gap_end = -1 and a band that
 * doubles until the search is accepted (stdaln.c:985-1000 for aln_extend_core, :723-735 for aln_local_core).  window(i) gives task
 * i's sub-window as [r0, r1) of its reference and [q0, q1) of its query; accept(i, score, bw) decides from the global score and the
 * band whether task i is done, and if so writes its score; the loop then writes its CIGAR (at most max_cigar operations). */
struct SubWindow { int64_t r0, r1, q0, q1; };
template <class Window, class Accept>
static int band_paths(int device, std::vector<int> act, const int64_t *ref_off, const uint8_t *ref, const int64_t *qry_off, const uint8_t *qry,
					  int gap_open, int gap_ext, const int *matrix25, int band, int32_t *n_cigar, uint32_t *cigar32, int max_cigar,
					  Window window, Accept accept)
{
	for (int bw = band; !act.empty(); bw <<= 1) {
		std::vector<int64_t> ro(act.size() + 1, 0), qo(act.size() + 1, 0); std::vector<uint8_t> rb, qb;
		for (size_t t = 0; t < act.size(); ++t) {
			const int i = act[t]; const SubWindow w = window(i);
			rb.insert(rb.end(), ref + ref_off[i] + w.r0, ref + ref_off[i] + w.r1);
			qb.insert(qb.end(), qry + qry_off[i] + w.q0, qry + qry_off[i] + w.q1);
			ro[t + 1] = (int64_t)rb.size(); qo[t + 1] = (int64_t)qb.size();
		}
		rb.push_back(0); qb.push_back(0);
		std::vector<int32_t> sg(act.size()), nc(act.size()); std::vector<uint32_t> cg(act.size() * (size_t)max_cigar);
		int r = nabwa_global_align(device, (int)act.size(), ro.data(), rb.data(), qo.data(), qb.data(), gap_open, gap_ext, -1,
								   matrix25, bw, sg.data(), nc.data(), cg.data(), max_cigar);
		if (r != NABWA_OK) return r;
		std::vector<int> next;
		for (size_t t = 0; t < act.size(); ++t) {
			const int i = act[t];
			if (accept(i, sg[t], bw)) {
				n_cigar[i] = nc[t];
				memcpy(cigar32 + (size_t)i * max_cigar, cg.data() + t * (size_t)max_cigar, (size_t)std::min(nc[t], max_cigar) * 4);
			} else next.push_back(i);
		}
		act.swap(next);
	}
	return NABWA_OK;
}

/* ------------------------------------------------------------------ batched aln_extend_core */

extern "C" int nabwa_extend_align(int device, int n, const int64_t *ref_off, const uint8_t *ref, const int64_t *qry_off,
								  const uint8_t *qry, int gap_open, int gap_ext, const int *matrix25, int band, const int32_t *G0,
								  int32_t *score, int32_t *n_cigar, uint32_t *cigar32, int max_cigar)
{
	if (n < 0 || (n && (!ref_off || !qry_off || !ref || !qry || !matrix25 || !G0 || !score || !n_cigar || !cigar32)) || max_cigar < 1 || band < 1)
		return nabwa_fail(NABWA_EINVAL, "bad argument");
	if (n == 0) return NABWA_OK;
	if (nabwa_device_count() <= device) return nabwa_fail(NABWA_ENODEV, "no such HIP device");
	HIP_CHECK(hipSetDevice(device));
	/* forward pass on the GPU */
	int W = 2;
	for (int i = 0; i < n; ++i) W = std::max<int64_t>(W, ref_off[i + 1] - ref_off[i] + 2);
	std::vector<int32_t> fs(n), ei(n), ej(n);
	{
		ExtParams P; memset(&P, 0, sizeof(P));
		ArenaUse A(device);
		if (const int r = A.reserve(n, ref_off, qry_off, { (size_t)n * 4, nabwa_dp_local_fits_lds(W) ? 256 : (size_t)n * nabwa_dp_local_rows_bytes(W),
														   (size_t)n * 4, (size_t)n * 4, (size_t)n * 4 })) return r;
		int32_t *d_g0 = A.next<int32_t>();
		P.eh = A.next<uint32_t>(); P.score = A.next<int32_t>(); P.end_i = A.next<int32_t>(); P.end_j = A.next<int32_t>();
		if (const int r = A.upload(n, ref_off, ref, qry_off, qry)) return r;
		HIP_CHECK(hipMemcpy(d_g0, G0, (size_t)n * 4, hipMemcpyHostToDevice));
		P.n = n; P.ref_off = A.d_ro; P.qry_off = A.d_qo; P.ref = A.d_ref; P.qry = A.d_qry; P.g0 = d_g0;
		P.gap_open = gap_open; P.gap_ext = gap_ext; P.band = band; memcpy(P.matrix, matrix25, sizeof(P.matrix)); P.W = W;
		nabwa_launch_dp_extend_fwd(&P, 0);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpy(fs.data(), P.score, (size_t)n * 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(ei.data(), P.end_i, (size_t)n * 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(ej.data(), P.end_j, (size_t)n * 4, hipMemcpyDeviceToHost));
	}
	/* path: the two prefixes up to the end of the best extension */
	std::vector<int> act;
	for (int i = 0; i < n; ++i) { score[i] = fs[i]; n_cigar[i] = 0; if (fs[i] > 0) act.push_back(i); }
	return band_paths(device, std::move(act), ref_off, ref, qry_off, qry, gap_open, gap_ext, matrix25, band, n_cigar, cigar32, max_cigar,
					  [&](int i) { return SubWindow{ 0, ei[i], 0, ej[i] }; },
					  [&](int i, int32_t sg, int bw) {
						  if (sg != fs[i] && bw <= std::max(ei[i], ej[i])) return false;
						  score[i] = sg;
						  return true;
					  });
}

/* ------------------------------------------------------------------ batched aln_local_core */

extern "C" int nabwa_local_align(int device, int n, const int64_t *ref_off, const uint8_t *ref, const int64_t *qry_off,
								 const uint8_t *qry, int gap_open, int gap_ext, const int *matrix25, int band, int thres,
								 int32_t *score, int32_t *coords /* n x 4: start_i,start_j,end_i,end_j (1-based) */, int32_t *subo,
								 int32_t *n_cigar, uint32_t *cigar32, int max_cigar)
{
	if (n < 0 || (n && (!ref_off || !qry_off || !ref || !qry || !matrix25 || !score || !coords || !n_cigar || !cigar32)) || max_cigar < 1 || band < 1 || thres < 1)
		return nabwa_fail(NABWA_EINVAL, "bad argument");
	if (n == 0) return NABWA_OK;
	if (nabwa_device_count() <= device) return nabwa_fail(NABWA_ENODEV, "no such HIP device");
	HIP_CHECK(hipSetDevice(device));
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double tl0 = now_s();
	double tl1 = 0, tl2 = 0, tl3 = 0;
	int W = 2, H = 2, max_score = 0;
	for (int i = 0; i < n; ++i) { W = std::max<int64_t>(W, ref_off[i + 1] - ref_off[i] + 2); H = std::max<int64_t>(H, qry_off[i + 1] - qry_off[i] + 1); }
	for (int i = 0; i < 25; ++i) max_score = std::max(max_score, matrix25[i]);
	std::vector<int32_t> o((size_t)n * 6), sub((size_t)n * H);
	{
		LocParams P; memset(&P, 0, sizeof(P));
		ArenaUse A(device);
		if (const int r = A.reserve(n, ref_off, qry_off, { nabwa_dp_local_fits_lds(W) ? 256 : (size_t)n * nabwa_dp_local_rows_bytes(W),
														   (size_t)n * H * 4, (size_t)n * 24 })) return r;
		P.eh = A.next<int32_t>(); P.suba = A.next<int32_t>(); P.out = A.next<int32_t>();
		if (const int r = A.upload(n, ref_off, ref, qry_off, qry)) return r;
		P.n = n; P.ref_off = A.d_ro; P.qry_off = A.d_qo; P.ref = A.d_ref; P.qry = A.d_qry;
		P.gap_open = gap_open; P.gap_ext = gap_ext; P.thres = thres; memcpy(P.matrix, matrix25, 100); P.max_score = max_score; P.W = W; P.H = H;
		P.row_forward = getenv("NABWA_DP_FORWARD") && !strcmp(getenv("NABWA_DP_FORWARD"), "rows");
		tl1 = now_s();
		nabwa_launch_dp_local(&P, 0);
		HIP_CHECK(hipGetLastError());
		if (timing) { HIP_CHECK(hipDeviceSynchronize()); tl2 = now_s(); }
		HIP_CHECK(hipMemcpy(o.data(), P.out, (size_t)n * 24, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(sub.data(), P.suba, (size_t)n * H * 4, hipMemcpyDeviceToHost));
	}
	tl3 = now_s();
	std::vector<int> act;
	for (int i = 0; i < n; ++i) {
		const int32_t *v = &o[(size_t)i * 6];
		const int l2 = (int)(qry_off[i + 1] - qry_off[i]);
		score[i] = v[0]; n_cigar[i] = 0;
		coords[4 * i] = v[2]; coords[4 * i + 1] = v[3]; coords[4 * i + 2] = v[4]; coords[4 * i + 3] = v[5];
		if (subo) subo[i] = 0;
		if (l2 == 0 || ref_off[i + 1] == ref_off[i]) { score[i] = -1; continue; }
		if (v[0] < thres || v[4] == 0 || v[5] == 0) continue;
		if (subo) {                                             /* stdaln.c:700-709 */
			int tmp2 = 0, tmp = (int)(v[3] - .33 * (v[5] - v[3]) + .499);
			const int32_t *sa = &sub[(size_t)i * H];
			for (int j = 1; j <= tmp; ++j) if (tmp2 < sa[j]) tmp2 = sa[j];
			tmp = (int)(v[5] + .33 * (v[5] - v[3]) + .499);
			for (int j = tmp; j <= l2; ++j) if (tmp2 < sa[j]) tmp2 = sa[j];
			subo[i] = tmp2;
		}
		act.push_back(i);
	}
	/* path: the sub-matrix between the start and the end of the local hit (1-based, inclusive) */
	const int r = band_paths(device, std::move(act), ref_off, ref, qry_off, qry, gap_open, gap_ext, matrix25, band, n_cigar, cigar32, max_cigar,
							 [&](int i) { const int32_t *v = &o[(size_t)i * 6]; return SubWindow{ v[2] - 1, v[4], v[3] - 1, v[5] }; },
							 [&](int i, int32_t sg, int bw) {
								 const int32_t *v = &o[(size_t)i * 6];
								 if (sg != v[1] && sg != v[0] && bw <= std::max(v[4] - v[2], v[5] - v[3]) + 1) return false;
								 score[i] = (v[1] > sg && v[0] > sg) ? -1 : sg;     /* "potential bug" branch, stdaln.c:737-740 */
								 return true;
							 });
	if (r != NABWA_OK) return r;
	if (timing) fprintf(stderr, "[nabwa] local_align %d tasks (window %d x %d): set-up + upload %.4f s, kernel %.4f s, download %.4f s, paths (global alignments) %.4f s\n", n, W, H, tl1 - tl0, tl2 - tl1, tl3 - tl2, now_s() - tl3);
	return NABWA_OK;
}
