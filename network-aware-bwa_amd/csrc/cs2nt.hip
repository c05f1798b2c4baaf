// cs2nt.hip -- colour space: an aligned colour read becomes a nucleotide read with nucleotide qualities (cs2nt.c), on the GPU.
//
// What the reference does per mapped read in bwa_refine_gapped's colour branch (bwase.c:383-402, cs2nt.c:112-191):
//   bwa_cs2nt_core : nt_ref[] along the colour CIGAR from the nucleotide pac, cs_read[] = colour << 6 | quality,
//                    cs2nt_DP (4 states per position, :36-77), cs2nt_nt_qual (:83-109), then seq / rseq / qual rewritten
// Here: one read per lane.  The recurrence is serial along the read (16 adds, 4 four-way minima per position), so the
// parallelism is across reads; a position's four back-pointers are one byte in a position-major plane (lanes write
// neighbouring bytes), the traceback turns that plane into nt_read[] in place, and the quality pass reads it back.
//   cs2nt_prep_kernel   : record form only -- walks the CIGAR, fetches nt_ref from the nucleotide pac in HBM, builds cs_read
//   cs2nt_core_kernel   : cs2nt_DP + cs2nt_nt_qual; inputs row-major (the flat entry) or position-major (the record form)
//   cs2nt_finish_kernel : record form only -- the decoded read as bwa_seq_t.seq / .rseq / .qual hold it afterwards
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/nabwa.h"
#include "nabwa_internal.hpp"
#include "dev_pool.hpp"
#include "finish_common.hpp"

#define CS_COLOR_MM 19          /* cs2nt.c:24-25 */
#define CS_NUCL_MM  25

namespace {

/* one mapped record for the record form */
struct CsRec { uint32_t pos; int32_t len, strand, n_cigar; int64_t off, cig; };

/* the best predecessor y of state x (first minimum, strict <, cs2nt.c:54-62): nst_ntnt2cs_table[1 << x | 1 << y] is x ^ y for bases 0-3 */
__device__ __forceinline__ int cs_step(const int h[4], int x, int col, int pen, int *best)
{
	int mn = h[0] + ((x ^ 0) != col ? pen : 0), ym = 0;
#pragma unroll
	for (int y = 1; y < 4; ++y) {
		const int s = h[y] + ((x ^ y) != col ? pen : 0);
		if (s < mn) { mn = s; ym = y; }
	}
	*best = mn;
	return ym;
}

/* PM = 0: case i has cs_read at off[i] (size = off[i + 1] - off[i]), nt_ref at off[i] + i, its result at off[i] - i, all row-major.
 * PM = 1: case i has size[i]; element k of nt_ref / cs_read / the result is at k * n + i.
 * bt: (max_size + 1) * n bytes, position-major in both forms. */
template <int PM>
__global__ __launch_bounds__(256) void cs2nt_core_kernel(int n, const int64_t *__restrict__ off, const int32_t *__restrict__ size_pm,
														  const uint8_t *__restrict__ nt_ref, const uint8_t *__restrict__ cs,
														  uint8_t *__restrict__ bt, uint8_t *__restrict__ out)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	int size; int64_t rb, cb, ob, st;
	if (PM) { size = size_pm[i]; rb = cb = ob = i; st = n; }
	else { size = (int)(off[i + 1] - off[i]); rb = off[i] + i; cb = off[i]; ob = off[i] - i; st = 1; }
	if (size < 1) return;
	int h[4];
	{
		const int r0 = nt_ref[rb];
#pragma unroll
		for (int x = 0; x < 4; ++x) h[x] = r0 >= 4 ? 0 : (x == r0 ? 0 : CS_NUCL_MM);
	}
	for (int k = 1; k <= size; ++k) {
		const int c = cs[cb + (int64_t)(k - 1) * st], q = c & 0x3f, col = c >> 6;
		const int pen = q == 63 ? 0 : (q < CS_COLOR_MM ? CS_COLOR_MM : q);
		const int r = nt_ref[rb + (int64_t)k * st];
		int g[4], b = 0;
#pragma unroll
		for (int x = 0; x < 4; ++x) {
			/* the nucleotide mismatch is the same for every y: it does not move the minimum */
			b |= cs_step(h, x, col, pen, &g[x]) << (2 * x);
			if (r < 4 && r != x) g[x] += CS_NUCL_MM;
		}
#pragma unroll
		for (int x = 0; x < 4; ++x) h[x] = g[x];
		bt[(int64_t)k * n + i] = (uint8_t)b;
	}
	int cur = 0;
	{
		int hm = h[0];
#pragma unroll
		for (int x = 1; x < 4; ++x) if (h[x] < hm) { hm = h[x]; cur = x; }
	}
	/* traceback: the plane holds nt_read[k] afterwards */
	for (int k = size; k >= 1; --k) {
		const int b = bt[(int64_t)k * n + i];
		bt[(int64_t)k * n + i] = (uint8_t)cur;
		cur = b >> (2 * cur) & 3;
	}
	bt[i] = (uint8_t)cur;
	/* cs2nt_nt_qual (cs2nt.c:83-109) */
	int n0 = cur, n1 = bt[(int64_t)n + i], c0 = cs[cb];
	for (int k = 1; k < size; ++k) {
		const int n2 = bt[(int64_t)(k + 1) * n + i], c1 = cs[cb + (int64_t)k * st];
		const int qa = c0 & 0x3f, qb = c1 & 0x3f;
		const bool m0 = (n0 ^ n1) == (c0 >> 6), m1 = (n1 ^ n2) == (c1 >> 6);
		int q = 0;
		if (m0 && m1) q = qa + qb + 10;
		else if (m0) q = qa - qb;
		else if (m1) q = qb - qa;
		q = q < 0 ? 0 : (q > 60 ? 60 : q);
		out[ob + (int64_t)(k - 1) * st] = (qa == 63 || qb == 63) ? 0 : (uint8_t)(n1 << 6 | q);
		n0 = n1; n1 = n2; c0 = c1;
	}
}

/* bwa_cs2nt_core up to the DP (cs2nt.c:128-166).  seq is bwa_seq_t.seq as the library holds it (the read reversed), so the read in
 * alignment orientation is seq backwards on the forward strand and rseq as it is on the reverse strand. */
__global__ __launch_bounds__(256) void cs2nt_prep_kernel(int nm, int cap, const CsRec *__restrict__ rec, const uint16_t *__restrict__ cigar,
														  const uint8_t *__restrict__ seq, const uint8_t *__restrict__ rseq,
														  const uint8_t *__restrict__ qual, const uint8_t *__restrict__ pac, int64_t l_pac,
														  uint8_t *__restrict__ nt_ref, uint8_t *__restrict__ cs, int32_t *__restrict__ size)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nm) return;
	const CsRec R = rec[i];
	/* (a hit of the chains lies inside the text -- pos + len <= l_pac, and a refined CIGAR comes from a window cut at l_pac --, so the
	 * bound is never met there; the reference has none and would read past its array, here such a base is 0) */
	auto base = [&](int64_t x) -> int { return x >= 0 && x < l_pac ? pac[x >> 2] >> ((~x & 3) << 1) & 3 : 0; };
	auto colour = [&](int y) -> int {
		const int c = R.strand ? rseq[R.off + y] : seq[R.off + R.len - 1 - y];
		int q = (int)qual[R.off + (R.strand ? R.len - 1 - y : y)] - 33;
		if (q > 60) q = 60;
		if (c > 3) q = 63;
		return (c << 6 | q) & 0xff;
	};
	nt_ref[i] = R.pos ? (uint8_t)base((int64_t)R.pos - 1) : 4;
	int z = 0;
	if (R.n_cigar == 0) {
		for (; z < R.len && z < cap; ++z) {
			cs[(int64_t)z * nm + i] = (uint8_t)colour(z);
			nt_ref[(int64_t)(z + 1) * nm + i] = (uint8_t)base((int64_t)R.pos + z);
		}
	} else {
		int64_t x = R.pos; int y = 0;
		for (int k = 0; k < R.n_cigar; ++k) {
			const int c = cigar[R.cig + k], l = c & 0x3fff, op = c >> 14;
			if (op == 0 || op == 1) {
				for (int t = 0; t < l && y < R.len && z < cap; ++t, ++y, ++z) {
					cs[(int64_t)z * nm + i] = (uint8_t)colour(y);
					nt_ref[(int64_t)(z + 1) * nm + i] = op == 0 ? (uint8_t)base(x++) : 4;
				}
			} else if (op == 3) y += l;
			else x += l;
		}
	}
	size[i] = z;
}

/* cs2nt.c:172-189: seq_out = the decoded read reversed (bwa_seq_t.seq as the library holds it), rseq_out = its reverse complement,
 * qual_out = its qualities + 33 in the read's own orientation; size - 1 bytes each from off on */
__global__ __launch_bounds__(256) void cs2nt_finish_kernel(int nm, const CsRec *__restrict__ rec, const int32_t *__restrict__ size,
															const uint8_t *__restrict__ dec, uint8_t *__restrict__ seq_out,
															uint8_t *__restrict__ rseq_out, uint8_t *__restrict__ qual_out)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nm) return;
	const CsRec R = rec[i];
	const int L = size[i] - 1;
	for (int k = 0; k < L; ++k) {
		const int v = dec[(int64_t)k * nm + i], b = v >> 6, q = (v & 0x3f) + 33;      /* position k in alignment orientation */
		if (R.strand) {
			rseq_out[R.off + k] = (uint8_t)b; seq_out[R.off + k] = (uint8_t)(3 - b); qual_out[R.off + L - 1 - k] = (uint8_t)q;
		} else {
			seq_out[R.off + L - 1 - k] = (uint8_t)b; rseq_out[R.off + L - 1 - k] = (uint8_t)(3 - b); qual_out[R.off + k] = (uint8_t)q;
		}
	}
}

}

/* ------------------------------------------------------------------ the flat entry */

extern "C" int nabwa_cs2nt(int device, int n, const int64_t *off, const uint8_t *nt_ref, const uint8_t *cs_read, uint8_t *out)
{
	if (n < 0 || (n && (!off || !nt_ref || !cs_read || !out))) return nabwa_fail(NABWA_EINVAL, "bad argument");
	if (n == 0) return NABWA_OK;
	int64_t max_size = 0;
	for (int i = 0; i < n; ++i) {
		const int64_t s = off[i + 1] - off[i];
		if (s < 1 || s > NABWA_CS2NT_MAX) return nabwa_fail(NABWA_EINVAL, "a case's size is outside 1..NABWA_CS2NT_MAX");
		max_size = std::max(max_size, s);
	}
	if (off[0] != 0) return nabwa_fail(NABWA_EINVAL, "off[0] must be 0");
	if (nabwa_device_count() <= device) return nabwa_fail(NABWA_ENODEV, "no such HIP device");
	HIP_CHECK(hipSetDevice(device));
	const size_t tot = (size_t)off[n];
	DevBuf d_off, d_ref, d_cs, d_bt, d_out;
	if (int r = d_off.get((size_t)(n + 1) * 8)) return r;
	if (int r = d_ref.get(tot + (size_t)n)) return r;
	if (int r = d_cs.get(tot)) return r;
	if (int r = d_bt.get((size_t)(max_size + 1) * (size_t)n)) return r;
	if (int r = d_out.get(tot)) return r;
	HIP_CHECK(hipMemcpy(d_off.p, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
	HIP_CHECK(hipMemcpy(d_ref.p, nt_ref, tot + (size_t)n, hipMemcpyHostToDevice));
	HIP_CHECK(hipMemcpy(d_cs.p, cs_read, tot, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(cs2nt_core_kernel<0>, dim3((n + 255) / 256), dim3(256), 0, 0, n, d_off.as<int64_t>(), (const int32_t*)nullptr,
					   d_ref.as<uint8_t>(), d_cs.as<uint8_t>(), d_bt.as<uint8_t>(), d_out.as<uint8_t>());
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipDeviceSynchronize());
	if (tot > (size_t)n) HIP_CHECK(hipMemcpy(out, d_out.p, tot - (size_t)n, hipMemcpyDeviceToHost));
	return NABWA_OK;
}

/* ------------------------------------------------------------------ the nucleotide reference of a colour index */

extern "C" int nabwa_index_attach_nt_reference(nabwa_index_t *ix, const char *prefix)
{
	if (!ix || !prefix) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (!ix->ref) return nabwa_fail(NABWA_EINVAL, "index has no reference attached (nabwa_index_attach_reference)");
	nabwa_reference *N = nullptr;
	const std::string p = std::string(prefix) + ".nt";
	if (int r = nabwa_reference_read(p.c_str(), &N)) return r;
	if (N->l_pac != ix->ref->l_pac) { delete N; return nabwa_fail(NABWA_EIO, "%s.nt.ann and the colour .ann disagree about the reference's length", prefix); }
	/* coordinates, names and ambiguity holes stay those of the colour annotations (bwa_cal_md1 gets bns, not ntbns): only the bases differ */
	nabwa_reference *R = new nabwa_reference();
	R->l_pac = ix->ref->l_pac; R->seed = ix->ref->seed; R->anns = ix->ref->anns; R->holes = ix->ref->holes;
	R->pac.swap(N->pac);
	delete N;
	if (nabwa_device_count() <= ix->device) { delete R; return nabwa_fail(NABWA_ENODEV, "no such HIP device"); }
	hipError_t e = hipSetDevice(ix->device);
	uint8_t *d = nullptr;
	if (e == hipSuccess) e = hipMalloc((void**)&d, R->pac.size());
	if (e == hipSuccess) e = hipMemcpy(d, R->pac.data(), R->pac.size(), hipMemcpyHostToDevice);
	if (e != hipSuccess) { if (d) (void)hipFree(d); delete R; return nabwa_hip_fail(e, "uploading the nucleotide pac", __FILE__, __LINE__); }
	nabwa_finish_drop_reference(ix);      /* the device path's hole table goes with the bases it was made for (finish_gpu.hip) */
	if (ix->d_ntpac) { (void)hipFree(ix->d_ntpac); ix->bytes -= ix->ntpac_bytes; }
	delete ix->ref_nt;
	ix->ref_nt = R; ix->d_ntpac = d; ix->ntpac_bytes = R->pac.size(); ix->bytes += ix->ntpac_bytes;
	return NABWA_OK;
}

/* ------------------------------------------------------------------ the record form */

int nabwa_cs2nt_records(nabwa_index_t *ix, void *base, size_t stride, int n, const int64_t *off, const uint8_t *seq, const uint8_t *rseq,
						const uint8_t *qual, uint8_t *nt_seq, uint8_t *nt_rseq, uint8_t *nt_qual, double *times)
{
	if (!ix->ref_nt || !ix->d_ntpac) return nabwa_fail(NABWA_EINVAL, "index has no nucleotide reference attached (nabwa_index_attach_nt_reference)");
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double t0 = now_s();
	std::vector<CsRec> rec; std::vector<int> which; std::vector<uint16_t> cig;
	int cap = 0;
	for (int i = 0; i < n; ++i) {
		const nabwa_se_t &s = *rec_at(base, stride, i);
		if (s.type == 0) continue;
		if ((int64_t)s.len != off[i + 1] - off[i]) return nabwa_fail(NABWA_EINVAL, "a record's len disagrees with its read");
		if (s.len < 1 || s.len > NABWA_CS2NT_MAX) return nabwa_fail(NABWA_ECAP, "a colour read is longer than NABWA_CS2NT_MAX");
		rec.push_back({ s.pos, s.len, s.strand, s.n_cigar, off[i], (int64_t)cig.size() });
		cig.insert(cig.end(), s.cigar, s.cigar + s.n_cigar);
		which.push_back(i);
		cap = std::max(cap, s.len);
	}
	const int nm = (int)rec.size();
	if (nm == 0) return NABWA_OK;
	HIP_CHECK(hipSetDevice(ix->device));
	const size_t tot = (size_t)off[n], plane = (size_t)(cap + 1) * (size_t)nm;
	DevBuf d_rec, d_cig, d_seq, d_rseq, d_qual, d_ref, d_cs, d_bt, d_dec, d_size, d_oseq, d_orseq, d_oqual;
	if (int r = d_rec.get((size_t)nm * sizeof(CsRec))) return r;
	if (int r = d_cig.get(cig.size() * 2)) return r;
	if (int r = d_seq.get(tot)) return r;
	if (int r = d_rseq.get(tot)) return r;
	if (int r = d_qual.get(tot)) return r;
	if (int r = d_ref.get(plane)) return r;
	if (int r = d_cs.get(plane)) return r;
	if (int r = d_bt.get(plane)) return r;
	if (int r = d_dec.get(plane)) return r;
	if (int r = d_size.get((size_t)nm * 4)) return r;
	if (int r = d_oseq.get(tot)) return r;
	if (int r = d_orseq.get(tot)) return r;
	if (int r = d_oqual.get(tot)) return r;
	HIP_CHECK(hipMemcpy(d_rec.p, rec.data(), (size_t)nm * sizeof(CsRec), hipMemcpyHostToDevice));
	if (!cig.empty()) HIP_CHECK(hipMemcpy(d_cig.p, cig.data(), cig.size() * 2, hipMemcpyHostToDevice));
	HIP_CHECK(hipMemcpy(d_seq.p, seq, tot, hipMemcpyHostToDevice));
	HIP_CHECK(hipMemcpy(d_rseq.p, rseq, tot, hipMemcpyHostToDevice));
	HIP_CHECK(hipMemcpy(d_qual.p, qual, tot, hipMemcpyHostToDevice));
	/* (the bytes of reads that stay unmapped, and those behind a decoded read, come back as 0) */
	HIP_CHECK(hipMemset(d_oseq.p, 0, tot));
	HIP_CHECK(hipMemset(d_orseq.p, 0, tot));
	HIP_CHECK(hipMemset(d_oqual.p, 0, tot));
	DevEvent ev_a, ev_b;
	HIP_CHECK(hipEventCreate(&ev_a.e)); HIP_CHECK(hipEventCreate(&ev_b.e));
	const dim3 grid((nm + 255) / 256), block(256);
	const double t1 = now_s();
	HIP_CHECK(hipEventRecord(ev_a, 0));
	hipLaunchKernelGGL(cs2nt_prep_kernel, grid, block, 0, 0, nm, cap, d_rec.as<CsRec>(), d_cig.as<uint16_t>(), d_seq.as<uint8_t>(), d_rseq.as<uint8_t>(),
					   d_qual.as<uint8_t>(), ix->d_ntpac, (int64_t)ix->ref_nt->l_pac, d_ref.as<uint8_t>(), d_cs.as<uint8_t>(), d_size.as<int32_t>());
	hipLaunchKernelGGL(cs2nt_core_kernel<1>, grid, block, 0, 0, nm, (const int64_t*)nullptr, d_size.as<int32_t>(), d_ref.as<uint8_t>(), d_cs.as<uint8_t>(),
					   d_bt.as<uint8_t>(), d_dec.as<uint8_t>());
	hipLaunchKernelGGL(cs2nt_finish_kernel, grid, block, 0, 0, nm, d_rec.as<CsRec>(), d_size.as<int32_t>(), d_dec.as<uint8_t>(), d_oseq.as<uint8_t>(),
					   d_orseq.as<uint8_t>(), d_oqual.as<uint8_t>());
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(ev_b, 0));
	HIP_CHECK(hipEventSynchronize(ev_b));
	float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ev_a, ev_b));
	const double t2 = now_s();
	std::vector<int32_t> size((size_t)nm);
	HIP_CHECK(hipMemcpy(size.data(), d_size.p, (size_t)nm * 4, hipMemcpyDeviceToHost));
	HIP_CHECK(hipMemcpy(nt_seq, d_oseq.p, tot, hipMemcpyDeviceToHost));
	HIP_CHECK(hipMemcpy(nt_rseq, d_orseq.p, tot, hipMemcpyDeviceToHost));
	HIP_CHECK(hipMemcpy(nt_qual, d_oqual.p, tot, hipMemcpyDeviceToHost));
	for (int t = 0; t < nm; ++t) {
		nabwa_se_t &s = *rec_at(base, stride, which[t]);
		if (size[t] < 1) return nabwa_fail(NABWA_EINVAL, "a colour CIGAR consumes no colour of its read");
		s.len = s.full_len = size[t] - 1;                            /* cs2nt.c:172 */
	}
	if (times) { times[0] += now_s() - t0; times[1] += (double)ms; }
	if (timing) fprintf(stderr, "[nabwa] cs2nt %d of %d reads: records + upload %.3f s, kernels %.3f ms, download %.3f s\n", nm, n, t1 - t0, (double)ms, now_s() - t2);
	return NABWA_OK;
}

/* ------------------------------------------------------------------ the single-end colour chain */

/* MD / NM on the nucleotide pac with the decoded read, then the flags (bwase.c:404-414; no bwa_correct_trimmed, :418-419) */
static int cs_md_flags(nabwa_index_t *ix, nabwa_se_t *out, int n, const int64_t *off, const uint8_t *nt_seq, const uint8_t *nt_rseq, FinGpu *gpu)
{
	const nabwa_reference *R = ix->ref, *Rn = ix->ref_nt;
	int md_over = 0;
	if (gpu && n) if (const int r = gpu->md_records(1, out, sizeof(nabwa_se_t), n, off)) return r;       /* NABWA_FINISH=gpu: MD / NM on the device */
	host_parallel(host_threads((size_t)n, 4096), (size_t)n, [&](int, size_t lo, size_t hi) {
		std::vector<uint8_t> fwd;
		for (size_t i = lo; i < hi; ++i) {
			nabwa_se_t &s = out[i];
			if (s.type == 0) { s.flag = 4; continue; }
			if (gpu ? !gpu->take_md((int)i, s) : !md_and_trim(Rn, s, nt_seq + off[i], nt_rseq + off[i], fwd)) md_over = 1;      /* len == full_len: nothing is trimmed */
			se_flags(R, s);
		}
	});
	if (md_over) return nabwa_fail(NABWA_ECAP, "MD string longer than NABWA_MAX_MD");
	return NABWA_OK;
}

extern "C" int nabwa_se_finish_cs(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const uint8_t *seq,
								  const uint8_t *rseq, const uint8_t *qual, const int32_t *full_len, const int32_t *n_aln,
								  const nabwa_aln1_t *aln, int n_occ, uint64_t *rng48, nabwa_se_t *out, uint8_t *nt_seq, uint8_t *nt_rseq,
								  uint8_t *nt_qual, double *times)
{
	if (!ix || !opt || !rng48 || n < 0 || (n && (!off || !seq || !rseq || !qual || !n_aln || !out || !nt_seq || !nt_rseq || !nt_qual)))
		return nabwa_fail(NABWA_EINVAL, "null argument");
	if (opt->mode & NABWA_MODE_COMPREAD) return nabwa_fail(NABWA_EINVAL, "the option block is a nucleotide one (BWA_MODE_COMPREAD): use nabwa_se_finish");
	if (!ix->ref) return nabwa_fail(NABWA_EINVAL, "index has no reference attached (nabwa_index_attach_reference)");
	if (!ix->ref_nt) return nabwa_fail(NABWA_EINVAL, "index has no nucleotide reference attached (nabwa_index_attach_nt_reference)");
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double t0 = now_s();
	int r = nabwa_se_posn(ix, opt, n, off, full_len, n_aln, aln, n_occ, rng48, out);
	if (r != NABWA_OK) return r;
	const double t1 = now_s();
	size_t j1 = 0, j2 = 0;
	/* NABWA_FINISH=gpu: windows, CIGAR rules and MD / NM on the device (finish_gpu.hip): the colour reads for the first refinement,
	 * the decoded reads for the second and for MD / NM */
	const int fin_mode = nabwa_finish_mode();
	if (fin_mode < 0) return nabwa_fail(NABWA_EINVAL, "NABWA_FINISH: host or gpu");
	std::unique_ptr<FinGpu> gpu;
	if (fin_mode == 1) {
		nabwa_finish_count_chain_call();
		gpu.reset(new FinGpu(ix));
		if (n && (r = gpu->set_reads(off[n], seq, rseq)) != NABWA_OK) return r;
	}
	if ((r = refine_batch(ix, out, sizeof(nabwa_se_t), n, off, seq, rseq, &j1, nullptr, gpu.get())) != NABWA_OK) return r;
	const double t2 = now_s();
	if ((r = nabwa_cs2nt_records(ix, out, sizeof(nabwa_se_t), n, off, seq, rseq, qual, nt_seq, nt_rseq, nt_qual, times)) != NABWA_OK) return r;
	const double t3 = now_s();
	if (gpu && n && (r = gpu->set_reads(off[n], nt_seq, nt_rseq)) != NABWA_OK) return r;
	if ((r = refine_batch(ix, out, sizeof(nabwa_se_t), n, off, nt_seq, nt_rseq, &j2, ix->ref_nt, gpu.get())) != NABWA_OK) return r;
	const double t4 = now_s();
	if ((r = cs_md_flags(ix, out, n, off, nt_seq, nt_rseq, gpu.get())) != NABWA_OK) return r;
	if (gpu) gpu->report("se_finish_cs");
	if (timing) fprintf(stderr, "[nabwa] se_finish_cs %d reads: posn %.3f s, colour refinement (%zu jobs) %.3f s, decode %.3f s, "
						"nucleotide refinement (%zu jobs) %.3f s, md/flags %.3f s\n", n, t1 - t0, j1, t2 - t1, t3 - t2, j2, t4 - t3, now_s() - t4);
	return NABWA_OK;
}
