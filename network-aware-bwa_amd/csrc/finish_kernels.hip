// finish_kernels.hip -- the kernels of the finishing chains' device path (NABWA_FINISH=gpu; nabwa_refine_gapped_core, nabwa_cal_md):
// the bodies of finish_body.hpp, one wavefront per job or record (four to a workgroup), the CIGAR rules one job per lane.
#include <hip/hip_runtime.h>
#include "finish_body.hpp"
#include "launchers.hpp"

#define FIN_WAVES 4       /* wavefronts of a workgroup; they share nothing */

__global__ __launch_bounds__(64 * FIN_WAVES) void refine_window_kernel(const uint8_t *pac, const FinJob *jobs, int n, const uint8_t *reads0,
																		 const uint8_t *reads1, const int64_t *ro, const int64_t *qo, uint8_t *ref, uint8_t *qry)
{
	const int t = (int)(blockIdx.x * FIN_WAVES + (threadIdx.x >> 6));
	if (t >= n) return;
	const FinJob J = jobs[t];
	fin_window_wave(pac, J, reads0, reads1, ref + ro[t], qry + qo[t]);
}

__global__ __launch_bounds__(256) void refine_cigar_kernel(const FinJob *jobs, int n, int end_correct, const int32_t *n_c32, const uint32_t *c32,
															int max_cigar, uint32_t *pos_out, int32_t *n_cigar, uint16_t *rows, unsigned int *n_bad)
{
	const int t = (int)(blockIdx.x * 256 + threadIdx.x);
	if (t >= n) return;
	uint32_t p = (uint32_t)jobs[t].pos;
	const int m = fin_cigar_job(c32 + t, (size_t)n, n_c32[t], max_cigar, jobs[t].ext, end_correct, jobs[t].pos, rows + (size_t)t * max_cigar, &p);
	pos_out[t] = p; n_cigar[t] = m < 0 ? 0 : m;
	if (m < 0) atomicAdd(n_bad, 1u);
}

/* WRITE = false: len_out[t] = the string's length without its NUL, nm[t]; WRITE = true: the string at md + md_off[t], NUL-terminated */
template <bool WRITE>
__global__ __launch_bounds__(64 * FIN_WAVES) void md_kernel(const FinRef R, const FinRec *recs, int n, const uint8_t *reads0, const uint8_t *reads1,
															  const uint16_t *cigar, int32_t *nm, int32_t *len_out, const int64_t *md_off, char *md)
{
	const int t = (int)(blockIdx.x * FIN_WAVES + (threadIdx.x >> 6));
	if (t >= n) return;
	const FinRec Q = recs[t];
	int32_t nm_t = 0;
	const uint32_t o = fin_md_wave<WRITE>(R, Q, reads0, reads1, cigar + Q.cig_off, WRITE ? md + md_off[t] : nullptr, &nm_t);
	if (!WRITE && (threadIdx.x & 63u) == 0) { nm[t] = nm_t; len_out[t] = (int32_t)o; }
}

extern "C" {
void nabwa_launch_refine_window(const uint8_t *pac, const FinJob *jobs, int n, const uint8_t *reads0, const uint8_t *reads1, const int64_t *ro,
								const int64_t *qo, uint8_t *ref, uint8_t *qry, hipStream_t s)
{
	if (n > 0) hipLaunchKernelGGL(refine_window_kernel, dim3((n + FIN_WAVES - 1) / FIN_WAVES), dim3(64 * FIN_WAVES), 0, s, pac, jobs, n, reads0, reads1, ro, qo, ref, qry);
}
void nabwa_launch_refine_cigar(const FinJob *jobs, int n, int end_correct, const int32_t *n_c32, const uint32_t *c32, int max_cigar,
							   uint32_t *pos_out, int32_t *n_cigar, uint16_t *rows, unsigned int *n_bad, hipStream_t s)
{
	if (n > 0) hipLaunchKernelGGL(refine_cigar_kernel, dim3((n + 255) / 256), dim3(256), 0, s, jobs, n, end_correct, n_c32, c32, max_cigar, pos_out, n_cigar, rows, n_bad);
}
void nabwa_launch_md_count(const FinRef *R, const FinRec *recs, int n, const uint8_t *reads0, const uint8_t *reads1, const uint16_t *cigar,
						   int32_t *nm, int32_t *len_out, hipStream_t s)
{
	if (n > 0) hipLaunchKernelGGL(md_kernel<false>, dim3((n + FIN_WAVES - 1) / FIN_WAVES), dim3(64 * FIN_WAVES), 0, s, *R, recs, n, reads0, reads1, cigar, nm, len_out,
								  (const int64_t*)nullptr, (char*)nullptr);
}
void nabwa_launch_md_write(const FinRef *R, const FinRec *recs, int n, const uint8_t *reads0, const uint8_t *reads1, const uint16_t *cigar,
						   const int64_t *md_off, char *md, hipStream_t s)
{
	if (n > 0) hipLaunchKernelGGL(md_kernel<true>, dim3((n + FIN_WAVES - 1) / FIN_WAVES), dim3(64 * FIN_WAVES), 0, s, *R, recs, n, reads0, reads1, cigar, (int32_t*)nullptr,
								  (int32_t*)nullptr, md_off, md);
}
}
