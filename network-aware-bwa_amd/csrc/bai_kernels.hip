// bai_kernels.hip -- the kernels of the BAM index (bodies: bai_body.hpp; host side: nabwa_bai.hip).
//
//   bai_sig_kernel         a persistent grid of workgroups of REC_BLOCK threads, REC_LANES lanes per record, the CIGAR's operations split over
//                          the lanes: every record's tuple into the arena, the lowest damaged record and the records without a reference counted
//   bai_iota_kernel        the ordinals beside the keys of the radix sort
//   bai_ref_kernel         a workgroup per REC_BLOCK tuples in stream order: virtual offsets, and what a reference's pseudo-bin and window count need
//   bai_head_kernel, bai_place_kernel    one lane per sorted tuple: bin and chunk heads; where bins and chunks start once the heads are scanned
//   bai_refsize_kernel     one lane per reference: the bytes and windows of its part
//   bai_lin_kernel         one lane per tuple: its virtual start into the windows it touches
//   bai_write_ref_kernel, bai_write_tuple_kernel, bai_write_lin_kernel    the file at the scanned offsets
#include <hip/hip_runtime.h>
#include "launchers.hpp"
#include "bai_body.hpp"

__global__ __launch_bounds__(REC_BLOCK) void bai_sig_kernel(const BaiParams P)
{
	__shared__ unsigned long long sum[REC_GROUPS];
	__shared__ uint32_t state[REC_GROUPS];
	bai_block(P, sum, state, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(256) void bai_iota_kernel(int64_t n, uint32_t *__restrict__ idx)
{
	const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (j < n) idx[j] = (uint32_t)j;
}

__global__ __launch_bounds__(REC_BLOCK) void bai_ref_kernel(const BaiFin F)
{
	__shared__ int l_tid[REC_BLOCK], l_win[REC_BLOCK];
	__shared__ unsigned int l_unm[REC_BLOCK];
	bai_ref_block(F, l_tid, l_win, l_unm, (int64_t)blockIdx.x);
}

#define BAI_ONE(name, body, count) \
__global__ __launch_bounds__(256) void name(const BaiFin F) \
{ \
	const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; \
	if (j < (count)) body(F, j); \
}
BAI_ONE(bai_head_kernel, bai_head_one, F.n)
BAI_ONE(bai_place_kernel, bai_place_one, F.n)
BAI_ONE(bai_refsize_kernel, bai_refsize_one, (int64_t)F.n_ref + 1)
BAI_ONE(bai_lin_kernel, bai_lin_one, F.n)
BAI_ONE(bai_write_ref_kernel, bai_write_ref, (int64_t)F.n_ref + 1)
BAI_ONE(bai_write_tuple_kernel, bai_write_tuple, F.n)
BAI_ONE(bai_write_lin_kernel, bai_write_lin, F.n_lin)

static inline dim3 grid_of(int64_t n) { return dim3((unsigned int)((n + 255) / 256)); }

extern "C" {
void nabwa_launch_bai_sig(const BaiParams *P, int n_blocks, hipStream_t s)
{
	hipLaunchKernelGGL(bai_sig_kernel, dim3(n_blocks), dim3(REC_BLOCK), 0, s, *P);
}
void nabwa_launch_bai_iota(int64_t n, uint32_t *idx, hipStream_t s)
{
	hipLaunchKernelGGL(bai_iota_kernel, grid_of(n), dim3(256), 0, s, n, idx);
}
void nabwa_launch_bai_step(int step, const BaiFin *F, hipStream_t s)
{
	switch (step) {
		case NABWA_BAI_STEP_REF: hipLaunchKernelGGL(bai_ref_kernel, dim3((unsigned int)((F->n + REC_BLOCK - 1) / REC_BLOCK)), dim3(REC_BLOCK), 0, s, *F); break;
		case NABWA_BAI_STEP_HEAD: hipLaunchKernelGGL(bai_head_kernel, grid_of(F->n), dim3(256), 0, s, *F); break;
		case NABWA_BAI_STEP_PLACE: hipLaunchKernelGGL(bai_place_kernel, grid_of(F->n), dim3(256), 0, s, *F); break;
		case NABWA_BAI_STEP_REFSIZE: hipLaunchKernelGGL(bai_refsize_kernel, grid_of((int64_t)F->n_ref + 1), dim3(256), 0, s, *F); break;
		case NABWA_BAI_STEP_LIN: hipLaunchKernelGGL(bai_lin_kernel, grid_of(F->n), dim3(256), 0, s, *F); break;
		case NABWA_BAI_STEP_WRITE_REF: hipLaunchKernelGGL(bai_write_ref_kernel, grid_of((int64_t)F->n_ref + 1), dim3(256), 0, s, *F); break;
		case NABWA_BAI_STEP_WRITE_TUPLE: hipLaunchKernelGGL(bai_write_tuple_kernel, grid_of(F->n), dim3(256), 0, s, *F); break;
		case NABWA_BAI_STEP_WRITE_LIN: hipLaunchKernelGGL(bai_write_lin_kernel, grid_of(F->n_lin), dim3(256), 0, s, *F); break;
	}
}
}
