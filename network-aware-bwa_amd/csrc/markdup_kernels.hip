// markdup_kernels.hip -- the kernels of duplicate marking (bodies: markdup_body.hpp; host side: nabwa_markdup.hip).
//
//   markdup_sig_kernel     a persistent grid of workgroups of REC_BLOCK threads, REC_LANES lanes per record: every record's class, ends and score
//                          into the call's scratch, the lowest damaged record into *bad
//   markdup_emit_kernel    one lane per record of a sound call: mates from the neighbours' scratch, tuples appended to the handle's arena
//   markdup_iota_kernel, markdup_gather_kernel    the index column and the key column of the next radix pass of the resolve
//   markdup_mark_kernel    one lane per sorted tuple: all but the head of a group are marked
//   markdup_prop_kernel    one lane per record: a half pair's unmapped mate takes its mate's mark
#include <hip/hip_runtime.h>
#include "launchers.hpp"
#include "markdup_body.hpp"

__global__ __launch_bounds__(REC_BLOCK) void markdup_sig_kernel(const MdParams P, unsigned int *__restrict__ bad)
{
	__shared__ unsigned long long sum[REC_GROUPS];
	__shared__ uint32_t diff[REC_GROUPS], meta[REC_GROUPS];
	md_block(P, sum, diff, meta, bad, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(256) void markdup_emit_kernel(const MdParams P, const MdArena A)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i < P.n_rec) md_emit_record(P, A, i);
}

__global__ __launch_bounds__(256) void markdup_iota_kernel(int64_t n, uint32_t *__restrict__ idx)
{
	const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (j < n) idx[j] = (uint32_t)j;
}

__global__ __launch_bounds__(256) void markdup_gather_kernel(int64_t n, const uint32_t *__restrict__ idx, const uint64_t *__restrict__ src, uint64_t *__restrict__ keys)
{
	const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (j < n) keys[j] = src[idx[j]];
}

__global__ __launch_bounds__(256) void markdup_mark_kernel(int64_t n, const uint32_t *__restrict__ idx, const uint64_t *__restrict__ hi, const uint64_t *__restrict__ lo,
														   const uint64_t *__restrict__ k3, uint8_t *__restrict__ dup, unsigned long long *__restrict__ stats)
{
	const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (j < n) md_mark_one(j, idx, hi, lo, k3, dup, stats);
}

__global__ __launch_bounds__(256) void markdup_prop_kernel(int64_t n, const uint8_t *__restrict__ link, uint8_t *dup, unsigned long long *__restrict__ stats)
{
	const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (o < n) md_prop_one(o, link, dup, stats);
}

static inline dim3 grid_of(int64_t n) { return dim3((unsigned int)((n + 255) / 256)); }

extern "C" {
void nabwa_launch_markdup_sig(const MdParams *P, int n_blocks, unsigned int *bad, hipStream_t s)
{
	hipLaunchKernelGGL(markdup_sig_kernel, dim3(n_blocks), dim3(REC_BLOCK), 0, s, *P, bad);
}
void nabwa_launch_markdup_emit(const MdParams *P, const MdArena *A, hipStream_t s)
{
	hipLaunchKernelGGL(markdup_emit_kernel, grid_of(P->n_rec), dim3(256), 0, s, *P, *A);
}
void nabwa_launch_markdup_iota(int64_t n, uint32_t *idx, hipStream_t s)
{
	hipLaunchKernelGGL(markdup_iota_kernel, grid_of(n), dim3(256), 0, s, n, idx);
}
void nabwa_launch_markdup_gather(int64_t n, const uint32_t *idx, const uint64_t *src, uint64_t *keys, hipStream_t s)
{
	hipLaunchKernelGGL(markdup_gather_kernel, grid_of(n), dim3(256), 0, s, n, idx, src, keys);
}
void nabwa_launch_markdup_mark(int64_t n, const uint32_t *idx, const uint64_t *hi, const uint64_t *lo, const uint64_t *k3, uint8_t *dup, unsigned long long *stats, hipStream_t s)
{
	hipLaunchKernelGGL(markdup_mark_kernel, grid_of(n), dim3(256), 0, s, n, idx, hi, lo, k3, dup, stats);
}
void nabwa_launch_markdup_prop(int64_t n, const uint8_t *link, uint8_t *dup, unsigned long long *stats, hipStream_t s)
{
	hipLaunchKernelGGL(markdup_prop_kernel, grid_of(n), dim3(256), 0, s, n, link, dup, stats);
}
}
