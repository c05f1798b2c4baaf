// damage_kernels.hip -- the kernels of the damage profile (bodies: damage_body.hpp; host side: nabwa_damage.hip).
//
//   damage_kernel      a persistent grid of workgroups of REC_BLOCK threads, REC_LANES lanes per record; each workgroup counts into its table
//                      in LDS (dynamic: the table of n_pos, at most 37 KB) and flushes the non-zero words into the call's 64-bit table
//   damage_add_kernel  the call's table onto the handle's totals, once the host has seen that no record of the call was damaged
#include <hip/hip_runtime.h>
#include "launchers.hpp"
#include "damage_body.hpp"

__global__ __launch_bounds__(REC_BLOCK) void damage_kernel(const DmgParams P, unsigned long long *__restrict__ call, unsigned int *__restrict__ bad)
{
	extern __shared__ uint32_t dmg_lds[];
	dmg_block(P, dmg_lds, call, bad, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(256) void damage_add_kernel(int words, const unsigned long long *__restrict__ call, unsigned long long *__restrict__ total)
{
	const int w = (int)(blockIdx.x * 256 + threadIdx.x);
	if (w < words) total[w] += call[w];
}

extern "C" {
void nabwa_launch_damage(const DmgParams *P, int n_blocks, unsigned long long *call, unsigned int *bad, hipStream_t s)
{
	const size_t lds = (size_t)dmg_tab(P->n_pos).words * sizeof(uint32_t);
	hipLaunchKernelGGL(damage_kernel, dim3(n_blocks), dim3(REC_BLOCK), lds, s, *P, call, bad);
}
void nabwa_launch_damage_add(int words, const unsigned long long *call, unsigned long long *total, hipStream_t s)
{
	hipLaunchKernelGGL(damage_add_kernel, dim3((words + 255) / 256), dim3(256), 0, s, words, call, total);
}
}
