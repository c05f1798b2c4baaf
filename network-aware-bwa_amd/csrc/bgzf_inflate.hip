// bgzf_inflate.hip -- the BGZF decompressor's kernel: one wavefront inflates one BGZF member's payload to the member's destination
// and leaves one status word (the body: bgzf_inflate_body.hpp).
#include <hip/hip_runtime.h>
#include "launchers.hpp"
#include "bgzf_inflate_body.hpp"

__global__ __launch_bounds__(BGZF_LANES) void bgzf_inflate_kernel(const uint8_t *cmp, const BgzfInBlk *blk, int n_blk, uint8_t *plain, uint32_t *status)
{
	__shared__ BgziShared Sh;
	const int k = blockIdx.x;
	if (k >= n_blk) return;
	const BgzfInBlk b = blk[k];                        /* the host has checked src + n_src and dst + isize against its buffers */
	bgzf_inflate_member(Sh, threadIdx.x, cmp + b.src, b.n_src, plain + b.dst, b.isize, b.crc, status + k);
}

extern "C" void nabwa_launch_bgzf_inflate(const uint8_t *cmp, const BgzfInBlk *blk, int n_blk, uint8_t *plain, uint32_t *status, hipStream_t s)
{
	hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(n_blk), dim3(BGZF_LANES), 0, s, cmp, blk, n_blk, plain, status);
}
