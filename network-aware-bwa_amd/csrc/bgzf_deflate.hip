// bgzf_deflate.hip -- the BGZF compressor's kernels: one wavefront turns one slice of <= 0xff00 bytes into one BGZF block in its slot
// of the staging area (the body: bgzf_deflate_body.hpp), a second kernel packs the blocks back to back.
#include <hip/hip_runtime.h>
#include "launchers.hpp"
#include "bgzf_deflate_body.hpp"

static_assert(sizeof(BgzfShared) <= 160 * 1024, "the slice's working set has to fit one CU's LDS");

__global__ __launch_bounds__(BGZF_LANES) void bgzf_deflate_kernel(const uint8_t *in, int64_t n, uint8_t *stage, uint32_t *sizes)
{
	__shared__ BgzfShared Sh;
	const uint32_t t = threadIdx.x;
	const int64_t at = (int64_t)blockIdx.x * BGZF_SLICE;
	const uint32_t m = n - at < (int64_t)BGZF_SLICE ? (uint32_t)(n - at) : BGZF_SLICE;      /* the grid has ceil(n / 0xff00) workgroups: m >= 1 */
	uint32_t *ow = (uint32_t*)(stage + (size_t)blockIdx.x * BGZF_STRIDE);
	bgzf_phase_load(Sh, t, (const uint32_t*)(in + at), m);
	__syncthreads();
	bgzf_phase_parse(Sh, t, m);
	__syncthreads();
	bgzf_phase_scan(Sh, t, m);
	__syncthreads();
	bgzf_phase_zero(Sh, t, ow);
	__threadfence();                                   /* the zeros are in place before another lane's atomic OR reaches the word */
	__syncthreads();
	bgzf_phase_emit(Sh, t, m, ow, sizes + blockIdx.x);
}

/* the same slice, the same parse and the same tokens; the block is a dynamic Huffman one where that is strictly shorter than what the
 * kernel above writes, and otherwise that block byte for byte (the phases: bgzf_deflate_body.hpp) */
__global__ __launch_bounds__(BGZF_LANES) void bgzf_deflate_dyn_kernel(const uint8_t *in, int64_t n, uint8_t *stage, uint32_t *sizes)
{
	__shared__ BgzfShared Sh;
	const uint32_t t = threadIdx.x;
	const int64_t at = (int64_t)blockIdx.x * BGZF_SLICE;
	const uint32_t m = n - at < (int64_t)BGZF_SLICE ? (uint32_t)(n - at) : BGZF_SLICE;      /* the grid has ceil(n / 0xff00) workgroups: m >= 1 */
	uint32_t *ow = (uint32_t*)(stage + (size_t)blockIdx.x * BGZF_STRIDE);
	bgzf_phase_load(Sh, t, (const uint32_t*)(in + at), m);
	__syncthreads();
	bgzf_phase_parse(Sh, t, m);
	__syncthreads();
	bgzf_phase_scan(Sh, t, m);
	bgzf_dyn_phase_clear(Sh, t);                       /* the hash table is dead: its place is the dynamic mode's tables */
	__syncthreads();
	bgzf_dyn_phase_count(Sh, t, m);
	__syncthreads();
	bgzf_dyn_phase_sort(Sh, t);
	__syncthreads();
	bgzf_dyn_phase_header(Sh, t);
	__syncthreads();
	bgzf_dyn_phase_measure(Sh, t, m, ow);
	__syncthreads();
	bgzf_dyn_phase_offsets(Sh, t);
	__threadfence();                                   /* the zeros are in place before another lane's atomic OR reaches the word */
	__syncthreads();
	bgzf_dyn_phase_emit(Sh, t, m, ow, sizes + blockIdx.x);
}

/* block k of the staging area to the sum of the sizes before it (at most a launch's slices, a few loads per lane); the last workgroup
 * writes the total.  A block starts at any byte of the packed area and at a multiple of 0x10000 of the staging area: bytes up to the
 * destination's next word, then whole words put together from two of the source's, then the bytes that are left. */
__global__ __launch_bounds__(256) void bgzf_pack_kernel(const uint8_t *stage, const uint32_t *sizes, int n_slices, uint8_t *packed, int64_t *total)
{
	__shared__ unsigned long long part[256];
	const int k = blockIdx.x, t = threadIdx.x;
	unsigned long long s = 0;
	for (int j = t; j < k; j += 256) s += sizes[j];
	part[t] = s;
	__syncthreads();
	for (int o = 128; o > 0; o >>= 1) { if (t < o) part[t] += part[t + o]; __syncthreads(); }
	const unsigned long long off = part[0];
	const uint32_t sz = sizes[k];                      /* 28..0x10000 */
	const uint8_t *src = stage + (size_t)k * BGZF_STRIDE;
	uint8_t *dst = packed + off;
	uint32_t head = (uint32_t)(4u - ((uintptr_t)dst & 3u)) & 3u;
	if (head > sz) head = sz;
	const uint32_t words = (sz - head) / 4, tail = head + words * 4;
	if ((uint32_t)t < head) dst[t] = src[t];
	const uint32_t *sw = (const uint32_t*)src;
	uint32_t *dw = (uint32_t*)(dst + head);
	/* word i of the destination is the source's bytes head + 4 i .. head + 4 i + 3: they end before sz <= 0x10000, so source word i + 1,
	 * read only when head > 0, begins before the slot's end */
	if (head == 0) for (uint32_t i = t; i < words; i += 256) dw[i] = sw[i];
	else for (uint32_t i = t; i < words; i += 256) dw[i] = (uint32_t)((((uint64_t)sw[i + 1] << 32) | sw[i]) >> (8 * head));
	if (tail + t < sz && t < 4) dst[tail + t] = src[tail + t];
	if (k == n_slices - 1 && t == 0) *total = (int64_t)(off + sz);
}

extern "C" void nabwa_launch_bgzf_deflate(const uint8_t *in, int64_t n, int n_slices, uint8_t *stage, uint32_t *sizes, hipStream_t s)
{
	hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(n_slices), dim3(BGZF_LANES), 0, s, in, n, stage, sizes);
}
extern "C" void nabwa_launch_bgzf_deflate_dyn(const uint8_t *in, int64_t n, int n_slices, uint8_t *stage, uint32_t *sizes, hipStream_t s)
{
	hipLaunchKernelGGL(bgzf_deflate_dyn_kernel, dim3(n_slices), dim3(BGZF_LANES), 0, s, in, n, stage, sizes);
}
extern "C" void nabwa_launch_bgzf_pack(const uint8_t *stage, const uint32_t *sizes, int n_slices, uint8_t *packed, int64_t *total, hipStream_t s)
{
	hipLaunchKernelGGL(bgzf_pack_kernel, dim3(n_slices), dim3(256), 0, s, stage, sizes, n_slices, packed, total);
}
