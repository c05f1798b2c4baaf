// nabwa_bgzf.hip -- the host side of the BGZF compressor (kernels: bgzf_deflate.hip): a handle that keeps its stream, its device buffers
// and its pinned staging buffers between calls, and the one-shot entry, which is the handle used once.  Input goes through in rounds
// of at most 1040 slices (64.7 MB, so that the 64 MB the tool's writer collects are one round; more slices are dealt evenly over
// the rounds they need): pageable -> pinned -> HBM, one block per slice, packed on the device, and only the packed bytes come back.
#include <hip/hip_runtime.h>
#include <string.h>
#include "../../include/nabwa.h"
#include "nabwa_internal.hpp"
#include "dev_pool.hpp"
#include "launchers.hpp"

#define SLICE  ((int64_t)0xff00)
#define STRIDE ((int64_t)0x10000)
#define CHUNK  ((int64_t)1040)                        /* slices per launch, at most */

struct nabwa_bgzf {
	int device = 0;
	int64_t cap = 0;                                   /* slices the buffers hold */
	DevStream st;
	DevBuf d_in, d_stage, d_packed, d_sizes, d_total;
	uint8_t *h_in = nullptr, *h_out = nullptr; int64_t *h_total = nullptr;      /* pinned */
	void unpin() { if (h_in) (void)hipHostFree(h_in); if (h_out) (void)hipHostFree(h_out); h_in = h_out = nullptr; }
	~nabwa_bgzf() { (void)hipSetDevice(device); if (st.s) (void)hipStreamSynchronize(st.s); unpin(); if (h_total) (void)hipHostFree(h_total); }
};

extern "C" int64_t nabwa_bgzf_bound(int64_t n)
{
	return n <= 0 ? 0 : (n + SLICE - 1) / SLICE * STRIDE;
}

extern "C" int nabwa_bgzf_create(int device, nabwa_bgzf_t **out)
{
	if (!out) return nabwa_fail(NABWA_EINVAL, "null argument");
	*out = nullptr;
	HIP_CHECK(hipSetDevice(device));
	nabwa_bgzf *z = new nabwa_bgzf; z->device = device;
	int r = NABWA_OK;
	hipError_t e = hipStreamCreateWithFlags(&z->st.s, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipHostMalloc((void**)&z->h_total, sizeof(int64_t), hipHostMallocDefault);
	if (e != hipSuccess) r = nabwa_hip_fail(e, "setting up the BGZF compressor", __FILE__, __LINE__);
	if (r == NABWA_OK) r = z->d_total.get(sizeof(int64_t));
	if (r != NABWA_OK) { delete z; return r; }
	*out = z;
	return NABWA_OK;
}

extern "C" void nabwa_bgzf_destroy(nabwa_bgzf_t *z) { delete z; }

/* buffers for `slices` slices (at most CHUNK); they only grow */
static int bgzf_reserve(nabwa_bgzf *z, int64_t slices)
{
	if (slices <= z->cap) return NABWA_OK;
	HIP_CHECK(hipStreamSynchronize(z->st));
	z->cap = 0;
	HIP_CHECK(z->d_in.release()); HIP_CHECK(z->d_stage.release()); HIP_CHECK(z->d_packed.release()); HIP_CHECK(z->d_sizes.release());
	z->unpin();
	if (int r = z->d_in.get((size_t)(slices * SLICE))) return r;
	if (int r = z->d_stage.get((size_t)(slices * STRIDE))) return r;
	if (int r = z->d_packed.get((size_t)(slices * STRIDE))) return r;
	if (int r = z->d_sizes.get((size_t)slices * sizeof(uint32_t))) return r;
	HIP_CHECK(hipHostMalloc((void**)&z->h_in, (size_t)(slices * SLICE), hipHostMallocDefault));
	HIP_CHECK(hipHostMalloc((void**)&z->h_out, (size_t)(slices * STRIDE), hipHostMallocDefault));
	z->cap = slices;
	return NABWA_OK;
}

extern "C" int nabwa_bgzf_handle_compress(nabwa_bgzf_t *z, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks)
{
	if (!z || n < 0 || cap < 0 || (n && !in) || (cap && !out)) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (n_out) *n_out = 0;
	if (n_blocks) *n_blocks = (n + SLICE - 1) / SLICE;
	if (n == 0) return NABWA_OK;
	HIP_CHECK(hipSetDevice(z->device));
	const int64_t slices_all = (n + SLICE - 1) / SLICE;
	const int64_t rounds = (slices_all + CHUNK - 1) / CHUNK, per = (slices_all + rounds - 1) / rounds;      /* no round of a few slices at the end */
	if (int r = bgzf_reserve(z, per)) return r;
	StreamDrain drain{ z->st };
	int64_t done = 0;                                  /* bytes the blocks take; written only while they fit */
	for (int64_t at = 0; at < n; at += per * SLICE) {
		const int64_t m = n - at < per * SLICE ? n - at : per * SLICE;
		const int ns = (int)((m + SLICE - 1) / SLICE);
		memcpy(z->h_in, in + at, (size_t)m);
		HIP_CHECK(hipMemcpyAsync(z->d_in.p, z->h_in, (size_t)m, hipMemcpyHostToDevice, z->st));
		nabwa_launch_bgzf_deflate(z->d_in.as<uint8_t>(), m, ns, z->d_stage.as<uint8_t>(), z->d_sizes.as<uint32_t>(), z->st);
		nabwa_launch_bgzf_pack(z->d_stage.as<uint8_t>(), z->d_sizes.as<uint32_t>(), ns, z->d_packed.as<uint8_t>(), z->d_total.as<int64_t>(), z->st);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpyAsync(z->h_total, z->d_total.p, sizeof(int64_t), hipMemcpyDeviceToHost, z->st));
		HIP_CHECK(hipStreamSynchronize(z->st));
		const int64_t got = *z->h_total;
		if (got < 0 || got > (int64_t)ns * STRIDE) return nabwa_fail(NABWA_ENODEV, "the BGZF kernels returned a size that cannot be");
		if (done + got <= cap) {
			HIP_CHECK(hipMemcpyAsync(z->h_out, z->d_packed.p, (size_t)got, hipMemcpyDeviceToHost, z->st));
			HIP_CHECK(hipStreamSynchronize(z->st));
			memcpy(out + done, z->h_out, (size_t)got);
		}
		done += got;
	}
	if (n_out) *n_out = done;
	if (done > cap) return nabwa_fail(NABWA_ECAP, "the output buffer is too small for the BGZF blocks (*n_out says how much is needed)");
	return NABWA_OK;
}

extern "C" int nabwa_bgzf_compress(int device, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks)
{
	nabwa_bgzf_t *z = nullptr;
	if (int r = nabwa_bgzf_create(device, &z)) return r;
	const int r = nabwa_bgzf_handle_compress(z, in, n, out, cap, n_out, n_blocks);
	nabwa_bgzf_destroy(z);
	return r;
}
