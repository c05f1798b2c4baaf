// bam_sort.hip -- coordinate sort of finished BAM records on the GPU (nabwa_bam_sort*, include/nabwa.h): the two kernels
// (bodies: bam_sort_body.hpp) and the host side, a handle that keeps its stream and its device buffers between calls.
//
//   upload bytes and offsets -> key kernel (key and index per record, the lowest record whose block_size is not what its offsets say)
//   -> hipcub radix sort of (key, index), stable -> sizes in the new order, exclusive scan: the new offsets -> gather kernel -> download
//
// Everything runs on the handle's stream.  The host decides what it can from the offsets alone, before any device call.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdio.h>
#include "../../include/nabwa.h"
#include "nabwa_internal.hpp"
#include "dev_pool.hpp"
#include "bam_sort_body.hpp"

// one lane per record.  off[] are the caller's offsets, base = off[0]: record i lies at in + (off[i] - base).  The host has checked that
// every record has at least BSORT_MIN_REC bytes, so bytes 0..11 exist.
__global__ __launch_bounds__(256) void bam_sort_key_kernel(int n, const uint8_t *__restrict__ in, const int64_t *__restrict__ off, int64_t base,
														   uint64_t *__restrict__ keys, uint32_t *__restrict__ idx, unsigned int *__restrict__ bad)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      /* 64 bits: n may be 2^31 - 1 */
	if (i >= n) return;
	const int64_t o = off[i], size = off[i + 1] - o;
	const uint8_t *rec = in + (o - base);
	keys[i] = bsort_key(rec);
	idx[i] = (uint32_t)i;
	if ((int64_t)bsort_u32(rec) + 4 != size) atomicMin(bad, (unsigned int)i);
}

// the size of the record that comes j-th in the new order; psize[n] = 0 closes the scan that turns the sizes into offsets
__global__ __launch_bounds__(256) void bam_sort_sizes_kernel(int n, const uint32_t *__restrict__ idx, const int64_t *__restrict__ off, int64_t *__restrict__ psize)
{
	const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (j > n) return;
	if (j == n) { psize[n] = 0; return; }
	const uint32_t i = idx[j];
	psize[j] = off[i + 1] - off[i];
}

// BSORT_LANES lanes per record: record idx[j] from its old place to out + ooff[j].  ooff[j + 1] - ooff[j] is its size; ooff[n] is the total,
// which is the input's total: nothing at or beyond it is written, nothing outside the record is read.
__global__ __launch_bounds__(256) void bam_sort_gather_kernel(int n, const uint8_t *__restrict__ in, const int64_t *__restrict__ off, int64_t base,
															  const uint32_t *__restrict__ idx, const int64_t *__restrict__ ooff, uint8_t *__restrict__ out)
{
	const int t = threadIdx.x & (BSORT_LANES - 1);
	const int64_t j = (int64_t)blockIdx.x * (256 / BSORT_LANES) + (threadIdx.x / BSORT_LANES);
	if (j >= n) return;
	const int64_t d = ooff[j];
	bsort_copy_part(in + (off[idx[j]] - base), out + d, ooff[j + 1] - d, t);
}

struct nabwa_bam_sort {
	int device = 0;
	DevStream st;
	DevBuf d_in, d_out, d_off, d_ooff, d_keys[2], d_idx[2], d_tmp, d_bad;
	int64_t cap_bytes = 0, cap_rec = 0; size_t cap_tmp = 0;
	unsigned int *h_bad = nullptr;                         /* pinned */
	hipEvent_t ev[7] = {};
	float ms[6] = { 0, 0, 0, 0, 0, 0 };
	~nabwa_bam_sort()
	{
		(void)hipSetDevice(device);
		if (st.s) (void)hipStreamSynchronize(st.s);
		if (h_bad) (void)hipHostFree(h_bad);
		for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
	}
};

static int fail_fmt(int code, const char *fmt, long long a, long long b = 0, long long c = 0)
{
	char m[256]; snprintf(m, sizeof m, fmt, a, b, c);
	return nabwa_fail(code, "%s", m);
}

/* what the offsets alone say; *total = the records' bytes */
static int sort_check(int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *total)
{
	if (n_rec < 0 || n_rec > 0x7fffffff) return fail_fmt(NABWA_EINVAL, "n_rec %lld: 0 .. 2147483647 records", (long long)n_rec);
	if (!in_off || cap < 0 || (n_rec && (!in || !out))) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (in_off[0] < 0) return nabwa_fail(NABWA_EINVAL, "the first offset is negative");
	for (int64_t i = 0; i < n_rec; ++i) {
		if (in_off[i + 1] <= in_off[i]) return fail_fmt(NABWA_EINVAL, "the offsets do not increase at record %lld", (long long)i);
		if (in_off[i + 1] - in_off[i] < BSORT_MIN_REC) return fail_fmt(NABWA_EINVAL, "record %lld has %lld bytes: a BAM record has at least 36", (long long)i, (long long)(in_off[i + 1] - in_off[i]));
	}
	*total = in_off[n_rec] - in_off[0];
	if (*total > cap) return fail_fmt(NABWA_ECAP, "the output buffer holds %lld bytes, the records need %lld", (long long)cap, (long long)*total);
	return NABWA_OK;
}

extern "C" int nabwa_bam_sort_create(int device, nabwa_bam_sort_t **out)
{
	if (!out) return nabwa_fail(NABWA_EINVAL, "null argument");
	*out = nullptr;
	const hipError_t e0 = hipSetDevice(device);
	if (e0 != hipSuccess) { (void)hipGetLastError(); return nabwa_hip_fail(e0, "hipSetDevice(device)", __FILE__, __LINE__); }      /* (the runtime's last error is not left for a later call to find) */
	nabwa_bam_sort_t *s = new nabwa_bam_sort_t; s->device = device;
	hipError_t e = hipStreamCreateWithFlags(&s->st.s, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipHostMalloc((void**)&s->h_bad, sizeof(unsigned int), hipHostMallocDefault);
	for (int k = 0; k < 7 && e == hipSuccess; ++k) e = hipEventCreate(&s->ev[k]);
	int r = e == hipSuccess ? NABWA_OK : nabwa_hip_fail(e, "setting up the BAM sort", __FILE__, __LINE__);
	if (r == NABWA_OK) r = s->d_bad.get(sizeof(unsigned int));
	if (r != NABWA_OK) { delete s; return r; }
	*out = s;
	return NABWA_OK;
}

extern "C" void nabwa_bam_sort_destroy(nabwa_bam_sort_t *s) { delete s; }

/* a buffer of at least `bytes`; out of device memory is the caller's to act on (a smaller run), anything else is the device's */
static int sort_get(DevBuf &b, size_t bytes)
{
	const hipError_t e = b.release();
	if (e != hipSuccess) return nabwa_hip_fail(e, "hipFree", __FILE__, __LINE__);
	const hipError_t m = hipMalloc(&b.p, bytes ? bytes : 1);
	if (m == hipErrorOutOfMemory) { (void)hipGetLastError(); b.p = nullptr; return fail_fmt(NABWA_ENOMEM, "the run does not fit the device: a buffer of %lld bytes could not be had", (long long)bytes); }
	if (m != hipSuccess) { b.p = nullptr; return nabwa_hip_fail(m, "hipMalloc", __FILE__, __LINE__); }
	return NABWA_OK;
}

/* buffers for `total` bytes in `n` records and `tmp` bytes of scratch; they only grow (by a quarter more than asked, as the inflater's) */
static int sort_reserve(nabwa_bam_sort_t *s, int64_t total, int64_t n, size_t tmp)
{
	if (total <= s->cap_bytes && n <= s->cap_rec && tmp <= s->cap_tmp) return NABWA_OK;
	HIP_CHECK(hipStreamSynchronize(s->st));
	if (total > s->cap_bytes) {
		s->cap_bytes = 0;
		const int64_t want = total + total / 4;
		if (int r = sort_get(s->d_in, (size_t)want)) return r;
		if (int r = sort_get(s->d_out, (size_t)want)) return r;
		s->cap_bytes = want;
	}
	if (n > s->cap_rec) {
		s->cap_rec = 0;
		const int64_t want = n + n / 4;
		if (int r = sort_get(s->d_off, (size_t)(want + 1) * 8)) return r;
		if (int r = sort_get(s->d_ooff, (size_t)(want + 1) * 8)) return r;
		for (int k = 0; k < 2; ++k) {
			if (int r = sort_get(s->d_keys[k], (size_t)want * 8)) return r;
			if (int r = sort_get(s->d_idx[k], (size_t)want * 4)) return r;
		}
		s->cap_rec = want;
	}
	if (tmp > s->cap_tmp) {
		s->cap_tmp = 0;
		const size_t want = tmp + tmp / 4;
		if (int r = sort_get(s->d_tmp, want)) return r;
		s->cap_tmp = want;
	}
	return NABWA_OK;
}

static int sort_run_checked(nabwa_bam_sort_t *s, int64_t n_rec, int64_t total, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t *out_off, uint64_t *keys_out, uint32_t *perm_out)
{
	HIP_CHECK(hipSetDevice(s->device));
	const int n = (int)n_rec;
	hipStream_t st = s->st;
	size_t tmp = 0, need = 0;
	{
		hipcub::DoubleBuffer<uint64_t> dk(nullptr, nullptr); hipcub::DoubleBuffer<uint32_t> dv(nullptr, nullptr);
		HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, dk, dv, n, 0, 64, st)); if (need > tmp) tmp = need;
		HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (int64_t*)nullptr, (int64_t*)nullptr, (size_t)n + 1, st)); if (need > tmp) tmp = need;
	}
	if (int r = sort_reserve(s, total, n_rec, tmp)) return r;
	StreamDrain drain{ st };
	const int64_t base = in_off[0];
	*s->h_bad = 0xffffffffu;
	HIP_CHECK(hipEventRecord(s->ev[0], st));
	HIP_CHECK(hipMemcpyAsync(s->d_in.p, in + base, (size_t)total, hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemcpyAsync(s->d_off.p, in_off, (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemcpyAsync(s->d_bad.p, s->h_bad, sizeof(unsigned int), hipMemcpyHostToDevice, st));
	HIP_CHECK(hipEventRecord(s->ev[1], st));
	hipLaunchKernelGGL(bam_sort_key_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, s->d_in.as<uint8_t>(), s->d_off.as<int64_t>(), base,
					   s->d_keys[0].as<uint64_t>(), s->d_idx[0].as<uint32_t>(), s->d_bad.as<unsigned int>());
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(s->ev[2], st));
	hipcub::DoubleBuffer<uint64_t> dk(s->d_keys[0].as<uint64_t>(), s->d_keys[1].as<uint64_t>());
	hipcub::DoubleBuffer<uint32_t> dv(s->d_idx[0].as<uint32_t>(), s->d_idx[1].as<uint32_t>());
	need = s->cap_tmp;
	HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(s->d_tmp.p, need, dk, dv, n, 0, 64, st));
	HIP_CHECK(hipEventRecord(s->ev[3], st));
	hipLaunchKernelGGL(bam_sort_sizes_kernel, dim3(n / 256 + 1), dim3(256), 0, st, n, dv.Current(), s->d_off.as<int64_t>(), s->d_ooff.as<int64_t>());
	HIP_CHECK(hipGetLastError());
	need = s->cap_tmp;
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(s->d_tmp.p, need, s->d_ooff.as<int64_t>(), s->d_ooff.as<int64_t>(), (size_t)n + 1, st));
	HIP_CHECK(hipEventRecord(s->ev[4], st));
	hipLaunchKernelGGL(bam_sort_gather_kernel, dim3((n + 256 / BSORT_LANES - 1) / (256 / BSORT_LANES)), dim3(256), 0, st, n, s->d_in.as<uint8_t>(), s->d_off.as<int64_t>(), base,
					   dv.Current(), s->d_ooff.as<int64_t>(), s->d_out.as<uint8_t>());
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(s->ev[5], st));
	HIP_CHECK(hipMemcpyAsync(s->h_bad, s->d_bad.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipStreamSynchronize(st));
	if (*s->h_bad != 0xffffffffu) {
		const int64_t i = (int64_t)*s->h_bad;
		uint32_t bs = 0;
		if (i < n_rec) memcpy(&bs, in + in_off[i], 4);
		return fail_fmt(NABWA_EDATA, "record %lld: its block_size says %lld bytes, its offsets %lld", (long long)i, (long long)bs + 4, i < n_rec ? (long long)(in_off[i + 1] - in_off[i]) : -1LL);
	}
	HIP_CHECK(hipMemcpyAsync(out, s->d_out.p, (size_t)total, hipMemcpyDeviceToHost, st));
	if (out_off) HIP_CHECK(hipMemcpyAsync(out_off, s->d_ooff.p, (size_t)(n_rec + 1) * 8, hipMemcpyDeviceToHost, st));
	if (keys_out) HIP_CHECK(hipMemcpyAsync(keys_out, dk.Current(), (size_t)n_rec * 8, hipMemcpyDeviceToHost, st));
	if (perm_out) HIP_CHECK(hipMemcpyAsync(perm_out, dv.Current(), (size_t)n_rec * 4, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipEventRecord(s->ev[6], st));
	HIP_CHECK(hipStreamSynchronize(st));
	for (int k = 0; k < 6; ++k) HIP_CHECK(hipEventElapsedTime(&s->ms[k], s->ev[k], s->ev[k + 1]));
	return NABWA_OK;
}

extern "C" int nabwa_bam_sort_run_ex(nabwa_bam_sort_t *s, int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *out_off, uint64_t *keys_out, uint32_t *perm_out)
{
	if (!s) return nabwa_fail(NABWA_EINVAL, "null argument");
	int64_t total = 0;
	if (int r = sort_check(n_rec, in, in_off, out, cap, &total)) return r;
	if (n_rec == 0) return NABWA_OK;
	return sort_run_checked(s, n_rec, total, in, in_off, out, out_off, keys_out, perm_out);
}

extern "C" int nabwa_bam_sort_ex(int device, int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *out_off, uint64_t *keys_out, uint32_t *perm_out)
{
	int64_t total = 0;
	if (int r = sort_check(n_rec, in, in_off, out, cap, &total)) return r;      /* before the device is looked for */
	if (n_rec == 0) return NABWA_OK;
	nabwa_bam_sort_t *s = nullptr;
	if (int r = nabwa_bam_sort_create(device, &s)) return r;
	const int r = sort_run_checked(s, n_rec, total, in, in_off, out, out_off, keys_out, perm_out);
	nabwa_bam_sort_destroy(s);
	return r;
}

extern "C" int nabwa_bam_sort_run(nabwa_bam_sort_t *s, int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *out_off, uint64_t *keys_out)
{
	return nabwa_bam_sort_run_ex(s, n_rec, in, in_off, out, cap, out_off, keys_out, nullptr);
}

extern "C" int nabwa_bam_sort(int device, int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *out_off, uint64_t *keys_out)
{
	return nabwa_bam_sort_ex(device, n_rec, in, in_off, out, cap, out_off, keys_out, nullptr);
}

extern "C" int nabwa_bam_sort_times(const nabwa_bam_sort_t *s, float ms[6])
{
	if (!s || !ms) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (int k = 0; k < 6; ++k) ms[k] = s->ms[k];
	return NABWA_OK;
}
