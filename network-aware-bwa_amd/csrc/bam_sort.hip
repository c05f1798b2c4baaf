// bam_sort.hip -- coordinate sort of finished BAM records on the GPU (nabwa_bam_sort*, include/nabwa.h): the two kernels
// (bodies: bam_sort_body.hpp) and the host side, a handle that keeps its stream and its device buffers between calls.
//
//   upload bytes and offsets -> key kernel (key and index per record, the lowest record whose block_size is not what its offsets say)
//   -> hipcub radix sort of (key, index), stable -> sizes in the new order, exclusive scan: the new offsets -> gather kernel -> download
//
// Everything runs on the handle's stream.  The host decides what it can from the offsets alone, before any device call.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "rec_stream.hpp"
#include "bam_sort_body.hpp"

#define SORT_FIT "the run does not fit the device: a buffer of %lld bytes could not be had"

// one lane per record.  off[] are the caller's offsets, base = off[0]: record i lies at in + (off[i] - base).  The host has checked that
// every record has at least REC_MIN_REC bytes, so bytes 0..11 exist.
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

// REC_LANES lanes per record: record idx[j] from its old place to out + ooff[j].  ooff[j + 1] - ooff[j] is its size; ooff[n] is the total,
// which is the input's total: nothing at or beyond it is written, nothing outside the record is read.
__global__ __launch_bounds__(256) void bam_sort_gather_kernel(int n, const uint8_t *__restrict__ in, const int64_t *__restrict__ off, int64_t base,
															  const uint32_t *__restrict__ idx, const int64_t *__restrict__ ooff, uint8_t *__restrict__ out)
{
	const int t = threadIdx.x & (REC_LANES - 1);
	const int64_t j = (int64_t)blockIdx.x * (256 / REC_LANES) + (threadIdx.x / REC_LANES);
	if (j >= n) return;
	const int64_t d = ooff[j];
	bsort_copy_part(in + (off[idx[j]] - base), out + d, ooff[j + 1] - d, t);
}

struct nabwa_bam_sort {
	RecStream rs;                                          /* h_words: bad */
	DevBuf d_in, d_out, d_off, d_ooff, d_keys[2], d_idx[2], d_tmp, d_bad;
	int64_t cap_bytes = 0, cap_rec = 0; size_t cap_tmp = 0;
	float ms[6] = { 0, 0, 0, 0, 0, 0 };
	~nabwa_bam_sort() { rs.quiesce(); }
};

/* what the offsets alone say; *total = the records' bytes */
static int sort_check(int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *total)
{
	if (int r = rec_check_offsets(n_rec, in, in_off, cap < 0 || (n_rec && !out))) return r;
	*total = in_off[n_rec] - in_off[0];
	if (*total > cap) return fail_fmt(NABWA_ECAP, "the output buffer holds %lld bytes, the records need %lld", (long long)cap, (long long)*total);
	return NABWA_OK;
}

extern "C" int nabwa_bam_sort_create(int device, nabwa_bam_sort_t **out)
{
	if (!out) return nabwa_fail(NABWA_EINVAL, "null argument");
	*out = nullptr;
	nabwa_bam_sort_t *s = new nabwa_bam_sort_t;
	int r = s->rs.setup(device, 0, 1, 7, "setting up the BAM sort");
	if (r == NABWA_OK) r = s->d_bad.get(sizeof(unsigned int));
	if (r != NABWA_OK) { delete s; return r; }
	*out = s;
	return NABWA_OK;
}

extern "C" void nabwa_bam_sort_destroy(nabwa_bam_sort_t *s) { delete s; }

static int sort_run_checked(nabwa_bam_sort_t *s, int64_t n_rec, int64_t total, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t *out_off, uint64_t *keys_out, uint32_t *perm_out)
{
	HIP_CHECK(hipSetDevice(s->rs.device));
	const int n = (int)n_rec;
	hipStream_t st = s->rs.st;
	size_t tmp = 0, need = 0;
	{
		hipcub::DoubleBuffer<uint64_t> dk(nullptr, nullptr); hipcub::DoubleBuffer<uint32_t> dv(nullptr, nullptr);
		HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, dk, dv, n, 0, 64, st)); if (need > tmp) tmp = need;
		HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (int64_t*)nullptr, (int64_t*)nullptr, (size_t)n + 1, st)); if (need > tmp) tmp = need;
	}
	/* the buffers only grow; a unit more than the records in each of theirs: the offsets need it, the keys and indices get it too */
	if (int r = rec_reserve(s->cap_bytes, total, 0, st, SORT_FIT, { { &s->d_in, 1 }, { &s->d_out, 1 } })) return r;
	if (int r = rec_reserve(s->cap_rec, n_rec, 0, st, SORT_FIT, { { &s->d_off, 8 }, { &s->d_ooff, 8 }, { &s->d_keys[0], 8 }, { &s->d_idx[0], 4 }, { &s->d_keys[1], 8 }, { &s->d_idx[1], 4 } }, 1)) return r;
	if (int r = rec_reserve_tmp(s->cap_tmp, tmp, s->d_tmp, st, SORT_FIT)) return r;
	StreamDrain drain{ st };
	const int64_t base = in_off[0];
	unsigned int *h_bad = s->rs.h_words;
	*h_bad = 0xffffffffu;
	if (int r = rec_upload(s->rs, s->d_in, s->d_off, s->d_bad.p, h_bad, 1, n_rec, in, in_off)) return r;
	hipLaunchKernelGGL(bam_sort_key_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, s->d_in.as<uint8_t>(), s->d_off.as<int64_t>(), base,
					   s->d_keys[0].as<uint64_t>(), s->d_idx[0].as<uint32_t>(), s->d_bad.as<unsigned int>());
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(s->rs.ev[2], st));
	hipcub::DoubleBuffer<uint64_t> dk(s->d_keys[0].as<uint64_t>(), s->d_keys[1].as<uint64_t>());
	hipcub::DoubleBuffer<uint32_t> dv(s->d_idx[0].as<uint32_t>(), s->d_idx[1].as<uint32_t>());
	need = s->cap_tmp;
	HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(s->d_tmp.p, need, dk, dv, n, 0, 64, st));
	HIP_CHECK(hipEventRecord(s->rs.ev[3], st));
	hipLaunchKernelGGL(bam_sort_sizes_kernel, dim3(n / 256 + 1), dim3(256), 0, st, n, dv.Current(), s->d_off.as<int64_t>(), s->d_ooff.as<int64_t>());
	HIP_CHECK(hipGetLastError());
	need = s->cap_tmp;
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(s->d_tmp.p, need, s->d_ooff.as<int64_t>(), s->d_ooff.as<int64_t>(), (size_t)n + 1, st));
	HIP_CHECK(hipEventRecord(s->rs.ev[4], st));
	hipLaunchKernelGGL(bam_sort_gather_kernel, dim3((n + 256 / REC_LANES - 1) / (256 / REC_LANES)), dim3(256), 0, st, n, s->d_in.as<uint8_t>(), s->d_off.as<int64_t>(), base,
					   dv.Current(), s->d_ooff.as<int64_t>(), s->d_out.as<uint8_t>());
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(s->rs.ev[5], st));
	HIP_CHECK(hipMemcpyAsync(h_bad, s->d_bad.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipStreamSynchronize(st));
	if (*h_bad != 0xffffffffu) {
		const int64_t i = (int64_t)*h_bad;
		return rec_fail_block_size(i, (int64_t)(i < n_rec ? rec_u32(in + in_off[i]) : 0) + 4, i < n_rec ? in_off[i + 1] - in_off[i] : -1);
	}
	HIP_CHECK(hipMemcpyAsync(out, s->d_out.p, (size_t)total, hipMemcpyDeviceToHost, st));
	if (out_off) HIP_CHECK(hipMemcpyAsync(out_off, s->d_ooff.p, (size_t)(n_rec + 1) * 8, hipMemcpyDeviceToHost, st));
	if (keys_out) HIP_CHECK(hipMemcpyAsync(keys_out, dk.Current(), (size_t)n_rec * 8, hipMemcpyDeviceToHost, st));
	if (perm_out) HIP_CHECK(hipMemcpyAsync(perm_out, dv.Current(), (size_t)n_rec * 4, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipEventRecord(s->rs.ev[6], st));
	HIP_CHECK(hipStreamSynchronize(st));
	for (int k = 0; k < 6; ++k) HIP_CHECK(hipEventElapsedTime(&s->ms[k], s->rs.ev[k], s->rs.ev[k + 1]));
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
