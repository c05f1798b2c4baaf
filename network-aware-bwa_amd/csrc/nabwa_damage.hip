// nabwa_damage.hip -- host side of the damage profile of finished BAM records (nabwa_damage*, include/nabwa.h): a handle on an
// index that keeps its stream, its device buffers and its totals between calls.
//
//   upload bytes and offsets -> damage_kernel into the call's table (zeroed) -> the lowest damaged record comes down -> none: damage_add_kernel
//   puts the call's table onto the totals; one: NABWA_EDATA, and the totals are as they were
//
// The reference is the index's copy in HBM (nabwa_finish_reference: the one NABWA_FINISH=gpu reads); the contig offsets go up once, at create.
// The host decides what it can from the arguments alone, before any device call.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/nabwa.h"
#include "launchers.hpp"
#include "nabwa_internal.hpp"
#include "dev_pool.hpp"
#include "finish_gpu.hpp"
#include "damage_body.hpp"

struct nabwa_damage {
	nabwa_index_t *ix = nullptr;
	nabwa_damage_opt_t opt = {};
	DmgTab T = {};
	FinRef R = {};
	int n_contigs = 0, n_blocks = 1;
	DevStream st;
	DevBuf d_in, d_off, d_contig, d_call, d_total, d_bad;
	int64_t cap_bytes = 0, cap_rec = 0;
	unsigned int *h_bad = nullptr;                         /* pinned */
	hipEvent_t ev[5] = {};
	float ms[3] = { 0, 0, 0 };
	~nabwa_damage()
	{
		(void)hipSetDevice(ix->device);
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

extern "C" void nabwa_damage_default_opt(nabwa_damage_opt_t *o)
{
	if (!o) return;
	o->n_pos = 25; o->min_mapq = 0; o->exclude_flags = 0xF04; o->require_flags = 0; o->which_ref = 0; o->pad = 0;
}

extern "C" int nabwa_damage_create(nabwa_index_t *ix, const nabwa_damage_opt_t *opt, nabwa_damage_t **out)
{
	if (out) *out = nullptr;
	if (!ix || !opt || !out) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (opt->n_pos < 1 || opt->n_pos > NABWA_DAMAGE_MAX_POS) return fail_fmt(NABWA_EINVAL, "n_pos %lld: 1 .. 256 positions from either end", opt->n_pos);      /* (before ix is looked at) */
	if (opt->which_ref < 0 || opt->which_ref > 1) return fail_fmt(NABWA_EINVAL, "which_ref %lld: 0 or 1", opt->which_ref);
	const nabwa_reference *ref = opt->which_ref ? ix->ref_nt : ix->ref;
	if (!ref || (opt->which_ref && !ix->d_ntpac))
		return nabwa_fail(NABWA_EINVAL, opt->which_ref ? "index has no nucleotide reference attached (nabwa_index_attach_nt_reference)" : "index has no reference attached (nabwa_index_attach_reference)");
	const hipError_t e0 = hipSetDevice(ix->device);
	if (e0 != hipSuccess) { (void)hipGetLastError(); return nabwa_hip_fail(e0, "hipSetDevice(device)", __FILE__, __LINE__); }
	FinRef R;
	if (const int r = nabwa_finish_reference(ix, opt->which_ref, &R)) return r;
	nabwa_damage_t *d = new nabwa_damage_t;
	d->ix = ix; d->opt = *opt; d->opt.pad = 0; d->T = dmg_tab(opt->n_pos); d->R = R; d->n_contigs = (int)ref->anns.size();
	std::vector<int64_t> co((size_t)d->n_contigs + 1, 0);
	for (int i = 0; i < d->n_contigs; ++i) co[(size_t)i] = ref->anns[(size_t)i].offset;
	int n_cu = 0;
	hipError_t e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ix->device);
	d->n_blocks = 4 * (n_cu > 0 ? n_cu : 1);              /* the persistent grid: the flushes of a call are bounded by it, not by the records */
	if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->st.s, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipHostMalloc((void**)&d->h_bad, sizeof(unsigned int), hipHostMallocDefault);
	for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipEventCreate(&d->ev[k]);
	int r = e == hipSuccess ? NABWA_OK : nabwa_hip_fail(e, "setting up the damage profile", __FILE__, __LINE__);
	const size_t tb = (size_t)d->T.words * 8;
	if (r == NABWA_OK) r = d->d_bad.get(sizeof(unsigned int));
	if (r == NABWA_OK) r = d->d_call.get(tb);
	if (r == NABWA_OK) r = d->d_total.get(tb);
	if (r == NABWA_OK) r = d->d_contig.get(co.size() * 8);
	if (r == NABWA_OK) {
		e = hipMemcpy(d->d_contig.p, co.data(), co.size() * 8, hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipMemset(d->d_total.p, 0, tb);
		if (e == hipSuccess) e = hipDeviceSynchronize();      /* the reference and the contigs are there before the handle's own stream reads them */
		if (e != hipSuccess) r = nabwa_hip_fail(e, "setting up the damage profile", __FILE__, __LINE__);
	}
	if (r != NABWA_OK) { delete d; return r; }
	*out = d;
	return NABWA_OK;
}

extern "C" void nabwa_damage_destroy(nabwa_damage_t *d) { delete d; }

/* a buffer of at least `bytes`; out of device memory is the caller's to act on (a smaller call) */
static int dmg_get(DevBuf &b, size_t bytes)
{
	const hipError_t e = b.release();
	if (e != hipSuccess) return nabwa_hip_fail(e, "hipFree", __FILE__, __LINE__);
	const hipError_t m = hipMalloc(&b.p, bytes ? bytes : 1);
	if (m == hipErrorOutOfMemory) { (void)hipGetLastError(); b.p = nullptr; return fail_fmt(NABWA_ENOMEM, "the call's records do not fit the device: a buffer of %lld bytes could not be had", (long long)bytes); }
	if (m != hipSuccess) { b.p = nullptr; return nabwa_hip_fail(m, "hipMalloc", __FILE__, __LINE__); }
	return NABWA_OK;
}

/* which of the three kinds of damage record i has, from its bytes on the host, for the message */
static int damaged(int64_t i, const uint8_t *rec, int64_t size)
{
	uint32_t bs, w12, w16, L;
	memcpy(&bs, rec, 4); memcpy(&w12, rec + 12, 4); memcpy(&w16, rec + 16, 4); memcpy(&L, rec + 20, 4);
	if ((int64_t)bs + 4 != size) return fail_fmt(NABWA_EDATA, "record %lld: its block_size says %lld bytes, its offsets %lld", (long long)i, (long long)bs + 4, (long long)size);
	const uint64_t need = (uint64_t)DMG_MIN_REC + (w12 & 0xffu) + 4 * (uint64_t)(w16 & 0xffffu) + ((uint64_t)L + 1) / 2 + L;
	if (need > (uint64_t)size) return fail_fmt(NABWA_EDATA, "record %lld: its name, CIGAR, bases and qualities need %lld bytes, it has %lld", (long long)i, (long long)need, (long long)size);
	return fail_fmt(NABWA_EDATA, "record %lld: its CIGAR does not consume its %lld bases", (long long)i, (long long)L);
}

extern "C" int nabwa_damage_add(nabwa_damage_t *d, int64_t n_rec, const uint8_t *in, const int64_t *in_off)
{
	if (!d) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (n_rec < 0 || n_rec > 0x7fffffff) return fail_fmt(NABWA_EINVAL, "n_rec %lld: 0 .. 2147483647 records", (long long)n_rec);
	if (!in_off || (n_rec && !in)) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (in_off[0] < 0) return nabwa_fail(NABWA_EINVAL, "the first offset is negative");
	for (int64_t i = 0; i < n_rec; ++i) {
		if (in_off[i + 1] <= in_off[i]) return fail_fmt(NABWA_EINVAL, "the offsets do not increase at record %lld", (long long)i);
		if (in_off[i + 1] - in_off[i] < DMG_MIN_REC) return fail_fmt(NABWA_EINVAL, "record %lld has %lld bytes: a BAM record has at least 36", (long long)i, (long long)(in_off[i + 1] - in_off[i]));
	}
	if (n_rec == 0) return NABWA_OK;
	const int64_t base = in_off[0], total = in_off[n_rec] - base;
	HIP_CHECK(hipSetDevice(d->ix->device));
	hipStream_t st = d->st;
	if (total > d->cap_bytes || n_rec > d->cap_rec) {      /* the buffers only grow (by a quarter more than asked, as the sort's) */
		HIP_CHECK(hipStreamSynchronize(st));
		if (total > d->cap_bytes) { d->cap_bytes = 0; const int64_t want = total + total / 4; if (int r = dmg_get(d->d_in, (size_t)want)) return r; d->cap_bytes = want; }
		if (n_rec > d->cap_rec) { d->cap_rec = 0; const int64_t want = n_rec + n_rec / 4; if (int r = dmg_get(d->d_off, (size_t)(want + 1) * 8)) return r; d->cap_rec = want; }
	}
	StreamDrain drain{ st };
	DmgParams P;
	P.in = d->d_in.as<uint8_t>(); P.off = d->d_off.as<int64_t>(); P.base = base; P.n_rec = (int32_t)n_rec;
	P.n_contigs = d->n_contigs; P.contig_off = d->d_contig.as<int64_t>(); P.R = d->R;
	P.n_pos = d->opt.n_pos; P.min_mapq = d->opt.min_mapq; P.exclude_flags = d->opt.exclude_flags; P.require_flags = d->opt.require_flags;
	*d->h_bad = 0xffffffffu;
	HIP_CHECK(hipEventRecord(d->ev[0], st));
	HIP_CHECK(hipMemcpyAsync(d->d_in.p, in + base, (size_t)total, hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemcpyAsync(d->d_off.p, in_off, (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemcpyAsync(d->d_bad.p, d->h_bad, sizeof(unsigned int), hipMemcpyHostToDevice, st));
	HIP_CHECK(hipEventRecord(d->ev[1], st));
	HIP_CHECK(hipMemsetAsync(d->d_call.p, 0, (size_t)d->T.words * 8, st));
	const int64_t trips = (n_rec + DMG_GROUPS - 1) / DMG_GROUPS;
	nabwa_launch_damage(&P, (int)(trips < d->n_blocks ? trips : d->n_blocks), d->d_call.as<unsigned long long>(), d->d_bad.as<unsigned int>(), st);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(d->ev[2], st));
	HIP_CHECK(hipMemcpyAsync(d->h_bad, d->d_bad.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipStreamSynchronize(st));
	if (*d->h_bad != 0xffffffffu) {
		const int64_t i = (int64_t)*d->h_bad;
		if (i >= n_rec) return fail_fmt(NABWA_EDATA, "record %lld is damaged", (long long)i);
		return damaged(i, in + in_off[i], in_off[i + 1] - in_off[i]);
	}
	HIP_CHECK(hipEventRecord(d->ev[3], st));
	nabwa_launch_damage_add(d->T.words, d->d_call.as<unsigned long long>(), d->d_total.as<unsigned long long>(), st);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(d->ev[4], st));
	HIP_CHECK(hipStreamSynchronize(st));
	for (int k = 0; k < 3; ++k) HIP_CHECK(hipEventElapsedTime(&d->ms[k], d->ev[k < 2 ? k : 3], d->ev[k < 2 ? k + 1 : 4]));
	return NABWA_OK;
}

extern "C" int nabwa_damage_fetch(nabwa_damage_t *d, uint64_t *sub5, uint64_t *sub3, uint64_t *len_hist, uint64_t *stats)
{
	if (!d) return nabwa_fail(NABWA_EINVAL, "null argument");
	HIP_CHECK(hipSetDevice(d->ix->device));
	std::vector<uint64_t> t((size_t)d->T.words);
	HIP_CHECK(hipMemcpyAsync(t.data(), d->d_total.p, t.size() * 8, hipMemcpyDeviceToHost, d->st));
	HIP_CHECK(hipStreamSynchronize(d->st));
	if (sub5) memcpy(sub5, t.data(), (size_t)d->T.sub3 * 8);
	if (sub3) memcpy(sub3, t.data() + d->T.sub3, (size_t)d->T.sub3 * 8);
	if (len_hist) memcpy(len_hist, t.data() + d->T.len, (size_t)NABWA_DAMAGE_LEN_BINS * 8);
	if (stats) memcpy(stats, t.data() + d->T.stats, (size_t)NABWA_DAMAGE_N_STATS * 8);
	return NABWA_OK;
}

extern "C" int nabwa_damage_clear(nabwa_damage_t *d)
{
	if (!d) return nabwa_fail(NABWA_EINVAL, "null argument");
	HIP_CHECK(hipSetDevice(d->ix->device));
	HIP_CHECK(hipMemsetAsync(d->d_total.p, 0, (size_t)d->T.words * 8, d->st));
	HIP_CHECK(hipStreamSynchronize(d->st));
	return NABWA_OK;
}

extern "C" int nabwa_damage_times(const nabwa_damage_t *d, float ms[3])
{
	if (!d || !ms) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (int k = 0; k < 3; ++k) ms[k] = d->ms[k];
	return NABWA_OK;
}
