// nabwa_damage.hip -- host side of the damage profile of finished BAM records (nabwa_damage*, include/nabwa.h): a handle on an
// index that keeps its stream, its device buffers and its totals between calls.
//
//   upload bytes and offsets -> damage_kernel into the call's table (zeroed) -> the lowest damaged record comes down -> none: damage_add_kernel
//   puts the call's table onto the totals; one: NABWA_EDATA, and the totals are as they were
//
// The reference is the index's copy in HBM (nabwa_finish_reference: the one NABWA_FINISH=gpu reads); the contig offsets go up once, at create.
// The host decides what it can from the arguments alone, before any device call.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "launchers.hpp"
#include "rec_stream.hpp"
#include "finish_gpu.hpp"
#include "damage_body.hpp"

#define DMG_FIT "the call's records do not fit the device: a buffer of %lld bytes could not be had"

struct nabwa_damage {
	RecStream rs;                                          /* h_words: bad */
	nabwa_index_t *ix = nullptr;
	nabwa_damage_opt_t opt = {};
	DmgTab T = {};
	FinRef R = {};
	int n_contigs = 0;
	DevBuf d_in, d_off, d_contig, d_call, d_total, d_bad;
	int64_t cap_bytes = 0, cap_rec = 0;
	float ms[3] = { 0, 0, 0 };
	~nabwa_damage() { rs.quiesce(); }
};

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
	nabwa_damage_t *d = new nabwa_damage_t;
	/* the persistent grid: the flushes of a call are bounded by it, not by the records */
	int r = d->rs.setup(ix->device, 4, 1, 5, "setting up the damage profile");
	if (r == NABWA_OK) r = nabwa_finish_reference(ix, opt->which_ref, &d->R);
	if (r != NABWA_OK) { delete d; return r; }
	d->ix = ix; d->opt = *opt; d->opt.pad = 0; d->T = dmg_tab(opt->n_pos); d->n_contigs = (int)ref->anns.size();
	std::vector<int64_t> co((size_t)d->n_contigs + 1, 0);
	for (int i = 0; i < d->n_contigs; ++i) co[(size_t)i] = ref->anns[(size_t)i].offset;
	hipError_t e = hipSuccess;
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

/* which of the three kinds of damage record i has, from its bytes on the host, for the message */
static int damaged(int64_t i, const uint8_t *rec, int64_t size)
{
	if (int r = rec_damaged_head(i, rec, size)) return r;
	return fail_fmt(NABWA_EDATA, "record %lld: its CIGAR does not consume its %lld bases", (long long)i, (long long)rec_u32(rec + 20));
}

extern "C" int nabwa_damage_add(nabwa_damage_t *d, int64_t n_rec, const uint8_t *in, const int64_t *in_off)
{
	if (!d) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (int r = rec_check_offsets(n_rec, in, in_off)) return r;
	if (n_rec == 0) return NABWA_OK;
	const int64_t base = in_off[0], total = in_off[n_rec] - base;
	HIP_CHECK(hipSetDevice(d->rs.device));
	hipStream_t st = d->rs.st;
	if (int r = rec_reserve(d->cap_bytes, total, 0, st, DMG_FIT, { { &d->d_in, 1 } })) return r;
	if (int r = rec_reserve(d->cap_rec, n_rec, 0, st, DMG_FIT, { { &d->d_off, 8 } }, 1)) return r;
	StreamDrain drain{ st };
	DmgParams P;
	P.in = d->d_in.as<uint8_t>(); P.off = d->d_off.as<int64_t>(); P.base = base; P.n_rec = (int32_t)n_rec;
	P.n_contigs = d->n_contigs; P.contig_off = d->d_contig.as<int64_t>(); P.R = d->R;
	P.n_pos = d->opt.n_pos; P.min_mapq = d->opt.min_mapq; P.exclude_flags = d->opt.exclude_flags; P.require_flags = d->opt.require_flags;
	unsigned int *h_bad = d->rs.h_words;
	*h_bad = 0xffffffffu;
	if (int r = rec_upload(d->rs, d->d_in, d->d_off, d->d_bad.p, h_bad, 1, n_rec, in, in_off)) return r;
	HIP_CHECK(hipMemsetAsync(d->d_call.p, 0, (size_t)d->T.words * 8, st));
	nabwa_launch_damage(&P, rec_grid(n_rec, REC_GROUPS, d->rs.n_blocks), d->d_call.as<unsigned long long>(), d->d_bad.as<unsigned int>(), st);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(d->rs.ev[2], st));
	HIP_CHECK(hipMemcpyAsync(h_bad, d->d_bad.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipStreamSynchronize(st));
	if (*h_bad != 0xffffffffu) {
		const int64_t i = (int64_t)*h_bad;
		if (i >= n_rec) return fail_fmt(NABWA_EDATA, "record %lld is damaged", (long long)i);
		return damaged(i, in + in_off[i], in_off[i + 1] - in_off[i]);
	}
	HIP_CHECK(hipEventRecord(d->rs.ev[3], st));
	nabwa_launch_damage_add(d->T.words, d->d_call.as<unsigned long long>(), d->d_total.as<unsigned long long>(), st);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(d->rs.ev[4], st));
	HIP_CHECK(hipStreamSynchronize(st));
	for (int k = 0; k < 3; ++k) HIP_CHECK(hipEventElapsedTime(&d->ms[k], d->rs.ev[k < 2 ? k : 3], d->rs.ev[k < 2 ? k + 1 : 4]));
	return NABWA_OK;
}

extern "C" int nabwa_damage_fetch(nabwa_damage_t *d, uint64_t *sub5, uint64_t *sub3, uint64_t *len_hist, uint64_t *stats)
{
	if (!d) return nabwa_fail(NABWA_EINVAL, "null argument");
	HIP_CHECK(hipSetDevice(d->rs.device));
	std::vector<uint64_t> t((size_t)d->T.words);
	HIP_CHECK(hipMemcpyAsync(t.data(), d->d_total.p, t.size() * 8, hipMemcpyDeviceToHost, d->rs.st));
	HIP_CHECK(hipStreamSynchronize(d->rs.st));
	if (sub5) memcpy(sub5, t.data(), (size_t)d->T.sub3 * 8);
	if (sub3) memcpy(sub3, t.data() + d->T.sub3, (size_t)d->T.sub3 * 8);
	if (len_hist) memcpy(len_hist, t.data() + d->T.len, (size_t)NABWA_DAMAGE_LEN_BINS * 8);
	if (stats) memcpy(stats, t.data() + d->T.stats, (size_t)NABWA_DAMAGE_N_STATS * 8);
	return NABWA_OK;
}

extern "C" int nabwa_damage_clear(nabwa_damage_t *d)
{
	if (!d) return nabwa_fail(NABWA_EINVAL, "null argument");
	HIP_CHECK(hipSetDevice(d->rs.device));
	HIP_CHECK(hipMemsetAsync(d->d_total.p, 0, (size_t)d->T.words * 8, d->rs.st));
	HIP_CHECK(hipStreamSynchronize(d->rs.st));
	return NABWA_OK;
}

extern "C" int nabwa_damage_times(const nabwa_damage_t *d, float ms[3])
{
	if (!d || !ms) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (int k = 0; k < 3; ++k) ms[k] = d->ms[k];
	return NABWA_OK;
}
