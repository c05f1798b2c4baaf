// nabwa_markdup.hip -- host side of duplicate marking of finished BAM records (nabwa_markdup*, include/nabwa.h): a handle that
// keeps its stream, its arena of tuples and its scratch between calls.
//
//   add:      upload bytes and offsets -> markdup_sig_kernel into the call's scratch -> the lowest damaged record comes down -> none:
//             markdup_emit_kernel appends the call's tuples to the arena and counts the classes; one: NABWA_EDATA, and the arena is as it was
//   resolve:  three stable radix sorts of (key, index) over the arena's columns, least significant first: k3 (pair bit, ~score, ordinal),
//             then lo, then hi -> markdup_mark_kernel -> markdup_prop_kernel -> dup[] and the counters come down
//
// The tuples stay on the device; the arena's columns are never sorted in place, so a resolve can follow more adds.  The host decides what
// it can from the arguments alone, before any device call.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <string.h>
#include "launchers.hpp"
#include "rec_stream.hpp"
#include "markdup_body.hpp"

#define MD_FIT "the records do not fit the device: a buffer of %lld bytes could not be had"

struct nabwa_markdup {
	RecStream rs;                                               /* h_words: n_tup, bad */
	nabwa_markdup_opt_t opt = {};
	DevBuf d_in, d_off, d_end, d_c3, d_score, d_meta;           /* a call: its bytes, its offsets, its scratch */
	DevBuf a_hi, a_lo, a_k3, a_link, d_dup;                     /* the arena: tuples, and a byte per ordinal twice */
	DevBuf d_cnt, d_stats;                                      /* n_tup and bad; the counters */
	DevBuf r_keys[2], r_idx[2], r_tmp;                          /* a resolve */
	int64_t cap_bytes = 0, cap_rec = 0, cap_tup = 0, cap_ord = 0, cap_res = 0, cap_dup = 0; size_t cap_tmp = 0;
	int64_t n_ord = 0, n_tup = 0;                               /* records and tuples added */
	float ms[5] = { 0, 0, 0, 0, 0 };
	~nabwa_markdup() { rs.quiesce(); }
};

extern "C" void nabwa_markdup_default_opt(nabwa_markdup_opt_t *o)
{
	if (!o) return;
	o->min_qual = 15; o->single_ends = NABWA_MARKDUP_ENDS_5P; o->exclude_flags = 0xB00; o->pad = 0;
}

extern "C" int nabwa_markdup_create(int device, const nabwa_markdup_opt_t *opt, nabwa_markdup_t **out)
{
	if (out) *out = nullptr;
	if (!opt || !out) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (opt->min_qual < 0 || opt->min_qual > 255) return fail_fmt(NABWA_EINVAL, "min_qual %lld: a base quality, 0 .. 255", opt->min_qual);
	if (opt->single_ends != NABWA_MARKDUP_ENDS_5P && opt->single_ends != NABWA_MARKDUP_ENDS_BOTH) return fail_fmt(NABWA_EINVAL, "single_ends %lld: NABWA_MARKDUP_ENDS_5P (0) or NABWA_MARKDUP_ENDS_BOTH (1)", opt->single_ends);
	nabwa_markdup_t *m = new nabwa_markdup_t;
	m->opt = *opt; m->opt.pad = 0;
	/* the persistent grid: eight workgroups of 256 fill a compute unit's wave slots */
	int r = m->rs.setup(device, 8, 2, 7, "setting up the duplicate marking");
	hipError_t e = hipSuccess;
	if (r == NABWA_OK) r = m->d_cnt.get(2 * sizeof(unsigned int));
	if (r == NABWA_OK) r = m->d_stats.get(NABWA_MARKDUP_N_STATS * 8);
	if (r == NABWA_OK) {
		e = hipMemsetAsync(m->d_cnt.p, 0, 2 * sizeof(unsigned int), m->rs.st);
		if (e == hipSuccess) e = hipMemsetAsync(m->d_stats.p, 0, NABWA_MARKDUP_N_STATS * 8, m->rs.st);
		if (e == hipSuccess) e = hipStreamSynchronize(m->rs.st);
		if (e != hipSuccess) r = nabwa_hip_fail(e, "setting up the duplicate marking", __FILE__, __LINE__);
	}
	if (r != NABWA_OK) { delete m; return r; }
	*out = m;
	return NABWA_OK;
}

extern "C" void nabwa_markdup_destroy(nabwa_markdup_t *m) { delete m; }

/* which kind of damage record i has, from its bytes on the host, for the message */
static int damaged(int64_t i, const uint8_t *rec, int64_t size)
{
	if (int r = rec_damaged_head(i, rec, size)) return r;
	REC_FIELDS(rec);
	uint64_t n_read = 0;
	for (uint32_t c = 0; c < n_cig; ++c) { const uint32_t w = rec_u32(rec + REC_MIN_REC + l_name + 4 * c); if (rec_op_read(w & 15u)) n_read += w >> 4; }
	if (L > 0 && n_read != L) return fail_fmt(NABWA_EDATA, "record %lld: its CIGAR does not consume its %lld bases", (long long)i, (long long)L);
	return fail_fmt(NABWA_EDATA, "record %lld: an unclipped end outside -2^30 .. 2^31 + 2^30", (long long)i);
}

extern "C" int nabwa_markdup_add(nabwa_markdup_t *m, int64_t n_rec, const uint8_t *in, const int64_t *in_off)
{
	if (!m) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (int r = rec_check_offsets(n_rec, in, in_off)) return r;
	if (n_rec == 0) return NABWA_OK;
	if (m->n_ord + n_rec > 0x7fffffff) return fail_fmt(NABWA_EINVAL, "%lld records after %lld: a handle takes 2147483647 between create / clear", (long long)n_rec, (long long)m->n_ord);
	const int64_t base = in_off[0], total = in_off[n_rec] - base;
	HIP_CHECK(hipSetDevice(m->rs.device));
	hipStream_t st = m->rs.st;
	unsigned int *h_cnt = m->rs.h_words;
	if (int r = rec_reserve(m->cap_bytes, total, 0, st, MD_FIT, { { &m->d_in, 1 } })) return r;
	if (int r = rec_reserve(m->cap_rec, n_rec, 0, st, MD_FIT, { { &m->d_off, 8 }, { &m->d_end, 8 }, { &m->d_c3, 4 }, { &m->d_score, 4 }, { &m->d_meta, 4 } }, 1)) return r;
	if (int r = rec_reserve(m->cap_ord, m->n_ord + n_rec, m->n_ord, st, MD_FIT, { { &m->a_link, 1 } })) return r;
	/* tuples: a fragment one, a pair of two records three */
	if (int r = rec_reserve(m->cap_tup, m->n_tup + (3 * n_rec + 1) / 2, m->n_tup, st, MD_FIT, { { &m->a_hi, 8 }, { &m->a_lo, 8 }, { &m->a_k3, 8 } })) return r;
	StreamDrain drain{ st };
	MdParams P;
	P.in = m->d_in.as<uint8_t>(); P.off = m->d_off.as<int64_t>(); P.base = base; P.n_rec = (int32_t)n_rec;
	P.min_qual = m->opt.min_qual; P.single_ends = m->opt.single_ends; P.exclude_flags = m->opt.exclude_flags;
	P.end = m->d_end.as<uint64_t>(); P.c3 = m->d_c3.as<uint32_t>(); P.score = m->d_score.as<uint32_t>(); P.meta = m->d_meta.as<uint32_t>();
	MdArena A;
	A.hi = m->a_hi.as<uint64_t>(); A.lo = m->a_lo.as<uint64_t>(); A.k3 = m->a_k3.as<uint64_t>(); A.link = m->a_link.as<uint8_t>();
	A.n_tup = m->d_cnt.as<unsigned int>(); A.stats = m->d_stats.as<unsigned long long>(); A.ord_base = (uint32_t)m->n_ord;
	unsigned int *d_bad = m->d_cnt.as<unsigned int>() + 1;
	h_cnt[1] = 0xffffffffu;
	if (int r = rec_upload(m->rs, m->d_in, m->d_off, d_bad, h_cnt + 1, 1, n_rec, in, in_off)) return r;
	nabwa_launch_markdup_sig(&P, rec_grid(n_rec, REC_GROUPS, m->rs.n_blocks), d_bad, st);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(m->rs.ev[2], st));
	HIP_CHECK(hipMemcpyAsync(h_cnt + 1, d_bad, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipStreamSynchronize(st));
	if (h_cnt[1] != 0xffffffffu) {
		const int64_t i = (int64_t)h_cnt[1];
		if (i >= n_rec) return fail_fmt(NABWA_EDATA, "record %lld is damaged", (long long)i);
		return damaged(i, in + in_off[i], in_off[i + 1] - in_off[i]);
	}
	HIP_CHECK(hipEventRecord(m->rs.ev[3], st));
	nabwa_launch_markdup_emit(&P, &A, st);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(m->rs.ev[4], st));
	HIP_CHECK(hipMemcpyAsync(h_cnt, m->d_cnt.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipStreamSynchronize(st));
	m->n_tup = (int64_t)h_cnt[0];
	m->n_ord += n_rec;
	float a = 0, b = 0;
	HIP_CHECK(hipEventElapsedTime(&m->ms[0], m->rs.ev[0], m->rs.ev[1]));
	HIP_CHECK(hipEventElapsedTime(&a, m->rs.ev[1], m->rs.ev[2]));
	HIP_CHECK(hipEventElapsedTime(&b, m->rs.ev[3], m->rs.ev[4]));
	m->ms[1] = a + b;
	return NABWA_OK;
}

extern "C" int nabwa_markdup_resolve(nabwa_markdup_t *m, uint8_t *dup, int64_t cap, uint64_t *stats)
{
	if (!m || cap < 0 || (cap > 0 && !dup)) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (cap < m->n_ord) return fail_fmt(NABWA_ECAP, "dup[] holds %lld records, %lld were added", (long long)cap, (long long)m->n_ord);
	HIP_CHECK(hipSetDevice(m->rs.device));
	hipStream_t st = m->rs.st;
	const int64_t n = m->n_tup, n_ord = m->n_ord;
	size_t tmp = 0;
	if (n) {
		hipcub::DoubleBuffer<uint64_t> dk(nullptr, nullptr); hipcub::DoubleBuffer<uint32_t> dv(nullptr, nullptr);
		HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, dk, dv, (int)n, 0, 64, st));
	}
	if (int r = rec_reserve(m->cap_res, n, 0, st, MD_FIT, { { &m->r_keys[0], 8 }, { &m->r_keys[1], 8 }, { &m->r_idx[0], 4 }, { &m->r_idx[1], 4 } })) return r;
	if (int r = rec_reserve_tmp(m->cap_tmp, tmp, m->r_tmp, st, MD_FIT)) return r;
	if (int r = rec_reserve(m->cap_dup, n_ord, 0, st, MD_FIT, { { &m->d_dup, 1 } })) return r;
	StreamDrain drain{ st };
	unsigned long long *d_stats = m->d_stats.as<unsigned long long>();
	HIP_CHECK(hipEventRecord(m->rs.ev[0], st));
	HIP_CHECK(hipMemsetAsync(d_stats + NABWA_MARKDUP_STAT_DUP_FRAGMENTS, 0, 3 * 8, st));
	if (n_ord) HIP_CHECK(hipMemsetAsync(m->d_dup.p, 0, (size_t)n_ord, st));
	hipcub::DoubleBuffer<uint64_t> dk(m->r_keys[0].as<uint64_t>(), m->r_keys[1].as<uint64_t>());
	hipcub::DoubleBuffer<uint32_t> dv(m->r_idx[0].as<uint32_t>(), m->r_idx[1].as<uint32_t>());
	if (n) {
		const uint64_t *cols[3] = { m->a_k3.as<uint64_t>(), m->a_lo.as<uint64_t>(), m->a_hi.as<uint64_t>() };
		nabwa_launch_markdup_iota(n, dv.Current(), st);
		HIP_CHECK(hipGetLastError());
		for (int k = 0; k < 3; ++k) {
			nabwa_launch_markdup_gather(n, dv.Current(), cols[k], dk.Current(), st);
			HIP_CHECK(hipGetLastError());
			size_t need = m->cap_tmp;
			HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(m->r_tmp.p, need, dk, dv, (int)n, 0, 64, st));
		}
	}
	HIP_CHECK(hipEventRecord(m->rs.ev[1], st));
	if (n) {
		nabwa_launch_markdup_mark(n, dv.Current(), m->a_hi.as<uint64_t>(), m->a_lo.as<uint64_t>(), m->a_k3.as<uint64_t>(), m->d_dup.as<uint8_t>(), d_stats, st);
		HIP_CHECK(hipGetLastError());
	}
	if (n_ord) {
		nabwa_launch_markdup_prop(n_ord, m->a_link.as<uint8_t>(), m->d_dup.as<uint8_t>(), d_stats, st);
		HIP_CHECK(hipGetLastError());
	}
	HIP_CHECK(hipEventRecord(m->rs.ev[2], st));
	if (n_ord) HIP_CHECK(hipMemcpyAsync(dup, m->d_dup.p, (size_t)n_ord, hipMemcpyDeviceToHost, st));
	uint64_t s[NABWA_MARKDUP_N_STATS];
	HIP_CHECK(hipMemcpyAsync(s, d_stats, sizeof s, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipEventRecord(m->rs.ev[3], st));
	HIP_CHECK(hipStreamSynchronize(st));
	if (stats) memcpy(stats, s, sizeof s);
	for (int k = 0; k < 3; ++k) HIP_CHECK(hipEventElapsedTime(&m->ms[2 + k], m->rs.ev[k], m->rs.ev[k + 1]));
	return NABWA_OK;
}

extern "C" int nabwa_markdup_clear(nabwa_markdup_t *m)
{
	if (!m) return nabwa_fail(NABWA_EINVAL, "null argument");
	HIP_CHECK(hipSetDevice(m->rs.device));
	HIP_CHECK(hipMemsetAsync(m->d_cnt.p, 0, 2 * sizeof(unsigned int), m->rs.st));
	HIP_CHECK(hipMemsetAsync(m->d_stats.p, 0, NABWA_MARKDUP_N_STATS * 8, m->rs.st));
	HIP_CHECK(hipStreamSynchronize(m->rs.st));
	m->n_ord = 0; m->n_tup = 0;
	return NABWA_OK;
}

extern "C" int nabwa_markdup_times(const nabwa_markdup_t *m, float ms[5])
{
	if (!m || !ms) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (int k = 0; k < 5; ++k) ms[k] = m->ms[k];
	return NABWA_OK;
}
