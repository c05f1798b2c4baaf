// nabwa_bai.hip -- host side of the BAM index of finished, coordinate-sorted BAM records (nabwa_bai*, include/nabwa.h): a handle
// that keeps its stream, its arena of tuples and its scratch between calls.
//
//   add:     upload bytes and offsets -> bai_sig_kernel writes the call's tuples behind the arena's -> the lowest damaged record and the count
//            of records without a reference come down -> none damaged: the arena is that much longer; one: NABWA_EDATA, and it is as it was
//   finish:  upload the block table -> one stable radix sort of (tid << 16 | bin, ordinal) -> bai_ref_kernel (virtual offsets, per-reference
//            maxima) -> bai_head_kernel -> inclusive sum -> bai_place_kernel -> bai_refsize_kernel -> two exclusive sums -> the file's size and
//            the window count come down -> bai_lin_kernel into the reversed window table -> the backward fill as an inclusive scan ->
//            the three writer kernels -> the file comes down
//
// The tuples stay on the device and are never sorted in place, so a finish can follow more adds.  The host decides what it can from the
// arguments alone, before any device call.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <string.h>
#include "launchers.hpp"
#include "rec_stream.hpp"
#include "bai_body.hpp"

#define BAI_FIT "the records do not fit the device: a buffer of %lld bytes could not be had"
/* the handle's pinned words: bad and n_no_coor of a call, then three 64-bit totals of a finish (at a multiple of 8 bytes) */
enum { BAI_H_CNT = 2, BAI_H_TOT = 3, BAI_H_WORDS = BAI_H_CNT + 2 * BAI_H_TOT };
static_assert(BAI_H_CNT % 2 == 0, "h_tot lies at a multiple of 8 bytes");

struct nabwa_bai {
	RecStream rs;                                               /* h_words: bad, n_no_coor of a call; then h_tot */
	int32_t n_ref = 0;
	DevBuf d_in, d_off, d_cnt;                                  /* a call: its bytes, its offsets; bad and n_no_coor */
	DevBuf a_key, a_be, a_us, a_ue;                             /* the arena: a tuple per ordinal */
	DevBuf f_blk_u, f_blk_c, f_vb, f_ve, f_keys[2], f_idx[2], f_heads, f_sc, f_bin_c0, f_tmp, f_lin, f_out;      /* a finish */
	DevBuf r_i32[8], r_u64[4];                                  /* per reference: maxwin, unm, o0, o1, b0, b1, c0, c1; ref_size, ref_nintv, ref_off, lin_off */
	int64_t cap_bytes = 0, cap_rec = 0, cap_ord = 0, cap_blk = 0, cap_fin = 0, cap_lin = 0, cap_out = 0; size_t cap_tmp = 0;
	int64_t n_ord = 0, n_no_coor = 0;                           /* records added; those of them without a reference */
	int64_t first_start = 0, last_end = 0; uint64_t last_key = 0;      /* of the records added: where they start and end in the stream; the last one's key */
	unsigned long long *h_tot = nullptr;                        /* pinned, behind the BAI_H_CNT words of rs.h_words: the last scanned heads word, the file's bytes, the windows */
	float ms[7] = { 0, 0, 0, 0, 0, 0, 0 };
	~nabwa_bai() { rs.quiesce(); }
};

extern "C" int nabwa_bai_create(int device, int32_t n_ref, nabwa_bai_t **out)
{
	if (out) *out = nullptr;
	if (!out) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (n_ref < 0) return fail_fmt(NABWA_EINVAL, "n_ref %lld: the number of reference sequences", n_ref);
	nabwa_bai_t *b = new nabwa_bai_t;
	b->n_ref = n_ref;
	/* the persistent grid: eight workgroups of 256 fill a compute unit's wave slots */
	int r = b->rs.setup(device, 8, BAI_H_WORDS, 9, "setting up the BAM index");
	if (r == NABWA_OK) b->h_tot = (unsigned long long*)(b->rs.h_words + BAI_H_CNT);
	if (r == NABWA_OK) r = b->d_cnt.get(2 * sizeof(unsigned int));
	for (int k = 0; k < 8 && r == NABWA_OK; ++k) r = b->r_i32[k].get(((size_t)n_ref + 1) * 4);
	for (int k = 0; k < 4 && r == NABWA_OK; ++k) r = b->r_u64[k].get(((size_t)n_ref + 1) * 8);
	if (r != NABWA_OK) { delete b; return r; }
	*out = b;
	return NABWA_OK;
}

extern "C" void nabwa_bai_destroy(nabwa_bai_t *b) { delete b; }

/* which kind of damage record i has, from its bytes on the host, for the message.  before: the key of the record in front of it */
static int damaged(int64_t i, const uint8_t *rec, int64_t size, int32_t n_ref, uint64_t before)
{
	if (int r = rec_damaged_head(i, rec, size)) return r;
	REC_FIELDS(rec);
	const int32_t tid = ref_id;
	if (tid >= n_ref) return fail_fmt(NABWA_EDATA, "record %lld: reference %lld of %lld", (long long)i, (long long)tid, (long long)n_ref);
	if (tid >= 0 && pos < 0) return fail_fmt(NABWA_EDATA, "record %lld: position %lld on reference %lld", (long long)i, (long long)pos, (long long)tid);
	if (NABWA_BAM_SORT_KEY(tid, pos) < before) return fail_fmt(NABWA_EDATA, "record %lld: out of coordinate order (reference %lld, position %lld behind a higher one)", (long long)i, (long long)tid, (long long)pos);
	return fail_fmt(NABWA_EDATA, "record %lld: it ends behind 2^29, which a .bai cannot address (position %lld)", (long long)i, (long long)pos);
}
static uint64_t key_of(const uint8_t *rec)
{
	return NABWA_BAM_SORT_KEY((int32_t)rec_u32(rec + 4), (int32_t)rec_u32(rec + 8));
}

extern "C" int nabwa_bai_add(nabwa_bai_t *b, int64_t n_rec, const uint8_t *in, const int64_t *in_off, int64_t stream_off)
{
	if (!b) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (int r = rec_check_offsets(n_rec, in, in_off)) return r;
	if (stream_off < 0) return fail_fmt(NABWA_EINVAL, "stream_off %lld is negative", (long long)stream_off);
	if (b->n_ord && stream_off < b->last_end) return fail_fmt(NABWA_EINVAL, "stream_off %lld lies before the end of the records added so far, %lld", (long long)stream_off, (long long)b->last_end);
	if (n_rec == 0) return NABWA_OK;
	if (b->n_ord + n_rec > 0x7fffffff) return fail_fmt(NABWA_EINVAL, "%lld records after %lld: a handle takes 2147483647 between create / clear", (long long)n_rec, (long long)b->n_ord);
	const int64_t base = in_off[0], total = in_off[n_rec] - base;
	if (stream_off > INT64_MAX / 2 - total) return fail_fmt(NABWA_EINVAL, "stream_off %lld: no stream is that long", (long long)stream_off);
	HIP_CHECK(hipSetDevice(b->rs.device));
	(void)hipGetLastError();                                   /* (an error some earlier call of the process left behind is not a launch of this call's) */
	hipStream_t st = b->rs.st;
	if (int r = rec_reserve(b->cap_bytes, total, 0, st, BAI_FIT, { { &b->d_in, 1 } })) return r;
	if (int r = rec_reserve(b->cap_rec, n_rec, 0, st, BAI_FIT, { { &b->d_off, 8 } }, 1)) return r;
	if (int r = rec_reserve(b->cap_ord, b->n_ord + n_rec, b->n_ord, st, BAI_FIT, { { &b->a_key, 8 }, { &b->a_be, 8 }, { &b->a_us, 8 }, { &b->a_ue, 8 } })) return r;
	StreamDrain drain{ st };
	BaiParams P;
	P.in = b->d_in.as<uint8_t>(); P.off = b->d_off.as<int64_t>(); P.base = base; P.stream_off = stream_off; P.last_key = b->n_ord ? b->last_key : 0;
	P.n_rec = (int32_t)n_rec; P.n_ref = b->n_ref;
	P.key = b->a_key.as<uint64_t>() + b->n_ord; P.be = b->a_be.as<uint64_t>() + b->n_ord; P.us = b->a_us.as<int64_t>() + b->n_ord; P.ue = b->a_ue.as<uint64_t>() + b->n_ord;
	P.cnt = b->d_cnt.as<unsigned int>();
	unsigned int *h_cnt = b->rs.h_words;
	h_cnt[0] = 0xffffffffu; h_cnt[1] = 0;
	if (int r = rec_upload(b->rs, b->d_in, b->d_off, b->d_cnt.p, h_cnt, 2, n_rec, in, in_off)) return r;
	nabwa_launch_bai_sig(&P, rec_grid(n_rec, REC_GROUPS, b->rs.n_blocks), st);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(b->rs.ev[2], st));
	HIP_CHECK(hipMemcpyAsync(h_cnt, b->d_cnt.p, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipStreamSynchronize(st));
	if (h_cnt[0] != 0xffffffffu) {
		const int64_t i = (int64_t)h_cnt[0];
		if (i >= n_rec) return fail_fmt(NABWA_EDATA, "record %lld is damaged", (long long)i);
		return damaged(i, in + in_off[i], in_off[i + 1] - in_off[i], b->n_ref, i ? key_of(in + in_off[i - 1]) : P.last_key);
	}
	if (!b->n_ord) b->first_start = stream_off;
	b->n_ord += n_rec; b->n_no_coor += (int64_t)h_cnt[1];
	b->last_end = stream_off + total; b->last_key = key_of(in + in_off[n_rec - 1]);
	HIP_CHECK(hipEventElapsedTime(&b->ms[0], b->rs.ev[0], b->rs.ev[1]));
	HIP_CHECK(hipEventElapsedTime(&b->ms[1], b->rs.ev[1], b->rs.ev[2]));
	return NABWA_OK;
}

extern "C" int nabwa_bai_finish(nabwa_bai_t *b, int64_t n_blk, const int64_t *blk_uoff, const int64_t *blk_coff, uint8_t *out, int64_t cap, int64_t *n_out, uint64_t *stats)
{
	if (n_out) *n_out = 0;
	if (!b || !blk_uoff || !blk_coff || cap < 0 || (cap > 0 && !out)) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (n_blk < 0 || n_blk > 0x7ffffffe) return fail_fmt(NABWA_EINVAL, "n_blk %lld: 0 .. 2147483646 blocks before the end-of-file block", (long long)n_blk);
	if (blk_uoff[0] < 0 || blk_coff[0] < 0) return nabwa_fail(NABWA_EINVAL, "the block table starts below 0");
	for (int64_t k = 0; k < n_blk; ++k) {
		if (blk_uoff[k + 1] < blk_uoff[k]) return fail_fmt(NABWA_EINVAL, "blk_uoff falls at block %lld", (long long)k);
		if (blk_coff[k + 1] <= blk_coff[k]) return fail_fmt(NABWA_EINVAL, "blk_coff does not rise at block %lld", (long long)k);
		if (blk_uoff[k + 1] - blk_uoff[k] > 65536) return fail_fmt(NABWA_EINVAL, "block %lld holds %lld bytes: a BGZF block holds at most 65536", (long long)k, (long long)(blk_uoff[k + 1] - blk_uoff[k]));
	}
	if (blk_coff[n_blk] >= ((int64_t)1 << 48)) return fail_fmt(NABWA_EINVAL, "blk_coff reaches %lld: a virtual offset has 48 bits for it", (long long)blk_coff[n_blk]);
	if (b->n_ord && (b->first_start < blk_uoff[0] || b->last_end > blk_uoff[n_blk]))
		return fail_fmt(NABWA_EINVAL, "the records added lie at %lld .. %lld of the stream, the block table ends at %lld", (long long)b->first_start, (long long)b->last_end, (long long)blk_uoff[n_blk]);
	const int64_t n = b->n_ord - b->n_no_coor, n_ref = b->n_ref;
	HIP_CHECK(hipSetDevice(b->rs.device));
	(void)hipGetLastError();                                   /* (an error some earlier call of the process left behind is not a launch of this call's) */
	hipStream_t st = b->rs.st;
	int end_bit = 17;
	while (end_bit < 48 && ((int64_t)1 << (end_bit - 16)) < n_ref) ++end_bit;
	size_t tmp = 0, t2 = 0;
	if (n) {
		hipcub::DoubleBuffer<uint64_t> dk(nullptr, nullptr); hipcub::DoubleBuffer<uint32_t> dv(nullptr, nullptr);
		HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, dk, dv, (int)n, 0, end_bit, st));
		HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, t2, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n, st));
		tmp = t2 > tmp ? t2 : tmp;
	}
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n_ref + 1, st));
	tmp = t2 > tmp ? t2 : tmp;
	if (int r = rec_reserve(b->cap_blk, n_blk + 1, 0, st, BAI_FIT, { { &b->f_blk_u, 8 }, { &b->f_blk_c, 8 } })) return r;
	if (int r = rec_reserve(b->cap_fin, n, 0, st, BAI_FIT, { { &b->f_vb, 8 }, { &b->f_ve, 8 }, { &b->f_keys[0], 8 }, { &b->f_keys[1], 8 }, { &b->f_idx[0], 4 }, { &b->f_idx[1], 4 },
														 { &b->f_heads, 8 }, { &b->f_sc, 8 }, { &b->f_bin_c0, 4 } }, 1)) return r;
	if (int r = rec_reserve_tmp(b->cap_tmp, tmp, b->f_tmp, st, BAI_FIT)) return r;
	StreamDrain drain{ st };
	BaiFin F;
	memset(&F, 0, sizeof F);
	F.n = n; F.n_blk = n_blk; F.n_ref = (int32_t)n_ref; F.n_no_coor = (uint64_t)b->n_no_coor;
	F.key = b->a_key.as<uint64_t>(); F.be = b->a_be.as<uint64_t>(); F.us = b->a_us.as<int64_t>(); F.ue = b->a_ue.as<uint64_t>();
	F.blk_u = b->f_blk_u.as<int64_t>(); F.blk_c = b->f_blk_c.as<int64_t>();
	F.vb = b->f_vb.as<uint64_t>(); F.ve = b->f_ve.as<uint64_t>();
	F.maxwin = b->r_i32[0].as<int>(); F.unm = b->r_i32[1].as<unsigned int>(); F.o0 = b->r_i32[2].as<unsigned int>(); F.o1 = b->r_i32[3].as<unsigned int>();
	F.b0 = b->r_i32[4].as<unsigned int>(); F.b1 = b->r_i32[5].as<unsigned int>(); F.c0 = b->r_i32[6].as<unsigned int>(); F.c1 = b->r_i32[7].as<unsigned int>();
	F.heads = b->f_heads.as<unsigned long long>(); F.sc = b->f_sc.as<unsigned long long>(); F.bin_c0 = b->f_bin_c0.as<uint32_t>();
	F.ref_size = b->r_u64[0].as<unsigned long long>(); F.ref_nintv = b->r_u64[1].as<unsigned long long>();
	F.ref_off = b->r_u64[2].as<unsigned long long>(); F.lin_off = b->r_u64[3].as<unsigned long long>();
	HIP_CHECK(hipEventRecord(b->rs.ev[0], st));
	HIP_CHECK(hipMemcpyAsync(b->f_blk_u.p, blk_uoff, (size_t)(n_blk + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemcpyAsync(b->f_blk_c.p, blk_coff, (size_t)(n_blk + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemsetAsync(b->r_i32[0].p, 0xff, ((size_t)n_ref + 1) * 4, st));      /* maxwin: -1, a reference without records */
	for (int k = 1; k < 8; ++k) HIP_CHECK(hipMemsetAsync(b->r_i32[k].p, 0, ((size_t)n_ref + 1) * 4, st));
	hipcub::DoubleBuffer<uint64_t> dk(b->f_keys[0].as<uint64_t>(), b->f_keys[1].as<uint64_t>());
	hipcub::DoubleBuffer<uint32_t> dv(b->f_idx[0].as<uint32_t>(), b->f_idx[1].as<uint32_t>());
	b->h_tot[0] = 0;
	if (n) {
		HIP_CHECK(hipMemcpyAsync(dk.Current(), F.key, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
		nabwa_launch_bai_iota(n, dv.Current(), st);
		HIP_CHECK(hipGetLastError());
		size_t need = b->cap_tmp;
		HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(b->f_tmp.p, need, dk, dv, (int)n, 0, end_bit, st));
	}
	F.skey = dk.Current(); F.sidx = dv.Current();
	HIP_CHECK(hipEventRecord(b->rs.ev[1], st));
	if (n) {
		nabwa_launch_bai_step(NABWA_BAI_STEP_REF, &F, st);
		nabwa_launch_bai_step(NABWA_BAI_STEP_HEAD, &F, st);
		HIP_CHECK(hipGetLastError());
		size_t need = b->cap_tmp;
		HIP_CHECK(hipcub::DeviceScan::InclusiveSum(b->f_tmp.p, need, F.heads, F.sc, (int)n, st));
		nabwa_launch_bai_step(NABWA_BAI_STEP_PLACE, &F, st);
		HIP_CHECK(hipMemcpyAsync(b->h_tot, F.sc + (n - 1), 8, hipMemcpyDeviceToHost, st));
	}
	nabwa_launch_bai_step(NABWA_BAI_STEP_REFSIZE, &F, st);
	HIP_CHECK(hipGetLastError());
	{
		size_t need = b->cap_tmp;
		HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(b->f_tmp.p, need, F.ref_size, F.ref_off, (int)n_ref + 1, st));
		need = b->cap_tmp;
		HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(b->f_tmp.p, need, F.ref_nintv, F.lin_off, (int)n_ref + 1, st));
	}
	HIP_CHECK(hipMemcpyAsync(b->h_tot + 1, F.ref_off + n_ref, 8, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipMemcpyAsync(b->h_tot + 2, F.lin_off + n_ref, 8, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipEventRecord(b->rs.ev[2], st));
	HIP_CHECK(hipStreamSynchronize(st));
	const int64_t bytes = 8 + (int64_t)b->h_tot[1] + 8, n_lin = (int64_t)b->h_tot[2];
	if (stats) {
		stats[NABWA_BAI_STAT_RECORDS] = (uint64_t)b->n_ord; stats[NABWA_BAI_STAT_PLACED] = (uint64_t)n; stats[NABWA_BAI_STAT_NO_COOR] = (uint64_t)b->n_no_coor;
		stats[NABWA_BAI_STAT_BINS] = b->h_tot[0] >> 32; stats[NABWA_BAI_STAT_CHUNKS] = b->h_tot[0] & 0xffffffffu;
		stats[NABWA_BAI_STAT_WINDOWS] = (uint64_t)n_lin; stats[NABWA_BAI_STAT_BYTES] = (uint64_t)bytes;
	}
	if (n_out) *n_out = bytes;
	if (!out && cap == 0) return NABWA_OK;
	if (cap < bytes) return fail_fmt(NABWA_ECAP, "the index has %lld bytes, the buffer %lld", (long long)bytes, (long long)cap);
	if (n_lin > 0x7fffffff) return fail_fmt(NABWA_EINVAL, "%lld windows: a finish takes 2147483647", (long long)n_lin);
	if (int r = rec_reserve(b->cap_lin, n_lin, 0, st, BAI_FIT, { { &b->f_lin, 8 } })) return r;
	if (n_lin) {                                               /* the backward fill's scratch, now that the windows are known */
		HIP_CHECK(hipcub::DeviceScan::InclusiveScan(nullptr, t2, (unsigned long long*)nullptr, (unsigned long long*)nullptr, BaiNextTouched(), (int)n_lin, st));
		if (int r = rec_reserve_tmp(b->cap_tmp, t2, b->f_tmp, st, BAI_FIT)) return r;
	}
	if (int r = rec_reserve(b->cap_out, bytes, 0, st, BAI_FIT, { { &b->f_out, 1 } })) return r;
	F.n_lin = n_lin; F.lin = b->f_lin.as<unsigned long long>(); F.out = b->f_out.as<uint32_t>();
	HIP_CHECK(hipEventRecord(b->rs.ev[3], st));
	if (n_lin) {
		HIP_CHECK(hipMemsetAsync(b->f_lin.p, 0xff, (size_t)n_lin * 8, st));
		nabwa_launch_bai_step(NABWA_BAI_STEP_LIN, &F, st);
		HIP_CHECK(hipGetLastError());
		size_t need = b->cap_tmp;
		HIP_CHECK(hipcub::DeviceScan::InclusiveScan(b->f_tmp.p, need, F.lin, F.lin, BaiNextTouched(), (int)n_lin, st));
	}
	HIP_CHECK(hipEventRecord(b->rs.ev[4], st));
	nabwa_launch_bai_step(NABWA_BAI_STEP_WRITE_REF, &F, st);
	if (n) nabwa_launch_bai_step(NABWA_BAI_STEP_WRITE_TUPLE, &F, st);
	if (n_lin) nabwa_launch_bai_step(NABWA_BAI_STEP_WRITE_LIN, &F, st);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(b->rs.ev[5], st));
	HIP_CHECK(hipMemcpyAsync(out, b->f_out.p, (size_t)bytes, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipEventRecord(b->rs.ev[6], st));
	HIP_CHECK(hipStreamSynchronize(st));
	HIP_CHECK(hipEventElapsedTime(&b->ms[2], b->rs.ev[0], b->rs.ev[1]));
	HIP_CHECK(hipEventElapsedTime(&b->ms[3], b->rs.ev[1], b->rs.ev[2]));
	for (int k = 0; k < 3; ++k) HIP_CHECK(hipEventElapsedTime(&b->ms[4 + k], b->rs.ev[3 + k], b->rs.ev[4 + k]));
	return NABWA_OK;
}

extern "C" int nabwa_bai_clear(nabwa_bai_t *b)
{
	if (!b) return nabwa_fail(NABWA_EINVAL, "null argument");
	HIP_CHECK(hipSetDevice(b->rs.device));
	HIP_CHECK(hipStreamSynchronize(b->rs.st));
	b->n_ord = 0; b->n_no_coor = 0; b->first_start = 0; b->last_end = 0; b->last_key = 0;
	return NABWA_OK;
}

extern "C" int nabwa_bai_times(const nabwa_bai_t *b, float ms[7])
{
	if (!b || !ms) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (int k = 0; k < 7; ++k) ms[k] = b->ms[k];
	return NABWA_OK;
}
