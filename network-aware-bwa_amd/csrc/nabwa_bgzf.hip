// nabwa_bgzf.hip -- the host side of the BGZF compressor (kernels: bgzf_deflate.hip) and decompressor (bgzf_inflate.hip): a handle that keeps its stream, its device buffers
// and its pinned staging buffers between calls, and the one-shot entry, which is the handle used once.  Input goes through in rounds
// of at most 1040 slices (64.7 MB, so that the 64 MB the tool's writer collects are one round; more slices are dealt evenly over
// the rounds they need): pageable -> pinned -> HBM, one block per slice, packed on the device, and only the packed bytes come back.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/nabwa.h"
#include "nabwa_internal.hpp"
#include "dev_pool.hpp"
#include "launchers.hpp"
#include "bgzf_inflate_body.hpp"                   /* BgzfInBlk, the status words */

#define SLICE  ((int64_t)0xff00)
#define STRIDE ((int64_t)0x10000)
#define CHUNK  ((int64_t)1040)                        /* slices per launch, at most */
#define INFLATE_ROUND ((int64_t)256 << 20)            /* inflated bytes per launch of the decompressor, at most */

struct nabwa_bgzf {
	int device = 0;
	int64_t cap = 0;                                   /* slices the buffers hold */
	DevStream st;
	DevBuf d_in, d_stage, d_packed, d_sizes, d_total;
	uint8_t *h_in = nullptr, *h_out = nullptr; int64_t *h_total = nullptr;      /* pinned */
	/* the decompressor's: device buffers that grow and stay, and what a round may hold at most */
	DevBuf i_cmp, i_plain, i_blk, i_status;
	int64_t i_cmp_cap = 0, i_plain_cap = 0, i_blk_cap = 0, i_status_cap = 0, i_round = 0;
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
	/* a round of the decompressor holds members of at most this many inflated bytes (one member always goes); the variable lowers
	 * it, so that a test reaches several rounds with a small input */
	z->i_round = INFLATE_ROUND;
	if (const char *e = getenv("NABWA_BGZF_INFLATE_CAP")) { const long long v = atoll(e); if (v > 0 && v < INFLATE_ROUND) z->i_round = v; }
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

extern "C" int nabwa_bgzf_handle_compress_ex(nabwa_bgzf_t *z, int codes, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks)
{
	if (!z || n < 0 || cap < 0 || (n && !in) || (cap && !out)) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (codes != NABWA_BGZF_CODES_FIXED && codes != NABWA_BGZF_CODES_DYNAMIC) return nabwa_fail(NABWA_EINVAL, "codes: NABWA_BGZF_CODES_FIXED or NABWA_BGZF_CODES_DYNAMIC");
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
		(codes == NABWA_BGZF_CODES_DYNAMIC ? nabwa_launch_bgzf_deflate_dyn : nabwa_launch_bgzf_deflate)(z->d_in.as<uint8_t>(), m, ns, z->d_stage.as<uint8_t>(), z->d_sizes.as<uint32_t>(), z->st);
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

extern "C" int nabwa_bgzf_handle_compress(nabwa_bgzf_t *z, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks)
{
	return nabwa_bgzf_handle_compress_ex(z, NABWA_BGZF_CODES_FIXED, in, n, out, cap, n_out, n_blocks);
}

extern "C" int nabwa_bgzf_compress_ex(int device, int codes, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks)
{
	if (codes != NABWA_BGZF_CODES_FIXED && codes != NABWA_BGZF_CODES_DYNAMIC) return nabwa_fail(NABWA_EINVAL, "codes: NABWA_BGZF_CODES_FIXED or NABWA_BGZF_CODES_DYNAMIC");
	nabwa_bgzf_t *z = nullptr;
	if (int r = nabwa_bgzf_create(device, &z)) return r;
	const int r = nabwa_bgzf_handle_compress_ex(z, codes, in, n, out, cap, n_out, n_blocks);
	nabwa_bgzf_destroy(z);
	return r;
}

extern "C" int nabwa_bgzf_compress(int device, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks)
{
	return nabwa_bgzf_compress_ex(device, NABWA_BGZF_CODES_FIXED, in, n, out, cap, n_out, n_blocks);
}

/* ---------------------------------------------------------------- the decompressor */
static const char *const INFLATE_WHY[BGZI_N_STATUS] = {
	"ok", "a deflate block of type 11", "a stored block whose LEN and NLEN disagree", "the payload ends before the final block's end code",
	"an over-subscribed set of code lengths", "an incomplete set of code lengths", "repeat code 16 with no length before it",
	"code lengths that run past HLIT + HDIST", "no code for the end of block", "a literal/length symbol above 285 or a distance symbol above 29",
	"a distance that reaches before the member's first byte", "more output than ISIZE", "less output than ISIZE", "the CRC-32 is not the trailer's",
	"too many length or distance codes", "bits that are no code", "the decoder's bound was reached" };

static int edata(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int edata(const char *fmt, ...)
{
	char b[512];
	va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
	return nabwa_fail(NABWA_EDATA, "%s", b);
}

/* the members of in[0, n): their table entries (blk may be null), the sum of ISIZE and their number.  src and dst count from the start
 * of the input and of the output */
static int bgzf_walk(const uint8_t *in, int64_t n, std::vector<BgzfInBlk> *blk, int64_t *n_out, int64_t *n_blocks)
{
	int64_t o = 0, out = 0, k = 0;
	while (o < n) {
		const uint8_t *h = in + o;
		const int64_t left = n - o;
		if (left < 18) return edata("BGZF member %lld at byte %lld: %lld bytes are no whole header", (long long)k, (long long)o, (long long)left);
		if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return edata("BGZF member %lld at byte %lld: not a gzip header with an extra field", (long long)k, (long long)o);
		const int64_t xlen = h[10] | (int64_t)h[11] << 8;
		if (left < 12 + xlen) return edata("BGZF member %lld at byte %lld: the extra field runs past the input", (long long)k, (long long)o);
		int64_t total = 0;
		for (int64_t q = 12; q + 4 <= 12 + xlen; ) {
			const int64_t sl = h[q + 2] | (int64_t)h[q + 3] << 8;
			if (h[q] == 'B' && h[q + 1] == 'C' && sl == 2 && q + 6 <= 12 + xlen) { total = (int64_t)(h[q + 4] | (int64_t)h[q + 5] << 8) + 1; break; }
			q += 4 + sl;
		}
		if (total < 12 + xlen + 8) return edata("BGZF member %lld at byte %lld: no BC field, or a BSIZE smaller than the header", (long long)k, (long long)o);
		if (total > left) return edata("BGZF member %lld at byte %lld: BSIZE says %lld bytes, the input has %lld", (long long)k, (long long)o, (long long)total, (long long)left);
		BgzfInBlk b; b.src = (uint64_t)(o + 12 + xlen); b.dst = (uint64_t)out; b.n_src = (uint32_t)(total - 12 - xlen - 8); b.pad = 0;
		memcpy(&b.crc, h + total - 8, 4); memcpy(&b.isize, h + total - 4, 4);
		if (b.isize > 0x10000u) return edata("BGZF member %lld at byte %lld: ISIZE %u is more than 64 KB", (long long)k, (long long)o, b.isize);
		if (blk) blk->push_back(b);
		out += b.isize; o += total; ++k;
	}
	if (n_out) *n_out = out;
	if (n_blocks) *n_blocks = k;
	return NABWA_OK;
}

extern "C" int nabwa_bgzf_inflated_size(const uint8_t *in, int64_t n, int64_t *n_out, int64_t *n_blocks)
{
	if (n < 0 || (n && !in)) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (n_out) *n_out = 0;
	if (n_blocks) *n_blocks = 0;
	return bgzf_walk(in, n, nullptr, n_out, n_blocks);
}

extern "C" int nabwa_bgzf_block_table(const uint8_t *in, int64_t n, int64_t *blk_uoff, int64_t *blk_coff, int64_t cap, int64_t *n_blk)
{
	if (n < 0 || (n && !in) || cap < 0 || !n_blk) return nabwa_fail(NABWA_EINVAL, "null argument");
	*n_blk = 0;
	std::vector<BgzfInBlk> blk;
	if (int r = bgzf_walk(in, n, &blk, nullptr, nullptr)) return r;
	if (blk.empty()) return edata("no BGZF member: %lld bytes", (long long)n);
	if (blk.back().isize != 0) return edata("BGZF member %lld, the last, is no end-of-file block: ISIZE %lld", (long long)blk.size() - 1, (long long)blk.back().isize);
	*n_blk = (int64_t)blk.size() - 1;
	if ((blk_uoff || blk_coff) && cap < (int64_t)blk.size()) return nabwa_fail(NABWA_ECAP, "the block table needs one entry per BGZF member (*n_blk + 1)");
	int64_t at = 0;                                    /* where member k starts: behind the trailer of the one before */
	for (size_t k = 0; k < blk.size(); ++k) {
		if (blk_uoff) blk_uoff[k] = (int64_t)blk[k].dst;
		if (blk_coff) blk_coff[k] = at;
		at = (int64_t)(blk[k].src + blk[k].n_src + 8);
	}
	return NABWA_OK;
}

static int inflate_grow(nabwa_bgzf *z, DevBuf &b, int64_t &cap, int64_t want)
{
	if (want <= cap) return NABWA_OK;
	HIP_CHECK(hipStreamSynchronize(z->st));
	cap = 0;
	HIP_CHECK(b.release());
	want += want / 4;                                  /* the next call's fill is about as large: no growth by a few bytes each time */
	if (int r = b.get((size_t)want)) return r;
	cap = want;
	return NABWA_OK;
}

extern "C" int nabwa_bgzf_handle_decompress(nabwa_bgzf_t *z, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks)
{
	if (!z || n < 0 || cap < 0 || (n && !in) || (cap && !out)) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (n_out) *n_out = 0;
	if (n_blocks) *n_blocks = 0;
	std::vector<BgzfInBlk> blk;
	int64_t total = 0, nb = 0;
	if (int r = bgzf_walk(in, n, &blk, &total, &nb)) return r;
	if (n_out) *n_out = total;
	if (n_blocks) *n_blocks = nb;
	if (total > cap) return nabwa_fail(NABWA_ECAP, "the output buffer is too small for the inflated bytes (*n_out says how much is needed)");
	if (nb == 0) return NABWA_OK;
	HIP_CHECK(hipSetDevice(z->device));
	StreamDrain drain{ z->st };
	std::vector<uint32_t> status;
	for (size_t k0 = 0; k0 < blk.size(); ) {
		/* a round: members k0 .. k1 - 1, at most i_round inflated bytes (one member at least); their compressed bytes, headers between
		 * them included, and their output are one stretch each */
		size_t k1 = k0 + 1;
		while (k1 < blk.size() && (int64_t)(blk[k1].dst + blk[k1].isize - blk[k0].dst) <= z->i_round) ++k1;
		const uint64_t c0 = blk[k0].src, c1 = blk[k1 - 1].src + blk[k1 - 1].n_src, p0 = blk[k0].dst, p1 = blk[k1 - 1].dst + blk[k1 - 1].isize;
		const int nk = (int)(k1 - k0);
		std::vector<BgzfInBlk> rel(blk.begin() + k0, blk.begin() + k1);
		for (BgzfInBlk &b : rel) { b.src -= c0; b.dst -= p0; }      /* src + n_src <= c1 - c0 and dst + isize <= p1 - p0: inside the buffers below */
		if (int r = inflate_grow(z, z->i_cmp, z->i_cmp_cap, (int64_t)(c1 - c0))) return r;
		if (int r = inflate_grow(z, z->i_plain, z->i_plain_cap, (int64_t)(p1 - p0))) return r;
		if (int r = inflate_grow(z, z->i_blk, z->i_blk_cap, (int64_t)nk * (int64_t)sizeof(BgzfInBlk))) return r;
		if (int r = inflate_grow(z, z->i_status, z->i_status_cap, (int64_t)nk * 4)) return r;
		if (c1 > c0) HIP_CHECK(hipMemcpyAsync(z->i_cmp.p, in + c0, (size_t)(c1 - c0), hipMemcpyHostToDevice, z->st));
		HIP_CHECK(hipMemcpyAsync(z->i_blk.p, rel.data(), (size_t)nk * sizeof(BgzfInBlk), hipMemcpyHostToDevice, z->st));
		HIP_CHECK(hipStreamSynchronize(z->st));            /* rel is pageable: the copy has left it before it goes */
		nabwa_launch_bgzf_inflate(z->i_cmp.as<uint8_t>(), z->i_blk.as<BgzfInBlk>(), nk, z->i_plain.as<uint8_t>(), z->i_status.as<uint32_t>(), z->st);
		HIP_CHECK(hipGetLastError());
		status.assign((size_t)nk, 0xffffffffu);
		HIP_CHECK(hipMemcpyAsync(status.data(), z->i_status.p, (size_t)nk * 4, hipMemcpyDeviceToHost, z->st));
		if (p1 > p0) HIP_CHECK(hipMemcpyAsync(out + p0, z->i_plain.p, (size_t)(p1 - p0), hipMemcpyDeviceToHost, z->st));
		HIP_CHECK(hipStreamSynchronize(z->st));
		for (int i = 0; i < nk; ++i)
			if (status[i] != BGZI_OK) {
				const BgzfInBlk &b = blk[k0 + i];
				return edata("BGZF member %lld (payload at byte %lld) does not inflate to what its trailer says: %s",
								  (long long)(k0 + i), (long long)b.src, status[i] < BGZI_N_STATUS ? INFLATE_WHY[status[i]] : "a status that cannot be");
			}
		k0 = k1;
	}
	return NABWA_OK;
}

extern "C" int nabwa_bgzf_decompress(int device, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks)
{
	nabwa_bgzf_t *z = nullptr;
	if (int r = nabwa_bgzf_create(device, &z)) return r;
	const int r = nabwa_bgzf_handle_decompress(z, in, n, out, cap, n_out, n_blocks);
	nabwa_bgzf_destroy(z);
	return r;
}
