// tests/emu/bai_emu.cpp -- TEST INFRASTRUCTURE ONLY.  The bodies of the BAM index (csrc/bai_body.hpp) compiled by g++ and run on the CPU as
// nabwa_bai.hip strings them together: the workgroups of the signature grid one after the other onto the arena, and for a finish one stable
// sort of the ordinals by (tid << 16 | bin), the per-reference pass, heads, their sum, places, sizes, the two exclusive sums, the window
// table with its backward fill as a scan of the reversed table, and the three writers.  Every buffer is exactly as long as the bodies may
// use it, so that AddressSanitizer sees a byte too many.
#define NABWA_EMU 1
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../../network-aware-bwa_amd/csrc/bai_body.hpp"

struct EmuBai {
	int32_t n_ref = 0;
	std::vector<uint64_t> key, be, ue;
	std::vector<int64_t> us;
	int64_t n_ord = 0, n_no_coor = 0;
	uint64_t last_key = 0;
};

extern "C" void *emu_bai_create(int32_t n_ref) { EmuBai *b = new EmuBai; b->n_ref = n_ref; return b; }
extern "C" void emu_bai_destroy(void *h) { delete (EmuBai*)h; }
static void shrink(EmuBai *b, size_t n) { b->key.resize(n); b->be.resize(n); b->us.resize(n); b->ue.resize(n); }
extern "C" void emu_bai_clear(void *h)
{
	EmuBai *b = (EmuBai*)h;
	shrink(b, 0); b->n_ord = 0; b->n_no_coor = 0; b->last_key = 0;
}

/* one call: -1 and the records added, or the lowest damaged record and the handle as it was.  n_blocks: the workgroups of the grid.  No
 * byte outside in[off[0], off[n]) is read. */
extern "C" int64_t emu_bai_add(void *h, int64_t n_rec, const uint8_t *in, const int64_t *off, int64_t stream_off, int n_blocks)
{
	EmuBai *b = (EmuBai*)h;
	if (n_rec == 0) return -1;
	shrink(b, (size_t)(b->n_ord + n_rec));
	unsigned int cnt[2] = { 0xffffffffu, 0 };
	BaiParams P;
	P.in = in + off[0]; P.off = off; P.base = off[0]; P.stream_off = stream_off; P.last_key = b->n_ord ? b->last_key : 0; P.n_rec = (int32_t)n_rec; P.n_ref = b->n_ref;
	P.key = b->key.data() + b->n_ord; P.be = b->be.data() + b->n_ord; P.us = b->us.data() + b->n_ord; P.ue = b->ue.data() + b->n_ord; P.cnt = cnt;
	for (int k = 0; k < n_blocks; ++k) {
		unsigned long long sum[BAI_GROUPS]; uint32_t state[BAI_GROUPS];
		memset(sum, 0xa5, sizeof sum); memset(state, 0xa5, sizeof state);      /* (LDS starts out as anything) */
		bai_block(P, sum, state, k, n_blocks);
		for (int g = 0; g < BAI_GROUPS; ++g) if (sum[g] || state[g] != BAI_ST_IDLE) return -2;      /* a workgroup leaves its words as it set them up */
	}
	if (cnt[0] != 0xffffffffu) { shrink(b, (size_t)b->n_ord); return (int64_t)cnt[0]; }
	const uint8_t *last = in + off[n_rec - 1];
	int32_t tid, pos;
	memcpy(&tid, last + 4, 4); memcpy(&pos, last + 8, 4);
	b->last_key = NABWA_BAM_SORT_KEY(tid, pos);
	b->n_ord += n_rec; b->n_no_coor += cnt[1];
	return -1;
}

/* the file for everything added, into out[0, cap) (out may be null: the size only), and stats[0, NABWA_BAI_N_STATS).  Returns the file's
 * size, or -2 where cap is below it */
extern "C" int64_t emu_bai_finish(void *h, int64_t n_blk, const int64_t *blk_u, const int64_t *blk_c, uint8_t *out, int64_t cap, uint64_t *stats)
{
	EmuBai *b = (EmuBai*)h;
	const int64_t n = b->n_ord - b->n_no_coor, n_ref = b->n_ref;
	std::vector<uint64_t> vb((size_t)n), ve((size_t)n), skey((size_t)n);
	std::vector<uint32_t> sidx((size_t)n), bin_c0((size_t)n + 1);
	std::vector<unsigned long long> heads((size_t)n), sc((size_t)n), ref_size((size_t)n_ref + 1), ref_nintv((size_t)n_ref + 1), ref_off((size_t)n_ref + 1), lin_off((size_t)n_ref + 1);
	std::vector<int> maxwin((size_t)n_ref, -1);
	std::vector<unsigned int> per[7];
	for (auto &v : per) v.assign((size_t)n_ref, 0);
	BaiFin F;
	memset(&F, 0, sizeof F);
	F.n = n; F.n_blk = n_blk; F.n_ref = (int32_t)n_ref; F.n_no_coor = (uint64_t)b->n_no_coor;
	F.key = b->key.data(); F.be = b->be.data(); F.us = b->us.data(); F.ue = b->ue.data(); F.blk_u = blk_u; F.blk_c = blk_c;
	F.vb = vb.data(); F.ve = ve.data(); F.maxwin = maxwin.data();
	F.unm = per[0].data(); F.o0 = per[1].data(); F.o1 = per[2].data(); F.b0 = per[3].data(); F.b1 = per[4].data(); F.c0 = per[5].data(); F.c1 = per[6].data();
	F.heads = heads.data(); F.sc = sc.data(); F.bin_c0 = bin_c0.data();
	F.ref_size = ref_size.data(); F.ref_nintv = ref_nintv.data(); F.ref_off = ref_off.data(); F.lin_off = lin_off.data();
	std::iota(sidx.begin(), sidx.end(), 0u);
	std::stable_sort(sidx.begin(), sidx.end(), [b](uint32_t x, uint32_t y) { return b->key[x] < b->key[y]; });
	for (int64_t j = 0; j < n; ++j) skey[(size_t)j] = b->key[sidx[(size_t)j]];
	F.skey = skey.data(); F.sidx = sidx.data();
	for (int64_t k = 0; k < (n + BAI_BLOCK - 1) / BAI_BLOCK; ++k) {
		int l_tid[BAI_BLOCK], l_win[BAI_BLOCK]; unsigned int l_unm[BAI_BLOCK];
		memset(l_tid, 0xa5, sizeof l_tid); memset(l_win, 0xa5, sizeof l_win); memset(l_unm, 0xa5, sizeof l_unm);
		bai_ref_block(F, l_tid, l_win, l_unm, k);
	}
	for (int64_t j = 0; j < n; ++j) bai_head_one(F, j);
	std::partial_sum(heads.begin(), heads.end(), sc.begin());
	for (int64_t j = n - 1; j >= 0; --j) bai_place_one(F, j);                  /* (the order of the lanes is no one's to rely on) */
	for (int64_t r = 0; r <= n_ref; ++r) bai_refsize_one(F, r);
	std::exclusive_scan(ref_size.begin(), ref_size.end(), ref_off.begin(), 0ull);
	std::exclusive_scan(ref_nintv.begin(), ref_nintv.end(), lin_off.begin(), 0ull);
	const int64_t bytes = 8 + (int64_t)ref_off[(size_t)n_ref] + 8, n_lin = (int64_t)lin_off[(size_t)n_ref];
	stats[NABWA_BAI_STAT_RECORDS] = (uint64_t)b->n_ord; stats[NABWA_BAI_STAT_PLACED] = (uint64_t)n; stats[NABWA_BAI_STAT_NO_COOR] = (uint64_t)b->n_no_coor;
	stats[NABWA_BAI_STAT_BINS] = n ? sc[(size_t)n - 1] >> 32 : 0; stats[NABWA_BAI_STAT_CHUNKS] = n ? sc[(size_t)n - 1] & 0xffffffffu : 0;
	stats[NABWA_BAI_STAT_WINDOWS] = (uint64_t)n_lin; stats[NABWA_BAI_STAT_BYTES] = (uint64_t)bytes;
	if (!out) return bytes;
	if (cap < bytes) return -2;
	std::vector<unsigned long long> lin((size_t)n_lin, BAI_UNTOUCHED);
	std::vector<uint32_t> file((size_t)bytes / 4, 0xa5a5a5a5u);
	F.n_lin = n_lin; F.lin = lin.data(); F.out = file.data();
	for (int64_t o = n - 1; o >= 0; --o) bai_lin_one(F, o);
	std::inclusive_scan(lin.begin(), lin.end(), lin.begin(), BaiNextTouched());
	for (int64_t r = 0; r <= n_ref; ++r) bai_write_ref(F, r);
	for (int64_t j = 0; j < n; ++j) bai_write_tuple(F, j);
	for (int64_t g = 0; g < n_lin; ++g) bai_write_lin(F, g);
	if (bytes) memcpy(out, file.data(), (size_t)bytes);
	return bytes;
}
