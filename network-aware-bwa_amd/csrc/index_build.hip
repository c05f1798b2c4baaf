// index_build.hip -- the GPU half of `bwa index`: <prefix>.pac in, <prefix>.bwt / .rbwt / .sa / .rsa out, the words the
// reference writes (bwt_dump_bwt / bwt_dump_sa, bwtio.c:161-182; the Occ-interleaved layout of bwt_bwtupdate_core,
// bwtmisc.c:125-152; bwt_cal_sa with sa_intv 32, bwtindex.c:173,185).  The suffix array of text+'$' is unique, so any
// correct construction writes the same bytes whichever of `-a is` / `-a bwtsw` the reference would have used.
//
// Per direction (the reverse index is built over the REVERSED text, not its complement; the reversal runs on the device):
//   1. sort key of every suffix i = its first 29 bases (58 bits, read straight from the packed text: two 64-bit loads and
//      a funnel shift) << 5 | min(29, n - i); '$' sorts first because a shorter suffix carries a smaller count
//   2. one 63-bit radix sort of (key, i) -> rows in 29-base order; group starts by a max-scan over "key differs" heads
//   3. prefix doubling (h = 29, 58, 116, ...) over the rows still tied: (group start, rank[i + h]) sorted per round, only
//      those rows selected, until none is tied.  h > n is an error, not a spin.
//   4. BWT byte per row, packed 16 bases a word with the 4 Occ counts every 128 rows, the '$' row left out (primary);
//      sampled SA every sa_intv rows.
//
// Memory plan (m = n + 1 rows, bytes per row):  step 1-2: keys 2 x 8 + values 2 x 4 = 24, + radix-sort scratch;
// step 2 tail: sorted keys 8 + SA 4 + spare value buffer 4 (the heads) + rank 4 + group start 4 + tied flag 1 = 25;
// step 3: SA + rank + group start + tied + selected rows = 17, + 24 per tied row (keys 2 x 8, values 2 x 4) + scratch.
// Nothing bounds the tied rows but m, so the estimate checked before the first allocation is the worst case,
// 41 B/row + sort scratch + the two packed texts; it is compared with hipMemGetInfo (and NABWA_INDEX_MAX_BYTES when set).
// Every device allocation goes through one arena that frees whatever is left on every return path.
//
// Length limit: the SA is u32 and has n + 1 rows; n must stay below 0xFFFFFFF0 (the reference's own limit is n < 2^32).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>
#include "nabwa_internal.hpp"
#include "../../include/nabwa.h"

#define IX_GRID(n) dim3((unsigned)(((n) + 255) / 256 < 65536 * 16 ? ((n) + 255) / 256 : 65536 * 16)), dim3(256)
#define IX_FOR_ALL(i, n) for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (n); i += (size_t)gridDim.x * 256)
#define KCH 29                               // bases in the first sort key: 58 bits + 5 bits of "valid" count
#define IX_MAX_N 0xFFFFFF80ull               // longest text the reference indexes: above it n_occ = (n + 127)/128 + 1 wraps in 32 bits (bwtmisc.c:131)

static int ix_fail(int code, const std::string &m) { return nabwa_fail(code, "%s", m.c_str()); }
static int ix_hip(hipError_t e, const char *what, int line)
{
	char b[512];
	snprintf(b, sizeof b, "%s failed: %s (index_build.hip:%d)", what, hipGetErrorString(e), line);
	return nabwa_fail(e == hipErrorOutOfMemory ? NABWA_ENOMEM : NABWA_ENODEV, "%s", b);
}
#define IXCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return ix_hip(e_, #x, __LINE__); } while (0)

// ---------------------------------------------------------------- device memory: one owner, freed on every path
struct Arena {
	struct Blk { void *p; size_t bytes; };
	std::vector<Blk> live;
	size_t cur = 0, peak = 0, min_free = SIZE_MAX, total = 0;
	int alloc(void **p, size_t bytes, const char *what)
	{
		*p = nullptr;
		const hipError_t e = hipMalloc(p, bytes ? bytes : 1);
		if (e != hipSuccess) {
			(void)hipGetLastError();
			char b[256];
			snprintf(b, sizeof b, "device allocation of %.3f GB for %s failed: %s", bytes / 1e9, what, hipGetErrorString(e));
			return nabwa_fail(e == hipErrorOutOfMemory ? NABWA_ENOMEM : NABWA_ENODEV, "%s", b);
		}
		live.push_back({ *p, bytes });
		cur += bytes; if (cur > peak) peak = cur;
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr < min_free) { min_free = fr; total = tot; }
		return 0;
	}
	template <class T> int get(T **p, size_t n, const char *what) { return alloc((void **)p, n * sizeof(T), what); }
	void release(void *p)
	{
		if (!p) return;
		for (size_t k = 0; k < live.size(); ++k)
			if (live[k].p == p) { (void)hipFree(p); cur -= live[k].bytes; live.erase(live.begin() + k); return; }
	}
	~Arena() { for (Blk &b : live) (void)hipFree(b.p); }
};

// ---------------------------------------------------------------- kernels

__device__ __forceinline__ uint32_t base_at(const uint8_t *pac, size_t i) { return pac[i >> 2] >> ((~i & 3) << 1) & 3; }

// reversed text: base j of the output = base n-1-j of the input, 4 bases per output byte
__global__ void index_reverse_pac(const uint8_t *__restrict__ in, size_t n, uint8_t *__restrict__ out)
{
	IX_FOR_ALL(b, (n + 3) / 4) {
		uint32_t x = 0;
		for (int u = 0; u < 4; ++u) {
			const size_t j = b * 4 + u;
			if (j < n) x |= base_at(in, n - 1 - j) << ((3 - u) << 1);
		}
		out[b] = (uint8_t)x;
	}
}

// first key of suffix i from the packed text (32 bases per big-endian 64-bit word; the buffer is padded by two words)
__global__ void index_key0(const uint64_t *__restrict__ pw, size_t n, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
	IX_FOR_ALL(i, n + 1) {
		const size_t w = i >> 5;
		const int o = (int)(i & 31);
		const uint64_t hi = __builtin_bswap64(pw[w]), lo = __builtin_bswap64(pw[w + 1]);
		const uint64_t win = o ? (hi << (2 * o)) | (lo >> (64 - 2 * o)) : hi;
		const size_t rem = n - i;
		const int valid = rem < KCH ? (int)rem : KCH;
		uint64_t packed = win >> (64 - 2 * KCH);
		if (valid < KCH) packed &= ~((1ull << (2 * (KCH - valid))) - 1);
		keys[i] = packed << 5 | (uint64_t)valid;
		vals[i] = (uint32_t)i;
	}
}

// head[j] = row of j if it starts a group else 0 (then max-scanned into group starts)
__global__ void index_heads(const uint64_t *__restrict__ keys, size_t m, const uint32_t *__restrict__ slots, uint32_t *__restrict__ head)
{
	IX_FOR_ALL(j, m) {
		const bool first = j == 0 || keys[j] != keys[j - 1];
		head[j] = first ? (slots ? slots[j] : (uint32_t)j) : 0u;
	}
}

// after the scan gs[j] = first row of j's group: ranks, group starts, and the rows of groups of two or more
__global__ void index_ranks(const uint64_t *__restrict__ keys, size_t m, const uint32_t *__restrict__ slots, const uint32_t *__restrict__ gs,
							const uint32_t *__restrict__ sa_vals, uint32_t *__restrict__ rank, uint32_t *__restrict__ group_start,
							uint8_t *__restrict__ tied)
{
	IX_FOR_ALL(j, m) {
		const bool first = j == 0 || keys[j] != keys[j - 1];
		const bool last = j + 1 == m || keys[j + 1] != keys[j];
		const uint32_t row = slots ? slots[j] : (uint32_t)j;
		rank[sa_vals[j]] = gs[j];
		group_start[row] = gs[j];
		tied[row] = !(first && last);
	}
}

// a tied row's suffix is at least h bases long (shorter ones end in '$' and are unique), so i + h <= n
__global__ void index_key2(size_t m, const uint32_t *__restrict__ slots, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ group_start,
						   const uint32_t *__restrict__ rank, uint32_t h, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
	IX_FOR_ALL(t, m) {
		const uint32_t row = slots[t], i = sa[row];
		keys[t] = (uint64_t)group_start[row] << 32 | (uint64_t)rank[i + h];
		vals[t] = i;
	}
}

__global__ void index_writeback(size_t m, const uint32_t *__restrict__ slots, const uint32_t *__restrict__ vals, uint32_t *__restrict__ sa)
{
	IX_FOR_ALL(t, m) sa[slots[t]] = vals[t];
}

struct IxMax { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };

// bw[r] = base before suffix SA[r]; 4 marks the '$' row (primary)
__global__ void index_bwt(const uint8_t *__restrict__ pac, size_t n, const uint32_t *__restrict__ sa, uint8_t *__restrict__ bw, uint32_t *__restrict__ primary)
{
	IX_FOR_ALL(r, n + 1) {
		const uint32_t p = sa[r];
		if (p == 0) { bw[r] = 4; *primary = (uint32_t)r; }
		else bw[r] = (uint8_t)base_at(pac, p - 1);
	}
}

// per 128-row block of the '$'-less BWT: the 8 packed words and the base counts
__global__ void index_pack_bwt(const uint8_t *__restrict__ bw, size_t n, uint32_t primary, uint32_t *__restrict__ words,
							   uint32_t *__restrict__ blk_cnt /* 4 arrays of nblk */, size_t nblk)
{
	IX_FOR_ALL(b, nblk) {
		uint32_t c[4] = { 0, 0, 0, 0 };
		for (int w = 0; w < 8; ++w) {
			uint32_t x = 0; bool any = false;
			for (int u = 0; u < 16; ++u) {
				const size_t k = b * 128 + w * 16 + u;
				if (k < n) {
					const uint8_t base = bw[k < primary ? k : k + 1];
					x |= (uint32_t)base << ((15 - u) << 1);
					++c[base]; any = true;
				}
			}
			if (any) words[b * 12 + 4 + w] = x;
		}
		blk_cnt[b] = c[0]; blk_cnt[nblk + b] = c[1]; blk_cnt[2 * nblk + b] = c[2]; blk_cnt[3 * nblk + b] = c[3];
	}
}

// checkpoint b sits before block b; the last one (the totals) follows the last, possibly partial, block
__global__ void index_ckpt(const uint32_t *__restrict__ blk_excl /* 4 x (nblk+1) */, size_t nblk, size_t n, uint32_t *__restrict__ words)
{
	IX_FOR_ALL(b, nblk + 1) {
		size_t pos = b * 12;
		if (b == nblk && (n & 127)) pos = (nblk - 1) * 12 + 4 + ((n & 127) + 15) / 16;
		for (int c = 0; c < 4; ++c) words[pos + c] = blk_excl[c * (nblk + 1) + b];
	}
}

// the totals: last exclusive sum + last block count, into slot nblk of each exclusive-sum array
__global__ void index_totals(const uint32_t *__restrict__ blk, uint32_t *__restrict__ blk_ex, size_t nblk)
{
	if (threadIdx.x < 4) blk_ex[threadIdx.x * (nblk + 1) + nblk] = blk_ex[threadIdx.x * (nblk + 1) + nblk - 1] + blk[threadIdx.x * nblk + nblk - 1];
}

__global__ void index_sa_sample(const uint32_t *__restrict__ sa, size_t n_sa, uint32_t intv, uint32_t *__restrict__ out)
{
	IX_FOR_ALL(j, n_sa) if (j > 0) out[j - 1] = sa[j * intv];
}

// ---------------------------------------------------------------- one direction

struct StageTimes { double sort = 0, doubling = 0, bwt = 0; int rounds = 0; uint64_t tied0 = 0; };

static double secs_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// radix-sort scratch for m (key, value) pairs: the size query allocates nothing
static int sort_scratch(size_t m, size_t *bytes)
{
	hipcub::DoubleBuffer<uint64_t> dk(nullptr, nullptr); hipcub::DoubleBuffer<uint32_t> dv(nullptr, nullptr);
	IXCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, dk, dv, m, 0, 64, 0));
	return 0;
}

// the packed text (n bases) on the device, zero-padded to whole 64-bit words plus two: what index_key0 reads
static size_t padded_pac_bytes(size_t n) { return ((n >> 5) + 2) * 8; }

static int build_direction(Arena &A, const uint8_t *d_pac, size_t n, int sa_intv, std::vector<uint32_t> &bwt_words,
						   std::vector<uint32_t> &sa_words, StageTimes &T)
{
	const size_t m = n + 1;
	auto t0 = std::chrono::steady_clock::now();
	uint64_t *kA = 0, *kB = 0; uint32_t *vA = 0, *vB = 0, *rank = 0, *gstart = 0, *slots = 0, *d_count = 0;
	uint8_t *tied = 0; void *tmp = 0; size_t tmp_bytes = 0, need = 0;
	auto ensure_tmp = [&](size_t want) -> int {
		if (want <= tmp_bytes) return 0;
		A.release(tmp); tmp = 0; tmp_bytes = 0;
		if (int rc = A.alloc(&tmp, want, "sort / scan scratch")) return rc;
		tmp_bytes = want;
		return 0;
	};
	int rc;
	if ((rc = A.get(&kA, m, "sort keys")) || (rc = A.get(&kB, m, "sort keys")) || (rc = A.get(&vA, m, "suffix array")) ||
		(rc = A.get(&vB, m, "sort values")) || (rc = A.get(&d_count, 2, "counter")))
		return rc;
	hipLaunchKernelGGL(index_key0, IX_GRID(m), 0, 0, (const uint64_t *)d_pac, n, kA, vA);
	IXCHK(hipGetLastError());
	hipcub::DoubleBuffer<uint64_t> dk(kA, kB); hipcub::DoubleBuffer<uint32_t> dv(vA, vB);
	IXCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, dk, dv, m, 0, 63, 0));
	if ((rc = ensure_tmp(need))) return rc;
	IXCHK(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, dk, dv, m, 0, 63, 0));
	uint64_t *keys = dk.Current(); uint32_t *sa = dv.Current(), *head = dv.Alternate();
	A.release(dk.Alternate());
	if ((rc = A.get(&rank, m + 1, "ranks")) || (rc = A.get(&gstart, m, "group starts")) || (rc = A.get(&tied, m, "tied flags"))) return rc;
	IXCHK(hipMemset(rank + m, 0, 4));
	hipLaunchKernelGGL(index_heads, IX_GRID(m), 0, 0, keys, m, (const uint32_t *)nullptr, head);
	IXCHK(hipGetLastError());
	IXCHK(hipcub::DeviceScan::InclusiveScan(nullptr, need, head, head, IxMax(), m, 0));
	if ((rc = ensure_tmp(need))) return rc;
	IXCHK(hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, head, head, IxMax(), m, 0));
	hipLaunchKernelGGL(index_ranks, IX_GRID(m), 0, 0, keys, m, (const uint32_t *)nullptr, head, sa, rank, gstart, tied);
	IXCHK(hipGetLastError());
	IXCHK(hipDeviceSynchronize());
	A.release(keys); A.release(head);
	if ((rc = A.get(&slots, m, "tied rows"))) return rc;
	T.sort = secs_since(t0);

	// ---- prefix doubling over the rows that are still tied (their number never grows: one allocation at the first round)
	t0 = std::chrono::steady_clock::now();
	uint64_t *k2a = 0, *k2b = 0; uint32_t *v2 = 0; size_t cap2 = 0;
	for (uint32_t h = KCH;; h *= 2) {
		hipcub::CountingInputIterator<uint32_t> iota(0);
		IXCHK(hipcub::DeviceSelect::Flagged(nullptr, need, iota, tied, slots, d_count, m, 0));
		if ((rc = ensure_tmp(need))) return rc;
		IXCHK(hipcub::DeviceSelect::Flagged(tmp, tmp_bytes, iota, tied, slots, d_count, m, 0));
		uint32_t cnt = 0;
		IXCHK(hipMemcpy(&cnt, d_count, 4, hipMemcpyDeviceToHost));
		if (T.rounds == 0) T.tied0 = cnt;
		if (cnt == 0) break;
		if ((uint64_t)h > (uint64_t)n) return ix_fail(NABWA_EINVAL, "prefix doubling did not converge (h > n): the suffix order is inconsistent");
		if (cnt > cap2) {
			A.release(k2a); A.release(k2b); A.release(v2); k2a = k2b = 0; v2 = 0;
			cap2 = cnt;
			if ((rc = A.get(&k2a, cap2, "doubling keys")) || (rc = A.get(&k2b, cap2, "doubling keys")) || (rc = A.get(&v2, 2 * cap2, "doubling values")))
				return rc;
		}
		hipLaunchKernelGGL(index_key2, IX_GRID((size_t)cnt), 0, 0, (size_t)cnt, slots, sa, gstart, rank, h, k2a, v2);
		IXCHK(hipGetLastError());
		hipcub::DoubleBuffer<uint64_t> ek(k2a, k2b); hipcub::DoubleBuffer<uint32_t> ev(v2, v2 + cap2);
		IXCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, ek, ev, (size_t)cnt, 0, 64, 0));
		if ((rc = ensure_tmp(need))) return rc;
		IXCHK(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, ek, ev, (size_t)cnt, 0, 64, 0));
		uint32_t *ghead = ev.Alternate();      // free after the sort: the heads of this round
		hipLaunchKernelGGL(index_writeback, IX_GRID((size_t)cnt), 0, 0, (size_t)cnt, slots, ev.Current(), sa);
		hipLaunchKernelGGL(index_heads, IX_GRID((size_t)cnt), 0, 0, ek.Current(), (size_t)cnt, slots, ghead);
		IXCHK(hipGetLastError());
		IXCHK(hipcub::DeviceScan::InclusiveScan(nullptr, need, ghead, ghead, IxMax(), (size_t)cnt, 0));
		if ((rc = ensure_tmp(need))) return rc;
		IXCHK(hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, ghead, ghead, IxMax(), (size_t)cnt, 0));
		hipLaunchKernelGGL(index_ranks, IX_GRID((size_t)cnt), 0, 0, ek.Current(), (size_t)cnt, slots, ghead, ev.Current(), rank, gstart, tied);
		IXCHK(hipGetLastError());
		++T.rounds;
	}
	A.release(k2a); A.release(k2b); A.release(v2);
	A.release(rank); A.release(gstart); A.release(slots); A.release(tied);
	T.doubling = secs_since(t0);

	// ---- BWT, the Occ-interleaved .bwt words, the sampled SA
	t0 = std::chrono::steady_clock::now();
	const size_t nblk = (n + 127) / 128;
	const size_t nw = 5 + (n + 15) / 16 + (nblk + 1) * 4;
	const size_t n_sa = (n + sa_intv) / sa_intv;
	uint8_t *bw = 0; uint32_t *words = 0, *blk = 0, *blk_ex = 0, *samples = 0;
	if ((rc = A.get(&bw, m + 1, "BWT bytes")) || (rc = A.get(&words, nw, ".bwt words")) || (rc = A.get(&blk, 4 * nblk, "block counts")) ||
		(rc = A.get(&blk_ex, 4 * (nblk + 1), "block sums")) || (rc = A.get(&samples, n_sa, "SA samples")))
		return rc;
	IXCHK(hipMemset(words, 0, nw * 4));
	hipLaunchKernelGGL(index_bwt, IX_GRID(m), 0, 0, d_pac, n, sa, bw, d_count);
	IXCHK(hipGetLastError());
	uint32_t primary = 0;
	IXCHK(hipMemcpy(&primary, d_count, 4, hipMemcpyDeviceToHost));
	hipLaunchKernelGGL(index_pack_bwt, IX_GRID(nblk), 0, 0, bw, n, primary, words + 5, blk, nblk);
	IXCHK(hipGetLastError());
	for (int c = 0; c < 4; ++c) {
		IXCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, blk + c * nblk, blk_ex + c * (nblk + 1), nblk, 0));
		if ((rc = ensure_tmp(need))) return rc;
		IXCHK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, blk + c * nblk, blk_ex + c * (nblk + 1), nblk, 0));
	}
	hipLaunchKernelGGL(index_totals, dim3(1), dim3(64), 0, 0, blk, blk_ex, nblk);
	hipLaunchKernelGGL(index_ckpt, IX_GRID(nblk + 1), 0, 0, blk_ex, nblk, n, words + 5);
	hipLaunchKernelGGL(index_sa_sample, IX_GRID(n_sa), 0, 0, sa, n_sa, (uint32_t)sa_intv, samples);
	IXCHK(hipGetLastError());
	uint32_t tot[4];
	for (int c = 0; c < 4; ++c) IXCHK(hipMemcpy(&tot[c], blk_ex + c * (nblk + 1) + nblk, 4, hipMemcpyDeviceToHost));
	const uint32_t hdr[5] = { primary, tot[0], tot[0] + tot[1], tot[0] + tot[1] + tot[2], tot[0] + tot[1] + tot[2] + tot[3] };
	if (hdr[4] != n) return ix_fail(NABWA_EINVAL, "BWT base counts do not add up to the text length");
	bwt_words.assign(nw, 0);
	IXCHK(hipMemcpy(bwt_words.data(), words, nw * 4, hipMemcpyDeviceToHost));
	memcpy(bwt_words.data(), hdr, 20);
	// .sa: primary, the 4 L2 words, sa_intv, seq_len, then SA[intv], SA[2 intv], ...
	sa_words.assign(7 + n_sa - 1, 0);
	memcpy(sa_words.data(), hdr, 20);
	sa_words[5] = (uint32_t)sa_intv; sa_words[6] = (uint32_t)n;
	if (n_sa > 1) IXCHK(hipMemcpy(sa_words.data() + 7, samples, (n_sa - 1) * 4, hipMemcpyDeviceToHost));
	A.release(bw); A.release(words); A.release(blk); A.release(blk_ex); A.release(samples); A.release(sa); A.release(tmp);
	A.release(d_count);
	T.bwt = secs_since(t0);
	return 0;
}

// ---------------------------------------------------------------- the entry point

static int write_words(const std::string &fn, const std::vector<uint32_t> &w)
{
	FILE *fp = fopen(fn.c_str(), "wb");
	if (!fp) return ix_fail(NABWA_EIO, "cannot write '" + fn + "'");
	const bool ok = fwrite(w.data(), 4, w.size(), fp) == w.size();
	if (fclose(fp) != 0 || !ok) return ix_fail(NABWA_EIO, "write to '" + fn + "' failed");
	return 0;
}

// the worst-case device bytes of a build of n bases (see the memory plan at the top)
extern "C" int nabwa_index_build_estimate(uint64_t l_pac, uint64_t *bytes)
{
	if (!bytes) return nabwa_fail(NABWA_EINVAL, "null argument");
	const size_t m = (size_t)l_pac + 1;
	size_t scratch = 0;
	if (int rc = sort_scratch(m, &scratch)) return rc;
	*bytes = 2 * padded_pac_bytes((size_t)l_pac) + 41ull * m + scratch + (64ull << 20);
	return 0;
}

extern "C" int nabwa_index_build(const char *prefix, int device, int sa_intv, int verbose)
{
	if (!prefix) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (sa_intv < 1) return nabwa_fail(NABWA_EINVAL, "sa_intv must be at least 1");
	const auto t_all = std::chrono::steady_clock::now();
	const std::string pre(prefix);
	// ---- the .pac, length as bwa_seq_len reads it (bwtmisc.c:43-54)
	std::vector<uint8_t> pac;
	{
		FILE *fp = fopen((pre + ".pac").c_str(), "rb");
		if (!fp) return ix_fail(NABWA_EIO, "cannot open '" + pre + ".pac'");
		fseek(fp, 0, SEEK_END);
		const long sz = ftell(fp);
		// the length from the file's size and last byte first: a text too long is refused before its bases are read
		int last = -1;
		if (sz >= 2 && fseek(fp, sz - 1, SEEK_SET) == 0) last = fgetc(fp);
		if (last >= 0 && last <= 3 && (uint64_t)(sz - 2) * 4 + (uint64_t)last > IX_MAX_N) {
			fclose(fp);
			char b[200];
			snprintf(b, sizeof b, "a text of %lld bases is too long: the reference's 32-bit Occ count (bwtmisc.c:131) holds at most %llu bases",
					 (long long)((int64_t)(sz - 2) * 4 + last), (unsigned long long)IX_MAX_N);
			return ix_fail(NABWA_EINVAL, b);
		}
		fseek(fp, 0, SEEK_SET);
		if (sz > 0) pac.resize((size_t)sz);
		const bool ok = sz > 0 && fread(pac.data(), 1, (size_t)sz, fp) == (size_t)sz;
		fclose(fp);
		if (!ok) return ix_fail(NABWA_EIO, "'" + pre + ".pac' is empty or unreadable");
	}
	const int64_t l_pac = pac.size() < 2 ? 0 : ((int64_t)pac.size() - 2) * 4 + pac.back();
	if (l_pac <= 0 || pac.back() > 3 || (size_t)((l_pac + 3) / 4) > pac.size() - 1)
		return ix_fail(NABWA_EIO, "'" + pre + ".pac' is malformed (its last byte does not match its size)");
	if ((uint64_t)l_pac > IX_MAX_N) {
		char b[200];
		snprintf(b, sizeof b, "a text of %lld bases is too long: the reference's 32-bit Occ count (bwtmisc.c:131) holds at most %llu bases",
				 (long long)l_pac, (unsigned long long)IX_MAX_N);
		return ix_fail(NABWA_EINVAL, b);
	}
	if ((uint64_t)l_pac + (uint64_t)sa_intv > 0xffffffffull) {      // the reference's loader would wrap n_sa (bwtio.c:175): no files it can read
		char b[200];
		snprintf(b, sizeof b, "a text of %lld bases with sa_intv %d: the reference's 32-bit SA count (bwtio.c:175) wraps above 0xffffffff",
				 (long long)l_pac, sa_intv);
		return ix_fail(NABWA_EINVAL, b);
	}
	const size_t n = (size_t)l_pac;

	// ---- the device and the memory budget, before any large allocation
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return nabwa_fail(NABWA_ENODEV, "no HIP device"); }
	if (device < 0 || device >= ndev) return nabwa_fail(NABWA_ENODEV, "no HIP device %s", std::to_string(device).c_str());
	IXCHK(hipSetDevice(device));
	uint64_t est = 0;
	if (int rc = nabwa_index_build_estimate((uint64_t)n, &est)) return rc;
	size_t dev_free = 0, dev_total = 0;
	IXCHK(hipMemGetInfo(&dev_free, &dev_total));
	uint64_t budget = dev_free;
	const char *cap_env = getenv("NABWA_INDEX_MAX_BYTES");
	if (cap_env && *cap_env) { const uint64_t cap = strtoull(cap_env, nullptr, 10); if (cap < budget) budget = cap; }
	if (est > budget) {
		char b[300];
		snprintf(b, sizeof b, "building the index of %zu bases needs up to %.3f GB of device memory; %.3f GB are allowed (device %d: %.3f GB free%s)",
				 n, est / 1e9, budget / 1e9, device, dev_free / 1e9, cap_env && *cap_env ? ", NABWA_INDEX_MAX_BYTES set" : "");
		return nabwa_fail(NABWA_ENOMEM, "%s", b);
	}
	if (verbose)
		fprintf(stderr, "[nabwa_index] %zu bases; device %d: estimate %.3f GB (worst case), %.3f GB free of %.3f GB\n", n, device, est / 1e9,
				dev_free / 1e9, dev_total / 1e9);

	// ---- both packed texts on the device: the upload, and its reverse made there
	Arena A;
	uint8_t *d_fwd = 0, *d_rev = 0;
	const size_t pb = padded_pac_bytes(n), nbytes = (n + 3) / 4;
	int rc;
	if ((rc = A.get(&d_fwd, pb, "packed text")) || (rc = A.get(&d_rev, pb, "reversed packed text"))) return rc;
	IXCHK(hipMemset(d_fwd, 0, pb));
	IXCHK(hipMemset(d_rev, 0, pb));
	IXCHK(hipMemcpy(d_fwd, pac.data(), nbytes, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(index_reverse_pac, IX_GRID(nbytes), 0, 0, d_fwd, n, d_rev);
	IXCHK(hipGetLastError());
	std::vector<uint8_t>().swap(pac);

	std::vector<uint32_t> bwt[2], sa[2];
	StageTimes T[2];
	for (int d = 0; d < 2; ++d) {
		const auto t0 = std::chrono::steady_clock::now();
		if ((rc = build_direction(A, d ? d_rev : d_fwd, n, sa_intv, bwt[d], sa[d], T[d]))) return rc;
		A.release(d ? d_rev : d_fwd);
		if (verbose)
			fprintf(stderr, "[nabwa_index] %s index: %.2f s (first sort %.2f s, %d doubling rounds over %llu tied rows %.2f s, BWT/Occ/SA %.2f s)\n",
					d ? "reverse" : "forward", secs_since(t0), T[d].sort, T[d].rounds, (unsigned long long)T[d].tied0, T[d].doubling, T[d].bwt);
	}
	if (verbose)
		fprintf(stderr, "[nabwa_index] device memory: peak %.3f GB allocated by the builder (estimate %.3f GB); device in use at the peak %.3f GB\n",
				A.peak / 1e9, est / 1e9, A.min_free == SIZE_MAX ? 0.0 : (A.total - A.min_free) / 1e9);
	const auto t_w = std::chrono::steady_clock::now();
	if ((rc = write_words(pre + ".bwt", bwt[0])) || (rc = write_words(pre + ".rbwt", bwt[1])) || (rc = write_words(pre + ".sa", sa[0])) ||
		(rc = write_words(pre + ".rsa", sa[1])))
		return rc;
	if (verbose) fprintf(stderr, "[nabwa_index] writing .bwt/.rbwt/.sa/.rsa: %.2f s; build total %.2f s\n", secs_since(t_w), secs_since(t_all));
	return 0;
}
