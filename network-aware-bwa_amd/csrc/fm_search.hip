// fm_search.hip -- bounded-backtracking FM-index search, one read per lane (gfx950).
//
// Computes what bwa_cal_sa_reg_gap does per read (bwtaln.c:93-142): the four bwt_cal_width
// passes (bwtaln.c:52-76) and bwt_match_gap (bwtgap.c:104-266), reproducing the exact
// pop/push order of the reference's per-score LIFO stacks (bwtgap.c:46-79) because that order
// decides which hits are found and in which order they are reported.
//
// Execution model: two persistent kernels per batch.  Kernel W (fm_width_kernel) runs the width
// passes: one lane = one strand of one read, every lane executes the same code on every trip, so its
// waves are converged.  Kernel S (fm_search_kernel) runs the search: every lane is its own state machine
// (pop / expansion / exact-tail step / tail jump / text tail / hit) and performs at most ONE rank query --
// Occ of all four bases at rows (k-1, l), one or two 64-byte bucket fetches -- per trip.  A wave draws
// work in blocks from a global counter.  v2 had both phases in one loop and ran at 31 % VALU lane
// utilisation, issue-bound (profiles/r01_v2_pmc.json); hence the split.
//
// Memory discipline (v2).  With ~260 k reads in flight the caches hold ~128 B of L2 and ~1 KB of
// Infinity Cache per lane, so every touch of lane-private state in HBM costs a 64-byte
// transaction -- as much as the rank query it accompanies (v1 moved 4.5x the algorithmic bytes,
// profiles/r01_v1_pmc.json).  Therefore:
//   * the child that continues the current path (always the LAST push of an expansion) is kept
//     in registers as the "pending" entry (in arena format); it is the next pop whenever its score is
//     not above the lowest score in memory (for the match child: always) and is spilled otherwise, so
//     the observable pop order is unchanged;
//   * an arena entry is one 16-byte word with its list link embedded; head[score] lives in LDS
//     ([score][lane], 2 bytes each); a 64-bit register mask tracks the non-empty scores;
//   * read bases and the per-position bound bytes are read through 16-byte windows in LDS, filled by
//     global_load_lds_dwordx4, that stay valid for 8-16 steps of a descent;
//   * the test "w[i-1] == w[i]" (bwtgap.c:208,212) is precomputed into bit 7 of the bound byte,
//     so the 32-bit interval widths are only touched by gap_shadow (bwtgap.c:81-91);
//   * the width passes write their results in 16-byte chunks (4 widths / 16 bound bytes).
// Work avoidance (v5): exact tails near the read end jump through the interval table; an
// interval of one row is carried as a text position and extended by text comparison, several levels per
// trip; the gap children of an expansion are one grouped stack entry, materialised only if popped; the
// next pop is fetched ahead into LDS while a tail is walked; reads with an exact occurrence (kernel W's
// class) are searched first, by waves that refill all 64 lanes together.
// Bump allocation (arena = pushes that reach memory).  Reads that outgrow the arena, the per-read hit list or the trip budget
// are flagged and searched from the start by kernel D (fm_deep.hip: one search per wavefront, paged arenas) -- never on the CPU.
#include "nabwa_dev.hpp"
#include "fm_search.hpp"
#include "launchers.hpp"

#define STATE_M 0
#define STATE_I 1
#define STATE_D 2
#define STATE_GROUP 3   // arena only: the gap children of one expansion, see fm_search_kernel
#define GRP_EXT 0x100u
// Markers in the `l` word of a stack entry.  A key at depth T = 16 uses all 32 bits (TTTTTTTTTTTTTTTT = 0xffffffff), and the generic
// child test is "k' <= l'": KEYM must therefore be the largest value.  (With KEYM = 0xfffffffe the all-T child of the last table
// level failed that test and reads from poly-T stretches lost a hit -- found on the repeat-model genome, round 2.)  Text positions
// stay below 0xfffffff0 (text_ok).
#define TXM 0xfffffffeu   // l of an interval carried in text form (k = text position)
#define KEYM 0xffffffffu  // l of an interval carried in key form (k = path key: the reference symbols matched so far as base-4 digits)
#define LVO(t_) ((size_t)((((uint64_t)1 << (2 * (t_))) - 4ull) / 3ull))   /* offset of level t in the interval table */
#ifndef NABWA_W_WAVES
#define NABWA_W_WAVES 5   // kernel W: waves per SIMD the register budget is bounded for (96 VGPRs)
#endif
#ifndef NABWA_WORK_CHUNK
#define NABWA_WORK_CHUNK 64u
#endif
#ifndef NABWA_RUN_MAX
#define NABWA_RUN_MAX 4   // levels one text-form trip may walk (every lane of the wave waits for the longest walk)
#endif

// 16-byte register windows are kept as two separate 64-bit scalars and indexed with a select and a
// shift: a dynamically indexed uint4 (or a struct of two halves) makes hipcc keep the value in
// scratch and load one piece back.
__device__ __forceinline__ uint32_t byte_of(uint64_t lo, uint64_t hi, uint32_t idx)
{
	asm volatile("" : "+v"(lo), "+v"(hi));   // opaque at the USE: no dynamic vector extract, and no wait at the load
	const uint64_t h = (idx & 8u) ? hi : lo;
	return (uint32_t)(h >> ((idx & 7u) << 3)) & 0xffu;
}
#define WIN_SET(lo_, hi_, a_, b_, c_, d_) do { lo_ = (uint64_t)(b_) << 32 | (a_); hi_ = (uint64_t)(d_) << 32 | (c_); } while (0)

__device__ __forceinline__ void set_word(uint4 &q, uint32_t c, uint32_t v)
{
	q.x = c == 0 ? v : q.x; q.y = c == 1 ? v : q.y; q.z = c == 2 ? v : q.z; q.w = c == 3 ? v : q.w;
}

extern __shared__ uint16_t s_head[];   // search kernel, first pass only: [score][lane of the block]

#ifndef NABWA_MIN_WAVES
#define NABWA_MIN_WAVES 4   // 128 VGPRs: 4 blocks per CU (measured +10 % over 3)
#endif

// =====================================================================================
// Kernel W: the four bwt_cal_width passes (bwtaln.c:52-76,123-130) of every read.
// One lane = one strand of one read (work item 2 * read + strand): its full pass, then its seed pass; all lanes run
// the same code on every trip, so the wave stays converged; results go to the read's own record in HBM in 16-byte chunks:
//   Wd [2][WL]  u32 interval widths (only gap_shadow reads them later)
//   Bd [2][WLB] bound bytes: min(bid,127) | (w[i-1]==w[i]) << 7
//   SBd[2][SLB] the same for the seed passes
// =====================================================================================
// WF: the forms of its trips, bits TM_W_RUNS / TM_W_TRIP8 of text_mode shifted down to bit 0 -- one instantiation per combination,
// picked at the launch (with_width_kernel): with the forms as run-time flags the old and the new paths together spilled 28 VGPRs at
// 5 waves; as instantiations WF = 0 has the paths of the kernel before v15 and no other (its end-of-pass block alone has moved, to the end
// of the loop body), and every other one holds the paths it can take alone.
// STATS (NABWA_W_STATS, TM_W_STATS): the same kernel, tables and all, that also counts its trips into slots TS_W_* of P.touch_counter.
#define W_FORMS(tm_) (((tm_) / TM_W_RUNS) & 3)
template <bool COUNT, int WF, bool STATS = false>
__global__ __launch_bounds__(NABWA_SEARCH_BLOCK, NABWA_W_WAVES) void fm_width_kernel(const SearchParams P)
{
	const uint32_t lane = threadIdx.x & 63u;
	bool run = false, done = false;
	unsigned int w_next = 0, w_end = 0;                     // this wave's block of work items (item = 2 * read + strand)
	uint32_t rid = 0, x = 0; int len = 0, phase = 0, wi = 0, n = 0, sbase = 0, nN = 0;
	uint32_t sq_off = 0;                                    // this read's offset in the padded base arrays
#define WREC (P.wdata + (size_t)rid * P.wstride)
#define BX(f_) (x ? P.bwt[1].f_ : P.bwt[0].f_)              /* this lane's index: strand x is matched against bwt[x] (bwtaln.c:123-130) */
	// text mode (nabwa_dev.hpp): the pass has narrowed to ONE row, the suffix at text position tp; the next symbol
	// matches iff it equals the text base in front of it, and the width stays 1 (kk == ll is kept as it is)
	bool tmode = false; uint32_t tp = 0, twtag = 0xffffffffu; uint2 twin = make_uint2(0u, 0u);
	const bool text_ok = (P.text_mode & 1) && P.bwt[0].sa_full && P.bwt[1].sa_full;
	uint32_t kk = 0, ll = 0, pw = 0; int bid = 0;
	uint32_t wkey = 0xffffffffu; bool tok = false; int tbase = 0;   // interval-table key of the KT symbols from position tbase of this phase (the current restart point)
	const int KT = (int)P.bwt[0].kmer_T, LW = (int)P.bwt[0].kmer_LW;
	// the primary keys of the table's levels (fm_search.hpp, fm_index.hip): [strand][level], picked per lane in a table trip
	__shared__ uint32_t s_pk[2 * NABWA_PK_LEVELS];
	const bool quads = (P.text_mode & TM_W_QUADS) && P.ixtab;
	if (threadIdx.x < 2 * NABWA_PK_LEVELS) s_pk[threadIdx.x] = quads ? P.ixtab[NABWA_IXTAB_WORDS + threadIdx.x] : 0xffffffffu;
	__syncthreads();
	// the forms of this kernel's trips (fm_search.hpp: TM_W_*); with both off every path is the one before v15
	constexpr bool w_trip8 = (WF & 2) != 0, w_runs = (WF & 1) != 0;      // (a run needs the packed read: nflag is set where there is none)
	// STATS: lane-trips [path] and positions [path] of this lane (paths: 0 text trip, 1 table trip, 2 single step with a rank query, 3 without),
	// text trips begun in a seed pass, this item's trips, this wave's trips
	uint32_t st_lt[4] = { 0u, 0u, 0u, 0u }, st_pos[2] = { 0u, 0u }, st_tx1 = 0u, st_item = 0u, st_max = 0u, st_wave = 0u;
	bool nflag = true;                                          // this strand has an N (word PW-1 of its packed bases), read once when the item is taken
	// after a restart (bwtaln.c:66-70) the pattern begins anew at the next position: its key comes from the packed read
	auto rekey = [&](int from) {
		tok = false; tbase = from;
		if (nflag || from + (w_trip8 ? 0 : 4) >= n) return;       // an N somewhere in this strand (or no table, no packed reads): step by step
		const int PW = P.pack_stride / 2;
		const uint32_t *const pk = P.rd_pack + (size_t)rid * P.pack_stride + x * PW;
		const int q = sbase + from;
		const uint32_t w0 = pk[q >> 4], w1 = pk[(q >> 4) + 1], sh = ((uint32_t)q & 15u) << 1;
		const uint32_t k16 = sh ? (w0 << sh) | (w1 >> (32u - sh)) : w0;
		wkey = k16 >> (2 * (16 - KT)); tok = true;
	};
	uint4 wacc = make_uint4(0, 0, 0, 0); uint64_t blo = 0, bhi = 0, slo = 0, shi = 0; int stag = -1;
	unsigned long long touches = 0;

	for (;;) {
		unsigned long long need = __ballot(!run && !done);
		// equal-length reads (P.w_sync): a wave takes 64 new items only when all its lanes are done, so every lane is at the
		// same position of the same phase and the wave executes ONE of the paths below per trip, not all of them
		if (P.w_sync && __ballot(run) != 0ull) need = 0ull;
		if (need) {
			// work items come in blocks of NABWA_WORK_CHUNK per wave: one atomic on the shared counter per block, not per
			// refill (a single address takes ~10^8 atomics per second)
			if (w_next == w_end) {
				unsigned int base = 0;
				if (lane == 0) base = atomicAdd(P.work_counter + WC_WIDTH, (unsigned int)NABWA_WORK_CHUNK);
				w_next = __builtin_amdgcn_readfirstlane(base); w_end = w_next + NABWA_WORK_CHUNK;
			}
			const unsigned int rank = (unsigned int)__popcll(need & ((1ull << lane) - 1ull)), avail = w_end - w_next;
			const unsigned int base = w_next;
			w_next += min((unsigned int)__popcll(need), avail);
			if (!run && !done && rank < avail) {
				const unsigned int idx = base + rank;
				if (idx < 2u * (unsigned int)P.n) {
					rid = P.ids ? (uint32_t)P.ids[idx >> 1] : idx >> 1; x = idx & 1u;
					const int64_t o = P.poff[rid];
					len = P.rd_len[rid];
					sq_off = (uint32_t)o;
					nN = 0; stag = -1;
					if (P.w_skip_clean && P.n_aln[rid] == 0) { /* its record is as the first run of this kernel left it */ }
					else if (len > 0) {
						run = true; phase = 0; wi = 0; n = len; sbase = 0; tmode = false;
						if (KT) { wkey = P.rd_key[6 * (size_t)rid + 2 + x]; tok = wkey != 0xffffffffu; }
						nflag = !KT || !P.rd_pack || P.rd_pack[(size_t)rid * P.pack_stride + (x + 1u) * (uint32_t)(P.pack_stride / 2) - 1u] != 0u;
						tbase = 0;
						kk = 0; ll = BX(seq_len); bid = 0; pw = 0; blo = bhi = 0;
					} else { if (x == 0u) P.rd_nN[rid] = 0; if (P.rd_cls) P.rd_cls[2 * (size_t)rid + x] = 0; }   // (an empty read: nothing to search)
				} else done = true;
			}
		}
		if (__ballot(!done) == 0ull) break;
		if (STATS) { ++st_wave; if (run) ++st_item; }
		// output of position p: width, bound byte, 16-byte chunk flushes; `last` = the terminator {w = 0, bid = ++bid}
		// after the final position (bwtaln.c:73-74)
		auto out_pos = [&](int p, bool last) {
			uint8_t *const rec = WREC;
			if (last) ++bid;
			const uint32_t wv = last ? 0u : ll - kk + 1u;
			const uint32_t bv = (uint32_t)(bid > 127 ? 127 : bid) | ((p > 0 && wv == pw) ? 128u : 0u);
			set_word(wacc, (uint32_t)p & 3u, wv);
			{ const uint64_t sh = (uint64_t)bv << (((uint32_t)p & 7u) << 3); if (p & 8) bhi |= sh; else blo |= sh; }
			pw = wv;
			if (phase == 0 && ((p & 3) == 3 || last)) *(uint4*)((uint32_t*)rec + x * P.WL + (p & ~3)) = wacc;
			if ((p & 15) == 15 || last) {
				*(uint4*)(rec + (phase ? P.woff_sbid + x * P.SLB : P.woff_bid + x * P.WLB) + (p & ~15)) =
					make_uint4((uint32_t)blo, (uint32_t)(blo >> 32), (uint32_t)bhi, (uint32_t)(bhi >> 32));
				blo = bhi = 0;
			}
		};
		// The same output for SEVERAL finished positions at once (the text runs and the 8-level table trips), without a turn per position:
		// the cnt bound bytes of positions p .. p+cnt-1 arrive as one 128-bit value (byte j = position p+j, zero from cnt on; the
		// terminator, where the pass ends, is the last of them), are shifted to their place behind the bytes the accumulator holds
		// and merged; the 16-byte chunk that became complete is stored, the rest stays in the accumulator.  cnt <= 16.
		auto put_bytes = [&](int p, int cnt, uint64_t nlo, uint64_t nhi, bool fin) {
			uint8_t *const dst = WREC + (phase ? P.woff_sbid + x * P.SLB : P.woff_bid + x * P.WLB) + (p & ~15);
			const uint32_t o = (uint32_t)p & 15u, s = (o & 7u) << 3;
			const uint64_t a0 = nlo << s, a1 = nhi << s | (s ? nlo >> (64u - s) : 0ull), a2 = s ? nhi >> (64u - s) : 0ull;
			const bool up = (o & 8u) != 0u;
			const uint64_t q0 = blo | (up ? 0ull : a0), q1 = bhi | (up ? a0 : a1), q2 = up ? a1 : a2, q3 = up ? a2 : 0ull;
			const uint32_t e = o + (uint32_t)cnt;
			const bool full = e >= 16u;
			if (full) *(uint4*)dst = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
			blo = full ? q2 : q0; bhi = full ? q3 : q1;
			if (fin) {
				if (e & 15u) *(uint4*)(dst + (full ? 16 : 0)) = make_uint4((uint32_t)blo, (uint32_t)(blo >> 32), (uint32_t)bhi, (uint32_t)(bhi >> 32));
				blo = bhi = 0;
			}
		};
		// ... and their widths (full pass only): w[0 .. cnt-1], entries from cnt on are never stored before they are written again.
		// The values move up by p & 3 places in two select stages, the accumulator's entries go in front, whole chunks are stored.
		auto put_widths = [&](int p, int cnt, const auto &w, bool fin) {
			constexpr int NW = (int)(sizeof(w) / sizeof(w[0])), NC = (NW + 6) / 4;
			uint32_t *const dst = (uint32_t*)WREC + x * P.WL + (p & ~3);
			const uint32_t o = (uint32_t)p & 3u;
			uint32_t s1[NW + 1], c[4 * NC];
#pragma unroll
			for (int j = 0; j <= NW; ++j) { const uint32_t a = j < NW ? w[j] : 0u, b = j ? w[j - 1] : 0u; s1[j] = (o & 1u) ? b : a; }
#pragma unroll
			for (int j = 0; j < 4 * NC; ++j) { const uint32_t a = j <= NW ? s1[j] : 0u, b = (j >= 2 && j - 2 <= NW) ? s1[j - 2] : 0u; c[j] = (o & 2u) ? b : a; }
			c[0] = o > 0u ? wacc.x : c[0]; c[1] = o > 1u ? wacc.y : c[1]; c[2] = o > 2u ? wacc.z : c[2];
			const uint32_t e = o + (uint32_t)cnt;
#pragma unroll
			for (int j = 0; j < NC; ++j)
				if (4u * j + 4u <= e || (fin && 4u * j < e)) *(uint4*)(dst + 4 * j) = make_uint4(c[4 * j], c[4 * j + 1], c[4 * j + 2], c[4 * j + 3]);
			uint4 r = make_uint4(c[0], c[1], c[2], c[3]);
#pragma unroll
			for (int j = 1; j < NC; ++j) if ((e >> 2) == (uint32_t)j) r = make_uint4(c[4 * j], c[4 * j + 1], c[4 * j + 2], c[4 * j + 3]);
			wacc = r;
		};
		// ... and the widths of a text run: all 1, the terminator's 0 at position term (-1: none in this run).  cnt <= 16: five chunks.
		auto put_ones = [&](int p, int cnt, int term, bool fin) {
			uint32_t *const dst = (uint32_t*)WREC + x * P.WL + (p & ~3);
			const uint32_t o = (uint32_t)p & 3u, e = o + (uint32_t)cnt;
			const int t = term - (p & ~3);
			uint4 c0 = make_uint4(t == 0 ? 0u : 1u, t == 1 ? 0u : 1u, t == 2 ? 0u : 1u, t == 3 ? 0u : 1u);
			c0.x = o > 0u ? wacc.x : c0.x; c0.y = o > 1u ? wacc.y : c0.y; c0.z = o > 2u ? wacc.z : c0.z;
			if (4u <= e || fin) *(uint4*)dst = c0;
#pragma unroll
			for (int j = 1; j < 5; ++j)
				if (4u * j + 4u <= e || (fin && 4u * j < e))
					*(uint4*)(dst + 4 * j) = make_uint4(t == 4 * j ? 0u : 1u, t == 4 * j + 1 ? 0u : 1u, t == 4 * j + 2 ? 0u : 1u, t == 4 * j + 3 ? 0u : 1u);
			wacc = e < 4u ? c0 : make_uint4(1u, 1u, 1u, 1u);
		};
		// bulk text trip: a full pass in text mode at a 16-position chunk boundary -- compare the chunk's 16 read symbols
		// with the 16 text bases to the left of the suffix as packed words; if all match, every width is 1, every bound
		// byte repeats (no restart, w[i-1] == w[i]) and the chunk's output is five 16-byte stores
		bool bulk = !w_runs && run && phase == 0 && tmode && (wi & 15) == 0 && wi + 16 < n && tp >= 16u && pw == 1u;
		// text run (TM_W_RUNS), in place of the bulk trip: up to 16 positions from ANY position of either pass.  The read's next 16
		// symbols are one extract from its packed words (as rekey takes them), the 16 text bases to the left of the suffix one from
		// the text's; the run is the number of leading 2-bit groups that agree, clamped to what the pass and the text have left.
		// A mismatch ends the run in front of it: that position restarts in the single step below, in the next trip or -- a run
		// of no position -- in this one.
		if constexpr (w_runs) if (run && tmode && !nflag && pw == 1u && tp > 0u) {
			const uint32_t *const pk = P.rd_pack + (size_t)rid * P.pack_stride + x * (P.pack_stride / 2);
			const int q = sbase + wi;
			const uint32_t r0 = pk[q >> 4], r1 = pk[(q >> 4) + 1], sh = ((uint32_t)q & 15u) << 1;
			const uint32_t rd = sh ? (r0 << sh) | (r1 >> (32u - sh)) : r0;
			const uint32_t b0 = tp >= 16u ? tp - 16u : 0u, ts = (b0 & 15u) << 1;
			const uint32_t *const txt = BX(text);
			const uint32_t t0 = txt[b0 >> 4], t1 = ts ? txt[(b0 >> 4) + 1u] : 0u;      // (the second word only where the 16 bases reach into it)
			uint32_t tx = (uint32_t)(((uint64_t)t1 << 32 | t0) >> ts);                // text bases b0 .. b0+15, base b0+m at bits 2m
			if (tp < 16u) tx <<= (16u - tp) << 1;                                     // base tp-1 at the top, where the read's next symbol is: the walk goes down the text
			const uint32_t df = tx ^ rd, same = df ? (uint32_t)__clz((int)df) >> 1 : 16u;
			const uint32_t left = (uint32_t)(n - wi);
			uint32_t kmax = min(min(16u, left), tp);
			if (left == 16u) kmax = min(kmax, 15u);                                   // (a run and its terminator are 16 bytes at the most)
			const uint32_t r = min(same, kmax);
			if (r) {
				const bool fin = r == left;
				const uint64_t b8 = (uint64_t)((uint32_t)(bid > 127 ? 127 : bid) | 128u) * 0x0101010101010101ull;
				const uint64_t mlo = r >= 8u ? ~0ull : (1ull << (r << 3)) - 1ull, mhi = r <= 8u ? 0ull : (r >= 16u ? ~0ull : (1ull << ((r - 8u) << 3)) - 1ull);
				uint64_t nlo = b8 & mlo, nhi = b8 & mhi;
				if (fin) {                                                            // the terminator {w = 0, bid = ++bid}: 0 is not the width before it
					++bid;
					const uint64_t tb = (uint64_t)(bid > 127 ? 127 : bid);
					if (r < 8u) nlo |= tb << (r << 3); else nhi |= tb << ((r - 8u) << 3);
				}
				if (phase == 0) put_ones(wi, (int)r + (fin ? 1 : 0), fin ? n : -1, fin);
				put_bytes(wi, (int)r + (fin ? 1 : 0), nlo, nhi, fin);
				if (STATS) { ++st_lt[0]; st_pos[0] += r; if (phase) ++st_tx1; }
				tp -= r; wi += (int)r; bulk = true;
			}
		}
		if constexpr (!w_runs) if (bulk) {
			if ((wi >> 4) != stag) { const uint4 q = *(const uint4*)((x ? P.rseq : P.seq) + sq_off + wi); WIN_SET(slo, shi, q.x, q.y, q.z, q.w); stag = wi >> 4; }
			const uint32_t w0 = (tp - 16u) >> 4;
			const uint32_t *const txt = BX(text);
			const uint32_t t0 = txt[w0], t1 = txt[w0 + 1u];
			// 2 low bits of each of the 16 read bytes, byte j -> bits 2j
			auto squeeze = [](uint64_t v) -> uint32_t {
				uint64_t y = v & 0x0303030303030303ull;
				y = (y | y >> 6) & 0x000F000F000F000Full; y = (y | y >> 12) & 0x000000FF000000FFull; y = (y | y >> 24) & 0xFFFFull;
				return (uint32_t)y;
			};
			const bool clean = ((slo | shi) & 0xFCFCFCFCFCFCFCFCull) == 0ull;           // no N among them
			const uint32_t rd = squeeze(slo) | squeeze(shi) << 16;
			// text bases tp-16 .. tp-1, base tp-16+m at bits 2m; the read meets them from the top down
			const uint32_t tx = (uint32_t)(((uint64_t)t1 << 32 | t0) >> (((tp - 16u) & 15u) << 1));
			uint32_t rv = __brev(tx); rv = (rv >> 1 & 0x55555555u) | (rv & 0x55555555u) << 1;   // 2-bit groups reversed
			bulk = clean && rv == rd;
			if (bulk) {
				uint8_t *const rec = WREC;
				uint32_t *const wp = (uint32_t*)rec + x * P.WL + wi;
#pragma unroll
				for (int u = 0; u < 4; ++u) *(uint4*)(wp + 4 * u) = make_uint4(1u, 1u, 1u, 1u);
				const uint32_t b4 = ((uint32_t)(bid > 127 ? 127 : bid) | 128u) * 0x01010101u;
				*(uint4*)(rec + P.woff_bid + x * P.WLB + wi) = make_uint4(b4, b4, b4, b4);
				if (STATS) { ++st_lt[0]; st_pos[0] += 16u; if (phase) ++st_tx1; }
				tp -= 16u; wi += 16;
			}
		}
		if (bulk) { /* chunk done */ }
		else if (w_trip8 && run && tok && wi - tbase < LW) {
			// table trip of up to 8 levels (TM_W_TRIP8; the instantiations without it take the 4-level trip below, these never), clamped to
			// the levels the table has left for this pattern and to the positions the pass has left -- so a pass may end inside it, and the terminator goes out in the same append.  Quads as below, one 32-byte load per two levels; where the
			// trip's last level is the table's last, its entry is loaded itself: the interval left behind is always the real one.
			const int t1 = wi - tbase + 1, m = min(min(8, LW - (wi - tbase)), n - wi);
			const uint2 *const lo = BX(kmer_lo);
			uint2 tv[8];
#pragma unroll
			for (int u = 0; u < 8; ++u) tv[u] = make_uint2(1u, 0u);
			if (quads) {
				uint4 qd[4][2];
#pragma unroll
				for (int h = 0; h < 4; ++h) {
					const int t = t1 + 2 * h;
					qd[h][0] = qd[h][1] = make_uint4(1u, 0u, 1u, 0u);
					if (2 * h + 1 < m) {
						const uint4 *const p = (const uint4*)(lo + LVO(t + 1) + 4 * (size_t)(wkey >> (2 * (KT - t))));
						qd[h][0] = p[0]; qd[h][1] = p[1];
					} else if (2 * h < m) {
						const uint2 v = (lo + LVO(t))[wkey >> (2 * (KT - t))];
						qd[h][0].x = v.x; qd[h][0].y = v.y;
					}
				}
#pragma unroll
				for (int h = 0; h < 4; ++h) {
					const int t = t1 + 2 * h;
					if (2 * h + 1 < m) {
						const uint32_t ch = wkey >> (2 * (KT - t - 1)), c = ch & 3u;
						const uint4 a = qd[h][0], b = qd[h][1];
						const uint32_t sum = (a.y - a.x) + (a.w - a.z) + (b.y - b.x) + (b.w - b.z) + 4u + ((ch >> 2) == s_pk[x * NABWA_PK_LEVELS + t] ? 1u : 0u);
						tv[2 * h] = make_uint2(1u, sum);
						tv[2 * h + 1] = c == 0u ? make_uint2(a.x, a.y) : (c == 1u ? make_uint2(a.z, a.w) : (c == 2u ? make_uint2(b.x, b.y) : make_uint2(b.z, b.w)));
					} else tv[2 * h] = make_uint2(qd[h][0].x, qd[h][0].y);
				}
			} else {
#pragma unroll
				for (int u = 0; u < 8; ++u)
					if (u < m) { const int t = t1 + u; tv[u] = (lo + LVO(t))[wkey >> (2 * (KT - t))]; }
			}
			// the levels as values: a level is part of the trip while no level before it was empty (the restart, bwtaln.c:66-70)
			const uint32_t full1 = BX(seq_len) + 1u, bb = (uint32_t)(bid > 127 ? 127 : bid), bb1 = (uint32_t)(bid + 1 > 127 ? 127 : bid + 1);
			uint32_t wv[9], pv = pw, nk = kk, nl = ll; uint64_t nlo = 0ull; int cnt = 0; bool alive = true, died = false;
#pragma unroll
			for (int u = 0; u < 8; ++u) {
				const bool act = alive && u < m, dead = tv[u].x > tv[u].y;
				const uint32_t w = dead ? full1 : tv[u].y - tv[u].x + 1u;
				const uint32_t by = (dead ? bb1 : bb) | ((wi + u > 0 && w == pv) ? 128u : 0u);
				wv[u] = act ? w : 0u;
				if (act) { nlo |= (uint64_t)by << (8 * u); pv = w; nk = tv[u].x; nl = tv[u].y; ++cnt; died = dead; }
				alive = act && !dead;
			}
			wv[8] = 0u;
			const int p0 = wi;
			if (STATS) { ++st_lt[1]; st_pos[1] += (uint32_t)cnt; }
			wi += cnt; pw = pv;
			if (died) { kk = 0; ll = BX(seq_len); ++bid; rekey(wi); } else { kk = nk; ll = nl; }
			const bool fin = wi == n;
			uint64_t nhi = 0ull;
			if (fin) {
				++bid;
				const uint64_t tb = (uint64_t)(bid > 127 ? 127 : bid);
				if (cnt < 8) nlo |= tb << (8 * cnt); else nhi = tb;
			}
			if (phase == 0) put_widths(p0, cnt + (fin ? 1 : 0), wv, fin);
			put_bytes(p0, cnt + (fin ? 1 : 0), nlo, nhi, fin);
		}
		else if (!w_trip8 && run && tok && wi - tbase + 4 <= LW && wi + 4 < n) {
			// table trip: the intervals after wi+1 .. wi+4 symbols of this phase are entries of levels wi+1 .. wi+4 of the
			// interval table (fm_index.hip) -- four independent 8-byte loads, the low levels cache-resident -- instead
			// of four dependent rank queries.  An empty entry is the reference's restart (bwtaln.c:66-70): from there on
			// the prefix is no longer the read's, so the rest of the phase steps normally.
			// Two levels per load (quads): the four children of a key are 32 contiguous bytes of the next level, and every row of the
			// parent's interval carries one BWT symbol A/C/G/T except the primary row -- so width(parent) = the sum of its children's
			// widths (an empty child {1, 0} gives 0) + 1 if the parent is its level's primary key.  The children of K(t1) and of K(t1+2)
			// give the widths of levels t1 and t1+2 that way (handed to out_pos as {1, width}) and the entries of t1+1 and t1+3 directly:
			// two line requests per trip instead of four, and the interval left behind is the real one of the last level.
			uint2 tv[4];
			const uint2 *const lo = BX(kmer_lo);
			const int t1 = wi - tbase + 1;
			if (quads) {
				uint4 qd[2][2];
#pragma unroll
				for (int h = 0; h < 2; ++h) {
					const int t = t1 + 2 * h;
					const uint4 *const p = (const uint4*)(lo + LVO(t + 1) + 4 * (size_t)(wkey >> (2 * (KT - t))));
					qd[h][0] = p[0]; qd[h][1] = p[1];
				}
#pragma unroll
				for (int h = 0; h < 2; ++h) {
					const int t = t1 + 2 * h;
					const uint32_t ch = wkey >> (2 * (KT - t - 1)), c = ch & 3u;
					const uint4 a = qd[h][0], b = qd[h][1];
					const uint32_t sum = (a.y - a.x) + (a.w - a.z) + (b.y - b.x) + (b.w - b.z) + 4u + ((ch >> 2) == s_pk[x * NABWA_PK_LEVELS + t] ? 1u : 0u);
					tv[2 * h] = make_uint2(1u, sum);
					tv[2 * h + 1] = c == 0u ? make_uint2(a.x, a.y) : (c == 1u ? make_uint2(a.z, a.w) : (c == 2u ? make_uint2(b.x, b.y) : make_uint2(b.z, b.w)));
				}
			} else {
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const int t = t1 + u;
					tv[u] = (lo + LVO(t))[wkey >> (2 * (KT - t))];
				}
			}
#pragma unroll
			for (int u = 0; u < 4; ++u) {
				kk = tv[u].x; ll = tv[u].y;
				const bool dead = kk > ll;
				if (dead) { kk = 0; ll = BX(seq_len); ++bid; }
				out_pos(wi, false);
				++wi;
				if (STATS) ++st_pos[1];
				if (dead) { rekey(wi); break; }
			}
			if (STATS) ++st_lt[1];
		} else if (run) {
			const int pos = sbase + wi;
			if ((pos >> 4) != stag) { const uint4 q = *(const uint4*)((x ? P.rseq : P.seq) + sq_off + (pos & ~15)); WIN_SET(slo, shi, q.x, q.y, q.z, q.w); stag = pos >> 4; }
			const int cc = (int)byte_of(slo, shi, (uint32_t)pos & 15u);
			// issue the loads of this step before consuming any (one memory latency per trip)
			uint4 qa[4], qb[4]; uint32_t rk = 0, rl = 0, sav = 0; bool kval = false, two = false;
			// (qa and qb are read only where q, and two, loaded them -- but left unset they cost 68 spilled VGPRs and 208 bytes of scratch)
#pragma unroll
			for (int u = 0; u < 4; ++u) { qa[u] = make_uint4(0, 0, 0, 0); qb[u] = make_uint4(0, 0, 0, 0); }
			const bool q = cc < 4 && !tmode;
			if (STATS) { if (q) ++st_lt[2]; else ++st_lt[3]; }
			if (q) {
				const uint32_t primary = BX(primary), kq = kk - 1u, lq = ll;
				const uint32_t kp = kq - (kq >= primary ? 1u : 0u), lp = lq - (lq >= primary ? 1u : 0u);
				const uint32_t bl = lp / NABWA_INTV; rl = lp - bl * NABWA_INTV;
				kval = kq != 0xffffffffu;
				const uint32_t bkk = kval ? kp / NABWA_INTV : bl; rk = kp - bkk * NABWA_INTV;
				two = bkk != bl;
				const uint4 *const bkt = BX(bk);
				const uint4 *pl = bkt + (size_t)bl * 4, *pk = bkt + (size_t)bkk * 4;
#pragma unroll
				for (int u = 0; u < 4; ++u) qa[u] = pl[u];
				if (two) {
#pragma unroll
					for (int u = 0; u < 4; ++u) qb[u] = pk[u];
				}
				if (COUNT) touches += ref_touches(x ? P.bwt[1] : P.bwt[0], kq, lq, false);
				// one row left: fetch its text position alongside this step's query (the step moves it one to the left)
				if (text_ok && kk == ll) sav = BX(sa_full)[kk];
			}
			if (tmode && tp > 0u && ((tp - 1u) >> 5) != twtag) {
				twtag = (tp - 1u) >> 5;
				twin = *(const uint2*)(BX(text) + 2 * (size_t)twtag);
			}
			if (tmode) {
				bool ok = cc < 4 && tp > 0u;
				if (ok) {
					const uint32_t t = tp - 1u, wd = (t & 16u) ? twin.y : twin.x;
					ok = (wd >> ((t & 15u) << 1) & 3u) == (uint32_t)cc;
					if (ok) tp = t;
				}
				if (cc > 3 && x == 0u && phase == 0) ++nN;
				if (!ok) { tmode = false; kk = 0; ll = BX(seq_len); ++bid; rekey(wi + 1); }   // the restart of bwtaln.c:66-70
			} else {
				const bool was_one = text_ok && cc < 4 && kk == ll;
				if (cc < 4) {
					Occ4 ck, cl;
					ck.c[0] = ck.c[1] = ck.c[2] = ck.c[3] = 0;
					cl = nabwa_count4(qa[0], qa[1], qa[2], qa[3], rl);
					if (kval) {
						const uint4 s0 = two ? qb[0] : qa[0], s1 = two ? qb[1] : qa[1], s2 = two ? qb[2] : qa[2], s3 = two ? qb[3] : qa[3];
						ck = nabwa_count4(s0, s1, s2, s3, rk);
					}
					const uint32_t L2c = cc == 0 ? BX(L2[0]) : (cc == 1 ? BX(L2[1]) : (cc == 2 ? BX(L2[2]) : BX(L2[3])));
					const uint32_t ok = cc == 0 ? ck.c[0] : (cc == 1 ? ck.c[1] : (cc == 2 ? ck.c[2] : ck.c[3]));
					const uint32_t ol = cc == 0 ? cl.c[0] : (cc == 1 ? cl.c[1] : (cc == 2 ? cl.c[2] : cl.c[3]));
					kk = L2c + ok + 1u; ll = L2c + ol;
				} else if (x == 0u && phase == 0) ++nN;
				if (kk > ll || cc > 3) { kk = 0; ll = BX(seq_len); ++bid; rekey(wi + 1); }
				else if (was_one) { tmode = true; tp = sav - 1u; twtag = 0xffffffffu; }
			}
			out_pos(wi, false);
			if (wi + 1 == n) out_pos(wi + 1, true);
			++wi;
		}
		// the end of a pass, whichever trip reached it (before v15: the single step alone)
		if (run && wi == n) {
			if (phase == 0 && P.rd_cls) P.rd_cls[2 * (size_t)rid + x] = (uint8_t)(bid - 1 > 4 ? 4 : bid - 1);   // restarts of this strand's pass (bid counts the terminator too, bwtaln.c:66-74)
			if (phase == 0 && len > P.seed_len) {
				phase = 1; wi = 0; n = P.seed_len; sbase = len - P.seed_len; tmode = false;
				if (KT) { wkey = P.rd_key[6 * (size_t)rid + 4 + x]; tok = wkey != 0xffffffffu; }
				tbase = 0;
				kk = 0; ll = BX(seq_len); bid = 0; pw = 0;
			} else {
				if (x == 0u) P.rd_nN[rid] = (uint8_t)(nN > 255 ? 255 : nN); run = false;
				if (STATS) { st_max = max(st_max, st_item); st_item = 0u; }
			}
		}
	}
	if (STATS && P.touch_counter) {      // positions of the single steps = their lane-trips: slots TS_W_RANK and TS_W_STEP carry the seed-pass text trips and nothing above them
		unsigned long long v[4] = { (unsigned long long)st_lt[0] << 32 | st_pos[0], (unsigned long long)st_lt[1] << 32 | st_pos[1],
									(unsigned long long)st_tx1 << 32 | st_lt[2], (unsigned long long)st_lt[3] };
		for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
			for (int u = 0; u < 4; ++u) v[u] += __shfl_down(v[u], o);
			st_max = max(st_max, (uint32_t)__shfl_down((int)st_max, o));
		}
		if (lane == 0) {
			atomicAdd(P.touch_counter + TS_W_TRIPS, (unsigned long long)st_wave); atomicMax(P.touch_counter + TS_W_MAX, (unsigned long long)st_max);
			atomicAdd(P.touch_counter + TS_W_TEXT, v[0]); atomicAdd(P.touch_counter + TS_W_TABLE, v[1]); atomicAdd(P.touch_counter + TS_W_RANK, v[2]); atomicAdd(P.touch_counter + TS_W_STEP, v[3]);
		}
	}
	if (COUNT) {
		for (int o = 32; o > 0; o >>= 1) touches += __shfl_down(touches, o);
		if (lane == 0 && P.touch_counter) atomicAdd(P.touch_counter + TS_TOUCH_W, touches);
	}
#undef WREC
#undef BX
}
// =====================================================================================
// Kernel S: bwt_match_gap (bwtgap.c:104-266), one read per lane, exact pop/push order.
//
// Every trip of the wave loop has three phases so that it pays ONE memory latency:
//   1. decide (registers + LDS only): pop the pending entry or pick the arena slot to pop,
//      run the pre-checks that need no memory, choose what this lane does in this trip;
//   2. issue every global load the lane needs -- arena entry, bound-byte window, read-base
//      window, seed-bound window, one or two Occ buckets -- back to back, no use in between;
//   3. consume: park a fetched entry, finish the pre-check, take an exact-tail step, land a jump, expand, or record a hit.
// When the bound window is stale at pop time the rank query is issued speculatively together
// with the window; if the entry then turns out to be pruned (bwtgap.c:156) the counts are dropped.
// =====================================================================================
enum {           // a lane's state between trips
	LS_IDLE  = 0,
	LS_POP   = 1,   // needs to pop
	LS_HAVE  = 2,   // the entry popped from the arena in the previous trip is in e_*
	LS_EXACT = 3,   // inside an exact tail (bwt.c:237-252), next position e_i - 1
	LS_EXIT  = 4
};
enum {           // what a lane does with its current entry in one trip: what the trip loads, and the state `st` it leaves
	TK_NONE      = 0,   // nothing: no entry, an entry pruned at the pop, or a pop whose arena entry is only fetched; st as phase 1 set it
	TK_EXPAND    = 1,   // a rank query (rows), 32 bytes of the next table level (key form) or the text word (text form): children pushed; LS_POP
	TK_TAIL      = 2,   // one exact-tail step on rows, a rank query: LS_EXACT, LS_POP when the interval dies or the hit is recorded
	TK_HIT       = 3,   // an entry with i == 0 is recorded, no query (text form: its row from isa): LS_POP
	TK_JUMP      = 4,   // a tail or forced walk lands at depth KT, one level-KT table entry: LS_EXACT (tail), LS_HAVE (forced), LS_POP (empty)
	TK_GROUP     = 5,   // a deletion popped from a gap group, the parent's rank query again: LS_HAVE as that child
	TK_ROWS      = 6,   // a key-form entry takes on rows, one table entry of its level: LS_HAVE as the same entry in row form (popped from a gap group: as that member)
	TK_TEXT_TAIL = 7    // an exact tail compared with the text, one text word: LS_EXACT, LS_HAVE at i == 0 (reported next trip), LS_POP on a mismatch
};

template <bool COUNT>
__global__ __launch_bounds__(NABWA_SEARCH_BLOCK, NABWA_MIN_WAVES) void fm_search_kernel(const SearchParams P_)
{
	SearchParams P = P_;
	// the gap options as scalar values of their own (nabwa_dev.hpp: own): they arrive as one 256-bit tuple, which this kernel -- it has
	// more uniform values than scalar registers -- spilled whole and read back, all eight dwords, at 26 places.  (Doing the same for
	// EVERY argument removes more v_readlane instructions still, 492 -> 212, and makes the kernel 3 % slower; for the index
	// descriptors' scalars, their pointers, the batch's pointers or the per-read arrays' pointers alone: 1 - 7 % slower.  Measured, not kept.)
	own(P.n); own(P.s_mm); own(P.s_gapo); own(P.s_gape); own(P.mode); own(P.indel_end_skip); own(P.max_del_occ); own(P.max_entries);
	own(P.max_gape); own(P.max_seed_diff); own(P.seed_len); own(P.max_top2);
	const uint32_t NIL = 0xffffu;
	const uint32_t lane = threadIdx.x & 63u;
	const size_t slot = (size_t)blockIdx.x * NABWA_SEARCH_BLOCK + threadIdx.x;
	uint8_t *const sc = P.scratch + slot * P.lane_stride;
	uint4 *const ent = (uint4*)sc;
	const bool gape_mode = P.mode & 0x01, nonstop = P.mode & 0x10, loggap = P.mode & 0x04;

	int st = LS_IDLE;
	unsigned int w_next = 0, w_end = 0; bool w_sync = false;   // this wave's block of read numbers; lockstep mode
	// per-read
	uint32_t item = 0; int len = 0; uint32_t mdmg = 0;   // mdmg: this read's max_diff | max_gapo << 8
	uint32_t sq_off = 0;                                    // this read's offset in the padded base arrays
	const int KT = (int)P.bwt[0].kmer_T;                    // 0 in the touch-counting run
	// the hand-over budget: in a batch most of whose reads occur exactly on neither strand (the width passes counted them: *n_sync, the reads in front
	// of the class-0 ones in the work order) the searches are bushy ones -- kernel D's kind -- and go there sooner (2 x 150 bp at 2 %: S 133 + D 90 ms
	// at 2000 trips, S 17 + D 154 ms at 200; 100 bp at 0.2 %: 2000 is the optimum; profiles/r03_deep_variants.txt)
	uint32_t budget = P.trip_budget;
	if (!COUNT && P.n_sync && P.trip_budget_hard && 2u * (uint32_t)__builtin_amdgcn_readfirstlane((int)*P.n_sync) > (uint32_t)P.n) budget = P.trip_budget_hard;
#define RID item                                            /* results and width records are indexed by read */
#define REC (P.wdata + (size_t)RID * P.wstride)            /* this read's width record (kernel W) */
#define MD_READ ((int)(mdmg & 0xffu))
#define MG_READ ((int)(mdmg >> 8 & 0xfu))    /* (at most 15 here: option blocks beyond that go to kernel D whole) */
	// current interval
	uint32_t k = 0, l = 0;
	// search globals
	int max_diff = 0, best_score = 0, best_cnt = 0, n_aln = 0, max_ent = 0, n_entries = 0;
	uint32_t bump = 0; uint64_t mask_lo = 0; bool seeded = false; int status = 0;   // masks: non-empty scores; the first pass has at most 64 levels (host) and uses mask_lo only
	// current entry
	int e_i = 0, e_a = 0, e_mm = 0, e_go = 0, e_ge = 0, e_state = 0, e_ldp = 0, e_score = 0, m = 0;
	// pending entry: the last child pushed by the previous expansion, still in registers
	// (kept in the 16-byte arena format, so spilling it is one store and popping it is the arena unpack; p_score < 0: none)
	uint4 pe = make_uint4(0, 0, 0, 0); int p_score = -1;
#define p_valid (p_score >= 0)
	// register windows over read data / the width record
	// 16-byte windows over read data / the width record live in LDS (first pass), [lane][16 bytes], filled by
	// global_load_lds_dwordx4 (no registers in between; layout checked by profiles/probes/lds_dma_probe.hip) and read a byte at a time
	int sq_tag = -1;                     // 16 read bases
	int bw_base = -1, bw_a = -1;         // 16 bound bytes of strand bw_a from bw_base
	int sw_base = -1, sw_a = -1;         // same for the seed bounds
	unsigned long long touches = 0; uint32_t rd_touch = 0, rd_trips = 0;  // COUNT only
	uint32_t rk_kf = 0, rk_row2 = 0, rk_row1 = 0, rk_tx = 0, rk_pop = 0, rk_tail = 0, rk_jump = 0, rk_gap = 0;   // COUNT only: this read's trips by kind (TS_LONG_*)
	unsigned long long st_trips = 0, st_expand = 0, st_exact = 0, st_ent = 0, st_spec = 0, st_query = 0, st_two = 0, st_exit = 0, st_jump = 0, st_txe = 0, st_txt = 0;
	bool ovf = false;
	// A read one of whose strands occurs exactly (kernel W's class 0; DESIGN.md 4, "sure0").  Its first hit is the exact one, at score 0, after which max_diff is 1
	// and the search ends at the first pop above s_mm (bwtgap.c:144,166-172): so, from the first trip on, an entry above s_mm is never popped, and a popped
	// 1-mismatch child is an exact tail;
	// the flag and what it counts share the register of the read's max_diff: mdmg bit 31 the flag (S0_ON), bit 30: store survivors landed (S0_LAND),
	// bits 16-22 / 23-29 this read's key-form children whose level-KT entry was empty / that were stored landed (at most 3 per level, KT - 1 levels, two strands),
	// bits 12 / 13 (above max_gapo, which is at most 15 in this kernel): strand 0 / 1 itself occurs exactly -- its class byte is 0 -- and the leap is on (S0_PRV << strand)
#define s0f mdmg
#define S0_ON  0x80000000u
#define S0_LAND 0x40000000u
#define S0_WAS 0x8000u      /* the flag was set at refill (it may be dropped on the way): the read is counted at its end */
#define S0_PRV 0x1000u

	auto head_get = [&](int score) -> uint32_t {
		return (uint32_t)s_head[score * NABWA_SEARCH_BLOCK + threadIdx.x];
	};
	auto head_set = [&](int score, uint32_t v) {
		s_head[score * NABWA_SEARCH_BLOCK + threadIdx.x] = (uint16_t)v;
	};
	auto mask_has = [&](int score) -> bool { return mask_lo >> score & 1ull; };
	auto mask_set = [&](int score) { mask_lo |= 1ull << score; };
	auto mask_clr = [&](int score) { mask_lo &= ~(1ull << score); };
	auto mask_any = [&]() -> bool { return mask_lo != 0ull; };
	auto mask_first = [&]() -> int {          // lowest non-empty score, 0x7fffffff when none
		return mask_lo ? __ffsll((unsigned long long)mask_lo) - 1 : 0x7fffffff;
	};
	// After the first hit best_score is final (bwtgap.c:170), and the loop ends at the first pop whose score
	// exceeds best_score + s_mm (bwtgap.c:144): such a child can never be expanded.  It is still COUNTED
	// (n_entries feeds max_entries and the bwtgap.c:140 cut-off) but never written to the arena.
	// (Before the first hit best_score is its start value, which no entry's score exceeds: that is what bwtgap.c:144 itself relies on.  A sure0 read
	// starts with best_score = 0, the score its first hit is known to have, so for it the rule holds from the first trip on.)
	auto never_popped = [&](int score) -> bool { return !nonstop && score > best_score + P.s_mm; };
	// append an entry to the in-memory list of its score (n_entries is maintained by the callers)
	// the arena word of an entry: {k, l, i | last_diff_pos << 16, counters / state / strand (+ the list link, first pass)}
	auto mk_entry = [&](uint32_t nk, uint32_t nl, int ni, int nldp, int nmm, int ngo, int nge, int nstate, int na) -> uint4 {
		const uint32_t z = (uint32_t)ni | (uint32_t)nldp << 16;
		return make_uint4(nk, nl, z, (uint32_t)nmm << 16 | (uint32_t)ngo << 20 | (uint32_t)nge << 24 | (uint32_t)nstate << 29 | (uint32_t)na << 31);
	};
	auto push_mem = [&](int score, uint4 e) {
		if (ovf || never_popped(score)) return;
		if ((uint32_t)score >= P.NS) { ovf = true; return; }       // cannot happen (nabwa_batch.hip sizes NS); the second pass would take over
		if (bump >= P.cap) { ovf = true; return; }
		const uint32_t s = bump++;
		const uint32_t prev = mask_has(score) ? head_get(score) : NIL;
		e.w |= prev;
		ent[s] = e;
		head_set(score, s);
		mask_set(score);
	};

	// first pass only: the entry at the head of the lowest non-empty score list is fetched ahead of its pop while the
	// lane walks an exact tail (a tail pushes nothing, so that head IS the next pop) and parked in LDS
	uint4 *const s_pf = (uint4*)(s_head + (size_t)P.NS * NABWA_SEARCH_BLOCK);
	uint2 *const s_key = (uint2*)(s_pf + NABWA_SEARCH_BLOCK);
	// Text mode (nabwa_dev.hpp).  An interval of ONE row is carried as {k = text position of that row's suffix, l = TXM}:
	// extending it by a symbol is a comparison with the text base to the left of the suffix, its only non-empty child
	// is the suffix one position further left, and rows are recovered (isa) only where one is reported.  Entries of
	// either form live side by side in the stacks.  s_tw: this lane's 16-base text word and its tag.
	uint2 *const s_tw = s_key + NABWA_SEARCH_BLOCK;
	uint32_t *const s_bw = (uint32_t*)(s_tw + NABWA_SEARCH_BLOCK), *const s_sw = s_bw + 4 * NABWA_SEARCH_BLOCK, *const s_sq = s_sw + 4 * NABWA_SEARCH_BLOCK;
	// s_fb: per strand (byte a) the lower bound of differences of the read's first len-KT symbols, bound[len-KT-1] -- what
	// decides whether every level down to depth KT is a forced match (see the tail jump); 0xff: unknown / no longer valid
	uint32_t *const s_fb = s_sq + 4 * NABWA_SEARCH_BLOCK;
	auto win_byte = [&](const uint32_t *W, uint32_t idx) -> uint32_t {
		return (uint32_t)((const uint8_t*)W)[(threadIdx.x << 4) + idx];
	};
	// 16 bytes from global memory into this lane's window slot
	auto win_load = [&](const void *src, uint32_t *W) {
		__builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src,
										 (void __attribute__((address_space(3)))*)(W + ((threadIdx.x & ~63u) << 2)), 16, 0, 0);
	};
#define BW_BYTE(i_) win_byte(s_bw, (uint32_t)(i_))
#define SW_BYTE(i_) win_byte(s_sw, (uint32_t)(i_))
#define SQ_BYTE(i_) win_byte(s_sq, (uint32_t)(i_))
	// Key form.  With all levels of the interval table present, a gap-free entry of depth d <= KT (d = len - i reference symbols
	// matched, substitutions included) needs no interval at all: its path key addresses level d, its four children are the
	// 32 bytes at level d+1, its exact tail or forced walk lands at level KT under (key ++ the read's next symbols).  Such
	// entries are carried as {k = key, l = KEYM}, are expanded without a rank query, and take on rows (one table load)
	// when they are reported, reach depth KT, or yield a gap child that is popped.
	const bool kf_ok = KT > 0 && (int)P.bwt[0].kmer_LW == KT && (int)P.bwt[1].kmer_LW == KT && (P.text_mode & 4);
	const bool text_ok = (P.text_mode & 2) && P.bwt[0].sa_full && P.bwt[1].sa_full && P.bwt[0].seq_len < 0xfffffff0u;
	uint32_t pf_slot = NIL;
	bool finish = false;
	// unpack a popped arena entry into the current-entry registers and unlink it (bwtgap.c:66-79)
	auto unpack = [&](const uint4 &r) {
		k = r.x; l = r.y; e_i = (int)(r.z & 0xffffu); e_ldp = (int)(r.z >> 16);
		e_mm = (int)(r.w >> 16 & 15u); e_go = (int)(r.w >> 20 & 15u); e_ge = (int)(r.w >> 24 & 31u);
		e_state = (int)(r.w >> 29 & 3u); e_a = (int)(r.w >> 31);
	};
	auto take_entry = [&](const uint4 &r_ent) {
		unpack(r_ent);
		const uint32_t nx = r_ent.w & 0xffffu;
		head_set(e_score, nx);
		if (nx == NIL) mask_clr(e_score);
		--n_entries;
		if (!nonstop && e_score > best_score + P.s_mm) finish = true;    // bwtgap.c:144
	};

	for (;;) {
		finish = false;
		// ---------------------------------------------------------------- refill
		unsigned long long need = __ballot(st == LS_IDLE);
		const bool any_busy = __ballot(st != LS_IDLE && st != LS_EXIT) != 0ull;
		// reads whose search is known to run alike (an exact occurrence exists: kernel W's class 0, sorted to the end) are
		// taken 64 at a time by a wave with all lanes idle, so its lanes stay in step and its trips stay converged
		if ((P.sync_refill || w_sync) && any_busy) need = 0ull;
		if (need) {
			if (w_next == w_end) {          // blocks of read numbers per wave, as in kernel W
				unsigned int b0 = 0;
				if (lane == 0) b0 = atomicAdd(P.work_counter + WC_SEARCH, (unsigned int)NABWA_WORK_CHUNK);
				w_next = __builtin_amdgcn_readfirstlane(b0); w_end = w_next + NABWA_WORK_CHUNK;
				// class 0 (end of the work order): lockstep.  Class 2+ (start of the work order): also 64 reads at a time without
				// refilling -- not for convergence but for the stragglers: the fewer lanes of a wave are still searching, the fewer
				// code paths a trip runs through, and the launch waits for exactly those reads (class 2+'s size, seen from n_sync)
				w_sync = P.n_sync && (w_next >= *P.n_sync || w_next < P.n_sync[NCLS_SIZE + 2 - NCLS_FIRST0]);
			}
			const unsigned int rank = (unsigned int)__popcll(need & ((1ull << lane) - 1ull)), avail = w_end - w_next;
			const unsigned int base = w_next;
			w_next += min((unsigned int)__popcll(need), avail);
			if (st == LS_IDLE && rank < avail) {
				const unsigned int idx = base + rank;
				if (idx < (unsigned int)P.n) {
					const uint32_t rid = P.ids ? (uint32_t)P.ids[idx] : idx;
					item = rid;
					const int64_t o = P.poff[rid];
					len = P.rd_len[rid];
					sq_off = (uint32_t)o;
					mdmg = (uint32_t)P.rd_maxdiff[rid] | (uint32_t)P.rd_maxgapo[rid] << 8;
					if (KT) {
						s_key[threadIdx.x] = *(const uint2*)(P.rd_key + 6 * (size_t)rid);   // interval-table keys of the two strands
						uint32_t fb = 0xffffu;
						if (len > KT) { const uint8_t *const bb = REC + P.woff_bid + (len - KT - 1); fb = (uint32_t)(bb[0] & 127u) | (uint32_t)(bb[P.WLB] & 127u) << 8; }
						s_fb[threadIdx.x] = fb;
					}
					n_aln = 0; max_ent = 0; status = NABWA_ST_OK; rd_touch = 0; rd_trips = 0; ovf = false;
					rk_kf = rk_row2 = rk_row1 = rk_tx = rk_pop = rk_tail = rk_jump = rk_gap = 0;
					sq_tag = -1; bw_a = -1; sw_a = -1; p_score = -1; pf_slot = NIL;
					if (text_ok) s_tw[threadIdx.x] = make_uint2(0u, 0x7fffffffu);
					// by the class bytes of the read itself (chunks of the work order straddle the class boundary); not where the entry count could come
					// near the bwtgap.c:140 cut-off (checked again at every expansion: one adds at most 9 entries, and 4 * len >= 9 for every read with a key)
					if (!COUNT && P.sure0 && P.rd_cls && !nonstop && P.s_gapo > P.s_mm && MD_READ >= 1 && len > 0 && 2 + 4 * len <= P.max_entries) {
						const uint32_t cw = *(const uint16_t*)(P.rd_cls + 2 * (size_t)rid);
						if ((cw & 0xffu) == 0u || (cw >> 8) == 0u) {
							s0f |= P.sure0 > 1 ? S0_ON | S0_LAND | S0_WAS : S0_ON | S0_WAS;
							if (P.sure0 > 2) s0f |= ((cw & 0xffu) == 0u ? S0_PRV : 0u) | ((cw >> 8) == 0u ? S0_PRV << 1 : 0u);
						}
					}
					if (len > 0 && (int)P.rd_nN[rid] <= MD_READ) {      // too many N: no search (bwtgap.c:118-123)
						// ---- start of bwt_match_gap (bwtgap.c:104-128)
						seeded = len > P.seed_len;
						max_diff = MD_READ;
						best_score = (s0f & S0_ON) ? 0 : (MD_READ + 1) * P.s_mm + (MG_READ + 1) * P.s_gapo + (P.max_gape + 1) * P.s_gape;
						best_cnt = 0;
						// roots: strand 0 is pushed first, strand 1 second -> strand 1 (pending) is expanded first
						bump = 0; mask_lo = 0ull;
						push_mem(0, mk_entry(0u, kf_ok ? KEYM : P.bwt[0].seq_len, len, 0, 0, 0, 0, STATE_M, 0));
						pe = mk_entry(0u, kf_ok ? KEYM : P.bwt[0].seq_len, len, 0, 0, 0, 0, STATE_M, 1); p_score = 0;
						n_entries = 2;
						st = LS_POP;
					} else { P.n_aln[item] = 0; P.max_ent[item] = 0; P.status[item] = NABWA_ST_OK; }
				} else st = LS_EXIT;
			}
		}
		if (__ballot(st != LS_EXIT) == 0ull) break;

		// ================================================================ phase 1: decide (no global loads)
		bool want_ent = false; uint32_t ent_slot = 0;
		bool have = st == LS_HAVE;
		if (st == LS_POP) {
			if (n_entries == 0) finish = true;
			else {
				if (max_ent < n_entries) max_ent = n_entries;
				if (n_entries > P.max_entries) finish = true;                 // bwtgap.c:140
				// a search that is still running after trip_budget trips is handed on to kernel D, which gives it a whole wave: the
				// launch cannot end before its longest lane does, and one lane walks a long search pop by pop
				else if (!COUNT && P.trip_budget && rd_trips > budget) { status = NABWA_ST_OVERFLOW; finish = true; }
			}
			if (!finish) {
				const int best_mem = mask_first();
				if (p_valid && p_score <= best_mem) {
					// the pending child is the newest entry of the lowest score: it is the pop
					unpack(pe);
					e_score = p_score; p_score = -1;
					--n_entries;
					if (!nonstop && e_score > best_score + P.s_mm) finish = true;    // bwtgap.c:144
					else have = true;
				} else if (best_mem == 0x7fffffff) {
					finish = true;      // only never-stored children are left: the reference pops one of them and stops (bwtgap.c:144)
				} else {
					if (p_valid) { push_mem(p_score, pe); p_score = -1; }
					if (ovf) { status = NABWA_ST_OVERFLOW; finish = true; }
					else {
						ent_slot = head_get(best_mem); e_score = best_mem;
						if (ent_slot == pf_slot) {                          // already here: pop it and go on in this trip
							const uint4 r = s_pf[threadIdx.x];
							take_entry(r);
							pf_slot = NIL;
							if (!finish) have = true;
						} else want_ent = true;
					}
				}
			}
		}
		// what this lane does with its current entry in this trip
		int kind = TK_NONE;
		bool need_win = false, spec = false, forced = false; int win_hi = 0;
		int grp_c = 0, mlev = -1, mpost = 0; uint32_t midx = 0; bool kx = false;      // mlev/midx: table entry that turns a key-form entry into rows (TK_ROWS)
		if (have && !finish && e_state == STATE_GROUP) {
			// pop ONE member of a gap group, newest first (deletion of T, G, C, A, then the insertion); the rest goes back
			// on the stack it came from, where it is again the top
			const uint32_t mk = (uint32_t)e_ldp & 0x1fu, ext = (uint32_t)e_ldp & GRP_EXT, more = (uint32_t)e_ldp >> 9;
			const int j = 31 - __clz((int)mk);
			const uint32_t rest = mk & ~(1u << j);
			if (rest) push_mem(e_score, mk_entry(k, l, e_i, (int)(rest | ext | more << 9), e_mm, e_go, e_ge, STATE_GROUP, e_a));
			else if (more) push_mem(e_score, mk_entry(k + 1u, l, e_i + 1, (int)(3u | (more - 1u) << 9), e_mm, e_go, e_ge, STATE_GROUP, e_a));   // (text form) the next older level
			if (ovf) { status = NABWA_ST_OVERFLOW; finish = true; }
			if (ext) ++e_ge; else ++e_go;
			if (l == KEYM) {                                                // key form: the parent (depth len - e_i - 1) or its child j-1, as rows
				const int dp = len - e_i - 1;
				kind = TK_ROWS; st = LS_POP; have = false;
				if (j == 0) { mpost = 1; mlev = dp; midx = k; } else { mpost = 2; mlev = dp + 1; midx = k * 4u + (uint32_t)(j - 1); }
			}
			else if (j == 0) { e_state = STATE_I; e_ldp = e_i; }            // the insertion keeps the parent's interval
			else if (l == TXM) { k -= 1u; e_i += 1; e_state = STATE_D; e_ldp = e_i; }   // text form: the deleted base is the one to the left
			else { kind = TK_GROUP; grp_c = j - 1; st = LS_POP; have = false; }    // a deletion: re-derive its interval
		}
		if (have && !finish) {
			st = LS_POP;
			m = max_diff - (e_mm + e_go); if (gape_mode) m -= e_ge;
			if (m >= 0) {
				const bool kf = l == KEYM;
				const int d = len - e_i;                                      // depth of a gap-free entry
				if (e_i == 0) { if (kf) { kind = TK_ROWS; mlev = d; midx = k; } else kind = TK_HIT; }
				else {
					// the pre-check needs bound[e_i-1]; an expansion then needs bound[e_i-2] as well
					const bool tail = m == 0 && (e_state == STATE_M || gape_mode || e_ge == P.max_gape);
					// a 1-mismatch child stored landed (see the expansion) is checked against the bound at its own position, as when it was created there
					const bool landed = e_state == STATE_M && e_ldp > e_i;
					win_hi = landed ? e_ldp - 1 : e_i - 1;
					const int win_lo = landed ? win_hi : ((tail || e_i < 2) ? e_i - 1 : e_i - 2);
					bool go = true;
					if (bw_a == e_a && win_lo >= bw_base && win_hi < bw_base + 16) {
						if (m < (int)(BW_BYTE(win_hi - bw_base) & 127u)) go = false;   // bwtgap.c:156
					} else { need_win = true; spec = true; }
					if (go) {
						const bool rdkey_ok = KT && (e_a ? s_key[threadIdx.x].y : s_key[threadIdx.x].x) != 0xffffffffu;
						// row form: the path is known when it is the read's own symbols with at most the one just consumed substituted
						const bool row_known = l != TXM && !kf && (e_go | e_ge) == 0 && e_state == STATE_M && (e_mm == 0 || (e_mm == 1 && e_ldp == e_i));
						if (tail) {                                 // nothing may differ any more: exact tail (bwt.c:237-252)
							kind = TK_TAIL;                                   // its cursor is e_i: position e_i - 1 is consumed next
							// tail jump: the interval after KT symbols (the path so far, then the read's own) is one table entry away
							if (l == TXM) kind = TK_TEXT_TAIL;                  // text form: compare the rest of the read with the text
							else if (kf) { if (rdkey_ok) kind = TK_JUMP; else { kind = TK_ROWS; mlev = d; midx = k; } }
							else if (rdkey_ok && row_known && d <= KT) kind = TK_JUMP;
						}
						else {
							// Forced matches.  Differences are allowed at a level only where the bound of the symbols still to
							// come is below m (bwtgap.c:204-207); the bounds never grow towards the read's start, and this entry
							// was not pruned, so bound[len-KT-1] == m means: on every level down to depth KT the only child is
							// the matching one, popped at once (same score, newest) -- an exact walk in all but name.  For an entry
							// whose path is known the table gives the interval it arrives with, or that it dies.
							forced = rdkey_ok && d < KT && (kf || row_known) && (int)(s_fb[threadIdx.x] >> (e_a << 3) & 0xffu) == m;
							if (forced) kind = TK_JUMP;
							else if (kf && d >= KT) { kind = TK_ROWS; mlev = d; midx = k; }     // depth KT: rows from here on
							// The leap ("sure0").  A text-form entry that is the read's own prefix on a strand kernel W proved to occur: its one row
							// IS that occurrence, so every symbol still to come matches the text, every mismatch sibling is empty, and the gap children of those
							// levels are counted and never stored (their score is above s_mm).  The walk would end in the suffix e_i positions further left with
							// i == 0: that entry is made here and reported in this same trip (TK_HIT), with the entries the walk's levels would have counted.
							// (k < e_i cannot be for a real occurrence; such an entry walks as before.)
							else if (l == TXM && (s0f & S0_ON) && (s0f & S0_PRV << e_a) && e_state == STATE_M && (e_mm | e_go | e_ge) == 0
									 && n_entries + 4 * len <= P.max_entries && k >= (uint32_t)e_i) {
								// On this strand every bound and seed bound is 0 while entries of score 0 are popped, so a level icur (e_i-1 .. 0) pushes its
								// insertion and its deletion (bwtgap.c:216-240) iff it is clear of both read ends, an opening is left, and -- inside the
								// seed -- max_seed_diff allows a difference (m == max_diff >= 1 here: no counted difference yet, and this is no tail)
								const int ies = P.indel_end_skip + (loggap ? 1 : 0);
								int hi = e_i - 1;
								if (hi > len - ies) hi = len - ies;
								if (seeded && P.max_seed_diff < 1 && hi > len - P.seed_len) hi = len - P.seed_len;
								const int gl = (MG_READ > 0 && hi >= ies) ? hi - ies + 1 : 0;
								if (P.s0_stats) { atomicAdd(P.s0_stats + S0S_LEAPS, 1ull); atomicAdd(P.s0_stats + S0S_LEAP_LEVELS, (unsigned long long)e_i); }
								// the chain's entry count only rises, so its peak is at the pop of the last entry: n_entries + 2 per such level + that entry
								n_entries += 2 * gl;
								if (max_ent < n_entries + 1) max_ent = n_entries + 1;
								k -= (uint32_t)e_i; e_i = 0; e_ldp = 0;
								kind = TK_HIT; need_win = false; spec = false;
							}
							else {
								if (P.s0_stats && l == TXM && (s0f & S0_ON) && (s0f & S0_PRV << e_a) && e_state == STATE_M && (e_mm | e_go | e_ge) == 0
									&& n_entries + 4 * len <= P.max_entries) atomicAdd(P.s0_stats + S0S_WALKED, 1ull);     // (then k < e_i)
								kind = TK_EXPAND; --e_i; kx = kf;
								if ((s0f & S0_ON) && n_entries + 4 * len > P.max_entries) s0f &= ~S0_ON;
							}
						}
					}
				}
			}
		} else if (st == LS_EXACT) kind = l == TXM ? TK_TEXT_TAIL : TK_TAIL;
		// a key-form entry turned into rows becomes the current entry of the next trip; a popped gap member takes its shape now
		auto rows_arrived = [&](uint32_t nk, uint32_t nl) {
			k = nk; l = nl;
			if (mpost == 1) { e_state = STATE_I; e_ldp = e_i; }
			else if (mpost == 2) { e_i += 1; e_state = STATE_D; e_ldp = e_i; }
			st = LS_HAVE;
		};
		if (kind == TK_ROWS && mlev == 0) { rows_arrived(0u, e_a ? P.bwt[0].seq_len : P.bwt[1].seq_len); kind = TK_NONE; }   // depth 0: every row

		const int qb = 1 - e_a;
		const bool tx = l == TXM && (kind == TK_EXPAND || kind == TK_HIT || kind == TK_TEXT_TAIL);
		const int spos = (kind == TK_TAIL || kind == TK_TEXT_TAIL) ? e_i - 1 : e_i;
		const int stag = (e_a << 20) | (spos >> 4);
		const bool need_seq = (kind == TK_EXPAND || kind == TK_TAIL || kind == TK_TEXT_TAIL) && stag != sq_tag;
		bool query = (kind == TK_EXPAND && !tx && !kx) || kind == TK_TAIL || kind == TK_GROUP;
		// text word in front of the suffix (TK_EXPAND and TK_TEXT_TAIL in text form)
		uint2 tw = make_uint2(0u, 0u); bool need_tw = false;
		if (tx && kind != TK_HIT && k > 0u) {
			const uint32_t tag = ((k - 1u) >> 4) | (uint32_t)qb << 31;
			tw = s_tw[threadIdx.x];
			need_tw = tw.y != tag;
			tw.y = tag;
		}
		const bool to_text = kind == TK_EXPAND && !tx && !kx && text_ok && k == l;   // one row left: its children go on in text form
		if (kind == TK_TAIL && !need_seq && SQ_BYTE((uint32_t)spos & 15u) > 3u) query = false;   // an N: no query
		const int ii = e_i - (len - P.seed_len);
		const bool use_seed = kind == TK_EXPAND && e_i > 0 && seeded && ii > 0;
		const bool need_seed = use_seed && !(sw_a == e_a && ii - 1 >= sw_base && ii < sw_base + 16);

		// ================================================================ phase 2: issue every load
		uint4 r_ent = make_uint4(0, 0, 0, 0);
		if (need_win) {
			int base = (win_hi | 7) - 15; if (base < 0) base = 0;
			win_load(REC + P.woff_bid + e_a * P.WLB + base, s_bw); bw_base = base; bw_a = e_a;
		}
		if (need_seq) {
			win_load((e_a ? P.rseq : P.seq) + sq_off + (spos & ~15), s_sq); sq_tag = stag;
		}
		if (need_seed) {
			int base = (ii | 7) - 15; if (base < 0) base = 0;
			win_load(REC + P.woff_sbid + e_a * P.SLB + base, s_sw); sw_base = base; sw_a = e_a;
		}
		uint32_t r_x = 0u;       // text word, or the row of a reported suffix, or the position of the last row
		if (need_tw) r_x = (qb ? P.bwt[1].text : P.bwt[0].text)[(k - 1u) >> 4];
		else if (tx && kind == TK_HIT) r_x = (qb ? P.bwt[1].isa : P.bwt[0].isa)[k];
		else if (to_text) r_x = (qb ? P.bwt[1].sa_full : P.bwt[0].sa_full)[k];
		uint2 r_km = make_uint2(1u, 0u);
		// sure0: a key-form parent that is the read's own prefix.  Each substituted child will be popped as an exact tail and jump (TK_JUMP) to the level-KT
		// entry of (its key ++ the read's next symbols), a key known here: fetch the three entries beside the children
		// (in the data registers of the rank query, which such a trip leaves free: a2 = the entries of the second and third substitute, a3.x = 4 | the read's symbol)
		uint4 a0, a1, a2, a3, b0, b1, b2, b3;
		a0 = a1 = a2 = a3 = b0 = b1 = b2 = b3 = make_uint4(0, 0, 0, 0);
		// (not where the bound at the children's position is above 0, or not at hand: see the expansion)
		bool gh = kx && e_i > 0 && (s0f & S0_ON) && (e_mm | e_go | e_ge) == 0 && len - e_i < KT && !need_win && (BW_BYTE(e_i - 1 - bw_base) & 127u) == 0u;
		if (kind == TK_JUMP || gh) {
			uint32_t key = e_a ? s_key[threadIdx.x].y : s_key[threadIdx.x].x, key2 = 0, key3 = 0;
			const int d = len - e_i;
			if (gh) {
				if (key == 0xffffffffu) { gh = false; key = 0; }
				else {
					const uint32_t sh = 2u * (uint32_t)(KT - d), low = key & ((1u << sh) - 1u);
					const uint32_t gh_c = key >> sh & 3u;
					a3.x = 4u | gh_c;
					key = (k * 4u + ((gh_c + 1u) & 3u)) << sh | low; key2 = (k * 4u + ((gh_c + 2u) & 3u)) << sh | low; key3 = (k * 4u + ((gh_c + 3u) & 3u)) << sh | low;
				}
			} else if (l == KEYM) {          // the path so far, then the read's own next KT - d symbols
				if (d > 0) { const uint32_t sh = 2u * (uint32_t)(KT - d); key = (k << sh) | (sh ? key & ((1u << sh) - 1u) : 0u); }
			} else if (e_mm) {     // the substituted symbol is the one k was derived with: k lies in (C(c), C(c+1)]
				const uint32_t c1 = qb ? P.bwt[1].L2[1] : P.bwt[0].L2[1], c2 = qb ? P.bwt[1].L2[2] : P.bwt[0].L2[2], c3 = qb ? P.bwt[1].L2[3] : P.bwt[0].L2[3];
				const uint32_t cs = (k > c1 ? 1u : 0u) + (k > c2 ? 1u : 0u) + (k > c3 ? 1u : 0u);
				const uint32_t sh = 2u * (uint32_t)(KT - d);
				key = (key & ~(3u << sh)) | cs << sh;
			}
			const uint2 *const tab = qb ? P.bwt[1].kmer : P.bwt[0].kmer;
			r_km = tab[key];
			if (gh) { const uint2 g2 = tab[key2], g3 = tab[key3]; a2 = make_uint4(g2.x, g2.y, g3.x, g3.y); }
		}
		if (kind == TK_ROWS) r_km = ((qb ? P.bwt[1].kmer_lo : P.bwt[0].kmer_lo) + LVO(mlev))[midx];
		// the rank query: Occ of all four bases at rows k-1 and l of index qb (bwt.c:159-216 conventions)
		uint32_t rk = 0, rl = 0; bool kvalid = false, two = false;
		if (kx) {       // key form: the four children of this level, 32 bytes of the next table level
			const uint4 *const ch = (const uint4*)((qb ? P.bwt[1].kmer_lo : P.bwt[0].kmer_lo) + LVO(len - e_i) + (size_t)k * 4);
			a0 = ch[0]; a1 = ch[1];
		}
		if (query) {
			const uint32_t primary = qb ? P.bwt[1].primary : P.bwt[0].primary;
			const uint4 *bk = qb ? P.bwt[1].bk : P.bwt[0].bk;
			const uint32_t kq = k - 1u, lq = l;
			const uint32_t kp = kq - (kq >= primary ? 1u : 0u), lp = lq - (lq >= primary ? 1u : 0u);
			const uint32_t bl = lp / NABWA_INTV; rl = lp - bl * NABWA_INTV;
			kvalid = kq != 0xffffffffu;
			const uint32_t bkk = kvalid ? kp / NABWA_INTV : bl; rk = kp - bkk * NABWA_INTV;
			two = bkk != bl;
			const uint4 *pl = bk + (size_t)bl * 4;
			a0 = pl[0]; a1 = pl[1]; a2 = pl[2]; a3 = pl[3];
			if (two) { const uint4 *pk = bk + (size_t)bkk * 4; b0 = pk[0]; b1 = pk[1]; b2 = pk[2]; b3 = pk[3]; }
		}

		// look-ahead pop (see s_pf): only from inside a tail, with nothing pending in registers
		bool pf_now = false; uint32_t pf_cand = NIL;
		if (want_ent) { pf_cand = ent_slot; pf_now = true; }                // a pop that was not fetched ahead: fetch now, pop next trip
		else if ((kind == TK_TAIL || kind == TK_JUMP || kind == TK_TEXT_TAIL) && !p_valid && mask_any()) {
			const int bm = mask_first();
			pf_cand = head_get(bm);
			pf_now = pf_cand != pf_slot;
		}
		if (pf_now) r_ent = ent[pf_cand];
		if (!COUNT && P.trip_budget && st != LS_IDLE && st != LS_EXIT) ++rd_trips;
		if (COUNT && st != LS_IDLE && st != LS_EXIT) {
			++rd_trips;
			if (kind == TK_EXPAND) { if (kx) ++rk_kf; else if (tx) ++rk_tx; else if (two) ++rk_row2; else ++rk_row1; if (e_go | e_ge) ++rk_gap; }
			else if (want_ent) ++rk_pop; else if (kind == TK_TAIL || kind == TK_TEXT_TAIL) ++rk_tail; else if (kind == TK_JUMP) ++rk_jump;
		}
		if (COUNT) {   // trip statistics (instrumented build only): TS_TRIPS, then lane-trips by activity
			const unsigned long long bx = __ballot(kind == TK_EXPAND), be = __ballot(kind == TK_TAIL), bm = __ballot(want_ent),
				bs = __ballot(spec), bq = __ballot(query), b2 = __ballot(query && two), bi = __ballot(st == LS_EXIT), bj = __ballot(kind == TK_JUMP), bt = __ballot(tx && kind == TK_EXPAND), b7 = __ballot(kind == TK_TEXT_TAIL);
			if (lane == 0) {
				st_trips += 1; st_expand += __popcll(bx); st_exact += __popcll(be); st_ent += __popcll(bm); st_spec += __popcll(bs);
				st_query += __popcll(bq); st_two += __popcll(b2); st_exit += __popcll(bi); st_jump += __popcll(bj); st_txe += __popcll(bt); st_txt += __popcll(b7);
			}
		}
		asm volatile("" ::: "memory");   // keep every consumer below every load above (no block merging across)
		__builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the window loads above wrote LDS behind the compiler's back
		// ================================================================ phase 3: consume
		if (pf_now) { s_pf[threadIdx.x] = r_ent; pf_slot = pf_cand; }
		if (spec && m < (int)(BW_BYTE(win_hi - bw_base) & 127u)) kind = TK_NONE;   // pruned after all (bwtgap.c:156)
		if (need_tw) { tw.x = r_x; s_tw[threadIdx.x] = tw; }
		int c = 4;
		if (kind == TK_EXPAND || kind == TK_TAIL) c = (int)SQ_BYTE((uint32_t)spos & 15u);
		if (kind == TK_TAIL && c > 3) query = false;
		Occ4 ck, cl;
		ck.c[0] = ck.c[1] = ck.c[2] = ck.c[3] = 0; cl = ck;
		if (query && kind != TK_NONE) {
			cl = nabwa_count4(a0, a1, a2, a3, rl);
			if (kvalid) {       // one counting sequence for row k-1 too: pick its bucket first (16 selects < a third copy of the count)
				const uint4 s0 = two ? b0 : a0, s1 = two ? b1 : a1, s2 = two ? b2 : a2, s3 = two ? b3 : a3;
				ck = nabwa_count4(s0, s1, s2, s3, rk);
			}
			if (COUNT && kind != TK_GROUP) rd_touch += ref_touches(qb ? P.bwt[1] : P.bwt[0], k - 1u, l, kind == TK_EXPAND);   // (the reference derived a group's members in the parent's query)
		}
		if (kx && kind == TK_EXPAND) {
			// key form: child j exists iff its table interval is not empty, and is again a key: present it to the generic
			// expansion below as "counts" (with C(.) = 0) that yield {key * 4 + j, KEYM}
			const uint32_t ek[4] = { a0.x, a0.z, a1.x, a1.z }, el[4] = { a0.y, a0.w, a1.y, a1.w };
#pragma unroll
			for (int j = 0; j < 4; ++j) { const bool ne = ek[j] <= el[j]; ck.c[j] = ne ? k * 4u + (uint32_t)j - 1u : 0u; cl.c[j] = ne ? KEYM : 0u; }
		}
		const bool tx1 = tx && kind == TK_EXPAND;
		if (tx1) {
			// the one row's only non-empty child is for the text base b to the left of the suffix, and it is the suffix
			// starting there: present it to the generic expansion below as "counts" (with C(.) = 0) that yield {k-1, TXM}
			const uint32_t b = k > 0u ? (tw.x >> (((k - 1u) & 15u) << 1) & 3u) : 4u;
#pragma unroll
			for (int j = 0; j < 4; ++j) { ck.c[j] = b == (uint32_t)j ? k - 2u : 0u; cl.c[j] = b == (uint32_t)j ? TXM : 0u; }
		}
		const bool syn = tx1 || (kx && kind == TK_EXPAND);
		const uint32_t L2q0 = syn ? 0u : (qb ? P.bwt[1].L2[0] : P.bwt[0].L2[0]), L2q1 = syn ? 0u : (qb ? P.bwt[1].L2[1] : P.bwt[0].L2[1]);
		const uint32_t L2q2 = syn ? 0u : (qb ? P.bwt[1].L2[2] : P.bwt[0].L2[2]), L2q3 = syn ? 0u : (qb ? P.bwt[1].L2[3] : P.bwt[0].L2[3]);
		const uint32_t seqlen_q = qb ? P.bwt[1].seq_len : P.bwt[0].seq_len;
#define L2Q(cc) ((cc) == 0 ? L2q0 : ((cc) == 1 ? L2q1 : ((cc) == 2 ? L2q2 : L2q3)))
#define CK(cc) ((cc) == 0 ? ck.c[0] : ((cc) == 1 ? ck.c[1] : ((cc) == 2 ? ck.c[2] : ck.c[3])))
#define CL(cc) ((cc) == 0 ? cl.c[0] : ((cc) == 1 ? cl.c[1] : ((cc) == 2 ? cl.c[2] : cl.c[3])))

		if (kind == TK_ROWS) rows_arrived(r_km.x, r_km.y);
		else if (kind == TK_GROUP) {                                   // the popped deletion: one more base of the reference, same read position
			k = L2Q(grp_c) + CK(grp_c) + 1u; l = L2Q(grp_c) + CL(grp_c);
			e_i += 1; e_state = STATE_D; e_ldp = e_i;
			st = LS_HAVE;
		} else if (kind == TK_JUMP) {                                 // landed at depth KT (len > KT, so the tail goes on)
			k = r_km.x; l = r_km.y;
			if (k > l) st = LS_POP;
			else if (forced) { e_i = len - KT; e_ldp = 0; st = LS_HAVE; }   // arrives as the matching child it would have become
			else { e_i = len - KT; st = LS_EXACT; }
		} else if (kind == TK_TEXT_TAIL) {
			// exact tail in text form: read symbols e_i-1, e_i-2, ... against the text to the left, as far as both 16-base words reach
			uint32_t pp = k; bool fail = false;
			for (;;) {
				const uint32_t cc = SQ_BYTE((uint32_t)(e_i - 1) & 15u);
				if (cc > 3u || pp == 0u) { fail = true; break; }
				const uint32_t q = pp - 1u;
				if ((tw.x >> ((q & 15u) << 1) & 3u) != cc) { fail = true; break; }
				pp = q; --e_i;
				if (e_i == 0 || (e_i & 15) == 0 || (pp & 15u) == 0u) break;
			}
			k = pp;
			if (fail) st = LS_POP;
			else if (e_i == 0) st = LS_HAVE;                          // matched to the end: reported (as a row) in the next trip
			else st = LS_EXACT;
		} else if (kind == TK_TAIL || kind == TK_HIT) {
			bool hit = false;
			if (kind == TK_HIT && tx) { k = r_x; l = r_x; }                // the row of the suffix (isa)
			if (kind == TK_HIT) hit = true;
			else if (c > 3) st = LS_POP;                          // an N in the tail: no match
			else {
				k = L2Q(c) + CK(c) + 1u; l = L2Q(c) + CL(c);
				if (k > l) st = LS_POP;
				else if (--e_i == 0) hit = true;
				else st = LS_EXACT;
			}
			if (hit) {
				// ---- hit bookkeeping (bwtgap.c:166-199)
				st = LS_POP;
				const int score = e_mm * P.s_mm + e_go * P.s_gapo + e_ge * P.s_gape;
				bool do_add = true;
				if (n_aln == 0) {
					if ((s0f & S0_ON) && score != 0) { status = NABWA_ST_OVERFLOW; finish = true; do_add = false; s0f &= ~S0_ON; if (P.s0_stats) atomicAdd(P.s0_stats + S0S_NET, 1ull); }   // not the exact hit first: kernel D searches the read from the start
					best_score = score;
					const int best_diff = e_mm + e_go + (gape_mode ? e_ge : 0);
					if (!nonstop) max_diff = best_diff + 1 > MD_READ ? MD_READ : best_diff + 1;
				}
				if (score == best_score) best_cnt += (int)(l - k + 1u);
				else if (best_cnt > P.max_top2) { finish = true; do_add = false; }
				uint4 *const out = P.aln + (size_t)item * P.aln_cap;
				if (do_add && e_go) {
					for (int j = 0; j < n_aln; ++j) { const uint4 h = out[j]; if (h.y == k && h.z == l) { do_add = false; break; } }
				}
				if (do_add) {
					if (n_aln == P.aln_cap) { status = NABWA_ST_OVERFLOW; finish = true; }
					else {
						// gap_shadow (bwtgap.c:81-91) on this strand's bounds, positions < last_diff_pos;
						// 8 positions per trip; the weq flags of positions 1..last_diff_pos are refreshed
						const uint32_t x = l - k + 1u, mx = seqlen_q; uint32_t jj = 0, pw = 0;
						uint8_t *const rec = REC;
						uint32_t *const wp = (uint32_t*)rec + e_a * P.WL; uint8_t *const bp = rec + P.woff_bid + e_a * P.WLB;
						for (int t0 = 0; t0 <= e_ldp && e_ldp > 0; t0 += 8) {
							const uint4 w0 = *(const uint4*)(wp + t0), w1 = *(const uint4*)(wp + t0 + 4);
							const uint2 bq = *(const uint2*)(bp + t0);
							uint32_t wv[8] = { w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w };
							uint32_t bb[2] = { bq.x, bq.y };
#pragma unroll
							for (int u = 0; u < 8; ++u) {
								const int t = t0 + u;
								uint32_t bv = bb[u >> 2] >> ((u & 3) * 8) & 0xffu;
								if (t < e_ldp) {
									if (wv[u] > x) wv[u] -= x;
									else if (wv[u] == x) { bv = (bv & 128u) | 1u; wv[u] = mx - (++jj); }
								}
								if (t <= e_ldp) {
									bv = (bv & 127u) | ((t > 0 && wv[u] == pw) ? 128u : 0u);
									bb[u >> 2] = (bb[u >> 2] & ~(0xffu << ((u & 3) * 8))) | bv << ((u & 3) * 8);
								}
								pw = wv[u];
							}
							*(uint4*)(wp + t0) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
							*(uint4*)(wp + t0 + 4) = make_uint4(wv[4], wv[5], wv[6], wv[7]);
							*(uint2*)(bp + t0) = make_uint2(bb[0], bb[1]);
						}
						bw_a = -1;   // the bound window may be stale now
						if (KT && e_ldp > len - KT - 1) s_fb[threadIdx.x] |= 0xffu << (e_a << 3);   // ... and so may the cached bound
						out[n_aln] = make_uint4((uint32_t)e_mm | (uint32_t)e_go << 8 | (uint32_t)e_ge << 16 | (uint32_t)e_a << 24,
												k, l, (uint32_t)score);
						++n_aln;
					}
				}
			}
		} else if (kind == TK_EXPAND) {
			// ---- node expansion (bwtgap.c:201-260); e_i is already decremented
			const uint32_t occ = tx1 ? 1u : l - k + 1u;                   // (key form: only read by deletion-state parents, which are never in key form)
			bool match_child = false;
			bool allow_diff = true, allow_M = true, mm_dead = false;
			if (e_i > 0) {
				const uint32_t B1 = BW_BYTE(e_i - 1 - bw_base), B0 = BW_BYTE(e_i - bw_base);
				const int b1 = (int)(B1 & 127u), b0v = (int)(B0 & 127u);
				// sure0: a 1-mismatch child is popped with m == 0, and a bound never falls back to 0 (gap_shadow sets 1): with a bound above 0 at
				// its position it fails bwtgap.c:156 whenever it is popped -- counted, never stored (the strand that does not occur: every level)
				mm_dead = (s0f & S0_ON) && b1 > 0;
				if (b1 > m - 1) allow_diff = false;
				else if (b1 == m - 1 && b0v == m - 1 && (B0 & 128u)) allow_M = false;
				if (use_seed) {
					const uint32_t S1 = SW_BYTE(ii - 1 - sw_base), S0 = SW_BYTE(ii - sw_base);
					const int s1 = (int)(S1 & 127u), s0 = (int)(S0 & 127u);
					const int m_seed = m - max_diff + P.max_seed_diff;      // max_seed_diff - (the same differences), bwtgap.c:153
					if (s1 > m_seed - 1) allow_diff = false;
					else if (s1 == m_seed - 1 && s0 == m_seed - 1 && (S0 & 128u)) allow_M = false;
				}
			}
			// children go through a one-entry delay: the last one stays in registers as `pending`
			auto emit = [&](int score, uint32_t nk, uint32_t nl, int ni, int nldp, int nmm, int ngo, int nge, int nstate, int count) {
				if (p_valid) push_mem(p_score, pe);
				pe = mk_entry(nk, nl, ni, nldp, nmm & 0xff, ngo & 0xff, nge & 0xff, nstate, e_a); p_score = score;
				n_entries += count;
			};
			const int sc0 = e_mm * P.s_mm + e_go * P.s_gapo + e_ge * P.s_gape;
			int tmp = e_go + e_ge;
			if (loggap) { const uint32_t v = (uint32_t)(e_ge + e_go); tmp = (v ? 31 - __clz((int)v) : 0) / 2 + 1; }
			// Text-form fast path.  While the next read symbols equal the text in front of the suffix, a level of the search
			// tree is fully determined without memory: the only non-empty child is the matching one, which is the next pop
			// (same score, newest), and the gap children -- if the bounds allow differences there -- are one insertion and
			// one deletion.  So several levels are walked in this trip, as far as the 16-byte windows reach, and their gap
			// groups leave as ONE stack entry (`more` older levels behind the newest, see the pop side).
			bool ran = false;
			if (tx1 && e_state == STATE_M && n_entries + 64 <= P.max_entries) {
				const int ies = P.indel_end_skip + tmp, seed_lo = len - P.seed_len;
				const int m_seed = m - max_diff + P.max_seed_diff;
				int n = 0, icur = e_i, ilast = e_i; uint32_t pcur = k; bool grp_run = false;
				for (;;) {
					const uint32_t cc = SQ_BYTE((uint32_t)icur & 15u);
					if (cc > 3u || pcur == 0u) break;
					const uint32_t q = pcur - 1u;
					if ((tw.x >> ((q & 15u) << 1) & 3u) != cc) break;
					bool ad = true;
					const bool us = seeded && icur > 0 && icur - seed_lo > 0;
					if (icur > 0) {
						if ((int)(BW_BYTE(icur - 1 - bw_base) & 127u) > m - 1) ad = false;
						if (us && (int)(SW_BYTE(icur - seed_lo - 1 - sw_base) & 127u) > m_seed - 1) ad = false;
					}
					const bool g = ad && icur >= ies && len - icur >= ies && e_go < MG_READ;
					if (n == 0) grp_run = g; else if (g != grp_run) break;
					++n; pcur = q; ilast = icur;
					// may the child (position icur, suffix q) be popped and expanded in this same trip?
					if (n == NABWA_RUN_MAX || icur == 0) break;
					if (m < (int)(BW_BYTE(icur - 1 - bw_base) & 127u)) break;       // its pop prunes it (bwtgap.c:156)
					if ((icur & 15) == 0 || (q & 15u) == 0u) break;                  // read / text window ends
					if (icur - 1 > 0 && icur - 2 < bw_base) break;                   // bound window ends
					if (seeded && icur - 1 > 0 && icur - 1 - seed_lo > 0 && icur - 1 - seed_lo - 1 < sw_base) break;
					--icur;
				}
				if (n) {
					ran = true;
					if (grp_run) emit(sc0 + P.s_gapo, k - (uint32_t)(n - 1), TXM, ilast, (int)(3u | (uint32_t)(n - 1) << 9), e_mm, e_go, e_ge, STATE_GROUP, 2 * n);
					emit(sc0, pcur, TXM, ilast, 0, e_mm, e_go, e_ge, STATE_M, 1);
				}
			}
			if (ran) { /* children done */ }
			else if (allow_diff && e_i >= P.indel_end_skip + tmp && len - e_i >= P.indel_end_skip + tmp) {
				// The gap children of one expansion (an insertion and/or up to four deletions, bwtgap.c:216-240) share one
				// score and are pushed back to back, i.e. they are ADJACENT in that score's stack.  They travel as one
				// STATE_GROUP entry: the parent's interval and position plus a member mask (bit 0 the insertion, bit 1+j the
				// deletion of base j, GRP_EXT: gap extension of a deletion rather than gap open, bits 9..15: `more` older levels of a
				// text-form run, each {insertion, deletion}); a member is materialised --
				// the deletions by repeating the parent's rank query -- only if it is ever popped (see the pop side).  Most
				// never are: once a hit exists, scores above best_score + s_mm end the search (bwtgap.c:144).
				uint32_t dm = 0;
#pragma unroll
				for (int j = 0; j < 4; ++j) { const uint32_t nk = L2Q(j) + CK(j) + 1u, nl = L2Q(j) + CL(j); if (nk <= nl) dm |= 2u << j; }
				if (e_state == STATE_M) {
					if (e_go < MG_READ) emit(sc0 + P.s_gapo, k, l, e_i, (int)(dm | 1u), e_mm, e_go, e_ge, STATE_GROUP, __popc(dm) + 1);
				} else if (e_state == STATE_I) {
					if (e_ge < P.max_gape) emit(sc0 + P.s_gape, k, l, e_i, e_i, e_mm, e_go, e_ge + 1, STATE_I, 1);
				} else if (e_ge < P.max_gape) {
					if ((e_ge + e_go < max_diff || occ < (uint32_t)P.max_del_occ) && dm)
						emit(sc0 + P.s_gape, k, l, e_i, (int)(dm | GRP_EXT), e_mm, e_go, e_ge, STATE_GROUP, __popc(dm));
				}
			}
			if (ran) { /* children done */ }
			else if (allow_diff && allow_M) {
#pragma unroll
				for (int j = 1; j <= 4; ++j) {
					const int cc = (c + j) & 3; const bool is_mm = (j != 4 || c > 3);
					const uint32_t nk = L2Q(cc) + CK(cc) + 1u, nl = L2Q(cc) + CL(cc);
					if (nk <= nl) {
						// sure0: the substituted child of a parent that is the read's own prefix, with the level-KT entry its tail jump will find (see the loads)
						uint32_t ek = nk, el = nl; int ei = e_i; bool dead = is_mm && mm_dead;
						if (kx && is_mm && !dead && a3.x == (4u | (uint32_t)c)) {
							const uint32_t gk = j == 1 ? r_km.x : (j == 2 ? a2.x : a2.z), gl = j == 1 ? r_km.y : (j == 2 ? a2.y : a2.w);
							if (gk > gl) { dead = true; s0f += 1u << 16; }    // the jump would find nothing
							else if (s0f & S0_LAND) {                          // stored as the jump would leave it; ldp > i marks it (its pop-time bound is the one at ldp - 1)
								ek = gk; el = gl; ei = len - KT; s0f += 1u << 23;
							}
						}
						if (dead) ++n_entries;                                // counted like a never-stored entry, never popped
						else emit(sc0 + (is_mm ? P.s_mm : 0), ek, el, ei, is_mm ? e_i : 0, e_mm + (is_mm ? 1 : 0), e_go, e_ge, STATE_M, 1);
						if (!is_mm) match_child = true;
					}
				}
			} else if (c < 4) {
				const uint32_t nk = L2Q(c) + CK(c) + 1u, nl = L2Q(c) + CL(c);
				if (nk <= nl) { emit(sc0, nk, nl, e_i, 0, e_mm, e_go, e_ge, STATE_M, 1); match_child = true; }
			}
			// the matching child of a one-row interval (always the last emit, still in the pending registers) goes on in text form
			if (to_text && match_child) { pe.x = r_x - 1u; pe.y = TXM; }
			if (ovf) { status = NABWA_ST_OVERFLOW; finish = true; }
		}
#undef L2Q
#undef CK
#undef CL

		if (finish) {
			const bool net = (s0f & S0_ON) && status == NABWA_ST_OK && n_aln == 0;       // the exact occurrence was not found: kernel D searches the read from the start
			if (net) status = NABWA_ST_OVERFLOW;
			if (P.s0_stats && (s0f & S0_WAS)) atomicAdd(P.s0_stats + S0S_READS, 1ull);
			if (P.s0_stats && (s0f >> 16 & 0x3fffu)) {
				atomicAdd(P.s0_stats + S0S_KF_EMPTY, (unsigned long long)(s0f >> 16 & 0x7fu)); atomicAdd(P.s0_stats + S0S_KF_LANDED, (unsigned long long)(s0f >> 23 & 0x7fu));
			}
			if (P.s0_stats && net) atomicAdd(P.s0_stats + S0S_NET, 1ull);
			P.n_aln[item] = n_aln; P.max_ent[item] = (!COUNT && status == NABWA_ST_OVERFLOW) ? (int)rd_trips : max_ent; P.status[item] = (uint8_t)status;      // (a search handed on: the trips it took here -- kernel D's statistics dump reads them; its own max_ent replaces this)
			if (COUNT && status == NABWA_ST_OK) touches += rd_touch;   // abandoned reads are counted by the wide pass
			if (COUNT && P.touch_counter && rd_trips > 8000u) {
				atomicAdd(P.touch_counter + TS_LONG_READS, 1ull); atomicAdd(P.touch_counter + TS_LONG_TRIPS, (unsigned long long)rd_trips); atomicAdd(P.touch_counter + TS_LONG_KF, (unsigned long long)rk_kf);
				atomicAdd(P.touch_counter + TS_LONG_ROW2, (unsigned long long)rk_row2); atomicAdd(P.touch_counter + TS_LONG_ROW1, (unsigned long long)rk_row1); atomicAdd(P.touch_counter + TS_LONG_TEXT, (unsigned long long)rk_tx);
				atomicAdd(P.touch_counter + TS_LONG_POP, (unsigned long long)rk_pop); atomicAdd(P.touch_counter + TS_LONG_TAIL, (unsigned long long)rk_tail); atomicAdd(P.touch_counter + TS_LONG_JUMP, (unsigned long long)rk_jump); atomicAdd(P.touch_counter + TS_LONG_GAP, (unsigned long long)rk_gap);
			}
			if (COUNT && P.touch_counter) { atomicMax(P.touch_counter + TS_MAX_TRIPS, (unsigned long long)rd_trips); if (rd_trips > 2000u) atomicAdd(P.touch_counter + TS_OVER_2000, 1ull); if (rd_trips > 500u) atomicAdd(P.touch_counter + TS_OVER_500, 1ull); }
			st = LS_IDLE;
		}
	}
	if (COUNT) {
		for (int o = 32; o > 0; o >>= 1) touches += __shfl_down(touches, o);
		if (lane == 0 && P.touch_counter) {
			atomicAdd(P.touch_counter + TS_TOUCH_S, touches);
			atomicAdd(P.touch_counter + TS_TRIPS, st_trips); atomicAdd(P.touch_counter + TS_EXPAND, st_expand); atomicAdd(P.touch_counter + TS_EXACT, st_exact);
			atomicAdd(P.touch_counter + TS_ENT_LOAD, st_ent); atomicAdd(P.touch_counter + TS_SPEC, st_spec); atomicAdd(P.touch_counter + TS_QUERY, st_query);
			atomicAdd(P.touch_counter + TS_TWO, st_two); atomicAdd(P.touch_counter + TS_EXITED, st_exit); atomicAdd(P.touch_counter + TS_JUMP, st_jump); atomicAdd(P.touch_counter + TS_TEXT_EXPAND, st_txe); atomicAdd(P.touch_counter + TS_TEXT_TAIL, st_txt);
		}
	}
}

#undef p_valid
#undef S0_ON
#undef S0_LAND
#undef S0_WAS
#undef S0_PRV
#undef s0f
#undef BW_BYTE
#undef SW_BYTE
#undef SQ_BYTE
#undef RID
#undef REC
#undef MD_READ
#undef MG_READ
// kernel W's instantiation for the forms text_mode asks for (W_FORMS), as f(kernel).  Twelve in all: four forms, plain, touch-counting and
// statistics.  The single-knob forms stay in the two diagnostic builds as well: the statistics test runs every knob setting
// (tests/test_gpu_width_spans.py), and the touch-counting run with NABWA_TRIP_STATS=jump keeps the batch's text_mode, whatever its knobs.
template <bool COUNT, bool STATS = false, typename F> static auto with_width_kernel(int text_mode, F f)
{
	switch (W_FORMS(text_mode)) {
	case 1: return f(fm_width_kernel<COUNT, 1, STATS>);
	case 2: return f(fm_width_kernel<COUNT, 2, STATS>);
	case 3: return f(fm_width_kernel<COUNT, 3, STATS>);
	default: return f(fm_width_kernel<COUNT, 0, STATS>);
	}
}

extern "C" void nabwa_launch_fm_width(const SearchParams *P, int n_blocks, hipStream_t s)
{
	auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3(n_blocks), dim3(NABWA_SEARCH_BLOCK), 0, s, *P); return 0; };
	if ((P->text_mode & TM_W_STATS) && P->touch_counter) with_width_kernel<false, true>(P->text_mode, go);      /* the trip statistics: NOT the counting build, which runs without tables */
	else if (P->touch_counter) with_width_kernel<true>(P->text_mode, go);
	else with_width_kernel<false>(P->text_mode, go);
}

extern "C" int nabwa_width_occupancy(int text_mode)
{
	return with_width_kernel<false>(text_mode, [](auto k) {
		int nb = 0;
		return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, NABWA_SEARCH_BLOCK, 0) == hipSuccess ? nb : 0;
	});
}

extern "C" void nabwa_launch_fm_search(const SearchParams *P, int n_blocks, hipStream_t s)
{
	const size_t lds = (size_t)P->NS * NABWA_SEARCH_BLOCK * 2 + NABWA_SEARCH_BLOCK * 84;
	if (P->touch_counter) hipLaunchKernelGGL((fm_search_kernel<true>), dim3(n_blocks), dim3(NABWA_SEARCH_BLOCK), lds, s, *P);
	else hipLaunchKernelGGL((fm_search_kernel<false>), dim3(n_blocks), dim3(NABWA_SEARCH_BLOCK), lds, s, *P);
}

extern "C" int nabwa_search_occupancy(int ns)
{
	int nb = 0;
	hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fm_search_kernel<false>, NABWA_SEARCH_BLOCK,
																(size_t)ns * NABWA_SEARCH_BLOCK * 2 + NABWA_SEARCH_BLOCK * 84);
	return e == hipSuccess ? nb : 0;
}
