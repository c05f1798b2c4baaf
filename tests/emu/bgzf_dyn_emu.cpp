// bgzf_dyn_emu.cpp -- the BGZF compressor's dynamic mode (csrc/bgzf_deflate_body.hpp, the phases of bgzf_deflate_dyn_kernel) on the CPU:
// the phases the kernel runs between its barriers, each as a loop over the 64 lanes, and the code builder on its own.  Test
// infrastructure only (tests/test_bgzf_dyn_emu.py); built with g++ as a library, and with bgzf_dyn_main.cpp as a stand-alone program
// under AddressSanitizer and UBSan, where an index past the LDS image, the slice or the block's slot is an error.
#define BGZF_EMU
#include "bgzf_deflate_body.hpp"
#include <string.h>
#include <vector>

static uint32_t lane_of(uint32_t i, int order) { return order == 0 ? i : order == 1 ? BGZF_LANES - 1 - i : (i * 37u) % BGZF_LANES; }

/* order: the lanes of every phase run 0 first-to-last, 1 last-to-first, 2 interleaved (the parse's shared hash table sees their
 * entries in that order, as in bgzf_emu.cpp; the later phases give the same bytes in any order, which the three runs show) */
extern "C" long emu_bgzf_dyn(const uint8_t *in, long n, uint8_t *out, int order)
{
	long done = 0;
	BgzfShared *Sh = new BgzfShared;
	for (long at = 0; at < n; at += BGZF_SLICE) {
		const uint32_t m = n - at < (long)BGZF_SLICE ? (uint32_t)(n - at) : BGZF_SLICE;
		std::vector<uint32_t> src((m + 3) / 4);                      /* exactly the words the load phase may read */
		memcpy(src.data(), in + at, m);
		memset(Sh, 0xa5, sizeof *Sh);                                /* LDS holds anything when a workgroup starts */
		uint32_t size = 0;
		for (uint32_t t = 0; t < BGZF_LANES; ++t) bgzf_phase_load(*Sh, t, src.data(), m);
		for (uint32_t i = 0; i < BGZF_LANES; ++i) bgzf_phase_parse(*Sh, lane_of(i, order), m);
		for (uint32_t i = 0; i < BGZF_LANES; ++i) { bgzf_phase_scan(*Sh, lane_of(i, order), m); bgzf_dyn_phase_clear(*Sh, lane_of(i, order)); }
		for (uint32_t i = 0; i < BGZF_LANES; ++i) bgzf_dyn_phase_count(*Sh, lane_of(i, order), m);
		for (uint32_t i = 0; i < BGZF_LANES; ++i) bgzf_dyn_phase_sort(*Sh, lane_of(i, order));
		for (uint32_t i = 0; i < BGZF_LANES; ++i) bgzf_dyn_phase_header(*Sh, lane_of(i, order));
		const uint32_t need = 18 + Sh->payload + 8;
		std::vector<uint32_t> slot((need + 3) / 4, 0xdeadbeefu);     /* exactly the words of the block, holding an earlier call's bytes */
		for (uint32_t i = 0; i < BGZF_LANES; ++i) bgzf_dyn_phase_measure(*Sh, lane_of(i, order), m, slot.data());
		for (uint32_t i = 0; i < BGZF_LANES; ++i) bgzf_dyn_phase_offsets(*Sh, lane_of(i, order));
		for (uint32_t i = 0; i < BGZF_LANES; ++i) bgzf_dyn_phase_emit(*Sh, lane_of(i, order), m, slot.data(), &size);
		if (size != need) { delete Sh; return -1; }
		memcpy(out + done, slot.data(), size);
		done += size;
	}
	delete Sh;
	return done;
}

/* the code builder alone: n <= 286 frequencies, 2^limit >= n, limit <= 15 -> len[0, n); 0, or -1 for arguments it does not take */
extern "C" int emu_bgzf_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *len)
{
	if (n < 2 || n > (int)BGZF_NLL || limit < 1 || limit > 15 || (1 << limit) < n) return -1;
	BgzfDyn *D = new BgzfDyn;
	memset(D, 0xa5, sizeof *D);
	std::vector<uint32_t> f(freq, freq + n);                         /* exactly n of each */
	std::vector<uint16_t> ord(n, 0xffff);
	std::vector<uint8_t> l(n, 0);
	for (uint32_t t = 0; t < BGZF_LANES; ++t) bgzf_rank_sort(f.data(), (uint32_t)n, ord.data(), t, BGZF_LANES);
	bgzf_build_lengths(*D, f.data(), (uint32_t)n, (uint32_t)limit, ord.data(), l.data());
	memcpy(len, l.data(), n);
	delete D;
	return 0;
}
