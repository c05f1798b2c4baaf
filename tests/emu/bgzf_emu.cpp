// bgzf_emu.cpp -- the BGZF compressor's per-slice body (csrc/bgzf_deflate_body.hpp) on the CPU: the phases the kernel runs between its
// barriers, each as a loop over the 64 lanes.  Test infrastructure only (tests/test_bgzf_emu.py); built with g++, and once more
// under AddressSanitizer, where an index past the LDS image, the slice or the block's slot is an error instead of a lost machine.
#define BGZF_EMU
#include "bgzf_deflate_body.hpp"
#include <string.h>
#include <vector>

/* order: the lanes of the parse phase run 0 first-to-last, 1 last-to-first, 2 interleaved -- on the GPU they run at once, and the
 * shared hash table sees their entries in any order */
extern "C" long emu_bgzf(const uint8_t *in, long n, uint8_t *out, int order)
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
		for (uint32_t i = 0; i < BGZF_LANES; ++i)
			bgzf_phase_parse(*Sh, order == 0 ? i : order == 1 ? BGZF_LANES - 1 - i : (i * 37u) % BGZF_LANES, m);
		for (uint32_t t = 0; t < BGZF_LANES; ++t) bgzf_phase_scan(*Sh, t, m);
		const uint32_t need = 18 + Sh->payload + 8;
		std::vector<uint32_t> slot((need + 3) / 4, 0xdeadbeefu);     /* exactly the words of the block, holding an earlier call's bytes */
		for (uint32_t t = 0; t < BGZF_LANES; ++t) bgzf_phase_zero(*Sh, t, slot.data());
		for (uint32_t t = 0; t < BGZF_LANES; ++t) bgzf_phase_emit(*Sh, t, m, slot.data(), &size);
		if (size != need) { delete Sh; return -1; }
		memcpy(out + done, slot.data(), size);
		done += size;
	}
	delete Sh;
	return done;
}
