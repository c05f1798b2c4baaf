// bgzf_inflate_emu.cpp -- the BGZF decompressor's per-member body (csrc/bgzf_inflate_body.hpp) on the CPU: the phases the kernel runs
// between its barriers, each as a loop over the 64 lanes.  Test infrastructure only: a shared object for tests/test_bgzf_inflate_emu.py,
// and part of the stand-alone program tests/emu/bgzf_inflate_main.cpp, which is built under AddressSanitizer, where an index past the
// payload, the output or a table is an error instead of a lost machine.
#define BGZF_EMU
#include "bgzf_inflate_body.hpp"
#include <string.h>
#include <vector>

/* one member: payload[0, n_src) -> out[0, isize); returns the status word.  Payload and output live in buffers of exactly their
 * sizes, so a read or write one byte outside either is seen by the sanitizer. */
extern "C" int emu_bgzf_inflate(const uint8_t *payload, uint32_t n_src, uint8_t *out, uint32_t isize, uint32_t crc)
{
	std::vector<uint8_t> pay(payload, payload + n_src), dst(isize, 0xa5);
	BgziShared *Sh = new BgziShared;
	memset(Sh, 0xa5, sizeof *Sh);                                    /* LDS holds anything when a workgroup starts */
	uint32_t status = 0xffffffffu;
	bgzf_inflate_member(*Sh, 0, pay.data(), n_src, dst.data(), isize, crc, &status);
	delete Sh;
	if (isize) memcpy(out, dst.data(), isize);
	return (int)status;
}
