// bgzf_in_inflater_main.cpp -- test harness for the optional inflater of csrc/bgzf_in.hpp's BamIn: as bgzf_in_main.cpp, but the BGZF
// blocks of a fill are inflated by a callable set from outside -- here a zlib-backed stand-in for the library's GPU decompressor, which
// also checks what the callable is promised (whole members cmp[from, to), one stretch of output).  A second argument "refuse" makes
// the stand-in return false for the first fill it sees: the run ends through die() with status 3.
#define TOOL "bgzf_in_inflater_main"
#define TOOL_DIE_STATUS 3
#include "../../network-aware-bwa_amd/csrc/bgzf_in.hpp"

int main(int argc, char **argv)
{
	if (argc < 2) return 2;
	const bool refuse = argc > 2 && !strcmp(argv[2], "refuse");
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	BamIn in(f, argv[1]);
	size_t calls = 0;
	in.inflater = [&](const uint8_t *cmp, size_t from, size_t to, const std::vector<BamIn::Blk> &blk, uint8_t *plain, std::string &why) {
		++calls;
		if (refuse) { why = "the stand-in refuses block 0"; return false; }
		if (blk.empty() || blk.front().src < from || blk.back().src + blk.back().n_src + 8 != to) { why = "the blocks are not the members cmp[from, to)"; return false; }
		size_t at = blk.front().dst;
		for (const BamIn::Blk &b : blk) {
			if (b.dst != at) { why = "the output is not one stretch"; return false; }
			std::vector<uint8_t> out(b.isize + 1);
			uLongf n = (uLongf)out.size();
			z_stream z; memset(&z, 0, sizeof(z));
			if (inflateInit2(&z, -15) != Z_OK) { why = "inflateInit"; return false; }
			z.next_in = (Bytef*)(cmp + b.src); z.avail_in = (uInt)b.n_src; z.next_out = out.data(); z.avail_out = (uInt)n;
			const int r = inflate(&z, Z_FINISH);
			const size_t got = n - z.avail_out;
			inflateEnd(&z);
			if (r != Z_STREAM_END || got != b.isize || (uint32_t)crc32(crc32(0, 0, 0), out.data(), (uInt)got) != b.crc) { why = "a block does not inflate"; return false; }
			if (got) memcpy(plain + b.dst, out.data(), got);
			at += b.isize;
		}
		return true;
	};
	std::vector<uint8_t> buf;
	size_t step = 1;
	for (;;) {
		const size_t want = 4 + step % 70001;
		const size_t have = in.need(want);
		if (have == 0) break;
		const size_t n = have < want ? have : want;
		buf.resize(n);
		if (!in.read(buf.data(), n)) return 4;
		if (fwrite(buf.data(), 1, n, stdout) != n) return 5;
		step = step * 31 + 7;
	}
	fprintf(stderr, "%s %zu\n", in.bgzf ? "bgzf" : in.raw ? "raw" : "stream", calls);
	return 0;
}
