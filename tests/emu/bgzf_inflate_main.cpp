// bgzf_inflate_main.cpp -- the BGZF decompressor's kernel body on the CPU as a program of its own: the file named on the command line
// holds BGZF members back to back; their inflated bytes go to standard output (exit 0), or the first bad member ends the run with
// "member K: status S" on standard error and exit 3 (a header that is not BGZF or runs past the file: exit 4).  Built with
// -fsanitize=address,undefined by tests/test_bgzf_inflate_asan.py: the sanitizer run of the kernel's indexing.
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <vector>

extern "C" int emu_bgzf_inflate(const uint8_t *payload, uint32_t n_src, uint8_t *out, uint32_t isize, uint32_t crc);

int main(int argc, char **argv)
{
	if (argc < 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	std::vector<uint8_t> in;
	uint8_t buf[65536];
	for (size_t r; (r = fread(buf, 1, sizeof buf, f)) > 0; ) in.insert(in.end(), buf, buf + r);
	fclose(f);
	std::vector<uint8_t> out;
	size_t o = 0;
	for (int k = 0; o < in.size(); ++k) {
		const uint8_t *h = in.data() + o;
		const size_t left = in.size() - o;
		size_t total = 0, xlen = 0;
		if (left >= 12 && h[0] == 31 && h[1] == 139 && h[2] == 8 && (h[3] & 4)) {
			xlen = h[10] | (size_t)h[11] << 8;
			if (left >= 12 + xlen)
				for (size_t q = 12; q + 4 <= 12 + xlen; ) {
					const size_t sl = h[q + 2] | (size_t)h[q + 3] << 8;
					if (h[q] == 'B' && h[q + 1] == 'C' && sl == 2 && q + 6 <= 12 + xlen) { total = (size_t)(h[q + 4] | (size_t)h[q + 5] << 8) + 1; break; }
					q += 4 + sl;
				}
		}
		if (total < 12 + xlen + 8 || total > left) { fprintf(stderr, "member %d: no BGZF header, or one that runs past the file\n", k); return 4; }
		uint32_t crc, isize;
		memcpy(&crc, h + total - 8, 4); memcpy(&isize, h + total - 4, 4);
		if (isize > 0x10000) { fprintf(stderr, "member %d: ISIZE above 64 KB\n", k); return 4; }
		const size_t at = out.size();
		out.resize(at + isize);
		uint8_t none;
		const int st = emu_bgzf_inflate(h + 12 + xlen, (uint32_t)(total - 12 - xlen - 8), isize ? out.data() + at : &none, isize, crc);
		if (st != 0) { fprintf(stderr, "member %d: status %d\n", k, st); return 3; }
		o += total;
	}
	if (!out.empty() && fwrite(out.data(), 1, out.size(), stdout) != out.size()) return 5;
	return 0;
}
