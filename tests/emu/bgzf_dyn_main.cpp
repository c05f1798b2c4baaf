// bgzf_dyn_main.cpp -- bgzf_dyn_emu.cpp as a program of its own, so that it runs under AddressSanitizer and UBSan without a sanitized
// library in another process.  Test infrastructure only (tests/test_bgzf_dyn_emu.py).
//   bgzf_dyn_main DIR N_CASES N_HISTS
// DIR/case<i>.in -> DIR/case<i>.<order>.out, the dynamic mode's blocks in the three lane orders;
// DIR/hist<i>.in (uint32 limit, uint32 n, n uint32 frequencies) -> DIR/hist<i>.out (n code lengths)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

extern "C" long emu_bgzf_dyn(const uint8_t *in, long n, uint8_t *out, int order);
extern "C" int emu_bgzf_code_lengths(const uint32_t *freq, int n, int limit, uint8_t *len);

static bool slurp(const std::string &path, std::vector<uint8_t> &b)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return false;
	fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
	b.resize((size_t)n);
	const bool ok = n == 0 || fread(b.data(), 1, (size_t)n, f) == (size_t)n;
	fclose(f);
	return ok;
}
static bool spill(const std::string &path, const uint8_t *p, size_t n)
{
	FILE *f = fopen(path.c_str(), "wb");
	if (!f) return false;
	const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
	return fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
	if (argc != 4) { fprintf(stderr, "usage: bgzf_dyn_main DIR N_CASES N_HISTS\n"); return 1; }
	const std::string dir = argv[1];
	const int n_cases = atoi(argv[2]), n_hists = atoi(argv[3]);
	for (int i = 0; i < n_cases; ++i) {
		std::vector<uint8_t> in;
		if (!slurp(dir + "/case" + std::to_string(i) + ".in", in)) { fprintf(stderr, "case %d: cannot read\n", i); return 1; }
		const size_t slices = (in.size() + 0xfeff) / 0xff00;
		for (int order = 0; order < 3; ++order) {
			std::vector<uint8_t> out(slices * 0x10000 + 1);
			const long n = emu_bgzf_dyn(in.data(), (long)in.size(), out.data(), order);
			if (n < 0) { fprintf(stderr, "case %d order %d: a block's size is not what its header phase said\n", i, order); return 1; }
			if (!spill(dir + "/case" + std::to_string(i) + "." + std::to_string(order) + ".out", out.data(), (size_t)n)) return 1;
		}
	}
	for (int i = 0; i < n_hists; ++i) {
		std::vector<uint8_t> in;
		if (!slurp(dir + "/hist" + std::to_string(i) + ".in", in) || in.size() < 8) { fprintf(stderr, "hist %d: cannot read\n", i); return 1; }
		const uint32_t *w = (const uint32_t*)in.data();
		const uint32_t limit = w[0], n = w[1];
		if (in.size() != 8 + 4 * (size_t)n) { fprintf(stderr, "hist %d: size\n", i); return 1; }
		std::vector<uint8_t> len(n);
		if (emu_bgzf_code_lengths(w + 2, (int)n, (int)limit, len.data()) != 0) { fprintf(stderr, "hist %d: refused\n", i); return 1; }
		if (!spill(dir + "/hist" + std::to_string(i) + ".out", len.data(), n)) return 1;
	}
	printf("bgzf_dyn_main ok\n");
	return 0;
}
