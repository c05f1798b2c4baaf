// tests/emu/finish_emu.cpp -- TEST INFRASTRUCTURE ONLY: the bodies of the finishing kernels (network-aware-bwa_amd/csrc/finish_body.hpp)
// compiled by g++ as a sequential emulation of one wavefront (NABWA_EMU, wave_spmd.hpp): the window, CIGAR and MD bodies as loops over
// the lanes.  A shared object for tests/test_finish_emu.py; with FINISH_EMU_MAIN a stand-alone program that runs a fixed set of cases,
// to be built with -fsanitize=address,undefined.  Every buffer a body reads or writes has exactly the size the kernel may touch -- the
// .pac ends at (l_pac + 3) / 4, the window at win_n, the MD string at its counted length + 1 --, so a byte outside is an error there.
#define NABWA_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../network-aware-bwa_amd/csrc/finish_body.hpp"

namespace {
struct EmuRef {
	std::vector<uint8_t> pac; std::vector<FinHole> holes; FinRef R;
	EmuRef(const uint8_t *pac_, int64_t l_pac, int n_holes, const int64_t *hole_off, const int32_t *hole_len, const char *hole_amb)
		: pac(pac_, pac_ + (l_pac + 3) / 4)
	{
		for (int i = 0; i < n_holes; ++i) holes.push_back(FinHole{ hole_off[i], hole_len[i], (int32_t)(uint8_t)hole_amb[i] });
		R.pac = pac.data(); R.l_pac = l_pac; R.holes = holes.data(); R.n_holes = n_holes; R.pad = 0;
	}
};
}

/* the extent of a job's window (bwase.c:197-209), as refine_batch computes it on the host: arithmetic only */
extern "C" void emu_fin_extent(int64_t l_pac, uint32_t pos, int len, int ext, int end_correct, int64_t *pos_signed, int64_t *win_lo, int *win_n)
{
	const int ref_len = len + abs(ext);
	const int64_t p = (int64_t)pos > l_pac ? (int64_t)(int32_t)pos : (int64_t)pos;
	int64_t lo, hi;
	if (ext > 0) { lo = p > 0 ? p : 0; hi = p + ref_len < l_pac ? p + ref_len : l_pac; }
	else { const int64_t x = p + (end_correct ? len : ref_len); lo = x - ref_len > 0 ? x - ref_len : 0; hi = x < l_pac ? x : l_pac; }
	*pos_signed = p; *win_lo = lo; *win_n = hi > lo ? (int)(hi - lo) : 0;
}

/* window and query of one job; reads0 = seq (the read reversed), reads1 = rseq or a query in alignment orientation */
extern "C" void emu_fin_window(const uint8_t *pac, int64_t l_pac, int64_t win_lo, int win_n, const uint8_t *reads0, const uint8_t *reads1, int len,
							   int copy, uint8_t *ref_out, uint8_t *qry_out)
{
	std::vector<uint8_t> p(pac, pac + (l_pac + 3) / 4), r0, r1, ref((size_t)win_n, 0xa5), qry((size_t)len, 0xa5);
	if (reads0) r0.assign(reads0, reads0 + len);
	if (reads1) r1.assign(reads1, reads1 + len);
	FinJob J; memset(&J, 0, sizeof J);
	J.win_lo = win_lo; J.win_n = win_n; J.len = len; J.copy = copy; J.src_off = 0;
	fin_window_wave(p.data(), J, r0.data(), r1.data(), ref.data(), qry.data());
	if (win_n) memcpy(ref_out, ref.data(), (size_t)win_n);
	memcpy(qry_out, qry.data(), (size_t)len);
}

/* c32[0, nc): the path's operations, len << 4 | op (row-major here: stride 1).  Returns n_cigar, or -1 */
extern "C" int emu_fin_cigar(const uint32_t *c32, int nc, int max_cigar, int ext, int end_correct, int64_t pos, uint16_t *row_out, uint32_t *pos_out)
{
	std::vector<uint32_t> c(c32, c32 + (nc > 0 ? nc : 0));
	std::vector<uint16_t> row((size_t)max_cigar, 0xa5a5);
	const int n = fin_cigar_job(c.data(), 1, nc, max_cigar, ext, end_correct, pos, row.data(), pos_out);
	if (n > 0) memcpy(row_out, row.data(), (size_t)n * 2);
	return n;
}

/* MD and NM of one record: the counting pass, then the writing pass into a buffer of exactly the counted size.  Returns the length
 * (without the NUL), -1 if the two passes disagree, -2 if md_cap is too small. */
extern "C" int emu_fin_md(const uint8_t *pac, int64_t l_pac, int n_holes, const int64_t *hole_off, const int32_t *hole_len, const char *hole_amb,
						  const uint8_t *reads0, const uint8_t *reads1, int len, int copy, uint32_t pos, int n_cigar, const uint16_t *cigar,
						  char *md_out, int md_cap, int32_t *nm_out)
{
	EmuRef E(pac, l_pac, n_holes, hole_off, hole_len, hole_amb);
	std::vector<uint8_t> r0, r1;
	if (reads0) r0.assign(reads0, reads0 + len);
	if (reads1) r1.assign(reads1, reads1 + len);
	std::vector<uint16_t> cg(cigar, cigar + n_cigar);
	FinRec Q; memset(&Q, 0, sizeof Q);
	Q.pos = pos; Q.len = len; Q.n_cigar = n_cigar; Q.copy = copy;
	int32_t nm0 = -1, nm1 = -1;
	const uint32_t n0 = fin_md_wave<false>(E.R, Q, r0.data(), r1.data(), cg.data(), nullptr, &nm0);
	std::vector<char> md((size_t)n0 + 1, (char)0xa5);
	const uint32_t n1 = fin_md_wave<true>(E.R, Q, r0.data(), r1.data(), cg.data(), md.data(), &nm1);
	if (n0 != n1 || nm0 != nm1 || md[n0] != 0 || strlen(md.data()) != n0) return -1;
	if ((int)n0 + 1 > md_cap) return -2;
	memcpy(md_out, md.data(), (size_t)n0 + 1);
	*nm_out = nm1;
	return (int)n0;
}

#ifdef FINISH_EMU_MAIN
/* A stand-alone run for the sanitizers: a small reference with a hole, reads cut from it at every pac phase and at both ends of the
 * text, with a mismatch, an insertion and a deletion planted; the MD string is checked against a base-by-base walk. */
static uint32_t rnd(uint64_t *s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(*s >> 33); }
int main()
{
	const int64_t l_pac = 1003;
	std::vector<uint8_t> base((size_t)l_pac), pac((size_t)(l_pac + 3) / 4, 0);
	uint64_t s = 7;
	for (int64_t i = 0; i < l_pac; ++i) { base[i] = (uint8_t)(rnd(&s) & 3u); pac[i >> 2] |= (uint8_t)(base[i] << ((~i & 3) << 1)); }
	const int64_t hoff[2] = { 300, 700 }; const int32_t hlen[2] = { 20, 1 }; const char hamb[2] = { 'N', 'R' };
	int n_bad = 0, n_run = 0;
	for (int len : { 17, 63, 64, 65, 100, 257 })
		for (int64_t p0 : { (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)290, (int64_t)310, (int64_t)650, l_pac - len - 3, l_pac - len }) {
			if (p0 < 0 || p0 + len > l_pac) continue;
			/* window */
			for (int ext : { 1, -2 }) {
				int64_t ps, lo; int wn;
				emu_fin_extent(l_pac, (uint32_t)p0, len, ext, 1, &ps, &lo, &wn);
				std::vector<uint8_t> q((size_t)len), ref((size_t)wn + 1), qo((size_t)len);
				for (int k = 0; k < len; ++k) q[k] = base[p0 + k];
				emu_fin_window(pac.data(), l_pac, lo, wn, q.data(), q.data(), len, ext > 0, ref.data(), qo.data());
				for (int k = 0; k < wn; ++k) if (ref[k] != base[lo + k]) ++n_bad;
				for (int k = 0; k < len; ++k) if (qo[k] != (ext > 0 ? q[k] : q[len - 1 - k])) ++n_bad;
				++n_run;
			}
			/* MD: ungapped with one mismatch, then 5M 2I .. 3D .. */
			std::vector<uint8_t> q((size_t)len);
			for (int k = 0; k < len; ++k) q[k] = base[p0 + k];
			q[len / 2] = (uint8_t)((q[len / 2] + 1) & 3);
			char md[1024]; int32_t nm = 0;
			uint16_t cg[5] = { FIN_CMAKE(0, 5), FIN_CMAKE(1, 2), FIN_CMAKE(0, (len - 7) / 2), FIN_CMAKE(2, 3), FIN_CMAKE(0, len - 7 - (len - 7) / 2) };
			for (int nc : { 0, 5 }) {
				const int r = emu_fin_md(pac.data(), l_pac, 2, hoff, hlen, hamb, q.data(), q.data(), len, 1, (uint32_t)p0, nc, cg, md, (int)sizeof md, &nm);
				if (r < 0) { ++n_bad; continue; }
				/* the walk of bwase.c:253-315 */
				std::string want; int u = 0, wnm = 0, y = 0; int64_t pos = p0; char t[32];
				auto rc = [&](int64_t x) -> int { for (int h = 0; h < 2; ++h) if (x >= hoff[h] && x < hoff[h] + hlen[h]) return hamb[h]; return base[x]; };
				auto bc = [](int c) -> char { return c > 3 ? (char)c : "ACGT"[c]; };
				const int n_ops = nc ? nc : 1;
				for (int k = 0; k < n_ops; ++k) {
					const int l = nc ? FIN_CLEN(cg[k]) : len, op = nc ? FIN_COP(cg[k]) : 0;
					if (op == 0) for (int z = 0; z < l && pos < l_pac; ++z, ++y, ++pos) { const int c = rc(pos); if (c > 3 || q[y] > 3 || c != q[y]) { snprintf(t, sizeof t, "%d%c", u, bc(c)); want += t; ++wnm; u = 0; } else ++u; }
					else if (op == 1) { y += l; wnm += l; }
					else { snprintf(t, sizeof t, "%d^", u); want += t; for (int z = 0; z < l && pos < l_pac; ++z, ++pos) want += bc(rc(pos)); u = 0; wnm += l; }
				}
				snprintf(t, sizeof t, "%d", u); want += t;
				if (want != md || wnm != nm) { ++n_bad; fprintf(stderr, "len %d pos %lld nc %d: got %s / %d, want %s / %d\n", len, (long long)p0, nc, md, nm, want.c_str(), wnm); }
				++n_run;
			}
		}
	/* CIGAR end rules */
	{
		const uint32_t c32[4] = { 2u << 4 | 2u, 10u << 4 | 0u, 3u << 4 | 1u, 1u << 4 | 2u };     /* 2D 10M 3I 1D */
		uint16_t row[8]; uint32_t pos = 0;
		const int n = emu_fin_cigar(c32, 4, 8, -3, 1, 100, row, &pos);
		if (n != 2 || row[0] != FIN_CMAKE(0, 10) || row[1] != FIN_CMAKE(3, 3) || pos != 100 + (3 - 3) + 2) ++n_bad;
		if (emu_fin_cigar(c32, 4, 3, -3, 1, 100, row, &pos) != -1) ++n_bad;
		++n_run;
	}
	printf("finish_emu: %d checks, %d failed\n", n_run, n_bad);
	return n_bad ? 1 : 0;
}
#endif
