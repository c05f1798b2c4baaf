// tests/emu/damage_emu.cpp -- TEST INFRASTRUCTURE ONLY.  The bodies of the damage profile (csrc/damage_body.hpp) compiled by g++ and run on the
// CPU as nabwa_damage.hip strings them together: the workgroups of the grid one after the other, each with its 32-bit table, into the call's
// 64-bit table; the call's table goes onto the caller's totals only when no record was damaged.
#define NABWA_EMU 1
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../network-aware-bwa_amd/csrc/damage_body.hpp"

/* one call: totals[0, words) += the call's table, and -1; or the lowest damaged record, and the totals as they were.  No byte outside
 * in[off[0], off[n]) and none outside pac[0, l_pac / 4 + 1) is read. */
extern "C" int64_t emu_damage_run(int64_t n_rec, const uint8_t *in, const int64_t *off, const uint8_t *pac, int64_t l_pac, int n_holes, const int64_t *hole_off,
								  const int32_t *hole_len, int n_contigs, const int64_t *contig_off, int n_pos, int min_mapq, uint32_t exclude_flags,
								  uint32_t require_flags, int n_blocks, uint64_t *totals)
{
	std::vector<FinHole> holes((size_t)n_holes);
	for (int i = 0; i < n_holes; ++i) holes[(size_t)i] = FinHole{ hole_off[i], hole_len[i], 'N' };
	DmgParams P;
	P.in = in + off[0]; P.off = off;                              /* (record i is in[off[i] ..), as for the library; the device holds the bytes from off[0] on) */ P.base = off[0]; P.n_rec = (int32_t)n_rec;
	P.n_contigs = n_contigs; P.contig_off = contig_off;
	P.R.pac = pac; P.R.l_pac = l_pac; P.R.holes = holes.data(); P.R.n_holes = n_holes; P.R.pad = 0;
	P.n_pos = n_pos; P.min_mapq = min_mapq; P.exclude_flags = exclude_flags; P.require_flags = require_flags;
	const DmgTab T = dmg_tab(n_pos);
	std::vector<unsigned long long> call((size_t)T.words, 0);
	std::vector<uint32_t> tab((size_t)T.words, 0xdeadbeefu);       /* (LDS starts out as anything) */
	unsigned int bad = 0xffffffffu;
	for (int b = 0; b < n_blocks; ++b) {
		dmg_block(P, tab.data(), call.data(), &bad, b, n_blocks);
		for (uint32_t v : tab) if (v) return -2;                   /* a workgroup leaves its table flushed */
	}
	if (bad != 0xffffffffu) return (int64_t)bad;
	for (int w = 0; w < T.words; ++w) totals[w] += call[(size_t)w];
	return -1;
}
