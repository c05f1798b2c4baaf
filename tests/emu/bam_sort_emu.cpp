// tests/emu/bam_sort_emu.cpp -- TEST INFRASTRUCTURE ONLY.  The per-lane bodies of the BAM coordinate sort (csrc/bam_sort_body.hpp) compiled
// by g++ and run lane by lane on the CPU: the key of a record, the copy of one record by its group of lanes, and the whole stage -- keys, a
// stable sort of (key, index), the scan of the permuted sizes, the gather -- as bam_sort.hip strings the kernels together.
#define NABWA_EMU 1
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../../network-aware-bwa_amd/csrc/bam_sort_body.hpp"

extern "C" uint64_t emu_bsort_key(const uint8_t *rec) { return bsort_key(rec); }
extern "C" uint32_t emu_bsort_u32(const uint8_t *p) { return bsort_u32(p); }

/* the group's lanes one after the other; backwards != 0: in the opposite order (no lane depends on another) */
extern "C" void emu_bsort_copy(const uint8_t *src, uint8_t *dst, int64_t n, int backwards)
{
	for (int k = 0; k < BSORT_LANES; ++k) bsort_copy_part(src, dst, n, backwards ? BSORT_LANES - 1 - k : k);
}

/* the stage: returns -1, or the lowest record whose block_size is not what its offsets say (the key kernel's flag) */
extern "C" int64_t emu_bsort_run(int64_t n, const uint8_t *in, const int64_t *off, uint8_t *out, int64_t *out_off, uint64_t *keys_out)
{
	std::vector<uint64_t> keys((size_t)n);
	std::vector<uint32_t> idx((size_t)n);
	int64_t bad = -1;
	for (int64_t i = 0; i < n; ++i) {
		const uint8_t *rec = in + (off[i] - off[0]);
		keys[(size_t)i] = bsort_key(rec);
		idx[(size_t)i] = (uint32_t)i;
		if ((int64_t)bsort_u32(rec) + 4 != off[i + 1] - off[i] && bad < 0) bad = i;
	}
	std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
	out_off[0] = 0;
	for (int64_t j = 0; j < n; ++j) out_off[j + 1] = out_off[j] + (off[idx[(size_t)j] + 1] - off[idx[(size_t)j]]);
	for (int64_t j = 0; j < n; ++j) {
		keys_out[j] = keys[idx[(size_t)j]];
		for (int t = 0; t < BSORT_LANES; ++t) bsort_copy_part(in + (off[idx[(size_t)j]] - off[0]), out + out_off[j], out_off[j + 1] - out_off[j], t);
	}
	return bad;
}
