// read_trim.hpp -- bwa_trim_read (bwaseqio.c:110-123), the one spelling of it: the length that is kept of a read of `full` bases when
// its 3' end is scanned for the stretch whose qualities fall short of trim_qual.  A read is never cut below BWA_MIN_RDLEN = 35 bases.
// phred(l) is the quality of base l in the read's own orientation; the callers differ in its domain and keep their own: the BAM
// front-end caps 255 at 93 (bam_rec.hpp), the tools' readers hand in phred + 33 characters (read_input.hpp), nabwa_encode_read raw phred.
#pragma once

template <class Phred> static inline int bwa_trimmed_len(int full, int trim_qual, Phred phred)
{
	int sum = 0, best = 0, best_l = full - 1;
	for (int l = full - 1; l >= 35 - 1; --l) {
		sum += trim_qual - phred(l);
		if (sum < 0) break;
		if (sum > best) { best = sum; best_l = l; }
	}
	return best_l + 1;
}
