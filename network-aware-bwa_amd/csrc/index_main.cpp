// index_main.cpp -- `nabwa_index`: the reference's `bwa index` command (bwtindex.c:39-196) on top of libnabwa.so.
//
//   nabwa_index [-a bwtsw|is|div] [-p prefix] [-c] <in.fasta>
//
// Writes the reference's eight files, <prefix>.pac .ann .amb .rpac .bwt .rbwt .sa .rsa (with -c also <prefix>.nt.pac .nt.ann
// .nt.amb, and the index is of the colour text), byte for byte what `bwa index` writes for the same input
// (tests/test_index_pac.py, tests/test_gpu_index_build.py).  The FASTA is packed on the host (nabwa_index_fa2pac); both
// FM-indexes are built on the GPU (nabwa_index_build).  -a is accepted and changes nothing: the suffix array is unique, so
// every algorithm writes the same bytes.
//
// Exit status: 0 done, 1 usage or bad input, 2 no usable GPU or a GPU failure.  Without a GPU nothing is written.
// NABWA_DEVICE picks the GPU (default 0).
#define TOOL "nabwa_index"
#include "tool_common.hpp"

static int usage()
{
	fprintf(stderr, "\n");
	fprintf(stderr, "Usage:   nabwa_index [-a bwtsw|div|is] [-p prefix] [-c] <in.fasta>\n\n");
	fprintf(stderr, "Options: -a STR    BWT construction algorithm of the reference: bwtsw, is or div (accepted; the output is the same)\n");
	fprintf(stderr, "         -p STR    prefix of the index [same as fasta name]\n");
	fprintf(stderr, "         -c        build color-space index\n\n");
	fprintf(stderr, "Environment: NABWA_DEVICE (the GPU, default 0), NABWA_INDEX_MAX_BYTES (a cap on the device memory the build may use)\n\n");
	return 1;
}

int main(int argc, char *argv[])
{
	const char *prefix = nullptr;
	int c, is_color = 0;
	while ((c = getopt(argc, argv, "ca:p:")) >= 0) {
		switch (c) {
		case 'a':
			if (strcmp(optarg, "div") != 0 && strcmp(optarg, "bwtsw") != 0 && strcmp(optarg, "is") != 0) {
				fprintf(stderr, "[nabwa_index] unknown algorithm: '%s'.\n", optarg);
				return 1;
			}
			break;
		case 'p': prefix = optarg; break;
		case 'c': is_color = 1; break;
		default: return 1;
		}
	}
	if (optind + 1 > argc) return usage();
	const char *fasta = argv[optind];
	if (!prefix) prefix = fasta;

	// no GPU, no output: bad input is still reported as such, and first (the check reads the input and writes nothing)
	int device;
	if (!tool_device(&device, nullptr)) {
		if (nabwa_index_fa2pac(fasta, nullptr) < 0) {
			fprintf(stderr, "[nabwa_index] %s\n", nabwa_last_error());
			return 1;
		}
		tool_device(&device, "; nothing was written");
		return 2;
	}

	double t0 = now_s();
	fprintf(stderr, "[nabwa_index] Pack %sFASTA... ", is_color ? "nucleotide FASTA and convert it to colours (" : "");
	const int64_t l_pac = is_color ? nabwa_index_fa2cspac(fasta, prefix) : nabwa_index_fa2pac(fasta, prefix);
	if (l_pac < 0) {
		fprintf(stderr, "\n[nabwa_index] %s\n", nabwa_last_error());
		return 1;
	}
	fprintf(stderr, "%s%.2f sec (%lld bases, .pac .ann .amb .rpac%s)\n", is_color ? ") " : "",
			now_s() - t0, (long long)l_pac, is_color ? " .nt.*" : "");

	t0 = now_s();
	const int rc = nabwa_index_build(prefix, device, 32, 1);
	if (rc != NABWA_OK) {
		fprintf(stderr, "[nabwa_index] building the FM-indexes failed: %s\n", nabwa_last_error());
		return rc == NABWA_ENODEV || rc == NABWA_ENOMEM ? 2 : 1;
	}
	fprintf(stderr, "[nabwa_index] GPU build %.2f sec\n", now_s() - t0);
	return 0;
}
