// tests/emu/bam_header_main.cpp -- TEST INFRASTRUCTURE ONLY.  header_text of csrc/bam_header.hpp as a stand-alone program:
//
//     bam_header_main [--coordinate] VERSION NAME:LENGTH[,NAME:LENGTH...] [WORD ...]  < old header text
//
// prints the text `nabwa_bam2bam` writes for that old header, those contigs and the command line WORD ...; --coordinate: as --sort does.
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <iostream>
#include <iterator>
#include <utility>
#include "../../network-aware-bwa_amd/csrc/bam_header.hpp"

int main(int argc, char **argv)
{
	int a = 1;
	bool coordinate = false;
	if (a < argc && !strcmp(argv[a], "--coordinate")) { coordinate = true; ++a; }
	if (argc - a < 2) return 2;
	const char *version = argv[a++];
	std::vector<std::pair<std::string, int32_t>> contigs;
	for (char *tok = strtok(argv[a++], ","); tok; tok = strtok(0, ",")) { char *c = strrchr(tok, ':'); if (!c) return 2; contigs.emplace_back(std::string(tok, c), (int32_t)atol(c + 1)); }
	const std::string old((std::istreambuf_iterator<char>(std::cin)), std::istreambuf_iterator<char>());
	auto each = [&](auto f) { for (auto &c : contigs) f(c.first.c_str(), c.second); };
	const std::string t = coordinate ? header_text(each, old, argc - a, argv + a, version, true) : header_text(each, old, argc - a, argv + a, version);
	fwrite(t.data(), 1, t.size(), stdout);
	return 0;
}
