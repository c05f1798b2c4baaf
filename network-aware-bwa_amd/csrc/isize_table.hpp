// isize_table.hpp -- the per-@RG insert-size table of bam2bam's two passes (insert_size.c:141-213): what pass 1 fills, infer_all turns into
// estimates and pass 2 reads.  Host only.
#pragma once
#include <stdint.h>
#include <map>
#include <string>
#include <vector>
#include "../../include/nabwa.h"

struct nabwa_isize_table {
	struct Rg { nabwa_isize_t ii; std::vector<uint16_t> hist; bool has_hist; };
	std::map<std::string, Rg> rg;        /* (the reference keeps a khash; its iteration order only decides the order of log lines) */
	double ap_prior; int64_t L;
	nabwa_poscache_t *poscache;          /* finish_pair's position cache of the file (bam2bam.c:1186-1203): lives as long as pass 2 does, like this table */
};

/* the read group's entry, made on first use (improve_isize_est, insert_size.c:141-165, adds one logical record's bin to its histogram) */
nabwa_isize_table::Rg *isize_slot(nabwa_isize_table *t, const std::string &rg);
