// search_slots.hpp -- the counter blocks the search kernels (W: fm_width_kernel, S: fm_search_kernel, D: deep_wave_body) and the host
// share, slot by slot.  Plain C++: included by device code, by host code and by the g++ emulation of kernel D (tests/emu/).
// A slot is one word of its block; the *_WORDS names are block sizes in words.  The numbers are the layout: scripts under profiles/
// read the statistics lines the host prints from them, in the order the format strings there give.
#pragma once

// Work counters (nabwa_batch::d_counter, SearchParams::work_counter): unsigned int, cleared before every launch.
enum {
	WC_SEARCH = 0,         // kernels S and D: the next work item (S draws NABWA_WORK_CHUNK at a time, D one)
	WC_WIDTH  = 1,         // kernel W: the next work item (2 * read + strand)
	WC_WORDS  = 4
};

// Class counters (nabwa_batch::d_ncls; partition_kernel's cnt): unsigned int.  A read's class is the smaller restart count of its two
// strands' width passes, clipped to NCLS_N - 1.
enum {
	NCLS_N       = 3,      // classes: 0 (an exact occurrence exists), 1, 2+
	NCLS_SIZE    = 0,      // + class: reads of the class (partition pass 1)
	NCLS_CURSOR  = 5,      // + class: reads of the class placed so far (partition pass 2)
	NCLS_FIRST0  = 10,     // first work item of class 0 = reads of classes 1 and 2+; SearchParams::n_sync points HERE
	NCLS_WORDS   = 16
};

// Touch and trip statistics of the counting run (nabwa_batch::d_sum as SearchParams::touch_counter): unsigned long long.
enum {
	TS_TOUCH_S     = 0,    // bucket touches of the reference's bwt_match_gap (kernel S; kernel D adds those of the reads it finishes)
	TS_TOUCH_W     = 1,    // bucket touches of the reference's bwt_cal_width passes (kernel W)
	TS_TRIPS       = 2,    // kernel S: wave-trips
	TS_EXPAND      = 3,    // lane-trips that expand an entry (TK_EXPAND)
	TS_EXACT       = 4,    // ... take an exact-tail step on rows (TK_TAIL)
	TS_ENT_LOAD    = 5,    // ... fetch the arena entry of a pop that was not fetched ahead
	TS_SPEC        = 6,    // ... issue their loads before the bound window that may prune the entry is at hand
	TS_QUERY       = 7,    // ... issue a rank query
	TS_TWO         = 8,    // ... issue one that spans two buckets
	TS_EXITED      = 9,    // ... of lanes that have run out of work
	TS_JUMP        = 10,   // ... jump a tail or a forced walk through the interval table (TK_JUMP)
	TS_TEXT_EXPAND = 11,   // ... expand an entry in text form
	TS_TEXT_TAIL   = 12,   // ... compare an exact tail with the text (TK_TEXT_TAIL)
	TS_MAX_TRIPS   = 13,   // the longest read's trips (a maximum)
	TS_OVER_2000   = 14,   // reads that took more than 2000 trips
	TS_OVER_500    = 15,   // ... more than 500
	TS_LONG_READS  = 16,   // the reads over 8000 trips: how many; then their trips by kind
	TS_LONG_TRIPS  = 17,   // all their trips
	TS_LONG_KF     = 18,   // expansions in key form
	TS_LONG_ROW2   = 19,   // expansions on rows, two buckets
	TS_LONG_ROW1   = 20,   // expansions on rows, one bucket
	TS_LONG_TEXT   = 21,   // expansions in text form
	TS_LONG_POP    = 22,   // pops that had to fetch their entry
	TS_LONG_TAIL   = 23,   // exact-tail steps, on rows or on the text
	TS_LONG_JUMP   = 24,   // table jumps
	TS_LONG_GAP    = 25,   // of all their expansions: those of entries with a gap
	// kernel W's trip statistics (NABWA_W_STATS; the statistics instantiation of fm_width_kernel, with tables).  A text trip is a bulk trip or a text
	// run, a table trip one of 4 or of up to 8 levels; positions do not count terminators.  The packed halves wrap at 2^32 (about 16 M reads of 100 bp).
	TS_W_TRIPS     = 26,   // wave-trips
	TS_W_MAX       = 27,   // the trips of the item (one strand of one read, both passes) that took most (a maximum)
	TS_W_TEXT      = 28,   // text trips: lane-trips << 32 | positions
	TS_W_TABLE     = 29,   // table trips: lane-trips << 32 | positions
	TS_W_RANK      = 30,   // single steps with a rank query: lane-trips (= positions); << 32: the text trips begun in a seed pass
	TS_W_STEP      = 31,   // single steps without one (text mode, or an N): lane-trips (= positions)
	TS_WORDS       = 32
};

// nabwa_batch_checksum borrows the start of d_sum between runs: unsigned long long.
enum {
	CKS_SUM   = 0,         // order-independent sum over all hit rows (checksum_kernel)
	CKS_ROWS  = 1,         // hit rows
	CKS_WORDS = 2
};

// sure0 statistics (NABWA_SURE0_STATS; nabwa_batch::d_s0stats, SearchParams::s0_stats): unsigned long long.
enum {
	S0S_READS       = 0,   // reads searched as "one strand occurs exactly"
	S0S_KF_EMPTY    = 1,   // their 1-mismatch key-form children whose level-KT table entry was empty
	S0S_KF_LANDED   = 2,   // ... that were stored landed at depth KT
	S0S_NET         = 3,   // reads handed to kernel D by the safety net (the exact hit did not come first, or not at all)
	S0S_LEAPS       = 4,   // leaps taken
	S0S_LEAP_LEVELS = 5,   // levels leapt over
	S0S_WALKED      = 6,   // proven entries that walked instead (text position < levels left)
	S0S_WORDS       = 8
};

// Kernel D's statistics (nabwa_batch::d_deep_ctr, DeepParams::stats): unsigned long long.  Clock values are 10 ns ticks.
enum {
	DS_ROUNDS        = 0,  // rounds
	DS_CHAINS_RUN    = 1,  // lane-chains run
	DS_CHAINS_DONE   = 2,  // chains committed
	DS_STEPS         = 3,  // chain steps (wave-steps)
	DS_CAREFUL       = 4,  // careful rounds (one pop each)
	DS_POOL_FAIL     = 5,  // searches the page pool ran dry under
	DS_TAIL_RANK     = 6,  // exact tails: rank steps (lane counts)
	DS_TAIL_TEXT     = 7,  // exact tails: finished on the text
	DS_PAGE_BUMP     = 8,  // NOT a statistic: the low word is DeepParams::page_bump, the pool's allocation cursor = pages handed out
	DS_FORCED_ROWS   = 9,  // expansions without a difference allowed, on several rows
	DS_MAX_CLK       = 10, // the longest read: time (a maximum)
	DS_MAX_ROUNDS    = 11, // ... its rounds (a maximum)
	DS_SUM_CLK       = 12, // time in reads, all waves
	DS_WAVE_CLK      = 13, // the longest wave (a maximum)
	DS_EMU_COOP      = 14, // emulation only: wave-wide expansions of one-row chains
	DS_EMU_COOP_LEV  = 15, // emulation only: the levels they took
	DS_PH_POP        = 16, // time per phase of a round: pop
	DS_PH_CHAIN      = 17, // chains
	DS_PH_TAIL       = 18, // exact tails
	DS_PH_COMMIT     = 19, // commit
	DS_PH_HIT        = 20, // hit bookkeeping
	DS_TAIL_TURNS    = 21, // turns of the exact-tail loop
	DS_LANE_STEPS    = 22, // chain steps, lane counts
	DS_KEY_EXPAND    = 23, // expansions of entries in key form
	DS_KEY_TAIL      = 24, // tail jumps and hits of entries in key form
	DS_RECORDS       = 25, // records filed
	DS_CHILDREN      = 26, // children stored
	DS_PRUNED        = 27, // entries pruned at the pop
	DS_EXPAND        = 28, // expansions
	DS_TWO           = 29, // rank queries on two buckets
	DS_FORCED_KEY    = 30, // expansions without a difference allowed, in key form
	DS_FORCED_ONE    = 31, // ... on one row
	// DeepParams::hist == 1: expansions by depth (read symbols consumed, clipped to DS_HIST1_BINS - 1), one row of bins per form
	DS_HIST1         = 32, // + form * DS_HIST1_BINS + depth; forms: 0 rows (several), 1 rows (one), 2 key form
	DS_HIST1_BINS    = 32,
	// DeepParams::hist == 2: rounds by width (1, 2, 3-4, 5-8, 9-16, 17-32, 33-64 entries: DS_HIST2_BINS bins)
	DS_HIST2_ROUNDS  = 32, // + bin: rounds
	DS_HIST2_STEPS   = 64, // + bin: their wave-steps
	DS_HIST2_BINS    = 7,
	DS_WORDS         = 128
};

// What the CPU emulation of kernel D returns (tests/emu/deep_emu.cpp: the 16 words of its `stats` argument, which it hands to the kernel
// body as DeepParams::stats): unsigned long long.  Words DS_ROUNDS .. DS_TAIL_TEXT are those slots themselves; the others are picked out of
// the wave's DS_* counts at the end of the emulated body, the two touch totals are the harness's own.
enum {
	ES_TOUCH_W    = 8,     // harness: the reference's bucket touches in the width passes
	ES_TOUCH_S    = 9,     // harness: ... in bwt_match_gap
	ES_KEY_EXPAND = 10,    // DS_KEY_EXPAND
	ES_KEY_TAIL   = 11,    // DS_KEY_TAIL
	ES_FORCED_KEY = 12,    // DS_FORCED_KEY: forced walks through the table
	ES_FORCED_ONE = 13,    // DS_FORCED_ONE: forced walks on the text
	ES_COOP       = 14,    // DS_EMU_COOP
	ES_COOP_LEV   = 15,    // DS_EMU_COOP_LEV
	ES_WORDS      = 16
};
