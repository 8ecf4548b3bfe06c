// FriExitAir's layout, stated once for C: the columns, periodic columns and public inputs of the constraint program
// air_library.fri_exit_builder() (which states the same numbers; tests/test_fri_exit.py reads this file and compares).
// A block of FRI_EXIT_BLOCK rows handles one challenge value v of an inner proof's transcript: the proof-of-work response in
// block 0, one query-index challenge in every block after it.  Row r < 64 of a block holds bit 63 - r of v; rows 63 .. 126 are the
// Horner steps of the final polynomial (other columns than the bit rows use, so the two overlap on row 63); the block's LAST row
// receives the challenge and, in an index block, the exit of the query's fold chain.
#pragma once
#include <stdint.h>

enum {
    FRI_EXIT_BLOCK_LOG = 7,
    FRI_EXIT_BLOCK = 1 << FRI_EXIT_BLOCK_LOG,
    FRI_EXIT_BITS = 64,          // rows 0 .. 63: the bits of v, MSB first
    FRI_EXIT_HORNER_ROW = 63,    // the first Horner step
    FRI_EXIT_MAX_FINAL_LEN = 64  // Horner steps on rows 63 .. 126
};

// main columns
enum {
    FRI_EXIT_BIT = 0,     // the bit of v this row holds (0 behind row 63)
    FRI_EXIT_V = 1,       // the weighted sum of the bits above this row; v from row 64 on
    FRI_EXIT_F = 2,       // prefix flag: the top pow_bits rows of the PoW block, the top 64 - LN rows of an index block
    FRI_EXIT_C = 3,       // its counter: the public length on row 0, minus F on every row, 0 on the last row
    FRI_EXIT_EF = 4,      // exponent flag: the FB rows behind F in an index block
    FRI_EXIT_C2 = 5,      // its counter
    FRI_EXIT_G = 6,       // helper (1 - F) * BIT: an index bit
    FRI_EXIT_EB = 7,      // helper EF * BIT: an exponent bit
    FRI_EXIT_W = 8,       // w_FB^(2^s) on exponent step s (w_FB on the F rows behind row 0, 0 elsewhere)
    FRI_EXIT_X = 9,       // the point: 7^(16^NL) times the powers of W taken so far; x_NL behind the exponent rows
    FRI_EXIT_IDX = 10,    // the weighted sum of the index bits above this row; the index from row 64 on
    FRI_EXIT_T = 11,      // "all ones so far" over the top 32 bits, held over the low 32
    FRI_EXIT_HF = 12,     // Horner flag: final_len rows from row 63
    FRI_EXIT_K = 13,      // Horner steps left (this row included): the step's coefficient is K - 1
    FRI_EXIT_CA = 14,     // the step's coefficient, two words
    FRI_EXIT_CB = 15,
    FRI_EXIT_ACC = 16,    // the Horner accumulator before this row's step, two words
    FRI_EXIT_ACT = 18,    // the block receives a challenge
    FRI_EXIT_ISPOW = 19,  // ... the proof-of-work response
    FRI_EXIT_ORD = 20,    // the block's ordinal among the transcript's challenges: ORD_POW + the block's number
    FRI_EXIT_COLS = 21
};

// periodic columns (period FRI_EXIT_BLOCK)
enum {
    FRI_EXIT_P_FIRST = 0,  // row 0
    FRI_EXIT_P_LAST = 1,   // row 127
    FRI_EXIT_P_BIT = 2,    // rows 0 .. 63
    FRI_EXIT_P_WEIGHT = 3, // 2^(63 - r) on rows 0 .. 63
    FRI_EXIT_P_HIGH = 4,   // rows 1 .. 31: T' = T * BIT
    FRI_EXIT_P_HOLD = 5,   // rows 32 .. 62: T' = T
    FRI_EXIT_P_LOW = 6,    // rows 32 .. 63: T * BIT = 0
    FRI_EXIT_P_PRE = 7,    // rows 0 .. 62: no Horner step
    FRI_EXIT_P_R62 = 8,    // row 62: the Horner flag may rise behind it
    FRI_EXIT_PERIODIC = 9
};

// public inputs
enum {
    FRI_EXIT_PUB_ORD_POW = 0,
    FRI_EXIT_PUB_ABSORBED = 1,
    FRI_EXIT_PUB_POW_BITS = 2,
    FRI_EXIT_PUB_SKIP = 3,  // 64 - LN
    FRI_EXIT_PUB_FB = 4,
    FRI_EXIT_PUB_W = 5,     // w_FB = w_LN^(16^NL)
    FRI_EXIT_PUB_G = 6,     // 7^(16^NL)
    FRI_EXIT_PUB_FINAL_LEN = 7,
    FRI_EXIT_PUB_DIGEST = 8,
    FRI_EXIT_PUB = 12
};

// bus: three messages a row, two helpers
enum { FRI_EXIT_N_HELP = 2, FRI_EXIT_AUX_COLS = 6, FRI_EXIT_MAX_LAYERS = 8 };
