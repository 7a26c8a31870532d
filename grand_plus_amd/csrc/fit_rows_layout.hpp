// fit_rows_layout.hpp -- who copies what in the dirty-row snapshot of csrc/fit_rows.hip, HIP-free: the standard
// library alone, so that tests/native/fit_rows_check.cpp holds the very lines the kernel runs against brute force, on the
// CPU and under the sanitizers.
//
// The dirty bitmap is row_mark_layout.hpp's: row r is bit r & 31 of word r >> 5, a bit at or above V is no row.  It is not
// restated here.  The snapshot launches workgroups of kWaves waves, at most `cap` of them; wave v of the n_waves in the
// grid owns the words v, v + n_waves, v + 2 n_waves, ... -- one word a trip, every word exactly one wave -- so the wave that
// reads a word is the one that clears it and no other wave ever looks at it.
//
// A row is per_row units (16-byte or 4-byte ones).  The 64 lanes of a wave form groups of 2^g lanes, 2^g the smallest power
// of two that covers per_row, at most 64; a group copies one row, so a pass of the wave copies 64 >> g of the word's set
// rows, in ascending order, and lane j0 of a group copies the units j0, j0 + 2^g, ... of its row.
#pragma once

#include "row_mark_layout.hpp"

namespace gp_fit_rows {

constexpr int kWaves = 4;                     // waves of a workgroup: words taken at once
constexpr int kLanes = 64;

// Workgroups of the snapshot over n_words words: a wave per word, at least one, at most cap.
GP_ROW_MARK_HD long long grid(long long n_words, long long cap)
{
    const long long g = (n_words + kWaves - 1) / kWaves;
    return g < 1 ? 1 : g < cap ? g : cap;
}

// Trips of the grid-stride loop: the words of the busiest wave.
GP_ROW_MARK_HD long long trips(long long n_words, long long n_waves) { return (n_words + n_waves - 1) / n_waves; }

// The word wave `wave` owns on trip `trip`; at or past n_words the wave has run out of words.
GP_ROW_MARK_HD long long owned_word(long long wave, long long trip, long long n_waves) { return trip * n_waves + wave; }

// The bits of word w that are rows of the table.
GP_ROW_MARK_HD unsigned live_bits(unsigned word, long long w, long long V) { return word & gp_row_mark::valid_mask(w, V); }

// log2 of the lanes that copy one row of per_row units.
GP_ROW_MARK_HD int group_log2(long long per_row)
{
    int g = 0;
    while (g < 6 && (1ll << g) < per_row) ++g;
    return g;
}

// Passes a wave needs for a word with n set rows, 64 >> g of them a pass.
GP_ROW_MARK_HD int passes(int n, int g)
{
    const int per_pass = kLanes >> g;
    return (n + per_pass - 1) / per_pass;
}

// Which of the word's set rows (0 = the lowest) lane `lane` copies on pass `pass`; at or past the word's count, none.
GP_ROW_MARK_HD int lane_slot(int lane, int pass, int g) { return pass * (kLanes >> g) + (lane >> g); }

// The first unit lane `lane` copies of its row; it goes on in steps of 1 << g.
GP_ROW_MARK_HD int lane_first(int lane, int g) { return lane & ((1 << g) - 1); }

// The row of the k-th set bit of word w (k below the popcount of `bits`).
GP_ROW_MARK_HD long long nth_row(unsigned bits, long long w, int k)
{
    for (int i = 0; i < k; ++i) bits &= bits - 1;                 // drop the k lowest set bits
    return (w << 5) + __builtin_ctz(bits);
}

}  // namespace gp_fit_rows
