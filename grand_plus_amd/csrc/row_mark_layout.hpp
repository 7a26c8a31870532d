// row_mark_layout.hpp -- the bitmap of the rows a batch touched and the row list compacted from it, HIP-free:
// the standard library alone, so that tests/native/row_mark_check.cpp holds the very lines the kernels of row_mark.hip
// run against brute force, on the CPU and under the sanitizers.
//
// The bitmap has one bit per row of a [V, H] table in 32-bit words: row r is bit r & 31 of word r >> 5, words(V) words in
// all.  A bit at or above V (the unused high bits of the last word) is never set by the mark kernel and never emitted by
// the compaction, whatever the word holds.  The words are split into n_chunks contiguous ascending chunks, one per
// workgroup; the list position of a row is the number of valid set bits before it (the exclusive popcount prefix), so the
// list ascends and names each row once.  keys[0 .. capacity) takes the first min(total, capacity) rows, then the sentinel
// V; total > capacity is an overflow, in the sense of mag_det_layout.hpp.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GP_ROW_MARK_HD __host__ __device__ inline
#else
#define GP_ROW_MARK_HD inline
#endif

namespace gp_row_mark {

constexpr int kTile = 256;                    // words a workgroup scans at a time: one per thread
constexpr int kMaxChunks = 1024;              // workgroups of the two compaction launches, and partials of the count

GP_ROW_MARK_HD long long word_of(long long row) { return row >> 5; }
GP_ROW_MARK_HD unsigned bit_of(long long row) { return 1u << (unsigned)(row & 31); }
GP_ROW_MARK_HD long long words(long long V) { return (V + 31) >> 5; }

// The bits of word w that are rows of the table: all 32 below the last word, the low V - 32 w of a partial last word,
// none at or past words(V).
GP_ROW_MARK_HD unsigned valid_mask(long long w, long long V)
{
    const long long left = V - (w << 5);
    return left >= 32 ? 0xffffffffu : left <= 0 ? 0u : (1u << (unsigned)left) - 1u;
}

GP_ROW_MARK_HD int popcount(unsigned x) { return __builtin_popcount(x); }

// Chunks: as many as there are tiles, at least one, at most kMaxChunks; every chunk but the last holds chunk_words words.
GP_ROW_MARK_HD long long chunks(long long n_words)
{
    const long long tiles = (n_words + kTile - 1) / kTile;
    return tiles < 1 ? 1 : tiles < kMaxChunks ? tiles : kMaxChunks;
}

GP_ROW_MARK_HD long long chunk_words(long long n_words, long long n_chunks)
{
    const long long per = (n_words + n_chunks - 1) / n_chunks;
    return (per + kTile - 1) / kTile * kTile;                     // whole tiles: a tile never straddles two chunks
}

// Chunk c is the words [chunk_begin(c), chunk_begin(c + 1)); a chunk past the last word is empty.
GP_ROW_MARK_HD long long chunk_begin(long long c, long long n_words, long long n_chunks)
{
    const long long at = c * chunk_words(n_words, n_chunks);
    return at < n_words ? at : n_words;
}

// The rows of word w in ascending order into keys[prefix ...), prefix the number of valid set bits before the word; a
// position at or past capacity is written nowhere.  Returns the word's count.
GP_ROW_MARK_HD int emit_word(unsigned word, long long w, long long prefix, long long V, long long capacity, long long* keys)
{
    word &= valid_mask(w, V);
    const int n = popcount(word);
    for (long long pos = prefix; word && pos < capacity; ++pos) {
        keys[pos] = (w << 5) + __builtin_ctz(word);                // the lowest set bit first
        word &= word - 1;
    }
    return n;
}

// How many rows the list holds: the total, clamped at capacity.  The tail [tail_begin, capacity) takes the sentinel.
GP_ROW_MARK_HD long long tail_begin(long long total, long long capacity) { return total < capacity ? total : capacity; }

// Whether some touched row found no place in the list.
GP_ROW_MARK_HD bool overflowed(long long total, long long capacity) { return total > capacity; }

}  // namespace gp_row_mark
