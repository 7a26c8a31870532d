// gather_chunk_layout.hpp -- the chunk, slot and size arithmetic of the chunked gather, HIP-free: the standard
// library alone, so that tests/native/gather_chunk_check.cpp holds the very lines the kernels of gather_chunk.hpp run
// against a brute-force enumeration, on the CPU and under the sanitizers.
//
// A segment is the run of equal keys at the sorted positions seg_start .. seg_start + n - 1.  It is cut into
// P = ceil(n / C) chunks counted from its own first position: chunk p starts at seg_start + p * C.  A segment with n > C is
// LONG: every chunk of it is summed into a scratch row, and the fold sums those rows in p order.  The scratch holds two
// rows per aligned span [m * C, (m + 1) * C) of positions.  Of the chunks that START in one span,
//   - at most one has p >= 1: two later chunks of one segment lie C apart, and a later chunk of another segment starts
//     more than C past it.  It takes row 2 m;
//   - at most one is chunk 0 of a long segment, because such a segment covers the rest of the span.  It takes row 2 m + 1.
// Every index here comes from a position, never from a key alone, so it is in range for any key array, sorted or not.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GP_GATHER_CHUNK_HD __host__ __device__ inline
#else
#define GP_GATHER_CHUNK_HD inline
#endif

namespace gp_gather_chunk {

constexpr long long kMinChunk = 64, kMaxChunk = 4096;

// A chunk length the kernels take: a power of two in [64, 4096].
GP_GATHER_CHUNK_HD bool chunk_ok(long long C) { return C >= kMinChunk && C <= kMaxChunk && (C & (C - 1)) == 0; }

// P: the chunks of a segment of n positions.
GP_GATHER_CHUNK_HD long long chunk_count(long long n, long long C) { return (n + C - 1) / C; }

// Where chunk p of the segment that starts at seg_start starts.
GP_GATHER_CHUNK_HD long long chunk_start(long long seg_start, long long p, long long C) { return seg_start + p * C; }

// The chunk that position q >= seg_start lies in, and whether q starts it.
GP_GATHER_CHUNK_HD long long chunk_of(long long q, long long seg_start, long long C) { return (q - seg_start) / C; }
GP_GATHER_CHUNK_HD bool starts_chunk(long long q, long long seg_start, long long C) { return ((q - seg_start) & (C - 1)) == 0; }

// The scratch: rows, and bytes for rows of `width` floats.
GP_GATHER_CHUNK_HD long long scratch_rows(long long n_sorted, long long C) { return 2 * ((n_sorted + C - 1) / C); }
GP_GATHER_CHUNK_HD long long scratch_bytes(long long n_sorted, long long C, long long width)
{
    return scratch_rows(n_sorted, C) * width * 4;
}

// The scratch row of chunk p of a long segment, q its first position: below scratch_rows(n_sorted, C) for every q < n_sorted.
GP_GATHER_CHUNK_HD long long slot_of(long long q, long long p, long long C) { return 2 * (q / C) + (p == 0 ? 1 : 0); }

// Whether the segment of `key` that starts at q0 has more than C positions.
GP_GATHER_CHUNK_HD bool is_long(const long long* keys, long long n_sorted, long long q0, long long key, long long C)
{
    return q0 + C < n_sorted && keys[q0 + C] == key;
}

// The first position of the segment that position base - 1 >= 0 lies in, key = keys[base - 1]: the lower bound of key in
// keys[0, base).  It gallops back from base - 1 (a short segment costs two or three loads) and then bisects.  Reads
// keys[0 .. base - 1] alone and returns a value in [0, base - 1], sorted keys or not.
GP_GATHER_CHUNK_HD long long seg_start_of(const long long* keys, long long base, long long key)
{
    long long hi = base - 1, step = 1;                   // keys[hi] >= key throughout
    while (hi - step >= 0 && keys[hi - step] >= key) {
        hi -= step;
        step <<= 1;
    }
    long long lo = hi - step >= 0 ? hi - step + 1 : 0;  // keys[lo - 1] < key, or lo = 0
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (keys[mid] >= key) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // namespace gp_gather_chunk
