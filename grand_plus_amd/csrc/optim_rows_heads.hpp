// optim_rows_heads.hpp -- how a wave walks the head rows of a window of 64 sorted positions, stated once for
// the two units that step the embedding table from a row list: optim_rows.hip (§7t) and optim_defer.hip (§7za).  Which
// positions are heads is optim_rows_layout.hpp's rule; this is only the consumption of their ballot.
#pragma once

#include "gp_common.hpp"

namespace {

// The next head rows of a window, up to R at a time: `heads` is the ballot of the window's heads, consumed lowest first;
// returns how many rows were taken (wave-uniform).
template <int R>
__device__ __forceinline__ int take_heads(u64& heads, long long key, long long (&rows)[R])
{
    int n = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        rows[r] = 0;
        if (heads) {
            const int l = __builtin_ctzll(heads);
            heads &= heads - 1;
            rows[r] = __shfl(key, l);
            n = r + 1;
        }
    }
    return n;
}

}  // namespace
