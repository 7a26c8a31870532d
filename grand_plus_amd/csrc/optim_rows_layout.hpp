// optim_rows_layout.hpp -- which rows of the embedding table a batch touched, HIP-free: the standard library
// alone, so that tests/native/optim_rows_check.cpp holds the very lines the kernels of optim_rows.hip run against brute
// force, on the CPU and under the sanitizers.
//
// keys[0 .. n_sorted) is ascending: the sorted key list of MAG's deterministic backward (mag_det_abi.hpp), one key per
// entry of the batch, the sentinel V in the tail.  Position i is a HEAD when its key is a row of the table and it is the
// first position of its run; this is the rule by which gather_sum_kernel (gather_sum.hpp) writes a row of dW.  A row is
// TOUCHED when it has a head; it then has exactly one, however many windows of 64 positions its run crosses.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GP_OPTIM_ROWS_HD __host__ __device__ inline
#else
#define GP_OPTIM_ROWS_HD inline
#endif

namespace gp_optim_rows {

// Whether position i in [0, n_sorted) is a head: 0 <= keys[i] < V, and i == 0 or keys[i - 1] != keys[i].
GP_OPTIM_ROWS_HD bool is_head(const long long* keys, long long i, long long V)
{
    const long long key = keys[i];
    return key >= 0 && key < V && (i == 0 || keys[i - 1] != key);
}

// The first position whose key is >= row; n_sorted when there is none.
GP_OPTIM_ROWS_HD long long lower_bound(const long long* keys, long long n_sorted, long long row)
{
    long long lo = 0, hi = n_sorted;                      // keys[lo - 1] < row <= keys[hi] throughout
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (keys[mid] < row) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Whether row in [0, V) is touched: the lower bound finds its key, and that position is then the row's head.
GP_OPTIM_ROWS_HD bool touched(const long long* keys, long long n_sorted, long long row)
{
    const long long pos = lower_bound(keys, n_sorted, row);
    return pos < n_sorted && keys[pos] == row;
}

// Windows of 64 positions that cover the list; the last may be partial.
GP_OPTIM_ROWS_HD long long windows(long long n_sorted) { return (n_sorted + 63) >> 6; }

}  // namespace gp_optim_rows
