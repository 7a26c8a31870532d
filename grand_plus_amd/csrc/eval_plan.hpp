// eval_plan.hpp -- how the evaluation's reduction cuts n rows into slices, stated once for
// gp_eval_reduce (evaluate.hip) and gp_eval_tail (eval_tail.hip).  HIP-free: nothing but <cstdint>, so that
// tests/native/eval_plan_check.cpp holds it against the numpy mirror of tests/eval_tail_cases.py on the CPU.
#pragma once

#include <cstdint>

namespace gp_eval {

constexpr int kSlots = 1024;                                  // slots of the reduction: GP_EVAL_WORKSPACE_BYTES / 40
constexpr int kMinSlice = 1024;                               // rows of a slice, at least
constexpr int kTailSlices = 64;                               // the slices one workgroup of gp_eval_tail walks, at most
constexpr int64_t kTailMaxRows = (int64_t)kTailSlices * kMinSlice;   // GP_EVAL_TAIL_MAX_ROWS
constexpr int64_t kTailWorkspaceBytes = 64;                   // GP_EVAL_TAIL_WORKSPACE_BYTES: the ticket counter, padded

struct ReducePlan {
    long long grid;                                           // slices: slice b is rows [b * slice, min(n, (b + 1) * slice))
    long long slice;
};

// the slices follow from n_rows alone: at least kMinSlice rows each, at most kSlots of them
inline ReducePlan reduce_plan(long long n_rows)
{
    long long grid = (n_rows + kMinSlice - 1) / kMinSlice;
    grid = grid < 1 ? 1 : grid > kSlots ? kSlots : grid;
    return {grid, (n_rows + grid - 1) / grid};
}

}  // namespace gp_eval
