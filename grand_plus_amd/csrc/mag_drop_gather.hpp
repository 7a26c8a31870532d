// mag_drop_gather.hpp -- the one call between mag_drop.hip (§7y: the checks, U and inv of the deterministic backward with
// input dropout) and mag_prop.hip, which keeps the gather's Op: the Op hashes the input-dropout mask of
// (sample, resident slot), and GP_MAG_SLOT_SEED's only definition on the device is mag_prop.hip's slot_seed.  Host code
// alone crosses the units: a struct of the call's operands, and the launches of the gather over them.
#pragma once

#include <stdint.h>

namespace gp_mag_drop {

struct GatherCall {
    const float* U;                                       // [S, n_batch * K, dim], mag_drop.hip's kernel wrote it
    int64_t n_vocab; int32_t dim;
    const int64_t* attr_indptr; const int32_t* attr_indices; const float* attr_data; int64_t n_nodes;
    const int32_t* col; const int32_t* filled; int64_t n_rows; int32_t K;
    const int32_t* batch_rows; int32_t n_batch; int32_t n_samples;
    float input_droprate; int drop;                       // drop: training and input_droprate > 0 (a mask is drawn)
    uint64_t seed; const uint64_t* d_seed;
    const int64_t* slot_base; const int64_t* order; const int64_t* sorted_keys; int64_t max_entries;
    float* dW;
    int32_t chunk; float* scratch;                        // chunk = 0: gather_sum_kernel; else gather_chunk.hpp's two launches
};

// gather_sum_kernel<MagDropOp>, or the chunked gather, on `stream` (a hipStream_t).  Returns a GP_* status.
int gather(const GatherCall& c, void* stream);

}  // namespace gp_mag_drop
