// fit_perm.hpp -- the keyed permutation with random access behind the fit loop's batch selection, and the
// geometry and keys of a step's selection.  The one definition: csrc/fit.hip evaluates it on the device,
// tests/native/fit_perm_check.cpp on the host, and grand_plus_amd/_common.perm_index mirrors it in Python.
//
// HIP-free: nothing but <cstdint>.  The 64-bit mixer is a template argument, so that the device passes gp_common.hpp's mix64
// and this header does not restate it.
//
// perm(mix, key, n, i), 1 <= n < 2^31, i < n: the image of i under a permutation of [0, n); no array is materialised.  A 4-round
// Feistel network over b bits -- b = the bits of n - 1, at least 2, rounded up to even; h = b / 2; mask = 2^h - 1 --
//     round r:  (L, R) <- (R, L ^ (mix(key ^ (r + 1) * GP_FIT_ROUND_MUL ^ R) & mask))
// repeated on its own output while the result is >= n (cycle walking).  A Feistel network is a bijection of [0, 2^b) for any
// round function, and the walk follows the cycle that holds i < n, so it ends inside [0, n); 2^b <= 4n bounds the expected
// number of walks by 4.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define GP_FIT_HD __host__ __device__ __forceinline__
#else
#define GP_FIT_HD inline
#endif

// odd 64-bit multipliers that no other derivation of csrc/ uses
#define GP_FIT_ROUND_MUL 0xC2B2AE3D27D4EB4Full
#define GP_FIT_EPOCH_MUL 0x165667B19E3779F9ull
#define GP_FIT_UNLABEL_MUL 0x27D4EB2F165667C5ull

namespace gp_fit {

constexpr int kRounds = 4;

// the even number of bits of the network's domain: 2^bits >= n, 2^bits <= 4n
GP_FIT_HD int perm_bits(uint32_t n)
{
    int b = 0;
    for (uint32_t m = n - 1; m != 0; m >>= 1) ++b;
    if (b < 2) b = 2;
    return (b + 1) & ~1;
}

template <class Mix>
GP_FIT_HD uint32_t perm(Mix mix, uint64_t key, uint32_t n, uint32_t i)
{
    const int h = perm_bits(n) / 2;
    const uint64_t mask = (1ull << h) - 1;
    uint64_t x = i;
    do {
        uint64_t L = x >> h, R = x & mask;
        for (int r = 0; r < kRounds; ++r) {
            const uint64_t f = mix(key ^ ((uint64_t)(r + 1) * GP_FIT_ROUND_MUL) ^ R) & mask;
            const uint64_t nr = L ^ f;
            L = R;
            R = nr;
        }
        x = (L << h) | R;
    } while (x >= n);
    return (uint32_t)x;
}

// ---- a step's selection (gp_fit_select): step t >= 1 of a run with batches of batch_size over n_train labelled nodes
struct StepSlice {
    uint64_t epoch;      // (t - 1) / nb, nb = ceil(n_train / batch_size)
    uint32_t lo;         // the slice's start in the epoch's permutation: ((t - 1) % nb) * batch_size
    uint32_t n_labeled;  // min(batch_size, n_train - lo): the last slice of an epoch is short
};

GP_FIT_HD StepSlice step_slice(uint64_t t, uint32_t n_train, uint32_t batch_size)
{
    const uint64_t nb = ((uint64_t)n_train + batch_size - 1) / batch_size;
    const uint64_t lo = ((t - 1) % nb) * batch_size;
    const uint64_t left = n_train - lo;
    return {(t - 1) / nb, (uint32_t)lo, (uint32_t)(left < batch_size ? left : batch_size)};
}

// the key of an epoch's permutation of the labelled pool, and of a step's permutation of the unlabelled pool
template <class Mix>
GP_FIT_HD uint64_t epoch_key(Mix mix, uint64_t base_seed, uint64_t epoch) { return mix(base_seed ^ ((epoch + 1) * GP_FIT_EPOCH_MUL)); }

template <class Mix>
GP_FIT_HD uint64_t unlabel_key(Mix mix, uint64_t step_seed) { return mix(step_seed ^ GP_FIT_UNLABEL_MUL); }

}  // namespace gp_fit
