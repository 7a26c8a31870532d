// gfpush_hash.hpp -- where a key goes: the hashes of every LDS table and sketch of the two GFPush kernels.
//
// No HIP: this header includes the C++ standard library only and compiles with plain g++ -std=c++17, so
// tests/native/gfpush_hash_check.cpp evaluates every function on a CPU, under the sanitizers, and tests/collision_cases.py holds
// its numpy mirror to that program.  gfpush_kernels.hpp and gfpush_sketch.hpp include it and keep no second copy; the inline
// assembly twins (GP_IW4_H*, insert_window) stay in gfpush_kernels.hpp.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define GP_HD __host__ __device__ __forceinline__
#else
#define GP_HD inline
#endif

namespace gp {

constexpr uint32_t kMaxProbe   = 24;      // an LDS insert that probes this many slots reports overflow
constexpr uint32_t kProbeSpan  = kMaxProbe * (kMaxProbe + 1) / 2;   // furthest a triangular probe sequence can walk (300 slots)
                                          // (recoverable: the level / aggregation is redone in more partitions)
constexpr uint32_t kSkMul24    = 0x9E3779u;     // sketch hash: cell = top bits of (low 24 bits of the key) * kSkMul24 -- a FULL-RATE multiply (sk_cell)

// Low 32 bits of the product of the low 24 bits of both operands: v_mul_u32_u24 on the device.
GP_HD uint32_t mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return (uint32_t)((uint64_t)(a & 0xFFFFFFu) * (uint64_t)(b & 0xFFFFFFu));
#endif
}

// Multiplicative (Fibonacci-style) hashes; slot_of() consumes the HIGH bits.
GP_HD uint32_t hash_a(uint32_t k) {            // residue / aggregation tables
    k *= 0x9E3779B1u; k ^= k >> 15; k *= 0x85EBCA77u;
    return k;
}
GP_HD uint32_t hash_b(uint32_t k) {            // partition choice (independent of hash_a)
    k *= 0x7FEB352Du; k ^= k >> 16; k *= 0x846CA68Bu;
    return k;
}
GP_HD uint32_t slot_of(uint32_t h, uint32_t cap) { return (uint32_t)(((uint64_t)h * cap) >> 32); }
// Home slot in an LDS table of `cap` slots.  Homes lie in [0, cap - kProbeSpan): a probe sequence then
// never leaves [0, cap), so the probing loops need no wrap-around (4 VALU per probe); 2 % of a full
// table is the price.  Every LDS table has cap >= kMinCap > kProbeSpan.
GP_HD uint32_t home_lds(uint32_t k, uint32_t cap) { return slot_of(hash_a(k), cap - kProbeSpan); }

// The sketch-cell hash of a key (cells are indexed by its top bits).  v_mul_u32_u24, not v_mul_lo_u32: the full 32 x 32-bit
// multiply issues at a quarter of the rate, and this hash is computed per edge in STREAM and per record in FILTER and in TOP-K's sweep.
// (Which nodes share a cell is irrelevant for a bound that only ever adds; the low 24 bits of a key are its unit number on every
// graph of up to 2^24 units.)
GP_HD uint32_t sk_cell(uint32_t key) { return mul24(key, kSkMul24); }
// Home slot of a key in the sketch kernel's LDS tables: the C++ twin of GP_IW4_HASHES (gfpush_kernels.hpp), full-rate multiplies only.
GP_HD uint32_t sk_home(uint32_t k, uint32_t cap) {
    uint32_t h = mul24(k, 0x9E3779u); h ^= h >> 15; h = mul24(h, 0x85EBCBu);
    // (HIP declares __umul24 as returning int, so this shift has always been an ARITHMETIC one on the device; it is kept, to leave
    //  the device code as it was.  The product is below 2^31 -- the shift kind makes no difference -- while cap - kProbeSpan < 32768.)
    return (uint32_t)((int32_t)mul24(h >> 16, cap - kProbeSpan) >> 16);
}

}  // namespace gp
