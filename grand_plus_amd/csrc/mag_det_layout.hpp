// mag_det_layout.hpp -- the slot / entry arithmetic of MAG's deterministic backward, HIP-free: the standard
// library alone, so that tests/native/mag_det_check.cpp holds the very lines the kernels of mag_det.hip run against a
// brute-force enumeration, on the CPU and under the sanitizers.
//
// A slot is e = b * K + k.  slot_base[0 .. n_slots] is the exclusive prefix sum of the slots' entry counts (a slot that
// does not exist counts 0), so slot_base[n_slots] is the call's total.  Entry j = slot_base[e] + t, t below the count of
// e: the order (b, k, t).  The caller's buffers hold max_entries entries: an entry with j >= max_entries is written
// nowhere, and the positions [min(total, max_entries), max_entries) past the last entry carry the sentinel.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GP_MAG_DET_HD __host__ __device__ inline
#else
#define GP_MAG_DET_HD inline
#endif

namespace gp_mag_det {

// The slot of entry j: the one e in [0, n_slots) with slot_base[e] <= j < slot_base[e + 1]; empty slots are passed over.
// n_slots for a j that is no entry (j < 0 or j >= the total).
GP_MAG_DET_HD long long slot_of(const long long* slot_base, long long n_slots, long long j)
{
    if (j < 0 || j >= slot_base[n_slots]) return n_slots;
    long long lo = 0, hi = n_slots;                       // slot_base[lo] <= j < slot_base[hi] throughout
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (slot_base[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// How many entries the buffers hold: the total, clamped at max_entries.
GP_MAG_DET_HD long long live_entries(long long total, long long max_entries)
{
    return total < max_entries ? total : max_entries;
}

// The tail [tail_begin, max_entries) takes the sentinel; it is empty when the entries fill the buffers or overflow them.
GP_MAG_DET_HD long long tail_begin(long long total, long long max_entries) { return live_entries(total, max_entries); }

// Whether the call overflowed: some entry has j >= max_entries.
GP_MAG_DET_HD bool overflowed(long long total, long long max_entries) { return total > max_entries; }

}  // namespace gp_mag_det
