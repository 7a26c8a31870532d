// optim_defer_layout.hpp -- the bookkeeping of the embedding table's deferred exact Adam step, HIP-free: the
// standard library alone, so that tests/native/optim_defer_check.cpp holds the very lines the kernels of optim_defer.hip
// run, on the CPU and under the sanitizers.
//
// Under dense Adam a row no batch touches still takes the zero-gradient update of every step.  Here that update is put
// off: last[r] is the step row r is current through, and the three per-step numbers the update needs -- step_size,
// rsqrt_bc2 and the clip coefficient -- are kept for every step in a ring of `capacity` entries, entry of step s in slot
// s % capacity under the tag s.  Replaying the steps last[r] + 1 .. through in order, each with its own entry, gives the
// row the bits the dense step would have given it.
//
// THE SERVED GAP.  T is the step state's tick.  The step kernel of step T writes slot T % capacity while other workgroups
// of the same launch replay the steps up to T - 1, so the oldest step a launch at tick T may read is T - capacity + 1
// (slot (T + 1) % capacity): a row is served when T - last[r] <= capacity, in all three kernels -- the pre-forward catch-up
// (through = T - 1), the step (through = T - 1, then the step itself) and the flush (through = T).  A row one step past
// that is UNSERVED: bit kFlagBit of the flag word is set and the row keeps its bits and its last[r].  So is a row whose
// last[r] is negative or ahead of the tick, any row once the tick no longer fits last's 32 bits, and a row for which some
// slot of the replay does not carry the tag of the step it should hold.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GP_OPTIM_DEFER_HD __host__ __device__ inline
#else
#define GP_OPTIM_DEFER_HD inline
#endif

namespace gp_optim_defer {

constexpr int kMinCapacity = 4;
constexpr int kMaxCapacity = 65536;
constexpr int kFlagBit = 2;               // bit 1 of the step's flag word (bit 0: a list or key buffer overflowed)

// One step of history, 16 bytes: what adam_element needs besides the element and the group's constants.
struct alignas(16) Entry {
    float step_size, rsqrt_bc2, coef;
    uint32_t tag;                         // the low 32 bits of the step the entry belongs to
};
static_assert(sizeof(Entry) == 16, "a ring entry is one 16-byte store");

enum Plan { kNothing = 0, kReplay = 1, kUnserved = 2 };

GP_OPTIM_DEFER_HD bool valid_capacity(long long capacity)
{
    return capacity >= kMinCapacity && capacity <= kMaxCapacity && (capacity & (capacity - 1)) == 0;
}

GP_OPTIM_DEFER_HD uint32_t slot(long long step, int capacity) { return (uint32_t)step & (uint32_t)(capacity - 1); }
GP_OPTIM_DEFER_HD uint32_t tag(long long step) { return (uint32_t)step; }

// What a row that is current through `last` needs to be current through `through` (T - 1 or T) at tick T.
GP_OPTIM_DEFER_HD Plan plan(unsigned long long tick, long long last, long long through, int capacity)
{
    if (tick > (unsigned long long)INT32_MAX) return kUnserved;
    const long long T = (long long)tick;
    if (last < 0 || last > T) return kUnserved;
    if (last >= through) return kNothing;
    return T - last <= capacity ? kReplay : kUnserved;
}

// Whether a ring entry is the one of `step`.
GP_OPTIM_DEFER_HD bool tag_ok(const Entry& e, long long step) { return e.tag == tag(step); }

// Whether every step of (last, through] stands in the ring under its own tag.  To be called for a kReplay row.  (The kernels
// ask tag_ok of 64 steps at a time, a lane each.)
GP_OPTIM_DEFER_HD bool tags_ok(const Entry* hist, long long last, long long through, int capacity)
{
    for (long long s = last + 1; s <= through; ++s)
        if (!tag_ok(hist[slot(s, capacity)], s)) return false;
    return true;
}

}  // namespace gp_optim_defer
