// gfpush_dense.hpp -- the dense-LDS GFPush kernel for graphs that fit one workgroup (option "kernel" = 3; gfx950 / CDNA4).
//
// Cora (2 708 nodes) and Citeseer (3 327 nodes) are small enough that a row's WHOLE state -- the residues of this level and of
// the next, the reserve, one touched bit per node -- fits one workgroup's LDS as plain arrays indexed by node id (24 bytes per
// node; the layout is DensePlan, gfpush_plan.hpp).  So this kernel has no hash table, no push list, no reserve log and no
// per-workgroup scratch in HBM at all.  Like the other two kernels it runs persistent workgroups that pull rows from the device
// queue, and restates precompute/graph.h:73-127:
//
//   level i < n_coef-1   every node v with cur[v] != 0 is the frontier: reserve[v] += coef[i] * r (graph.h:90); a dangling node
//                        sends r to next[seed] and is NOT put to the push test (graph.h:91-93); otherwise r >= rmax * (double)deg
//                        decides -- the reference's fp64 expression, deg the indptr difference -- and r / (double)deg goes to
//                        every stored column of v, once per stored entry (graph.h:94-99); cur[v] is cleared in the same sweep,
//                        then the two arrays swap roles
//   last level           reserve[v] += coef[n_coef-1] * r only (graph.h:104-110)
//   TOP-K                an exact radix select over reserve[] among the values > 0 (graph.h:111-126), emitted by (value desc,
//                        column asc), every slot written once
//
// A level's work is balanced over EDGES: a wave takes 64 consecutive nodes and ballots the pushers.  A pusher of up to kDnSerial
// (8) edges walks them in its own lane -- a load and an add per edge, no cross-lane traffic; the citation graphs' mean degree is
// 4 to 5.  The larger pushers' degrees are prefix-summed in registers and all 64 lanes walk the concatenated edge range, each
// finding the owner of its edge by a six-step search over the 64 prefix values (cross-lane reads, no LDS list).  A 5 000-leaf
// hub is 79 steps of one wave, not one lane's serial loop.  (Measured, DESIGN.md section 7x: the shared walk for every pusher
// is 19 % slower on the Cora line; two or four 64-edge windows per step of the shared walk are slower still.)
// Adds into next[] are native fp64 LDS atomics: a node with one contribution holds exactly that quotient (0.0 + x == x), sums of
// several depend on arrival order in their last bits, as in the other kernels.
//
// Known difference: a residue that underflows to exactly 0.0 is "absent" here, while the reference keeps a map entry of value 0.
// That can only move `support` / `frontier`, and needs a chain of more than 80 levels on graphs this small.
#pragma once

#include "gfpush_kernels.hpp"

namespace gp {

// Control block of the dense kernel (at the start of dynamic LDS; kDenseCtlBytes of gfpush_plan.hpp are reserved for it).
struct DenseCtl {
    long long row;              // queue position pulled for the row in flight
    u32 lvl[3][2];              // per level, by level number mod 3: frontier nodes, edges.  Level i adds to slot i % 3, everyone reads it
                                // behind the level's barrier, and thread 0 then clears slot (i + 2) % 3 for the level after the next
    u32 tk_bin, tk_above, tk_count, tk_need;     // select: digit chosen this pass, members above it, members in it | slots the row fills
    u32 n_sel, pad;             // select: entries gathered so far
    u64 st[12];                 // statistics of this workgroup (Stat), flushed to p.counters once at the end
    double coef[kCoefLds];      // the first coefficients of the recipe
};
static_assert(sizeof(DenseCtl) <= 512, "the control block must fit its LDS reservation (kDenseCtlBytes)");

#ifndef GP_DN_SERIAL
#define GP_DN_SERIAL 8
#endif
constexpr u32 kDnSerial = GP_DN_SERIAL;               // a pusher of up to this many edges walks them in its own lane (0: every edge goes through the wave's shared walk)

struct DenseSel { u64 bits; u32 col; u32 pad; };      // 16 B: one selected (value, column) pair

// The select orders (value bits, ~column) as one 80-bit composite, largest first: positive doubles order as their bit patterns,
// ties go to the smaller column.  It is walked in ten 8-bit digits: eight of the value, two of ~column (node ids < 2^16 here).
__device__ __forceinline__ u32 dense_digit(u64 bits, u32 v, int pass) {
    return pass < 8 ? (u32)(bits >> (56 - 8 * pass)) & 255u : pass == 8 ? ((~v) >> 8) & 255u : (~v) & 255u;
}
// whether the composite's first `depth` digits equal those fixed so far (p_bits / p_lo hold them in place)
__device__ __forceinline__ bool dense_match(u64 bits, u32 v, int depth, u64 p_bits, u32 p_lo) {
    if (depth == 0) return true;
    if (depth <= 8) return (bits >> (64 - 8 * depth)) == (p_bits >> (64 - 8 * depth));
    return bits == p_bits && (((~v) >> 8) & 255u) == (p_lo >> 8);
}
// whether the composite's first `depth` digits are at or above the fixed ones: the row's selected set once the select has ended
__device__ __forceinline__ bool dense_selected(u64 bits, u32 v, int depth, u64 p_bits, u32 p_lo) {
    if (depth <= 8) return (bits >> (64 - 8 * depth)) >= (p_bits >> (64 - 8 * depth));
    const u32 lo = (~v) & 0xFFFFu;
    return bits > p_bits || (bits == p_bits && (depth == 9 ? (lo >> 8) >= (p_lo >> 8) : lo >= p_lo));
}

template <int BLOCK, bool STAGED>
__global__ void __launch_bounds__(BLOCK) gfpush_dense_kernel(const KParams)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    KP p = kparams();
    constexpr u32 W = BLOCK / 64;
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = wave_id();
    const u32 n = (u32)p.n_nodes, n_pad = p.dn_npad, n_chunks = n_pad >> 6;
    DenseCtl* ctl = (DenseCtl*)smem;
    u32* hist = (u32*)(smem + p.dn_hist);
    double* const arr0 = (double*)(smem + p.dn_cur);
    double* const arr1 = (double*)(smem + p.dn_next);
    double* resv = (double*)(smem + p.dn_reserve);
    u64* marks = (u64*)(smem + p.dn_marks);
    int* l_indptr = (int*)(smem + p.dn_indptr);
    int* l_indices = (int*)(smem + p.dn_indices);
    DenseSel* sel = (DenseSel*)(smem + p.dn_cur);           // TOP-K's list lives in cur | next, which are dead by then

    // ---- once per workgroup: everything a row assumes to be clear, the coefficients, the CSR when it is staged
    for (u32 i = tid; i < 3u * n_pad; i += BLOCK) arr0[i] = 0.0;             // cur | next | reserve are one run
    for (u32 i = tid; i < n_chunks; i += BLOCK) marks[i] = 0ull;
    if (tid < (u32)(sizeof(ctl->st) / sizeof(ctl->st[0]))) ctl->st[tid] = 0;
    if (tid < (u32)kCoefLds && (int)tid < p.n_coef) ctl->coef[tid] = p.coef[tid];
    if (STAGED) {
        for (u32 i = tid; i <= n; i += BLOCK) l_indptr[i] = p.indptr[i];
        for (u32 j = tid; j < (u32)p.nnz; j += BLOCK) l_indices[j] = (int)((u32)p.indices[j] & p.node_mask);
    }
    const long long n_rows = p.n_seeds;
    const int L = p.n_coef - 1;
    u32 max_e = 0;

    for (;;) {
        __syncthreads();                                     // the previous row's clean-up has ended
        if (tid == 0) {
            ctl->row = (long long)__hip_atomic_fetch_add(&p.counters[p.queue_counter], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int i = 0; i < 3; ++i) { ctl->lvl[i][0] = 0; ctl->lvl[i][1] = 0; }
            ctl->n_sel = 0;
        }
        __syncthreads();
        const long long qpos = uni(ctl->row);
        if (qpos >= n_rows) break;
        const long long row = p.row_map ? (long long)uni(p.row_map[qpos]) : qpos;
        const int seed = uni(p.seeds[row]);
        if (seed < 0 || seed >= p.n_nodes) {                 // the device API does not pre-validate seeds
            if (tid == 0) { ctl->st[sFailed] += 1; if (p.out_filled) p.out_filled[row] = 0; }
            continue;
        }

        // ---- the levels.  Counts of this wave for the row (wave-uniform), added to the control block when the row ends.
        u64 w_edges = 0; u32 w_front = 0, w_push = 0, w_supp = 0, n_levels = 0;
        double* cur = arr0; double* nxt = arr1;
        for (int i = 0; i <= L; ++i) {
            const bool last = i == L;
            const double c = i < kCoefLds ? ctl->coef[i] : p.coef[i];
            u32 lf = 0, my_edges = 0;                        // frontier nodes of this wave's chunks; edges pushed by this lane
            // level 0 is the seed alone (graph.h:81): its chunk, its lane, r = 1.0 without a store
            const u32 c_lo = i == 0 ? (u32)seed >> 6 : 0u, c_hi = i == 0 ? c_lo + 1u : n_chunks;
            for (u32 ch = c_lo + (wave + W - c_lo % W) % W; ch < c_hi; ch += W) {
                const u32 v = (ch << 6) + lane;
                const double r = i == 0 ? ((int)v == seed ? 1.0 : 0.0) : cur[v];
                const bool active = r != 0.0;
                const u64 am = __ballot(active);
                if (am == 0ull) continue;
                u32 deg = 0; int rel = 0; double share = 0.0;
                if (active) {
                    resv[v] = resv[v] + c * r;                               // graph.h:90 / :109
                    if (i != 0) cur[v] = 0.0;
                    if (!last) {
                        const int s0 = STAGED ? l_indptr[v] : p.indptr[v], s1 = STAGED ? l_indptr[v + 1] : p.indptr[v + 1];
                        const int d = s1 - s0;
                        if (d == 0) __hip_atomic_fetch_add(&nxt[seed], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // graph.h:91-93
                        else if (r >= p.rmax * (double)d) { deg = (u32)d; rel = s0; share = r / (double)d; }              // graph.h:94-95
                    }
                }
                if (lane == 0) { const u64 old = marks[ch]; marks[ch] = old | am; }
                lf += (u32)__popcll(am);
                if (last) continue;
                const u64 pm = __ballot(deg != 0u);
                if (pm == 0ull) continue;
                w_push += (u32)__popcll(pm); my_edges += deg;
                // a pusher of up to kDnSerial edges walks them itself: a load and an add per edge, no cross-lane traffic ...
                if (deg != 0u && deg <= kDnSerial) {
                    for (u32 j = 0; j < deg; ++j) {
                        const u32 col = STAGED ? (u32)l_indices[rel + (int)j] : (u32)p.indices[rel + (int)j] & p.node_mask;
                        __hip_atomic_fetch_add(&nxt[col], share, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);           // graph.h:96-99
                    }
                }
                // ... the edges of the larger ones are concatenated and walked by all 64 lanes: lane j owns [excl_j, incl_j) of the
                // run, edge e of it is column word rel_j + e
                const u32 big = deg > kDnSerial ? deg : 0u;
                if (__ballot(big != 0u) == 0ull) continue;
                const u32 incl = wave_incl_scan_dpp(big);
                const u32 total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
                rel -= (int)(incl - big);
                for (u32 base = 0; base < total; base += 64u) {
                    const u32 e = min(base + lane, total - 1u);
                    u32 lo = 0;                                              // the first lane whose inclusive sum exceeds e
#pragma unroll
                    for (u32 step = 32u; step > 0u; step >>= 1) {
                        const u32 t = (u32)__shfl((int)incl, (int)(lo + step - 1u));
                        if (t <= e) lo += step;
                    }
                    const int o_rel = __shfl(rel, (int)lo);
                    const double o_share = __shfl(share, (int)lo);
                    if (base + lane < total) {
                        const u32 col = STAGED ? (u32)l_indices[o_rel + (int)e] : (u32)p.indices[o_rel + (int)e] & p.node_mask;
                        __hip_atomic_fetch_add(&nxt[col], o_share, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);          // graph.h:96-99
                    }
                }
            }
            const u32 le = wave_sum32(my_edges);
            if (lane == 0 && (lf | le)) {
                __hip_atomic_fetch_add(&ctl->lvl[i % 3][0], lf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&ctl->lvl[i % 3][1], le, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            w_front += lf; w_edges += le;
            __syncthreads();
            const u32 f_all = uni(ctl->lvl[i % 3][0]), e_all = uni(ctl->lvl[i % 3][1]);
            if (tid == 0) { ctl->lvl[(i + 2) % 3][0] = 0; ctl->lvl[(i + 2) % 3][1] = 0; }
            if (f_all == 0u) break;                          // an empty frontier stays empty (both arrays are clear)
            ++n_levels; max_e = max(max_e, e_all);
            { double* t = cur; cur = nxt; nxt = t; }
        }
        // touched nodes of the row: the size of the reference's reserve map
        for (u32 ch = wave; ch < n_chunks; ch += W) w_supp += (u32)__popcll(uni(marks[ch]));

        // ---- TOP-K: the K-th largest composite among the values > 0, digit by digit
        u64 p_bits = 0; u32 p_lo = 0, need = 0, rem = 0; int depth = 0;
        for (int pass = 0; pass < 10; ++pass) {
            for (u32 i = tid; i < 256u; i += BLOCK) hist[i] = 0u;
            __syncthreads();
            for (u32 v = tid; v < n_pad; v += BLOCK) {
                const double x = resv[v];
                if (x > 0.0) {                                               // graph.h:121
                    const u64 bits = (u64)__double_as_longlong(x);
                    if (dense_match(bits, v, pass, p_bits, p_lo))
                        __hip_atomic_fetch_add(&hist[dense_digit(bits, v, pass)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            __syncthreads();
            if (wave == 0u) {                                // lane l holds bins 255 - 4 l .. 252 - 4 l: largest digits first
                u32 h[4], s = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { h[j] = hist[255u - 4u * lane - (u32)j]; s += h[j]; }
                const u32 incl = wave_incl_scan_dpp(s), excl = incl - s;
                const u32 total = (u32)__builtin_amdgcn_readlane((int)incl, 63);
                const u32 want = pass == 0 ? min((u32)p.K, total) : rem;
                if (lane == 0u && pass == 0) ctl->tk_need = want;
                if (want > 0u && excl < want && want <= incl) {
                    u32 a = excl;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (a < want && want <= a + h[j]) { ctl->tk_bin = 255u - 4u * lane - (u32)j; ctl->tk_above = a; ctl->tk_count = h[j]; }
                        a += h[j];
                    }
                }
            }
            __syncthreads();
            if (pass == 0) { need = uni(ctl->tk_need); rem = need; }
            if (need == 0u) break;
            const u32 bin = uni(ctl->tk_bin), cnt = uni(ctl->tk_count);
            rem -= uni(ctl->tk_above);
            if (pass < 8) p_bits |= (u64)bin << (56 - 8 * pass);
            else p_lo |= bin << (pass == 8 ? 8 : 0);
            depth = pass + 1;
            if (cnt == rem) break;                           // every member of the digit is taken: the set is known
        }
        // gather the selected pairs, rank them by (value desc, column asc), write slot `rank`: each slot once, none from `need` on
        if (need > 0u) {
            for (u32 v = tid; v < n_pad; v += BLOCK) {
                const double x = resv[v];
                if (x > 0.0) {
                    const u64 bits = (u64)__double_as_longlong(x);
                    if (dense_selected(bits, v, depth, p_bits, p_lo)) {
                        const u32 at = __hip_atomic_fetch_add(&ctl->n_sel, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (at < need) { sel[at].bits = bits; sel[at].col = v; }
                    }
                }
            }
        }
        __syncthreads();
        const long long out0 = row * (long long)p.K;
        for (u32 i = tid; i < need; i += BLOCK) {
            const u64 my = sel[i].bits; const u32 my_col = sel[i].col;
            u32 rank = 0;
            for (u32 j = 0; j < need; ++j) {
                const u64 o = sel[j].bits; const u32 o_col = sel[j].col;
                rank += (u32)(o > my || (o == my && o_col < my_col));
            }
            p.out_row[out0 + rank] = seed; p.out_col[out0 + rank] = (int)my_col; p.out_val[out0 + rank] = __longlong_as_double((long long)my);
        }
        // ---- the state the next row assumes: reserve and marks of what was touched (cur and next are clear behind the last level) ...
        for (u32 ch = wave; ch < n_chunks; ch += W) {
            const u64 m = uni(marks[ch]);
            if (m == 0ull) continue;
            if ((m >> lane) & 1ull) resv[(ch << 6) + lane] = 0.0;
            if (lane == 0u) marks[ch] = 0ull;
        }
        if (lane == 0u) {
            if (w_push) __hip_atomic_fetch_add(&ctl->st[sPush], (u64)w_push, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (w_edges) __hip_atomic_fetch_add(&ctl->st[sEdges], w_edges, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (w_front) __hip_atomic_fetch_add(&ctl->st[sFront], (u64)w_front, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (w_supp) __hip_atomic_fetch_add(&ctl->st[sSupport], (u64)w_supp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (tid == 0u) {
                __hip_atomic_fetch_add(&ctl->st[sFilled], (u64)need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&ctl->st[sLds], (u64)n_levels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        // ... and the list's bytes in cur | next
        for (u32 i = tid; i < 2u * need; i += BLOCK) arr0[i] = 0.0;
        publish_filled(p, row, need);
    }

    // flush statistics: one atomic per counter per workgroup
    __syncthreads();
    if (tid == 0) {
        const Counter dst[sNumStats] = { kPushes, kEdges, kFrontier, kDegLookups, kFilled, kSupport, kLdsLevels, kGlobalLevels, kFailedRows };
#pragma unroll
        for (int i = 0; i < sNumStats; ++i)
            if (ctl->st[i]) __hip_atomic_fetch_add(&p.counters[dst[i]], ctl->st[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (max_e) __hip_atomic_fetch_max(&p.counters[kMaxLevelEdges], (u64)max_e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace gp
