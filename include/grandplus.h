/*
 * grandplus.h -- C ABI of the MI355X-native GFPush propagation-matrix precompute.
 *
 * This is the drop-in boundary for the ONE hot path of THUDM/GRAND-plus: the pybind11
 * class `propagation.Graph` (reference precompute/propagation.cpp:8-12) whose two
 * members are `Graph(indptr, indices, seed)` (precompute/graph.h:32-47) and
 * `gfpush_omp(node_idx, row_idx, col_idx, value, coef, rmax, K)`
 * (precompute/graph.h:53-131).  Every entry point takes plain pointers and sizes; no
 * torch / pybind11 / HIP types appear in a signature (streams travel as void*).
 *
 * Implemented by grand_plus_amd/libgrandplus.so (grand_plus_amd/csrc/gfpush.hip, hand-written
 * HIP for gfx950).  There is no CPU fallback: without a usable GPU gp_graph_create
 * returns GP_ERR_NO_DEVICE.
 */
#ifndef GRANDPLUS_H
#define GRANDPLUS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GP_ABI_VERSION 4

/* Status codes (0 = success).  The Python / pybind11 shims map INVALID_* to
 * ValueError, NO_DEVICE / HIP / OVERFLOW to RuntimeError, NOMEM to MemoryError. */
enum {
    GP_OK                = 0,
    GP_ERR_NULL          = 1,   /* a required pointer is NULL                                   */
    GP_ERR_INVALID_CSR   = 2,   /* indptr not monotone / indptr[0]!=0 / indptr[n]!=nnz / column out of range */
    GP_ERR_INVALID_SEED  = 3,   /* a seed id is outside [0, n_nodes)                            */
    GP_ERR_INVALID_ARG   = 4,   /* K < 1, K > GP_MAX_K, n_coef < 1, non-finite coef/rmax, rmax < 0, negative size */
    GP_ERR_NO_DEVICE     = 5,   /* no HIP device / device index out of range                    */
    GP_ERR_HIP           = 6,   /* a HIP runtime call failed (see gp_last_error)                */
    GP_ERR_NOMEM         = 7,   /* device or host allocation failed                             */
    GP_ERR_OVERFLOW      = 8    /* a row exceeded a workspace bound (never expected; rows are not silently wrong) */
};

#define GP_MAX_K 1024

typedef struct gp_graph gp_graph;   /* opaque: CSR resident in one GPU's HBM + workspaces */

/* Counters accumulated over the gfpush calls on a graph since the last gp_reset_stats
 * (gp_gfpush resets them itself, so after it they describe that one call).  All exact. */
typedef struct gp_stats {
    int64_t rows;            /* seeds processed                                                  */
    int64_t pushes;          /* P: (node, level) pushes        -- graph.h:94 branch taken        */
    int64_t edges;           /* E: sum of deg over the pushes  -- graph.h:96-99 iterations       */
    int64_t filled;          /* output slots written (v > 0)   -- graph.h:121                    */
    int64_t support;         /* sum over rows of reserve-map size -- graph.h:111 (exact with option exact_stats=1) */
    int64_t frontier;        /* sum over rows and levels of frontier size                        */
    int64_t lds_levels;      /* levels whose residue table lived in LDS                          */
    int64_t global_levels;   /* levels whose residue table lived in the per-workgroup HBM table  */
    int64_t failed_rows;     /* rows that hit a workspace bound (=> GP_ERR_OVERFLOW)             */
    int64_t degree_lookups;  /* frontier nodes whose degree (two indptr words) had to be read    */
    double  kernel_ms;       /* HIP-event time of the LAST gfpush kernel on its stream           */
    int32_t workgroups;      /* persistent workgroups launched                                   */
    int32_t block_threads;   /* threads per workgroup                                            */
    int32_t lds_bytes;       /* dynamic LDS per workgroup                                        */
    int32_t lds_slots;       /* residue-table slots that fit in that LDS                         */
    int64_t workspace_bytes; /* HBM scratch held for this configuration                          */
    /* Filled only by the diagnostic build (libgrandplus_diag.so, -DGP_DIAG): 100 MHz ticks
     * spent per phase, summed over workgroups.  Always 0 in the product library. */
    int64_t diag_ticks_scan, diag_ticks_expand, diag_ticks_topk, diag_ticks_total;
    int64_t diag_ticks_scan_hbm, diag_ticks_expand_hbm;   /* the part of scan/expand spent on HBM-table levels */
    int64_t diag_sub[16];    /* free-form sub-phase ticks / counts of the diagnostic build          */
    /* In the product library the slots count what is rare instead: [1..7] rows the sketch kernel handed back, by reason;
     * [8] LDS level tables that overflowed (an insert probed 24 slots) and were wiped and re-streamed / split in two -- both
     * kernels; [9] one-wave levels that undid their claims -- both kernels; [10] doublings of the partitions of the sketch
     * kernel's TOP-K aggregation after an overflow.  [0], [11..15] stay 0.  Each is counted on the branch that recovers. */
    /* ABI 2: workspace policy.  Every workgroup's scratch slab is sized from an estimate; rows that outgrow it are
     * re-run by a second launch on a few workgroups whose slabs are sized from the rigorous 1/rmax bounds. */
    int64_t retried_rows;    /* rows that took that second launch (they are complete and exact, just slower) */
    int64_t max_level_edges; /* largest number of edges one level of one row traversed                       */
    int64_t max_log_records; /* largest number of reserve-log records (sum over levels of frontier size) of one row */
    /* ABI 3: which kernel ran the rows.  2 = the sketch-filtered kernel (csrc/gfpush_sketch.hpp: keyless fixed-point upper
     * bounds decide which targets get an exact fp64 accumulator; `frontier` and `support` are not counted by it and stay 0,
     * its log holds one record per pushed edge, so max_log_records counts edges), 1 = the general kernel
     * (csrc/gfpush_kernels.hpp), which also re-runs the rows the sketch kernel hands back (retried_rows).  3 = the dense-LDS
     * kernel (csrc/gfpush_dense.hpp, option "kernel" = 3): pushes, edges, filled, frontier and support (the sum over rows of the
     * nodes a row touched: the size of the reference's reserve map) are always exact, lds_levels counts the levels it swept,
     * max_level_edges is the real maximum; global_levels, retried_rows, degree_lookups, max_log_records, workspace_bytes,
     * lds_slots and the sketch fields stay 0; lds_bytes is what its layout needs, not the whole CU's. */
    int32_t kernel;
    int32_t sketch_pad;
    int64_t sketch_candidate_edges;  /* pushed edges whose target might push and went into the exact table (of `edges`) */
    int64_t sketch_second_sweeps;    /* rows whose top-K needed a second sweep over their log                          */
    /* ABI 4: the measured choice.  With nothing forced (options kernel / block_threads / lds_bytes all 0, "measure_choice" 1) the
     * first call of >= 32 768 rows of a recipe (rmax, n_coef, K) on a graph times its candidates -- they are exact and
     * interchangeable -- on its first 16 384 rows (into scratch outputs), and every later call of that recipe, of any size, runs what the rmax / graph-size thresholds
     * pick unless another candidate was more than 5 % faster: [0] the general kernel in the launch shape the thresholds pick,
     * [1] the sketch kernel, [2] the general kernel in the other shape.
     * Milliseconds of those timing runs behind the LAST call's decision (0 = not a candidate / nothing was measured for it);
     * `kernel`, `block_threads`, `lds_bytes` say what ran. */
    float   choice_ms[3];
    int32_t choice_pad;
} gp_stats;

/* ABI / build information. */
int         gp_abi_version(void);
const char* gp_strerror(int status);
const char* gp_last_error(void);          /* thread-local detail of the last failure ("" if none) */
int         gp_device_count(void);        /* number of visible HIP devices (0 if none)           */

/*
 * Replaces Graph::Graph (graph.h:32-47).  Validates the CSR (the reference does not), copies
 * indptr/indices to `device`'s HBM (the reference borrows the caller's buffers: graph.h:35-36;
 * here the caller may free them after the call) and derives degrees on the fly from indptr
 * (graph.h:42-45).  The reference's unused `seed` argument (graph.h:40) is accepted by the
 * shims and dropped before this call.
 * indptr is checked on the host (O(N)); the column ids are checked on the DEVICE behind the upload (range; and whether
 * every row is strictly increasing, which only decides a shortcut): GP_ERR_INVALID_CSR either way, before the handle exists.
 * Arrays of >= 64 MB are uploaded through four 16 MB pinned staging buffers filled by two helper threads, joined before
 * the call returns.
 */
int gp_graph_create(const int32_t* indptr, int64_t n_nodes,
                    const int32_t* indices, int64_t nnz,
                    int device, gp_graph** out);

/*
 * Multi-GPU form of the same constructor: ONE process, ONE call, every GPU of the node.
 * n_gpus = 0 means all visible devices.  The CSR is uploaded to GPU 0; the other GPUs receive their replica by a
 * device-to-device copy the first time a gp_gfpush call is large enough to be sharded (>= "min_rows_per_gpu" rows per
 * GPU, default 2048; smaller calls run on GPU 0 alone).  gp_gfpush on such a handle cuts the seeds into contiguous
 * blocks of ceil(S / n_gpus) rows, runs every block on its GPU from its own host thread and stream, reassembles the
 * sparse row matrix with ONE ncclAllGather (RCCL over xGMI) of the packed per-GPU slabs
 * [value f64 | row i32 | col i32 | filled i32], copies it to the host once from GPU 0 and writes the v > 0 slots into
 * the caller's arrays (graph.h:117-126).  RCCL is opened with dlopen the first time it is needed.
 * gp_gfpush_device is refused on a multi-GPU handle (device buffers live on one GPU).  Extra options of such a handle:
 *   "min_rows_per_gpu"  sharding threshold (default 2048)
 *   "gather_host"       1 = no collective: every GPU copies its own slab to the host (measured comparison)
 *   "force_collective"  1 = take the sharded path, all-gather included, even for small calls / one GPU (tests)
 * every other option is forwarded to the per-GPU graphs.  gp_get_stats returns the sums over the GPUs of the last call
 * (kernel_ms = the slowest GPU).
 */
int gp_graph_create_multi(const int32_t* indptr, int64_t n_nodes,
                          const int32_t* indices, int64_t nnz,
                          int n_gpus, gp_graph** out);
/* The same constructor over an explicit list of devices.  A device may appear more than once: the handle then holds several
 * parts -- each with its own replica of the CSR, stream, workspace and host thread -- on that one GPU and gathers the slabs
 * through the host (RCCL takes one rank per device; "gather_host" cannot be switched off on such a handle).  This is how a box
 * with a single GPU runs the whole sharded path of gp_gfpush; it is not a way to go faster. */
int gp_graph_create_multi_on(const int32_t* indptr, int64_t n_nodes,
                             const int32_t* indices, int64_t nnz,
                             const int* devices, int n_parts, gp_graph** out);
int gp_graph_num_gpus(const gp_graph* g);

void gp_graph_destroy(gp_graph* g);

int64_t gp_graph_num_nodes(const gp_graph* g);
int64_t gp_graph_nnz(const gp_graph* g);
int     gp_graph_device(const gp_graph* g);

/*
 * Replaces Graph::gfpush_omp (graph.h:53-131) with HOST buffers, exactly as the pybind11
 * surface hands them over: seeds int32[S]; row_idx/col_idx int32[S*K], value f64[S*K]
 * caller-allocated and written IN PLACE at slot it*K+i (graph.h:120); only slots with
 * v > 0 are written (graph.h:121), everything else keeps the caller's contents.  Within a row
 * the filled slots are i = 0..filled-1 ordered by (value desc, column asc) -- the reference
 * leaves that order unspecified (nth_element, graph.h:115).  Synchronous.  The calling thread merges
 * finished rows into the caller's arrays while the kernels run; one helper thread, joined before the
 * call returns, resets the pinned slab the next call will use.  No OpenMP, no process-wide settings: the one
 * thing the call touches outside its own memory is the CALLING THREAD's timer slack (prctl PR_SET_TIMERSLACK,
 * 1 us while it waits for rows in 60 us sleeps; put back before the call returns).
 */
int gp_gfpush(gp_graph* g,
              const int32_t* seeds, int64_t n_seeds,
              const double* coef, int n_coef, double rmax, int K,
              int32_t* row_idx, int32_t* col_idx, double* value);

/*
 * Same computation with DEVICE buffers on g's GPU, enqueued on `stream` (a hipStream_t
 * passed as void*; NULL = the default stream) and NOT synchronised: the form bench.py and
 * the multi-GPU driver use (inputs already resident in HBM, RCCL all-gather consumes the
 * outputs on device).  d_row/d_col/d_val are [S*K]; slots i >= d_filled[it] of a row are left
 * untouched.  d_filled is int32[S] (may be NULL).  coef is a HOST array (n_coef doubles).
 * ONE-OFF SYNCHRONOUS CALLS: the first call that takes the sketch kernel builds the self-addressed CSR (one stream
 * synchronisation), and the first call of >= 32 768 rows of a recipe times its candidates first (gp_stats.choice_ms: six
 * launches of 16 384 rows into scratch output buffers of the library's own -- never into d_row/d_col/d_val -- and two stream
 * synchronisations).  Every other call only enqueues.  Option "measure_choice" = 0 avoids the second.
 */
int gp_gfpush_device(gp_graph* g,
                     const int32_t* d_seeds, int64_t n_seeds,
                     const double* coef, int n_coef, double rmax, int K,
                     int32_t* d_row, int32_t* d_col, double* d_val, int32_t* d_filled,
                     void* stream);

/* Waits for the last gfpush on g and returns the counters (GP_ERR_OVERFLOW if a row failed). */
int gp_get_stats(gp_graph* g, gp_stats* out);

/* Zeroes the counters at the next gfpush call. */
int gp_reset_stats(gp_graph* g);

/*
 * Tuning knobs (all optional; defaults are chosen for MI355X):
 *   "block_threads"   256 | 512 | 1024      threads per persistent workgroup
 *   "lds_bytes"       dynamic LDS per workgroup (<= 163840)
 *   "max_workgroups"  upper bound on persistent workgroups (0 = CUs x resident blocks)
 *   "workspace_mb"    HBM scratch budget in MiB (default 65536, never more than 90 % of the free device memory).
 *                      Under pressure the per-workgroup slabs shrink, not the number of workgroups; rows that
 *                      outgrow their slab are re-run on a few workgroups with worst-case slabs (gp_stats.retried_rows)
 *   "est_level_edges" edges per level the per-workgroup slabs are sized for (0 = automatic: max(32768, bound/4),
 *                      grown from the observed maxima of earlier calls)
 *   "force_global"    1 = never use the LDS residue table (testing the HBM-table path)
 *   "max_degree_bits" cap on the spare column-id bits used to carry degrees (0 = none; testing the
 *                      path taken by graphs with N >= 2^29); only before the first gfpush call
 *   "exact_stats"     1 = always aggregate the whole reserve map, so that gp_stats.support is the
 *                      exact sum of reserve-map sizes (default 0: nodes that provably cannot
 *                      reach the top-K are never tabled and `support` counts only tabled nodes)
 *   "direct_tables"   0 = never index the level tables by node id (default 1: graphs with N <= table slots of the
 *                      512-thread kernel -- Cora, Citeseer -- skip hashing altogether)
 *   "seedrow"         0 = level 1 of a row goes through EXPAND and a hash table like every other level (default 1: on graphs
 *                      whose CSR rows hold strictly increasing column ids the seed's neighbour list IS level 1's frontier)
 *   "solo_levels"     0 = levels of <= 256 edges go through EXPAND + SCAN of the whole workgroup (default 1: one wave does such a
 *                      level start to finish, the others park at one barrier)
 *   "kernel"          0 = choose per call (default), 1 = always the general kernel, 2 = the sketch-filtered kernel whenever
 *                      the call allows it (all coef >= 0, at most 40 levels, K <= 128, rmax > 0).  Automatic choice: the
 *                      sketch kernel for rmax >= 5e-6 on graphs of >= 65 536 nodes.
 *                      3 = the dense-LDS kernel on graphs of up to 6 720 nodes (Cora, Citeseer): a row's residues, reserve and
 *                      touched marks are plain fp64 arrays indexed by node id in one workgroup's LDS -- no hash table, no push
 *                      list, no reserve log, no workspace.  Any coef, n_coef >= 1, K <= 1024, rmax >= 0.  Opt-in: the
 *                      automatic choice never picks it and it is never calibrated.  On a call it cannot take (a larger
 *                      graph, "lds_pad" leaving no room for its state) kernel = 3 runs what kernel = 0 would; gp_stats.kernel
 *                      says which kernel ran, and that is not an error.  Same contract as the other kernels: slots
 *                      0..filled-1 by (value desc, column asc), last bits of sums depend on the order of the adds
 *   "dn_block_threads" / "dn_csr_lds"   the dense kernel's shape: 0 (default: 512) | 256 | 512 | 1024 threads per workgroup;
 *                      1 = indptr + indices are staged into LDS once per workgroup when they fit beside the row state (default
 *                      0: the CSR is read from memory -- staging costs a workgroup per CU and measured slower)
 *   "sk_block_threads" / "sk_lg_mu" / "sk_lg_mr" / "sk_target"   geometry of the sketch kernel (0 = default): threads per
 *                      workgroup (512 = three per CU with 52 KB, 768 = two with 80 KB, 1024 = one with 160 KB: measurements
 *                      only), log2 cells of the level sketch and of the reserve sketch, cell rank of the first TOP-K
 *                      threshold (default 4 K)
 *   "gk_acsr"         0 = the general kernel always runs on the packed CSR + indptr (default 1: on graphs of >= 65 536 nodes
 *                      it runs on the self-addressed copy -- rows at 128-byte units, a pusher's row start and degree in
 *                      its key -- like the sketch kernel)
 *   "row_order"       0 = the first launch of a call takes its rows in caller order (default 1: heaviest first -- a pre-pass of
 *                      two small kernels classes every row by the edges of its levels 1 and 2, read off its seed's columns, and
 *                      the row queue hands the classes out in descending order, so that no long row is drawn last and holds the
 *                      launch open; calls of no more rows than workgroups skip it).  Results, `filled` and the statistics do
 *                      not depend on it: everything stays indexed by row
 *   "verify_merge"    1 = gp_gfpush (host buffers) compares every row it merged while the kernel was running with the pinned
 *                      slab once the launches have retired and fails with GP_ERR_HIP if one differs (a debugging aid: the
 *                      merge rule relies on stores to host memory arriving whole; default 0)
 *   "diag_flags"      ignored by the product library; the diagnostic build (-DGP_DIAG) skips phases for
 *                      instruction attribution (bit 0: TOP-K) -- its results are then meaningless
 * Returns GP_ERR_INVALID_ARG for an unknown key or an out-of-range value.
 */
int gp_set_option(gp_graph* g, const char* key, int64_t value);

/* ------------------------------------------------------------------------------------------
 * Next row of the scope table: GRAND+'s feature augmentation
 * ("random propagation"), reference Grand_Plus.random_prop (model.py:80-87, model_mag.py:80-86):
 * DropNode on the scores, weighted segment-sum of neighbour features, divide by
 * (sum of kept scores + 1e-12).  fp32 like the reference.  All pointers are DEVICE pointers on
 * `device`; the launch is asynchronous on `stream`.
 *
 * `training` != 0 applies dropout with rate `dropnode_rate`: kept scores are scaled by
 * 1/(1-rate) (model.py:82).  The keep decision of entry e is d_keep[e] != 0 when d_keep is
 * given (parity tests), otherwise a counter-based RNG of (seed, e) -- change `seed` every call.
 * ------------------------------------------------------------------------------------------ */

/* Fused form: consumes the [S x K] rows gfpush left on the device.  Output row b is built from
 * matrix row r = d_batch_rows[b] (r = b when d_batch_rows is NULL), using its first d_filled[r]
 * slots (all K when d_filled is NULL): out[b,:] = sum_k w_k X[col[r,k],:] / (sum_k w_k + 1e-12),
 * w_k = (float)val[r,k] * keep_k/(1-rate).  Replaces the caller-side slicing, feature gather and
 * upload of model.py:310-316 together with random_prop itself.  d_x is X[n_nodes x feat_dim]. */
int gp_random_prop_rows(int device, const float* d_x, int64_t n_nodes, int32_t feat_dim,
                        const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                        const int32_t* d_batch_rows, int32_t n_batch,
                        float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                        float* d_out, void* stream);

/* SURVEY.md 8f next-3 -- where is the row of node v?  The reference slices `topk_adj[batch_index]` on the CPU every step
 * (model.py:310); here the seed list leaves a device-resident index once per precompute and a batch of node ids is turned into
 * row positions by one small kernel, no host work per element.
 * gp_seed_positions: d_pos_of_node int32[n_nodes] <- first position of every seed of d_seeds[n_seeds] (a duplicated seed keeps
 * its first), -1 for nodes that are no seed; *d_n_bad (device int32) <- seeds outside [0, n_nodes).
 * gp_batch_positions: d_out[i] <- d_pos_of_node[d_node_ids[i]] (int64 ids, as torch index tensors are), -1 for an id that is no
 * seed or out of range; *d_n_missing (device int32) <- how many of those.  Both are enqueued on `stream`. */
int gp_seed_positions(int device, const int32_t* d_seeds, int64_t n_seeds, int64_t n_nodes, int32_t* d_pos_of_node, int32_t* d_n_bad, void* stream);
int gp_batch_positions(int device, const int32_t* d_pos_of_node, int64_t n_nodes, const int64_t* d_node_ids, int64_t n,
                       int32_t* d_out, int32_t* d_n_missing, void* stream);

/* Reference-shaped form: feats[n_entries x feat_dim] already gathered, scores[n_entries],
 * idx[n_entries] sorted ascending (the row-major order of scipy's .nonzero(), model.py:312);
 * out[n_out x feat_dim] with n_out = idx[-1] + 1 (model.py:84). */
int gp_random_prop_coo(int device, const float* d_feats, int64_t n_entries, int32_t feat_dim,
                       const float* d_scores, const int64_t* d_idx, int64_t n_out,
                       float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                       float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward of random_prop and MAG's embedding-bag layer.  All pointers are DEVICE
 * pointers on `device`; launches are asynchronous on `stream`; arguments are checked before
 * the device is touched.  (dropnode_rate / dropout_rate, training, seed, d_keep) mean what they
 * mean for the forward entries above: pass the forward's values and the backward applies the
 * forward's mask (recomputed from (seed, entry), never stored).
 *
 * Gradients flow to the feature operand only; scores and attr_data are constants.
 * ------------------------------------------------------------------------------------------ */

/* d_grad_feats[e,:] = w'_e / (den_b + 1e-12) * d_grad_out[b,:], b = d_idx[e]: every row of
 * d_grad_feats[n_entries x feat_dim] is written (dropped entries get zeros).  No atomics. */
int gp_random_prop_coo_backward(int device, const float* d_grad_out, int64_t n_out, int32_t feat_dim,
                                const float* d_scores, const int64_t* d_idx, int64_t n_entries,
                                float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                                float* d_grad_feats, void* stream);

/* d_grad_x[col[r,k],:] += w'_{r,k} / (den_b + 1e-12) * d_grad_out[b,:], r = d_batch_rows[b], into a
 * caller-zeroed d_grad_x[n_nodes x feat_dim].  fp32 global atomics: not bitwise reproducible unless `deterministic=True`
 * (Python), which calls gp_random_prop_rows_backward_det of grandplus_scatter.h in its place.
 * Column ids outside [0, n_nodes) are skipped. */
int gp_random_prop_rows_backward(int device, const float* d_grad_out, int32_t n_batch, int32_t feat_dim,
                                 const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                                 const int32_t* d_batch_rows, float dropnode_rate, int training, uint64_t seed,
                                 const uint8_t* d_keep, float* d_grad_x, int64_t n_nodes, void* stream);

/* Embedding-bag, reference MLP.emb (model_mag.py:48-55), table W[n_vocab x dim] fp32:
 *   out[m,:] = sum_j keep_{j,:}/(1-rate) * d_j * W[a_j,:] / (sum_j d_j + 1e-10)
 * The bag of row m is storage entries [d_offsets[src], d_offsets[src+1]) of d_attr_idx (int32 when
 * idx_bytes = 4, int64 when 8) and d_attr_data, with src = d_nodes[m] when d_nodes is given (rows of a
 * device-resident node-attribute CSR with n_src rows), else src = m.  The entry's position j in the
 * batch's entry order is d_entry_base[m] + t when d_entry_base is given, else its storage position; the
 * dropout of element (j, h) is d_keep[j*dim + h] or the RNG of (seed, j*dim + h).  The denominator
 * uses the raw d_attr_data.  Attribute ids outside [0, n_vocab) and src outside [0, n_src) are never
 * read; *d_n_bad (device int32, optional) is set to how many there were.  fp32 sums. */
int gp_embedding_bag(int device, const float* d_weight, int64_t n_vocab, int32_t dim,
                     const int64_t* d_offsets, int64_t n_src, const int64_t* d_nodes, const int64_t* d_entry_base, int64_t n_rows,
                     const void* d_attr_idx, int idx_bytes, const float* d_attr_data,
                     float dropout_rate, int training, uint64_t seed, const uint8_t* d_keep,
                     float* d_out, int32_t* d_n_bad, void* stream);

/* Its backward into a dense, caller-zeroed d_grad_weight[n_vocab x dim] (nn.Embedding(sparse=False)):
 *   dW[a_j,:] += keep_{j,:}/(1-rate) * d_j / (den_m + 1e-10) * d_grad_out[m,:]
 * Same bag layout and counter as gp_embedding_bag; out-of-range ids are never written.  fp32 global
 * atomics (one 256-B wave-instruction per entry at dim = 64): not bitwise reproducible unless `deterministic=True`
 * (Python), which calls gp_embedding_bag_backward_det of grandplus_scatter.h in its place. */
int gp_embedding_bag_backward(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                              const int64_t* d_offsets, int64_t n_src, const int64_t* d_nodes, const int64_t* d_entry_base, int64_t n_rows,
                              const void* d_attr_idx, int idx_bytes, const float* d_attr_data,
                              float dropout_rate, int training, uint64_t seed, const uint8_t* d_keep,
                              float* d_grad_weight, int32_t* d_n_bad, void* stream);

/* ------------------------------------------------------------------------------------------
 * S-sample random_prop: the `--sample S` augmentations of one training step
 * (model.py:321-322) in one launch, 1 <= n_samples <= 16 (anything else: GP_ERR_INVALID_ARG).
 * d_out is [S x n_out x feat_dim], sample-major: out[s] is the [n_out x feat_dim] block the
 * single-sample entry above returns, bit for bit, when called with seed_s (or with mask row s):
 *
 *     seed_0 = seed
 *     seed_s = mix(seed ^ (s * 0xD6E8FEB86659FD93)),  s >= 1,   all arithmetic mod 2^64, where
 *     mix(x) : x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *              x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  return x ^ (x >> 31)
 *
 * (grand_plus_amd.augment.sample_seed mirrors it.)  An explicit mask d_keep is uint8 [S x L]: row s
 * is the d_keep the single-sample call takes; L = keep_stride for the fused form (>= the largest
 * r*K + K used, normally the length of d_col) and n_entries for the COO form.  Each neighbour
 * feature row is read once per chunk of up to 8 samples: for S <= 8 the HBM bound is
 * 4 F (entries + S n_out) + (4 + 4 S) entries bytes (a second feature pass for S > 8).
 * ------------------------------------------------------------------------------------------ */
int gp_random_prop_rows_multi(int device, const float* d_x, int64_t n_nodes, int32_t feat_dim,
                              const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                              const int32_t* d_batch_rows, int32_t n_batch, int32_t n_samples,
                              float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep, int64_t keep_stride,
                              float* d_out, void* stream);

/* n_out is the caller's (idx[-1] + 1 when it wants the reference's shape; passing it saves the host read). */
int gp_random_prop_coo_multi(int device, const float* d_feats, int64_t n_entries, int32_t feat_dim,
                             const float* d_scores, const int64_t* d_idx, int64_t n_out, int32_t n_samples,
                             float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                             float* d_out, void* stream);

/* d_grad_feats[e,:] = sum_s w'_{s,e} / (den_{s,b} + 1e-12) * d_grad_out[s,b,:], b = d_idx[e], summed over s in order:
 * every row is written, no atomics, bitwise reproducible. */
int gp_random_prop_coo_multi_backward(int device, const float* d_grad_out, int64_t n_out, int32_t feat_dim,
                                      const float* d_scores, const int64_t* d_idx, int64_t n_entries, int32_t n_samples,
                                      float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                                      float* d_grad_feats, void* stream);

/* d_grad_x[col[r,k],:] += sum_s w'_{s,r,k} / (den_{s,b} + 1e-12) * d_grad_out[s,b,:] into a caller-zeroed d_grad_x: the
 * samples are summed in registers, then one fp32 atomic per element and entry (per chunk of samples when K > 962).
 * Not bitwise reproducible unless `deterministic=True` (Python: gp_random_prop_rows_backward_det, grandplus_scatter.h). */
int gp_random_prop_rows_multi_backward(int device, const float* d_grad_out, int32_t n_batch, int32_t feat_dim,
                                       const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                                       const int32_t* d_batch_rows, int32_t n_samples, float dropnode_rate, int training, uint64_t seed,
                                       const uint8_t* d_keep, int64_t keep_stride, float* d_grad_x, int64_t n_nodes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The GRAND+ training objective after the MLP, fused (model.py:123-139, 321-331).
 * d_z fp32 [S x B x C] (S = n_samples <= 16, B = n_rows, C = n_classes <= 4096): logits, or
 * log-probabilities when inputs_are_log_probs != 0.  Rows b < n_labeled carry d_labels[b] (int64);
 * the rest are the unlabelled batch.  With logp = log_softmax(z) and p = exp(logp):
 *   L_sup  = (1/S) sum_s mean_{b < n_l, y_b != ignore_index} -logp[s,b,y_b]
 *   avg_p  = (1/S) sum_s p[s];  mask_b = b >= n_l and max_c avg_p[b,c] > conf
 *   q_b    = softmax(log(avg_p[b]) / tem)  (log(avg_p) formed in the log domain)
 *   L_con  = (1/S) sum_s mean_{b in mask} (kind GP_LOSS_KL: sum_c -q logp;  GP_LOSS_L2: sum_c (p - q)^2)
 *   loss   = L_sup + weight * L_con
 * A mean over an empty set is NaN (as torch.mean of an empty tensor) and contributes no gradient.
 * Labels outside [0, C) other than ignore_index are never read as an index: they are left out of
 * L_sup and counted.
 *
 * gp_grand_loss writes d_out fp32[3] = {loss, L_sup, L_con} and d_counts int32[4] = {n_conf, n_valid,
 * n_correct (argmax of the last sample == label), n_bad_labels}.  d_workspace: device memory of
 * GP_GRAND_LOSS_WORKSPACE_BYTES(n_rows) bytes, 8-byte aligned, owned by the caller (nothing is
 * allocated on the call path).  Two launches: a row kernel and a one-workgroup fp64 reduce.
 *
 * gp_grand_loss_backward writes d_grad_z [S x B x C] (the gradient with respect to d_z) from the same
 * arguments, the forward's d_counts and the device scalars d_grad_loss (required), d_grad_sup and
 * d_grad_con (the gradients of L_sup and L_con themselves; NULL = 0).  One launch.
 *
 * Both enqueue on `stream` and never synchronise; no atomics, so both are bitwise reproducible.
 * Arguments (sizes, NULL pointers, tem <= 0, unknown kind) are checked before the device is touched.
 * ------------------------------------------------------------------------------------------ */
#define GP_LOSS_KL 0
#define GP_LOSS_L2 1
#define GP_GRAND_LOSS_WORKSPACE_BYTES(n_rows) ((int64_t)(n_rows) * 20)

int gp_grand_loss(int device, const float* d_z, int32_t n_samples, int64_t n_rows, int32_t n_classes,
                  const int64_t* d_labels, int64_t n_labeled, int64_t ignore_index, float weight, float tem, float conf,
                  int kind, int inputs_are_log_probs, void* d_workspace, float* d_out, int32_t* d_counts, void* stream);
int gp_grand_loss_backward(int device, const float* d_z, int32_t n_samples, int64_t n_rows, int32_t n_classes,
                           const int64_t* d_labels, int64_t n_labeled, int64_t ignore_index, float weight, float tem, float conf,
                           int kind, int inputs_are_log_probs, const float* d_grad_loss, const float* d_grad_sup,
                           const float* d_grad_con, const int32_t* d_counts, float* d_grad_z, void* stream);

/* ------------------------------------------------------------------------------------------
 * GRAND+'s MLP, one block for all S samples of a step (model.py:48-66, model_mag.py:57-67):
 *
 *     block(x) = Linear( dropout_p( BN( node_norm( relu?(x) ) ) ) ),   node_norm(u) = u / (1e-12 + |u|_2)
 *
 * d_x fp32 [S x B x F_in] contiguous (S = n_samples in [1, 16], B = n_rows, F_in = f_in), d_out [S x B x F_out];
 * d_weight [F_out x F_in] and d_bias [F_out] (NULL = no bias) as nn.Linear holds them.  flags: GP_MLP_RELU,
 * GP_MLP_NORM (node_norm), GP_MLP_BN, GP_MLP_TRAINING.
 *   BatchNorm in training uses sample s's own mean and biased variance over its B rows (B >= 2) and updates
 *   d_running_mean / d_running_var (NULL = no running statistics) once per sample, in sample order:
 *   r <- (1 - momentum) r + momentum stat_s with the unbiased variance, and *d_num_batches_tracked += S (NULL = none).
 *   In eval the running statistics are folded into one per-column affine map.  d_bn_weight / d_bn_bias NULL = 1 / 0.
 *   Dropout (training and dropout > 0): entry b * F_in + f of sample s is kept by d_keep[(s * B + b) * F_in + f] != 0
 *   when d_keep (uint8 [S x B x F_in]) is given, else by random_prop's counter hash (keep_scale, csrc/gp_common.hpp) on the seed
 *       GP_MLP_LAYER_SEED(gp_sample_seed(seed, s), layer),   GP_MLP_LAYER_SEED(x, l) = mix(x ^ (l + 1) * 0xA0761D6478BD642F)
 *   with gp_sample_seed and mix of the S-sample random_prop above (grand_plus_amd.mlp.layer_seed mirrors it).  Kept
 *   entries are scaled by 1 / (1 - dropout); dropout = 1 gives zeros, dropout = 0 draws nothing.
 *   The Linear is fp32-input MFMA; the steps before it are applied while its A tile is staged.
 *
 * Contracts:
 *   - sample independence: out[s] equals the n_samples = 1 call on x[s] with gp_sample_seed(seed, s) (or keep row s),
 *     bit for bit.  Every output element is one fixed k-ordered chain per reduction chunk, the chunks summed in order,
 *     and the chunking depends on (B, F_in, F_out) only, never on S or on the row tiling;
 *   - determinism: forward, every gradient and the running statistics are bitwise equal run to run (no atomics);
 *   - no host synchronisation and no allocation on the call path: the caller passes the buffers below;
 *   - the number of launches does not depend on S (forward at most 4, backward at most 7);
 *   - any B: grid dimensions stay within their limits (eval over millions of rows).
 *   Arguments are checked before the device is touched.
 *
 * gp_mlp_block_forward: d_saved (required with GP_MLP_NORM or GP_MLP_BN) receives GP_MLP_SAVED_FLOATS floats: the row
 * scales [S*B], then per (s, f) the BN mean, 1/sqrt(var + eps), and the affine map's scale and shift.  d_saved_a
 * (optional, [S x B x F_in]) receives the Linear's input a as it was used; the backward needs it for the weight gradient.
 * d_workspace: GP_MLP_FORWARD_WORKSPACE_BYTES bytes.
 *
 * gp_mlp_block_backward takes the forward's arguments, d_saved, d_saved_a and d_grad_out [S x B x F_out], and writes
 * those of d_grad_x [S x B x F_in], d_grad_weight, d_grad_bias, d_grad_bn_weight, d_grad_bn_bias that are not NULL
 * (all are overwritten, summed over the S*B rows in a fixed order).  d_grad_x is the gradient at d_x through every
 * step of the block.  d_workspace: GP_MLP_BACKWARD_WORKSPACE_BYTES bytes.
 * ------------------------------------------------------------------------------------------ */
#define GP_MLP_RELU 1
#define GP_MLP_NORM 2
#define GP_MLP_BN 4
#define GP_MLP_TRAINING 8
#define GP_MLP_SAVED_FLOATS(S, B, f_in) ((int64_t)(S) * (int64_t)(B) + 4 * (int64_t)(S) * (int64_t)(f_in))
#define GP_MLP_FORWARD_WORKSPACE_BYTES(S) ((int64_t)(S) * 2097152)
#define GP_MLP_BACKWARD_WORKSPACE_BYTES(S, B, f_in) (4 * ((int64_t)(S) * (int64_t)(B) * (int64_t)(f_in) + 524288))

int gp_mlp_block_forward(int device, const float* d_x, int32_t n_samples, int64_t n_rows, int32_t f_in, int32_t f_out,
                         const float* d_weight, const float* d_bias, int flags,
                         const float* d_bn_weight, const float* d_bn_bias, float* d_running_mean, float* d_running_var,
                         int64_t* d_num_batches_tracked, float bn_eps, float bn_momentum,
                         float dropout, uint64_t seed, int32_t layer, const uint8_t* d_keep,
                         float* d_out, float* d_saved, float* d_saved_a, void* d_workspace, void* stream);
int gp_mlp_block_backward(int device, const float* d_x, int32_t n_samples, int64_t n_rows, int32_t f_in, int32_t f_out,
                          const float* d_weight, int flags, const float* d_bn_weight,
                          float dropout, uint64_t seed, int32_t layer, const uint8_t* d_keep,
                          const float* d_saved, const float* d_saved_a, const float* d_grad_out,
                          float* d_grad_x, float* d_grad_weight, float* d_grad_bias, float* d_grad_bn_weight, float* d_grad_bn_bias,
                          void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The end of a training step, fused (model.py:116-120, 333-334, same in model_mag.py):
 *
 *     norm = || all gradients ||_2;   coef = max_norm > 0 ? min(max_norm / (norm + 1e-6), 1) : 1     (clip_grad_norm_)
 *     g = grad * coef + weight_decay * p;   m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g g
 *     p -= step_size * (m / (sqrt(v) * rsqrt_bc2 + eps))                                              (torch.optim.Adam)
 *
 * for fp32 tensors on `device`.  `tensors` is a HOST array of n_tensors entries of DEVICE pointers (numel = 0 is legal
 * and contributes nothing); it is copied into the kernel arguments, GP_OPTIM_MAX_TENSORS entries per launch, so nothing
 * is uploaded.  step_size = lr / (1 - beta1^t) and rsqrt_bc2 = 1 / sqrt(1 - beta2^t) are the caller's, formed in double
 * from its step count t.  beta1 and beta2 are doubles because the kernel needs (float)(1 - beta), which a beta already
 * rounded to float no longer gives (1 - (float)0.999 is off by 1.3e-5 of itself); lr only takes part through step_size.
 * The squares are summed in float64 (exact products); the update is fp32 without fused multiply-adds.  A NaN norm gives
 * a NaN coef, as torch.clamp does.  *d_norm_out (device float) receives the norm before clipping.
 * d_workspace: GP_OPTIM_WORKSPACE_BYTES bytes of device memory, 8-byte aligned, the caller's.
 *
 * flags:
 *   GP_OPTIM_CLIP_ONLY   the standalone clip_grad_norm: grad * coef is written back into grad (the const of the struct
 *                        member is cast away in this mode only) and nothing else is touched; param / exp_avg / exp_avg_sq may
 *                        be NULL.  With max_norm <= 0 nothing is written but the norm.
 *   GP_OPTIM_NORM_ONLY   only the squared-norm partials are left in d_workspace (d_norm_out may be NULL);
 *   GP_OPTIM_NORM_READY  d_workspace holds the partials of an earlier GP_OPTIM_NORM_ONLY call on this stream: one norm
 *                        over several calls with different hyper-parameters (an optimiser's parameter groups).
 *
 * Contracts:
 *   - launches: at most 2 when n_tensors <= GP_OPTIM_MAX_TENSORS (one with NORM_ONLY or NORM_READY); more tensors are
 *     cut into groups of GP_OPTIM_MAX_TENSORS: one norm launch per group, then one update launch per group;
 *   - no atomics: the partials are summed in index order with one fixed tree, bitwise the same run to run and in
 *     every workgroup;
 *   - element independence: an element's update depends only on its own param, grad, exp_avg, exp_avg_sq and on coef,
 *     not on its position, its tensor's alignment or the other tensors of the call;
 *   - grad is read-only (without GP_OPTIM_CLIP_ONLY);
 *   - nothing on the call path synchronises, copies or allocates; arguments are checked before the device is touched:
 *     GP_ERR_INVALID_ARG for n_tensors < 0, numel < 0, an unknown flag or a non-finite hyper-parameter, GP_ERR_NULL for
 *     a missing pointer.
 * ------------------------------------------------------------------------------------------ */
typedef struct gp_optim_tensor {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t numel;
} gp_optim_tensor;
#define GP_OPTIM_MAX_TENSORS 32
#define GP_OPTIM_WORKSPACE_BYTES 8192   /* 1024 float64 partials, however many elements there are */
#define GP_OPTIM_CLIP_ONLY 1
#define GP_OPTIM_NORM_ONLY 2
#define GP_OPTIM_NORM_READY 4

int gp_clip_adam_step(int device, const gp_optim_tensor* tensors, int32_t n_tensors, int flags,
                      float max_norm, float lr, double beta1, double beta2, float eps, float weight_decay,
                      float step_size, float rsqrt_bc2, void* d_workspace, float* d_norm_out, void* stream);

/* The head of an evaluation (the two evaluation entry points, the GP_EVAL_* flags and GP_EVAL_WORKSPACE_BYTES):
 * declared in a header of their own, part of this ABI. */
#include "grandplus_eval.h"

/* The deterministic scatter backwards (sort-then-gather forms of the two atomic backwards above, their order
 * contract and the GP_SCATTER_*_WORKSPACE_BYTES macros): declared in a header of their own, part of this ABI. */
#include "grandplus_scatter.h"

/* The eval-only MLP block over any number of rows (the inference entry point, its arithmetic and row-independence
 * contracts and GP_MLP_INFER_WORKSPACE_BYTES): declared in a header of its own, part of this ABI. */
#include "grandplus_infer.h"

/* The last two eval blocks as one kernel, the hidden activations staying in LDS (the entry point, its bitwise
 * contract against two gp_mlp_infer_block calls and GP_MLP_INFER_CHAIN_WORKSPACE_BYTES): declared in a header of its own,
 * part of this ABI. */
#include "grandplus_infer_chain.h"

/* MAG's fused front end (resident rows -> S augmented embeddings in one launch, forward and backward, with its
 * mask formulas, order contract and bounds rules): declared in a header of its own, part of this ABI. */
#include "grandplus_mag.h"

/* Heaviest rows first (option "row_order"): the internal entry points that expose the order a call's rows were handed
 * out in, and the sketch kernel's per-workgroup exit stamps: declared in a header of their own, part of this ABI. */
#include "grandplus_order.h"

/* The device-resident state of a training step (gp_step_state, the launch that advances it, the launch that
 * writes a step's dropout masks from its seed, and gp_clip_adam_step with its bias corrections read from it): declared in
 * a header of their own, part of this ABI. */
#include "grandplus_step.h"

/* The fit loop around that step (the step's batch selection drawn on the device from the step state, the
 * early-stop rule over gp_fit_track, and the snapshot of the best weights): declared in a header of their own, part of
 * this ABI. */
#include "grandplus_fit.h"

/* ------------------------------------------------------------------------------------------
 * exact full-graph feature propagation of the inference path, reference
 * predict() (model.py:181-224), lines 186-210.  mode 0 = ppr, 1 = avg, 2 = single (args.prop_mode);
 * `order` = args.order propagation steps.  A is the CSR of `g` (adj + I as the caller built it,
 * model.py:243); d_edge_weight = its stored values (float32[nnz], device) or NULL for an all-ones
 * matrix -- what adj + I is for every shipped dataset.  d_features / d_out are float32[n_nodes x
 * feat_dim] on g's device (the reference iterates in float64 and casts the result to float32,
 * model.py:175; here sums are fp64, storage fp32).  Enqueued on `stream`; one host synchronisation
 * happens inside (long-row census).
 * ------------------------------------------------------------------------------------------ */
int gp_propagate_features(gp_graph* g, const float* d_features, int32_t feat_dim, const float* d_edge_weight,
                          int mode, int order, double alpha, float* d_out, void* stream);

/* internal: the device CSR of a graph for the other translation units (indices words carry degree bits
 * above *node_mask; packs them first if that has not happened yet) */
int gp_internal_graph_csr(gp_graph* g, const int** d_indptr, const int** d_indices, uint32_t* node_mask, void* stream);

/* internal (tests): the SELF-ADDRESSED copy of the CSR the sketch kernel runs on (built now if it does not exist yet), copied
 * to the host.  Rows start at units of 32 column words (128 bytes); node_pos[u] = first unit of row u (n_nodes + 1 entries); a
 * column word is (unit of the target) | min(deg(target), *deg_sat) << *unit_bits; padding and the sentinel word
 * acsr[32 * *n_units] are -1; unit_info[first unit of a row] = its node id, [second unit of a multi-unit row] = its degree.
 * Call with NULL buffers for the sizes, then with h_acsr int32[32 * n_units + 1], h_node_pos uint32[n_nodes + 1], h_unit_info
 * int32[n_units].  *n_units = 0: the graph does not allow the layout (unit numbers would leave fewer than two degree bits) and
 * the general kernel takes every call. */
int gp_internal_graph_acsr(gp_graph* g, int32_t* h_acsr, uint32_t* h_node_pos, int32_t* h_unit_info,
                           int64_t* n_units, int* unit_bits, uint32_t* deg_sat);

/* internal: the extended counters of the diagnostic build (-DGP_DIAG; all 0 in the product library): [0] wave
 * cycles, [1] cycles the waves waited at workgroup barriers, [2] barriers passed, [16 + 6*level + k] per level
 * (k = 0 expand ticks, 1 scan ticks, 2 edges, 3 frontier nodes, 4 push-list entries, 5 table passes); n <= 128 */
int gp_internal_diag_counters(gp_graph* g, int64_t* out, int n);

/* internal (host arithmetic only, no GPU needed): how gp_gfpush cuts a call of n_seeds rows over the n_parts GPUs of a
 * multi-GPU handle.  out[0] = GPUs that compute, [1] = GPUs in the gather, [2] = rows per GPU = ceil(S / G),
 * [3] = bytes per packed slab, [4] = 1 when the call is handed to GPU 0 as it is; then (first row, rows) per GPU.
 * n_out >= 5 + 2 * n_parts.  The CPU tests drive the >= 2-GPU partitioning through this seam. */
int gp_internal_multi_plan(int64_t n_seeds, int K, int n_parts, int64_t min_rows_per_gpu, int force_collective, int gather_host,
                           int64_t* out, int n_out);

/* internal: lets the second translation unit report through gp_last_error (not for callers) */
void gp_internal_set_error(int status, const char* where, const char* detail);
/* Milliseconds the calling thread's last gp_graph_create spent: [0] HIP runtime + device, [1] allocations, [2] upload, [3] validation on
 * the device, [4] per-graph objects (bench.py's cold_call block). */
void gp_internal_create_ms(double* out5);
/* Starts the HIP runtime's context on `device` (hipSetDevice + hipFree(NULL)): what a process's first allocation otherwise pays. */
int gp_internal_warm_device(int device);

#ifdef __cplusplus
}
#endif
#endif /* GRANDPLUS_H */
