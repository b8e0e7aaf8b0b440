/* rlap_hip.h -- C ABI of librlap_hip.so, the MI355X (gfx950) implementation of
 * rLap's approximate-Cholesky / randomized Schur-complement augmentor.
 *
 * This is the drop-in boundary for ONE path of kvignesh1420/rlap:
 *   torch op  extension_cpp::approximate_cholesky(Tensor edge_info, int num_nodes,
 *             int num_remove, str o_v, str o_n) -> Tensor
 *             (reference: rlap/csrc/py_api_binder.cc:54-69,80-88)
 *   torch op  extension_cpp::identity(Tensor a) -> Tensor
 *             (reference: rlap/csrc/py_api_binder.cc:71-76)
 * which are what rlap/ops.py:52-58 and :61-63 call.  Plain pointers and sizes
 * only; every array pointer is DEVICE memory unless its name starts with h_.
 * All work is enqueued on the handle's HIP stream without any host synchronisation
 * in between (every workspace size is an upper bound computed from E, n and G; input
 * checks and growth limits are evaluated by the kernels); the call returns after ONE
 * read-back of the scalars it reports. (Inputs of >= 2^21 entries: one more, early, 32-byte read-back
 * decides whether the COO sort can be skipped because the input is sorted already.)
 * Threading: a handle owns its workspace and serialises the calls made on it (a mutex);
 * for concurrent calls give every host thread its own handle (and stream) -- the
 * reference builds a fresh ApproximateCholesky per call (py_api_binder.cc:57).
 */
#ifndef RLAP_HIP_H
#define RLAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rlap_handle_s* rlap_handle;

/* o_v: reference strings "random" / "degree" / "coarsen" (rlap/ops.py:49) */
enum { RLAP_OV_RANDOM = 0, RLAP_OV_DEGREE = 1, RLAP_OV_COARSEN = 2 };
/* o_n: reference strings "asc" / "desc" / "random" (rlap/ops.py:50) */
enum { RLAP_ON_ASC = 0, RLAP_ON_DESC = 1, RLAP_ON_RANDOM = 2 };

/* status codes */
enum {
    RLAP_OK = 0,
    RLAP_E_NOT_SYMMETRIC = 1, /* reference: prints + exit(0), factorizers.cc:19-22 */
    RLAP_E_INDEX_RANGE = 2,
    RLAP_E_BAD_ARG = 3,
    RLAP_E_POOL_OVERFLOW = 4, /* internal growth limits; the call retries with a larger */
    RLAP_E_LOG_OVERFLOW = 5,  /* workspace by itself, these only surface if that fails  */
    RLAP_E_RNG_OVERFLOW = 6,
    RLAP_E_OUT_OVERFLOW = 7,  /* out_cap_rows too small; *needed rows reported */
    RLAP_E_HIP = 8,
    RLAP_E_TOO_LARGE = 9,     /* nnz + growth pool exceeds int32 slot ids */
    RLAP_E_INTERNAL = 10,
    RLAP_E_WORKSPACE = 11,    /* caller-provided workspace / uniform table too small: rlap_workspace_needed() says how much */
    RLAP_E_NOT_GROUPED = 12,  /* rlap_snapshot_stats: a column id starts two separate blocks of rows in one segment */
    RLAP_E_OUT_CAPACITY = 13  /* rlap_snapshot_ppr, rlap_edge_drop, rlap_node_sample, rlap_edge_add: the kept entries exceed out_cap_rows; nothing written, rows_needed reported */
};

typedef struct {
    int64_t nnz;          /* directed entries after zero-drop + duplicate sum */
    int64_t n_eliminated; /* sum over graphs of min(t, n-1) (preconditioner.cc:358) */
    int64_t n_draws;      /* uniforms consumed (max over graphs)              */
    int64_t out_rows;     /* rows of sc_edge_info                             */
    int64_t live_entries; /* L: live directed entries read by the output pass */
    float ms_setup;       /* COO->CSR, symmetry, twins, PQ init (HIP events)  */
    float ms_elim;        /* elimination kernel                               */
    float ms_output;      /* sc_order + sc_merge + sc_compact                 */
    float ms_sc_merge;    /* output pass A alone                              */
    float ms_sc_compact;  /* output pass B alone (ballot/prefix compaction)   */
    float ms_total;
    int32_t n_retries;    /* times the call was repeated with a larger workspace (RLAP_E_*_OVERFLOW inside) */
    int32_t reserved;     /* COO sort: 0 done, 1 skipped (input in (col,row) order), 2 skipped, input in (row,col) order read transposed */
    int64_t n_rounds;     /* elimination: batch rounds, summed over graphs              */
    int64_t n_singles;    /* elimination: vertices that took the single-vertex path     */
    /* (appended fields: the offsets above are unchanged) */
    int32_t elim_kernel;  /* elimination kernel of the final attempt: 0 none ran (t = 0, empty graph), 1 round kernel, 2 dataflow kernel */
    int32_t retry_causes; /* bit k set: an attempt of the call was repeated for retry kind k (1 append pool, 2 PQ log, 3 uniform table,
                             4 output-pass scratch, 5 input read transposed was not exactly symmetric, 6 dataflow long-column scratch,
                             7 dataflow reorder buffer too small, 8 the dataflow kernel gave up); 7 and 8 repeat on the round kernel */
    int32_t flow_abort;   /* why the dataflow kernel gave up (retry kind 8): 0 it did not, 1 stall watchdog, 2 sorted-index check,
                             3 appended count over 2^22, 4 column longer than its buffer */
    int32_t n_rounds_narrow; /* degree order: the part of n_rounds that the 16-slot round kernel ran before it handed over to the
                             32-slot one (0: it was not used, or the first column was already longer than 16 slots) */
    int32_t n_squeezes;   /* degree order on large graphs: squeeze passes (dead entries removed from all columns between two launches
                             of the 16-slot kernel) behind which that kernel committed at least one more round, summed over graphs */
    int32_t pad;
} rlap_stats;

/* Lifetime.  A handle binds to the HIP device current at creation.  It owns a few KB of tables (allocated in
 * rlap_create); every per-call buffer is carved from ONE workspace arena and the cached MT19937-64 uniform table is a
 * second buffer -- the caller's (rlap_set_workspace) or, without one, the handle's own (one hipMalloc each, repeated only
 * when a call is of a larger size class than any before it; never a hipFree/hipMalloc in a call that fits). */
int rlap_create(rlap_handle* out);
int rlap_destroy(rlap_handle h);
int rlap_set_stream(rlap_handle h, void* hip_stream); /* hipStream_t; NULL = default */

/* Where the sampling uniforms come from (SURVEY section 7 step 7 / 8(b) `mode`).  0 = "exact" (default): the first outputs of
 * the default-seeded std::mt19937_64 in elimination order, preconditioner.cc:356-357,386 -- results equal the reference's.
 * 1 = "frontier": the j-th uniform of a vertex's elimination is a function of (seed, vertex, j); same distribution, no order
 * in which draws must be made (for o_v = random the multi-CU kernel then waits for nothing but its true neighbours);
 * bit-exact against the oracle in the same mode, NOT against the reference.  Applies to the handle's later calls. */
int rlap_set_rng_mode(rlap_handle h, int mode);

/* Workspace contract (SURVEY 8(b) "caller owns every buffer"; the reference's only allocation is the torch tensor of its
 * result, py_api_binder.cc:42).
 *   rlap_workspace_bytes : upper bound, for a fresh handle, of the arena bytes and of the uniform-table entries a call on
 *                          E directed input entries, n_total vertices (summed over the G graphs of a batch) needs, whatever
 *                          num_remove and the split of n_total over the graphs are.
 *   rlap_workspace_query : the same for THIS handle (its growth factors rise after an RLAP_E_*_OVERFLOW retry).
 *   rlap_set_workspace   : d_ws (256-byte aligned, ws_bytes) and d_rng (rng_entries doubles) are used by all later calls; the
 *                          library then allocates and frees nothing.  NULL gives a buffer back to the handle.  The table is
 *                          generated into d_rng by the first call that needs it (and again whenever d_rng changes).
 *   A call that does not fit returns RLAP_E_WORKSPACE without touching the device; rlap_workspace_needed reports what it
 *   wanted (the caller allocates that much and repeats the call). */
int rlap_workspace_bytes(int64_t E, int64_t n_total, int64_t G, int symmetrize, size_t* ws_bytes, int64_t* rng_entries);
int rlap_workspace_query(rlap_handle h, int64_t E, int64_t n_total, int64_t G, int symmetrize, size_t* ws_bytes, int64_t* rng_entries);
int rlap_set_workspace(rlap_handle h, void* d_ws, size_t ws_bytes, double* d_rng, int64_t rng_entries);
int rlap_workspace_needed(rlap_handle h, size_t* ws_bytes, int64_t* rng_entries);
int rlap_set_timing(rlap_handle h, int enable);       /* fill rlap_stats.ms_* with HIP events */
const char* rlap_status_string(int status);

/* identity: (rows, cols) f64 row-major -> column-major staging -> row-major.
 * Replaces extension_cpp::identity (py_api_binder.cc:71-76, tensorToEigen :10-31,
 * eigenToTensor :33-51).  d_tmp needs rows*cols doubles. */
int rlap_identity(rlap_handle h, const double* d_in, double* d_tmp, double* d_out, int64_t rows, int64_t cols);

/* Split the reference's packed edge_info (E,3) f64 row-major [row, col, w]
 * (rlap/ops.py:47) into the COO arrays the calls below take. */
int rlap_unpack_edge_info(rlap_handle h, const double* d_edge_info, int64_t E, int64_t* d_row, int64_t* d_col, double* d_w);

/* Exchange format of sc_edge_info for the batched multi-GPU mode (no reference counterpart: the
 * reference has no multi-process path): row [row, col, w] <-> two 64-bit words (row << 32 | col, bits of w), so
 * that the RCCL all-gather moves 16 instead of 24 bytes per row.  d_packed holds 2 * rows 64-bit words.  Stream-ordered. */
int rlap_pack_rows(rlap_handle h, const double* d_sc, int64_t rows, void* d_packed);
int rlap_unpack_rows(rlap_handle h, const void* d_packed, int64_t rows, double* d_sc);

/* The op.  Replaces ApproximateCholesky::setup + getSchurComplement
 * (factorizers.cc:46-73) for one graph:
 *   d_row/d_col/d_w : COO, E directed entries (d_w NULL = all ones; w==0 rows are
 *                     dropped, duplicates summed: reader.cc:42-61)
 *   n, t            : num_nodes, num_remove
 *   d_perm          : o_v=random only: the node_id vector (a permutation of
 *                     0..n-1) popped from the BACK (preconditioner.cc:588-613);
 *                     the reference draws it from std::random_device.  Checked on
 *                     the device: anything but a permutation gives RLAP_E_BAD_ARG.
 *                     NULL = drawn on the device from shuffle_seed (keyed shuffle)
 *   shuffle_seed    : o_n=random / o_v=coarsen only: seed of the keyed neighbour
 *                     order that stands in for std::shuffle(random_device)
 *   d_out           : (out_cap_rows,3) f64 row-major [row, col, w]
 *   h_out_rows      : rows written (or needed, with RLAP_E_OUT_OVERFLOW)      */
int rlap_approx_chol(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E,
                     int64_t n, int64_t t, int o_v, int o_n, const int64_t* d_perm, uint64_t shuffle_seed,
                     double* d_out, int64_t out_cap_rows, int64_t* h_out_rows, rlap_stats* h_stats);

/* Batched graphs (a disjoint union): graph g owns the node ids
 * [h_node_ptr[g], h_node_ptr[g+1]); no edge may cross graphs.  Each graph is
 * eliminated independently with its own num_remove and its own restart of the
 * sampling stream -- what G separate reference calls would do: the rows of graph g
 * are those of rlap_approx_chol on graph g alone (ids shifted by node_ptr[g]) with
 * its slice of d_perm and with shuffle_seed + g (the keyed neighbour order hashes
 * graph-local ids).  d_perm holds, for graph g, a permutation of LOCAL ids
 * 0..n_g-1 at [node_ptr[g], node_ptr[g+1]).
 * Rows come out grouped by graph, with global node ids; h_out_row_ptr[G+1]. */
int rlap_approx_chol_batched(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E,
                             int64_t G, const int64_t* h_node_ptr, const int64_t* h_num_remove, int o_v, int o_n,
                             const int64_t* d_perm, uint64_t shuffle_seed, double* d_out, int64_t out_cap_rows,
                             int64_t* h_out_row_ptr, rlap_stats* h_stats);

/* Views: K independent Schur complements of one input (a single graph, G = 1, or a batch of G graphs given by h_node_ptr as
 * for rlap_approx_chol_batched) in one call -- what graph-contrastive training asks for at every step (two or more views).
 * (view k, graph g) equals graph k*G + g of rlap_approx_chol_batched on the K-fold disjoint union of the input, with the same
 * shuffle_seed, ids shifted back: by the batched contract that is rlap_approx_chol on graph g with shuffle_seed + k*G + g and
 * perm slice (k, g).  K = 1, G = 1 is rlap_approx_chol.  Holds in both rng modes (rlap_set_rng_mode).
 *   h_num_remove : [K*G], view-major: num_remove of (view k, graph g) at k*G + g
 *   d_perm       : o_v=random only, [K*N] (N = h_node_ptr[G]) or NULL: at k*N + node_ptr[g], a permutation of graph g's LOCAL ids
 *   d_out        : rows grouped view-major (all graphs of view 0, then view 1, ...), node ids in the INPUT's id space [0, N)
 *   h_out_ptr    : [K*G+1] row offsets of (view k, graph g) at k*G + g
 *   h_stats      : of the union: counts summed over views (n_draws: max over views and graphs)
 * The input is read, sorted, symmetry-checked and linked once (an asymmetric input fails once, RLAP_E_NOT_SYMMETRIC); its CSR is
 * then replicated K times on the device.  Note: in mode "exact", o_v = degree with o_n = asc / desc draws nothing that depends on
 * the seed (the reference's default-seeded std::mt19937_64, preconditioner.cc:356), so two views with equal num_remove are equal;
 * mode "frontier" gives distinct samples.
 * Workspace: as a batched call on the union, rlap_workspace_query(h, K*E, K*N, K*G, 0, ...).
 * K < 1: RLAP_E_BAD_ARG; K*N, K*E and K*G are subject to the limits of a batched call of that size (RLAP_E_TOO_LARGE). */
int rlap_approx_chol_views(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E,
                           int64_t G, const int64_t* h_node_ptr, int64_t K, const int64_t* h_num_remove, int o_v, int o_n,
                           const int64_t* d_perm, uint64_t shuffle_seed, double* d_out, int64_t out_cap_rows, int64_t* h_out_ptr,
                           rlap_stats* h_stats);

/* Depths: K nested Schur complements of ONE graph from one elimination.  h_num_remove[K] must be non-decreasing (zero and equal
 * neighbours allowed; each value is clamped to n-1 as in rlap_approx_chol).  Snapshot k goes to rows [h_out_ptr[k], h_out_ptr[k+1])
 * of d_out and equals rlap_approx_chol(..., t = h_num_remove[k]) with the same d_perm / shuffle_seed / rng mode: indices, row order
 * and weights.  The elimination runs once, in segments [t_{k-1}, t_k), each followed by the output pass of its snapshot.
 *   h_out_ptr    : [K+1]; out_cap_rows: K*E rows always suffice (an elimination never adds entries)
 *   h_stats      : n_eliminated, n_draws and live_entries of the deepest snapshot, out_rows the sum over snapshots, elim_kernel
 *                  the one kernel that ran every segment; a retry in any segment repeats the whole call
 * Decreasing depths, K < 1 or a null pointer: RLAP_E_BAD_ARG.  Workspace: may want more than rlap_workspace_query(h, E, n, 1, 0, ...)
 * reports for a single call -- RLAP_E_WORKSPACE then, with rlap_workspace_needed() telling how much. */
int rlap_approx_chol_depths(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E, int64_t n,
                            int64_t K, const int64_t* h_num_remove, int o_v, int o_n, const int64_t* d_perm, uint64_t shuffle_seed,
                            double* d_out, int64_t out_cap_rows, int64_t* h_out_ptr, rlap_stats* h_stats);

/* Views x depths: D nested snapshots of every (view k, graph g) of a views call, from one elimination of the K-fold union (G = 1:
 * one graph; K = 1: a batch; K = G = 1 is rlap_approx_chol_depths, D = 1 is rlap_approx_chol_views).
 *   h_num_remove : [D][K*G], row-major; column k*G + g is the depth list of (view k, graph g): non-decreasing down the column (zero
 *                  and repeated values allowed), each value clamped to n_g - 1 as in every other call
 *   d_perm       : o_v=random only, [K*N] laid out as in rlap_approx_chol_views, or NULL; every depth uses the same perm
 *   h_out_ptr    : [D*K*G + 1]; rows are depth-major, then view, then graph: snapshot (d, k, g) is rows
 *                  [h_out_ptr[(d*K + k)*G + g], h_out_ptr[(d*K + k)*G + g + 1]), node ids in the INPUT's id space
 *   out_cap_rows : D*K*E rows always suffice
 *   h_stats      : as for rlap_approx_chol_depths, over the union
 * Contract: snapshot (d, k, g) equals rlap_approx_chol on graph g alone with t = h_num_remove[d][k*G + g], shuffle_seed + k*G + g
 * and perm slice (k, g), ids shifted by node_ptr[g] -- indices, row order and weights, in both rng modes.  Equivalently depth row d
 * of the output equals rlap_approx_chol_views(..., h_num_remove = row d), h_out_ptr included up to a base offset.  The elimination
 * runs once, segment d covering positions [t_{d-1}, t_d) of every graph; one host synchronisation per call (two for inputs of at
 * least 2^21 entries), as for the other calls.
 * A decreasing column, D, K or G < 1, or a null pointer: RLAP_E_BAD_ARG; limits as for rlap_approx_chol_views, and D*K*G < 2^30
 * (RLAP_E_TOO_LARGE).  Workspace: may want more than rlap_workspace_query(h, K*E, K*N, K*G, 0, ...) reports -- RLAP_E_WORKSPACE
 * then, with rlap_workspace_needed() telling how much. */
int rlap_approx_chol_views_depths(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E,
                                  int64_t G, const int64_t* h_node_ptr, int64_t K, int64_t D, const int64_t* h_num_remove,
                                  int o_v, int o_n, const int64_t* d_perm, uint64_t shuffle_seed,
                                  double* d_out, int64_t out_cap_rows, int64_t* h_out_ptr, rlap_stats* h_stats);

/* Snapshot statistics: for every segment s of a result of the calls above (rows [ptr[s], ptr[s+1]) of d_sc, S segments), its node
 * count and the largest eigenvalue of its symmetric adjacency matrix A -- what scripts/rlap_vc_spectral.py records per snapshot
 * (torch.unique, the row count, svd_lowrank of to_dense_adj) without a dense matrix.
 *   d_sc, m       : (m, 3) f64 rows [row, col, w] as the calls return them: every column's rows contiguous, the matrix symmetric
 *   d_ptr         : [S+1] row offsets (0 = ptr[0] <= ... <= ptr[S] = m)
 *   d_node_ptr    : NULL: every id lies in [0, num_nodes); else [G+1] offsets with G dividing S: segment s is graph s % G and its ids
 *                   lie in [node_ptr[s % G], node_ptr[s % G + 1]) (batched, views and depths results all put the graph fastest)
 *   weighted      : 0: A has unit entries (to_dense_adj without edge_attr); else the rows' weights
 *   tol, max_iter : Lanczos stops at step j when beta_j |y_j| <= tol * theta_j (theta_j the largest eigenvalue of T_j, y its unit
 *                   eigenvector); 0 < tol, 1 <= max_iter <= 1024
 *   d_nodes       : [S] distinct ids of the segment's rows
 *   d_lambda_max  : [S] the largest eigenvalue of A (0 for a segment without rows); for non-negative A its spectral radius
 *   d_iters, d_converged : [S] Lanczos steps taken, and whether the bound was met within max_iter (1 for an empty segment)
 *   h_info        : (nullable) what the call did
 * Deterministic: the same input gives the same bits.  d_sc and d_ptr are only read.  Scratch comes from the arena (RLAP_E_WORKSPACE
 * when a caller-provided one is too small, rlap_workspace_needed() saying how much).  Layout errors: an id out of its segment's range
 * RLAP_E_INDEX_RANGE, a column id that starts two blocks of one segment RLAP_E_NOT_GROUPED, a row id without a column of its own
 * RLAP_E_NOT_SYMMETRIC; a bad ptr / node_ptr RLAP_E_BAD_ARG. */
typedef struct {
    int64_t small_segments;   /* segments that ran in one workgroup each (up to 7,168 nodes) */
    int64_t large_segments;   /* segments whose Lanczos steps ran as device-wide launches    */
    int64_t lanczos_steps;    /* steps of the longest segment                                */
    int64_t large_steps;      /* steps enqueued for the large segments (in chunks of 32)     */
    int64_t large_launches;   /* device-wide launches of those steps                         */
    int32_t host_syncs;       /* host synchronisations of the call                           */
    int32_t not_converged;    /* segments that stopped without meeting the bound             */
} rlap_snapshot_info;

int rlap_snapshot_stats(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                        int64_t G, int64_t num_nodes, int weighted, double tol, int32_t max_iter, int64_t* d_nodes,
                        double* d_lambda_max, int32_t* d_iters, int32_t* d_converged, rlap_snapshot_info* h_info);

/* PPR diffusion of snapshots: for every segment s (as for rlap_snapshot_stats: d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes), with
 * V_s its distinct ids, A its symmetric adjacency on V_s (duplicate rows summed; the rows' weights, or unit entries), A + I with a self
 * loop, d = A 1:
 *     S = alpha (I - (1 - alpha) D^-1/2 A D^-1/2)^-1,  entries S_ij >= eps kept,  then (normalize_out) D_S^-1/2 S D_S^-1/2
 * with D_S the row sums of the kept entries -- PyGCL's compute_ppr (transition_matrix('sym'), diffusion_matrix_exact('ppr'),
 * sparsify_dense('threshold'), transition_matrix('sym')) without a dense matrix.
 *   alpha, eps, tol : 0 < alpha < 1, eps > 0, tol > 0.  S is found by K fixed Chebyshev steps, K = min{K : T_K(1/(1-alpha)) >= 1/tol}
 *                     (include: rlap_amd/csrc/rlap_cheb.h, at most 4096): every entry lies within tol of exact before normalisation
 *   flags           : RLAP_PPR_WEIGHTED (the rows' weights, else unit entries), RLAP_PPR_SELF_LOOP (A + I), RLAP_PPR_NORMALIZE
 *                     (the closing D_S^-1/2 . D_S^-1/2), RLAP_PPR_ZERO_ROWS (rows of weight 0 are allowed: an id whose only row is
 *                     (i, i, 0) is a node without edges)
 *   d_out           : (out_cap_rows, 3) f64 rows [i, j, value] in the input's id space, segment-major, then ascending i, then j
 *   d_out_ptr       : [S+1] row offsets of the segments in d_out
 *   h_info          : (nullable) what the call did; rows_needed = the kept entries
 * Exactly symmetric (the pair {i, j} takes its value from the column of the smaller id); the same input gives the same bits, and a
 * segment's rows do not depend on the other segments of the call.  More kept entries than out_cap_rows: RLAP_E_OUT_CAPACITY, nothing
 * written, h_info->rows_needed says how many (call again with that capacity).  Layout errors as for rlap_snapshot_stats; a weight
 * <= 0 (< 0 with RLAP_PPR_ZERO_ROWS) or not finite with RLAP_PPR_WEIGHTED, or alpha / eps / tol out of range: RLAP_E_BAD_ARG.
 * Scratch from the arena (grows with out_cap_rows; RLAP_E_WORKSPACE when a caller-provided one is too small). */
enum { RLAP_PPR_WEIGHTED = 1, RLAP_PPR_SELF_LOOP = 2, RLAP_PPR_NORMALIZE = 4, RLAP_PPR_ZERO_ROWS = 8 };
typedef struct {
    int64_t steps;            /* K, the Chebyshev steps                                              */
    int64_t small_tiles;      /* tiles (segment, 64 sources) that ran their K steps in one workgroup */
    int64_t large_tiles;      /* tiles that stepped with device-wide launches                         */
    int64_t groups;           /* tile groups (live tile bytes within the budget of DESIGN 4.8)        */
    int64_t launches;         /* kernel launches of the sweeps                                        */
    int64_t rows_needed;      /* kept entries: the rows of d_out (written, or needed)                 */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call                                    */
    int32_t pad;
} rlap_ppr_info;

int rlap_snapshot_ppr(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                      int64_t G, int64_t num_nodes, double alpha, double eps, double tol, int flags, double* d_out,
                      int64_t out_cap_rows, int64_t* d_out_ptr, rlap_ppr_info* h_info);

/* Markov diffusion of snapshots: for every segment s (as for rlap_snapshot_ppr), with Â = D^-1/2 A D^-1/2 (0 where
 * d = 0; A + I with a self loop), beta = 1 - alpha and order D >= 1:
 *     M = alpha Â + (1/D) sum_{k=0..D} beta^k Â^(k+1),  entries M_ij >= eps kept,  then (normalize) D_M^-1/2 M D_M^-1/2
 * with D_M the row sums of the kept entries -- a restatement of PyGCL's compute_markov_diffusion (z = Â; t = Â; D times: t = beta Â t,
 * z += t; z /= D; z += alpha Â; sparsify_dense('threshold')) without a dense matrix; it is not a run of that function.  Every column
 * is computed in Horner form by D + 1 applications of Â (rlap_amd/csrc/rlap_markov.h holds every scalar step).
 *   alpha, order, eps : 0 <= alpha <= 1, 1 <= order <= 1024 (markov::MAX_ORDER), eps > 0
 *   flags             : RLAP_MARKOV_WEIGHTED / _SELF_LOOP / _NORMALIZE / _ZERO_ROWS, as the RLAP_PPR_* flags
 *   d_out, d_out_ptr, out_cap_rows, RLAP_E_OUT_CAPACITY : as for rlap_snapshot_ppr (h_info->rows_needed says how many rows)
 * Exactly symmetric (the pair {i, j} takes its value and its keep decision from the column of the smaller id); the same input gives
 * the same bits, and a segment's rows do not depend on the other segments of the call.  An id without edges keeps no
 * row without the self loop and the one entry alpha + (1/D) sum_k beta^k with it.  Layout errors as for rlap_snapshot_stats; a
 * weight <= 0 (< 0 with RLAP_MARKOV_ZERO_ROWS) or not finite with RLAP_MARKOV_WEIGHTED, or alpha / order / eps out of range:
 * RLAP_E_BAD_ARG.  Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small).  Three host synchronisations. */
enum { RLAP_MARKOV_WEIGHTED = 1, RLAP_MARKOV_SELF_LOOP = 2, RLAP_MARKOV_NORMALIZE = 4, RLAP_MARKOV_ZERO_ROWS = 8 };
typedef struct {
    int64_t order;            /* D: D + 1 applications of the normalised adjacency                    */
    int64_t small_tiles;      /* tiles (segment, 64 sources) that ran all sweeps in one workgroup     */
    int64_t large_tiles;      /* tiles that stepped with device-wide launches                         */
    int64_t groups;           /* tile groups (one regime each, live tile bytes within the budget)     */
    int64_t launches;         /* kernel launches of the sweeps                                        */
    int64_t rows_needed;      /* kept entries: the rows of d_out (written, or needed)                 */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call                                    */
    int32_t pad;
} rlap_markov_info;

int rlap_snapshot_markov(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                         int64_t G, int64_t num_nodes, double alpha, int32_t order, double eps, int flags, double* d_out,
                         int64_t out_cap_rows, int64_t* d_out_ptr, rlap_markov_info* h_info);

/* Induced subgraphs and relabelling of snapshots: for every segment s (described as for rlap_snapshot_stats: d_sc, m, d_ptr, S,
 * d_node_ptr, G, num_nodes; S = 0 with m = 0 is allowed) the rows whose two ids both lie in the segment's node set, in their input
 * order -- torch.unique + PyG's subgraph() of every snapshot of a call, without a sort.  The call is a filter: it makes no assumption
 * about the order or the symmetry of the rows of a segment, so a plain edge list is a valid input, as is the (out, out_ptr) of
 * rlap_snapshot_ppr.
 *   d_nodes, d_nodes_ptr, nodes_len : the node sets.  d_nodes == NULL: the set of segment s is the ids that appear in its rows
 *                     (after the self-loop rule below).  d_nodes with d_nodes_ptr ([S+1], from 0 to nodes_len): the list
 *                     d_nodes[d_nodes_ptr[s] .. d_nodes_ptr[s+1]) per segment.  d_nodes without d_nodes_ptr: one list of nodes_len
 *                     ids for all segments; with d_node_ptr the set of segment s is the part of the list inside its graph's range.
 *                     Lists are sets: any order, repeats allowed; an id that no row of the segment has still belongs to the set.
 *   flags           : RLAP_SUB_RELABEL (the ids of the written rows become labels), RLAP_SUB_NO_SELF_LOOPS (rows with i == j are
 *                     dropped, and with d_nodes == NULL they do not put i into the set: remove_self_loops before unique)
 *   d_out           : (m, 3) f64, the kept rows segment by segment, the weight copied bit for bit.  The label of an id is its rank
 *                     among the sorted distinct ids of the set, starting at 0 in every segment.  That equals PyG's
 *                     subgraph(relabel_nodes=True) whenever the subset handed to it is sorted and distinct (a torch.unique result).
 *   d_out_ptr       : [S+1] row offsets of the segments in d_out
 *   d_ids, ids_cap  : the sorted distinct ids of every segment's set, segment by segment -- the map label -> id; ids_cap is the
 *                     capacity of d_ids in entries and must be at least min(2 m, (S / G) num_nodes) for d_nodes == NULL, nodes_len
 *                     with d_nodes_ptr, (S / G) nodes_len for a shared list
 *   d_ids_ptr       : [S+1] offsets of the segments in d_ids: the id of label l of segment s is d_ids[d_ids_ptr[s] + l]
 *   h_info          : (nullable) what the call did
 * The same input gives the same bits.  An id of a row or of a segment's list outside the segment's range (of a shared list: outside
 * [0, num_nodes)): RLAP_E_INDEX_RANGE; a bad ptr / node_ptr / nodes_ptr, or ids_cap below the bound: RLAP_E_BAD_ARG.  Scratch from
 * the arena: (S / G) num_nodes flag bytes, the bitmap packed from them, its scan and one count per 1,024 rows (RLAP_E_WORKSPACE when
 * a caller-provided one is too small, rlap_workspace_needed() saying how much).  One host synchronisation. */
enum { RLAP_SUB_RELABEL = 1, RLAP_SUB_NO_SELF_LOOPS = 2 };
typedef struct {
    int64_t rows_kept;        /* rows written to d_out                */
    int64_t ids_written;      /* ids written to d_ids                 */
    int64_t arena_bytes;      /* scratch bytes of the call            */
    int32_t host_syncs;       /* host synchronisations of the call    */
    int32_t pad;
} rlap_subgraph_info;

int rlap_snapshot_subgraph(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                           int64_t G, int64_t num_nodes, const int64_t* d_nodes, const int64_t* d_nodes_ptr, int64_t nodes_len,
                           int flags, double* d_out, int64_t* d_out_ptr, int64_t* d_ids, int64_t ids_cap, int64_t* d_ids_ptr,
                           rlap_subgraph_info* h_info);

/* Encoder-ready snapshots: for every segment s (described as for rlap_snapshot_stats: d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes,
 * and in the same layout: the rows of a segment grouped by column id, every row id with a column block of its own -- the result of
 * every elimination entry point) the int64 edge_index, the self loops and the coefficients of PyG's
 * gcn_norm(edge_index, edge_weight, num_nodes, improved, add_self_loops, flow="source_to_target") for
 * edge_index = sc[:, :2].long().t(): row id = source, column id = target.  (Unpinned: PyG's published semantics, not a run of it.)
 * With [lo, hi) the id range of segment s and n_s = hi - lo:
 *   RLAP_GCN_WEIGHTED   : the rows' weights; without it every row weighs 1
 *   RLAP_GCN_SELF_LOOPS : add_remaining_self_loops -- the rows with row == col leave the list, the others keep their input order,
 *                         then one loop (i, i) for every i in [lo, hi) ascending follows.  The loop of i weighs fill_value (1; 2 is
 *                         PyG's improved=True) unless the segment had loop rows of i: then the weight of the last of them in input
 *                         order (1 when unweighted).  Segment s has rows_s - loops_s + n_s entries.  Without the flag the list is
 *                         the rows as they are, loop rows included.
 *   RLAP_GCN_NORMALIZE  : deg[i] = the sum of the weights of the list's entries whose target is i (a column block and the loop),
 *                         dis[i] = deg[i]^-1/2, 0 where deg[i] == 0; the value of entry (i, j, w) is dis[i] * w * dis[j].  Without
 *                         the flag the value is w itself: the call is the conversion alone, plus the loops if asked for.
 *   RLAP_GCN_F32        : d_val is float32 (the float64 value rounded once); else float64
 *   d_src, d_dst, d_val : [cap] each, the two rows of edge_index and the values, segment-major; ids stay in the input's id space
 *   cap                 : at least m + (S / G) num_nodes with RLAP_GCN_SELF_LOOPS, m without; entries <= cap are written, and
 *                         entries == cap whenever the input has no loop rows (every elimination result)
 *   d_eptr              : [S+1] entry offsets of the segments
 *   h_info              : (nullable) what the call did
 * num_nodes may exceed the elimination's (ids without rows are legal: eliminated vertices, trailing isolated nodes); their loop has
 * degree fill_value.  Every degree is summed in one fixed order that depends on the row's place in its block only, without atomics:
 * the same input gives the same bits, and a segment's values do not depend on the other segments of the call.  Layout errors as for
 * rlap_snapshot_stats; a bad ptr / node_ptr, cap below the bound, a fill_value that is not finite or <= 0 with RLAP_GCN_SELF_LOOPS, or
 * with RLAP_GCN_WEIGHTED and RLAP_GCN_NORMALIZE a weight that is not finite or <= 0 (PyG would return NaN): RLAP_E_BAD_ARG.  Not in
 * this layout: the (out, out_ptr) of rlap_snapshot_ppr (grouped by row id) and arbitrary edge lists.  Scratch from the arena
 * (RLAP_E_WORKSPACE when a caller-provided one is too small, rlap_workspace_needed() saying how much).  One host synchronisation. */
enum { RLAP_GCN_WEIGHTED = 1, RLAP_GCN_SELF_LOOPS = 2, RLAP_GCN_NORMALIZE = 4, RLAP_GCN_F32 = 8 };
typedef struct {
    int64_t entries;          /* entries written to d_src / d_dst / d_val        */
    int64_t loops_removed;    /* loop rows of the input that left the list        */
    int64_t arena_bytes;      /* scratch bytes of the call                        */
    int32_t host_syncs;       /* host synchronisations of the call                */
    int32_t pad;
} rlap_gcn_info;

int rlap_snapshot_gcn_norm(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                           int64_t G, int64_t num_nodes, int flags, double fill_value, int64_t* d_src, int64_t* d_dst, void* d_val,
                           int64_t cap, int64_t* d_eptr, rlap_gcn_info* h_info);

/* GCN propagation of snapshots: y = A^ x for every layer of a result at once, A^ the entry list that rlap_snapshot_gcn_norm produces
 * with the same flags and fill_value -- what GCNConv(normalize=False) does next with that list (a scatter-add of val * x[src] into
 * dst), without the list, without float atomics and in a fixed order.  d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes: exactly as for
 * rlap_snapshot_gcn_norm, layout, checks and error codes included.  L = S / G is the number of layers (view x depth); the segments
 * (l, g) of one layer cover disjoint id ranges.
 *   flags     : RLAP_GCN_WEIGHTED, RLAP_GCN_SELF_LOOPS, RLAP_GCN_NORMALIZE as for rlap_snapshot_gcn_norm (RLAP_GCN_F32 is not one of
 *               this call's), and
 *               RLAP_SPMM_TRANSPOSE   : the transposed product (the backward pass: with o_v = random the two weights of a pair are
 *                                       not always the same bits, so A^ is symmetric only up to that)
 *               RLAP_SPMM_X_F32       : d_x and d_y are float32; without it float64
 *               RLAP_SPMM_X_PER_LAYER : d_x is (L, num_nodes, F), one feature matrix per layer; without it (num_nodes, F), shared
 *   d_x, F    : the features, row-major, F >= 1 columns
 *   d_y       : (L, num_nodes, F) of d_x's type; every element is written, 0 for an id without entries and without a loop
 *   h_info    : (nullable) what the call did
 * With c_e the float64 value that rlap_snapshot_gcn_norm gives entry e of segment (l, g) -- the same bits --
 *     forward    : y[l, j, :] = sum over the entries e with target j of c_e * x[l or shared, source(e), :]
 *     transposed : y[l, i, :] = sum over the entries e with source i of c_e * x[l or shared, target(e), :]
 * The order of every sum is fixed (rlap_amd/csrc/rlap_spmm.h, which a host mirror can compile): float64 throughout, the product
 * rounded and then the add, no fma; the terms of one output element in list order -- the rows of the block (transposed: the rows with
 * that source) in input order, the loop last; a list of more than 256 entries is cut into chunks of 256, each summed from 0, the
 * chunk sums added in chunk order, then the loop.  A float32 result is the float64 sum rounded once.  So the same input gives the
 * same bits, a segment's result does not depend on the other segments of the call, and nothing depends on what d_y or the arena held.
 * Limits: F <= 65,536 and L * num_nodes * F < 2^40 (RLAP_E_TOO_LARGE); F < 1, a null pointer, a flag that is not this call's, a bad
 * ptr / node_ptr, fill_value or weight as for rlap_snapshot_gcn_norm: RLAP_E_BAD_ARG.  Layout errors as for rlap_snapshot_stats; d_y
 * is then unspecified.  Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small, rlap_workspace_needed()
 * saying how much); the transposed call also sorts the rows by source there.  One host synchronisation.  Test hook: a scratch_entries
 * >= 0 of rlap_debug_set_limits is also the number of chunk sums this call may keep (lists past it are summed by one group of lanes,
 * same bits), until it is set negative again. */
enum { RLAP_SPMM_TRANSPOSE = 16, RLAP_SPMM_X_F32 = 32, RLAP_SPMM_X_PER_LAYER = 64 };
typedef struct {
    int64_t entries;          /* entries of the list the product ran over (rows that stay + loops)   */
    int64_t blocks;           /* column blocks of the call: the ids with rows                         */
    int64_t chunked_lists;    /* lists longer than one chunk                                          */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call                                    */
    int32_t pad;
} rlap_spmm_info;

int rlap_snapshot_propagate(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                            int64_t G, int64_t num_nodes, int flags, double fill_value, const void* d_x, int64_t F, void* d_y,
                            rlap_spmm_info* h_info);

/* Propagation plans: the x-independent half of rlap_snapshot_propagate, built once per elimination result and used by any number
 * of planned calls.  A plan is a device buffer that the CALLER owns (the library allocates nothing) plus the host
 * descriptor below; it holds, per direction, every list of the product as packed 16-byte records {double coefficient, int32 source
 * id, int32 0} in list order, the int64 record offset of every (layer, id), a directory of the chunks of the lists longer than 256
 * entries, and one loop coefficient per (layer, id).  The buffer is valid while it is unchanged, and independent of d_sc once the
 * build has returned.  A planned call returns the bits of rlap_snapshot_propagate on the same input with the same flags, for every
 * F, both types, both forms of d_x and both directions: the coefficients come from the same functions on the same inputs, the lists
 * hold the entries that stay in the order of rlap_amd/csrc/rlap_spmm.h, and the sum is that header's rule.
 *
 * The size query is host arithmetic (no GPU needed): an upper bound on the plan buffer for the directions `flags` asks for.
 * A negative count, S < 1, G that does not divide S or a flag that is not the build's: RLAP_E_BAD_ARG; m, S, num_nodes or
 * (S / G) num_nodes beyond the limits of rlap_snapshot_propagate: RLAP_E_TOO_LARGE.
 *
 * The build takes d_sc .. num_nodes, RLAP_GCN_WEIGHTED / SELF_LOOPS / NORMALIZE and fill_value exactly as rlap_snapshot_gcn_norm,
 * checks and error codes included, and
 *   RLAP_PLAN_FORWARD, RLAP_PLAN_TRANSPOSED : the directions to build; with neither, both
 *   d_plan, plan_bytes : the buffer (256-byte aligned) and its size, at least what the size query says (else RLAP_E_BAD_ARG)
 *   h_desc             : what a planned call needs without looking at the device; zeroed on any error (d_plan is then unspecified)
 *   h_info             : (nullable) what the build did
 * Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small); one host synchronisation.
 *
 * The planned call takes RLAP_SPMM_TRANSPOSE, RLAP_SPMM_X_F32 and RLAP_SPMM_X_PER_LAYER; d_x, F, d_y and the limits are those of
 * rlap_snapshot_propagate.  It does not read d_sc.  A direction the plan does not hold, or a descriptor that is not a successful
 * build's: RLAP_E_BAD_ARG before anything is launched.  No host synchronisation (every data-dependent error was found by the
 * build).  Arena: the chunk sums alone, by the budget rule and test hook of rlap_snapshot_propagate.  A buffer altered after the
 * build is the caller's error; the kernels clamp every id and offset they read from it, so it gives wrong numbers, never an access
 * out of range. */
enum { RLAP_PLAN_FORWARD = 256, RLAP_PLAN_TRANSPOSED = 512 };
typedef struct {
    int64_t m, segments, graphs, num_nodes;               /* the build's m, S, G (1 without node_ptr), num_nodes  */
    double fill_value;
    int64_t entries_forward, entries_transposed;          /* records of a direction (-1: not built)               */
    int64_t chunks_forward, chunks_transposed;            /* chunks of its lists longer than one chunk            */
    int64_t loop_offset;                                  /* byte offsets of the parts within the buffer          */
    int64_t off_forward, dir_forward, rec_forward;
    int64_t off_transposed, dir_transposed, rec_transposed;
    int64_t plan_bytes;                                   /* bytes of the buffer in use (the rest may be trimmed) */
    int32_t flags;                                        /* the build's flags, both direction bits resolved      */
    int32_t magic;                                        /* marks a successful build                             */
} rlap_plan_desc;
typedef struct {
    int64_t entries;                  /* entries of the list the products run over (rows that stay + loops)  */
    int64_t blocks;                   /* column blocks of the call: the ids with rows                         */
    int64_t chunked_lists_forward;    /* lists longer than one chunk (-1: direction not built)                */
    int64_t chunked_lists_transposed;
    int64_t loops_removed;            /* loop rows of the input that left the lists                           */
    int64_t arena_bytes;              /* scratch bytes of the call                                            */
    int32_t host_syncs;               /* host synchronisations of the call                                    */
    int32_t pad;
} rlap_plan_info;

int rlap_snapshot_plan_bytes(int64_t m, int64_t S, int64_t G, int64_t num_nodes, int flags, size_t* bytes);
int rlap_snapshot_plan_build(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                             int64_t G, int64_t num_nodes, int flags, double fill_value, void* d_plan, size_t plan_bytes,
                             rlap_plan_desc* h_desc, rlap_plan_info* h_info);
int rlap_snapshot_plan_propagate(rlap_handle h, const void* d_plan, const rlap_plan_desc* h_desc, int flags, const void* d_x, int64_t F,
                                 void* d_y, rlap_spmm_info* h_info);

/* Propagation plans for rows in ANY order: the arguments, the flags, the descriptor and the info of
 * rlap_snapshot_plan_build, for an input that need not be an elimination result -- a plain COO edge list, the (out, pptr) of
 * rlap_snapshot_ppr, a subgraph result.  The rows of a segment may come in any order; duplicate rows, directed structure, loop rows
 * and ids without rows are legal.  Row id is the source, column id the target.  The plan has the layout of the build above, so the
 * size query above is its bound and every planned call runs on it unchanged.  What the lists hold depends on a row's place in the
 * input alone (rlap_amd/csrc/rlap_edgeplan.h): the forward list of (layer, j) is the rows with target j in input order, the
 * transposed list of (layer, i) the rows with source i in input order; the degree of (layer, j) is summed over the forward list in
 * the fixed order of rlap_snapshot_gcn_norm, the loop's weight (that of the list's last loop row, or fill_value) last; an id
 * without incoming rows has the loop's weight alone, or degree 0.  For an input in the elimination layout the buffer equals
 * rlap_snapshot_plan_build's bit for bit, both directions.
 *   h_info->blocks : the non-empty forward lists
 *   h_desc         : zeroed on every refusal
 * An id that is not an integer of its graph's range [node_ptr[g], node_ptr[g+1]) (or [0, num_nodes)): RLAP_E_INDEX_RANGE; with
 * RLAP_GCN_WEIGHTED and RLAP_GCN_NORMALIZE a weight that is not finite or <= 0, a bad ptr / node_ptr, a buffer below the size query:
 * RLAP_E_BAD_ARG.  Limits: m < 2^31 - 1 and (S / G) num_nodes < 2^31 (RLAP_E_TOO_LARGE, never truncated).  Scratch from the arena
 * (two stable sorts of (slot, row) by rocPRIM; RLAP_E_WORKSPACE when a caller-provided one is too small); one host synchronisation;
 * no atomic on a floating-point value: the same input gives the same bits. */
int rlap_edge_plan_build(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                         int64_t G, int64_t num_nodes, int flags, double fill_value, void* d_plan, size_t plan_bytes,
                         rlap_plan_desc* h_desc, rlap_plan_info* h_info);

/* The sparse first layer: feature plans with per-view column masks.  A dense row-major (N, Fin) feature matrix x --
 * bag-of-words rows, the same in every step of a run -- is turned once into lists, and every step's (x * keep[k]) @ W for K views
 * and dW = sum_k keep[k] * (x^T G[k]) run over them; the masked copies of x never exist.  The rules are
 * rlap_amd/csrc/rlap_featlin.h's: an entry is kept iff (double)x[i][j] != 0.0 (-0.0 is dropped, NaN and infinities stay), its
 * coefficient is that double; the forward list of row i holds its entries by ascending j, the transposed list of column j by
 * ascending i; a forward value sums the list's chunks of 256 (cut by position in the full list) from 0.0 in list order, an entry
 * whose column the view drops adding nothing, then the chunk sums in chunk order; a transposed value adds, for the views that keep
 * the column in view order, the list's sum by rlap_spmm.h's rule; float64 sums, rounded once, no atomic on a float: the same bits
 * on every run.  The plan is a device buffer that the CALLER owns plus the host descriptor below; per direction it holds an int64
 * offset table, a directory of the chunks of the lists longer than 256 entries and 16-byte records {double coefficient, int32 id,
 * int32 0}, every part 256-byte aligned.  It does not depend on d_x after the build.
 *
 *   rlap_feature_count      : the kept entries of d_x ((N, Fin) row-major; float32 with RLAP_FEAT_X_F32, else float64) to *h_nnz.
 *                             One host synchronisation.
 *   rlap_feature_plan_bytes : host arithmetic (no GPU needed): the bytes of a plan buffer for the directions `flags` asks for
 *                             (RLAP_PLAN_FORWARD / RLAP_PLAN_TRANSPOSED; with neither, both).  A negative count, N < 1 or Fin < 1:
 *                             RLAP_E_BAD_ARG; N or Fin >= 2^31 or nnz >= 2^31 - 1: RLAP_E_TOO_LARGE.
 *   rlap_feature_plan_build : builds the directions asked for into d_plan (256-byte aligned, at least the size query's bytes).
 *                             Forward by a count per row, a scan and a ranked fill, transposed by counts per (column, block of
 *                             rows), a scan and a fill in row order: deterministic, no atomic on the lists.  Scratch from the arena
 *                             (RLAP_E_WORKSPACE when a caller-provided one is too small).  One host synchronisation, which reads
 *                             back the recount: a count that differs from nnz gives RLAP_E_BAD_ARG.  h_desc is zeroed on every
 *                             refusal.  h_info (nullable): nnz, the longest list, the long lists and their chunks per direction
 *                             (-1: not built).
 *   rlap_feature_plan_apply : forward: d_w is W (Fin, Fout), d_out is y (K, N, Fout).  With RLAP_SPMM_TRANSPOSE: d_w is G
 *                             (K, N, Fout), d_out is dW (Fin, Fout).  RLAP_SPMM_X_F32: float32 operands and result, else float64.
 *                             d_keep is uint8 (K, Fin), non-zero = kept, or NULL (K must be 1; everything is kept).  K in 1..32,
 *                             Fout >= 1.  No host synchronisation.  A direction the plan lacks, a descriptor that is not a
 *                             successful build's, a bad K or flag: RLAP_E_BAD_ARG before any launch; Fout or the elements of an
 *                             operand beyond the limits of rlap_snapshot_propagate: RLAP_E_TOO_LARGE.  Arena: the columns' keep
 *                             words and (transposed) the chunk sums, by the budget rule and test hook of
 *                             rlap_snapshot_propagate.  The kernels clamp every id and offset they read from the buffer: an
 *                             altered buffer gives wrong numbers, never an access out of range. */
enum { RLAP_FEAT_X_F32 = 1 };
typedef struct {
    int64_t num_nodes, in_features, nnz;                  /* the build's N, Fin and kept entries                  */
    int64_t chunks_forward, chunks_transposed;            /* chunks of the lists longer than one chunk (-1: not built) */
    int64_t off_forward, dir_forward, rec_forward;        /* byte offsets of the parts within the buffer (-1)     */
    int64_t off_transposed, dir_transposed, rec_transposed;
    int64_t plan_bytes;                                   /* bytes of the buffer                                  */
    int32_t flags;                                        /* RLAP_FEAT_X_F32 and both direction bits, resolved    */
    int32_t magic;                                        /* marks a successful build                             */
} rlap_feature_desc;
typedef struct {
    int64_t nnz;                                          /* kept entries                                         */
    int64_t longest_forward, longest_transposed;          /* entries of the longest list (-1: not built)          */
    int64_t long_lists_forward, long_lists_transposed;    /* lists longer than one chunk                          */
    int64_t chunks_forward, chunks_transposed;            /* their chunks                                         */
    int64_t arena_bytes;                                  /* scratch bytes of the call                            */
    int32_t host_syncs;                                   /* host synchronisations of the call                    */
    int32_t pad;
} rlap_feature_info;

int rlap_feature_count(rlap_handle h, const void* d_x, int64_t N, int64_t Fin, int flags, int64_t* h_nnz);
int rlap_feature_plan_bytes(int64_t N, int64_t Fin, int64_t nnz, int flags, size_t* bytes);
int rlap_feature_plan_build(rlap_handle h, const void* d_x, int64_t N, int64_t Fin, int64_t nnz, int flags, void* d_plan, size_t plan_bytes,
                            rlap_feature_desc* h_desc, rlap_feature_info* h_info);
int rlap_feature_plan_apply(rlap_handle h, const void* d_plan, const rlap_feature_desc* h_desc, int flags, const void* d_w,
                            const uint8_t* d_keep, int64_t K, int64_t Fout, void* d_out, rlap_feature_info* h_info);

/* Centrality-adaptive edge dropping, K views a call: the uniform, degree, PageRank and eigenvector edge-dropping
 * augmentors of GCA as the training scripts use them, on the device.  The centrality is found once and serves every view; row e is
 * kept in view k iff u(k, e) >= q(k, e), a counter-based coin against the drop probability.  Every rule -- counts, centralities,
 * scores, probability, coin and the order of every sum -- is defined in rlap_amd/csrc/rlap_edgedrop.h.
 *   d_src, d_dst, E    : the rows (source, target), int64 on the device, in any order; duplicates, loops and directed rows stay
 *   d_w                : (nullable) one weight a row, carried to the output and never read for the scores; NULL: 1.0
 *   num_nodes          : every id lies in [0, num_nodes)
 *   scheme             : RLAP_DROP_UNIFORM (q = p), _DEGREE, _PAGERANK, _EIGENVECTOR
 *   flags              : RLAP_DROP_SOURCE: counts and scores by a row's source; default by its target
 *   h_p, K             : K drop parameters in [0, 1] ON THE HOST, 1 <= K <= 32; view k uses h_p[k] and seed + k
 *   threshold          : the cap of every drop probability, in [0, 1]
 *   pr_damp, pr_iters  : PageRank: the damping in [0, 1] and the number of steps
 *   evc_tol, evc_max_iter : eigenvector: stops after the step with sum |x' - x| <= num_nodes * evc_tol, or after evc_max_iter steps
 *   d_rows, out_cap_rows  : (out_cap_rows, 3) f64 rows [source, target, weight], view-major, input order inside a view
 *   d_ptr              : [K+1] row offsets of the views in d_rows
 *   d_mask             : (nullable) (K, E) bytes: 1 where the row is kept
 *   d_centrality, d_node_weight : (nullable) [num_nodes] f64 (zeros for RLAP_DROP_UNIFORM or E = 0)
 *   h_info             : (nullable) what the call did; iters / converged report the eigenvector iteration
 * View k of a K-view call equals a one-view call with (h_p[k], seed + k); the same input gives the same bits; no atomic touches a
 * floating-point value.  More kept rows than out_cap_rows: RLAP_E_OUT_CAPACITY, no row written, h_info->rows_needed says how many.
 * An id outside [0, num_nodes): RLAP_E_INDEX_RANGE.  A null pointer, K < 1, a parameter out of its range, an unknown scheme or flag:
 * RLAP_E_BAD_ARG.  E >= 2^31 - 1, num_nodes >= 2^31, K > 32 or more than 100,000 steps: RLAP_E_TOO_LARGE, never truncated.  Scratch
 * from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small); one host synchronisation. */
enum { RLAP_DROP_UNIFORM = 0, RLAP_DROP_DEGREE = 1, RLAP_DROP_PAGERANK = 2, RLAP_DROP_EIGENVECTOR = 3 };
enum { RLAP_DROP_SINK = 0, RLAP_DROP_SOURCE = 1 };
typedef struct {
    int64_t rows_needed;      /* kept rows of all views: the rows of d_rows (written, or needed)      */
    int64_t launches;         /* kernels the call enqueued                                            */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t iters;            /* steps of the iteration (eigenvector: until it stopped)               */
    int32_t converged;        /* eigenvector: whether the stopping rule held within evc_max_iter      */
    int32_t host_syncs;       /* host synchronisations of the call                                    */
    int32_t pad;
} rlap_edge_drop_info;

int rlap_edge_drop(rlap_handle h, const int64_t* d_src, const int64_t* d_dst, const double* d_w, int64_t E, int64_t num_nodes, int scheme,
                   int flags, const double* h_p, int64_t K, double threshold, uint64_t seed, double pr_damp, int64_t pr_iters,
                   double evc_tol, int64_t evc_max_iter, double* d_rows, int64_t out_cap_rows, int64_t* d_ptr, uint8_t* d_mask,
                   double* d_centrality, double* d_node_weight, rlap_edge_drop_info* h_info);

/* Node dropping and random-walk subgraph views, K views a call: PyGCL's NodeDropping and RWSampling as the training
 * scripts use them, on the device.  A view is a node set -- drop: node v stays iff its coin u_node(k, v) >= p[k]; walk: every node
 * that num_seeds[k] uniform random walks of walk_length steps visit, starts included -- and row e is in view k iff its source and
 * its target are both in the set; ids are not relabelled.  Every rule -- both coins, the pick, a step of a walk -- is defined in
 * rlap_amd/csrc/rlap_nodesample.h.
 *   d_src, d_dst, E    : the rows (source, target), int64 on the device, in any order; duplicates, loops and directed rows stay
 *   d_w                : (nullable) one weight a row, carried to the output and never read otherwise; NULL: 1.0
 *   num_nodes          : every id lies in [0, num_nodes)
 *   scheme             : RLAP_SAMPLE_DROP or RLAP_SAMPLE_WALK
 *   h_p                : drop: K drop probabilities in [0, 1] ON THE HOST (walk: not read, may be NULL)
 *   h_num_seeds        : walk: K walker counts in [0, 2^31) ON THE HOST (drop: not read, may be NULL)
 *   K                  : 1 <= K <= 32; view k uses h_p[k] or h_num_seeds[k], and seed + k
 *   walk_length        : walk: steps of a walk, in [0, 1024]; a walker on a node without outgoing rows stays there
 *   d_rows, out_cap_rows  : (out_cap_rows, 3) f64 rows [source, target, weight], view-major, input order inside a view
 *   d_ptr              : [K+1] row offsets of the views in d_rows
 *   d_node_mask        : (nullable) (K, num_nodes) bytes: 1 where the node is in the view's set
 *   d_walks            : (nullable, walk only) (sum of h_num_seeds, walk_length + 1) int64: the walks, view-major
 *   h_info             : (nullable) what the call did
 * View k of a K-view call equals a one-view call with (h_p[k] or h_num_seeds[k], seed + k); the same input gives the same bits; the
 * only atomics are integer ORs into a bitmap.  More kept rows than out_cap_rows: RLAP_E_OUT_CAPACITY, no row written,
 * h_info->rows_needed says how many.  An id outside [0, num_nodes): RLAP_E_INDEX_RANGE.  A null pointer, K < 1, a parameter out of
 * its range, an unknown scheme, d_walks with drop, walkers without nodes: RLAP_E_BAD_ARG.  E >= 2^31 - 1, num_nodes >= 2^31, K > 32
 * or a walker count >= 2^31: RLAP_E_TOO_LARGE, never truncated.  Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one
 * is too small); one host synchronisation. */
enum { RLAP_SAMPLE_DROP = 0, RLAP_SAMPLE_WALK = 1 };
typedef struct {
    int64_t rows_needed;      /* kept rows of all views: the rows of d_rows (written, or needed)      */
    int64_t launches;         /* kernels the call enqueued                                            */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call                                    */
    int32_t pad;
} rlap_node_sample_info;

int rlap_node_sample(rlap_handle h, const int64_t* d_src, const int64_t* d_dst, const double* d_w, int64_t E, int64_t num_nodes, int scheme,
                     const double* h_p, const int64_t* h_num_seeds, int64_t K, int64_t walk_length, uint64_t seed, double* d_rows,
                     int64_t out_cap_rows, int64_t* d_ptr, uint8_t* d_node_mask, int64_t* d_walks, rlap_node_sample_info* h_info);

/* Edge adding, K views a call: the EdgeAdding augmentor of the training scripts (scripts/augmentor_benchmarks.py:44-65)
 * on the device.  View k adds h_num_add[k] rows whose two ends are drawn uniformly from [0, num_nodes - 2] -- the scripts'
 * torch.randint(0, num_nodes - 1, ...) has an exclusive upper end, so the last node never receives an added row; restated as it
 * stands -- and, with RLAP_ADD_COALESCE, holds the distinct (source, target) pairs of the input and the added rows, ascending by
 * (source, target), the order of sort_edge_index and coalesce.  Every rule -- the coin, the draw, the key of a pair, the tie rule of
 * the merge and the weight -- is defined in rlap_amd/csrc/rlap_edgeadd.h.
 *   d_src, d_dst, E    : the rows (source, target), int64 on the device, in any order; duplicates, loops and directed rows allowed
 *   d_w                : (nullable) one weight a row; NULL: 1.0
 *   num_nodes          : every id lies in [0, num_nodes); at least 2 where a row is added
 *   h_num_add, K       : K counts >= 0 ON THE HOST, 1 <= K <= 32: the rows view k adds (the caller's int(E * ratio)); view k uses
 *                        h_num_add[k] and seed + k
 *   flags              : RLAP_ADD_COALESCE: sort and merge.  A pair's weight is s_in + (double)c_add: s_in the sum of its input
 *                        rows from 0.0 in input order (0.0 without one), c_add the number of its added rows.  Without the flag view
 *                        k is the E rows in input order, then its added rows in draw order with weight 1.0 (CCA-SSG's add_edge).
 *   d_rows, out_cap_rows : (out_cap_rows, 3) f64 rows [source, target, weight], view-major; K * E + sum(h_num_add) always suffices
 *   d_ptr              : [K+1] row offsets of the views in d_rows
 *   d_added, d_aptr    : (nullable, both or neither; d_added may be null where nothing is added) (sum of h_num_add, 2) int64: the
 *                        added pairs in draw order, view-major, and their [K+1] offsets
 *   h_info             : (nullable) what the call did
 * View k of a K-view call equals a one-view call with (h_num_add[k], seed + k); the same input gives the same bits; no atomic touches
 * a floating-point value.  With RLAP_ADD_COALESCE the input is sorted at most once a call, whatever K is (one stable rocPRIM sort of
 * (key, row)), and not at all when its keys already ascend (h_info->input_sorted); the added rows' keys are sorted once for all views
 * where the view number fits beside the key in 63 bits, once a view otherwise (h_info->sorts counts every sort).  One host
 * synchronisation: the call is enqueued for ascending keys and read back once; for an input that is not ascending that read-back
 * holds the row total all the same (counted through a set of the input's keys), and the sort and the rows follow on the handle's
 * stream without another read-back: d_rows is complete in stream order, as the results of the calls that do not synchronise are.
 * More rows than out_cap_rows: RLAP_E_OUT_CAPACITY, no row written, h_info->rows_needed says how many.  An id outside
 * [0, num_nodes): RLAP_E_INDEX_RANGE.  A null pointer, K < 1, a negative count, an unknown flag, one of d_added / d_aptr without the
 * other, num_nodes < 2 with a row to add: RLAP_E_BAD_ARG.  E + max(h_num_add) >= 2^31 - 1, num_nodes >= 2^31 or K > 32:
 * RLAP_E_TOO_LARGE, never truncated.  Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small). */
enum { RLAP_ADD_COALESCE = 1 };
typedef struct {
    int64_t rows_needed;      /* rows of all views: the rows of d_rows (written, or needed)           */
    int64_t added;            /* added rows of all views: sum(h_num_add)                              */
    int64_t input_distinct;   /* distinct (source, target) pairs of the input (coalesce only)         */
    int64_t launches;         /* kernels the call enqueued                                            */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t input_sorted;     /* coalesce: 1 when the input's keys ascended, so no sort of the input  */
    int32_t sorts;            /* rocPRIM sorts the call enqueued                                      */
    int32_t host_syncs;       /* host synchronisations of the call                                    */
    int32_t pad;
} rlap_edge_add_info;

int rlap_edge_add(rlap_handle h, const int64_t* d_src, const int64_t* d_dst, const double* d_w, int64_t E, int64_t num_nodes,
                  const int64_t* h_num_add, int64_t K, uint64_t seed, int flags, double* d_rows, int64_t out_cap_rows, int64_t* d_ptr,
                  int64_t* d_added, int64_t* d_aptr, rlap_edge_add_info* h_info);

/* Per-graph readout of batched node embeddings: y[l, g, :] = the sum (or mean) of x[l, i, :] over the ids i of graph g,
 * [node_ptr[g], node_ptr[g+1]) -- what global_add_pool(z, batch) does after every GIN layer of a graph-level step, without float
 * atomics and in a fixed order.
 *   d_x, L, num_nodes, F : the embeddings (L, num_nodes, F), row-major, float64 or (RLAP_READOUT_X_F32) float32; L >= 0, F >= 1
 *   d_node_ptr, G        : [G+1] offsets on the device, G >= 1: non-decreasing from 0 to num_nodes (the caller's to check)
 *   flags                : RLAP_READOUT_MEAN divides the sum by the graph's number of ids; RLAP_READOUT_X_F32
 *   d_y                  : (L, G, F) of d_x's type; every element is written
 *   h_info               : (nullable) what the call did
 * One element is the rule of rlap_amd/csrc/rlap_spmm.h on the list of the graph's ids in increasing order, every coefficient 1.0, no
 * loop term: float64 terms, chunks of 256 ids summed from 0 in id order, the chunk sums added to 0 in chunk order; the mean is that
 * sum divided once, in float64, by the count; an empty graph gives exactly 0 for both; a float32 result is the float64 value rounded
 * once; values that are not finite pass through as the arithmetic gives them.  So the same input gives the same bits, and a graph's
 * result does not depend on L, on F's tiling, on the other graphs of the call or on what d_y or the arena held.
 * The backward call is the gradient with respect to d_x: d_gx[l, i, :] = d_gy[l, g(i), :], for the mean divided by the count of g(i)
 * (one float64 division, rounded once for float32); d_gy is (L, G, F), d_gx (L, num_nodes, F), every element of it is written.
 * Neither call synchronises with the host.  The work of the forward call is mapped to (graph, chunk) on the device; its grid is sized
 * from the bound ceil(num_nodes / 256) + G chunks.  h_info->chunks and ->chunked_graphs (graphs of more than 256 ids, whose chunk
 * sums go through the arena) are EXACT when G == 1, where the host knows them from num_nodes; otherwise they are the host's BOUNDS,
 * ceil(num_nodes / 256) + G and min(G, num_nodes / 257): the table is never read back.  As for the plans, the table is the caller's
 * to get right: the kernels clamp what they read from it before it becomes an address, so a table that is not well formed gives wrong
 * numbers, never an access out of range.
 * A negative count, F < 1, G < 1, a null pointer or a flag that is not this call's: RLAP_E_BAD_ARG.  F, L * num_nodes, L * G or the
 * elements of d_x or d_y beyond the limits of rlap_snapshot_propagate: RLAP_E_TOO_LARGE.  Scratch of the forward call from the arena
 * (RLAP_E_WORKSPACE when a caller-provided one is too small, rlap_workspace_needed() saying how much). */
enum { RLAP_READOUT_MEAN = 1, RLAP_READOUT_X_F32 = 32 };
typedef struct {
    int64_t rows;             /* num_nodes                                                            */
    int64_t graphs;           /* G                                                                    */
    int64_t chunks;           /* chunks of the call: exact when G == 1, else the bound                */
    int64_t chunked_graphs;   /* graphs of more than one chunk: exact when G == 1, else the bound     */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
    int32_t pad;
} rlap_readout_info;

int rlap_graph_readout(rlap_handle h, const void* d_x, int64_t L, int64_t num_nodes, int64_t F, const int64_t* d_node_ptr, int64_t G,
                       int flags, void* d_y, rlap_readout_info* h_info);
int rlap_graph_readout_backward(rlap_handle h, const void* d_gy, int64_t L, int64_t num_nodes, int64_t F, const int64_t* d_node_ptr,
                                int64_t G, int flags, void* d_gx, rlap_readout_info* h_info);

/* The fused InfoNCE contrastive loss of two views' node embeddings, forward and backward: what
 * DualBranchContrast(InfoNCEBatched(tau), mode="L2L") computes for one direction, without the N x N similarity matrix.
 *   d_a, d_b, N, F : anchor and sample embeddings, (N, F) float32 row-major; N >= 1, 1 <= F <= 512
 *   tau            : the temperature, in [1/32, 1024]
 *   flags          : RLAP_INFONCE_POSITIVE_RAW takes the positive term as s_ii (the reference's InfoNCEBatched, which does not divide
 *                    it by tau); without it the term is s_ii / tau (GCL's InfoNCE)
 *   forward        : d_loss one double; d_rows [N] doubles, the row terms c s_ii - 1/tau - log Z_i; d_z [N] doubles, the row sums
 *                    Z_i = sum_j exp((s_ij - 1) / tau), which the backward call reads
 *   backward       : d_z as the forward call left it; d_g the upstream gradient, one double ON THE DEVICE (so that no
 *                    synchronisation is needed); d_ga, d_gb (N, F) float32, the gradients with respect to d_a and d_b
 *   h_info         : (nullable) what the call did
 * The positive of row i is column i; every column, the positive included, is in the denominator.  Every value and the order of every
 * sum are defined in rlap_amd/csrc/rlap_infonce.h: rows normalised in float64 and rounded once; s_ij the float32 fmaf chain over the
 * columns in increasing order (what the f32 matrix-core instruction computes); a float32 exponential written out there; Z_i summed in
 * float64 in an order that depends on N alone; the loss summed by the chunk rule of rlap_amd/csrc/rlap_spmm.h.  The backward call
 * recomputes the similarities with the same chain.  So the same input gives the same bits, whatever the arena held; no atomic
 * touches a floating-point value; neither call synchronises with the host; memory is O(N F): the similarities are never stored.
 * Features that are not finite are not looked for (that would cost a synchronisation): they give a NaN loss, as in torch.
 * tau outside its range (or not a number), N < 1, F < 1, a null pointer or a flag that is not this call's: RLAP_E_BAD_ARG.  F > 512 or
 * N >= 2^31: RLAP_E_TOO_LARGE.  Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small, the
 * workspace-needed query saying how much). */
enum { RLAP_INFONCE_POSITIVE_RAW = 1 };
typedef struct {
    int64_t rows;             /* N                                                                    */
    int64_t features;         /* F                                                                    */
    int64_t parts;            /* contiguous parts the column tiles are dealt into: a function of N    */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
    int32_t pad;
} rlap_infonce_info;

int rlap_infonce(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, double* d_loss,
                 double* d_rows, double* d_z, rlap_infonce_info* h_info);
int rlap_infonce_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags,
                          const double* d_z, const double* d_g, float* d_ga, float* d_gb, rlap_infonce_info* h_info);

/* The symmetric pair of the above: loss = 0.5 * (l(a, b) + l(b, a)), what DualBranchContrast(...) computes for both
 * directions, from ONE pass over the similarities: s(b, a) is the transpose of s(a, b) bit for bit, so the row sums Z_i (the
 * denominators of the first direction) and the column sums Zc_j (of the second) come from the same tiles, and the backward call folds
 * both directions into one weight e_ij (1 / Z_i + 1 / Zc_j): five N x N x F products a step where two calls of each of the above make ten.
 *   arguments      : as rlap_infonce / rlap_infonce_backward, except
 *   d_rows         : [2, N] doubles: c s_ii - 1/tau - log Z_i, then c s_jj - 1/tau - log Zc_j
 *   d_z            : [2, N] doubles: Z, then Zc; the backward call reads both
 *   d_ga, d_gb     : the gradients of the pair's loss with respect to d_a and d_b
 * The rule is rlap_amd/csrc/rlap_infonce.h's: Z_i as in rlap_infonce over a split of the column tiles of its own; Zc_j in float64 in
 * an order that depends on N alone (groups of row blocks, row blocks, the four 32-row tiles of a block, a stated tree over a tile's 32
 * rows).  The same input gives the same bits, whatever the arena held; no atomic touches a floating-point value; neither call
 * synchronises with the host; memory is O(N F).  The loss equals 0.5 * (rlap_infonce(a, b) + rlap_infonce(b, a)) up to the order of
 * the sums.  The refusals and statuses are rlap_infonce's. */
typedef struct {
    int64_t rows;             /* N                                                                    */
    int64_t features;         /* F                                                                    */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int64_t parts;            /* contiguous parts of the column tiles (forward): a function of N      */
    int64_t groups;           /* contiguous groups of the 128-row blocks (forward): a function of N   */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
    int32_t pad;
} rlap_infonce_pair_info;

int rlap_infonce_pair(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, double* d_loss,
                      double* d_rows, double* d_z, rlap_infonce_pair_info* h_info);
int rlap_infonce_pair_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags,
                               const double* d_z, const double* d_g, float* d_ga, float* d_gb, rlap_infonce_pair_info* h_info);

/* The four calls above with intraview negatives: DualBranchContrast(..., intraview_negs=True), the loss GRACE was
 * published with.  Row i of a view is contrasted with the rows of the other view and with rows of its own view:
 *   Z_i = sum_j exp((s(a_i, b_j) - 1) / tau) + sum over j in I(i) of exp((s(a_i, a_j) - 1) / tau)
 * (the pair: Zc_j likewise with the rows of b), the positive staying s(a_i, b_i).
 *   intraview      : RLAP_INFONCE_INTRA_MASKED -- I(i) is every j != i: GCL's InfoNCE under the sampler's masks;
 *                    RLAP_INFONCE_INTRA_ALL    -- I(i) is every j: the reference's InfoNCEBatched under the same sampler, which never
 *                    reads the masks and so counts the row's similarity with itself.
 *                    Any other value, 0 included: RLAP_E_BAD_ARG (the calls above are the ones without intraview negatives).
 *   other arguments: as the call of the same name without _intra; d_z holds the totals Z ([N]; the pair: [2, N], Z then Zc), so the
 *                    backward call needs nothing else from the forward one.  It takes the same flags and intraview.
 * The rule is rlap_amd/csrc/rlap_infonce.h's: the intraview sums run over the same parts and tiles as the row sum and follow it in
 * the float64 chain; the backward call folds the two directions of a view's own similarities (symmetric bit for bit) into one
 * weight and adds them to the same float32 chains, a part's tiles of the other view first, then the same tiles of the own view.  The
 * same input gives the same bits, whatever the arena held; no atomic touches a floating-point value; no call synchronises with
 * the host; memory is O(N F).  The refusals and statuses are rlap_infonce's. */
enum { RLAP_INFONCE_INTRA_MASKED = 1, RLAP_INFONCE_INTRA_ALL = 2 };

int rlap_infonce_intra(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, int intraview,
                       double* d_loss, double* d_rows, double* d_z, rlap_infonce_info* h_info);
int rlap_infonce_intra_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, int intraview,
                                const double* d_z, const double* d_g, float* d_ga, float* d_gb, rlap_infonce_info* h_info);
int rlap_infonce_pair_intra(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, int intraview,
                            double* d_loss, double* d_rows, double* d_z, rlap_infonce_pair_info* h_info);
int rlap_infonce_pair_intra_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, int intraview,
                                     const double* d_z, const double* d_g, float* d_ga, float* d_gb, rlap_infonce_pair_info* h_info);

/* The fused CCA-SSG loss of two views' node embeddings, forward and backward: the standardisation of
 * CCA-SSG/model.py and the loss of CCA-SSG/main.py.  With z = (h - mean_0(h)) / std_0(h) (unbiased), c = z1^T z2 / N,
 * c1 = z1^T z1 / N and c2 = z2^T z2 / N:  loss = -trace(c) + lambd * (||I - c1||_F^2 + ||I - c2||_F^2).
 *   d_a, d_b, N, F : the two views' embeddings, (N, F) float32 row-major; N >= 2, 1 <= F <= 512
 *   lambd          : the trade-off, finite and >= 0
 *   flags          : reserved, 0
 *   forward        : d_terms four doubles: loss, inv = -trace(c), dec1, dec2; d_colstat [4 F] doubles: the column means of d_a, their
 *                    deviations, the means of d_b, their deviations; d_gram [2 F F] float32: r1 = I - c1 and r2 = I - c2, rounded
 *                    from float64, exactly symmetric.  The backward call reads d_colstat and d_gram.
 *   backward       : d_colstat, d_gram as the forward call left them; d_g the upstream gradient, one double ON THE DEVICE (so that
 *                    no synchronisation is needed); d_ga, d_gb (N, F) float32, the gradients with respect to d_a and d_b
 *   h_info         : (nullable) what the call did
 * Every value and the order of every sum are defined in rlap_amd/csrc/rlap_cca.h: the column statistics in float64 in two passes;
 * the Gram sums as float32 fmaf chains over the nodes in increasing order (what the f32 matrix-core instruction computes), per part
 * of the rows, the parts a function of (N, F) alone and added in float64; the terms summed by the chunk rule of
 * rlap_amd/csrc/rlap_spmm.h.  The backward call standardises again and does not repeat the Gram products.  So the same input gives
 * the same bits, whatever the arena held; no atomic touches a floating-point value; neither call synchronises with the host.
 * A column of zero variance divides by zero, as in the reference: the loss and the gradients are then NaN, and the status is
 * RLAP_OK (looking for it would cost a synchronisation).  A null pointer, N < 2, F < 1, F > 512, a lambd that is negative or not
 * finite, or flags other than 0: RLAP_E_BAD_ARG.  N >= 2^31: RLAP_E_TOO_LARGE.  Scratch from the arena (RLAP_E_WORKSPACE when a
 * caller-provided one is too small, the workspace-needed query saying how much). */
typedef struct {
    int64_t rows;             /* N                                                                    */
    int64_t features;         /* F                                                                    */
    int64_t parts;            /* contiguous parts the rows are dealt into: a function of (N, F)       */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
    int32_t pad;
} rlap_cca_info;

int rlap_cca_loss(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, int flags, double* d_terms,
                  double* d_colstat, float* d_gram, rlap_cca_info* h_info);
int rlap_cca_loss_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, int flags,
                           const double* d_colstat, const float* d_gram, const double* d_g, float* d_ga, float* d_gb,
                           rlap_cca_info* h_info);

/* The fused Barlow Twins loss of two views' node embeddings, forward and backward: the published bt_loss of PyGCL's
 * L.BarlowTwins, restated (the package is not pinned).  With z = (h - mean_0(h)) / (std_0(h) + eps) (unbiased) and
 * c = z1^T z2 / N:  loss = sum_k (1 - c_kk)^2 + lambd * sum_{k != l} c_kl^2.
 *   d_a, d_b, N, F : the two views' embeddings, (N, F) float32 row-major; N >= 2, 1 <= F <= 512
 *   lambd          : the weight of the off-diagonal term, finite and >= 0
 *   eps            : added to the deviations, finite and >= 0
 *   flags          : RLAP_BT_NO_STANDARDIZE: z = h; no statistics are taken, d_colstat is neither written nor read (NULL is legal)
 *   forward        : d_terms three doubles: loss, on = sum_k (1 - c_kk)^2, off = sum_{k != l} c_kl^2; d_colstat [4 F] doubles: the
 *                    column means of d_a, their deviations, the means of d_b, their deviations; d_cross [F F] float32: c, row-major
 *                    (rows: the columns of d_a), rounded from float64.  The backward call reads d_colstat and d_cross.
 *   backward       : d_colstat, d_cross as the forward call left them; d_g the upstream gradient, one double ON THE DEVICE (so that
 *                    no synchronisation is needed); d_ga, d_gb (N, F) float32, the gradients with respect to d_a and d_b
 *   h_info         : (nullable) what the call did
 * Every value and the order of every sum are defined in rlap_amd/csrc/rlap_bt.h: the column statistics as in rlap_cca_loss; the
 * full, non-symmetric cross sums as float32 fmaf chains over the nodes in increasing order (what the f32 matrix-core instruction
 * computes), per part of the rows, the parts a function of (N, F) alone and added in float64; the terms summed by the chunk rule of
 * rlap_amd/csrc/rlap_spmm.h.  The backward call standardises again and does not repeat the cross product.  So the same input gives
 * the same bits, whatever the arena held; no atomic touches a floating-point value; neither call synchronises with the host.
 * Nothing is clamped: a column of zero variance has z = +0 when eps > 0 -- the loss is finite and that column of its gradient is
 * NaN -- and with eps = 0 its z is NaN, as in rlap_cca_loss: the terms, that column and the other view's whole gradient are NaN; the
 * status is RLAP_OK either way.  A null pointer, N < 2, F < 1,
 * F > 512, a lambd or an eps that is negative or not finite, or an unknown flag: RLAP_E_BAD_ARG.  N >= 2^31: RLAP_E_TOO_LARGE.
 * Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small, the workspace-needed query saying how much). */
enum { RLAP_BT_NO_STANDARDIZE = 1 };

typedef struct {
    int64_t rows;             /* N                                                                    */
    int64_t features;         /* F                                                                    */
    int64_t parts;            /* contiguous parts the rows are dealt into: a function of (N, F)       */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
    int32_t pad;
} rlap_bt_info;

int rlap_bt_loss(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, double eps, int flags,
                 double* d_terms, double* d_colstat, float* d_cross, rlap_bt_info* h_info);
int rlap_bt_loss_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, double eps, int flags,
                          const double* d_colstat, const float* d_cross, const double* d_g, float* d_ga, float* d_gb,
                          rlap_bt_info* h_info);

/* The fused dense layer, forward and backward: y = act(x W + b) in one pass over x -- the torch.nn.Linear and the
 * elementwise launches behind it of the encoders, the GIN layers' MLP and the projection heads -- and the gradients from (x, W, y, gy).
 *   d_x, M, Fin    : (M, Fin) float32 row-major; 1 <= M < 2^31, 1 <= Fin <= 512.  An (L, N, Fin) tensor is its M = L N rows.
 *   d_w, Fout      : the weight, (Fin, Fout) float32 row-major, or with RLAP_LINEAR_WEIGHT_OUT_IN (Fout, Fin) -- torch.nn.Linear's
 *                    layout, no transposed copy is needed on the host; 1 <= Fout <= 512
 *   d_b            : (nullable) the bias, (Fout,) float32
 *   act, alpha     : RLAP_LINEAR_ACT_NONE, _RELU or _ELU; alpha is ELU's, finite and > 0 (checked whatever act is)
 *   forward        : d_y (M, Fout) float32
 *   backward       : d_y as the forward call left it, d_gy the upstream gradient (M, Fout); results, each nullable (a null pointer
 *                    skips its kernels): d_gx (M, Fin), d_gw of d_w's layout, d_gb (Fout,)
 *   h_info         : (nullable) what the call did
 * Every value and the order of every sum are defined in rlap_amd/csrc/rlap_linear.h: x W and gy' W^T as float32 fmaf chains over
 * the inner index in increasing order (what the f32 matrix-core instruction computes), the bias, the activation and one rounding
 * applied to the accumulator in float64; the weight gradient as such chains over the rows per part, the parts a function of
 * (M, Fin, Fout) alone and added in float64; the bias gradient by the chunk rule of rlap_amd/csrc/rlap_spmm.h.  gy' = gy act'(y)
 * is formed wherever it is read and never stored.  So the same input gives the same bits, whatever the arena held and however the
 * pointers are aligned; no atomic touches a floating-point value; neither call synchronises with the host; x, y, gy and gx are
 * read and written in place -- only the weight is copied (padded) into the arena.
 * A null d_x, d_w, d_y (or d_gy), M < 1, a width outside [1, 512], an unknown act or flag, an alpha that is not finite and > 0:
 * RLAP_E_BAD_ARG.  M >= 2^31: RLAP_E_TOO_LARGE.  Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small,
 * the workspace-needed query saying how much). */
enum { RLAP_LINEAR_WEIGHT_OUT_IN = 1 };
enum { RLAP_LINEAR_ACT_NONE = 0, RLAP_LINEAR_ACT_RELU = 1, RLAP_LINEAR_ACT_ELU = 2 };

typedef struct {
    int64_t rows;             /* M                                                                    */
    int64_t fin;              /* Fin                                                                  */
    int64_t fout;             /* Fout                                                                 */
    int64_t parts;            /* parts the rows are dealt into for the weight gradient: a function of (M, Fin, Fout) */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
    int32_t pad;
} rlap_linear_info;

int rlap_linear_act(rlap_handle h, const float* d_x, int64_t M, int64_t Fin, int64_t Fout, const float* d_w, const float* d_b, int act,
                    double alpha, int flags, float* d_y, rlap_linear_info* h_info);
int rlap_linear_act_backward(rlap_handle h, const float* d_x, const float* d_w, const float* d_y, const float* d_gy, int64_t M, int64_t Fin,
                             int64_t Fout, int act, double alpha, int flags, float* d_gx, float* d_gw, float* d_gb,
                             rlap_linear_info* h_info);

/* The fused graph-to-local losses of node embeddings against graph summaries, forward and backward: one direction of
 * DualBranchContrast(JSD(), mode="G2L") and of BootstrapContrast(BootstrapLatent(), mode="G2L"), without the concatenated copy,
 * the dense (G, N) masks and the dense similarity matrix.  With s_ij = <h_i, g_j> and g(i) the graph of node i:
 *   JSD        positives (i, g(i)); negatives every (i, j) with j != g(i) when G >= 2, or s'_i = <neg_i, g_0> when G == 1;
 *              loss = mean_neg(softplus(s) - ln 2) - mean_pos(ln 2 - softplus(-s))
 *   bootstrap  loss = (sum_i cos(h_i, g_g(i))) / G, the sign as published: not negated; g is a constant
 *   d_h, N, F       : node embeddings (N, F) float32 row-major; N >= 1, 1 <= F <= 512
 *   d_neg           : JSD only: the embeddings of the corrupted input, (N, F); required when G == 1, NULL when G >= 2
 *   d_g, G          : graph summaries (G, F) float32; G >= 1
 *   d_node_ptr      : [G+1] offsets on the device, non-decreasing from 0 to N (the caller's to check): node i belongs to the graph
 *                     whose id range holds it; empty graphs and G > N are legal
 *   flags           : reserved, 0
 *   forward         : d_loss one double; d_rows doubles: JSD [2 N], the positive terms pos_i and then the negative sums neg_i;
 *                     bootstrap [N], the cosines c_i
 *   backward        : d_gup the upstream gradient, one double ON THE DEVICE (so that no synchronisation is needed); d_gh (N, F),
 *                     d_gneg (N, F) exactly when d_neg is given, d_gg (G, F): the gradients with respect to d_h, d_neg and d_g.
 *                     The bootstrap has a gradient for d_h alone.
 *   h_info          : (nullable) what the call did
 * Every value and the order of every sum are defined in rlap_amd/csrc/rlap_g2l.h: s_ij the float32 fmaf chain over the columns in
 * increasing order (what the f32 matrix-core instruction computes); softplus from rlap_infonce.h's float32 exponential and the
 * float64 log1p; neg_i summed in float64 in an order that depends on G alone, the positive and the padding left out of it; the losses
 * summed by the chunk rule of rlap_amd/csrc/rlap_spmm.h; dg summed per part of the nodes, the parts a function of (N, G, F) alone.
 * The bootstrap normalises rows as rlap_infonce does.  So the same input gives the same bits, whatever the arena held; no atomic
 * touches a floating-point value; no call synchronises with the host; the table is never read back: the kernels clamp what they read
 * from it before it becomes an address, so a table that is not well formed gives wrong numbers, never an access out of range.
 * Features that are not finite are not looked for: a score that is not finite gives a NaN loss.
 * A null pointer, N < 1, F < 1, G < 1, G == 1 without d_neg, G >= 2 with d_neg, or flags other than 0: RLAP_E_BAD_ARG.  F > 512, or
 * N or G >= 2^31: RLAP_E_TOO_LARGE.  Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small, the
 * workspace-needed query saying how much). */
typedef struct {
    int64_t rows;             /* N                                                                    */
    int64_t graphs;           /* G                                                                    */
    int64_t features;         /* F                                                                    */
    int64_t parts;            /* contiguous parts of the node tiles in dg: a function of (N, G, F)    */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
    int32_t pad;
} rlap_g2l_info;

int rlap_g2l_jsd(rlap_handle h, const float* d_h, const float* d_neg, const float* d_g, int64_t N, int64_t F, const int64_t* d_node_ptr,
                 int64_t G, int flags, double* d_loss, double* d_rows, rlap_g2l_info* h_info);
int rlap_g2l_jsd_backward(rlap_handle h, const float* d_h, const float* d_neg, const float* d_g, int64_t N, int64_t F,
                          const int64_t* d_node_ptr, int64_t G, int flags, const double* d_gup, float* d_gh, float* d_gneg, float* d_gg,
                          rlap_g2l_info* h_info);
int rlap_g2l_bootstrap(rlap_handle h, const float* d_h, const float* d_g, int64_t N, int64_t F, const int64_t* d_node_ptr, int64_t G,
                       int flags, double* d_loss, double* d_rows, rlap_g2l_info* h_info);
int rlap_g2l_bootstrap_backward(rlap_handle h, const float* d_h, const float* d_g, int64_t N, int64_t F, const int64_t* d_node_ptr,
                                int64_t G, int flags, const double* d_gup, float* d_gh, rlap_g2l_info* h_info);

/* The linear-probe evaluator on the device: R independent runs of LREvaluator's loop (scripts/node_shared.py:163-230) or
 * of CCA-SSG/main.py:152-194's in one call -- full-batch Adam on a Linear(F, C) under log-softmax + NLL, scored on a validation and a
 * test list, the selection rule applied on the device.
 *   d_x, N, F, ldx  : features (N, F) float32, row i at d_x + i * ldx (ldx >= F); 1 <= F <= 512; only read
 *   d_y, C          : [N] int64 labels in [0, C), 2 <= C <= 64
 *   R               : runs, 1 <= R <= 32
 *   d_train, h_train_ptr (and valid, test) : run r's list is d_*[h_*_ptr[r] .. h_*_ptr[r+1]), row indices in [0, N) ON THE DEVICE in
 *                     any order, a repeated row counting twice; the [R+1] offsets ON THE HOST, from 0, strictly increasing (no list
 *                     is empty)
 *   epochs, lr, weight_decay, beta1, beta2, eps : Adam with L2 weight decay; epochs >= 1, lr finite
 *   test_interval, select : RLAP_PROBE_SELECT_SCRIPTS scores after every epoch e (from 0) with (e + 1) % test_interval == 0 and records
 *                     the test scores when the validation count rises above the best so far; RLAP_PROBE_SELECT_CCA scores after every
 *                     epoch (test_interval is not read): when val >= best_val, best_val = val, and when test > best_test the test
 *                     scores are recorded.  Both compare integer counts of correct rows: the denominators are fixed, so below 2^24
 *                     rows this equals the reference's comparison of float32 ratios.
 *   d_weight0, d_bias0 : (R, C, F), (R, C) float32: the initial parameters, so the call is a pure function of its arguments
 *   d_weight, d_bias   : the final parameters (may be the initial buffers)
 *   d_scores        : (R, 4) doubles: micro-F1, macro-F1 and accuracy of the test list at the recorded evaluation, the last epoch's
 *                     training loss
 *   d_best          : (R, 2) int64: the recorded epoch and the best validation count
 *   d_confusion     : (R, 2, C, C) int64: validation and test at the recorded evaluation, rows true, columns predicted
 *   d_status        : one int32 ON THE DEVICE, valid once the stream has run: RLAP_OK, RLAP_E_INDEX_RANGE (an index outside [0, N): row
 *                     0 was read in its place) or RLAP_E_BAD_ARG (a label outside [0, C): the row marks no class and is not counted)
 *   h_info          : (nullable) what the call did; detail says which host-side check refused it (1 shape, 2 a list, 3 a parameter,
 *                     4 a pointer)
 * rlap_probe_scores is the scoring pass alone on one list per run: d_pred one int64 per listed row, d_confusion (R, C, C), d_scores
 * (R, 3): micro-F1, macro-F1, accuracy.
 * Every value and the order of every sum are defined in rlap_amd/csrc/rlap_probe.h: the logits and the gradient sums are float32 fmaf
 * chains (what the f32 matrix-core instruction computes), the gradient per part of the training list, the parts a function of (n, F,
 * C) alone and added in float64; the softmax with rlap_infonce.h's exponential; Adam operation by operation.  The parameter
 * trajectory holds IEEE operations only, so the same input gives the same bits, whatever the arena held; no atomic touches a
 * floating-point value; neither call synchronises with the host.  The scores are sklearn's accuracy_score and f1_score (micro, macro)
 * as the scripts call them, float64 functions of the integer counts.
 * A null pointer, N < 1, F < 1, C < 2, ldx < F, R < 1, an empty list or offsets that do not start at 0, epochs < 1, test_interval < 1,
 * an unknown select, an lr that is not finite, weight_decay < 0, a beta outside [0, 1), eps <= 0: RLAP_E_BAD_ARG.  F > 512, C > 64,
 * R > 32, N >= 2^31: RLAP_E_TOO_LARGE.  Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small, the
 * workspace-needed query saying how much). */
enum { RLAP_PROBE_SELECT_SCRIPTS = 0, RLAP_PROBE_SELECT_CCA = 1 };
typedef struct {
    int64_t runs;             /* R                                                                    */
    int64_t parts;            /* parts of the longest training list: a function of (n, F, C)          */
    int64_t launches;         /* kernels the call enqueued                                            */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
    int32_t detail;           /* the host-side check that refused the call, 0 otherwise               */
} rlap_probe_info;

int rlap_linear_probe(rlap_handle h, const float* d_x, int64_t N, int64_t F, int64_t ldx, const int64_t* d_y, int64_t C, int64_t R,
                      const int64_t* d_train, const int64_t* h_train_ptr, const int64_t* d_valid, const int64_t* h_valid_ptr,
                      const int64_t* d_test, const int64_t* h_test_ptr, int64_t epochs, double lr, double weight_decay,
                      int64_t test_interval, int select, double beta1, double beta2, double eps, const float* d_weight0,
                      const float* d_bias0, float* d_weight, float* d_bias, double* d_scores, int64_t* d_best, int64_t* d_confusion,
                      int32_t* d_status, rlap_probe_info* h_info);
int rlap_probe_scores(rlap_handle h, const float* d_x, int64_t N, int64_t F, int64_t ldx, const int64_t* d_y, int64_t C, int64_t R,
                      const int64_t* d_index, const int64_t* h_ptr, const float* d_weight, const float* d_bias, int64_t* d_pred,
                      int64_t* d_confusion, double* d_scores, int32_t* d_status, rlap_probe_info* h_info);

/* Per-view batch norm with fused activations, forward and backward: every layer l of d_x (L, N, F) is normalised over
 * its N rows with its own column statistics -- one BatchNorm1d call a view, as the reference's encoders make it -- with an optional
 * ReLU in front and a ReLU or PReLU behind in the same pass, and the running buffers updated once a layer, the layers in order.
 *   d_x, L, N, F   : (L, N, F) float32 row-major; L >= 1, 1 <= F <= 4096, N >= 2 in training mode (N >= 1 with RLAP_NORM_EVAL)
 *   d_weight, d_bias : (nullable) (F) float32; a null pointer means 1 and 0
 *   d_slope        : the PReLU slope, one float32 or (RLAP_NORM_SLOPE_PER_CHANNEL) (F); required with RLAP_NORM_POST_PRELU
 *   d_running_mean, d_running_var : (F) float32.  Training: nullable, updated on the device, rm = (float)((1 - momentum) rm +
 *                    momentum mean), rv the same with the unbiased variance, layer 0 first.  RLAP_NORM_EVAL: required, only read.
 *   momentum, eps  : momentum in [0, 1]; eps > 0 and finite
 *   flags          : RLAP_NORM_PRE_RELU; one of RLAP_NORM_POST_RELU / RLAP_NORM_POST_PRELU; RLAP_NORM_SLOPE_PER_CHANNEL; RLAP_NORM_EVAL
 *   d_y            : (L, N, F) float32; every element is written
 *   d_stat         : (L, 3, F) float64: the shift c (the layer's first row behind the front activation), m (mean = c + m) and
 *                    1 / sqrt(var + eps).  Written by a training call, read by its backward call; unused with RLAP_NORM_EVAL (nullable)
 *   h_info         : (nullable) what the call did
 * Every value and the order of every sum are defined in rlap_amd/csrc/rlap_norm.h: float64 throughout, the column sums by the
 * chunk rule of rlap_spmm.h over the rows in order, every output rounded once to float32.  So the same input gives the same bits,
 * and a layer's result does not depend on L, on the other layers or on what d_y or the arena held.  A column of zero variance
 * gives 1 / sqrt(eps), no NaN.  No atomic touches a floating-point value; neither call synchronises with the host.
 * The backward call reads d_x, the upstream d_gy (L, N, F) and the forward call's d_stat (training), and writes d_gx (L, N, F),
 * d_gweight (F), d_gbias (F) and d_gslope (1, or F per channel): the parameter gradients are summed over the layers in layer
 * order (the single slope then over the columns in order).  A null gradient output is skipped.
 * Both post flags, PReLU without a slope, RLAP_NORM_EVAL without both running buffers, N < 2 in training mode, F outside [1, 4096],
 * L < 1, eps or momentum out of range or not a number, a null d_x, d_y, d_gy or (training) d_stat, an unknown flag: RLAP_E_BAD_ARG
 * before anything is launched.  L * N * F >= 2^40: RLAP_E_TOO_LARGE.  Scratch from the arena (RLAP_E_WORKSPACE when a
 * caller-provided one is too small, the workspace-needed query saying how much). */
enum { RLAP_NORM_PRE_RELU = 1, RLAP_NORM_POST_RELU = 2, RLAP_NORM_POST_PRELU = 4, RLAP_NORM_SLOPE_PER_CHANNEL = 8, RLAP_NORM_EVAL = 16 };
typedef struct {
    int64_t rows;             /* N                                                                    */
    int64_t features;         /* F                                                                    */
    int64_t layers;           /* L                                                                    */
    int64_t chunks;           /* chunks of 256 rows a layer has                                       */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t vec;              /* 1: 16 bytes a lane (F % 4 == 0, pointers on the 16-byte grid); 0: one element a lane */
    int32_t launches;         /* kernels the call enqueued                                            */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
    int32_t pad;
} rlap_norm_info;

int rlap_batch_norm(rlap_handle h, const float* d_x, int64_t L, int64_t N, int64_t F, const float* d_weight, const float* d_bias,
                    const float* d_slope, float* d_running_mean, float* d_running_var, double momentum, double eps, int flags,
                    float* d_y, double* d_stat, rlap_norm_info* h_info);
int rlap_batch_norm_backward(rlap_handle h, const float* d_x, const float* d_gy, int64_t L, int64_t N, int64_t F, const float* d_weight,
                    const float* d_bias, const float* d_slope, const float* d_running_mean, const float* d_running_var, double eps,
                    int flags, const double* d_stat, float* d_gx, float* d_gweight, float* d_gbias, float* d_gslope,
                    rlap_norm_info* h_info);

/* Fused bias, activation and dropout, forward and backward: y = dropout(act(x + bias), p) on every element of d_x
 * (L, N, F) in one pass -- what the reference's encoders run behind every GCN and GIN layer as three torch passes.  No mask is
 * stored: the dropout coin is a function of (seed, layer, row, column, F, p) alone and the backward call draws it again.
 *   d_x, L, N, F   : (L, N, F) float32 row-major; L >= 1, N >= 1, 1 <= F <= 4096
 *   d_bias         : (nullable) (F) float32; a null pointer means 0
 *   d_slope        : the PReLU slope, one float32 or (RLAP_ROW_SLOPE_PER_CHANNEL) (F); required with RLAP_ROW_ACT_PRELU
 *   p, seed        : the drop probability, 0 <= p < 1, used as T / 65536 with T = llrint(p * 65536) (at most 65535); what is kept is
 *                    scaled by 1 / (1 - T / 65536).  Layer l of a call draws the coins of layer 0 of the call with seed + l.
 *   flags          : at most one of RLAP_ROW_ACT_RELU / RLAP_ROW_ACT_PRELU; RLAP_ROW_SLOPE_PER_CHANNEL (with PReLU only);
 *                    RLAP_ROW_TRAINING -- without it, or with T = 0, nothing is dropped and the call gives the bits of the call
 *                    without dropout
 *   d_y            : (L, N, F) float32; every element is written
 *   h_info         : (nullable) what the call did
 * Every value, the coin and the order of every sum are defined in rlap_amd/csrc/rlap_rowops.h: float64 throughout, every output
 * rounded once to float32.  So the same input gives the same bits, and a layer's result does not depend on L, on the lane path or on
 * what d_y or the arena held.  No atomic touches a floating-point value; neither call synchronises with the host.
 * The backward call reads d_x and the upstream d_gy (L, N, F) with the forward call's p, seed and flags, and writes d_gx (L, N, F),
 * d_gbias (F) and d_gslope (1, or F per channel; ignored without PReLU): the column sums by the chunk rule of rlap_spmm.h over the
 * rows in order, the layers added in layer order (the single slope then over the columns in order).  A null gradient output is
 * skipped; without d_gbias and d_gslope the call is one pass and takes no scratch.
 * Both activation flags, PReLU without a slope, the per-channel flag without PReLU, p outside [0, 1) or not a number, F outside
 * [1, 4096], L < 1, N < 1, a null d_x, d_y or d_gy, an unknown flag: RLAP_E_BAD_ARG before anything is launched.
 * L * N * F >= 2^40: RLAP_E_TOO_LARGE.  Scratch from the arena (RLAP_E_WORKSPACE when a caller-provided one is too small, the
 * workspace-needed query saying how much). */
enum { RLAP_ROW_ACT_RELU = 1, RLAP_ROW_ACT_PRELU = 2, RLAP_ROW_SLOPE_PER_CHANNEL = 4, RLAP_ROW_TRAINING = 8 };
typedef struct {
    int64_t rows;             /* N                                                                    */
    int64_t features;         /* F                                                                    */
    int64_t layers;           /* L                                                                    */
    int64_t chunks;           /* chunks of 256 rows a layer has                                       */
    int64_t arena_bytes;      /* scratch bytes of the call                                            */
    int32_t vec;              /* 1: 16 bytes a lane (F % 4 == 0, pointers on the 16-byte grid); 0: one element a lane */
    int32_t launches;         /* kernels the call enqueued                                            */
    int32_t instance;         /* layer norm: 16-byte steps a lane holds in registers (1, 2, 4, 8, 16); else 0 */
    int32_t host_syncs;       /* host synchronisations of the call: 0                                 */
} rlap_rowops_info;

int rlap_bias_act_dropout(rlap_handle h, const float* d_x, int64_t L, int64_t N, int64_t F, const float* d_bias, const float* d_slope,
                    double p, uint64_t seed, int flags, float* d_y, rlap_rowops_info* h_info);
int rlap_bias_act_dropout_backward(rlap_handle h, const float* d_x, const float* d_gy, int64_t L, int64_t N, int64_t F,
                    const float* d_bias, const float* d_slope, double p, uint64_t seed, int flags, float* d_gx, float* d_gbias,
                    float* d_gslope, rlap_rowops_info* h_info);

/* Per-row layer norm with a fused activation and dropout, forward and backward: every row of d_x (L, N, F) is
 * normalised over its F columns (biased variance, as torch.nn.LayerNorm), then y = dropout(act(xh * weight + bias), p) in the same
 * pass -- the other branch of the reference's Normalize, with the PReLU and the dropout that follow it.  A wave holds a row in
 * registers; the row is read once and d_y written once.
 *   d_weight, d_bias : (nullable) (F) float32; a null pointer means 1 and 0
 *   eps            : > 0 and finite; a constant row gives 1 / sqrt(eps), no NaN
 *   the other arguments, the flags, the coin and the refusals are rlap_bias_act_dropout's
 * The row sums run in an order that depends on F alone (rlap_amd/csrc/rlap_rowops.h: row_sum), on either lane path.  Nothing but d_x
 * is kept for the backward call, which forms mean and 1 / sqrt(var + eps) again from the row, writes d_gx and, where one of
 * d_gweight (F), d_gbias (F), d_gslope is asked for, a second pass over d_x and d_gy for their column sums by the chunk rule (the
 * rows' statistics go through the arena). */
int rlap_layer_norm(rlap_handle h, const float* d_x, int64_t L, int64_t N, int64_t F, const float* d_weight, const float* d_bias,
                    const float* d_slope, double eps, double p, uint64_t seed, int flags, float* d_y, rlap_rowops_info* h_info);
int rlap_layer_norm_backward(rlap_handle h, const float* d_x, const float* d_gy, int64_t L, int64_t N, int64_t F, const float* d_weight,
                    const float* d_bias, const float* d_slope, double eps, double p, uint64_t seed, int flags, float* d_gx,
                    float* d_gweight, float* d_gbias, float* d_gslope, rlap_rowops_info* h_info);

/* The op with the step BEFORE the path fused in (scripts/node_shared.py:326-327,
 * scripts/augmentor_benchmarks.py:77-78):
 *   symmetrize != 0 : the input holds every undirected edge in one or both directions; (b,a) is
 *                     added for every (a,b) and duplicates are folded inside the COO->CSR kernels
 *                     (PyG to_undirected + coalesce: an edge SET with unit weights when d_w is
 *                     NULL, summed weights otherwise).  out_cap_rows must allow 2*E rows.
 *   n < 0           : num_nodes = max id + 1, found on the device (one 8-byte read-back)
 *   t < 0           : num_remove = (int64)(remove_frac * num_nodes)
 *   h_num_nodes     : (nullable) the num_nodes used */
int rlap_approx_chol_from_edges(rlap_handle h, const int64_t* d_src, const int64_t* d_dst, const double* d_w, int64_t E,
                                int64_t n, int64_t t, double remove_frac, int symmetrize, int o_v, int o_n,
                                const int64_t* d_perm, uint64_t shuffle_seed, double* d_out, int64_t out_cap_rows,
                                int64_t* h_out_rows, int64_t* h_num_nodes, rlap_stats* h_stats);

/* Test hook: first-attempt limits for the next calls on this handle (negative = default): append-pool factor,
 * PQ-log factor, length of the uniform table the kernels may use, entries of the output pass's long-column
 * scratch.  A call that runs into one of them repeats itself with the regular sizes (rlap_stats.n_retries). */
int rlap_debug_set_limits(rlap_handle h, double pool_factor, double log_factor, int64_t rng_len, int64_t scratch_entries);

/* Test hook: entries of the dataflow kernel's reorder buffer (the tag order of the surviving columns) for the first attempt of the
 * next call on this handle (negative = default).  A call whose out-of-order appended entries do not fit repeats itself on the round
 * kernel (rlap_stats.retry_causes bit 7). */
int rlap_debug_set_flow_limits(rlap_handle h, int64_t reorder_cap);

/* Debug aid (also: environment RLAP_DEBUG_POISON=<byte> at rlap_create): before every attempt of the next calls the whole
 * workspace arena, the caller's output buffer and the elimination kernel's LDS are filled with `byte` (0..255; negative = off),
 * so that a kernel reading something it was never given reads that byte and not the previous call's (or the previous
 * workgroup's) data -- a stale read changes the result deterministically instead of once in a thousand runs. */
int rlap_debug_set_poison(rlap_handle h, int byte);

/* Debug aid (also: environment RLAP_DEBUG_JITTER=<n> at rlap_create): behind every workgroup barrier of the elimination kernel
 * a changing subset of the waves sleeps for n x 0.25 us (0 = off, at most 64).  A value that one wave reads behind a barrier while
 * another wave already rewrites it -- a race that needs a wave to fall a microsecond behind and otherwise shows once in some
 * thousand calls -- then shows in every call.  Results must not depend on it. */
int rlap_debug_set_jitter(rlap_handle h, int quarter_us);

/* First `count` uniforms of the sampling stream (default-seeded std::mt19937_64
 * through uniform_real_distribution<double>(0,1), preconditioner.cc:356-357)
 * as generated on the device; for known-answer tests. */
int rlap_rng_uniforms(rlap_handle h, int64_t count, double* d_out);

/* Test hook: the wave-parallel std::sort emulation used by the kernels, on `narr` arrays of doubles
 * (array a = d_keys[d_offs[a] .. d_offs[a+1]), each at most 512 long).  d_perm_out[d_offs[a]+i] = index of the
 * element that ends at position i; compared with libstdc++'s std::sort by tests/test_gpu_parity.py.
 * desc bit 0 = descending; bit 1 = arrays of at most 64 elements use the register-resident variant of the batch kernel;
 * bit 2 = the half-wave variant (arrays of at most 32 elements, two per wave; longer ones are left untouched);
 * bit 5 = the long-column sort of the dataflow elimination (rlap_flow.hip; any length up to 65000), bit 6 with it = records in global memory, bit 7 with it = 16-bit indices sorted in LDS (the form columns beyond 3,400 entries take);
 * bit 8 with it = the sort's duration in 10 ns ticks instead of the first index (timing tool); bit 9 with it = the keys are distinct
 * non-negative integers: the radix form the elimination uses where keys cannot repeat (ids of a column without multi-edges, tags). */
int rlap_debug_wave_sort(rlap_handle h, const double* d_keys, const int32_t* d_offs, int32_t narr, int32_t desc, int32_t* d_perm_out);

/* Host-side synthetic input (bench/tests): Barabasi-Albert graph as a symmetric,
 * coalesced COO sorted by (col,row).  Returns the directed entry count; call with
 * NULL arrays to size them (upper bound 2*m*(n-m)). */
int64_t rlap_util_ba_graph(int64_t n, int64_t m, uint64_t seed, int64_t* h_row, int64_t* h_col);

#ifdef __cplusplus
}
#endif
#endif
