/*
 * gsn_abi.h -- C ABI of libgsn_hip.so, the MI355X-native (gfx950) replacement for GSN's two data-parallel
 * hot paths.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * Each entry point cites the reference interface it replaces (paths relative to gbouritsas/GSN).  The
 * reference's "plugin API" for these paths is plain Python imports; INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns int: GSN_OK (0) or a negative GSN_E_* code; gsn_last_error() returns a thread-local
 *     message for the last failing call on this thread.  No C++ exception crosses the ABI.
 *   - the library never allocates or frees caller-visible memory: outputs and scratch are caller buffers
 *     (query sizes first).  Device entry points take device pointers plus `stream` (a hipStream_t passed as
 *     void*, e.g. torch.cuda.current_stream().cuda_stream) and are asynchronous on that stream.
 *   - host entry points (pattern analysis, plan building) are synchronous, re-entrant and thread-safe.
 *   - int64 index tensors are accepted as PyTorch hands them over (edge_index is int64 [2, E], row-major).
 */
#ifndef GSN_ABI_H
#define GSN_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSN_ABI_VERSION 1
#define GSN_KMAX 9 /* max pattern vertices the LDS-resident counting kernels handle: --k 8 of star_graph is a 9-vertex pattern (utils.py:59-62) */
#define GSN_KMAX_WIDE 16 /* max pattern vertices of a wide plan table (GSN_FLAG_WIDE; gsn_count_sparse_hip only) and of gsn_pattern_orbits */
#define GSN_SEG_RANGE_ROWS 16 /* rows one thread reduces in the fused scatter-add epilogue (see gsn_segsum_prepare_hip) */

enum {
    GSN_OK = 0,
    GSN_E_INVALID = -1,     /* bad argument */
    GSN_E_UNSUPPORTED = -2, /* valid in the reference but outside this build or this entry (e.g. k > GSN_KMAX without GSN_FLAG_WIDE; n > 768 in gsn_count_hip: INTEGRATION.md 11) */
    GSN_E_HIP = -3,         /* HIP runtime error (message has hipGetErrorString) */
    GSN_E_NOSPACE = -4,     /* caller buffer too small */
    GSN_E_NODEVICE = -5     /* no gfx950 device visible */
};

enum { GSN_MODE_VERTEX = 0, GSN_MODE_EDGE = 1 };

/* per-graph status written by gsn_count_hip into `status` (int32 per graph) */
enum {
    GSN_ST_OK = 0,
    GSN_ST_KEYERROR = 1, /* a match uses an edge direction that is not a column of edge_index: the reference raises
                            KeyError at utils_graph_processing.py:173 */
    GSN_ST_TOO_LARGE = 2, /* graph exceeds max_nodes / max_edges given to the call */
    GSN_ST_BAD_INDEX = 3, /* a vertex id outside [0, num_nodes) */
    GSN_ST_ASYMMETRIC = 4,     /* gsn_laplacian_eig_hip: the graph's arc set is not symmetric (A != A^T) */
    GSN_ST_NO_CONVERGENCE = 5, /* gsn_laplacian_eig_hip: not converged after max_sweeps sweeps (the rows hold the last iterate) */
    GSN_ST_UNSEEN = 6          /* gsn_lookup_codes_hip (strict): a value that is not among its column's fitted values */
};

/* gsn_lookup_codes_hip: what a value outside its column's fitted values becomes */
enum { GSN_LOOKUP_STRICT = 0, GSN_LOOKUP_CLAMP = 1 };

const char *gsn_last_error(void);
/* what the last propagate / segment-sum / CSR entry point called on this thread launched: "kernel<template arguments> grid=G" per launch,
 * joined by ';' (empty: nothing was launched).  Thread-local, valid until the next call on this thread; never fails.  The dispatch rules
 * of csrc/propagate.hip report from their launch sites, so a test can state which kernel a shape takes. */
const char *gsn_propagate_last_route(void);
int gsn_version(void);
/* number of visible gfx950 devices (0 if none / no driver); never fails */
int gsn_device_count(void);
/* 0 when `stream` is not being captured into a HIP graph, else an id unique to the capture (hipStreamGetCaptureInfo); never fails.
 * Host-side scratch that a launch sequence zero-fills is keyed on it (a fill recorded in one capture does not run in another). */
int64_t gsn_stream_capture_id(void *stream);
/* 64-bit content fingerprint of n device tensors, ADDED into *acc (device, caller-zeroed): meta (device int64) = n base pointers, then
 * n sizes in 4-byte words; max_words = the largest of them (sizes the grid).  Order-independent sum of mixed (tensor, position, word)
 * values; one launch.  host_out (PINNED host memory, may be NULL): the value is also copied there asynchronously behind the kernel.
 * The host mirror enqueues it behind a layer forward and compares the value at the next forward (a parameter
 * written through `.data` does not move PyTorch's version counter, on which the derived-weight caches are keyed). */
int gsn_fingerprint_hip(int n_tensors, const int64_t *meta, int64_t max_words, unsigned long long *acc, unsigned long long *host_out,
                        void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-1  pattern analysis (host).  Replaces utils_graph_processing.automorphism_orbits (:10-56) and
 * induced_edge_automorphism_orbits (:58-100): vertex orbits of Aut(H) numbered by rank of the orbit's smallest
 * vertex; the pattern's directed edges sorted by (u,v); edge-orbit ids in first-seen order of the key
 * {orbit(u),orbit(v)} (ordered pair iff directed_orbits); |Aut(H)|.
 *   directed_orbits  bit 0 (GSN_FLAG_DIRECTED_ORBITS): the reference's `directed_orbits`;  bit 1 (GSN_FLAG_DIRECTED): the
 *                    reference's `directed` (main.py:558, utils_graph_processing.py:14-16) -- every row (u,v) of `edges` is the
 *                    ARC u -> v, automorphisms preserve arcs, out_arcs lists the arcs themselves
 *   edges            [n_edges][2] int64, vertices 0..k-1; self loops / duplicates are dropped like the reference does
 *   out_vertex_orbit [GSN_KMAX_WIDE]  (patterns of up to GSN_KMAX_WIDE = 16 vertices, with or without GSN_FLAG_WIDE)
 *   out_arcs         [k*(k-1)][2]  sorted directed edge list, at most 240 rows;  out_arc_orbit [k*(k-1)]
 *   Every automorphism is stored while the orbits are taken; a pattern with more than 2^20 of them is GSN_E_UNSUPPORTED (the message
 *   names the count).  Every pattern of <= 9 vertices stays below (K9, star_graph(9): 362 880); star_graph(10), K10 and larger do not.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GSN_FLAG_DIRECTED_ORBITS 1
#define GSN_FLAG_DIRECTED 2
#define GSN_FLAG_WIDE 4 /* gsn_count_plan_build only: admit patterns of 10 .. GSN_KMAX_WIDE vertices (see there) */
int gsn_pattern_orbits(int64_t n_edges, const int64_t *edges, int directed_orbits, int64_t *out_k,
                       int64_t *out_vertex_orbit, int64_t *out_n_vertex_orbits, int64_t *out_arcs,
                       int64_t *out_arc_orbit, int64_t *out_n_arcs, int64_t *out_n_edge_orbits,
                       int64_t *out_aut_count);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-1  vertex orbits of an arbitrary small graph (host).  The automorphism part of the reference's deprecated
 * edge_automorphism_orbits (utils_graph_processing.py:189-251, --edge_automorphism line_graph): there the graph is the
 * LINE graph of the pattern and graph-tool enumerates its automorphisms (:214-224); here orbits come from
 * "is there an automorphism with sigma(u) = v" searches, numbered like np.unique(..., return_inverse) numbers the
 * per-vertex orbit minima (:231): orbit id = rank of the orbit's smallest vertex.
 *   edges      [n_edges][2] int64, vertices 0..n_vertices-1 (n_vertices <= 64); self loops / duplicates dropped
 *   out_orbit  [n_vertices]
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_graph_vertex_orbits(int64_t n_vertices, int64_t n_edges, const int64_t *edges, int64_t *out_orbit,
                            int64_t *out_n_orbits);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-1  counting plan (host).  Compiles a list of patterns (the reference's `subgraph_dicts`,
 * utils_data_gen.py:31-42) into the packed table the kernel executes: one rooted search per (pattern, vertex orbit)
 * [vertex mode] or per (pattern, directed-edge orbit) [edge mode], with symmetry-breaking order constraints for the
 * root's stabiliser.  Output columns follow utils_ids.py:19-25: patterns in the given order, orbit ids ascending.
 *   directed_orbits  flag bits as for gsn_pattern_orbits.  GSN_FLAG_DIRECTED (vertex mode only; edge mode ->
 *           GSN_E_UNSUPPORTED, the reference's directed edge counter dies on an unbound name, utils_graph_processing.py:146 vs
 *           :164): patterns AND the graphs later counted with this plan are digraphs (gt.Graph(directed=True), :108-113) -- a
 *           column (u,v) of edge_index is the arc u -> v, matches preserve arcs and, induced, non-arcs in each direction
 *           GSN_FLAG_WIDE: patterns of up to GSN_KMAX_WIDE = 16 vertices are accepted (17 and more: GSN_E_UNSUPPORTED; without the bit
 *           ten and more are).  A list whose largest pattern has <= GSN_KMAX vertices gives the same table as without the bit.  Otherwise
 *           the WHOLE table is emitted in the wide format (16-bit level masks, another magic word): gsn_count_sparse_hip executes it, every
 *           other entry that takes a plan table answers GSN_E_UNSUPPORTED.  The automorphism cap of gsn_pattern_orbits applies.
 *   pat_ptr [n_patterns+1] into pat_edges [.][2]
 *   plan    caller buffer of `capacity` uint32 words (call with plan=NULL to get *out_words)
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_count_plan_build(int mode, int induced, int directed_orbits, int64_t n_patterns, const int64_t *pat_ptr,
                         const int64_t *pat_edges, uint32_t *plan, int64_t capacity, int64_t *out_words,
                         int64_t *out_n_cols);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-1  batched counting (device).  Replaces utils_ids.subgraph_counts2ids (:7-29) applied to every graph of a batch,
 * i.e. the per-graph / per-pattern calls of subgraph_isomorphism_vertex_counts (utils_graph_processing.py:103-131) or
 * subgraph_isomorphism_edge_counts (:134-179) and the graph-tool VF2 enumeration under them.  One launch per batch.
 *   plan_host / plan_dev  the same plan table on host (launch configuration) and in device memory (kernel input)
 *   node_ptr [G+1], edge_ptr [G+1]   int64 device: graph g owns vertices node_ptr[g]..node_ptr[g+1] and columns
 *                                    edge_ptr[g]..edge_ptr[g+1] of edge_index
 *   edge_index            int64 device [2][E_total] (row 1 starts at edge_index + edge_row_stride); both directions
 *                         present as in PyG; self loops tolerated (their rows stay 0); duplicates: last column wins
 *   ids_are_global        1: vertex ids carry the batch offset node_ptr[g] (PyG collate), 0: graph-local ids
 *   graph_ids             optional int32 device [n_items]: process only these graphs (NULL = all G, n_items = G)
 *   max_nodes, max_edges  upper bounds over the processed graphs (sizes LDS); violators get GSN_ST_TOO_LARGE
 *   out                   int64 device [rows_total][n_cols] (rows = vertices or columns); fully overwritten for the
 *                         processed graphs, zeros included
 *   status                int32 device [G], written per processed graph (GSN_ST_*)
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_count_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                  const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                  int64_t edge_row_stride, int ids_are_global, const int32_t *graph_ids, int64_t n_items,
                  int64_t max_nodes, int64_t max_edges, int64_t *out, int32_t *status, void *stream);

/* The same counts for the graphs gsn_count_hip refuses (more than 768 vertices, tables beyond 160 KiB of LDS, 65 535 columns per graph):
 * the same reference lines (utils_ids.py:7-29 over utils_graph_processing.py:103-131 / :134-179), by a kernel whose graph lives in HBM as
 * sorted neighbour lists -- one lane per rooted search, no table sized by LDS (csrc/count_sparse.hip).  Opt-in: gsn_count_hip never
 * forwards to it.  Arguments as gsn_count_hip, except
 *   max_nodes, max_edges  carry no size limit here (no GSN_ST_TOO_LARGE)
 *   workspace             device scratch of workspace_bytes >= gsn_count_sparse_workspace_bytes(...), 256-byte aligned; GSN_E_NOSPACE below
 * Statuses: GSN_ST_BAD_INDEX (an endpoint outside the graph, or the graph's pointers outside the launch's): that graph's rows are zero,
 * the other graphs are counted; GSN_ST_KEYERROR as gsn_count_hip.  Rows of graphs outside graph_ids are untouched.
 * Limits: vertices and columns are numbered from node_ptr[0] / edge_ptr[0] of the launch in 32 bits (< 2^31 - 1 vertices, <= 2^30 columns:
 * GSN_E_UNSUPPORTED beyond); no fused encodings.  Directed plans (GSN_FLAG_DIRECTED) are vertex-mode plans, as for gsn_count_hip: every
 * column (u, v) is the arc u -> v, antiparallel columns are two arcs, repeated columns merge, self loops drop out; a directed plan in edge
 * mode -> GSN_E_UNSUPPORTED (there are no directed edge counts).  The call reads four pointer entries back (one stream synchronisation), so
 * it cannot be captured into a graph.  Deterministic: every cell has one writer. */
int gsn_count_sparse_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                         const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                         int64_t edge_row_stride, int ids_are_global, const int32_t *graph_ids, int64_t n_items,
                         int64_t max_nodes, int64_t max_edges, int64_t *out, int32_t *status, void *workspace,
                         int64_t workspace_bytes, void *stream);
/* Host: bytes of workspace for a launch that spans n_vertices_total = node_ptr[G] - node_ptr[0] vertices and n_columns_processed =
 * edge_ptr[G] - edge_ptr[0] columns (the launch's tables cover the whole span, also when graph_ids names a few of its graphs); n_cols =
 * the plan's output columns (no table depends on it today).  The size serves undirected and directed plans alike (the function takes no
 * flag: the row table is sized for out- and in-lists always).  -1 beyond the 32-bit limits above. */
int64_t gsn_count_sparse_workspace_bytes(int64_t n_vertices_total, int64_t n_columns_processed, int64_t n_cols);

/* Counting with the identifier encoding fused into the kernel's output: what the reference does in two steps -- int64 counts
 * (utils_ids.py:7-29), then DiscreteEmbedding('one_hot_encoder') on them in front of every GSN layer
 * (utils_graph_learning.py:78 / :170-187, models_graph_classification.py:222) -- in one launch, without the int64 rows going
 * to HBM and back and without the gsn_one_hot_hip launch.  Arguments as gsn_count_hip, plus
 *   n_classes  HOST int32 [n_cols] (as gsn_one_hot_hip; n_cols <= 64): column c becomes n_classes[c] floats, blocks in column order
 *   clamp      != 0: counts above n_classes[c] - 1 go to the last class (as gsn_one_hot_hip)
 *   enc_out    fp32 device [rows_total][sum n_classes]: per column a single 1 at the count (all 0 when the count is out of
 *              range and clamp == 0); fully overwritten for the processed graphs
 *   out        the int64 rows as well, or NULL (then only the encoded rows are written) */
int gsn_count_encode_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                         const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                         int64_t edge_row_stride, int ids_are_global, const int32_t *graph_ids, int64_t n_items,
                         int64_t max_nodes, int64_t max_edges, int64_t *out, int32_t *status, const int32_t *n_classes,
                         int clamp, float *enc_out, void *stream);
/* The same, and the encoded rows a second time as fp16 into columns pack_col0 .. of an exact row pack (gsn_pack16 below: the layout the
 * packed-row layer kernel reads; 1.0 = 0x3c00): `pack` fp16 device [rows_total][pack_stride], only the sum n_classes columns from
 * pack_col0 are written.  Written from the kernel's staged class indices: GSN_E_UNSUPPORTED when those are not staged (a graph split
 * over several workgroups, a column with more than 255 classes) -- pack the fp32 rows with gsn_pack16_rows_hip then.
 * enc_out may be NULL (r05): the fp32 rows are then not written at all -- the int64 counts (`out`) and the pack columns are what leaves the
 * kernel: what utils_ids.py:27 stores, and the encoder output (utils_graph_learning.py:170-187) in the form the packed-row layer reads. */
int gsn_count_encode_pack16_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                                const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                                int64_t edge_row_stride, int ids_are_global, const int32_t *graph_ids, int64_t n_items,
                                int64_t max_nodes, int64_t max_edges, int64_t *out, int32_t *status, const int32_t *n_classes,
                                int clamp, float *enc_out, uint16_t *pack, int64_t pack_stride, int64_t pack_col0, void *stream);

/* The same launch leaving what the first GSN layer needs beside the identifiers (r06).  Every fifth workgroup of the grid is a SIDE workgroup:
 * it takes the graphs of the four counting workgroups dispatched in front of it, sorts their columns in LDS and writes
 *   (i)   the target-sorted CSR of its graph's columns -- seg_ptr / perm / sorted_target / sorted_other exactly as
 *         gsn_csr_build_graphs_hip writes them (GSN_sparse.py:140-143: the reference re-sorts a COO tensor in every layer);
 *   (ii)  the node pack: one-hot of integer node codes (utils_graph_learning.py:170-187: DiscreteEmbedding('one_hot_encoder') on
 *         data.x) as fp16 [n_nodes][32], column 31 = 1.0 -- what gsn_one_hot_pack16_hip(col0 = 0, one_col = 31) writes;
 *   (iii) columns edge_col0 .. 15 of the edge pack fp16 [n_edges][16]: the one-hot of integer edge codes at edge_col0 .., zeros behind it (the
 *         counting workgroups write the identifier classes at pack_col0 .. as in gsn_count_encode_pack16_hip; with pack_col0 = 0 and
 *         edge_col0 = sum n_classes the whole row is written by the launch and the pack needs no zero fill).
 * Each part is optional (null pointers).  The counting workgroups run exactly what they run without side outputs (the work inside them, where
 * the graph already sits in LDS, was measured and lost: the molecule instantiation is at its register bound, profiles/r06_count_side_ab.txt).
 * Needs one workgroup per item (no graph list, no graph split over several workgroups) and graphs whose sort fits LDS, edge-mode or vertex-mode
 * plan alike; GSN_E_UNSUPPORTED otherwise, nothing launched -- the caller uses the separate entry points.
 * node_ptr[0] must be 0, node_ptr[n_graphs] = n_nodes, edge_ptr[n_graphs] = n_edges (a collated batch).  Statuses: a column that leaves
 * its graph raises GSN_ST_BAD_INDEX on that graph (its CSR entries are then unspecified but inside the batch's ranges), a graph
 * beyond max_nodes / max_edges GSN_ST_TOO_LARGE (sorted all the same when it fits the launch's LDS, else its vertices own no columns and
 * its columns map to themselves: as gsn_csr_build_graphs_hip); *code_status (device int32, may be NULL; set to 0 by the launch's first side workgroup: the word is this launch's) gets 1 ORed in when a code lies outside its
 * column's classes and clamp is 0 (that column's segment stays zero, as gsn_one_hot_pack16_hip). */
typedef struct {
    int csr_row;                 /* which row of edge_index is the aggregation target (1: flow = source_to_target) */
    int32_t *seg_ptr;            /* [n_nodes + 1] or NULL: no CSR */
    int32_t *perm;               /* [n_edges] */
    int32_t *sorted_target;      /* [n_edges] or NULL */
    int32_t *sorted_other;       /* [n_edges] or NULL */
    int64_t n_nodes, n_edges;    /* batch totals */
    const int64_t *node_codes;   /* [n_nodes][node_code_cols] or NULL: no node pack */
    int node_code_cols;          /* 1 .. 4 */
    int node_n_classes[4];       /* sum <= 28 */
    int node_clamp;
    uint16_t *node_pack;         /* fp16 [n_nodes][32], 16-byte aligned */
    const int64_t *edge_codes;   /* [n_edges][edge_code_cols] or NULL: only the identifier columns of the edge pack are written */
    int edge_code_cols;          /* 1 .. 4 */
    int edge_n_classes[4];
    int edge_clamp;
    int edge_col0;               /* first pack column of the edge codes' one-hot: a multiple of 4, behind the identifier columns; <= 8 classes */
    int32_t *code_status;        /* or NULL */
} gsn_count_side;
int gsn_count_encode_pack16_side_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                                     const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                                     int64_t edge_row_stride, int ids_are_global, int64_t max_nodes, int64_t max_edges, int64_t *out,
                                     int32_t *status, const int32_t *n_classes, int clamp, uint16_t *pack, int64_t pack_stride,
                                     int64_t pack_col0, const gsn_count_side *side, void *stream);

/* The same launch with COMPACT outputs in place of the packs: layer 0's inputs are one-hot encodings of a few integer codes, and the keys
 * below say which rows of two tiny tables they are (gsn_count_layer_step_keys_hip reads them; ~0.2 GB of pack rows per 65 536 molecules are
 * then neither written nor read back).  Each is optional (NULL) except idmask:
 *   nkey   uint8  [n_nodes]   row of vertex v in the NODE DICTIONARY: the mixed-radix number of its code digits, column 0 most significant.
 *                             Column c has node_n_classes[c] digits when side->node_clamp (the clamped code), one more otherwise: digit
 *                             node_n_classes[c] = "none", a code outside its classes (zero segment, *code_status set as above).  Row k of the
 *                             dictionary is what gsn_one_hot_pack16_hip(clamp = 0, col0 = 0, one_col = 31) writes for the k-th digit tuple
 *                             in that order; <= 256 rows (GSN_E_UNSUPPORTED beyond).  With nkey, side->node_pack may be NULL.
 *   ekeys  uint32 [n_edges]   target-sorted order (position i of perm): nkey[sorted_target[i]] | nkey[sorted_other[i]] << 8 | m << 16, m = the
 *                             edge codes' hot columns of column perm[i] as a bit mask (bit j = pack column side->edge_col0 + j).  Needs the
 *                             four CSR arrays, which are written as before.
 *   idmask uint16 [n_edges]   column order: the hot pack columns pack_col0 .. of the row's identifier classes as a bit mask (bit j = pack
 *                             column j; a count outside its classes, unclamped, sets none) -- 2 bytes in place of 2 sum(n_classes);
 *                             pack_col0 + sum(n_classes) <= 16.
 * No edge pack is written (side->edge_codes only feed ekeys); everything else is gsn_count_encode_pack16_side_hip's. */
typedef struct {
    uint8_t *nkey;
    uint32_t *ekeys;
    uint16_t *idmask;
} gsn_count_keys;
int gsn_count_encode_keys_side_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                                   const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                                   int64_t edge_row_stride, int ids_are_global, int64_t max_nodes, int64_t max_edges, int64_t *out,
                                   int32_t *status, const int32_t *n_classes, int clamp, int64_t pack_col0, const gsn_count_side *side,
                                   const gsn_count_keys *keys, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-2  aggregation target index (device).  The scatter-add of the layers,
 *   torch.sparse.FloatTensor(edge_index, msgs, [N,N,d]) + torch.sparse.sum(msgs, aggr_dim).to_dense()
 * (GSN_sparse.py:140-143, GSN_edge_sparse.py:136-139, MPNN_*.py, *_ogb.py), is executed as a segmented sum over a
 * target-sorted edge permutation.  This builds that CSR once per batch (stable counting sort by target):
 *   index   int64 device [E]  aggregation targets (edge_index[1] for flow=source_to_target, [0] otherwise)
 *   seg_ptr int32 device [N+1] out; perm int32 device [E] out (edge ids grouped by target, original order kept inside)
 *   sorted_target int32 device [E] out or NULL: sorted_target[q] = index[perm[q]] (the target of the q-th sorted edge)
 *   other int64 device [E] or NULL (the other row of edge_index), sorted_other int32 device [E] out or NULL:
 *         sorted_other[q] = other[perm[q]] (the message source of the q-th sorted edge) -- lets a kernel that walks the
 *         edges in target order gather x_i / x_j / per-edge rows through ONE index load each
 *   scratch int32 device [gsn_csr_scratch_elems(N)]
 * ---------------------------------------------------------------------------------------------------------------- */
int64_t gsn_csr_scratch_elems(int64_t n_nodes);
int gsn_csr_build_hip(int64_t n_nodes, int64_t n_edges, const int64_t *index, const int64_t *other, int32_t *seg_ptr,
                      int32_t *perm, int32_t *sorted_target, int32_t *sorted_other, int32_t *scratch, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-2  propagate: fused gather -> message -> segmented sum (device, fp32).
 *   out[t, :] = sum_{e : tgt(e) = t} msg_e,   msg_e assembled on the fly from up to three sources
 *     kind GSN_MSG_CAT  : msg_e = concat(a[src_e] (da), b_e or b[src_e] (db), c_e (dc))   -- 'gin' messages
 *                         (GSN_sparse.py:160-164, GSN_edge_sparse.py:154-158) and plain pre-computed messages (da=0,dc=0)
 *     kind GSN_MSG_RELU_SUM : msg_e = relu(a[src_e] + b_e or b[src_e] + c_e), all width d  -- 'ogb' messages
 *                         (GSN_edge_sparse_ogb.py:119-125, MPNN_edge_sparse_ogb.py message)
 *   a: per-node [N][da];  b: per-edge [E][db] (b_per_node=0) or per-node [N][db] gathered at src (b_per_node=1);
 *   c: per-edge [E][dc];  any of a/b/c may be NULL with width 0.   out: [N][d_out], fully overwritten.
 *   src int64 [E] message source vertex (edge_index[0] for source_to_target); seg_ptr/perm from gsn_csr_build_hip;
 *   sorted_src int32 [E] = src[perm[q]] (gsn_csr_build_hip's sorted_other) or NULL -- saves one dependent load per edge.
 * gsn_propagate_bwd_hip is the adjoint: given g_out [N][d_out] it writes g_a [N][da] (overwritten, gathers through the
 * source-sorted CSR seg_ptr_src/perm_src), g_b ([E][db] or [N][db]) and g_c [E][dc]; for RELU_SUM the forward inputs
 * are needed again to recompute the relu mask.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { GSN_MSG_CAT = 0, GSN_MSG_RELU_SUM = 1 };

int gsn_propagate_fwd_hip(int kind, int64_t n_nodes, int64_t n_edges, const int64_t *src, const int32_t *seg_ptr,
                          const int32_t *perm, const int32_t *sorted_src, const float *a, int64_t da, const float *b, int64_t db,
                          int b_per_node, const float *c, int64_t dc, float *out, void *stream);

/* out[t][0 .. width) = sum over the rows q of t's segment of b[row(q)][0 .. width), where b is a COLUMN SLICE of wider rows (row stride ld
 * floats; row(q) = perm[q], or q when perm is NULL): gsn_propagate_fwd_hip's concatenation with the per-edge block alone, reading the slice in
 * place -- the per-vertex sums of a gathered block's input gradient (the x_i / x_j blocks of an edge stage, GSN_sparse.py:166-171). */
int gsn_segment_sum_rows_hip(int64_t n_nodes, int64_t n_edges, const int64_t *src, const int32_t *seg_ptr, const int32_t *perm,
                             const int32_t *sorted_src, const float *b, int64_t width, int64_t ld, float *out, void *stream);

int gsn_propagate_bwd_hip(int kind, int64_t n_nodes, int64_t n_edges, const int64_t *src, const int64_t *tgt,
                          const int32_t *seg_ptr_src, const int32_t *perm_src, const float *a, int64_t da,
                          const float *b, int64_t db, int b_per_node, const float *c, int64_t dc,
                          const float *g_out, float *g_a, float *g_b, float *g_c, void *stream);

/* The same pass with the layer's own term and the central encoders' column padding inside it (r03; what the reference does with
 * three elementwise tensor ops and two concatenations per layer):
 *     out[t] = (1 + *eps) * self[t] + sum_{e -> t} msg_e
 *   GSN_sparse.py:157-163 / GSN_edge_sparse.py:95-109 (gin):   self = cat(x, identifiers or their central value, central edge value);
 *   GSN_edge_sparse_ogb.py:63-84, :103-106 (ogb):              self = x (+ identifiers, global scope).
 * self_blocks: up to three blocks, concatenated (CAT: their widths add up to d_out) or added (RELU_SUM: each d_out wide); row_stride
 * in floats, 0 = ONE row for every vertex (central_encoder's constant value, utils_graph_learning.py:232-260).  eps: device pointer
 * to the layer's eps (parameter or buffer), NULL = 0.  pad_b / pad_c: zero columns in front of the per-edge blocks b / c of a
 * concatenation (utils_graph_learning.py:240-242: the extra first column of an extended one-hot encoding), so that
 * d_out = da + pad_b + db + pad_c + dc.  gsn_propagate_pad_bwd_hip: the adjoint of the messages with the same column layout;
 * gsn_propagate_self_bwd_hip: the adjoint of the self term.
 */
typedef struct gsn_self_block {
    const float *data;
    int64_t width;
    int64_t row_stride;
} gsn_self_block;

int gsn_propagate_self_fwd_hip(int kind, int64_t n_nodes, int64_t n_edges, const int64_t *src, const int32_t *seg_ptr,
                               const int32_t *perm, const int32_t *sorted_src, const float *a, int64_t da, const float *b, int64_t db,
                               int b_per_node, const float *c, int64_t dc, int64_t pad_b, int64_t pad_c, int n_self,
                               const gsn_self_block *self_blocks, const float *eps, float *out, void *stream);

/* Adjoint of the self term (one pass over g_out [N][d_out]): g_self[k] (fp32 [N][width_k], NULL = not wanted / single-row block)
 * receives (1 + eps) * the block's columns of g_out; g_colsum (fp64 [d_out], zero-filled, may be NULL) the column sums of
 * (1 + eps) * g_out -- the gradient of a single-row block is its slice; g_eps (fp64 [1], zero-filled, may be NULL) sum g_out . self. */
int gsn_propagate_self_bwd_hip(int kind, int64_t n_nodes, int64_t d_out, const float *g_out, int n_self,
                               const gsn_self_block *self_blocks, float *const *g_self, const float *eps, double *g_eps,
                               double *g_colsum, void *stream);

int gsn_propagate_pad_bwd_hip(int kind, int64_t n_nodes, int64_t n_edges, const int64_t *src, const int64_t *tgt,
                              const int32_t *seg_ptr_src, const int32_t *perm_src, const float *a, int64_t da,
                              const float *b, int64_t db, int b_per_node, const float *c, int64_t dc, int64_t pad_b, int64_t pad_c,
                              const float *g_out, float *g_a, float *g_b, float *g_c, void *stream);
/* The relu-sum adjoint of a layer whose own term is its gathered block (out = (1 + eps) a + sum relu(a[src] + b + c): GSN_edge_sparse_ogb.py:63-84,
 * :103-106 with self = x) in TWO launches: g_a receives the per-source sums of the masked per-edge gradients AND (1 + eps) g_out, g_eps (fp64, added
 * to; may be NULL) = sum g_out . a.  Replaces gsn_propagate_pad_bwd_hip + gsn_propagate_self_bwd_hip + the sum of their results.  b / c per edge,
 * widths d (or 0).  GSN_E_UNSUPPORTED (nothing launched): no edges, d > 320 or not a multiple of 4, unaligned rows, no per-edge gradient wanted. */
int gsn_propagate_bwd_fold_self_hip(int64_t n_nodes, int64_t n_edges, const int64_t *src, const int64_t *tgt, const int32_t *seg_ptr_src,
                                    const int32_t *perm_src, const float *a, int64_t d, const float *b, int64_t db, const float *c, int64_t dc,
                                    const float *g_out, float *g_a, float *g_b, float *g_c, const float *eps, double *g_eps, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-2  fused dense stage (device; fp32 in / fp32 out; matrix products run as six exact bf16 plane products per fp32
 * product on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- fp32-equivalent error -- or, with GSN_LINEAR_BF16X6=0,
 * on v_mfma_f32_32x32x2_f32).  One models_misc.mlp layer
 * (models_misc.py:52-58)   Y = act( bn( X W^T + bias ) )   over M rows, where the rows of X are assembled on the fly
 * as a concatenation of up to five blocks, each either direct ([M][w]) or gathered through an int64 index
 * ([R][w] rows picked by idx[M]) -- this is torch.cat((x_i, x_j, identifiers.., edge_features), -1) feeding msg_fn
 * (GSN_sparse.py:166-171, GSN_edge_sparse.py:160-165) without materialising the cat or the gathers.
 *   W [n_out][k_total] row-major fp32 as nn.Linear stores it (k_total = sum of block widths); bias [n_out] or NULL
 *   bn_mean / bn_scale / bn_shift [n_out], all three or none:  y = (h - mean) * scale + shift  with
 *       scale = gamma / sqrt(var + eps), shift = beta  (eval: running stats; train: the batch stats of pass 1)
 *   act: 0 identity, 1 relu, 2 elu, 3 tanh   (models_misc.choose_activation)
 *   row_perm int32 [M] or NULL: output row r is computed from logical input row row_perm[r]
 *   out   [M][n_out] fp32, or NULL when only statistics are wanted
 *   stats double [2][n_out] or NULL: if given (train-mode BatchNorm1d, first pass) the kernel ADDS per-column sum and
 *         sum of squares of the PRE-BN values h = X W^T + bias into it (caller zeroes it) and skips bn / act; with
 *         `out` also given the same pass writes those raw h rows to it (then apply gsn_bn_act_hip)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
    const float *data;     /* [rows][width] fp32, row stride = width */
    const int64_t *idx;    /* int64 gather index (a row of edge_index) or NULL */
    int64_t width;
    const int32_t *idx32;  /* int32 gather index (perm / sorted_target / sorted_source of gsn_csr_build_hip) or NULL;
                              at most one of idx / idx32; both NULL: direct (row r) */
} gsn_block;

int gsn_linear_fwd_hip(int64_t m_rows, int n_blocks, const gsn_block *blocks, const float *W, const float *bias,
                       int64_t n_out, const float *bn_mean, const float *bn_scale, const float *bn_shift, int act,
                       const int32_t *row_perm, float *out, double *stats, void *stream);
/* gsn_linear_fwd_hip with W given through element strides (W[j][k] at W + j * w_row_stride + k * w_col_stride): the input-gradient product
 * gX = gH W of a dense stage reads the stage's own weight as its transpose (1, K) -- no transposed copy per stage and step.  No row_perm.
 * GSN_E_UNSUPPORTED when the bf16x6 kernel is switched off (GSN_LINEAR_BF16X6=0). */
int gsn_linear_fwd_strided_hip(int64_t m_rows, int n_blocks, const gsn_block *blocks, const float *W, int64_t w_row_stride,
                               int64_t w_col_stride, const float *bias, int64_t n_out, const float *bn_mean, const float *bn_scale,
                               const float *bn_shift, int act, float *out, double *stats, void *stream);

/* Split-K form of the two entry points above for FEW rows (a dense backward at the reference's batch sizes, train_test_funcs.py:88-106 with
 * README.md:112,121's batch sizes: M = 10^3 rows is a third of the chip's CUs, each walking all K slices): gsn_linear_splitk_plan gives the
 * number of K ranges this library would use for the shape (1: take gsn_linear_fwd_hip / _strided_hip); gsn_linear_fwd_splitk_hip ADDS
 * blocks W^T (+ bias) to `out`, which must hold zeros on entry (float atomics: the order of the ranges' partial sums varies in the last bits).
 * Identity epilogue only.  w_row_stride = w_col_stride = 0: W is row-major [n_out][K]. */
int gsn_linear_splitk_plan(int64_t m_rows, int64_t k_total, int64_t n_out);
int gsn_linear_fwd_splitk_hip(int64_t m_rows, int n_blocks, const gsn_block *blocks, const float *W, int64_t w_row_stride,
                              int64_t w_col_stride, const float *bias, int64_t n_out, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-2  fused MLP chain (device; fp32 in / fp32 out; matrix products as in gsn_linear_fwd_hip: bf16x6 by default,
 * GSN_CHAIN_BF16X6=0 for the fp32-MFMA kernels).  One or two dependent stages of models_misc.mlp (models_misc.py:52-58)
 * evaluated per 32- or 64-row tile without writing the intermediates to HBM:
 *     Y_s = act_s( bn_s( [ blocks_s | Y_{s-1} ] W_s^T + bias_s ) ),   out = Y_last   ([M][n_out_last])
 * i.e. the input of stage s > 0 is the concatenation of its own HBM blocks (e.g. x in update_fn's cat((x, agg)),
 * GSN_sparse.py:114 / GSN_edge_sparse.py:112) followed by the previous stage's output.  Weights are held in registers,
 * activations in LDS.  Same per-stage parameters as gsn_linear_fwd_hip.  `stats` (double [2][n_out_last]) replaces the
 * output by column sums / sums of squares of the LAST stage's pre-BN values (train-mode BatchNorm1d, pass 1).
 * gsn_mlp_chain_supported() tells whether a chain fits the fused kernel (<= 2 stages, every K_s <= 160, n_out_s <= 128,
 * at most 6 blocks, stage-1 blocks <= 64 columns, activations identity / relu); otherwise run the stages one by one
 * with gsn_linear_fwd_hip.
 */
typedef struct {
    const gsn_block *blocks;
    int n_blocks;
    const float *W;       /* [n_out][k_total] row-major; k_total = sum(block widths) + (s > 0 ? n_out of stage s-1 : 0) */
    const float *bias;    /* [n_out] or NULL */
    int64_t n_out;
    const float *bn_mean, *bn_scale, *bn_shift; /* all three or none */
    int act;
} gsn_chain_stage;

/* Fused scatter-add: with `seg_target` (int32 [M], the target of every row, rows visited in target-sorted order through
 * row_perm = perm and seg_target = sorted_target of gsn_csr_build_hip) the last stage's rows are summed per target
 * inside the kernel and `out` is [n_seg][n_out_last] -- the torch.sparse.sum of GSN_sparse.py:140-143 without writing
 * the [E, d] messages.  `out` must first be prepared with gsn_segsum_prepare_hip (zeroes the rows of empty segments
 * and of segments that straddle a GSN_SEG_RANGE_ROWS-row boundary, which the kernel adds to atomically; all other rows
 * are plain stores, so a segment's summation order is its row order except for segments longer than that range).
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_mlp_chain_supported(int n_stages, const gsn_chain_stage *stages);
int gsn_mlp_chain_fwd_hip(int64_t m_rows, int n_stages, const gsn_chain_stage *stages, const int32_t *row_perm,
                          const int32_t *seg_target, float *out, double *stats, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-2  one whole `general` layer in ONE launch (device; fp32 in / fp32 out): GSN_sparse.forward / propagate / message
 * (GSN_sparse.py:93-176), GSN_edge_sparse (GSN_edge_sparse.py:82-170) and the MPNN twins with msg_kind='general':
 *     r_e   = act_e( bn_e( cat(edge blocks) We^T + be ) )                          per edge, rows in target-sorted order
 *     S_v   = sum_{e -> v} r_e                                                     torch.sparse.sum (:140-143)
 *     out_v = act_1( bn_1( act_0( bn_0( [x_v | S_v | deg_v,0,0,0] W0^T + b0 ) ) W1^T + b1 ) )
 * where the caller has folded msg_fn's last Linear into update_fn's first (W0 = [W3x | W3a W2 | W3a b2 | 0 0 0], layers.py)
 * and deg_v = seg_ptr[v+1] - seg_ptr[v].  r_e, S_v and the hidden rows stay in LDS: every input is read once and the
 * output written once.  Matrix products: both operands split into two fp16 planes after exact power-of-two row / matrix
 * scaling, three plane products on v_mfma_f32_32x32x16_f16 with fp32 accumulation (error vs fp64 as an fp32 FMA loop's;
 * two products for rows that are exact in fp16, e.g. one-hot encodings).  Summation order of S_v = row order.
 *   seg_ptr  int32 [n_nodes+1]  target-sorted CSR of gsn_csr_build_hip
 *   edge     stage with 1..6 blocks, every block gathered through an int32 index in sorted-row order (sorted_target,
 *            sorted_source or perm of gsn_csr_build_hip), widths multiples of 4, sum <= 80; n_out <= 128
 *   x        [n_nodes][d_x], d_x multiple of 4; d_x + edge.n_out + 4 <= 160
 *   node0    W [n0][d_x + edge.n_out + 4], no blocks;  node1  W [n1][n0], no blocks;  n0, n1 <= 128, multiples of 4
 *   act 0 identity / 1 relu; bn_* as in gsn_linear_fwd_hip (eval-mode / resolved statistics)
 * and, the hidden layers of a d = 128 model (GSN_edge_sparse.py:82-170 with K = 260 / 272 edge rows, MPNN_edge_sparse.py:110-151;
 * csrc/layer_w.hip): d_x = 128, every stage 128 wide, edge blocks = x through one index, x through another, then <= 16 further
 * columns (widths multiples of 4, each gathered through one of those two indices or a third).  For this shape the forward call
 * runs a small pass over x in front of the layer kernel (one int per node: the exponent of the row's largest |value|, stream-
 * ordered scratch from hipMallocAsync unless the caller brings it: gsn_layer_fused_fwd_ws_hip) and returns GSN_E_UNSUPPORTED when it would
 * have to allocate while the stream is being captured into a graph, or when the first two edge blocks are not `x` itself; the caller
 * then composes the layer from the other entry points.
 * gsn_layer_fused_supported() says whether the shapes fit; otherwise compose gsn_mlp_chain_fwd_hip launches.
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_layer_fused_supported(const gsn_chain_stage *edge, int64_t d_x, const gsn_chain_stage *node0,
                              const gsn_chain_stage *node1);
/* The weights in the form the kernel keeps them in registers (per stage a power-of-two scale from max |W * bn_scale|, fp16
 * plane fragments per wave and K step) are made ONCE per weight version by gsn_layer_fused_prepare_hip into a device buffer of
 * gsn_layer_fused_prepared_bytes() bytes (16-byte aligned) and handed to every forward call as `prepared`; re-run it when W,
 * bias-independent: bn_scale or W of a stage changed.  (Split inside the forward kernel, every workgroup re-read every weight
 * row at the same moment: 50 - 400 k cycles of prologue per launch under load.) */
int64_t gsn_layer_fused_prepared_bytes(const gsn_chain_stage *edge, int64_t d_x, const gsn_chain_stage *node0,
                                       const gsn_chain_stage *node1);
int gsn_layer_fused_prepare_hip(const gsn_chain_stage *edge, int64_t d_x, const gsn_chain_stage *node0,
                                const gsn_chain_stage *node1, void *prepared, void *stream);
int gsn_layer_fused_fwd_hip(int64_t n_nodes, int64_t n_edges, const int32_t *seg_ptr, const gsn_chain_stage *edge,
                            const float *x, int64_t d_x, const gsn_chain_stage *node0, const gsn_chain_stage *node1,
                            const void *prepared, float *out, void *stream);
/* The same with caller-owned scratch: gsn_layer_fused_workspace_bytes() device bytes (0 for shapes that need none; today the d = 128
 * shape: 4 bytes per node), 4-byte aligned, contents undefined before and after.  With it the call allocates nothing and can be
 * captured into a HIP graph; `workspace` may be null when the size is 0.
 * Chaining layers of a d = 128 model: `out_row_exp` (int32 [n_nodes] or null; 128-wide outputs only) receives, per output row, the
 * exponent field of its largest |value| (255: the row holds an Inf / NaN) -- the d = 128 kernel writes it with the rows, the other
 * kernels by a pass over the rows they wrote; `x_row_exp` (or null) is that array of the layer that produced `x`: the d = 128 kernel
 * then skips its own pass over x (and needs no workspace).  It must describe the CURRENT contents of x. */
int64_t gsn_layer_fused_workspace_bytes(int64_t n_nodes, const gsn_chain_stage *edge, int64_t d_x, const gsn_chain_stage *node0,
                                        const gsn_chain_stage *node1);
int gsn_layer_fused_fwd_ws_hip(int64_t n_nodes, int64_t n_edges, const int32_t *seg_ptr, const gsn_chain_stage *edge,
                               const float *x, int64_t d_x, const gsn_chain_stage *node0, const gsn_chain_stage *node1,
                               const void *prepared, float *out, void *workspace, int64_t workspace_bytes,
                               const int32_t *x_row_exp, int32_t *out_row_exp, void *stream);

/* The d = 128 shape on GRAPH-ALIGNED tiles (csrc/layer_g.hip): the same layer, the same `prepared` buffer as gsn_layer_fused_fwd_hip for that
 * shape, for a collated batch whose graph boundaries the caller knows (torch_geometric's Batch.ptr; the pointers of
 * gsn_csr_build_graphs_hip): graph g owns the consecutive vertices node_ptr[g] .. node_ptr[g+1] and no edge leaves its graph.  The node
 * part of the edge stage, x [W_i | W_j]^T, is then computed once per NODE (MPNN_edge_sparse.py:139-151 evaluates it once per EDGE:
 * cat(x_i, x_j, e) W^T), on tiles of whole graphs, and the edge stage is a gather-add of P_i[target] + P_j[source] + z_e W_z^T.
 * No workspace, no row exponents.  Every graph must have <= 128 vertices (max_nodes, the caller's bound): GSN_E_UNSUPPORTED otherwise --
 * the caller then uses gsn_layer_fused_fwd_ws_hip.  node_ptr int64 [n_graphs + 1] device, node_ptr[0] = 0, node_ptr[n_graphs] = n_nodes. */
int gsn_layer_fused_graphs_supported(const gsn_chain_stage *edge, int64_t d_x, const gsn_chain_stage *node0,
                                     const gsn_chain_stage *node1);
int gsn_layer_fused_fwd_graphs_hip(int64_t n_nodes, int64_t n_edges, const int32_t *seg_ptr, const gsn_chain_stage *edge,
                                   const float *x, int64_t d_x, const gsn_chain_stage *node0, const gsn_chain_stage *node1,
                                   const void *prepared, int64_t n_graphs, const int64_t *node_ptr, int64_t max_nodes,
                                   float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-2  the same one-launch layer on EXACT fp16 ROW PACKS (csrc/layer_rp.hip).  Layer 0 of every reference model reads one-hot /
 * small-integer encodings (utils_graph_learning.py:78-88, :170-187: DiscreteEmbedding('one_hot_encoder')): every value is exact in
 * fp16.  A producer that knows this (gsn_count_encode_hip, gsn_one_hot_hip, or gsn_pack16_rows_hip over an existing fp32 tensor) writes
 * the rows a second time as fp16 in the layout the matrix pipe reads, and the layer kernel skips what it otherwise does per edge row:
 * gathering fp32, converting, testing the conversion for exactness.  Same arithmetic, same results as gsn_layer_fused_fwd_hip.
 *   node_rows  fp16 [n_nodes][32]   columns 0 .. d_x-1 = x, columns d_x .. 30 = 0, column 31 = 1.0   (16-byte aligned)
 *   edge_rows  fp16 [edge_rows][16] the edge-level blocks of the edge stage (identifiers, edge features) concatenated in block order,
 *                                   zero padded; NULL when the edge stage is cat(x[i], x[j]) alone
 * Every value must be exactly what the fp32 tensors hold and < 2 in magnitude (the edge stage's weight scale is made for that bound);
 * gsn_pack16_rows_hip checks both and ORs 1 into *status (device int32, caller-zeroed) when a value is not.
 * The edge stage must be: block 0 = x through an int32 index, block 1 = x through another, blocks 2.. = the edge-level blocks, all through
 * ONE int32 index (perm of gsn_csr_build_hip), <= 16 columns together; widths as gsn_layer_fused_fwd_hip's register-resident shape
 * (every stage 128 wide, d_x + 4 <= 32).  The prepared weights are NOT those of gsn_layer_fused_prepare_hip (another k-slot order):
 * gsn_layer_fused_pack16_prepare_hip into gsn_layer_fused_pack16_prepared_bytes() bytes.  The fp32 `data` pointers of the blocks are not
 * read.  gsn_layer_fused_fwd_pack16_hip returns GSN_E_UNSUPPORTED when the packs are beyond its 32-bit byte offsets (n_nodes >= 2^25).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
    const uint16_t *node_rows;
    const uint16_t *edge_rows;
} gsn_pack16;
int gsn_pack16_rows_hip(const float *src, int64_t rows, int64_t width, uint16_t *dst, int64_t dst_stride, int64_t col0,
                        int64_t one_col, int32_t *status, void *stream);
/* gsn_one_hot_hip's encoding (utils_graph_learning.py:170-187: DiscreteEmbedding('one_hot_encoder') over integer columns) written straight
 * into columns col0 .. col0 + sum(n_classes) of a pack (dst_stride fp16 columns per row, a multiple of 8, <= 64, rows 16-byte aligned);
 * one_col >= 0: that column = 1.0.  With col0 == 0 and one_col >= 0 the call owns the whole pack (a node pack: its remaining columns are
 * zero by contract) and writes every column of every row.
 * A code outside its column's classes leaves that column's segment zero (clamp: counted as the nearest class), as gsn_one_hot_hip, and
 * ORs 1 into *status (device int32, caller-zeroed; may be NULL) -- the reference's F.one_hot raises there. */
int gsn_one_hot_pack16_hip(int64_t m_rows, int n_cols, const int64_t *values, const int32_t *n_classes, int clamp, uint16_t *dst,
                           int64_t dst_stride, int64_t col0, int64_t one_col, int32_t *status, void *stream);
int gsn_layer_fused_pack16_supported(const gsn_chain_stage *edge, int64_t d_x, const gsn_chain_stage *node0,
                                     const gsn_chain_stage *node1);
int64_t gsn_layer_fused_pack16_prepared_bytes(const gsn_chain_stage *edge, int64_t d_x, const gsn_chain_stage *node0,
                                              const gsn_chain_stage *node1);
int gsn_layer_fused_pack16_prepare_hip(const gsn_chain_stage *edge, int64_t d_x, const gsn_chain_stage *node0,
                                       const gsn_chain_stage *node1, void *prepared, void *stream);
int gsn_layer_fused_fwd_pack16_hip(int64_t n_nodes, int64_t n_edges, const int32_t *seg_ptr, const gsn_chain_stage *edge,
                                   const float *x, int64_t d_x, const gsn_chain_stage *node0, const gsn_chain_stage *node1,
                                   const void *prepared, const gsn_pack16 *pack, int64_t edge_rows, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-1 + HP-2 as ONE host call (r06): the orbit counting of a collated batch with its side outputs
 * (gsn_count_encode_pack16_side_hip: int64 identifiers, CSR, node pack, whole edge pack rows) and, behind it on the same stream, layer 0
 * of the model on the packs (gsn_layer_fused_fwd_pack16_hip) -- what the reference reaches through utils_ids.py:7-29
 * (subgraph_counts2ids), utils_graph_learning.py:170-187 (the one-hot encoders) and GSN_edge_sparse.py:82-170 (forward) as three
 * Python-level stages.  Two kernel launches, no allocation, no host synchronisation, capturable into a HIP graph; the two structs carry
 * the arguments of the two entry points verbatim (same meaning, same checks, same status codes), so a host keeps them filled in and
 * pays one foreign call per step.  layer->seg_ptr and the edge stage's block indices are normally count->side's CSR arrays. */
typedef struct {
    const uint32_t *plan_host, *plan_dev;
    int64_t plan_words, n_graphs;
    const int64_t *node_ptr, *edge_ptr, *edge_index;
    int64_t edge_row_stride;
    int ids_are_global;
    int64_t max_nodes, max_edges;
    int64_t *out;
    int32_t *status;
    const int32_t *n_classes;
    int clamp;
    uint16_t *pack;
    int64_t pack_stride, pack_col0;
    const gsn_count_side *side;
} gsn_count_call;
typedef struct {
    int64_t n_nodes, n_edges;
    const int32_t *seg_ptr;
    const gsn_chain_stage *edge;
    const float *x;
    int64_t d_x;
    const gsn_chain_stage *node0, *node1;
    const void *prepared;
    const gsn_pack16 *pack;
    int64_t edge_rows;
    float *out;
} gsn_layer_pack16_call;
int gsn_count_layer_step_hip(const gsn_count_call *count, const gsn_layer_pack16_call *layer, void *event_between, void *stream);
/* event_between: a hipEvent_t recorded on `stream` between the two launches, or NULL (a measuring host brackets the two kernels of the one
 * call with it: bench.py's per-kernel HIP-event times). */
/* The same step on code keys (gsn_count_encode_keys_side_hip + the KEYS variant of the packed-row layer kernel): the counting launch leaves
 * count->side's CSR and `keys` instead of the two packs, the layer gathers its x_i / x_j / x_v operand rows from `node_dict` (fp16
 * [dict_rows][32], the node dictionary described at gsn_count_keys, <= 256 rows, 16-byte aligned, constant per class configuration) through
 * the key bytes and expands its edge-level operand rows from idmask[perm[e]] | bond mask << side->edge_col0 through a constant table in
 * LDS.  The operand fragments are those of the pack path bit for bit, and so are the layer rows.  count->pack and layer->pack are not read
 * (count->pack_col0 is); the edge stage's blocks 0 / 1 / 2 must be indexed by side->sorted_target / sorted_other / perm.  Two launches, no
 * allocation, no host synchronisation, capturable; event_between as above. */
/* The constant table that variant expands the edge-level operand rows from, as its kernel fills it into LDS: host array fp16 bits [256][8],
 * entry b = the eight values 0 / 1.0 (0x3c00) of the bits of b, value j from bit j (no device work). */
int gsn_layer_keys_byte_table(uint16_t *dst);
int gsn_count_layer_step_keys_hip(const gsn_count_call *count, const gsn_layer_pack16_call *layer, const gsn_count_keys *keys,
                                  const uint16_t *node_dict, int64_t dict_rows, void *event_between, void *stream);
/* The x_i tables of that step.  Chunks 0 and 1 of an edge row -- x_i, with the folded bias on column 31 -- are the dictionary row of the
 * row's TARGET, and their products stand at the front of the edge stage's accumulation chain, so the accumulators behind them depend on
 * that dictionary row alone.  gsn_layer_key_tables_hip runs those products (the layer kernel's own instruction sequence on the prepared
 * fragments) once per dictionary row and writes fp32 tabs[4][gsn_layer_key_tables_max_rows()][32] (feature block, dictionary row, feature;
 * gsn_layer_key_tables_words() words); gsn_count_layer_step_tabs_hip is gsn_count_layer_step_keys_hip whose layer starts every block's
 * accumulators from the table row of the row's target and multiplies the remaining three chunks: 24 matrix instructions per block in place
 * of 40, the same bits.  dict_rows <= gsn_layer_key_tables_max_rows() (31; GSN_E_UNSUPPORTED beyond); `tabs` belongs to one (prepared
 * buffer, dictionary) pair and is made again when either changes; tabs == NULL is gsn_count_layer_step_keys_hip.  One tiny launch, capturable. */
int64_t gsn_layer_key_tables_words(void);
int64_t gsn_layer_key_tables_max_rows(void);
int gsn_layer_key_tables_hip(const void *prepared, const uint16_t *node_dict, int64_t dict_rows, float *tabs, void *stream);
int gsn_count_layer_step_tabs_hip(const gsn_count_call *count, const gsn_layer_pack16_call *layer, const gsn_count_keys *keys,
                                  const uint16_t *node_dict, int64_t dict_rows, const float *tabs, void *event_between, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-2  dense stage on DIRECT rows with fp16x3 matrix arithmetic (device): the same operation as gsn_linear_fwd_hip
 *     out[m, :] = act( bn( cat(blocks[0][m], blocks[1][m], ..) W^T + b ) )          (models_misc.py:52-58)
 * for blocks without a row index (node-level stages: the node product of a wide layer, its K = 260 node stage, jk projections,
 * the d = 300 ogb stages).  Two fp16 planes per operand after an exact power-of-two scaling (every input row by its largest
 * magnitude -- a pre-pass inside the call --, every output column of W by its largest entry), three plane products per fp32
 * product on the 16-bit matrix pipe, fp32 accumulation: the error of an fp32 FMA loop at half the matrix work of the bf16x6
 * kernel, over the whole fp32 exponent range; a row with an Inf / NaN comes out NaN.
 *   gsn_linear_f16x3_kpad(K)          K rounded up to whole K slices of 32 columns (two at least)
 *   gsn_linear_f16x3_prepare_hip      splits W [n_out][K] once: planes = 2 * n_out * kpad(K) fp16 values (laid out
 *                                     [n_out][kpad / 32][high | low][32]: one cache line per row and slice), col_inv = n_out floats
 *                                     (device buffers of the caller; valid until W changes)
 *   gsn_linear_f16x3_scratch_bytes    size of row_scratch for m_rows rows of K columns: the rows' inverse scales and their two
 *                                     fp16 planes (split once per call by a pre-pass, read by every column tile)
 *   gsn_linear_f16x3_fwd_hip          blocks: data + width only (idx / idx32 must be NULL), widths multiples of 4, 16-byte
 *                                     aligned; row_scratch: gsn_linear_f16x3_scratch_bytes(m_rows, K) bytes, 16-byte aligned;
 *                                     bias / bn_* / act as gsn_linear_fwd_hip
 *   gsn_linear_f16x3_fwd_stats_hip    the train-mode BatchNorm stage (models_misc.py:52-58, bn in train mode): out = the pre-BN rows
 *                                     x W^T + b, and their fp64 column sums / sums of squares ADDED to stats[2][n_out] by the same
 *                                     launch (gsn_linear_fwd_hip's `stats` contract); n_out a multiple of 4, out 16-byte aligned
 * ---------------------------------------------------------------------------------------------------------------- */
int64_t gsn_linear_f16x3_kpad(int64_t k_total);
int64_t gsn_linear_f16x3_mpad(int64_t m_rows);   /* rows of a row scratch: m_rows + at least 128 rows of zero planes, in whole 256-row tiles */
int64_t gsn_linear_f16x3_scratch_bytes(int64_t m_rows, int64_t k_total);
int gsn_linear_f16x3_prepare_hip(const float *W, int64_t n_out, int64_t k_total, void *planes, float *col_inv, void *stream);
/* the same from a weight given through element strides (W[j][k] at W + j * w_row_stride + k * w_col_stride; a transposed view of a row-major
 * matrix: 1, leading dimension) */
int gsn_linear_f16x3_prepare_strided_hip(const float *W, int64_t n_out, int64_t k_total, int64_t w_row_stride, int64_t w_col_stride,
                                         void *planes, float *col_inv, void *stream);
int gsn_linear_f16x3_fwd_hip(int64_t m_rows, int n_blocks, const gsn_block *blocks, const void *planes, const float *col_inv,
                             const float *bias, int64_t n_out, const float *bn_mean, const float *bn_scale, const float *bn_shift,
                             int act, float *row_scratch, float *out, void *stream);
int gsn_linear_f16x3_fwd_stats_hip(int64_t m_rows, int n_blocks, const gsn_block *blocks, const void *planes, const float *col_inv,
                                   const float *bias, int64_t n_out, float *row_scratch, float *out, double *stats, void *stream);
/* The rows' pre-pass by itself (row_scratch left exactly as gsn_linear_f16x3_fwd_hip leaves it: [mpad(m_rows)] inverse row scales,
 * then [mpad(m_rows)] rows of kpad(K) / 32 lines of 32 high | 32 low halfs; rows past m_rows hold zeros), and the product over rows split EARLIER (row_scratch is read, not written; blocks
 * give the widths only).  A training step splits every row set once: the forward product's scratch of X and the input-gradient product's
 * scratch of gH are what gsn_wgrad_f16x3_hip multiplies. */
int gsn_linear_f16x3_split_rows_hip(int64_t m_rows, int n_blocks, const gsn_block *blocks, float *row_scratch, void *stream);
int gsn_linear_f16x3_fwd_presplit_hip(int64_t m_rows, int n_blocks, const gsn_block *blocks, const void *planes, const float *col_inv,
                                      const float *bias, int64_t n_out, const float *bn_mean, const float *bn_scale, const float *bn_shift,
                                      int act, float *row_scratch, float *out, void *stream);
int gsn_linear_f16x3_fwd_stats_presplit_hip(int64_t m_rows, int n_blocks, const gsn_block *blocks, const void *planes, const float *col_inv,
                                            const float *bias, int64_t n_out, float *row_scratch, float *out, double *stats, void *stream);
/* gsn_bn_act_hip (out = act((h - mean) * scale + shift), models_misc.py:52-59's BatchNorm + activation on finished statistics) writing the row
 * scratch of its output -- for a stage output that only feeds the next product on the fp16x3 kernel (gsn_linear_f16x3_fwd_[stats_]presplit_hip) and
 * that product's plane weight gradient: no row pre-pass; `out` (fp32 rows) may be NULL.  n_cols a multiple of 4, at most 640. */
int gsn_bn_act_planes_hip(int64_t m_rows, int64_t n_cols, const float *h, const float *mean, const float *scale, const float *shift, int act,
                          float *out, float *row_scratch, void *stream);
/* HP-2 adjoint: weight gradient of a dense stage from fp16 planes (r06; torch.nn.Linear's weight.grad under models_misc.py:52-58):
 *     grad_w[n_out][K] += gH^T X
 * g_scratch = the row scratch of gH [m_rows][n_out] (its "K" is n_out), x_scratch = the row scratch of X [m_rows][K], both as
 * gsn_linear_f16x3_fwd_hip / _split_rows_hip leave them.  Three fp16 plane products per fp32 product; the per-row scales of the two
 * operands are reconciled per slab of rows inside the kernel (csrc/wgrad_f16.hip).  Same contract as gsn_wgrad_hip otherwise: grad_w is
 * ADDED to with float atomics (order varies in the last bits from run to run); a row with an Inf / NaN in gH or X makes the tile NaN. */
int gsn_wgrad_f16x3_hip(int64_t m_rows, int64_t n_out, int64_t k_total, const void *g_scratch, const void *x_scratch, float *grad_w,
                        void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * HP-2  edge stage of a `general` layer with the node part of its Linear taken out of the edge loop (device, fp32).
 * msg_fn's first Linear acts on cat(x_i, x_j, z_e) (GSN_sparse.py:166-171, GSN_edge_sparse.py:160-165, MPNN twins);
 * cat(x_i, x_j, z_e) W^T = x_i W_i^T + x_j W_j^T + z_e W_z^T, so the caller computes P = x [W_i | W_j]^T once per NODE
 * (gsn_linear_fwd_hip, N rows instead of E; bias and eval-mode BatchNorm folded into P_i and the weights) and this entry does
 *     out[t] = sum_{e : tgt(e) = t} act( P_i[t] + P_j[src(e)] + z_e W_z^T )            (GSN_edge_sparse.py:136-139 scatter-add)
 *   seg_ptr, sorted_src, perm   the target-sorted CSR of gsn_csr_build_hip / gsn_csr_build_graphs_hip
 *   p_i, p_j   fp32 device rows of `pitch` floats (two column ranges of one [N][2 d] matrix, or two matrices), d columns used
 *   z0, z1     per-edge blocks [E][w0], [E][w1] (identifiers / edge features; widths multiples of 4, w0 + w1 <= 16) or NULL
 *   wz_t       [w0 + w1][d] = W_z^T;   act 0 identity / 1 relu;   out [N][d] fully overwritten;  d multiple of 4, <= 256
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_edge_split_sum_hip(int64_t n_nodes, int64_t n_edges, const int32_t *seg_ptr, const int32_t *sorted_src,
                           const int32_t *perm, const float *p_i, const float *p_j, int64_t pitch, const float *z0,
                           int64_t w0, const float *z1, int64_t w1, const float *wz_t, int64_t d, int act, float *out,
                           void *stream);

/* The same CSR for a PyG-collated batch, one launch.  A batch is a disjoint union (torch_geometric's Batch / the reference's
 * DataLoader, main.py:19, utils_data_prep.py:35-60): graph g owns the consecutive columns edge_ptr[g] .. edge_ptr[g+1] of
 * edge_index and the consecutive vertices node_ptr[g] .. node_ptr[g+1], so every graph is sorted on its own in LDS (one wave
 * per graph) -- no global atomics, no global scan, same stable result as gsn_csr_build_hip.
 *   node_ptr, edge_ptr  int64 device [n_graphs + 1] (the arrays gsn_count_hip takes)
 *   max_nodes, max_edges  upper bounds over the graphs (size LDS: (2 (max_nodes + 1) + 2 max_edges) * 4 B <= 64 KiB, else
 *                       GSN_E_UNSUPPORTED -> use gsn_csr_build_hip)
 *   index, other, seg_ptr, perm, sorted_target, sorted_other   as gsn_csr_build_hip
 *   status              int32 device [1], zeroed by the caller: raised to GSN_ST_BAD_INDEX when a column's `index` entry lies
 *                       outside its graph's vertex range (the arrays do not describe a collated batch; outputs are then
 *                       unspecified), GSN_ST_TOO_LARGE when a graph exceeds max_nodes / max_edges */
int gsn_csr_build_graphs_hip(int64_t n_graphs, const int64_t *node_ptr, const int64_t *edge_ptr, int64_t n_nodes,
                             int64_t n_edges, int64_t max_nodes, int64_t max_edges, const int64_t *index,
                             const int64_t *other, int32_t *seg_ptr, int32_t *perm, int32_t *sorted_target,
                             int32_t *sorted_other, int32_t *status, void *stream);

int gsn_segsum_prepare_hip(int64_t n_seg, int64_t n_rows, const int32_t *seg_ptr, const int32_t *row_target,
                           int64_t n_out, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Identifier encoding (device).  The multi-hot encoding the reference applies to the integer identifiers in front of
 * every GSN layer: utils_graph_learning.one_hot_encoder.forward (:170-187) via DiscreteEmbedding('one_hot_encoder')
 * (models_graph_classification.py:222).  values int64 [M][C] -> out fp32 [M][sum n_classes], column c becoming
 * n_classes[c] floats with a single 1 at index values[r][c].  n_classes is a HOST array.  clamp != 0: indices are
 * clamped into [0, n_classes[c]-1] (the reference would raise on an out-of-range index).
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_one_hot_hip(int64_t m_rows, int n_cols, const int64_t *values, const int32_t *n_classes, int clamp, float *out,
                    void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Dataset-level dense recoding of integer columns (device): utils_encoding.one_hot_unique (utils_encoding.py:37-59),
 * i.e. per column np.unique(values[:, c], return_inverse=True): codes[r][c] = rank of values[r][c] among the distinct
 * values of column c, n_distinct[c] = their number (the reference's `d`).
 *   gsn_column_range_hip : col_min / col_max (device int64 [C]) of values int64 [M][C]; also what one_hot_max needs
 *                          (utils_encoding.py:62-69: d[c] = max + 1).
 *   gsn_column_ranks_hip : col_min as produced above; col_base (device int64 [C+1]) = prefix sums of the per-column table
 *                          sizes (max - min + 1), which the caller computes after reading the ranges back;
 *                          table = device scratch of table_elems = col_base[C] int32.
 * All asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_column_range_hip(int64_t m_rows, int n_cols, const int64_t *values, int64_t *col_min, int64_t *col_max,
                         void *stream);
int gsn_column_ranks_hip(int64_t m_rows, int n_cols, const int64_t *values, const int64_t *col_min,
                         const int64_t *col_base, int64_t table_elems, int32_t *table, int64_t *codes,
                         int64_t *n_distinct, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The same recoding over the FULL int64 range, by sorting (device): utils_encoding.one_hot_unique (utils_encoding.py:37-59) for
 * columns whose ranges are too wide for the presence table above -- counts of cliques, paths and stars in graphs that are not
 * molecules pass 2^28.  Order is signed int64 order (keys are compared as value ^ 2^63, never through value - min): a column may
 * hold INT64_MIN and INT64_MAX.
 *   values      int64 device [M][C]
 *   uniques     int64 device [C][M]: the first n_distinct[c] entries of uniques + c*M are the distinct values of column c in
 *               increasing order (np.unique(values[:, c])); the rest of the row is not written
 *   n_distinct  int64 device [C]
 *   codes       int64 device [M][C]: codes[r][c] = index of values[r][c] in that column's distinct values (return_inverse)
 *   scratch     device, 8-byte aligned, scratch_bytes >= gsn_unique_sort_scratch_bytes(M, C) (GSN_E_NOSPACE below): the sorted
 *               keys and one counter per 1024 keys -- 8 C (1 + 1/1024) bytes per row, rounded up to 256 bytes twice.
 *               gsn_unique_sort_scratch_bytes takes host arguments only, makes no GPU call and is 0 for an empty shape.
 * A keys-only bitonic sort (tiles of 4096 keys in 32 KiB of LDS, wave64, 256 threads), a compaction of the run starts and one
 * binary search per element: no payload, no order-dependent scatter -- two runs give the same bytes in all three outputs.  M == 0
 * or C == 0: nothing is launched, GSN_OK.  Null pointers with a non-empty shape: GSN_E_INVALID.  More than 65535 columns or 2^40
 * elements: GSN_E_UNSUPPORTED.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------------------------------- */
int64_t gsn_unique_sort_scratch_bytes(int64_t m_rows, int64_t n_cols);
int gsn_unique_sort_hip(int64_t m_rows, int64_t n_cols, const int64_t *values, int64_t *uniques, int64_t *n_distinct,
                        int64_t *codes, void *scratch, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Codes of further rows under a FITTED recoding (device): what utils_encoding.one_hot_unique (utils_encoding.py:37-59) cannot
 * do in the reference, which encodes train and test together -- rows that were not in the dataset get the codes the model was
 * trained with.
 *   values        int64 device [R][C]
 *   uniques       int64 device, flat: column c's sorted distinct values are uniques[col_ptr[c] .. col_ptr[c+1])
 *   col_ptr       int64 device [C+1]
 *   mode          GSN_LOOKUP_STRICT: codes[r][c] = index of values[r][c] among column c's values; a value that is not among
 *                 them (every value of a column with none) gets -1, raises *status to GSN_ST_UNSEEN and lowers *first_unseen
 *                 to r*C + c.  status: int32 device [1], zeroed by the caller; first_unseen: int64 device [1], set to -1 by the
 *                 caller (compared as unsigned), so it ends as the smallest r*C + c of an unseen value -- row first_unseen / C.
 *                 GSN_LOOKUP_CLAMP: codes[r][c] = max(0, (number of column c's values <= values[r][c]) - 1): the nearest
 *                 fitted value not above, 0 below the smallest and for a column with no values (the analogue of the step's
 *                 `clamp`); status and first_unseen are not touched and may be NULL.
 *   codes         int64 device [R][C]
 * R == 0 or C == 0: nothing is launched, GSN_OK.  Null pointers with a non-empty shape: GSN_E_INVALID (uniques may be NULL when
 * every column is empty).  Asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_lookup_codes_hip(int64_t n_rows, int64_t n_cols, const int64_t *values, const int64_t *uniques, const int64_t *col_ptr,
                         int mode, int64_t *codes, int32_t *status, int64_t *first_unseen, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Embedding of categorical columns (device): utils_graph_learning.multi_embedding.forward (:151-163), the
 * DiscreteEmbedding('embedding') of identifiers / degrees / node and edge types, and the same shape as ogb's
 * AtomEncoder / BondEncoder ('atom_encoder' / 'bond_encoder', :99-107).  codes int64 [M][C]; table c is fp32
 * [rows_c][d] row-major.  meta (device int64 [2C]) = table base addresses then rows_c.  concat != 0: out [M][C*d] is the
 * concatenation, else out [M][d] the sum over columns.  status (device int32, caller-zeroed) is raised to
 * GSN_ST_BAD_INDEX when a code is outside its table (that row's values are NaN).  bwd accumulates grad_out into the gradient tables named by
 * grad_meta (caller zero-fills them).  table_rows = the row counts again as a HOST array [C] (NULL allowed in fwd): they
 * pick the kernel -- tables that together have <= 448 rows are held in LDS per workgroup (64-wide slices), larger ones
 * are read / accumulated in HBM; the backward of summed embeddings over >= 4096 rows is the product OneHot(codes)^T grad_out on the
 * matrix pipe (exact bf16 planes, fp32 accumulation).
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_embed_fwd_hip(int64_t m_rows, int n_cols, int d, int concat, const int64_t *codes, const int64_t *meta,
                      const int64_t *table_rows, float *out, int32_t *status, void *stream);
int gsn_embed_bwd_hip(int64_t m_rows, int n_cols, int d, int concat, const int64_t *codes, const int64_t *grad_meta,
                      const int64_t *table_rows, const float *grad_out, void *stream);
/* The same backward with the gradient tables inside ONE caller-zeroed device allocation: table c starts at grad_flat +
 * table_offsets[c] floats (table_offsets, table_rows: HOST arrays [C]).  The table addresses travel as launch arguments: no device pointer
 * array, so no host-to-device copy per call and no memcpy node per embedding in a captured training step (utils_graph_learning.py:134-167
 * under train_test_funcs.py:88-106 at the reference's batch sizes).  gsn_embed_bwd_flat_supported: 1 when the shape is handled (<= 16
 * code columns; tables that fit the LDS slices or the matrix-pipe product), else 0 and gsn_embed_bwd_flat_hip returns
 * GSN_E_UNSUPPORTED -- use gsn_embed_bwd_hip then. */
int gsn_embed_bwd_flat_supported(int64_t m_rows, int n_cols, int concat, const int64_t *table_rows);
int gsn_embed_bwd_flat_hip(int64_t m_rows, int n_cols, int d, int concat, const int64_t *codes, float *grad_flat,
                           const int64_t *table_offsets, const int64_t *table_rows, const float *grad_out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * First Linear of msg_fn over one-hot encoded inputs as a weight-row gather with fused bias / BatchNorm / activation
 * and fused scatter-add (device).  Replaces, for inputs that are DiscreteEmbedding('one_hot_encoder') outputs
 * (utils_graph_learning.py:78-81, models_graph_classification.py:205-222), the reference's sequence
 *     one_hot -> cat(x_i, x_j, ids, e) -> msg_fn.fc[0] -> bn -> act     (GSN_edge_sparse.py:152-170, models_misc.py:52-59)
 *     -> torch.sparse.sum scatter-add                                   (GSN_edge_sparse.py:136-139)
 * Row q of the target-sorted edge order takes, per slot s, the code  codes[idx[q] * stride + col]  (idx NULL: row q) and
 * adds row  w_off + code  of WT = W^T ([k_total][n_out] fp32 row-major):
 *     out[seg_target[q]] += act(bn(bias + sum_s WT[w_off_s + code_s]))
 * `out` [n_targets][n_out] must have been prepared with gsn_segsum_prepare_hip; seg_target int32 [m_rows] ascending.
 * stats != NULL: statistics pass instead -- fp64 [2][n_out] column sums of (bias + sum) and of its square (caller
 * zero-fills), no `out`.  status (device int32, caller-zeroed) is raised to GSN_ST_BAD_INDEX if a code is outside
 * [0, n_classes) (the code is then treated as 0).  act: 0 identity, 1 relu, 2 elu, 3 tanh.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GSN_MAX_CODE_SLOTS 16
typedef struct gsn_code_slot {
    const int64_t *codes;  /* device, [rows][stride] */
    const int32_t *idx;    /* device int32 [m_rows] row of `codes` feeding sorted position q, or NULL */
    int32_t stride, col;   /* row pitch of `codes` in elements, column used */
    int32_t w_off;         /* first row of this slot's block in WT */
    int32_t n_classes;     /* number of rows of that block */
    int32_t clamp;         /* != 0: codes are clamped into [0, n_classes-1] instead of being reported (cf. gsn_one_hot_hip) */
    int32_t reserved;
} gsn_code_slot;
int gsn_code_stage_supported(int n_slots, int64_t k_total, int64_t n_out);
int gsn_code_stage_fwd_hip(int64_t m_rows, int n_slots, const gsn_code_slot *slots, const float *WT, int64_t k_total,
                           const float *bias, int64_t n_out, const float *bn_mean, const float *bn_scale,
                           const float *bn_shift, int act, const int32_t *seg_target, float *out, double *stats,
                           int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * BatchNorm + activation applied to materialised pre-BN rows (device): y = act((h - mean) * scale + shift) per column,
 * models_misc.mlp.forward (:52-59) for a train-mode stage whose statistics were taken in the same pass that wrote h
 * (gsn_linear_fwd_hip with both `out` and `stats`).  h, out fp32 [M][C] row-major (may alias); vectors may be NULL.
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_bn_act_hip(int64_t m_rows, int64_t n_cols, const float *h, const float *mean, const float *scale,
                   const float *shift, int act, float *out, void *stream);
/* The statistics of materialised pre-BN rows (device): ADDS per-column sum and sum of squares of h [M][C] into stats double [2][C]
 * (caller zeroes it) -- what gsn_linear_fwd_hip's `stats` argument takes inside its product, for rows that another kernel wrote
 * (the fp16x3 dense kernel of a train-mode stage, models_misc.py:52-59 with nn.BatchNorm1d in training mode). */
int gsn_column_stats_hip(int64_t m_rows, int64_t n_cols, const float *h, double *stats, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Backward of a dense mlp stage  H = X W^T + b, Z = bn(H), Y = act(Z)  (models_misc.py:52-59) for inputs that are plain
 * row-major blocks (device).  What PyTorch autograd does for the reference's nn.Linear / BatchNorm1d / activation.
 *   gsn_bn_act_bwd_hip : grad_h = d/dH from grad_y.  y = the stage output (activation derivative is taken from it);
 *       train_bn != 0: batch-statistics BatchNorm -- h = pre-BN rows, mean / invstd = the batch statistics, coef =
 *       gamma * invstd, sums = fp64 [2][C] scratch (zero-filled) that receives sum(gZ) = grad beta and sum(gZ * xhat) =
 *       grad gamma;  train_bn == 0: grad_h = gZ * coef (coef NULL = 1; h, mean, invstd, sums unused);  train_bn == 2: BatchNorm
 *       on its running statistics (module in eval mode, models_misc.py:41-45 under model.eval()) with gradients for gamma / beta:
 *       h = pre-BN rows, mean / invstd = the running statistics, sums as above, grad_h = gZ * coef.
 *       grad_bias (fp64 [C], zero-filled, may be NULL) receives the column sums of grad_h.  grad_h may alias grad_y.
 *   gsn_wgrad_hip : grad_w[n_out][K] += grad_h^T X  with X the concatenation of `blocks` (direct, or gathered through idx / idx32 as
 *       in gsn_linear_fwd_hip: the x_i / x_j blocks of an edge stage are read where they lie); caller zero-fills.
 *   The input gradient is gsn_linear_fwd_hip(grad_h, weight = W^T).
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_bn_act_bwd_hip(int64_t m_rows, int64_t n_cols, const float *grad_y, const float *y, const float *h,
                       const float *mean, const float *invstd, const float *coef, int train_bn, int act, double *sums,
                       float *grad_h, double *grad_bias, void *stream);
/* The same for a BatchNorm stage (train_bn 1 or 2) WITHOUT reading the stage output: the activation's derivative is taken from
 * z = (h - mean) * coef + shift, recomputed from the pre-BN rows with the forward pass's expression (gsn_bn_act_hip) -- one read of
 * [M][C] less in each of the two passes (they are HBM-bound: 3 -> 2 and 4 -> 3 array passes). */
int gsn_bn_act_bwd_from_h_hip(int64_t m_rows, int64_t n_cols, const float *grad_y, const float *h, const float *mean,
                              const float *invstd, const float *coef, const float *shift, int train_bn, int act, double *sums,
                              float *grad_h, double *grad_bias, void *stream);
/* The same again for a stage whose grad_h is consumed as fp16 planes only (r06): no fp32 grad_h is written; row_scratch
 * (gsn_linear_f16x3_scratch_bytes(m_rows, n_cols) bytes, 16-byte aligned) receives grad_h's inverse row scales and planes, ready for
 * gsn_linear_f16x3_fwd_presplit_hip (the input gradient grad_h W) and gsn_wgrad_f16x3_hip.  n_cols a multiple of 4, at most 640.  grad_bias
 * receives the column sums analytically: zero under batch statistics (the statistics absorb a shift of H), coef * sum(gZ) on running ones. */
int gsn_bn_act_bwd_planes_hip(int64_t m_rows, int64_t n_cols, const float *grad_y, const float *h, const float *mean, const float *invstd,
                              const float *coef, const float *shift, int train_bn, int act, double *sums, float *row_scratch,
                              double *grad_bias, void *stream);
int gsn_wgrad_hip(int64_t m_rows, int64_t n_out, const float *grad_h, int n_blocks, const gsn_block *blocks, float *grad_w,
                  void *stream);
/* The folded first weight of update_fn for a `general` layer whose aggregation runs in front of msg_fn's last Linear (W2, b2) --
 * GSN_edge_sparse.py:153-170 / GSN_sparse.py:166-171 with  update_fn.fc[0](cat(x, sum_e(W2 r_e + b2))) = cat(x, S, deg) out^T:
 *   out [rows][d_x + h_cols + 1 + pad_cols] = [ w3[:, :d_x] | w3[:, d_x:] W2 | w3[:, d_x:] b2 | 0 ],   w3 [rows][d_x + a_cols] (row stride ld3),
 *   w2 [a_cols][h_cols] (row stride ld2), b2 [a_cols]; pad_cols zero columns (the degree block is passed four floats wide so that the
 *   stage's rows are staged as float4).  One launch, fp32 FMA dot products.
 * _bwd: g [rows][>= d_x + h_cols + 1] (row stride ldg; columns past d_x + h_cols are not read) -> g_w3 [rows][d_x + a_cols], g_w2 [a_cols][h_cols], g_b2 [a_cols] (all written,
 *   contiguous), one launch.  A training step rebuilds the fold at every step (the three matrices move). */
int gsn_fold_weights_fwd_hip(int64_t rows, int64_t d_x, int64_t a_cols, int64_t h_cols, int64_t pad_cols, const float *w3, int64_t ld3,
                             const float *w2, int64_t ld2, const float *b2, float *out, void *stream);
int gsn_fold_weights_bwd_hip(int64_t rows, int64_t d_x, int64_t a_cols, int64_t h_cols, const float *g, int64_t ldg, const float *w3,
                             int64_t ld3, const float *w2, int64_t ld2, const float *b2, float *g_w3, float *g_w2, float *g_b2,
                             void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * out[r] = concat_b blocks[b].data[idx_b[r]]  (device): torch.cat((x_i, x_j, identifiers, edge_features), -1) of
 * GSN_sparse.py:166-171 / GSN_edge_sparse.py:160-165 materialised as fp32 [M][sum widths].  Only the training path uses
 * it (the assembled rows feed the weight gradient); inference gathers on the fly inside the dense kernels.
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_gather_cat_hip(int64_t m_rows, int n_blocks, const gsn_block *blocks, float *out, void *stream);

/* out[r] = x[r] + table[idx[r]]  (device; fp32 [M][d], table [T][d], idx int64 [M]): the virtual-node embedding added to the vertices of
 * its graph, models_graph_classification_ogb_original.py:236 `x + vn_embedding[data.batch]`, in one pass.  A row whose index lies
 * outside [0, T) comes out NaN.  Adjoint: grad x = grad out; grad table = the sum readout of grad out (gsn_propagate_fwd_hip). */
int gsn_add_gathered_hip(int64_t n_rows, int64_t d, const float *x, const float *table, const int64_t *idx, int64_t n_table, float *out,
                         void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Train-mode BatchNorm1d bookkeeping (device), what nn.BatchNorm1d does around the normalisation (models_misc.py:41-45):
 * stats fp64 [2][C] = column sum and sum of squares of the M pre-BN rows ->  mean, invstd = 1/sqrt(biased var + eps),
 * scale = gamma * invstd, shift = beta (gamma / beta NULL: 1 / 0), and running_mean / running_var (both or neither)
 * updated with `momentum` and the unbiased variance.  All vectors fp32 [C], one launch.
 * ---------------------------------------------------------------------------------------------------------------- */
int gsn_bn_finalize_hip(int64_t n_cols, int64_t m_rows, double eps, double momentum, const double *stats, const float *gamma,
                        const float *beta, float *running_mean, float *running_var, float *mean, float *invstd, float *scale,
                        float *shift, void *stream);
/* gsn_bn_finalize_count_hip and gsn_bn_act_hip in one launch (same expressions, same values): the batch statistics' vectors, the running
 * statistics and the counter are written, then out = act((h - mean) * scale + shift) over the M rows.  For row counts where a launch costs
 * more than the pass (the reference's batch sizes: 32 .. 128 graphs). */
int gsn_bn_finalize_act_hip(int64_t n_cols, int64_t m_rows, double eps, double momentum, const double *stats, const float *gamma,
                            const float *beta, float *running_mean, float *running_var, float *mean, float *invstd, float *scale,
                            float *shift, int64_t *num_batches_tracked, const float *h, int act, float *out, void *stream);

/* The same with nn.BatchNorm1d's `num_batches_tracked` (int64 [1], device; NULL = none) incremented by the kernel. */
int gsn_bn_finalize_count_hip(int64_t n_cols, int64_t m_rows, double eps, double momentum, const double *stats, const float *gamma,
                              const float *beta, float *running_mean, float *running_var, float *mean, float *invstd, float *scale,
                              float *shift, int64_t *num_batches_tracked, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The same bookkeeping and the BatchNorm adjoint over a PADDED batch (gsn_loader_collate_padded_hip), whose real rows are the prefix
 * [0, v) of the m_rows rows the stage runs over.  A row bound is (n_valid int64 [1], row_ptr int64 [n_slots + 1] or NULL, n_slots):
 *     v = clamp(row_ptr ? row_ptr[clamp(*n_valid, 0, n_slots)] : *n_valid, 0, m_rows)
 * read ON THE DEVICE by every kernel (n_slots = 0 with a NULL row_ptr); no device value causes a read outside row_ptr.  The host m_rows
 * (the capacity) only sizes launches and buffers, as in gsn_eval_accumulate_counted_hip.
 *
 * gsn_bn_finalize_bounded_hip stands in for gsn_bn_finalize_count_hip (one launch): stats = the [2][C] sums over ALL m_rows rows as the
 * product kernels leave them, h = the materialised pre-BN rows fp32 [m_rows, C].  The sums of the shorter of the row ranges [0, v) and
 * [v, m_rows) are taken from h -- directly, or subtracted from stats in fp64 -- so at most half the rows are read; then the vectors and
 * the running statistics follow with count v through the expressions of gsn_bn_finalize_count_hip (v == m_rows: the same bits).
 * v == 0: mean 0, invstd 1, scale 1, shift 0, running statistics untouched, the batch counted.  v == 1: variance 0, invstd
 * 1 / sqrt(eps), finite (the caller refuses that batch as torch does).  scratch: gsn_bn_finalize_bounded_scratch_bytes(n_cols) bytes,
 * 8-byte aligned, ZERO-FILLED by the caller before every call (fp64 partial sums and one ticket per 64 columns).
 *
 * gsn_bn_act_bwd_from_h_bounded_hip is gsn_bn_act_bwd_from_h_hip with the column sums over the rows < v, the divisor v, grad_bias over
 * the rows < v, and grad_h rows >= v written as +0 WITHOUT reading grad_y there (products over all m_rows rows then add exact zeros).
 * ---------------------------------------------------------------------------------------------------------------- */
int64_t gsn_bn_finalize_bounded_scratch_bytes(int64_t n_cols);
int gsn_bn_finalize_bounded_hip(int64_t n_cols, int64_t m_rows, double eps, double momentum, const double *stats, const float *h,
                                const int64_t *n_valid, const int64_t *row_ptr, int64_t n_slots, void *scratch, const float *gamma,
                                const float *beta, float *running_mean, float *running_var, float *mean, float *invstd, float *scale,
                                float *shift, int64_t *num_batches_tracked, void *stream);
int gsn_bn_act_bwd_from_h_bounded_hip(int64_t m_rows, int64_t n_cols, const float *grad_y, const float *h, const float *mean,
                                      const float *invstd, const float *coef, const float *shift, int train_bn, int act, double *sums,
                                      float *grad_h, double *grad_bias, const int64_t *n_valid, const int64_t *row_ptr, int64_t n_slots,
                                      void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Directional GSN aggregation (directional_gsn/nets/dgn_layer.py:30-56, nets/aggregators.py, nets/scalers.py).
 * For each node v, over its in-edges e = (u -> v) in edge-id order (the target-sorted CSR of edge_index[1]: seg_ptr [N+1],
 * perm [E] edge ids stable by target, src [E] = edge_index[0][perm]), with message h[u] (fp32 [N, d]) and vector field
 * w = cat(node_field[u] - node_field[v], edge_field[e]) (either part may be absent: width 0; edge_field rows by edge id):
 *   out[v, (s * A + slot) * d + f] = scaler_s(D) * aggregator(h[src], w[:, col], h[v])[f]        out fp32 [N, S * A * d]
 * for the n_aggs descriptors (A = n_aggs, slots a permutation of 0 .. A-1) and the n_scalers (<= 4) scaler codes; avg_d_log is
 * avg_d['log'].  The reference scales only when more than one scaler is given (dgn_layer.py:50): the caller then passes
 * GSN_DGN_IDENTITY alone.  Nodes without in-edges get a zero row.  A directional descriptor whose column is outside the field
 * returns GSN_E_INVALID before any launch (the reference raises IndexError).
 * Backward: grad_h [N, d] (fully written) = d L / d h from grad_out; grad_msg [E, d] is caller scratch (per-edge message gradients
 * at edge ids), src_seg_ptr / src_perm the CSR of edge_index[0].  Deterministic (no atomics); max / min route the gradient to the
 * lowest edge id holding the extremum.  The fields carry no gradient.
 * ---------------------------------------------------------------------------------------------------------------- */
enum {
    GSN_DGN_MEAN = 0, GSN_DGN_SUM = 1, GSN_DGN_MAX = 2, GSN_DGN_MIN = 3, GSN_DGN_VAR = 4, GSN_DGN_STD = 5,
    GSN_DGN_DIR_AV = 6,          /* sum h |w| / (sum |w| + EPS) */
    GSN_DGN_DIR_SOFTMAX = 7,     /* sum h softmax_edges(alpha |w|) */
    GSN_DGN_DIR_DX = 8,          /* |sum h w' - (sum w') h_in|, w' = w / (sum |w| + EPS) */
    GSN_DGN_DIR_DX_NOABS = 9,    /* the same without abs */
    GSN_DGN_DIR_DX_BALANCED = 10 /* dx with w' = (relu(w) / (sum relu(w) + EPS) + relu(-w) / (sum relu(-w) + EPS)) / 2 */
};
enum { GSN_DGN_IDENTITY = 0, GSN_DGN_AMPLIFICATION = 1, GSN_DGN_ATTENUATION = 2 };
typedef struct {
    int32_t kind;  /* GSN_DGN_* */
    int32_t col;   /* vector-field column of the directional kinds */
    float alpha;   /* GSN_DGN_DIR_SOFTMAX */
    int32_t slot;  /* output aggregator index */
} gsn_dgn_agg;
int gsn_dgn_aggregate_fwd_hip(int64_t n_nodes, int64_t n_edges, int64_t d, const int32_t *seg_ptr, const int32_t *perm, const int32_t *src,
                              const float *h, const float *node_field, int64_t node_stride, int64_t node_width, const float *edge_field,
                              int64_t edge_stride, int64_t edge_width, const gsn_dgn_agg *aggs, int n_aggs, const int32_t *scalers,
                              int n_scalers, double avg_d_log, float *out, void *stream);
int gsn_dgn_aggregate_bwd_hip(int64_t n_nodes, int64_t n_edges, int64_t d, const int32_t *seg_ptr, const int32_t *perm, const int32_t *src,
                              const int32_t *src_seg_ptr, const int32_t *src_perm, const float *h, const float *node_field,
                              int64_t node_stride, int64_t node_width, const float *edge_field, int64_t edge_stride, int64_t edge_width,
                              const gsn_dgn_agg *aggs, int n_aggs, const int32_t *scalers, int n_scalers, double avg_d_log,
                              const float *grad_out, float *grad_msg, float *grad_h, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Laplacian eigenvector fields of the directional GSN (directional_gsn/data/HIV.py:21-51, positional_encoding: scipy's ARPACK once per
 * graph).  For every graph of the launch, with A[u, v] = number of arcs u -> v (duplicates add, self loops count) and
 * d = max(in-degree, 1):   norm NONE: L = diag(d) - A    SYM: L = I - D^-1/2 A D^-1/2    WALK: L = I - D^-1 A,
 * the k (1 .. GSN_EIG_KMAX) eigenpairs of smallest eigenvalue in increasing order (equal eigenvalues in the solver's own, deterministic
 * order):  vec fp32 [N, k] row-major (row node_ptr[g] + i: vertex i of graph g), val fp32 [G, k].  Every vector has unit 2-norm and its
 * component of largest magnitude is positive (lowest vertex on exact ties).  A graph with n < k vertices gets zero vectors and NaN values
 * in columns j >= n.  Two runs give the same bits.
 *   node_ptr / edge_ptr   int64 device [G + 1] (G = n_graphs_total), edge_index int64 device [2, n_edges] with batch-global vertex ids: the
 *                         arrays gsn_count_layer_step_hip takes
 *   graph_ids, n_ids      the graphs of this launch (int32 device, no id twice), or NULL: all G graphs
 *   n_class               32, 64, 128 or 256: the most vertices a graph of this launch may have.  32 .. 128 solve in LDS; 256 solves in
 *                         `scratch`, gsn_laplacian_eig_scratch_floats(256, n_ids) floats of device memory (0 for the other classes)
 *   max_sweeps            1 .. 64: the bound of the Jacobi iteration
 *   status                int32 device [G], written for every graph of the launch: GSN_ST_OK; GSN_ST_TOO_LARGE (more than n_class
 *                         vertices), GSN_ST_BAD_INDEX (an arc end outside the graph's vertices, or node_ptr outside the batch) and
 *                         GSN_ST_ASYMMETRIC (A != A^T) with zero rows and NaN values; GSN_ST_NO_CONVERGENCE with the last iterate's rows
 *   sweeps_used           int32 device [G] or NULL: the sweeps each graph ran
 * One workgroup per graph, one launch per call, asynchronous on `stream`; graphs outside the launch keep their rows.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GSN_EIG_KMAX 8
enum { GSN_EIG_NORM_NONE = 0, GSN_EIG_NORM_SYM = 1, GSN_EIG_NORM_WALK = 2 };
int gsn_laplacian_eig_hip(int64_t n_graphs_total, const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                          int64_t n_edges, const int32_t *graph_ids, int64_t n_ids, int n_class, int norm, int k, int max_sweeps,
                          float *vec, float *val, int32_t *status, int32_t *sweeps_used, float *scratch, int64_t scratch_floats,
                          void *stream);
int64_t gsn_laplacian_eig_scratch_floats(int n_class, int64_t n_ids);

/* ------------------------------------------------------------------------------------------------------------------
 * Adam update of every parameter of every parameter group in ONE launch (train_test_funcs.py:22: torch.optim.Adam(model.parameters(),
 * lr, weight_decay); :106: optimizer.step()).  torch.optim.Adam with amsgrad = False, maximize = False; per element, in fp32:
 *   g' = g + wd p            (decoupled: p <- p (1 - lr wd), g' = g)
 *   m <- b1 m + (1 - b1) g'        v <- b2 v + (1 - b2) g'^2        p <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * with bcK = 1 - bK^t, t = the tensor's step counter + 1; bc1, bc2 and lr / bc1 are taken in float64 once per chunk.
 *   tensors   int64 device [n_tensors][GSN_ADAM_TENSOR_WORDS]: parameter pointer (fp32), gradient pointer (fp32; 0: no gradient in this
 *             step -- parameter, moments and counter of the tensor stay as they are), offset of its exp_avg in `exp_avg` and of its
 *             exp_avg_sq in `exp_avg_sq` (in elements), element count, group index.  Pointers need 4-byte alignment only.
 *   chunks    int32 device [n_chunks][2]: (tensor, first element) of workgroup i, which updates elements [first, first +
 *             GSN_ADAM_CHUNK_ELEMS) of that tensor, clipped to its size.  Every element of every tensor lies in exactly one chunk.
 *   groups    float64 device [n_groups][GSN_ADAM_GROUP_DOUBLES]: lr, beta1, beta2, eps, weight_decay, decoupled (0 / 1), 0, 0.  Read by
 *             the kernel at every launch: a replayed HIP graph follows what the host writes here between replays.
 *   steps     fp32 device [n_tensors]: the step counters (fp32 as torch.optim.Adam keeps them).  The workgroup that finishes last adds 1
 *             to the counter of every tensor that had a gradient -- no second launch, no host-side counter.
 *   done      uint32 device, zero before the first call; the launch leaves it zero.  One optimizer = one word; calls that share it must
 *             be ordered (one stream, or one graph).
 *   max_elems the largest element count in `tensors` (the tables are device memory: the host cannot read them); more than 2^31 - 1 is
 *             GSN_E_UNSUPPORTED.
 * n_chunks == 0 launches nothing and returns GSN_OK.  Asynchronous on `stream`; two runs on the same inputs give the same bits.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GSN_ADAM_CHUNK_ELEMS 8192
#define GSN_ADAM_TENSOR_WORDS 6
#define GSN_ADAM_GROUP_DOUBLES 8
int gsn_adam_step_hip(int n_tensors, const int64_t *tensors, int64_t n_chunks, const int32_t *chunks, int n_groups, const double *groups,
                      float *exp_avg, float *exp_avg_sq, float *steps, unsigned *done, int64_t max_elems, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Evaluation on the device (train_test_funcs.py:94-103, :177-259; utils.py:164-187; utils_graph_learning.py:11-21).  Common to the
 * entries below: no float atomics, every reduction in a fixed order (two runs give the same bytes), workspaces from the caller, nothing
 * allocates, copies synchronously or synchronises -- every entry can be captured into a HIP graph.
 *
 * Masked mean loss -- train_test_funcs.py:98-101: is_labeled = (y == y); loss_fn(y_hat[is_labeled], y[is_labeled]) -- without the
 * boolean index.  Kinds after utils.py:164-175.  Element-wise kinds (BCE, L1, MSE): y_hat fp32 [rows, cols], y fp32 with the same element
 * count, a NaN target = unlabelled.  GSN_LOSS_CE: y_hat fp32 [rows, cols = classes], y int64 [rows]; a target outside [0, cols) makes the
 * loss NaN and that row's gradient zero.  Per-element values are fp32; they are summed in float64 over chunks of 1 024 consecutive elements
 * (rows for CE), the partials in chunk order, and the mean is rounded once: loss fp32 [1], count int64 [1] = the labelled elements (rows
 * for CE), both device memory.  No labelled element (an empty shape included): NaN loss, zero gradient (as torch); GSN_LOSS_CE with
 * rows > 0 and cols == 0 is GSN_E_INVALID.  rows * cols <= 65 536: ONE launch of one
 * workgroup, no scratch; beyond, a partial and a combine launch and gsn_masked_loss_scratch_bytes(kind, rows, cols) bytes of scratch.
 * Backward (one launch): grad_y_hat [rows, cols] = grad_loss[0] * d loss / d y_hat, recomputed from y_hat and y, with grad_loss (fp32)
 * and count (as the forward left it) READ FROM DEVICE MEMORY; zeros at unlabelled positions.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { GSN_LOSS_BCE = 0, GSN_LOSS_L1 = 1, GSN_LOSS_MSE = 2, GSN_LOSS_CE = 3 };
int64_t gsn_masked_loss_scratch_bytes(int kind, int64_t rows, int64_t cols);
int gsn_masked_loss_fwd_hip(int kind, int64_t rows, int64_t cols, const float *y_hat, const void *y, float *loss, int64_t *count,
                            void *scratch, int64_t scratch_bytes, void *stream);
int gsn_masked_loss_bwd_hip(int kind, int64_t rows, int64_t cols, const float *y_hat, const void *y, const float *grad_loss,
                            const int64_t *count, float *grad_y_hat, void *stream);
/* The same two launches with the row count READ FROM DEVICE MEMORY (a padded batch): rows >= v = clamp(*n_valid, 0, rows) are unlabelled
 * whatever they hold (integer pad targets of GSN_LOSS_CE are 0, not NaN) and are not read; loss, count and the gradient of the first v
 * rows are the bits of the entries above called with rows = v, gradient rows >= v are +0.  The host `rows` picks the launch shape and the
 * scratch size (gsn_masked_loss_scratch_bytes(kind, rows, cols)). */
int gsn_masked_loss_fwd_counted_hip(int kind, int64_t rows, int64_t cols, const float *y_hat, const void *y, const int64_t *n_valid,
                                    float *loss, int64_t *count, void *scratch, int64_t scratch_bytes, void *stream);
int gsn_masked_loss_bwd_counted_hip(int kind, int64_t rows, int64_t cols, const float *y_hat, const void *y, const int64_t *n_valid,
                                    const float *grad_loss, const int64_t *count, float *grad_y_hat, void *stream);

/* One batch of an evaluation epoch (train_test_funcs.py:193-202 and :234-251 per batch, without their .item() / .cpu()), in the launches
 * of the masked loss: the batch loss through the same device functions and partition (the same bits), then
 *   acc_f64[GSN_EVAL_WEIGHTED_LOSS] += (double)loss * num_graphs      acc_f64[GSN_EVAL_BATCH_LOSS] += (double)loss
 *   acc_f64[GSN_EVAL_METRIC]        += the fp32 reduction='sum' of L1Loss / MSELoss over every element (GSN_METRIC_L1 / _MSE; utils.py:177-183)
 *   acc_i64[GSN_EVAL_CORRECT]       += rows whose arg-max (first index of the row maximum) equals the target (GSN_METRIC_ACCURACY; CE only)
 *   acc_i64[GSN_EVAL_BATCHES]       += 1
 * and the batch's rows appended to pred_buf fp32 [capacity, cols] and true_buf [capacity, y_cols] (fp32, or int64 for GSN_LOSS_CE where
 * y_cols = 1) at row acc_i64[GSN_EVAL_CURSOR], which the call advances by `rows`: the cursor lives on the device, so a replayed capture
 * appends.  A batch that would pass `capacity` changes nothing but acc_i64[GSN_EVAL_STATUS] |= GSN_EVAL_OVERFLOW.  acc_f64 / acc_i64 have
 * GSN_EVAL_ACC_WORDS entries each, zeroed by the caller to start an epoch.  loss_out (fp32 [1], device) may be NULL.  Either buffer may be
 * NULL: nothing is appended to it.  Scratch as gsn_masked_loss_fwd_hip: gsn_eval_accumulate_scratch_bytes.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { GSN_METRIC_NONE = 0, GSN_METRIC_L1 = 1, GSN_METRIC_MSE = 2, GSN_METRIC_ACCURACY = 3 };
enum { GSN_EVAL_WEIGHTED_LOSS = 0, GSN_EVAL_BATCH_LOSS = 1, GSN_EVAL_METRIC = 2 };                          /* acc_f64 */
enum { GSN_EVAL_CURSOR = 0, GSN_EVAL_BATCHES = 1, GSN_EVAL_CORRECT = 2, GSN_EVAL_STATUS = 3 };              /* acc_i64 */
#define GSN_EVAL_ACC_WORDS 4
#define GSN_EVAL_OVERFLOW 1
int64_t gsn_eval_accumulate_scratch_bytes(int kind, int64_t rows, int64_t cols);
int gsn_eval_accumulate_hip(int kind, int metric, int64_t rows, int64_t cols, int64_t y_cols, const float *y_hat, const void *y,
                            int64_t num_graphs, double *acc_f64, int64_t *acc_i64, float *pred_buf, void *true_buf, int64_t capacity,
                            float *loss_out, void *scratch, int64_t scratch_bytes, void *stream);
/* The same with the row count READ FROM DEVICE MEMORY (a padded batch whose valid rows come first; gsn_loader_collate_padded_hip writes
 * n_valid): with v = clamp(*n_valid, 0, rows) it does exactly what gsn_eval_accumulate_hip does when called with rows = v and
 * num_graphs = v on the same pointers -- loss, metric and arg-max over the first v rows, v rows appended, cursor advanced by v, weight v,
 * nothing at all when v == 0 -- through the same device functions and the same partition.  The host `rows` only picks the launch shape and
 * the scratch size (gsn_eval_accumulate_scratch_bytes(kind, rows, cols)); rows behind v are never read. */
int gsn_eval_accumulate_counted_hip(int kind, int metric, int64_t rows, int64_t cols, int64_t y_cols, const float *y_hat, const void *y,
                                    const int64_t *n_valid, double *acc_f64, int64_t *acc_i64, float *pred_buf, void *true_buf,
                                    int64_t capacity, float *loss_out, void *scratch, int64_t scratch_bytes, void *stream);

/* ROC-AUC and average precision per column of y_pred fp32 [m_rows, n_cols] against y_true fp32 [m_rows, n_cols] (labels 0, 1, NaN =
 * unlabelled) -- what ogb's Evaluator computes through sklearn.metrics.roc_auc_score / average_precision_score (train_test_funcs.py:257-259)
 * -- from exact integer rank statistics.  Key of an element: (monotone uint32 image of the score, -0.0 as +0.0) << 1 | label; columns are
 * sorted by the network of gsn_unique_sort_hip; equal-score runs give, per column c,
 *   out_i64[c][0 .. 3) = { n_labelled, n_pos, U2 = sum over runs of pos * (2 * negatives below + negatives in the run) }
 *   out_f64[c][0 .. 2) = { auc = U2 / (2 n_pos n_neg),  ap = sum over runs, highest score first, of (pos / n_pos) * tp / (tp + fp) }
 *   status[c] (int32): GSN_RANK_ONE_CLASS (auc undefined: NaN), GSN_RANK_NO_POSITIVE (ap undefined: NaN), GSN_RANK_NONFINITE (a NaN or
 *   infinite prediction in a labelled row), GSN_RANK_BAD_LABEL (a label other than 0, 1, NaN); with either of the last two the numbers of
 *   the column are those of its remaining rows and the caller raises.
 * m_rows < 2^31, n_cols <= 65 535 (GSN_E_UNSUPPORTED beyond).  scratch: gsn_rank_metrics_scratch_bytes(m_rows, n_cols), 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { GSN_RANK_ONE_CLASS = 1, GSN_RANK_NO_POSITIVE = 2, GSN_RANK_NONFINITE = 4, GSN_RANK_BAD_LABEL = 8 };
int64_t gsn_rank_metrics_scratch_bytes(int64_t m_rows, int64_t n_cols);
int gsn_rank_metrics_hip(int64_t m_rows, int64_t n_cols, const float *y_pred, const float *y_true, int64_t *out_i64, double *out_f64,
                         int32_t *status, void *scratch, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * One collated batch of a device-resident dataset in ONE launch (gsn_amd/loader.py; the reference's `for data in loader` over
 * torch_geometric's DataLoader, train_test_funcs.py:48-174).  The dataset lives on the device as one concatenation per attribute (a
 * FIELD) with an int64 row pointer [G + 1] over its graphs; a batch is positions [first, first + batch) of an epoch's `order` (int64
 * device [n_graphs_total]: the graph at every position).  `plan` (int64 device [n_classes][n_graphs_total]) holds, per pointer class c
 * and position i, the rows of class c in front of position i INSIDE ITS OWN BATCH: the destination row of that graph's segment.
 *   fields   host array of n_fields <= GSN_LOADER_MAX_FIELDS records; the table travels BY VALUE in the launch (no device copy of it):
 *     src, row_ptr   the field's storage and its row pointer (device); graph g owns rows [row_ptr[g], row_ptr[g + 1])
 *     dst, dst_rows  this batch's output and its row count (columns for GSN_LOADER_EDGE_INDEX); dst_rows == 0: nothing is read or
 *                    written for the field (dst may be NULL)
 *     row_bytes, elem_bytes   bytes of a row (a multiple of elem_bytes) and of the unit it is moved in (4 or 8; src and dst aligned to it)
 *     ptr_class      the row of `plan` that holds the field's destination rows
 *     kind           GSN_LOADER_COPY: rows copied unchanged.  GSN_LOADER_EDGE_INDEX: int64 [2, *] with graph-local vertex ids, source
 *                    row stride src_stride and destination row stride dst_stride (elements); both rows are copied and
 *                    plan[inc_class][position] -- the vertices in front of the graph in its batch -- is added to every value
 *     flags          GSN_LOADER_F_NODES marks the field whose rows are the vertices (`x`): its wave also writes batch_vec[row] = slot
 *                    for its rows, node_ptr_out[slot] and, for the last slot, node_ptr_out[batch]; the GSN_LOADER_EDGE_INDEX field
 *                    does the same for edge_ptr_out.  Either output may be NULL (not written).
 * One wave per (field, slot) pair, pairs handed out by a grid-stride loop; every output byte has exactly one writer: no atomics, no
 * LDS, no dependency between workgroups.  A segment that would pass its destination (dst_rows) is not copied -- plan and row pointers
 * come from the same host sizes, so this never happens with a loader's own tables.  All offsets are int64.
 * batch == 0, or no field with rows and no pointer output: nothing is launched, GSN_OK.  More than GSN_LOADER_MAX_FIELDS fields, element
 * bytes other than 4 / 8, a null pointer where rows are expected, or positions outside [0, n_graphs_total]: GSN_E_INVALID.  Asynchronous
 * on `stream`, allocates nothing, can be captured into a HIP graph.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GSN_LOADER_MAX_FIELDS 16
enum { GSN_LOADER_COPY = 0, GSN_LOADER_EDGE_INDEX = 1 };
#define GSN_LOADER_F_NODES 1
typedef struct gsn_loader_field {
    const void *src;
    const int64_t *row_ptr;
    void *dst;
    int64_t dst_rows;
    int64_t row_bytes;
    int64_t src_stride, dst_stride;
    int32_t elem_bytes;
    int32_t ptr_class;
    int32_t kind;
    int32_t inc_class;
    int32_t flags;
    int32_t reserved;
} gsn_loader_field;
int gsn_loader_collate_hip(int n_fields, const gsn_loader_field *fields, const int64_t *order, const int64_t *plan,
                           int64_t n_graphs_total, int64_t first, int64_t batch, int64_t *batch_vec, int64_t *node_ptr_out,
                           int64_t *edge_ptr_out, void *stream);

/* The same batch collated into caller-owned STATIC buffers of fixed capacity, in ONE launch (gsn_amd/loader.py: PaddedDataLoader): shapes
 * and pointers do not change from batch to batch, so what consumes the batch can be captured into a HIP graph once and replayed.
 *   pad      by value: n_real = b real graphs (1 <= b < graph_slots) with n_real_nodes = N_r vertices and n_real_edges = E_r edge columns;
 *            capacities node_capacity = N_cap, edge_capacity = E_cap, graph_slots = G_cap; n_chunk >= 2 and e_chunk >= 1, the most
 *            vertices / edge columns a pad graph may have.
 *   fields   as above, with dst_rows the field's CAPACITY: N_cap for a per-vertex field, E_cap with GSN_LOADER_F_PAD_EDGES (and for
 *            edge_index, whose dst_stride is >= E_cap), G_cap with GSN_LOADER_F_PAD_GRAPH (one row per graph).
 *   fill     host array of one 8-byte word per field, by value in the launch: every element of a pad row of the field is that word (its low
 *            4 bytes for 4-byte elements).  Ignored for edge_index.
 * Slots [0, b) are the real graphs, laid out exactly as gsn_loader_collate_hip lays them out.  The S = G_cap - b slots behind them are PAD
 * GRAPHS.  With r_n = N_cap - N_r - S and r_e = E_cap - E_r, pad graph k has 1 + min(n_chunk - 1, max(0, r_n - k (n_chunk - 1))) vertices
 * and min(e_chunk, max(0, r_e - k e_chunk)) edge columns: every slot has a vertex, and the totals are exactly N_cap and E_cap.  Column t of
 * a pad graph with v vertices is the self loop of its vertex t mod v.  batch_vec [N_cap], node_ptr_out / edge_ptr_out [G_cap + 1] and
 * n_valid [1] (= b) are written as well; batch_vec, edge_ptr_out and n_valid may be NULL.
 * One wave per (field, slot) pair over all G_cap slots; EVERY byte of every output is written by every launch, by exactly one writer (the
 * buffers are reused: nothing of the previous batch survives).  No atomics, no LDS, int64 offsets.
 * GSN_E_INVALID when the batch does not fit -- N_r + S > N_cap, E_r > E_cap, or spare rows the S pad graphs cannot hold -- or a field's
 * dst_rows is not its capacity, besides what gsn_loader_collate_hip refuses.  Asynchronous on `stream`, allocates nothing.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GSN_LOADER_F_PAD_EDGES 2
#define GSN_LOADER_F_PAD_GRAPH 4
typedef struct gsn_loader_pad {
    int64_t n_real, graph_slots;
    int64_t n_real_nodes, n_real_edges;
    int64_t node_capacity, edge_capacity;
    int64_t n_chunk, e_chunk;
} gsn_loader_pad;
int gsn_loader_collate_padded_hip(int n_fields, const gsn_loader_field *fields, const uint64_t *fill, const int64_t *order, const int64_t *plan,
                                  int64_t n_graphs_total, int64_t first, const gsn_loader_pad *pad, int64_t *batch_vec,
                                  int64_t *node_ptr_out, int64_t *edge_ptr_out, int64_t *n_valid, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Dropout with the residual add in ONE launch, and its adjoint, without a mask tensor (models_graph_classification_ogb_original.py:243-245:
 * x = F.dropout(x, p, training) followed by x += x_interm[-1] at :247-248; :257-259: the virtual node's vn + F.dropout(act(vn));
 * models_graph_classification.py:240: prediction += F.dropout(lin_proj(x_global)); directional_gsn/nets/dgn_layer.py:81: h = F.dropout(h);
 * dgn_net.py:58: in_feat_dropout).
 * The mask is drawn from Philox4x32-10 (multipliers D2511F53, CD9E8D57; Weyl constants 9E3779B9, BB67AE85).  For element e of the tensor
 * -- counted from its first element, never from an address -- of a call with state (seed, calls), both 64 bits:
 *   group q = e >> 2; counter = (lo32 q, hi32 q, lo32 calls, hi32 calls); key = (lo32 seed, hi32 seed); r = output word e & 3;
 *   KEEP iff r >= thr, with thr = min(2^32 - 1, round(p 2^32)) and scale = float32(1 / (1 - p)) from the caller.
 * Forward:  v = keep ? x * scale : +0 (a select: a NaN or Inf in a dropped element does not propagate); out = v, or res + v when res is
 *           not NULL -- product and sum rounded separately, never one fused multiply-add: bit for bit res + mask * x * scale in fp32.
 * Backward: grad_x = keep ? grad_out * scale : +0 from the (seed, calls) the forward left in `used`.  The residual's gradient is grad_out.
 *   n         elements of x, res, out (grad_out, grad_x); fp32, contiguous, 4-byte aligned.  When every tensor of the call is 16-byte aligned
 *             the groups move as 16 bytes, else as four words of the SAME group: the mask does not depend on alignment, grid or shape.
 *   state     int64 device [2]: seed, calls.  Read by every workgroup in front of its elements; the workgroup that finishes last writes
 *             calls + 1 -- no second launch, no host-side counter: a replayed HIP graph draws what an eager call at that state would draw.
 *   done      uint32 device, zero before the first call; the launch leaves it zero.  One state = one word; calls that share it must be
 *             ordered (one stream, or one graph).
 *   used      int64 device [2], written by the forward: the (seed, calls) of this call.  The backward reads it and never touches `state`.
 * A workgroup takes GSN_DROPOUT_CHUNK_ELEMS consecutive elements, a lane one Philox call per group of four; more than (2^31 - 1) chunks:
 * GSN_E_UNSUPPORTED.  n == 0 launches nothing, leaves the state as it is and returns GSN_OK.  Asynchronous on `stream`, allocates nothing,
 * can be captured into a HIP graph.  gsn_dropout_chunk_elems() returns GSN_DROPOUT_CHUNK_ELEMS of the built library.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GSN_DROPOUT_CHUNK_ELEMS 8192
int gsn_dropout_fwd_hip(int64_t n, const float *x, const float *res /* may be NULL */, float *out, uint32_t thr, float scale,
                        int64_t *state /* [2]: seed, calls */, unsigned *done, int64_t *used /* [2], written */, void *stream);
int gsn_dropout_bwd_hip(int64_t n, const float *grad_out, float *grad_x, uint32_t thr, float scale, const int64_t *used, void *stream);
int64_t gsn_dropout_chunk_elems(void);

#ifdef __cplusplus
}
#endif
#endif /* GSN_ABI_H */
