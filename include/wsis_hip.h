/*
 * wsis_hip.h -- C ABI of the MI355X (gfx950) hot path of 3D-WSIS.
 *
 * This is the drop-in boundary.  Two shared libraries export it:
 *
 *   libwsis_host.so  (g++ only, never touches the HIP runtime -- safe in forked DataLoader workers)
 *       wsis_host_*   : voxelization_idx, bfs_cluster, reference-order helpers
 *   libwsis_hip.so   (hipcc --offload-arch=gfx950)
 *       wsis_*        : every device operator
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory, h_* is HOST memory; the caller (PyTorch) allocates
 *     every input, output and workspace buffer and passes raw pointers + sizes.  The library never
 *     allocates device memory that outlives a call and never frees caller memory.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *   - every function returns int: 0 = ok, <0 = error; wsis_last_error()/wsis_host_last_error()
 *     return a thread-local message.  No C++ exception crosses the ABI.
 *   - variable-size outputs use count-then-fill or documented upper bounds with the true count
 *     written to a device int32 the caller reads back.
 *   - feature rows are row-major fp32 [rows, C]; indices are int32 [M,4] = (batch, c0, c1, c2).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * fpthink/3D-WSIS tree).  [UPSTREAM] marks semantics of an un-vendored dependency (spconv v1.0
 * llijiang fork, PointGroup lib/pointgroup_ops, torch_scatter 2.0.x) restated in SURVEY.md App. A.
 */
#ifndef WSIS_HIP_H_
#define WSIS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSIS_ABI_VERSION 3

/* error codes */
#define WSIS_OK 0
#define WSIS_ERR_ARG (-1)      /* bad argument (null pointer, bad size, unsupported shape) */
#define WSIS_ERR_HIP (-2)      /* a HIP runtime call failed (message has hipGetErrorString) */
#define WSIS_ERR_OVERFLOW (-3) /* a caller-provided capacity was too small */

/* ------------------------------------------------------------------------------------------ */
/* libwsis_host.so : host-only operators                                                      */
/* ------------------------------------------------------------------------------------------ */

int wsis_host_version(void);
const char* wsis_host_last_error(void);

/* pointgroup_ops.voxelization_idx(coords, batchsize, mode)  [UPSTREAM PG_OP.voxelize_idx]
 * call sites: modules/datasets/scannetv2_dataset.py:449,528  test_scannetv2.py:389
 * Pass 1: scan points in order, voxel id = order of first occurrence of the (b,x,y,z) row.
 *   h_coords int64 [N,4]; writes h_p2v int32 [N]; *M = #voxels; *max_active = longest point list. */
int wsis_host_voxelize_idx_map(const int64_t* h_coords, int64_t N, int32_t* h_p2v, int64_t* M,
                               int32_t* max_active);
/* Pass 2: h_voxel_locs int64 [M,4] = coords of each voxel's first point;
 *   h_v2p int32 [M, 1+max_active] = [count, p0, p1, ... ascending, 0 padded]. */
int wsis_host_voxelize_idx_fill(const int64_t* h_coords, int64_t N, const int32_t* h_p2v, int64_t M,
                                int32_t max_active, int64_t* h_voxel_locs, int32_t* h_v2p);

/* pointgroup_ops.bfs_cluster(semantic_label, ball_query_idxs, start_len, threshold)
 * [UPSTREAM PG_OP.bfs_cluster; no call site in the reference, named by BASELINE.json north_star]
 * Pass 1: FIFO BFS, seeds ascending, neighbour accepted iff same label & unvisited.  Writes
 *   h_point_cluster int32 [N] = kept-cluster id or -1 and h_order int32 [N] = discovery rank of the
 *   point inside its cluster; *n_clusters, *n_points = totals over kept clusters (size >= threshold). */
int wsis_host_bfs_cluster_count(const int32_t* h_semantic, const int32_t* h_ball_idx,
                                const int32_t* h_start_len, int64_t N, int32_t threshold,
                                int32_t* h_point_cluster, int32_t* h_order, int64_t* n_clusters,
                                int64_t* n_points);
/* Pass 2: h_cluster_idxs int32 [n_points,2] = (cluster id, point idx) in discovery order,
 *   h_cluster_offsets int32 [n_clusters+1]. */
int wsis_host_bfs_cluster_fill(const int32_t* h_point_cluster, const int32_t* h_order, int64_t N,
                               int64_t n_clusters, int64_t n_points, int32_t* h_cluster_idxs,
                               int32_t* h_cluster_offsets);

/* Superpoint-graph BFS of the test-time grouping, test_scannetv2.py:312-340 (`BFS`) driven by the seed loop of
 * :372-381.  Seeds ascending over superpoints whose class is valid and that are unvisited; a
 * neighbour joins iff same class as the seed, unvisited, and ||centre[cur] - centre[nb]||_2 < 0.25*ins_size[seed]
 * (fp32).  h_adj_off int32 [S+1], h_adj int32 [nnz] = igraph `neighbors(mode='all')` lists; h_class_valid
 * uint8 [n_class].  h_group int32 [S] = group id in seed order or -1. */
int wsis_host_graph_bfs(const int32_t* h_label, const uint8_t* h_class_valid, int32_t n_class,
                        const float* h_centre, const float* h_ins_size, const int32_t* h_adj_off,
                        const int32_t* h_adj, int64_t S, int32_t* h_group, int64_t* n_groups);

/* The serial half of segmentator.segment_mesh [UPSTREAM ScanNet Segmentator], prepare_data_inst_ScanNetV2.py:77 (DESIGN.md
 * 4.17 steps 6-8; steps 1-5 are wsis_mesh_* below and a stable sort).  h_a / h_b int32 [E], h_w fp32 [E]: the edges
 * sorted ascending by (w, edge index); an unsorted h_w or an endpoint outside [0, V) is WSIS_ERR_ARG.  Sweep 1: every
 * vertex a component of size 1 and thr = kThresh; an edge whose roots differ and whose w <= thr of both joins them, and
 * the new root gets thr = w + kThresh / (float)size (fp32).  Sweep 2, same order: roots that differ join if either has
 * fewer than segMinVerts vertices.  h_out_ids int64 [V]: dense ids numbered by each segment's smallest vertex;
 * *n_segments their number.  E = 0 or V = 0 is legal. */
int wsis_host_mesh_merge(const int32_t* h_a, const int32_t* h_b, const float* h_w, int64_t E, int64_t V, float kThresh,
                         int32_t segMinVerts, int64_t* h_out_ids, int64_t* n_segments);

/* ------------------------------------------------------------------------------------------ */
/* libwsis_hip.so : device operators                                                          */
/* ------------------------------------------------------------------------------------------ */

int wsis_version(void);
const char* wsis_last_error(void);
/* number of visible HIP devices (0 when none) -- does not create a context */
int wsis_device_count(void);

/* ---- a2: pointgroup_ops.voxelization(feats, map_rule, mode)  train_scannetv2.py:189 ---------
 * out[m,:] = sum_{i<n_m} w * feats[v2p[m,1+i],:], w = 1/n_m for mode 4 else 1, accumulated in
 * list order in fp32.  d_v2p int32 [M, stride] with stride = 1+max_active. */
int wsis_voxelize_fwd(const float* d_feats, const int32_t* d_v2p, float* d_out, int64_t M, int32_t C,
                      int32_t stride, int32_t mode, void* stream);
/* d_dfeats [N,C] must be zero-initialised by the caller; dfeats[p,:] = w * dout[m,:]. */
int wsis_voxelize_bwd(const float* d_dout, const int32_t* d_v2p, float* d_dfeats, int64_t M, int32_t C,
                      int32_t stride, int32_t mode, void* stream);

/* ---- GPU voxelization_idx (a1 off the CPU workers) ------------------------------------------------
 * Same contract as wsis_host_voxelize_idx_* (first-occurrence voxel ids, ascending point lists), bit-exact.
 * d_coords int64 [N,4] device.  Pass 1 writes d_p2v int32 [N] and d_counts2 int32[2] = {M, max_active}; the caller
 * reads them back, allocates voxel_locs int64 [M,4] and v2p int32 [M,1+max_active], and calls pass 2 with the SAME
 * workspace (it holds the points sorted by voxel id). */
int64_t wsis_voxelize_idx_workspace_bytes(int64_t N);
int wsis_voxelize_idx_map(const int64_t* d_coords, int64_t N, int32_t* d_p2v, int32_t* d_counts2, void* d_ws,
                          int64_t ws_bytes, void* stream);
int wsis_voxelize_idx_fill(const int64_t* d_coords, int64_t N, int64_t M, int32_t max_active,
                           int64_t* d_voxel_locs, int32_t* d_v2p, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- a5/a6: rulebooks [UPSTREAM spconv getIndicePair]  sparse_unet3d.py:130,261,292 ---------
 * Native rulebook format = gather table nbr int32 [K, M_rows]: nbr[k][r] = row of the OTHER side
 * paired with row r under flat kernel offset k (row-major over the 3 kernel dims), or -1.
 * Hash table: open addressing, d_keys int64 [cap] (cap power of two >= 2*M), d_vals int32 [cap];
 * key = linear index ((b*S0+c0)*S1+c1)*S2+c2. */
int wsis_hash_build(const int32_t* d_indices, int64_t M, const int32_t* h_shape3, int64_t* d_keys,
                    int32_t* d_vals, int64_t cap, void* stream);
/* SubMConv3d: out rows == in rows.  nbr[k][o] = i with coord[i] = coord[o] - pad + kappa.
 * d_mask uint32 [M] (optional, may be null, needs K<=32): bit k set iff nbr[k][o] >= 0. */
int wsis_rulebook_subm(const int32_t* d_indices, int64_t M, const int32_t* h_shape3,
                       const int32_t* h_ksize3, const int32_t* h_pad3, const int64_t* d_keys,
                       const int32_t* d_vals, int64_t cap, int32_t* d_nbr, uint32_t* d_mask,
                       void* stream);
/* SparseConv3d (stride s, pad p, dilation 1): out_shape_j = floor((in_j + 2p_j - (k_j-1) - 1)/s_j)+1.
 * Step 1: candidate keys + sort + unique -> d_out_keys int64 [<= n_cand] ascending linear index,
 * count in d_count int32[1].  n_cand = M_in when k==s && p==0, else M_in*K. */
int64_t wsis_rulebook_down_ncand(int64_t M_in, const int32_t* h_ksize3, const int32_t* h_stride3,
                                 const int32_t* h_pad3);
int64_t wsis_rulebook_down_workspace_bytes(int64_t n_cand);
int wsis_rulebook_down_keys(const int32_t* d_indices_in, int64_t M_in, const int32_t* h_in_shape3,
                            const int32_t* h_out_shape3, const int32_t* h_ksize3,
                            const int32_t* h_stride3, const int32_t* h_pad3, int64_t* d_cand,
                            int64_t* d_out_keys, int32_t* d_count, void* d_ws, int64_t ws_bytes,
                            void* stream);
/* Step 2 (after the caller read M_out): decode out indices [M_out,4], build the coarse hash table,
 * fill nbr_down int32 [K, M_out] (coarse row -> fine row) and nbr_up int32 [K, M_in]
 * (fine row -> coarse row); optional masks as in wsis_rulebook_subm. */
int wsis_rulebook_down_fill(const int32_t* d_indices_in, int64_t M_in, const int32_t* h_in_shape3,
                            const int32_t* h_out_shape3, const int32_t* h_ksize3,
                            const int32_t* h_stride3, const int32_t* h_pad3,
                            const int64_t* d_out_keys, int64_t M_out, int32_t* d_indices_out,
                            int64_t* d_keys, int32_t* d_vals, int64_t cap, int32_t* d_nbr_down,
                            int32_t* d_nbr_up, uint32_t* d_mask_down, uint32_t* d_mask_up,
                            void* stream);
/* Tile ordering for the implicit GEMM: d_order int32 [M] = stable argsort of d_mask (rows with the
 * same set of active offsets become neighbours so whole tiles skip inactive offsets). */
int64_t wsis_mask_order_workspace_bytes(int64_t M);
/* Spatial + mask tile ordering: stable sort by (batch, Morton code of the row's block of 2^block_shift voxels
 * per side, offset mask), then the full 32-row slices heaviest first.  Rows of one block become neighbours, so the
 * gathers of a tile hit the same L1/L2 lines; inside a block equal offset sets stay adjacent.  d_mask may be NULL
 * (pure spatial order).  This is the one-table call of the implementation behind wsis_tile_order_batch: the key
 * has no table number and keeps 8 bits of the batch index (batches of up to 256 scenes). */
int64_t wsis_tile_order_workspace_bytes(int64_t M);
int wsis_tile_order(const int32_t* d_indices, const uint32_t* d_mask, int64_t M, int32_t block_shift,
                    int32_t* d_order, void* d_ws, int64_t ws_bytes, void* stream);
int wsis_mask_order(const uint32_t* d_mask, int64_t M, int32_t* d_order, void* d_ws, int64_t ws_bytes,
                    void* stream);
/* The tile orders of up to 16 gather tables (every table of a UNet pyramid) from ONE sort: h_indices[t] /
 * h_mask[t] are host arrays of device pointers (int32 [M_t,4] / uint32 [M_t] or NULL), h_M the row counts.
 * d_order_all int32 [sum M_t]: table t's order (row numbers local to the table, what wsis_tile_order returns
 * for it) at offset sum_{u<t} M_u.  The key carries the table number in its top 4 bits and 4 bits of the batch
 * index below them: the batch index of every row must be < 16 (batch_size, checked on the host side).
 * N = sum M_t for the workspace query; the two workspace queries are one function of the row total. */
int64_t wsis_tile_order_batch_workspace_bytes(int64_t N);
int wsis_tile_order_batch(int32_t n, const void* const* h_indices, const void* const* h_mask, const int64_t* h_M,
                          int32_t block_shift, int32_t batch_size, int32_t* d_order_all, void* d_ws,
                          int64_t ws_bytes, void* stream);

/* Packed gather table for the convolution kernels: nbr_packed[k][t] = nbr[k][order[t]] (columns in tile
 * order, so a 128-row tile reads K coalesced 512-byte pieces).  With d_order == NULL the kernels take the
 * unpacked table as is. */
int wsis_rulebook_pack(const int32_t* d_nbr, const int32_t* d_order, int32_t* d_nbr_packed, int64_t M,
                       int32_t K, void* stream);
/* the same for up to 16 tables in one launch: host arrays of device pointers / sizes, one entry per table
 * (wsis_rulebook_pack is this launch with one table) */
int wsis_rulebook_pack_batch(int32_t n, const void* const* h_nbr, const void* const* h_order,
                             void* const* h_nbr_packed, const int64_t* h_M, const int32_t* h_K, void* stream);

/* The whole rulebook pyramid of a UBlock from ONE call (SubM k3 p1 table per level, SparseConv3d k2 s2 tables between
 * levels: sparse_unet3d.py:130,261,292) when every level's row count is known on the host (h_counts[l-1] = rows of
 * level l, e.g. from the loader's host-side coordinates): no device read-back, one arena, the same entry points in the
 * same order as the per-table build (identical tables).  wsis_rulebook_pyramid_layout returns the arena size and
 * fills h_layout [n_levels][WSIS_PYR_FIELDS] with byte offsets into the arena (-1: not present; ROWS / CAP are values):
 * the packed tables + tile orders the convolutions take, the unpacked tables, masks, coordinate hashes, the coarse
 * levels' indices, and the device's own output count per strided level (int32 at COUNT: compare with h_counts). */
enum {
  WSIS_PYR_ROWS = 0, WSIS_PYR_CAP, WSIS_PYR_INDICES, WSIS_PYR_KEYS, WSIS_PYR_VALS, WSIS_PYR_SUBM_NBR, WSIS_PYR_SUBM_MASK,
  WSIS_PYR_SUBM_ORDER, WSIS_PYR_SUBM_NBR_P, WSIS_PYR_CAND, WSIS_PYR_OUT_KEYS, WSIS_PYR_COUNT, WSIS_PYR_DOWN_WS,
  WSIS_PYR_DOWN_NBR, WSIS_PYR_UP_NBR, WSIS_PYR_DOWN_MASK, WSIS_PYR_UP_MASK, WSIS_PYR_DOWN_ORDER, WSIS_PYR_UP_ORDER,
  WSIS_PYR_DOWN_NBR_P, WSIS_PYR_UP_NBR_P, WSIS_PYR_FIELDS
};
int64_t wsis_rulebook_pyramid_layout(int64_t M0, const int64_t* h_counts, int32_t n_levels, int64_t* h_layout);
int wsis_rulebook_pyramid(const int32_t* d_indices0, int64_t M0, const int32_t* h_shape3, const int64_t* h_counts,
                          int32_t n_levels, int32_t batch_size, int32_t block_shift, void* d_arena, int64_t arena_bytes,
                          void* stream);
/* Which form the output coordinates of a strided level take inside wsis_rulebook_pyramid (a query: nothing is issued):
 * 1 = bitmap over the output grid + prefix popcount (k == s, p == 0, batch_size >= 1, 1 <= batch_size * out cells
 * <= 2^31, and the bitmap with its chunk sums fits wsis_rulebook_down_workspace_bytes of the level's candidates),
 * 0 = candidate keys + sort + unique, -1 = bad arguments.  The build itself decides by the same function; both forms
 * give the same rows (ascending linear index; batch indices outside [0, batch_size) are not part of the build). */
int32_t wsis_rulebook_down_form(int64_t M_in, const int32_t* h_out_shape3, const int32_t* h_ksize3,
                                const int32_t* h_stride3, const int32_t* h_pad3, int32_t batch_size);

/* ---- a7-a11: sparse convolution [UPSTREAM spconv indiceConv / indiceConvBackward] -----------
 * out[r,:] = sum_k X[nbr[k][r],:] @ W[k]  (rows with nbr<0 contribute nothing), fp32.
 *   SubMConv3d fwd      : X=in,   nbr=subm table,  W=weight [K,Cin,Cout]
 *   SubMConv3d dIn      : X=dOut, nbr=subm table,  W=wsis_weight_transpose(weight, flip=1)
 *   SparseConv3d fwd    : X=in,   nbr=nbr_down,    W=weight
 *   SparseConv3d dIn    : X=dOut, nbr=nbr_up,      W=transpose(weight, flip=0)
 *   SparseInverseConv3d : X=in,   nbr=nbr_up,      W=weight ; dIn: X=dOut, nbr=nbr_down, W^T
 * d_nbr is the PACKED table when d_order (int32 [M_out], tile ordering from wsis_mask_order) is given,
 * the plain table when d_order is NULL; d_bias optional [Cout];
 * d_residual optional [M_out,Cout] added in the epilogue (sparse_unet3d.py:170 fused).
 * K==1 with d_nbr==null is the dense 1x1 shortcut (sparse_unet3d.py:115-119). */
/* Small levels split the K offsets over blockIdx.z and reduce partial slabs from d_ws in a fixed order
 * (size from the query; 256 bytes when no split is used). */
int64_t wsis_spconv_fwd_workspace_bytes(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout);
int wsis_spconv_fwd(const float* d_X, const int32_t* d_nbr, const int32_t* d_order, const float* d_W,
                    const float* d_bias, const float* d_residual, float* d_out, int64_t M_in,
                    int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, void* d_ws, int64_t ws_bytes,
                    void* stream);
/* The same product with the weights given as B^T, d_WT [K,Cout,Cin] (row = output channel, Cin contiguous) -- the
 * wave-autonomous LDS-DMA kernel (csrc/spconv2.hip) that every UNet layer with channel counts that are multiples of 32
 * runs on (wsis_spconv_fwd_t_supported; K <= 32).  Replaces the same upstream call sites as wsis_spconv_fwd:
 *   forward (sparse_unet3d.py:130,261,292) : d_WT = wsis_weight_transpose(weight, flip=0), flip = 0
 *   dIn (autograd backward)    : d_WT = the layer's own weight [K,Cin_fwd,Cout_fwd] (its rows ARE the dIn
 *                                            output channels), flip = 1 for submanifold tables (offset k uses
 *                                            slice K-1-k), 0 for the coupled strided / inverse tables
 * with NW = 1 bit-identical to wsis_spconv_fwd; small levels split the offsets over the waves of a workgroup (added
 * through LDS in wave order) and, below that, over blockIdx.z into partial slabs in d_ws (fixed order).  d_sync: a
 * sync slot (wsis_sync_bytes; may be NULL; reserved for in-launch reductions: wsis_spconv_fwd_f). */
int32_t wsis_spconv_fwd_t_supported(int32_t K, int32_t Cin, int32_t Cout);
/* number of offset slabs the launch plan of wsis_spconv_fwd_t uses for this shape (1 = one kernel, no second pass) */
int32_t wsis_spconv_fwd_t_slabs(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout);
int64_t wsis_spconv_fwd_t_workspace_bytes(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout);
/* d_stats (optional): BatchNorm partials of the finished output, [ceil(M_out / 32)][2][Cout] floats per 32-row slice
 * in tile order: (sum, sum of squared deviations from the SLICE's own mean), fixed order of additions -- the
 * statistics pass of the BatchNorm that consumes this tensor (sparse_unet3d.py:128-137) fused into the producer's
 * epilogue; combined in fp64 (Chan) by wsis_bn_stats_finalize, so nothing cancels in fp32. */
int wsis_spconv_fwd_t(const float* d_X, const int32_t* d_nbr, const int32_t* d_order, const float* d_WT, int32_t flip,
                      const float* d_bias, const float* d_residual, float* d_out, float* d_stats, int64_t M_in,
                      int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, void* d_ws, int64_t ws_bytes,
                      void* d_sync, void* stream);
/* the same product for a dIn pass whose output dy [M_out, Cout] feeds the backward of a BatchNorm(+ReLU) with input
 * d_bn_x [M_out, Cout] (reference: spconv's dIn followed by torch's batch_norm backward, sparse_unet3d.py:128-137):
 * besides d_out the epilogue writes, per 32-row slice, (sum dz, sum dz * xhat) with xhat = (x - mean) rsqrt(var + eps)
 * and dz = dy masked where relu && xhat * gamma + beta <= 0, into d_partials [ceil(M_out / 32)][2][Cout] -- the
 * reduction wsis_bn_bwd would otherwise make in a pass of its own (wsis_bn_bwd_from_partials consumes them). */
int wsis_spconv_fwd_t_bn(const float* d_X, const int32_t* d_nbr, const int32_t* d_order, const float* d_WT, int32_t flip,
                         float* d_out, float* d_partials, const float* d_bn_x, const float* d_bn_mean,
                         const float* d_bn_var, const float* d_bn_gamma, const float* d_bn_beta, float eps, int32_t relu,
                         int64_t M_in, int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, void* d_ws, int64_t ws_bytes,
                         void* d_sync, void* stream);
/* ---- EXPERIMENTAL build only (make -C 3d-wsis_amd/csrc EXPERIMENTAL=1; wsis_experimental() says which build a library
 * is): the retired designs of DESIGN.md section 8 -- measured slower than the default path, kept buildable and tested.
 * The default library does not export the entry points inside these guards. */
/* The fused form of wsis_spconv_fwd_t for one layer of `BatchNorm1d -> ReLU -> conv` chains (sparse_unet3d.py:127-143):
 *   bn_in   (optional) BatchNorm(+ReLU) of the INPUT applied while the gathered rows are read: the activation
 *           relu(bn(x)) is never written; mean / var are the batch statistics (training) or the running statistics;
 *   targets (optional, needs d_stats and a sync slot) the statistics of the OUTPUT are FINISHED inside the launch: the
 *           last workgroups to arrive add the slice partials (the order of wsis_bn_stats_finalize, bit-identical) and
 *           write mean / var and update the running statistics of up to two BatchNorm layers that normalise this tensor
 *           (the UNet's skip connection feeds a second one).
 * One launch whatever the level: up to 16 waves of a workgroup split a work item's offsets, no slabs, no second kernel.
 * With both NULL it is wsis_spconv_fwd_t without slabs.  Workspace: wsis_spconv_fwd_f_workspace_bytes. */
typedef struct wsis_bn_in {
  const float* mean;
  const float* var;
  const float* gamma; /* may be NULL (1) */
  const float* beta;  /* may be NULL (0) */
  float eps;
  int32_t relu;
} wsis_bn_in;
typedef struct wsis_stat_target {
  float* mean;
  float* var;
  float* running_mean; /* may be NULL (with running_var) */
  float* running_var;
  float momentum;
  int32_t reserved;
} wsis_stat_target;
#if defined(WSIS_EXPERIMENTAL) && WSIS_EXPERIMENTAL
int64_t wsis_spconv_fwd_f_workspace_bytes(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout);
int wsis_spconv_fwd_f(const float* d_X, const wsis_bn_in* bn_in, const int32_t* d_nbr, const int32_t* d_order,
                      const float* d_WT, int32_t flip, const float* d_bias, const float* d_residual, float* d_out,
                      float* d_stats, const wsis_stat_target* targets, int32_t n_targets, int64_t M_in, int64_t M_out,
                      int32_t K, int32_t Cin, int32_t Cout, void* d_ws, int64_t ws_bytes, void* d_sync, void* stream);
#endif /* WSIS_EXPERIMENTAL */
/* WT[k'] = W[k]^T with k' = (flip ? K-1-k : k); W [K,Cin,Cout] -> WT [K,Cout,Cin]. */
int wsis_weight_transpose(const float* d_W, float* d_WT, int32_t K, int32_t Cin, int32_t Cout,
                          int32_t flip, void* stream);
/* dW[k] = sum_r X[nbr[k][r],:]^T (x) dY[r,:]   -> d_dW [K,Cin,Cout] (overwritten); d_nbr/d_order as above.
 * Deterministic: per-workgroup partial slabs in d_ws reduced in a fixed order. */
int64_t wsis_spconv_dw_workspace_bytes(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout);
int wsis_spconv_dw(const float* d_X, const int32_t* d_nbr, const int32_t* d_order, const float* d_dY,
                   float* d_dW, int64_t M_in, int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, void* d_ws,
                   int64_t ws_bytes, void* stream);

/* ---- 16-bit sparse convolution (bf16 / fp16 operands, fp32 accumulation): csrc/spconv_lp.hip --------------------
 * The same products as wsis_spconv_fwd_t / wsis_spconv_dw for features and weights in 16 bits -- what upstream spconv
 * runs for half features under mixed precision [UPSTREAM spconv indiceConv / indiceConvBackward with fp16 tensors].
 * dtype: 0 = bf16, 1 = fp16; every 16-bit buffer holds that type.  Domain: Cin and Cout multiples of 32, at most 512,
 * any K, gathered tensors below 2 GiB (32-bit gather offsets); outside it the caller widens to fp32. */
int32_t wsis_spconv_lp_supported(int32_t K, int32_t Cin, int32_t Cout);
/* The launch plan the two products below run for this shape (host-only, reads nothing on the device; the launches
 * compute it with the same helper).  M_out = output rows of wsis_spconv_fwd_lp, or dY rows of wsis_spconv_dw_lp.
 * out[8]: forward / dIn  [0] NT (32-column output tiles per wave: 2 when Cout / 32 is even and
 *                            ceil(M_out / 32) * Cout / 64 >= 4096, else 1), [1] ncg = Cout / (32 NT) channel groups,
 *                            [2] forward blocks;
 *         weight gradient [3] row chunks (partial slabs; 1 = written straight into dW), [4] rows per chunk (a
 *                            multiple of 32), [5] waves per workgroup, [6] tile groups, [7] LDS bytes.
 * Returns 0, or nonzero for M_out outside [1, 2^31), a shape outside wsis_spconv_lp_supported or a NULL out. */
int32_t wsis_spconv_lp_plan(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, int32_t* out);
/* out[r] = sum_k X[nbr[k][r]] @ W[k] with 16-bit X [M_in, Cin] and B^T weights d_WT [K, Cout, Cin] (slice K-1-k when
 * flip: the conventions of wsis_spconv_fwd_t, which it replaces at the same call sites for 16-bit features:
 * sparse_unet3d.py:130,261,292 forward, SURVEY a11 dIn with d_WT = the plain 16-bit cast of the weight).  d_nbr / d_order
 * as for wsis_spconv_fwd; K == 1 with d_nbr == NULL is the dense 1x1 shortcut; d_bias optional fp32 [Cout].  fp32
 * accumulators, each output element rounded to 16 bits once; the order of additions of an output row depends on the
 * offset index only (bit-reproducible).  No offset split: the workspace query returns a minimal size. */
int64_t wsis_spconv_fwd_lp_workspace_bytes(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout);
int wsis_spconv_fwd_lp(const void* d_X, const int32_t* d_nbr, const int32_t* d_order, const void* d_WT, int32_t flip,
                       const float* d_bias, void* d_out, int64_t M_in, int64_t M_out, int32_t K, int32_t Cin,
                       int32_t Cout, int32_t dtype, void* d_ws, int64_t ws_bytes, void* stream);
/* The same with an optional 16-bit residual [M_out, Cout] (d_residual; NULL: exactly wsis_spconv_fwd_lp): each output
 * element is acc + bias + residual in fp32, rounded to 16 bits ONCE -- the skip connection of the residual block
 * (sparse_unet3d.py:163-172, the in[5] residual of the executor's fp32 CONV op).  d_residual must not alias d_out. */
int wsis_spconv_fwd_lp_res(const void* d_X, const int32_t* d_nbr, const int32_t* d_order, const void* d_WT,
                           int32_t flip, const float* d_bias, const void* d_residual, void* d_out, int64_t M_in,
                           int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* d_ws,
                           int64_t ws_bytes, void* stream);
/* dW[k] = sum_r X[nbr[k][r]]^T (x) dY[r] with 16-bit X [M_in, Cin] and dY [M_out, Cout] -> fp32 d_dW [K, Cin, Cout]
 * (overwritten): the 16-bit form of wsis_spconv_dw [UPSTREAM spconv indiceConvBackward, filter gradient].  Partial slabs
 * per row chunk in d_ws, added in chunk order: no atomics, bit-reproducible. */
int64_t wsis_spconv_dw_lp_workspace_bytes(int64_t M_out, int32_t K, int32_t Cin, int32_t Cout);
int wsis_spconv_dw_lp(const void* d_X, const int32_t* d_nbr, const int32_t* d_order, const void* d_dY, float* d_dW,
                      int64_t M_in, int64_t M_out, int32_t K, int32_t Cin, int32_t Cout, int32_t dtype, void* d_ws,
                      int64_t ws_bytes, void* stream);
/* fp32 W [K, Cin, Cout] -> 16-bit d_out, rounded to nearest even (NaN stays NaN): [K, Cout, Cin] = W[k]^T when transpose
 * (the d_WT of the forward pass), [K, Cin, Cout] otherwise (the dIn operand); slice k goes to K-1-k when flip.  The
 * 16-bit counterpart of wsis_weight_transpose. */
int wsis_weight_cast_lp(const float* d_W, void* d_out, int32_t K, int32_t Cin, int32_t Cout, int32_t transpose,
                        int32_t flip, int32_t dtype, void* stream);

/* The same weight gradient for a convolution whose INPUT is BatchNorm(+ReLU)(d_X) applied on the fly (the activation
 * relu(bn(x)) of sparse_unet3d.py:128-137 is never materialised: the forward pass normalises the gathered rows as it
 * reads them, wsis_spconv_fwd_f): dW[k] = sum_pairs relu(bn(X[i]))^T (x) dY[o].  "Own rows" form: the slices run over
 * the convolution's INPUT rows, which are normalised once per slice (d_mean / d_var [Cin], optional d_gamma / d_beta;
 * d_mean == NULL: X as it stands), and the paired dY rows are gathered through the dIn table d_nbr_b / d_order_b
 * (packed, rows = inputs; flip = 1 for submanifold tables, whose dIn offset k pairs with forward offset K - 1 - k).
 * Cin % 32 == 0, Cout % 32 == 0, K <= 32.  Fixed summation order, no atomics. */
int32_t wsis_spconv_dw_bn_supported(int32_t K, int32_t Cin, int32_t Cout);
int64_t wsis_spconv_dw_bn_workspace_bytes(int64_t M_in, int32_t K, int32_t Cin, int32_t Cout);
int wsis_spconv_dw_bn(const float* d_X, const float* d_mean, const float* d_var, const float* d_gamma,
                      const float* d_beta, float eps, int32_t relu, const int32_t* d_nbr_b, const int32_t* d_order_b,
                      int32_t flip, const float* d_dY, float* d_dW, int64_t M_in, int64_t M_out, int32_t K, int32_t Cin,
                      int32_t Cout, void* d_ws, int64_t ws_bytes, void* stream);

/* Live timing of the dominant kernels (bench.py roofline): with profiling enabled every forward / dIn convolution
 * (which = 0) and every weight-gradient product (which = 1) is bracketed by HIP events on its launch stream: one in
 * front of the main kernel, one behind it, and -- where the product is finished by a second launch (the fixed-order sum
 * of offset slabs / workgroup slabs) -- one behind that launch.  wsis_prof_summary synchronises them, returns the
 * summed duration INCLUDING the finishing launches and the count, and clears the list; wsis_prof_records returns the
 * per-product durations in issue order instead (h_main_ms: main kernel only, h_total_ms: with the finishing launch).
 * which = 2: the BatchNorm ops of wsis_run_ops (forward and backward), one event pair around ALL launches of an op
 * (statistics finish + apply): h_main_ms == h_total_ms. */
int wsis_prof_enable(int32_t on);
int wsis_prof_summary(int32_t which, double* total_ms, int64_t* launches);
int wsis_prof_records(int32_t which, double* h_main_ms, double* h_total_ms, int64_t cap, int64_t* n);

/* ---- sync slots of the one-launch reductions ------------------------------------------------------------------
 * Operators that finish a two-level reduction in the SAME launch (last-arrival tickets; published flag for the
 * finish + apply forms) keep their cross-workgroup words in CALLER memory: d_sync points at a 4-KiB slot that the
 * caller zero-fills ONCE (e.g. torch.zeros); every launch leaves its slot zero again, so consecutive launches on one
 * stream may share a slot, launches that may overlap on different streams need different slots.  d_sync == NULL selects
 * the multi-launch form of the operator.  wsis_run_ops takes a block of wsis_sync_bytes() bytes (64 slots, one per op
 * index modulo 64, + one slot for the barrier words of the resident deep-level launches, which the library itself
 * zeroes in front of every such launch).  A wait that does not see its producers within 2 s sets word 19 of the slot
 * (nothing hangs).  One process drives one GPU: the launch plans cache device properties (CU count, LDS
 * limits) of the first device they ran on. */
int64_t wsis_sync_bytes(void);

/* ---- a12: BatchNorm1d(+ReLU) over the active voxels  sparse_unet3d.py:128-137, backbone_3D_WSIS.py:47,52-55 ---
 * Training statistics with a fixed reduction tree (deterministic).  d_ws from wsis_bn_workspace_bytes.
 * wsis_bn_stats: d_mean/d_var [C] (biased var); running stats (optional pair) updated with `momentum` and the
 * unbiased variance, as torch.nn.BatchNorm1d does. */
int64_t wsis_bn_workspace_bytes(int64_t M, int32_t C);
int wsis_bn_stats(const float* d_x, int64_t M, int32_t C, float* d_mean, float* d_var, float* d_running_mean,
                  float* d_running_var, float momentum, void* d_ws, int64_t ws_bytes, void* stream);
/* mean / biased variance (and the running-statistics update) of C channels from the n_part = ceil(M / 32) rows of
 * (sum, centred sum of squares) partials with row pitch 2*C floats written by wsis_spconv_fwd_t(d_stats): fp64,
 * fixed order, two levels (chunk sums in d_ws, then one thread per channel). */
int64_t wsis_bn_stats_finalize_workspace_bytes(int64_t n_part, int32_t C);
int wsis_bn_stats_finalize(const float* d_partials, int64_t n_part, int64_t M, int32_t C, float* d_mean, float* d_var,
                           float* d_running_mean, float* d_running_var, float momentum, void* d_ws, int64_t ws_bytes,
                           void* d_sync, void* stream);
/* wsis_bn_stats_finalize followed by wsis_bn_apply (y = relu?((x - mean) * gamma / sqrt(var + eps) + beta)) as ONE
 * launch where that is possible (a sync slot, C % 4 == 0, a grid of <= 512 resident workgroups): the workgroups that
 * finish the statistics publish them, all wait for that (bounded) and apply.  Identical results to the two calls, which
 * it makes itself otherwise (d_sync == NULL, WSIS_BN_FUSED_APPLY=0, odd shapes).  Same workspace as
 * wsis_bn_stats_finalize. */
int wsis_bn_stats_finalize_apply(const float* d_partials, int64_t n_part, int64_t M, int32_t C, float* d_mean,
                                 float* d_var, float* d_running_mean, float* d_running_var, float momentum,
                                 const float* d_x, const float* d_gamma, const float* d_beta, float eps, int32_t relu,
                                 float* d_y, void* d_ws, int64_t ws_bytes, void* d_sync, void* stream);
/* backward of the fused BN(+ReLU) when dy was produced by wsis_spconv_fwd_t_bn: d_partials holds the n_part =
 * ceil(M / 32) rows of (sum dz, sum dz * xhat) slice partials (pitch 2*C floats) that the convolution's epilogue wrote,
 * so the reduction pass over x and dy of wsis_bn_bwd is replaced by an fp64 sum of the partials (fixed order, chunk
 * sums in d_ws: wsis_bn_stats_finalize_workspace_bytes); then dx as in wsis_bn_bwd (training mode). */
int wsis_bn_bwd_from_partials(const float* d_partials, int64_t n_part, const float* d_x, const float* d_dy,
                              const float* d_mean, const float* d_var, const float* d_gamma, const float* d_beta,
                              float eps, int32_t relu, float* d_dx, float* d_dgamma, float* d_dbeta,
                              const float* d_addend, int64_t M, int32_t C, void* d_ws, int64_t ws_bytes, void* d_sync,
                              void* stream);
/* (with d_dx the reduction finish and the apply pass are one launch where wsis_bn_stats_finalize_apply's conditions
 * hold; identical results) */
/* y = relu?( (x-mean)*rsqrt(var+eps)*gamma + beta )   (gamma/beta may be NULL = 1/0) */
int wsis_bn_apply(const float* d_x, const float* d_mean, const float* d_var, const float* d_gamma,
                  const float* d_beta, float eps, int32_t relu, float* d_y, int64_t M, int32_t C, void* stream);
/* The evaluation-mode apply for 16-bit x [M, C] (dtype 0 = bf16, 1 = fp16) with fp32 statistics and affine parameters:
 * exactly the fp32 arithmetic of wsis_bn_apply on the widened x, rounded ONCE to 16 bits into d_y, or stored as fp32
 * when out_fp32 (then d_y equals wsis_bn_apply of the widened x bit for bit).  C % 4 == 0: x and y aligned to four
 * elements. */
int wsis_bn_apply_lp(const void* d_x, const float* d_mean, const float* d_var, const float* d_gamma,
                     const float* d_beta, float eps, int32_t relu, void* d_y, int32_t out_fp32, int64_t M, int32_t C,
                     int32_t dtype, void* stream);
/* Training statistics of a 16-bit x [M, C] (dtype 0 = bf16, 1 = fp16): what torch's BatchNorm computes for the half
 * features of sparse_unet3d.py:128-137 under mixed precision, here with fp32 statistics and running statistics.  The
 * result is wsis_bn_stats of the widened x BIT FOR BIT: the same kernels instantiated for the element type (same grids,
 * same reduction tree, same branch by M: one launch up to WSIS_BN_SMALL_ROWS rows, partial + final above).  Workspace:
 * wsis_bn_workspace_bytes(M, C).  Domain: C % 8 == 0 (rows are multiples of 16 bytes), C <= 1024, x 16-byte aligned. */
int wsis_bn_stats_lp(const void* d_x, int64_t M, int32_t C, float* d_mean, float* d_var, float* d_running_mean,
                     float* d_running_var, float momentum, void* d_ws, int64_t ws_bytes, int32_t dtype, void* stream);
/* wsis_bn_bwd for 16-bit x, dy and (optional) addend, the backward of the same call sites (sparse_unet3d.py:128-137 under
 * mixed precision): dgamma / dbeta are fp32 and equal wsis_bn_bwd on the widened inputs bit for bit; dx is that call's fp32
 * dx (addend included) rounded ONCE to nearest even into 16-bit d_dx, or stored unrounded as fp32 when out_fp32.  d_dx may
 * be NULL.  Domain and workspace as wsis_bn_stats_lp. */
int wsis_bn_bwd_lp(const void* d_x, const void* d_dy, const float* d_mean, const float* d_var, const float* d_gamma,
                   const float* d_beta, float eps, int32_t relu, int32_t training, void* d_dx, int32_t out_fp32,
                   float* d_dgamma, float* d_dbeta, const void* d_addend, int64_t M, int32_t C, int32_t dtype, void* d_ws,
                   int64_t ws_bytes, void* stream);
/* backward of the fused BN(+ReLU): dgamma = sum dz*xhat, dbeta = sum dz (dz = dy masked by the ReLU),
 * dx = gamma*rstd*(dz - dbeta/M - xhat*dgamma/M) when training, gamma*rstd*dz otherwise; d_dx may be NULL.
 * d_addend (optional, [M,C]) is added to dx in the same pass: the gradient arriving over the residual skip
 * connection of sparse_unet3d.py:164-172, which autograd would otherwise add with one more kernel. */
int wsis_bn_bwd(const float* d_x, const float* d_dy, const float* d_mean, const float* d_var,
                const float* d_gamma, const float* d_beta, float eps, int32_t relu, int32_t training,
                float* d_dx, float* d_dgamma, float* d_dbeta, const float* d_addend, int64_t M, int32_t C, void* d_ws,
                int64_t ws_bytes, void* stream);

/* the apply pass of wsis_bn_bwd alone, from reduced sums: dx = gamma*rstd*(dz - d_sum_dz/M - xhat*d_sum_dz_xhat/M)
 * (+ addend).  For BatchNorm statistics shared across ranks (torch.nn.SyncBatchNorm, train_scannetv2.py:734-736:
 * mean / var over all ranks' rows) the caller all-reduces the two sum vectors of wsis_bn_bwd (d_dx = NULL) and passes
 * them scaled by M / N_global. */
int wsis_bn_bwd_apply(const float* d_x, const float* d_dy, const float* d_mean, const float* d_var,
                      const float* d_gamma, const float* d_beta, const float* d_sum_dz_xhat, const float* d_sum_dz,
                      float eps, int32_t relu, float* d_dx, const float* d_addend, int64_t M, int32_t C, void* stream);
/* wsis_bn_bwd_apply for 16-bit x, dy and (optional) addend (dtype 0 = bf16, 1 = fp16): the apply pass of wsis_bn_bwd_lp
 * alone, from reduced fp32 sums.  dx is rounded ONCE to 16 bits, or stored as fp32 when out_fp32 (then it equals
 * wsis_bn_bwd_apply on the widened inputs bit for bit).  Fed the dgamma / dbeta that wsis_bn_bwd_lp(d_dx = NULL) wrote,
 * dx equals wsis_bn_bwd_lp's own bit for bit.  Domain as wsis_bn_stats_lp (all tensors 16-byte aligned); no workspace. */
int wsis_bn_bwd_apply_lp(const void* d_x, const void* d_dy, const float* d_mean, const float* d_var, const float* d_gamma,
                         const float* d_beta, const float* d_sum_dz_xhat, const float* d_sum_dz, float eps, int32_t relu,
                         void* d_dx, int32_t out_fp32, const void* d_addend, int64_t M, int32_t C, int32_t dtype,
                         void* stream);

/* ---- the statistics exchange of a BatchNorm layer shared across R ranks, one small launch per side of the collective.
 * One thread per channel, fp64, the ranks in ascending order, no atomics: every operation is an IEEE + - * / or a
 * round-to-nearest cast, so the results are the bits a host restatement of the expressions below gives.
 *
 * wsis_bn_sync_pack: what a rank contributes to the all-gather, d_out fp64 [2C + 1] = mean[C], var[C], (double)M of its M
 * local rows.  M == 0 (a rank without rows still enters the collective): zeros, neither pointer is read. */
int wsis_bn_sync_pack(const float* d_mean, const float* d_var, int64_t M, int32_t C, double* d_out, void* stream);
/* wsis_bn_sync_combine: d_gathered fp64 [R][2C + 1] (rank r's wsis_bn_sync_pack in row r) -> statistics over all rows,
 *   N = sum_r n_r,  mean64 = (sum_r m_r n_r) / N,  var64 = (sum_r (v_r + (m_r - mean64)^2) n_r) / N   (sums in ascending r)
 * stored as fp32 d_mean / d_var; d_count[0] = N (fp64, stays on the device for wsis_bn_sync_sums_scale).  With the
 * running pair: rm = (1 - momentum) rm + momentum mean,  rv = (1 - momentum) rv + momentum float(var64 N / max(N - 1, 1))
 * in fp32.  N == 0 (no rank holds a row): mean = var = 0, the running pair stays. */
int wsis_bn_sync_combine(const double* d_gathered, int32_t R, int32_t C, float* d_mean, float* d_var,
                         float* d_running_mean, float* d_running_var, float momentum, double* d_count, void* stream);
/* wsis_bn_sync_sums_pack: the local sums of wsis_bn_bwd / wsis_bn_bwd_lp (d_dx = NULL) widened for the all-reduce, d_out
 * fp64 [2C] = dgamma[C], dbeta[C]; a NULL input (a rank without rows) gives zeros. */
int wsis_bn_sync_sums_pack(const float* d_dgamma, const float* d_dbeta, int32_t C, double* d_out, void* stream);
/* wsis_bn_sync_sums_scale: the all-reduced d_sums fp64 [2C] as the fp32 arguments of wsis_bn_bwd_apply(_lp), which
 * divides by the LOCAL row count M: d_sum_dz_xhat[c] = float(d_sums[c] * ((double)M / d_count[0])), d_sum_dz[c] likewise
 * from d_sums[C + c]. */
int wsis_bn_sync_sums_scale(const double* d_sums, int64_t M, const double* d_count, int32_t C, float* d_sum_dz_xhat,
                            float* d_sum_dz, void* stream);

/* ---- a14/a15: row gather and torch_scatter.scatter  backbone_3D_WSIS.py:179,188,225,232,244 --
 * CSR of a (possibly unsorted) index vector: d_perm int32 [N] = stable argsort(index),
 * d_offsets int32 [S+1].  d_index is int64 [N] (torch_scatter takes LongTensor). */
int64_t wsis_segment_csr_workspace_bytes(int64_t N, int64_t S);
int wsis_segment_csr(const int64_t* d_index, int64_t N, int64_t S, int32_t* d_perm, int32_t* d_offsets,
                     void* d_ws, int64_t ws_bytes, void* stream);
/* The CSRs of up to 8 index vectors from ONE sort (a batch of 3D-WSIS needs six: superpoint ids, p2v map, the two
 * directions of the affinity graph and of the ECC graph): h_index[t] device int64 [h_N[t]], h_S[t] segments.  Table t's
 * perm is d_perm_all[sum_{u<t} h_N[u] ...] (row numbers local to the table), its offsets d_offsets_all[sum_{u<t}
 * (h_S[u] + 1) ...]; identical to wsis_segment_csr per table. */
int64_t wsis_segment_csr_batch_workspace_bytes(int64_t N_all);
int wsis_segment_csr_batch(int32_t n, const void* const* h_index, const int64_t* h_N, const int64_t* h_S,
                           int32_t* d_perm_all, int32_t* d_offsets_all, void* d_ws, int64_t ws_bytes, void* stream);
/* reduce: 0 = sum, 1 = mean (sum / max(count,1)), 2 = max (empty segments -> 0).
 * out [S,C]; d_argmax int32 [S,C] only for max (row index into src, -1 for empty). Points are
 * accumulated in ascending original position => deterministic. */
int wsis_segment_reduce_fwd(const float* d_src, const int32_t* d_perm, const int32_t* d_offsets,
                            float* d_out, int32_t* d_argmax, int64_t N, int64_t S, int32_t C,
                            int32_t reduce, void* stream);
/* dsrc [N,C]: sum -> dout[index[p]]; mean -> dout[index[p]]/max(cnt,1); max -> scattered to argmax
 * rows (dsrc must be zero-initialised for max). */
int wsis_segment_reduce_bwd(const float* d_dout, const int64_t* d_index, const int32_t* d_offsets,
                            const int32_t* d_argmax, float* d_dsrc, int64_t N, int64_t S, int32_t C,
                            int32_t reduce, void* stream);
/* out[p,:] = src[idx[p],:] (int32 or int64 index selected by idx_is_64). */
int wsis_gather_rows(const float* d_src, const void* d_idx, int32_t idx_is_64, float* d_out, int64_t N,
                     int32_t C, void* stream);

/* Position encoding of the edge affinity (backbone_3D_WSIS.py:54-58 fc_position = Linear(3,16) -> ReLU -> Linear(16,1),
 * :222-224 applied to centre[u_e] - centre[v_e]): pos [E] in one launch; backward (no gradient for the centres: they are
 * data) writes every non-NULL dW1 [16,3] / db1 [16] / dW2 [1,16] / db2 [1] in two launches, fixed summation order. */
int64_t wsis_pos_enc_workspace_bytes(int64_t E);
int wsis_pos_enc_fwd(const float* d_centre, const int64_t* d_eu, const int64_t* d_ev, const float* d_W1, const float* d_b1,
                     const float* d_W2, const float* d_b2, float* d_pos, int64_t E, void* stream);
int wsis_pos_enc_bwd(const float* d_centre, const int64_t* d_eu, const int64_t* d_ev, const float* d_W1, const float* d_b1,
                     const float* d_W2, const float* d_dpos, float* d_dW1, float* d_db1, float* d_dW2, float* d_db2, int64_t E,
                     void* d_ws, int64_t ws_bytes, void* stream);

/* ---- a16: edge affinity attention  backbone_3D_WSIS.py:218-249 ------------------------------
 * logit_e = (q[u_e].k[v_e]) * scale * pos_enc_e ; a = segment softmax over edges sharing u ;
 * res[u,:] = sum_e a_e v[v_e,:].  CSR over u: d_perm_u/d_off_u from wsis_segment_csr(edge_u).
 * res [Su,D] with Su = max(u)+1 (rows without edges -> 0). */
int wsis_edge_affinity_fwd(const float* d_q, const float* d_k, const float* d_v, const float* d_pos,
                           const int64_t* d_eu, const int64_t* d_ev, const int32_t* d_perm_u,
                           const int32_t* d_off_u, float scale, float* d_aff, float* d_res, int64_t E,
                           int64_t Su, int32_t D, void* stream);
/* backward: inputs dAff [E] (may be null), dRes [Su,D].  Outputs dq [S,D] (rows >= Su and rows
 * without edges zero), dk, dv [S,D], dpos [E].  Needs CSR over v as well.  d_tmp float [2*E]. */
int wsis_edge_affinity_bwd(const float* d_q, const float* d_k, const float* d_v, const float* d_pos,
                           const float* d_aff, const int64_t* d_eu, const int64_t* d_ev,
                           const int32_t* d_perm_u, const int32_t* d_off_u, const int32_t* d_perm_v,
                           const int32_t* d_off_v, float scale, const float* d_daff,
                           const float* d_dres, float* d_dq, float* d_dk, float* d_dv, float* d_dpos,
                           float* d_tmp, int64_t E, int64_t S, int64_t Su, int32_t D, void* stream);

/* ---- a21: edge-conditioned message passing of the superpoint GNN --------------------------
 * modules/model/spg_modules.py:97-121,168-183 (PyG NNConv, flow=target_to_source, aggr='mean', vv=False):
 *   out[s,:] = mean_{e: src_e = s} x[dst_e,:] @ W_e,  W_e = d_w[e] in R^{C x C}, C <= 32.
 * CSR over the sources (forward) and over the targets (backward) from wsis_segment_csr.  Backward writes
 * dx [S,C] and the per-edge filter gradient dw [E,C,C] (every entry written). */
/* The same messages WITHOUT the per-edge [E, C*C] filter tensor: the filter is affine in the fnet hidden
 * state h_e in R^64 (graphnet.py:19-36: W_e = reshape(Wl h_e + bl)), so m_e = x_t @ W_e = sum_c h_e[c] U_t[c,:] + U_t[64,:]
 * with the per-NODE tensor U [S, 65*32], U_t[c,b] = sum_a x_t[a] Wl[a*32+b, c], row 64 = the bias term (one small GEMM
 * per GRU step, done by the caller).  d_h [E,64], d_U [S,65*32], CSR over the targets; forward writes m [E,32]
 * (every in-edge of every target), backward writes dU [S,65*32] (zeros for targets without in-edge) and dh [E,64].
 * C = 32, hidden width 64 (the model's 'gru_7_0' configuration); one wavefront per target, fixed order. */
int wsis_ecc_contract_fwd(const float* d_h, const float* d_U, const int32_t* d_perm_dst, const int32_t* d_off_dst,
                          float* d_m, int64_t S, int64_t E, void* stream);
int wsis_ecc_contract_bwd(const float* d_h, const float* d_U, const float* d_dm, const int32_t* d_perm_dst,
                          const int32_t* d_off_dst, float* d_dU, float* d_dh, int64_t S, int64_t E, void* stream);
/* accumulate != 0: dh += (every edge row is owned by one wavefront: still fixed order); the R repeats of the
 * recurrence share h, so its gradient is summed in place instead of by R - 1 extra launches */
int wsis_ecc_contract_bwd_acc(const float* d_h, const float* d_U, const float* d_dm, const int32_t* d_perm_dst,
                              const int32_t* d_off_dst, float* d_dU, float* d_dh, int64_t S, int64_t E,
                              int32_t accumulate, void* stream);
/* the same with the backward of the segmented mean that follows the messages folded in (spg_modules.py:97-121,
 * aggr='mean'): dm[e,:] = d_dinp[src_e,:] / out-degree(src_e) is formed on the fly from the source index / CSR offsets */
int wsis_ecc_contract_bwd_mean(const float* d_h, const float* d_U, const float* d_dinp, const int64_t* d_src_index,
                               const int32_t* d_off_src, const int32_t* d_perm_dst, const int32_t* d_off_dst, float* d_dU,
                               float* d_dh, int64_t S, int64_t E, int32_t accumulate, void* stream);
/* the dense product in front of the contraction (graphnet.py:19-36 folded as above): U [S,65*32] = hx [S,32] @ W' [32,65*32] */
int wsis_ecc_u_fwd(const float* d_hx, const float* d_W, float* d_U, int64_t S, void* stream);
int wsis_ecc_message_fwd(const float* d_x, const float* d_w, const int64_t* d_dst, const int32_t* d_perm_src,
                         const int32_t* d_off_src, float* d_out, int64_t S, int64_t E, int32_t C, void* stream);
int wsis_ecc_message_bwd(const float* d_x, const float* d_w, const float* d_dout, const int64_t* d_src,
                         const int32_t* d_perm_dst, const int32_t* d_off_dst, const int32_t* d_off_src,
                         float* d_dx, float* d_dw, int64_t S, int64_t E, int32_t C, void* stream);

/* Column sums out[c] = sum_r x[r, c] of x [M, C] (C % 4 == 0, C <= 1024): the bias gradient of the point-level
 * Linear layers (backbone_3D_WSIS.py:59-64, `dy.sum(0)` in torch's AddmmBackward).  One launch, two levels, fixed
 * summation order (run-to-run identical); inputs of more than one chunk need a sync slot (d_sync, see
 * wsis_sync_bytes). */
int64_t wsis_colsum_workspace_bytes(int64_t M, int32_t C);
int wsis_colsum(const float* d_x, int64_t M, int32_t C, float* d_out, void* d_ws, int64_t ws_bytes, void* d_sync,
                void* stream);

/* Prediction heads over the superpoint rows: replaces the per-layer module chains of
 * modules/model/backbone_3D_WSIS.py:59-64 (`head(cin, cout)` = Linear(cin,cin) -> BatchNorm1d -> ReLU -> Linear(cin,cout)),
 * :195-204 (sp_sem_seg / sp_offset_vector_head / sp_occupancy_head / sp_ins_size_head on the GNN output), :210-216 (the
 * bias-free w_qs / w_ks / w_vs on the same rows) and :253 (feature_term), cin == 64.  All blocks of one call read the same
 * input x [S,64]: blocks 0 .. n_heads-1 are heads (cout <= 32), blocks n_heads .. n_heads+n_lin-1 plain Linear(64,64)
 * layers without bias.  Forward = 3 launches, backward = 4 (csrc/heads.hip), fixed summation orders, exact fp32.
 * The tables hold DEVICE pointers in torch's layouts (Linear weight [out,in]); the struct itself is host memory.
 *   forward   reads W1,b1,gamma,beta,W2,b2 (+ running_* in eval mode), writes hidden[p] [S,64] (heads: the pre-BatchNorm
 *             activations, kept for backward; plain layers: their OUTPUT), out[p] [S,cout[p]], d_saved [n_heads,2,64]
 *             (mean, 1/sqrt(var+eps)); training != 0 uses batch statistics and updates running_* (NULL: not tracked)
 *   backward  reads dout[p] (heads: [S,cout[p]]; plain layers: [S,64]; NULL = zero), hidden, d_saved; writes d_dx [S,64]
 *             and every non-NULL dW1 [64,64] / db1 [64] / dgamma / dbeta [64] / dW2 [cout,64] / db2 [cout] (overwritten) */
#define WSIS_HEADS_MAX 8
typedef struct wsis_heads {
  int32_t n_heads, n_lin;
  int32_t cout[WSIS_HEADS_MAX];
  const float* W1[WSIS_HEADS_MAX];
  const float* b1[WSIS_HEADS_MAX];
  const float* gamma[WSIS_HEADS_MAX];
  const float* beta[WSIS_HEADS_MAX];
  const float* W2[WSIS_HEADS_MAX];
  const float* b2[WSIS_HEADS_MAX];
  float* running_mean[WSIS_HEADS_MAX];
  float* running_var[WSIS_HEADS_MAX];
  float* hidden[WSIS_HEADS_MAX];
  float* out[WSIS_HEADS_MAX];
  const float* dout[WSIS_HEADS_MAX];
  float* dW1[WSIS_HEADS_MAX];
  float* db1[WSIS_HEADS_MAX];
  float* dgamma[WSIS_HEADS_MAX];
  float* dbeta[WSIS_HEADS_MAX];
  float* dW2[WSIS_HEADS_MAX];
  float* db2[WSIS_HEADS_MAX];
} wsis_heads;
int64_t wsis_heads_workspace_bytes(int64_t S, int32_t n_heads, int32_t n_lin);
int wsis_heads_fwd(const wsis_heads* h, const float* d_x, int64_t S, float eps, float momentum, int32_t training,
                   float* d_saved, void* d_ws, int64_t ws_bytes, void* stream);
int wsis_heads_bwd(const wsis_heads* h, const float* d_x, int64_t S, int32_t training, const float* d_saved, float* d_dx,
                   void* d_ws, int64_t ws_bytes, void* stream);

/* GRUCellEx of the superpoint GNN (modules/model/spg_modules.py:207-253: GRU cell + input gate + per-row
 * normalisation of the gate pre-activations), C == 32: one kernel forward, one backward + a fixed-order reduce of
 * the parameter gradients.  Weights in torch.nn.GRUCell layout: Wih/Whh [3C,C] (r,z,n blocks), Wig [C,C]. */
int64_t wsis_gru_cell_workspace_bytes(int64_t S);
int wsis_gru_cell_fwd(const float* d_x, const float* d_h, const float* d_Wig, const float* d_big,
                      const float* d_Wih, const float* d_Whh, const float* d_bih, const float* d_bhh, float* d_hy,
                      int64_t S, int32_t C, void* stream);
int wsis_gru_cell_bwd(const float* d_x, const float* d_h, const float* d_Wig, const float* d_big,
                      const float* d_Wih, const float* d_Whh, const float* d_bih, const float* d_bhh,
                      const float* d_dhy, float* d_dx, float* d_dh, float* d_dWig, float* d_dbig, float* d_dWih,
                      float* d_dWhh, float* d_dbih, float* d_dbhh, int64_t S, int32_t C, void* d_ws,
                      int64_t ws_bytes, void* stream);
/* The same backward as evaluation `slot` of a sequence of `n_slots` evaluations that share the six parameter
 * tensors (the R repeats of spg_modules.py:152-185): every evaluation leaves its parameter-gradient slabs in its own
 * region of d_ws (n_slots x the single-call workspace); the call with finish != 0 reduces ALL regions in one
 * fixed-order launch into d_dW* / d_db* (= the sum over the sequence; may be NULL on the other calls).
 * The upstream gradient of the evaluation is d_dhy + d_dhy2 (either may be NULL): d_dhy2 [S, pitch >= 32] is the output
 * gradient of this hidden state inside the concatenated sequence (cat_all), added on load instead of by a launch. */
int wsis_gru_cell_bwd_seq(const float* d_x, const float* d_h, const float* d_Wig, const float* d_big,
                          const float* d_Wih, const float* d_Whh, const float* d_bih, const float* d_bhh,
                          const float* d_dhy, const float* d_dhy2, int64_t dhy2_pitch, float* d_dx, float* d_dh, float* d_dWig,
                          float* d_dbig, float* d_dWih, float* d_dWhh, float* d_dbih, float* d_dbhh, int64_t S, int32_t C,
                          int32_t slot, int32_t n_slots, int32_t finish, void* d_ws, int64_t ws_bytes, void* stream);
/* wsis_gru_cell_fwd whose input is the segmented MEAN of the edge messages d_m [E,32] over the CSR (d_perm, d_off) of the
 * rows (spg_modules.py:97-121 aggr='mean' followed by the cell, :168-183): the mean is formed per row in the order of
 * wsis_segment_reduce_fwd and written to d_x_out [S,32] (kept for the backward) -- one launch instead of two. */
int wsis_gru_cell_fwd_mean(const float* d_m, const int32_t* d_perm, const int32_t* d_off, float* d_x_out, const float* d_h,
                           const float* d_Wig, const float* d_big, const float* d_Wih, const float* d_Whh, const float* d_bih,
                           const float* d_bhh, float* d_hy, int64_t S, int32_t C, void* stream);

/* LSTMCellEx of the superpoint GNN (modules/model/spg_modules.py:264-318: LSTM cell + input gate + per-row
 * normalisation of the gate pre-activations, the biases inside the norm), C == 32: one kernel forward, one backward +
 * a fixed-order reduce of the parameter gradients.  Weights in torch.nn.LSTMCell layout: Wih/Whh [4C,C] (i,f,g,o
 * blocks), Wig [C,C].  Workspace of the backward: spg_modules.py:264-318 has none; here the per-workgroup slabs. */
int64_t wsis_lstm_cell_workspace_bytes(int64_t S);
/* (hy, cy) = cell(x, (h, c)), all [S,32] (spg_modules.py:264-318, the branch of :298-310).  S == 0 is a no-op. */
int wsis_lstm_cell_fwd(const float* d_x, const float* d_h, const float* d_c, const float* d_Wig, const float* d_big,
                       const float* d_Wih, const float* d_Whh, const float* d_bih, const float* d_bhh, float* d_hy,
                       float* d_cy, int64_t S, int32_t C, void* stream);
/* Backward of spg_modules.py:264-318 from the saved inputs (the forward is recomputed).  d_dhy or d_dcy may be NULL
 * (= zero; not both): the cy of the last repeat has no consumer.  No floating-point atomics: equal inputs give equal
 * bytes.  S >= 1. */
int wsis_lstm_cell_bwd(const float* d_x, const float* d_h, const float* d_c, const float* d_Wig, const float* d_big,
                       const float* d_Wih, const float* d_Whh, const float* d_bih, const float* d_bhh,
                       const float* d_dhy, const float* d_dcy, float* d_dx, float* d_dh, float* d_dc, float* d_dWig,
                       float* d_dbig, float* d_dWih, float* d_dWhh, float* d_dbih, float* d_dbhh, int64_t S, int32_t C,
                       void* d_ws, int64_t ws_bytes, void* stream);

/* ---- a17: dense inter-superpoint affinity + label propagation -------------------------------
 * train_scannetv2.py:562-570, modules/datasets/scannetv2_dataset.py:664-721 (fp64, host numpy).
 * A [S,S] fp64 zero-filled then A[u_e, v_e] = aff_e (edge order, later edges win). */
int wsis_affinity_dense_build(const int64_t* d_eu, const int64_t* d_ev, const float* d_aff, int64_t E,
                              double* d_A, int64_t S, void* stream);
/* T0 = rownorm(A * adj * sem_c) for one class c:
 *   sem[r][j] = (m[r] && m[j]) || (r==j && label[r]==c), m[r] = (pred[r]==c && conf[r]>thr);
 *   adj [S,S] uint8 (adjacency + I); rows summing to 0 are divided by 1. */
int wsis_affinity_transition(const double* d_A, const uint8_t* d_adj, const int32_t* d_pred,
                             const float* d_conf, const int32_t* d_label, int32_t cls, float thr,
                             double* d_T0, int64_t S, void* stream);
/* C = A @ B, fp64 [S,S] row-major on the f64 matrix cores (v_mfma_f64_16x16x4_f64).  Kd = 0: A and B hold nothing (they
 * may be NULL) and C is written as zeros. */
int wsis_dgemm(const double* d_A, const double* d_B, double* d_C, int64_t M, int64_t N, int64_t Kd,
               void* stream);
/* column-wise max / first argmax of T restricted to rows with label[r]==c (other rows count as 0):
 * scores fp64 [S], arg int32 [S]  (np.max/np.argmax(axis=0) semantics, first max wins). */
int wsis_affinity_colmax(const double* d_T, const int32_t* d_label, int32_t cls, double* d_scores,
                         int32_t* d_arg, int64_t S, void* stream);
/* The whole per-scene propagation of scannetv2_dataset.py:689-721 for ALL present classes in one call, exploiting that
 * T0_c = rownorm(A * adj * sem_c) is as sparse as the edge list and that only the rows of the superpoints labelled c of
 * T0_c^(iterations+1) are looked at: W0 = A * adj as CSR (d_col / d_val: caller buffers of nnz_cap >= nnz(A) entries),
 * per class row sums, then per labelled superpoint a chain of (row vector) x (sparse matrix) products in LDS (fp64,
 * k-ascending sums = the order of a dot product) and the column max / first argmax of wsis_affinity_colmax.
 * d_cls_of int32 [n_present] = the present classes ascending, d_ci_of_cls int32 [class_num] = index into d_cls_of or -1;
 * d_scores fp64 [n_present, S], d_arg int32 [n_present, S].  S <= 8188 (two rows of S doubles in LDS); beyond that use
 * wsis_affinity_transition / wsis_dgemm / wsis_affinity_colmax. */
int64_t wsis_affinity_propagate_sparse_workspace_bytes(int64_t S, int32_t n_present);
int wsis_affinity_propagate_sparse(const double* d_A, const uint8_t* d_adj, const int32_t* d_pred, const float* d_conf,
                                   const int32_t* d_label, const int32_t* d_cls_of, const int32_t* d_ci_of_cls,
                                   int32_t n_present, int32_t class_num, float thr, int32_t iterations, int64_t S,
                                   int32_t* d_col, double* d_val, int64_t nnz_cap, double* d_scores, int32_t* d_arg,
                                   void* d_ws, int64_t ws_bytes, void* stream);

/* ---- a19/a20: ballquery_batch_p / bfs_cluster [UPSTREAM PG_OP] ------------------------------
 * For point p: ascending indices k of same-batch points with |x_p-x_k|^2 < r^2 (strict, incl. p),
 * capped at 1000.  Deterministic offsets = exclusive prefix sum of the counts.
 * Pass 1 writes d_start_len int32 [N,2] and d_total int32[1]; pass 2 fills d_idx int32 [total] and must get
 * the SAME workspace back untouched (it holds the uniform grid: points radix-sorted by cell of size ~radius and
 * a cell hash; each point visits 27 cells instead of its whole batch item).  B < 1024, |coordinate| < 2^17 cells. */
int64_t wsis_ballquery_workspace_bytes(int64_t N);
int wsis_ballquery_count(const float* d_xyz, const int32_t* d_batch_idx, const int32_t* d_batch_off,
                         int64_t N, int32_t B, float radius, int32_t* d_start_len, int32_t* d_total,
                         void* d_ws, int64_t ws_bytes, void* stream);
int wsis_ballquery_fill(const float* d_xyz, const int32_t* d_batch_idx, const int32_t* d_batch_off,
                        int64_t N, int32_t B, float radius, const int32_t* d_start_len, int32_t* d_idx,
                        int64_t total, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- a20 on the device: pointgroup_ops.bfs_cluster(semantic_label, ball_query_idxs, start_len, threshold) [UPSTREAM
 * PointGroup, host code] with CUDA tensors.  wsis_cc_same_label: connected components of the ball-query graph
 * restricted to equal labels, d_root[i] = smallest point index of i's component (the host walk's seed),
 * d_size[root] = its point count (d_parent: int32 [N] scratch).  The caller keeps the components of >= threshold
 * points, numbers them in seed order (d_seeds, exclusive prefix d_offsets [n+1]) and wsis_bfs_order writes
 * cluster_idxs [sum, 2] = (cluster id, point) in the host walk's FIFO discovery order: one workgroup per cluster,
 * d_pos int32 [N] preset to -1, d_stamp int32 [N] preset to INT32_MAX. */
int wsis_cc_same_label(const int32_t* d_sem, const int32_t* d_idx, const int32_t* d_start_len, int64_t N,
                       int32_t* d_parent, int32_t* d_root, int32_t* d_size, void* stream);
int wsis_bfs_order(const int32_t* d_idx, const int32_t* d_start_len, const int32_t* d_sem, const int32_t* d_seeds,
                   const int32_t* d_offsets, int64_t n_clusters, int32_t* d_pos, int32_t* d_stamp,
                   int32_t* d_cluster_idxs, void* stream);

/* ---- S3DIS wall split: utils/planeSegment.py:29-63 (get_room_walls, called at test_s3dis.py:533), which runs open3d's
 * PointCloud.segment_plane(distance, 3, iter) once per wall [UPSTREAM open3d].  One such call is `iter` candidate planes
 * scored against every remaining wall point; wsis_plane_score scores all H candidates in one pass over the points.
 * d_xyz fp32 [N,3]; d_planes fp64 [H,4] = (a, b, c, d), unit normal; dist_i = |((a*x + b*y) + c*z) + d| with x, y, z
 * widened to fp64, in that order, uncontracted.  d_count[h] int64 = #{i : dist_i < thr} (strict; a non-finite
 * coordinate is never an inlier), d_sumsq[h] fp64 = sum of dist_i^2 over those i.  The counts are exact; the sums are
 * added in an order fixed by (N, H) (per-workgroup rows in d_ws, added in row order by a second launch: no atomics), so
 * they are bit-reproducible.  1 <= H <= 1024 (more hypotheses: several calls); N == 0 writes zeros without a launch.
 * The workspace query returns -1 for N < 0 or H outside [1, 1024]. */
int64_t wsis_plane_score_workspace_bytes(int64_t N, int32_t H);
int wsis_plane_score(const float* d_xyz, int64_t N, const double* d_planes, int32_t H, double thr, int64_t* d_count,
                     double* d_sumsq, void* d_ws, int64_t ws_bytes, void* stream);
/* utils/planeSegment.py:45-58 / open3d segment_plane's inlier index: d_mask uint8 [N], 1 where dist_i < thr for the ONE
 * plane d_plane4 fp64 [4] -- the same expression and the same strict comparison as wsis_plane_score, so the number of
 * ones equals that call's count. */
int wsis_plane_mark(const float* d_xyz, int64_t N, const double* d_plane4, double thr, uint8_t* d_mask, void* stream);

/* ---- weak-label stage updates: modules/datasets/scannetv2_dataset.py:515-964 (s3dis_dataset.py has the same methods),
 * called at the stage boundaries of train_scannetv2.py:477-480, 575-577, 664-666.  The reference builds one mask
 * `superpoint == spID` per superpoint (O(S*N)); here every per-point stage is one pass.  Labels are int64 [S] with -100
 * for "none"; a superpoint is LABELLED when semantic and instance label are both != -100; offset vectors are fp64 [S,3].
 * No floating-point atomics: every float result is bit-identical from run to run.
 *
 * wsis_wl_sp_stats replaces every `xyz_origin[superpoint == spID].mean(0)` / `.sum(0)` / `spMask.sum()` of :753-757,
 * :798-803, :888-889, :909-910, :937-945: d_sum fp32 [S,3], d_count int32 [S], d_centre fp32 [S,3] = sum / count of the
 * fp32 coordinates, accumulated in fp32 (one wave per superpoint over the CSR d_perm / d_offsets of wsis_segment_csr, fixed
 * order).  A superpoint without points gets a NaN centre; callers refuse such input. */
int wsis_wl_sp_stats(const float* d_xyz, const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t S,
                     float* d_sum, int32_t* d_count, float* d_centre, void* stream);
/* extend_label_to_neighbor :780-805 / propagate_label_to_neighbor :823-852, the choice of the source: d_src int32 [S] =
 * the LARGEST labelled k adjacent to n in either direction of d_edges int64 [E,2] with sem[k] == d_pred[n], for n with both
 * labels -100 and (d_conf != NULL) float64(d_conf[n]) > thr; -1 where there is none.  The reference visits k ascending
 * and the last writer wins.  d_conf == NULL drops the confidence test (:839).  E == 0 writes -1 everywhere. */
int wsis_wl_neighbor_source(const int64_t* d_edges, int64_t E, const int64_t* d_sem, const int64_t* d_ins,
                            const int64_t* d_pred, const float* d_conf, double thr, int64_t S, int32_t* d_src,
                            void* stream);
/* What both stages and weak_label_propagation :746-770 write: for every i with k = d_src[i] in [0, S):
 * sem_out[i] = sem[k], ins_out[i] = ins[k], off_out[i] = (float64(centre[k]) + off[k]) - float64(centre[i]); every other
 * row is copied.  d_is1ins int64 [E] is recomputed from ins_out for every edge: 0 if either end is -100, -1 if equal,
 * 1 otherwise (:761-770, :807-816, :854-863).  The outputs may not alias the inputs (the reference reads the old graph). */
int wsis_wl_apply_source(const int32_t* d_src, const int64_t* d_sem, const int64_t* d_ins, const double* d_off,
                         const float* d_centre, const int64_t* d_edges, int64_t E, int64_t S, int64_t* d_sem_out,
                         int64_t* d_ins_out, double* d_off_out, int64_t* d_is1ins, void* stream);
/* propagate_label_to_whole_scene :873-964.  d_prior int32 [P]: the labelled superpoints, ascending; prior p has the
 * instance centre c_p = float64(centre[p]) + off[p].  Every superpoint i that is not labelled looks, among the priors
 * with sem == d_pred[i], for the smallest ||c_p - q_i||_2 (fp64, sqrt((dx*dx + dy*dy) + dz*dz) uncontracted; q_i =
 * centre[i] + d_pred_off[i] added in fp32; first index on equal distances; priors staged in LDS 256 at a time).
 * d_assigned int32 [S] = that prior's index in d_prior, or -1 (labelled, no candidate, or distance > max_dist, strict);
 * d_dist fp64 [S] = the smallest distance (+inf without a candidate).  An assigned i gets the prior's labels and
 * off_out[i] = g_p - float64(centre[i]) with g_p = sum float64(d_sum[i]) / sum d_count[i] over the superpoints assigned
 * to p, added in ascending i; every other row is copied.  P == 0 is valid.  The outputs may not alias the inputs. */
int wsis_wl_scene_assign(const int32_t* d_prior, int64_t P, const int64_t* d_sem, const int64_t* d_ins,
                         const double* d_off, const float* d_centre, const float* d_sum, const int32_t* d_count,
                         const int64_t* d_pred, const float* d_pred_off, double max_dist, int64_t S, int32_t* d_assigned,
                         double* d_dist, int64_t* d_sem_out, int64_t* d_ins_out, double* d_off_out, void* stream);
/* generate_point_level_weak_label :581-590: fp64 [N] point labels = the two labels of the point's superpoint (d_sp
 * int64 [N]) if it is labelled, else -100. */
int wsis_wl_point_labels(const int64_t* d_sp, int64_t N, const int64_t* d_sem, const int64_t* d_ins, double* d_weak_sem,
                         double* d_weak_ins, void* stream);
/* cal_occupancy :515-542.  d_rank_sp int32 [S] = rank in [0, R) of the weak instance label the points of a superpoint
 * carry (-100 has a rank of its own).  d_vox_count int64 [R] = number of distinct (trunc(float32(xyz) * scale)) triples
 * among the points of each rank: one key pass, wsis_voxelize_idx_map on (rank, voxel), one counting pass. */
int64_t wsis_wl_occupancy_workspace_bytes(int64_t N);
int wsis_wl_occupancy(const float* d_xyz, const int64_t* d_sp, const int32_t* d_rank_sp, int64_t N, int32_t R,
                      float scale, int64_t* d_vox_count, void* d_ws, int64_t ws_bytes, void* stream);
/* cal_instance_size :545-564.  d_rank int32 [S] = rank in [0, R) of int(instance_label) of every vertex; d_rmax fp64 [R]
 * = max(0, max ||off_v||_2) over the vertices of the rank (fp64); d_size fp64 [S] = d_rmax[rank].  The maximum is an
 * integer atomic on the bit pattern of the non-negative norm: independent of the order of arrival. */
int wsis_wl_instance_size(const double* d_off, const int32_t* d_rank, int64_t S, int32_t R, double* d_rmax,
                          double* d_size, void* stream);
/* the label statistics of :602-640 in one pass: d_counters int64 [8] = GT_all, GT_label, semantic_label_num,
 * correct_semantic_label_num, floor_wall_sem_num, floor_wall_correct_sem_num, instance_label_num,
 * correct_instance_label_num; h_stuff: HOST array of the n_stuff <= 8 "floor & wall" classes (ScanNet and S3DIS: 0, 1). */
int wsis_wl_label_stats(const double* d_weak_sem, const double* d_weak_ins, const double* d_sem_gt,
                        const double* d_ins_gt, int64_t N, const double* h_stuff, int32_t n_stuff, int64_t* d_counters,
                        void* stream);

/* ---- per-scene preparation of a training item: ScanNetV2Inst_spg.__getitem__ (modules/datasets/scannetv2_dataset.py:96-190)
 * and its S3DIS twin (s3dis_dataset.py:126-206), one pass per stage over data that stays on the device (csrc/sceneprep.hip;
 * driven by wsis_datasets.DeviceScenePrep).  No floating-point atomics: every float result is bit-identical from run to
 * run.  Sizes are below 2^31; instance ids are below WSIS_SP_MAX_IDS (the reference has no such limit: more ids are
 * refused with WSIS_ERR_OVERFLOW).  Unlike the reference, an id outside its table (a superpoint id >= S, an instance id
 * >= n_ids, an index of d_pick outside [0, n_src), more ones in a mask than n_out) is not an exception on the spot: it is
 * counted in word 6 of the state block, which the caller reads with its other counts.
 *
 * The state block: WSIS_SP_STATE_WORDS uint64 words in device memory, set up by wsis_sp_state_init once per item.
 *   words 0-2 / 3-5   per-column minimum / maximum of xyz_scaled, as ORDERED keys of the doubles (key = ~bits for a
 *                     negative value, bits | 2^63 otherwise: unsigned order of the keys = order of the doubles)
 *   word 6            number of out-of-table ids met (0 on valid input)
 *   words 8-10        per-column maximum of loc (wsis_sp_emit)
 *   word 11, 12       number of kept superpoints S', number of instance ids present k (wsis_sp_tables)
 *   words 16+4r ..    crop round r < WSIS_SP_ROUNDS: number of ones of its mask, then the ordered keys of the per-column
 *                     minimum of x over the kept points (all-ones keys when the mask is empty) */
#define WSIS_SP_ROUNDS 32
#define WSIS_SP_STATE_WORDS (16 + 4 * WSIS_SP_ROUNDS)
#define WSIS_SP_MAX_IDS 65536
int64_t wsis_sp_state_bytes(void);
int wsis_sp_state_init(void* d_state, void* stream);
/* data_aug_with_graph :194-209 with the matrix of :211-222 drawn by the caller, `xyz = xyz_middle * scale` :149 and the
 * bounds behind `xyz -= xyz.min(0)` :151-152 and room_range :259.  d_in [n_src,3] fp32 (in_f64 == 0) or fp64 (the graph's
 * superpoint_offset_vector); row i of the outputs comes from row d_pick[i] of d_in (d_pick int64 [n], the S3DIS quarter
 * of s3dis_dataset.py:135-144) or from row i (d_pick NULL).  h_m9: HOST fp64 [3,3] row-major.  d_middle fp64 [n,3], column
 * j = fma(z, m[2][j], fma(y, m[1][j], x * m[0][j])) on coordinates widened to fp64 -- np.matmul's result bit for bit;
 * d_scaled fp64 [n,3] = d_middle * scale and the bounds in the state block (both skipped when d_scaled is NULL; d_state
 * may then be NULL too). */
int wsis_sp_affine(const void* d_in, int32_t in_f64, const int64_t* d_pick, int64_t n_src, int64_t n, const double* h_m9,
                   double scale, double* d_middle, double* d_scaled, void* d_state, void* stream);
/* elastic :222-249 (s3dis_dataset.py:232-259 is the same method), PointGroup's elastic distortion, on the scaled
 * coordinates of wsis_sp_affine.  The reference defines the method and reads `with_elastic` (:39) but never calls it; the
 * call site is PointGroup's [UPSTREAM].  The noise is drawn by the caller (the order of the random draws
 * is the contract): d_grids fp32 [3, bb0, bb1, bb2], the three grids of `noise` :238 one after the other; h_bb3 HOST
 * int32 [3], every entry >= 3 and bb0*bb1*bb2 < 2^31.
 * Blur: the six scipy.ndimage.convolve calls of :239-244 (axis 0, 1, 2, 0, 1, 2; mode="constant", cval=0), one launch per
 * pass over the three grids: out[i] = fp32((w*in[i-1] + w*in[i]) + w*in[i+1]) along the axis, in fp64 with
 * w = fp64(fp32(1)/fp32(3)), a neighbour outside the grid counting as 0 -- scipy's result bit for bit.  d_tmp: workspace
 * of the size of d_grids; the result is in d_grids. */
int wsis_elastic_blur(float* d_grids, float* d_tmp, const int32_t* h_bb3, void* stream);
/* Apply: :245-249 in place on d_xyz fp64 [n,3], one thread per point.  Axis j has the nodes -(bb_j-1)*gran + 2*gran*k
 * (np.linspace :245, exact integers); per axis i = clip(#nodes < x - 1, 0, bb_j-2), t = (x - a[i]) / (a[i+1] - a[i]); the
 * displacement d_m = sum over the eight corners (cx,cy,cz) = 000, 001, ..., 111 of fp64(grid_m[i0+cx, i1+cy, i2+cz]) *
 * ((wx*wy)*wz), w = t or 1 - t, from 0.0 (scipy's RegularGridInterpolator :246, bit for bit); a point with a coordinate
 * outside [a[0], a[last]] on any axis gets d = 0 on all three (fill_value=0); d_xyz[i,m] += d_m * mag.  Indices and weights
 * are computed once for the three grids.  d_bounds: uint64 [6] in device memory, a block of its own that the call
 * initialises: the ORDERED keys (see the state block) of the per-column minimum / maximum of the result; n == 0 leaves
 * them at all-ones / zero.  gran >= 1 and (bb_j-1)*gran < 2^52 (the nodes are integers fp64 holds exactly). */
int wsis_elastic_apply(double* d_xyz, int64_t n, const float* d_grids, const int32_t* h_bb3, int32_t gran, double mag,
                          void* d_bounds, void* stream);
/* One round of crop :252-273 (form 1) or of crop_v2 s3dis_dataset.py:285-319 (form 2) on x = d_scaled - h_min3 (HOST
 * fp64 [3], the decoded minima): form 1, mask_i = all_j(x_ij + a_j >= 0) and all_j(x_ij + a_j < b_j) with a = offset, b =
 * full_scale; form 2, mask_i = a_j <= x_ij <= b_j on columns 0 and 1 (a = lo, b = hi).  One fp64 operation and one
 * compare per element, as the reference: the mask is exact.  d_mask uint8 [n]; the count and the kept-point minima go to
 * round `round` of the state block.  The loops, and with them the order of the random draws, stay with the caller. */
int wsis_sp_crop_mask(const double* d_scaled, int64_t n, const double* h_min3, int32_t form, const double* h_a3,
                      const double* h_b3, uint8_t* d_mask, void* d_state, int32_t round, void* stream);
/* The boolean-mask gathers of :155-160 in the dtypes collate_fn ends with (:343-474), kept points in their original
 * order (d_mask NULL: every point).  For kept point i, output row o, source row p = d_pick[i] or i:
 *   d_loc int64 [n_out,3] = trunc toward zero of ((d_scaled[i] - h_min3) + h_off3) (`torch.from_numpy(xyz).long()` :176;
 *     h_off3 = the last crop offset, or minus the kept-point minimum for crop_v2), its column maxima in the state block;
 *   d_loc_float fp32 = d_middle[i] rounded to nearest, d_middle_kept fp64 = d_middle[i];
 *   d_feat fp32 = d_rgb[p] + h_jitter3 (HOST fp32 [3]; NULL: no jitter);  d_sem_out = d_sem[p];
 *   d_ins_raw = d_ins[p], the instance label before re-compaction;  d_sp_old = d_sp[p].
 * d_flags int32 [S + n_ids], zeroed by the call: [s] = 1 for every kept superpoint id, [S + id] = 1 for every kept
 * instance id >= 0.  n_out: rows the outputs have room for (the count of the mask).  The workspace holds one count per
 * 1024 points; the query returns -1 outside the domain. */
int64_t wsis_sp_emit_workspace_bytes(int64_t n, int64_t S, int64_t n_ids);
int wsis_sp_emit(const uint8_t* d_mask, const int64_t* d_pick, int64_t n_src, int64_t n, int64_t n_out,
                 const double* d_scaled, const double* d_middle, const double* h_min3, const double* h_off3,
                 const float* d_rgb, const float* h_jitter3, const int64_t* d_sem, const int64_t* d_ins,
                 const int64_t* d_sp, int64_t S, int64_t n_ids, int64_t* d_loc, float* d_loc_float,
                 double* d_middle_kept, float* d_feat, int64_t* d_sem_out, int64_t* d_ins_raw, int64_t* d_sp_old,
                 int32_t* d_flags, void* d_state, void* d_ws, int64_t ws_bytes, void* stream);
/* The two id tables from d_flags of wsis_sp_emit, one workgroup, O(S + n_ids), no sort:
 *   np.unique(superpoint, return_inverse=True) :169 -- d_subset int64 [S]: the first S' entries are the kept ids,
 *     ascending; d_sp_new int32 [S]: the rank of a kept id, -1 otherwise;
 *   get_cropped_inst_label :311-330 -- d_ins_map int32 [n_ids]: new id of a present id, -1 otherwise.  The reference walks
 *     j upward while j < the current maximum and lets an empty j take over the points of the current largest id: with k
 *     ids present, the i-th empty id below k takes the i-th largest present id, ids below k stay.
 * d_scratch int32 [2 * n_ids].  S' and k go to the state block. */
int wsis_sp_tables(const int32_t* d_flags, int64_t S, int64_t n_ids, int32_t* d_sp_new, int64_t* d_subset,
                   int32_t* d_ins_map, int32_t* d_scratch, void* d_state, void* stream);
/* One gather per point: d_sp_out int64 [n] = d_sp_new[d_sp_old], d_ins_out int64 [n] = d_ins_map[d_ins_raw] with
 * negative labels (-100) passed through, d_seg int64 [n] = d_ins_out, or n_ids for a point without an instance: the
 * index vector whose wsis_segment_csr (n_ids + 1 segments) wsis_sp_instance_info walks. */
int wsis_sp_relabel(const int64_t* d_sp_old, const int64_t* d_ins_raw, int64_t n, const int32_t* d_sp_new, int64_t S,
                    const int32_t* d_ins_map, int64_t n_ids, int64_t* d_sp_out, int64_t* d_ins_out, int64_t* d_seg,
                    void* stream);
/* get_instance_info :275-309.  d_perm / d_offsets: CSR of d_seg over K + 1 segments.  One wave per instance id: fp64 sum
 * (lane l adds the points l, l + 64, ... of the row in order, then one xor butterfly), minimum and maximum of d_middle
 * fp64 [n,3]; d_info fp32 [n,9] row of every point of the id = (sum / count, min, max), each cast to fp32; the points of
 * segment K (no instance) get -100.0 in all nine columns; d_pointnum int32 [K] = points per id.  An id without points
 * writes no row and count 0 (the reference would fail on its empty minimum).  The order of the sum is fixed but not
 * numpy's: columns 0:3 may differ from the reference by one fp32 step, never more. */
int wsis_sp_instance_info(const double* d_middle, const int32_t* d_perm, const int32_t* d_offsets, int64_t n, int64_t K,
                          float* d_info, int32_t* d_pointnum, void* stream);

/* ---- building the superpoint graph of a scene: data/ScanNetV2/prepare_data_inst_ScanNetV2.py (build_weak_label_graph
 * :172-285, compute_edges_feature :340-433) and data/S3DIS/prepare_S3DIS_inst_data.py (build_graph_10NBR :101-224,
 * compute_edges_feature :268-358), the per-point and per-pair parts (csrc/graphprep.hip; driven by wsis_graph_prep).  The
 * reference forms one `np.where(superpoint == spID)` mask per superpoint and use (O(S*N)); here one wave walks one row of
 * the point CSR d_perm / d_offsets of wsis_segment_csr (stable: a row lists its points in ascending index order, the
 * order of xyz[np.where(superpoint == spID)[0]]).  No floating-point atomics, fixed summation order (lane l takes the
 * entries l, l + 64, ... of its row, then one xor butterfly): two calls give the same bytes.
 *
 * wsis_gp_sp_moments replaces the superpoint loop of compute_edges_feature (ScanNet :359-394, S3DIS :287-322) and the
 * centres of :208-211 / :132-135.  d_count int64 [S]; d_centroid fp32 [S,3] = the fp64 mean of the widened fp32
 * coordinates, rounded; d_cov6 fp64 [S,6] = (xx, yy, zz, xy, xz, yz) central second moments about that fp64 mean, divided
 * by n - 1 for n >= 3 (np.cov), by n for n == 2 (np.var), zero for n == 1; d_ev3 fp64 [S,3] = its eigenvalues, descending
 * (cyclic Jacobi, at most 12 sweeps), zero for n < 3.  d_length / d_surface / d_volume fp32 [S]: n == 1: 0, 0, 0;
 * n == 2: sqrt(xx + yy + zz), 0, 0; n >= 3: ev0, sqrt(ev0 * ev1 + 1e-10), sqrt(ev0 * ev1 * ev2 + 1e-10), evaluated in fp64
 * and rounded.  d_cov6 and d_ev3 may be NULL. */
int wsis_gp_sp_moments(const float* d_xyz, const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t S,
                       int64_t* d_count, float* d_centroid, float* d_length, float* d_surface, float* d_volume,
                       double* d_cov6, double* d_ev3, void* stream);
/* stats.mode(labels[spMask])[0][0] of ScanNet :241-249 / S3DIS :173-183.  d_rank int32 [N]: the dense rank of every
 * point's label among the distinct label values in ascending order (-100 has a rank like any other value).  d_mode int32
 * [S] = the most frequent rank of the row, the smallest one on a tie (-1 for a row without points); d_mode_count int32 [S]
 * = how often it occurs.  Integer only; cost = distinct labels of the row x row length. */
int wsis_gp_label_mode(const int32_t* d_rank, const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t S,
                       int32_t* d_mode, int32_t* d_mode_count, void* stream);
/* KDTree(superpoint_center).query_radius(r) of ScanNet :213-215 / .query(k = 11) of S3DIS :141-156, by brute force over the
 * d_centres fp32 [S,3]: d2 = (dx*dx + dy*dy) + dz*dz on coordinates widened to fp64, uncontracted.  Row s of d_nbr int32
 * [S,k] / d_dist2 fp64 [S,k]: the OTHER superpoints (self is excluded by id) with d2 <= radius * radius, ascending in
 * (d2, id), padded with -1 / +inf; d_count int32 [S] = how many satisfy the radius, which may exceed k.  radius may be
 * +inf; 1 <= k <= 128. */
int wsis_gp_neighbors(const float* d_centres, int64_t S, int32_t k, double radius, int32_t* d_nbr, double* d_dist2,
                      int32_t* d_count, void* stream);
/* The edge loop of compute_edges_feature (ScanNet :398-426, S3DIS :325-354): d_out fp32 [E,13] = delta mean 3, delta std 3,
 * centroid[s] - centroid[t] 3, length / surface / volume ratios a[s] / (a[t] + 1e-6f) in fp32, the point-count ratio
 * n_s / (n_t + 1e-6) in fp64 rounded to fp32, for the directed edges d_edges int64 [E,2].  Pair j of (s, t) = (point j of
 * the smaller row, point d_samp[d_samp_off[e] + j] of the larger row), (j, j) for rows of equal length: the caller draws
 * the np.random.choice(n_big, n_small, replace=False) of :409-412 and passes them as one CSR (d_samp_off int64 [E+1],
 * d_samp int32; an edge between rows of equal length has an empty list).  delta = xs - xt in fp32; its mean and population
 * standard deviation per column in fp64 (two passes), rounded to fp32; one pair: mean = delta, std = 0 (:419-421).  An
 * edge with an endpoint outside [0, S) or a list of the wrong length gets a row of NaN; a sample index is clamped to its
 * row. */
int wsis_gp_edge_features(const float* d_xyz, const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t S,
                          const int64_t* d_edges, int64_t E, const int64_t* d_samp_off, const int32_t* d_samp,
                          const float* d_centroid, const float* d_length, const float* d_surface, const float* d_volume,
                          float* d_out, void* stream);

/* ---- the S3DIS partition front end: the array stages of generate_SPG_superpoint (data/S3DIS/partition/
 * partition_S3DIS.py:81-115) before the l0 cut-pursuit solver (csrc/partition.hip; driven by wsis_partition; the
 * solver itself is the wsis_cp_* group below).  No floating-point atomics, fixed summation order, uncontracted products: two calls give the same
 * bytes.  Every index read from a table is clamped to its table before use.
 *
 * wsis_pt_bins: the voxel of every point, libply_c.prune ply_c/ply_c.cpp:311-337.  d_min3 fp32 [3] = the per-axis
 * minimum of d_xyz fp32 [N,3]; d_coords int64 [N,4] = (0, bx, by, bz), b = floorf((x - x_min) / voxel) with an fp32
 * subtraction and a correctly rounded fp32 division, NOT clamped to n_bin (the reference does not: a point at x_max on
 * a cell boundary has bin n_bin) -- the rows wsis_voxelize_idx_map takes, whose first-occurrence ids are the insertion
 * index of the reference's std::map (:175-189).  *d_nonfinite = 1 if a coordinate is NaN or infinite (the bins of such
 * input are defined but meaningless: the caller refuses it), else 0.  d_ws: wsis_pt_bins_workspace_bytes(N). */
int64_t wsis_pt_bins_workspace_bytes(int64_t N);
int wsis_pt_bins(const float* d_xyz, int64_t N, float voxel, int64_t* d_coords, float* d_min3, int32_t* d_nonfinite,
                 void* d_ws, int64_t ws_bytes, void* stream);
/* The voxel averages of libply_c.prune (ply_c.cpp:255-290, 368-390) over the point CSR d_perm / d_offsets of
 * wsis_segment_csr(point_to_voxel) (a row lists its points in ascending index order): one sequential chain per voxel.
 * d_out_xyz fp32 [V,3] = the fp32 sum of the coordinates in point order, divided by (float)count; d_out_rgb uint8 [V,3]
 * = (uint8)((float)sum / (float)count) of the uint32 colour sums (truncation); d_count int32 [V]; with d_labels int32 [N]
 * (else NULL) d_label_hist uint32 [V, n_labels + 1], the label being the column.  A label outside [0, n_labels] is not
 * counted: the caller refuses such input before the launch (the reference's .at() throws). */
int wsis_pt_prune_accumulate(const float* d_xyz, const uint8_t* d_rgb, const int32_t* d_labels, int32_t n_labels,
                             const int32_t* d_perm, const int32_t* d_offsets, int64_t N, int64_t V, float* d_out_xyz,
                             uint8_t* d_out_rgb, uint32_t* d_label_hist, int32_t* d_count, void* stream);
/* NearestNeighbors(k + 1, 'kd_tree').kneighbors of graphs.py:34-38: the exact k nearest neighbours of every point among
 * the same V points.  d2 = (dx*dx + dy*dy) + dz*dz on coordinates widened to fp64; row v of d_nbr int32 [V,k] / d_dist2
 * fp64 [V,k] ascends in (d2, id), self excluded by id.  1 <= k <= 64, V >= k + 1.  The points are sorted by the key of a
 * uniform grid cell (edge `cell`; cell <= 0: chosen from the bounding box and V) and cells are found through the sorted
 * keys: the workspace is O(V) whatever the extent.  One wave per query visits the cells ring by ring and stops when the
 * k-th d2 is below the squared distance to the nearest face of the searched block; after 3 rings it scans every point
 * instead.  d_stats int32 [V,2] (may be NULL): candidates evaluated, 1 if the query took that scan. */
int64_t wsis_pt_knn_workspace_bytes(int64_t V);
int wsis_pt_knn(const float* d_xyz, int64_t V, int32_t k, double cell, int32_t* d_nbr, double* d_dist2, int32_t* d_stats,
                void* d_ws, int64_t ws_bytes, void* stream);
/* libply_c.compute_geof (ply_c.cpp:406-463) in fp64: per point the mean and the six central second moments of the k + 1
 * positions (self, then d_nbr[v][0..k)), divided by k + 1; eigenvalues and eigenvectors by cyclic Jacobi (at most 12
 * sweeps), eigenvalues descending and clamped at 0; d_geof fp32 [V,4] = linearity, planarity, scattering, verticality of
 * :448-458, each rounded to fp32 once (lambda_0 = 0 gives NaN, as the reference's expressions do).  d_cov6 fp64 [V,6] =
 * (xx, yy, zz, xy, xz, yz) and d_ev3 fp64 [V,3] may be NULL. */
int wsis_pt_geof(const float* d_xyz, const int32_t* d_nbr, int64_t V, int32_t k, float* d_geof, double* d_cov6,
                 double* d_ev3, void* stream);
/* partition_S3DIS.py:105-108 and the graph arrays of graphs.py:69-74.  d_features fp32 [V,7] = linearity, planarity,
 * scattering, 2 * verticality, (float)((double)c / 255.0) of the three colours; d_source / d_target uint32 [V * k_adj] =
 * v repeated, the first k_adj neighbours of v; d_distances fp32 = (float)sqrt(dist2); *d_mean fp32 = the fp64 sum of
 * those distances in index order over their count -- two levels of sequential chains: every chunk of 256 consecutive
 * distances is added in index order, then the chunk sums are added in index order (the result depends on that chunk
 * length alone) --,
 * rounded once; d_edge_weight = 1.f / (lambda + d / mean) in fp32.  1 <= k_adj <= k <= 64. */
int64_t wsis_pt_edge_features_workspace_bytes(int64_t V, int32_t k_adj);
int wsis_pt_edge_features(const float* d_geof, const uint8_t* d_rgb, const int32_t* d_nbr, const double* d_dist2, int64_t V,
                          int32_t k, int32_t k_adj, float lambda, float* d_features, uint32_t* d_source,
                          uint32_t* d_target, float* d_distances, float* d_edge_weight, float* d_mean, void* d_ws,
                          int64_t ws_bytes, void* stream);

/* ---- l0 cut pursuit with L2 fidelity: libcp.cutpursuit of partition_S3DIS.py:110-111 (data/S3DIS/partition/cut-pursuit:
 * src/cutpursuit.cpp:77-105, include/API.h:959-974, include/CutPursuit.h, include/CutPursuit_L2.h; mode 1, speed 4) as
 * stages (csrc/cutpursuit.hip; driven by wsis_partition.cut_pursuit).  Node weights are 1.  No
 * floating-point atomic, fixed summation orders, integer flow: two calls give the same bytes.  No workgroup waits for
 * another; every loop over launches runs on the host, is bounded and returns WSIS_ERR_OVERFLOW at its bound.  d_source /
 * d_target int32 [E] < V; d_comp int32 [V] = component of a node; d_comp_off int32 [C+1] / d_comp_nodes int32 [V] = the
 * nodes of a component, ascending (wsis_segment_csr of d_comp); d_sat uint8 [C] = the saturated flags; d_active uint8
 * [E] = the edge's two arcs are active (cut).
 *
 * wsis_cp_arc_tails / wsis_cp_arcs: the arc pairs of API.h:959-974 (addDoubledge), as a CSR by tail node.  Arc a < E is
 * source[a] -> target[a], arc a + E its reverse; d_tails int64 [2E] = their tails; d_perm int32 [2E] = the arcs sorted by
 * tail, stable (the perm of wsis_segment_csr(d_tails)), whose offsets are the CSR's rows.  Per CSR position: d_arc_head,
 * d_arc_rev (the position of the opposite arc) and d_arc_edge (the input edge).  Repeated edges stay separate arcs. */
int wsis_cp_arc_tails(const int32_t* d_source, const int32_t* d_target, int64_t E, int64_t* d_tails, void* stream);
int64_t wsis_cp_arcs_workspace_bytes(int64_t E);
int wsis_cp_arcs(const int32_t* d_source, const int32_t* d_target, int64_t E, const int32_t* d_perm, int32_t* d_arc_head,
                 int32_t* d_arc_rev, int32_t* d_arc_edge, void* d_ws, int64_t ws_bytes, void* stream);
/* CutPursuit_L2.h init_labels: the 2-means of every unsaturated component with more than one node, one workgroup per
 * component, sums and energies in fp64.  Restart r of main iteration `iteration` draws from a hash of (seed, iteration, r,
 * smallest node of the component, draw): the first kernel is node (draw 0) % size of the component's ascending order, the
 * second the first node at which the running sum of squared distances to the first exceeds (draw 1) / 2^32 times their
 * total (node 0 if none).  kmeans_ite times: label = nearer to kernel 1 than to kernel 0, strictly; kernel 0 = mean of the
 * labelled nodes, kernel 1 = mean of the others (the reference's order); an empty class ends the iterations.  The restart
 * with the lowest energy (first among equals) gives d_label uint8 [V]; other nodes get 0. */
int64_t wsis_cp_kmeans_workspace_bytes(int64_t V);
int wsis_cp_kmeans(const float* d_features, int32_t D, const int32_t* d_comp_off, const int32_t* d_comp_nodes,
                   const uint8_t* d_sat, int64_t C, int64_t V, uint32_t seed, uint32_t iteration, int32_t restarts,
                   int32_t kmeans_ite, uint8_t* d_label, void* d_ws, int64_t ws_bytes, void* stream);
/* CutPursuit_L2.h compute_center and set_capacities: d_centres fp64 [C,2,D] = the means of the nodes with label 1 and
 * with label 0; a component with an empty class becomes saturated (d_sat is updated).  d_term fp64 [V] = cost_B -
 * cost_notB of set_capacities: > 0 is the capacity from the source, < 0 minus the capacity to the sink; 0 in saturated
 * components (the reference leaves their old capacities). */
int wsis_cp_capacities(const float* d_features, int32_t D, const int32_t* d_comp_off, const int32_t* d_comp_nodes, int64_t C,
                       int64_t V, const uint8_t* d_label, uint8_t* d_sat, double* d_centres, double* d_term, void* stream);
/* The integer capacities of one flow: d_src_cap / d_snk_cap int32 [V] from d_term, d_arc_cap int32 [2E] (CSR positions) =
 * lam * w of the arc's edge, 0 on active edges (d_active may be NULL), each rint(x / scale).  scale = 2^(e - 30) with the
 * largest capacity of the call in [2^(e-1), 2^e) (1 if all are 0): a capacity fits int32, the excess of 2^30 nodes int64;
 * integers come through exactly whenever scale <= 1.  d_scale2 fp64 [2]: [0] = scale, [1] = scratch. */
int wsis_cp_quantize(const double* d_term, int64_t V, const float* d_edge_weight, const uint8_t* d_active, int64_t E, double lam,
                     const int32_t* d_arc_edge, int32_t* d_src_cap, int32_t* d_snk_cap, int32_t* d_arc_cap, double* d_scale2,
                     void* stream);
/* boost::boykov_kolmogorov_max_flow of CutPursuit_L2.h split: the minimum cut by push-relabel with global relabelling,
 * first phase (a maximum preflow).  Node v has an arc from the source of d_src_cap[v] and one to the sink of
 * d_snk_cap[v]; d_arc_off int32 [V+1], d_arc_head / d_arc_rev / d_arc_cap int32 [A] as wsis_cp_arcs gives them (self loops
 * carry nothing).  d_sink_side uint8 [V] = 1 exactly where the sink is reachable in the residual graph -- the same set for
 * every maximum preflow; *d_cut int64 = the value of that cut.  Rounds of plain launches: a global relabel to the exact
 * residual distances, then a bounded number of push/relabel sweeps; *h_rounds (host) = rounds used.  max_rounds reached:
 * WSIS_ERR_OVERFLOW and no result. */
int64_t wsis_cp_min_cut_workspace_bytes(int64_t V, int64_t A);
int wsis_cp_min_cut(const int32_t* d_src_cap, const int32_t* d_snk_cap, const int32_t* d_arc_off, const int32_t* d_arc_head,
                    const int32_t* d_arc_rev, const int32_t* d_arc_cap, int64_t V, int64_t A, int32_t max_rounds,
                    uint8_t* d_sink_side, int64_t* d_cut, int32_t* h_rounds, void* d_ws, int64_t ws_bytes, void* stream);
/* CutPursuit.h activate_edges and compute_connected_components: an unsaturated component whose nodes share one label
 * becomes saturated (d_sat is updated); an edge whose ends differ in label becomes active; then the connected components
 * over inactive edges by hooking onto the smaller root and pointer jumping.  d_comp_new int32 [V]: ids 0..count-1 in order
 * of the components' smallest nodes; d_sat_new uint8 [V] (count entries used): the flag of the component each came from;
 * *d_count int32; *h_rounds (host) = hooking rounds. */
int64_t wsis_cp_activate_workspace_bytes(int64_t V);
int wsis_cp_activate(const int32_t* d_source, const int32_t* d_target, int64_t E, const uint8_t* d_label,
                     const int32_t* d_comp, const int32_t* d_comp_off, const int32_t* d_comp_nodes, int64_t C, int64_t V,
                     uint8_t* d_sat, uint8_t* d_active, int32_t* d_comp_new, uint8_t* d_sat_new, int32_t* d_count,
                     int32_t* h_rounds, void* d_ws, int64_t ws_bytes, void* stream);
/* CutPursuit.h compute_reduced_graph with CutPursuit_L2.h compute_value and compute_merge_gain.  wsis_cp_values: d_mean
 * fp64 [C,D] and d_weight fp64 [C] (the node count).  wsis_cp_border_keys: d_keys int64 [E] = min * C + max of the two
 * components of an edge, INT64_MAX inside a component.  wsis_cp_borders, over the keys sorted stably (d_order int64 = the
 * edges in that order, d_ukeys int64 [B] the distinct keys, d_border_off int64 [B+1] their rows): d_ba < d_bb int32 [B] the
 * two components, d_bw fp64 [B] the sum of w over the border's edges in edge order, d_gain fp64 [B] = compute_merge_gain
 * + lam * d_bw. */
int wsis_cp_values(const float* d_features, int32_t D, const int32_t* d_comp_off, const int32_t* d_comp_nodes, int64_t C,
                   double* d_mean, double* d_weight, void* stream);
int wsis_cp_border_keys(const int32_t* d_source, const int32_t* d_target, const int32_t* d_comp, int64_t E, int64_t C,
                        int64_t* d_keys, void* stream);
int wsis_cp_borders(const int64_t* d_ukeys, const int64_t* d_border_off, const int64_t* d_order, const float* d_edge_weight,
                    int64_t E, const double* d_mean, const double* d_weight, int32_t D, double lam, int64_t B, int64_t C,
                    int32_t* d_ba, int32_t* d_bb, double* d_bw, double* d_gain, void* stream);
/* CutPursuit.h merge: the greedy matching of the borders with gain > 0 by (gain descending, index ascending), each
 * component in one merge at the most, as rounds of borders that beat every live border at both ends.  d_taken uint8 [B];
 * d_map int32 [C]: the component a component joins (itself if none).  wsis_cp_relabel: the ids after the merges, still in
 * order of smallest node; a merged component is unsaturated; the edges of a merged border are inactive again. */
int64_t wsis_cp_merge_workspace_bytes(int64_t C);
int wsis_cp_merge(const int32_t* d_ba, const int32_t* d_bb, const double* d_gain, int64_t B, int64_t C, uint8_t* d_taken,
                  int32_t* d_map, int32_t* h_rounds, void* d_ws, int64_t ws_bytes, void* stream);
int64_t wsis_cp_relabel_workspace_bytes(int64_t C);
int wsis_cp_relabel(const int32_t* d_map, int64_t C, const int32_t* d_source, const int32_t* d_target, int64_t E,
                    const int32_t* d_comp, int64_t V, const uint8_t* d_sat, uint8_t* d_active, int32_t* d_comp_new,
                    uint8_t* d_sat_new, int32_t* d_count, void* d_ws, int64_t ws_bytes, void* stream);
/* CutPursuit_L2.h compute_energy from the components alone: d_out3 fp64 = {1/2 sum_v |f_v - mean|^2, lam * sum of w over the
 * edges between components, nodes in saturated components}. */
int64_t wsis_cp_energy_workspace_bytes(void);
int wsis_cp_energy(const float* d_features, int32_t D, const int32_t* d_comp, const double* d_mean, int64_t V, int64_t C,
                   const int32_t* d_source, const int32_t* d_target, const float* d_edge_weight, int64_t E, double lam,
                   const uint8_t* d_sat, double* d_out3, void* d_ws, int64_t ws_bytes, void* stream);

/* ---- ScanNet mesh superpoints: the data-parallel steps of segmentator.segment_mesh(vertices, faces)
 * [UPSTREAM ScanNet Segmentator], call sites data/ScanNetV2/prepare_data_inst_ScanNetV2.py:77 and :157 (csrc/meshseg.hip,
 * wsis_graph_prep.segment_mesh; the definition is restated there, the external binary is not on hand).
 * All arithmetic fp32, uncontracted, in the written order, division and square root correctly rounded: the outputs equal
 * tests/mesh_segment_ref.py bit for bit.  No floating-point atomics; two calls give the same bytes.  The sort by weight
 * (stable) lies between wsis_mesh_edge_weights and wsis_host_mesh_merge and is the caller's.
 *
 * wsis_mesh_face_normals (:77, step 1): one thread per face of d_faces int64 [F,3] over d_vertices fp32 [V,3]; d_fnormal
 * fp32 [F,3] = c / |c| of c = (p2 - p1) x (p3 - p1), 0 where |c| = 0.  d_keys int64 [3F]: d_keys[3 f + slot] = the vertex
 * of that slot -- wsis_segment_csr(d_keys, 3F, V) is the vertex -> face-slot CSR (stable: a row is in ascending face-slot
 * order).  d_err int32 [2] (zeroed here) = {face indices outside [0, V), non-finite vertex coordinates (all V vertices are
 * looked at, used or not)}.  An index outside [0, V) is read as vertex 0: with d_err[0] != 0 the outputs mean nothing.
 * V = 0 with F > 0 is refused. */
int wsis_mesh_face_normals(const float* d_vertices, int64_t V, const int64_t* d_faces, int64_t F, float* d_fnormal,
                           int64_t* d_keys, int32_t* d_err, void* stream);
/* (:77, step 2) d_vnormal fp32 [V,3]: the running mean n += (n_f - n) * (1 / (cnt + 1)) over the vertex's row of the CSR
 * d_perm int32 [3F] / d_offsets int32 [V+1], one lane per vertex (the recurrence is sequential); not re-normalised; a
 * vertex in no face keeps 0. */
int wsis_mesh_vertex_normals(const float* d_fnormal, const int32_t* d_perm, const int32_t* d_offsets, int64_t V, int64_t F,
                             float* d_vnormal, void* stream);
/* (:77, steps 3-4) one thread per edge: face f gives (i1,i2), (i1,i3), (i3,i2) at 3f, 3f+1, 3f+2 (repeated edges stay);
 * d_a / d_b int32 [3F], d_w fp32 [3F]: with d = (p_b - p_a) / |p_b - p_a| (0 if the length is 0), dot = n_a . n_b and
 * dot2 = n_b . d:  w = 1 - dot, squared if dot2 > 0. */
int wsis_mesh_edge_weights(const float* d_vertices, const float* d_vnormal, int64_t V, const int64_t* d_faces, int64_t F,
                           int32_t* d_a, int32_t* d_b, float* d_w, void* stream);

/* ---- evaluation counts: what evaluation/basic/ins_seg_evaluator.py:70-115 (assign_instances_for_scan),
 * evaluation/basic/instances.py:53-85 (VertInstance.get_instances), utils/eval_s3dis.py:42-112 and
 * evaluation/basic/sem_seg_evaluator.py:34-37 (fill_confusion) count per scene, called from test_scannetv2.py:133-143,
 * 212-275, test_s3dis.py:135-148, 216-292 and do_validation (train_scannetv2.py:296-400).  The reference forms one
 * `np.logical_and(gt_ids == id, pred_mask)` per (prediction, ground-truth instance); here the masks are read once.
 * Integer counting only: exact, independent of the order of arrival, no floating point.
 *
 * wsis_mask_overlap: d_mask row-major [P, N] of elem_bytes = 1 (bool / uint8) or 8 (int64) per element; an element is a
 * member iff ANY of its bits is set (np.not_equal(mask, 0)).  d_col int32 [N] in [0, G), anything else (negative): the
 * point counts in d_rows only.  d_table int64 [P, G]: T[p, u] = #{i : mask[p, i] != 0 and col[i] == u}; d_rows int64 [P]
 * = #{i : mask[p, i] != 0} (instance_count).  Both are zeroed by the call.  P, N >= 0, 1 <= G <= 4096; P == 0 or N == 0
 * writes zeros without a launch.  A workgroup owns wsis_mask_overlap_chunk() points and wsis_mask_overlap_tile_rows(G)
 * rows (-1 for G outside the domain), whose counters sit in LDS.  The workspace query returns -1 outside the domain and 0
 * inside it: this form needs no workspace, d_ws may be NULL. */
int32_t wsis_mask_overlap_chunk(void);
int32_t wsis_mask_overlap_tile_rows(int32_t G);
int64_t wsis_mask_overlap_workspace_bytes(int64_t P, int64_t N, int32_t G);
int wsis_mask_overlap(const void* d_mask, int32_t elem_bytes, int64_t P, int64_t N, const int32_t* d_col, int32_t G,
                      int64_t* d_table, int64_t* d_rows, void* d_ws, int64_t ws_bytes, void* stream);
/* np.add.at(table, (a, b), 1) of sem_seg_evaluator.py:37, and the (instance, class) histogram behind
 * stats.mode(sem_gt[ins_gt == id]) of utils/eval_s3dis.py:43-46: d_table int64 [A, B], zeroed by the call, counts (a_i, b_i)
 * for every i with 0 <= a_i < A and 0 <= b_i < B; other points are skipped.  A, B >= 1, A * B <= 65536. */
int wsis_label_pairs(const int32_t* d_a, const int32_t* d_b, int64_t N, int32_t A, int32_t B, int64_t* d_table,
                     void* stream);

/* ---- a18 (point-level part): semantic loss of MultiTaskLoss.forward (losses_3D_WSIS.py:52-67 of the reference):
 * CrossEntropyLoss(ignore_index) + mean_c(1 - dice_c) with dice_c = (2 sum p_c y_c + 1e-5) / (sum p_c^2 + sum y_c
 * + 1e-4 + 1e-5) over the rows whose label != ignore_label, p = softmax(scores).  d_scores fp32 [N,C] (C <= 32),
 * d_labels int64 [N].  fwd: d_out2[0] = loss, d_out2[1] = number of kept rows; d_saved fp32 [2C+1] feeds bwd.
 * bwd: d_dscores [N,C] = *d_grad_loss * dloss/dscores (zero rows for ignored labels).  Deterministic. */
int64_t wsis_semantic_loss_workspace_bytes(int64_t N);
int wsis_semantic_loss_fwd(const float* d_scores, const int64_t* d_labels, int64_t N, int32_t C, int64_t ignore_label,
                           float* d_out2, float* d_saved, void* d_ws, int64_t ws_bytes, void* stream);
int wsis_semantic_loss_bwd(const float* d_scores, const int64_t* d_labels, int64_t N, int32_t C, int64_t ignore_label,
                           const float* d_saved, const float* d_grad_loss, float* d_dscores, void* stream);

/* Superpoint semantic term (losses_3D_WSIS.py:72-74: CrossEntropyLoss(ignore_index) on the [S,C] superpoint scores, mean
 * over the kept rows) with the logged scores.sum(): d_out3 = {loss, sum of all scores, n_kept}; one launch each way (the
 * forward finishes its workgroup sums by a ticket in the caller's sync slot, d_sync: see wsis_sync_bytes; S >= 1, C <= 32).
 * wsis_loss_sum: out = t_0 + t_1 + ... in order (the weighted sum of losses_3D_WSIS.py:130-151, all weights 1); bit i of
 * `paired` adds term i to term i+1 first (the reference's `offset_norm_loss + offset_dir_loss`).  d_terms is a HOST array
 * of n <= 8 device scalars. */
int64_t wsis_sp_ce_loss_workspace_bytes(int64_t S);
int wsis_sp_ce_loss_fwd(const float* d_scores, const int64_t* d_labels, int64_t S, int32_t C, int64_t ignore_label,
                        float* d_out3, void* d_ws, int64_t ws_bytes, void* d_sync, void* stream);
int wsis_sp_ce_loss_bwd(const float* d_scores, const int64_t* d_labels, int64_t S, int32_t C, int64_t ignore_label,
                        const float* d_out3, const float* d_grad_loss, float* d_dscores, void* stream);
int wsis_loss_sum(const float* const* d_terms, int32_t n, uint32_t paired, float* d_out, void* stream);

/* Superpoint regression terms of the same loss (losses_3D_WSIS.py:79-96 offset L1 + cosine, :113-127 occupancy and
 * instance-size L1) over the rows whose two labels both differ from ignore_label: d_out5 = {offset_norm, offset_dir,
 * occupancy, instance_size, n_valid}.  bwd: gradients of the three predictions from four upstream scalars. */
int wsis_sp_regression_loss_fwd(const float* d_pred_off, const float* d_gt_off, const float* d_pred_occ,
                                const float* d_gt_occ, const float* d_pred_size, const float* d_gt_size,
                                const int64_t* d_sem_label, const int64_t* d_ins_label, int64_t S,
                                int64_t ignore_label, float* d_out5, void* stream);
int wsis_sp_regression_loss_bwd(const float* d_pred_off, const float* d_gt_off, const float* d_pred_occ,
                                const float* d_gt_occ, const float* d_pred_size, const float* d_gt_size,
                                const int64_t* d_sem_label, const int64_t* d_ins_label, int64_t S,
                                int64_t ignore_label, const float* d_out5, const float* d_g_norm,
                                const float* d_g_dir, const float* d_g_occ, const float* d_g_size, float* d_doff,
                                float* d_docc, float* d_dsize, void* stream);

/* Discriminative loss of one scene's superpoint embeddings (losses_3D_WSIS.py:157-230: pull delta_v, push on the L1
 * distance of the instance means with delta_d, regularisation), instances in n_slots <= 64 slots (slot = instance id;
 * the bound is known on the host), S <= 1536 rows, D = 7.  Rows count when both labels differ from ignore_label.
 * d_saved: wsis_disc_loss_saved_floats() floats, feeds bwd.  One workgroup, deterministic. */
int32_t wsis_disc_loss_saved_floats(void);
int wsis_disc_loss_fwd(const float* d_x, const int64_t* d_ins_label, const int64_t* d_sem_label, int64_t S,
                       int32_t D, int32_t n_slots, int64_t ignore_label, float delta_v, float delta_d, float p_var,
                       float p_dist, float p_reg, float* d_out1, float* d_saved, void* stream);
int wsis_disc_loss_bwd(const float* d_x, const int64_t* d_ins_label, const int64_t* d_sem_label, int64_t S,
                       int32_t D, int32_t n_slots, int64_t ignore_label, float delta_v, float delta_d, float p_var,
                       float p_dist, float p_reg, const float* d_saved, const float* d_grad_loss, float* d_dx,
                       void* stream);

/* ---- optimizer step (train_scannetv2.py:251; AdamW of config/ScanNet_v2_3D_WSIS.yaml:58-61) in one launch.
 * d_segments: device array of {float* p; const float* g; float* m; float* v; int64_t n; float step_size;
 * float inv_sqrt_bc2; float g_clamp; int32_t group;} (wsis_adamw_segment_bytes() bytes each; n == 0 skips the parameter;
 * g_clamp > 0 clamps the gradient to [-g_clamp, g_clamp] first and writes it back: train_scannetv2.py:247-249; step_size =
 * lr / (1 - beta1^t), inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t) with t = updates of that parameter so far, this one
 * included); d_blocks int32 [n_blocks,2] = (segment, chunk of wsis_adamw_chunk() elements) for every chunk of every
 * segment.  Update rule of torch.optim.AdamW (decoupled weight decay), fp32.  `group` is read by the *_groups entry
 * points below only. */
int32_t wsis_adamw_segment_bytes(void);
int32_t wsis_adamw_chunk(void);
int wsis_adamw_step(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks, double lr, double beta1,
                    double beta2, double eps, double weight_decay, void* stream);

/* ---- dynamic loss scaling for fp16 training, state on the device.  Replaces torch.amp.GradScaler around the step:
 * unscale_ (a Python walk over every gradient and multi-tensor foreach launches), found_inf.item() (a device->host
 * read on every step) and the host's decision whether optimizer.step() runs -- here three launches and no read-back.
 * All three take the segment and block tables of the optimizer step above.
 *
 * grad_nonfinite: reads the gradients only; any +-inf or NaN element stores 1.0f to *d_found_inf.  Never stores 0.
 *
 * adamw_step_scaled: d_grad_scale, d_found_inf: fp32 [1] on the device, either may be NULL (scale 1 / never skipped);
 * d_skipped: int32 [n_segments], zero-filled by the caller once.  *d_found_inf != 0: no parameter, moment or gradient
 * byte is written and d_skipped[s] += 1 for every segment with n > 0.  Otherwise the gradient is g * inv with
 * inv = (float)(1.0 / (double)scale) (torch's unscale_ rounding; exact for a power of two); a segment with g_clamp > 0
 * clamps THAT value and writes it back, a segment without does not write its gradient: its .grad still holds the
 * scaled values after the step.  For this entry point the 8 bytes of (step_size, inv_sqrt_bc2) hold int64 t_host, the
 * updates the host has issued for the parameter (skipped ones included); the kernel forms t = t_host - d_skipped[s]
 * and both corrections from lr, beta1, beta2 in double, rounded once.
 *
 * loss_scale_update: torch._amp_update_scale_ (overflow: scale *= backoff, tracker = 0; else tracker + 1 and at
 * growth_interval scale *= growth if that is finite, tracker = 0), then *d_found_inf = 0 for the next step. */
int wsis_grad_nonfinite(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks, float* d_found_inf,
                        void* stream);
int wsis_adamw_step_scaled(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks, double lr, double beta1,
                           double beta2, double eps, double weight_decay, const float* d_grad_scale,
                           const float* d_found_inf, int32_t* d_skipped, void* stream);
int wsis_loss_scale_update(float* d_scale, int32_t* d_growth_tracker, float* d_found_inf, double growth_factor,
                           double backoff_factor, int32_t growth_interval, void* stream);

/* ---- several parameter groups in the step's one launch.  Replaces torch.optim.AdamW built with more than one
 * parameter group around train_scannetv2.py:93-94,251 (no weight decay on norm parameters and biases, a lower learning
 * rate for the pre-trained UNet, a fix_module part added between stages): torch steps group by group, six launches each.
 * d_groups: device array of n_groups rows {double lr, beta1, beta2, eps, weight_decay} (wsis_adamw_group_bytes() = 40
 * bytes each), what wsis_adamw_step / wsis_adamw_step_scaled take as arguments; the kernel rounds
 * (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)eps, (float)(1.0 - beta2) per group as
 * those entry points do on the host, so one group row gives their bytes.  `group` of a segment (int32, the last 4 of
 * its 56 bytes) names its row; the caller guarantees 0 <= group < n_groups.  step_groups: step_size and inv_sqrt_bc2 of
 * a segment are the caller's, from its group's lr and betas.  step_scaled_groups: the corrections come from the group
 * row's lr, beta1, beta2 and t = t_host - d_skipped[s]; *d_found_inf != 0 skips EVERY group: no parameter, moment or
 * gradient byte is written and d_skipped[s] += 1 for every segment with n > 0.  wsis_grad_nonfinite serves both. */
int32_t wsis_adamw_group_bytes(void);
int wsis_adamw_step_groups(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks, const void* d_groups,
                           int32_t n_groups, void* stream);
int wsis_adamw_step_scaled_groups(const void* d_segments, const int32_t* d_blocks, int64_t n_blocks,
                                  const void* d_groups, int32_t n_groups, const float* d_grad_scale,
                                  const float* d_found_inf, int32_t* d_skipped, void* stream);

/* ---- op-list executor: one C call issues a recorded forward or backward pass of the sparse UNet ------------
 * Replaces the Python-dispatched module walk of sparse_unet3d.py:103-350 (ResidualBlock.forward / UBlock.forward
 * and their autograd backward): the host records the pass as wsis_op records (plain device pointers + sizes) and
 * wsis_run_ops launches every kernel on `stream`.  Each op is exactly one of the single-op entry points above
 * (same kernels and summation orders -> bit-identical to calling them one by one):
 *   CONV         in: X, nbr, order, W, bias, residual          out: Y                      (wsis_spconv_fwd)
 *   BN_RELU      in: x, gamma, beta, running_mean, running_var out: y, mean, var           (wsis_bn_stats+apply)
 *   CAT          in: a [M,Cin], b [M,Cout]                     out: [M,Cin+Cout]           (torch.cat dim 1)
 *   SPLIT        in: [M,Cin+Cout]                              out: a [M,Cin], b [M,Cout]  (its backward)
 *   ADD          in: src [M_in*Cin]                            out: dst += src             (gradient fan-in)
 *   CONV_BWD     in: X, W, dY, nbr_f, order_f, nbr_b, order_b  out: dX (may be NULL), dW (may be NULL)
 *                M_in = rows of X / dX, M_out = rows of dY     (weight_transpose + wsis_spconv_fwd + wsis_spconv_dw)
 *   BN_RELU_BWD  in: x, dy, mean, var, gamma, beta, addend     out: dx, dgamma, dbeta      (wsis_bn_bwd)
 *   CAST_LP      in: x fp32 [M_in, Cin]                        out: y 16-bit [M_in, Cin]   (round to nearest even)
 * The 16-bit forms of CONV, BN_RELU, CAT, SPLIT, CONV_BWD and BN_RELU_BWD (WSIS_OPF_LP) are listed below the op kinds.
 * BN ops use M_in rows and Cin channels.  d_ws from wsis_run_ops_workspace_bytes (max over the ops); d_sync: a
 * zero-filled block of wsis_sync_bytes() bytes (may be NULL: multi-launch forms).
 * Streams: everything the caller's later work depends on is ordered on `stream` when the call returns.  Work that the
 * chain of ops does not wait for runs on a library-owned side stream of `stream`, forked and joined with events inside
 * the call: the weight gradients of CONV_BWD ops (WSIS_DW_STREAM=0: on `stream`; forked in FRONT of their op's dIn launch
 * below WSIS_DW_EARLY_ROWS active voxels per batch -- they need X and dY, not dX; the weight gradient of a pass's last op
 * goes on `stream` itself, WSIS_DW_TAIL_MAIN) and the pass's weight transposes (WSIS_WT_SIDE; joined in front of the
 * first op that reads one).  Same kernels on either stream: the results do not depend on these switches. */
enum {
  WSIS_OP_CONV = 1, WSIS_OP_BN_RELU = 2, WSIS_OP_CAT = 3, WSIS_OP_SPLIT = 4, WSIS_OP_ADD = 5, WSIS_OP_CONV_BWD = 6,
  WSIS_OP_BN_RELU_BWD = 7, WSIS_OP_CAST_LP = 8
};
/* WSIS_OPF_STATS on CONV: out[1] = BatchNorm partials of the output (wsis_spconv_fwd_t d_stats).
 * WSIS_OPF_STATS on BN_RELU (training): the statistics come from partials instead of a pass over x: in[5] = partials
 * of channels [0, K), in[6] = partials of channels [K, Cin) (NULL when K == Cin; the input is a concatenation of two
 * producers' outputs), ceil(M_in / 32) rows each. */
/* WSIS_OPF_BN_IN on CONV: the input is BatchNorm(+ReLU, WSIS_OPF_RELU)(in[0]) applied on the fly (wsis_spconv_fwd_f):
 * in[6] = mean, in[7] = var, in[8] = gamma, in[9] = beta, eps = op.eps -- the BN_RELU op in front of it is then not in the
 * list at all (or only computes statistics: BN_RELU with out[0] == NULL).  On CONV_BWD: in[0] is that raw tensor and
 * in[7..10] = mean, var, gamma, beta: the weight gradient runs as wsis_spconv_dw_bn.
 * WSIS_OPF_STAT_FIN on CONV (with WSIS_OPF_STATS): the statistics of the output are finished inside the launch for
 * n = 1 or 2 BatchNorm layers: target 0 = out[2] mean, out[3] var, in[10] running_mean, in[11] running_var, op.momentum;
 * target 1 (when out[4] != NULL) = out[4], out[5], out[6], out[7], op.momentum2. */
/* WSIS_OPF_LP: a 16-bit op of an inference or training pass; op.reserved = dtype (0 = bf16, 1 = fp16).  Every form is
 * exactly one single-op entry point (or a fixed sequence of them), so a pass is bit-identical to calling them one by one.
 * WSIS_OPF_LP_TRAIN (with WSIS_OPF_LP): the op belongs to a 16-bit TRAINING pass.  The forms that only such a pass has --
 * BN_RELU with WSIS_OPF_TRAINING, BN_RELU_BWD, CONV_BWD, SPLIT -- need it; without it they are refused, so an inference
 * list that holds one of them by mistake still fails before anything is launched.  The other flagged ops may carry it.
 *   CONV         wsis_spconv_fwd_lp_res: X, residual (in[5]) and Y in 16 bits.  The 16-bit B^T weights are cast from the
 *                fp32 in[3] inside the same call (wsis_weight_cast_lp, transpose = 1; slice K-1-k with WSIS_OPF_FLIP) into
 *                the call's workspace, so the pass follows every optimizer step.  Shape inside wsis_spconv_lp_supported.
 *   BN_RELU      16-bit x; y in 16 bits, or fp32 with WSIS_OPF_OUT_F32.  Evaluation form (running statistics in[3], in[4]):
 *                wsis_bn_apply_lp.  With WSIS_OPF_TRAINING (and WSIS_OPF_UPDATE_RUNNING; LP_TRAIN): wsis_bn_stats_lp into out[1] /
 *                out[2] (fp32), then wsis_bn_apply_lp with them; Cin % 8 == 0.
 *   BN_RELU_BWD  (LP_TRAIN) wsis_bn_bwd_lp: x, dy, addend in 16 bits, dgamma / dbeta fp32, dx in 16 bits or fp32 with WSIS_OPF_OUT_F32.
 *   CONV_BWD     (LP_TRAIN) X and dY in 16 bits.  dX (out[0], may be NULL) = wsis_spconv_fwd_lp of dY through nbr_b / order_b with the
 *                weight cast inside the call (wsis_weight_cast_lp, transpose = 0, no flip; the product takes slice K-1-k
 *                with WSIS_OPF_FLIP -- the sequence of spconv.ops._backward_lp); dW (out[1], may be NULL) =
 *                wsis_spconv_dw_lp straight into the fp32 gradient.  Both products inside wsis_spconv_lp_supported, dY below
 *                2 GiB.  The weight gradients take the same side-stream fork / join plan as the fp32 ones.
 *   CAT, SPLIT   the fp32 ops with Cin / 2 and Cout / 2 (both even): they copy 4-byte words (SPLIT: LP_TRAIN).
 *   CAST_LP      carries the flag too (its dtype).
 * A flagged op the executor cannot run (a training form without WSIS_OPF_LP_TRAIN; WSIS_OPF_STATS, WSIS_OPF_BN_IN or
 * WSIS_OPF_STAT_FIN on a flagged op; a shape outside the 16-bit domain; ADD) fails the call with WSIS_ERR_ARG before
 * anything is launched.  Lists without the flag run as before. */
enum {
  WSIS_OPF_RELU = 1, WSIS_OPF_TRAINING = 2, WSIS_OPF_UPDATE_RUNNING = 4, WSIS_OPF_FLIP = 8, WSIS_OPF_STATS = 16,
  WSIS_OPF_BN_IN = 32, WSIS_OPF_STAT_FIN = 64, WSIS_OPF_LP = 128, WSIS_OPF_OUT_F32 = 256, WSIS_OPF_LP_TRAIN = 512
};
typedef struct wsis_op {
  int32_t kind, flags;
  int64_t M_in, M_out;
  int32_t K, Cin, Cout, reserved;
  float eps, momentum;
  float momentum2, reserved2;
  const void* in[12];
  void* out[8];
} wsis_op;
int64_t wsis_run_ops_workspace_bytes(const wsis_op* ops, int32_t n);
int wsis_run_ops(const wsis_op* ops, int32_t n, void* d_ws, int64_t ws_bytes, void* d_sync, void* stream);
/* The same with a milestone: once op `mark_op` (0-based) has been issued, `waiter_stream` is made to wait for
 * everything issued so far on `stream` and on the library's weight-gradient side stream.  The data-parallel step uses
 * it to start the RCCL all-reduce of the finished first part of the flat gradient buffer while the rest of the backward
 * pass still runs (the reference's DDP buckets, train_scannetv2.py:738).  mark_op < 0: no milestone. */
int wsis_run_ops_marked(const wsis_op* ops, int32_t n, void* d_ws, int64_t ws_bytes, void* d_sync, void* stream,
                        int32_t mark_op, void* waiter_stream);
/* Creates the library's weight-gradient side stream of `stream` and binds both to their hardware queues (first command).
 * Call before creating an RCCL communicator in the same process (wsis_parallel.warm_streams does): streams take their
 * hardware queue in the order of their first use, and two streams of a step must not end up sharing one. */
int wsis_warm_streams(void* stream);
/* Launch-plan hint for the weight-gradient products (wsis_spconv_dw, wsis_spconv_dw_bn, the backward ops of wsis_run_ops):
 * `rows` = active voxels of the finest level of the batch being trained (train_scannetv2.py:191: the rows of the
 * SparseConvTensor the UNet receives).  From 250,000 rows (two ScanNet scenes per step) the launches take twice the
 * waves at every level: with several scenes per step the GPU is busy throughout and the gradients should get done
 * fast; with one scene they should stay out of the way of the dIn products.  0 (initial) = no hint.
 * Performance only -- results stay within the same tolerance, but the slab partition and with it the order of additions
 * of a weight gradient follow the plan: give the same hint to runs whose bits are compared.
 * PROCESS-GLOBAL and sticky: one word shared by every device, stream and the library's weight-gradient worker thread;
 * it keeps its value until the next call (the Python layer sets it at the top of every forward pass).  A caller of
 * wsis_spconv_dw / wsis_spconv_dw_bn that never calls this runs with the hint of whatever batch the process saw last. */
int wsis_hint_batch_rows(int64_t rows);
/* A pass issued in PARTS -- the host does something between two parts (the statistics exchange of a SyncBatchNorm layer:
 * train_scannetv2.py:734-736 converts every BatchNorm when num_gpus > 1; model/unet_native.py).  Parts with last == 0
 * leave the weight-gradient side stream un-joined; the part with last != 0 (n may be 0) joins everything forked since.
 * Every part needs its OWN workspace (wsis_run_ops_workspace_bytes of that part), alive until the last part returns. */
int wsis_run_ops_part(const wsis_op* ops, int32_t n, void* d_ws, int64_t ws_bytes, void* d_sync, void* stream,
                      int32_t last);

#if defined(WSIS_EXPERIMENTAL) && WSIS_EXPERIMENTAL
/* A run of consecutive ops whose output tensors have at most WSIS_DEEP_ROWS (8192) rows -- the deep UNet levels of a
 * scene, sparse_unet3d.py:321-350 -- is issued as ONE resident launch (csrc/deep.hip: 256 workgroups walk the ops as
 * phases with grid barriers between them; same kernels' code, same order of additions, results identical to the
 * launch-by-launch form).  WSIS_DEEP=0 switches it off.  Counters of this process, for tests: */
int64_t wsis_deep_launches(void);
int64_t wsis_deep_phases(void);
#endif /* WSIS_EXPERIMENTAL */
/* 1: this library was built with EXPERIMENTAL=1 (the guarded entry points above exist), 0: the default build */
int32_t wsis_experimental(void);
#ifdef __cplusplus
}
#endif
#endif /* WSIS_HIP_H_ */
