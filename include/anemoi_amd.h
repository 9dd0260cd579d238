/*
 * anemoi_amd.h -- C ABI of the MI355X (gfx950) forward-path kernels.
 *
 * Drop-in boundary for the encoder -> processor -> decoder forward path of
 * ecmwf/anemoi-models.  The reference has no FFI of its own: the boundary there
 * is the set of nn.Module.forward methods in anemoi/models/layers (SURVEY.md
 * section 8b).  Each entry point below replaces the ATen / torch_geometric op
 * sequence of one such method; the citation names the reference lines it
 * replaces (paths relative to /root/reference/src/anemoi/models).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     stated otherwise; `stream` is a hipStream_t passed as void*.
 *   - node / edge feature matrices are row-major with an explicit leading
 *     dimension (in elements), so slices of wider buffers can be passed.
 *   - `dtype` selects the storage type of activations and GEMM weights:
 *     ANEMOI_F32 (exact f32 MFMA / f32 math) or ANEMOI_BF16 (bf16 storage,
 *     f32 accumulate).  Biases, LayerNorm affine parameters, edge attributes and
 *     the lin_edge weights are always f32.
 *   - every function returns ANEMOI_OK (0) or an error code; the message of the
 *     last error on the calling thread is available from anemoi_last_error().
 *     Nothing is allocated, no global state is kept, all launches go to `stream`.
 */
#ifndef ANEMOI_AMD_H
#define ANEMOI_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANEMOI_OK 0
#define ANEMOI_ERR_INVALID 1     /* bad argument; Python shim raises ValueError        */
#define ANEMOI_ERR_UNSUPPORTED 2 /* unsupported shape/dtype; shim raises NotImplementedError */
#define ANEMOI_ERR_LAUNCH 3      /* HIP launch failure; shim raises RuntimeError          */

#define ANEMOI_F32 0
#define ANEMOI_BF16 1
#define ANEMOI_I32 2 /* launch-trail records only (anemoi_trail_note): no kernel computes in these */
#define ANEMOI_U8 3

#define ANEMOI_ACT_NONE 0
#define ANEMOI_ACT_GELU 1 /* exact erf form, nn.GELU() default */
#define ANEMOI_ACT_SILU 2
#define ANEMOI_ACT_RELU 3

typedef void* anemoi_stream_t; /* hipStream_t */

/* ABI version (bumped on any signature change) and last error text of this thread. */
int anemoi_abi_version(void);
/* Target architecture and the hipcc / clang the library was built with (static string).  The inline-asm kernels carry
 * hand-counted wait states hipcc does not check; a report of wrong results should quote this line. */
const char* anemoi_build_info(void);
const char* anemoi_last_error(void);

/*
 * LayerNorm over the last dimension: y[r,:] = (x[r,:] - mean_r) * rstd_r * gamma + beta.
 * Replaces nn.LayerNorm calls layers/block.py:614 (layer_norm1), :491-494 (layer_norm1/2 of the
 * mapper block), node_dst_mlp[0] :349-351, node_data_extractor[0] layers/mapper.py:408-410.
 * Statistics in f32 (two-pass, biased variance, eps inside the sqrt) as ATen does.
 */
int anemoi_layer_norm(int dtype, const void* x, int64_t ldx, const float* gamma, const float* beta, void* y,
                      int64_t ldy, int64_t rows, int C, float eps, anemoi_stream_t stream);

/* y = LayerNorm(x) + residual in one pass (each term rounded to the activation dtype first, as the two separate
 * operations of the reference round: the trailing LayerNorm of layers/mlp.py:74-84 followed by "+ x" / "+ edge_attr" in
 * layers/block.py:222, layers/conv.py:70). */
int anemoi_layer_norm_residual(int dtype, const void* x, int64_t ldx, const float* gamma, const float* beta,
                               const void* residual, int64_t ldr, void* y, int64_t ldy, int64_t rows, int C, float eps,
                               anemoi_stream_t stream);

/* The same, and stats[r] = { rstd_r, -mean_r * rstd_r } (f32 pairs, as anemoi_row_stats leaves them) out of the same pass:
 * the training forward keeps them for anemoi_layer_norm_backward instead of reading x a second time. */
int anemoi_layer_norm_stats(int dtype, const void* x, int64_t ldx, const float* gamma, const float* beta, void* y,
                            int64_t ldy, float* stats, int64_t rows, int C, float eps, anemoi_stream_t stream);

/*
 * Fused Linear: y = act(x @ W^T + bias) + residual, on MFMA.
 *   x [M, K] (ldx), W [N, K] row-major contiguous in `dtype` (nn.Linear layout), bias [N] f32 or NULL,
 *   residual [M, N] (ldr) in `dtype` or NULL, y [M, N] (ldy) in `out_dtype`.
 * K must be a multiple of 32 (the host pads the K dimension of x and W with zeros).
 * Replaces the nn.Linear calls layers/block.py:615-618 (lin_self/query/key/value as ONE GEMM over the
 * concatenated weight), :630 (projection, + x_skip :632 as residual), node_dst_mlp[1..3] :633
 * (GELU and the "+ out" residual fused), layers/mapper.py:112-113,416 (emb_nodes_*), :100
 * (node_data_extractor[1]), layers/attention.py:68,110 and the MLPs of layers/mlp.py:74-84.
 */
int anemoi_linear(int dtype, int out_dtype, const void* x, int64_t ldx, const void* w, const float* bias,
                  const void* residual, int64_t ldr, void* y, int64_t ldy, int64_t M, int N, int K, int act,
                  anemoi_stream_t stream);

/*
 * LayerNorm statistics of the rows of x [rows, C] (ldx): stats[r] = { rstd_r, -mean_r * rstd_r } (f32 pairs, same
 * two-pass arithmetic as anemoi_layer_norm).  First half of a LayerNorm -> Linear pair (next entry point).
 */
int anemoi_row_stats(int dtype, const void* x, int64_t ldx, float* stats, int64_t rows, int C, float eps,
                     anemoi_stream_t stream);

/*
 * Linear with the LayerNorm of its input folded in:  y = act(LN(x) @ W^T + b) + residual  computed as
 *   y[m,n] = act( rstd_m * (x @ W'^T)[m,n] + (-mean_m rstd_m) * colsum[n] + bias[n] ) + residual[m,n]
 * where the caller passes  W' = W * gamma (input columns scaled by the LayerNorm weight, in `dtype`),
 * colsum[n] = sum_k W'[n,k] (f32, from the rounded W'), bias = b + W beta (f32) and stats from anemoi_row_stats(x).
 * x is the UN-normalised input: the normalised activation is never written to memory.  Replaces the pairs
 * layer_norm1 -> lin_query/key/value/self (layers/block.py:614-618, :491-497), node_dst_mlp[0] -> node_dst_mlp[1]
 * (:349-351) and layer_norm -> lin_qkv / mlp[0] of the transformer block (:99-105).  Same shapes / alignment as
 * anemoi_linear; colsum 16-byte aligned for the fast path.
 */
int anemoi_linear_ln(int dtype, int out_dtype, const void* x, int64_t ldx, const void* w, const float* bias,
                     const float* colsum, const float* stats, const void* residual, int64_t ldr, void* y, int64_t ldy,
                     int64_t M, int N, int K, int act, anemoi_stream_t stream);

/*
 * anemoi_linear_ln / anemoi_linear without activation, plus the LayerNorm statistics of the RESULT's rows
 * (stats_out [M, 2] f32 = { rstd, -mean * rstd } of y[m, 0:N], the format of anemoi_row_stats) for the LayerNorm that
 * consumes y next (reference layers/block.py:631-633 node_dst_mlp[0], :614 layer_norm1 of the next block,
 * layers/mapper.py:416 node_data_extractor[0]): on the bf16 fast path the GEMM's epilogue leaves per-row partial sums of
 * the bf16 values it stores in `workspace` (>= M * (N / 128) * 8 bytes, 8-byte aligned; N % 256 == 0) and a tiny kernel
 * folds them -- y is not read again.  Other shapes / dtypes (or workspace == NULL): same result through
 * anemoi_row_stats on y.  colsum / stats_in: both NULL = plain Linear, both set = LayerNorm-folded input as in
 * anemoi_linear_ln.  x, y, residual in `dtype`.
 */
int anemoi_linear_stats(int dtype, const void* x, int64_t ldx, const void* w, const float* bias, const float* colsum,
                        const float* stats_in, const void* residual, int64_t ldr, void* y, int64_t ldy, int64_t M, int N,
                        int K, void* workspace, int64_t workspace_bytes, float eps, float* stats_out,
                        anemoi_stream_t stream);

/*
 * Edge attributes in CSR (destination-sorted) order:
 *   out[e, :] = [ a0[perm[e] % rows0, 0:d0] | a1[perm[e] % rows0, 0:d1] | 0 ... ]   (row stride ld_out)
 * and, when one_col >= 0, out[e, one_col] = 1 (the constant attribute that carries the lin_edge bias through the
 * folded kernel below).  `perm[e]` is the original (batched) edge id of CSR slot e.  Replaces TrainableTensor.forward
 * (layers/graph.py:37-44: repeat over the batch + concat of the trainable tensor) composed with the edge
 * gather that torch_geometric's propagate performs per block.  a1 may be NULL (d1 = 0).
 */
int anemoi_edge_attr_csr(const float* a0, int d0, const float* a1, int d1, int64_t rows0, const int32_t* perm,
                         float* out, int ld_out, int one_col, int64_t n_edges, anemoi_stream_t stream);

/*
 * Fused GraphTransformer edge phase for all destinations (K1 + K2 of SURVEY.md section 2a):
 *   e_ij   = W_e a_ij + b_e                                        (lin_edge, layers/block.py:499,620)
 *   s_ij,h = q_i,h . (k_j,h + e_ij,h) / sqrt(D)                    (layers/conv.py:134-137)
 *   alpha  = exp(s - max_i) / (sum_i exp(s - max_i) + 1e-16)       (PyG softmax, layers/conv.py:139)
 *   out_i  = sum_j alpha_ij,h (v_j,h + e_ij,h)  [+ x_r_i]          (layers/conv.py:142 + scatter-sum;
 *                                                                   "+ x_r" of layers/block.py:531,630)
 * Graph given as CSR by destination: rowptr [n_dst+1], col [E] (source index), edge_attr [E, ea_ld] f32 in
 * CSR order.  Edges of one destination are accumulated in CSR order (= original edge order when the CSR is a
 * stable sort), destinations without edges give out_i = 0 (+ x_r_i).  One pass, no atomics, no [E, C]
 * temporaries.  q/k/v/x_r/out are [*, C] slices with leading dimensions; H heads of D = C/H channels.
 */
int anemoi_gt_edge_attention(int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                             const void* x_r, int64_t ldr, const float* edge_attr, int ea_ld, int edge_dim,
                             const float* w_edge, const float* b_edge, const int32_t* rowptr, const int32_t* col,
                             void* out, int64_t ldo, int64_t n_dst, int C, int H, anemoi_stream_t stream);

/*
 * The same edge phase with lin_edge folded into the neighbouring GEMMs (the fast path used by the block mirrors).
 * lin_edge is linear, so with W_e' = [W_e | b_e], a'_ij = [a_ij | 1] and per head h:
 *   q_i,h . e_ij,h       = u_i,h . a'_ij      with u_i,h = W_h'^T q_i,h  -> H*up extra OUTPUT columns of the q/k/v GEMM
 *   sum_j alpha e_ij,h   = W_h' t_i,h         with t_i,h = sum_j alpha a'_ij -> H*up extra INPUT columns of `projection`
 * The kernel therefore never touches W_e:  u [n_dst, H, up] (ldu) is read next to q, edge_attr is [E, up] f32 in CSR
 * order with a constant 1 in column edge_dim, and out (ldo >= C + H*up) receives
 *   out[:, 0:C] = sum_j alpha_ij v_j (+ x_r)      out[:, C:C+H*up] = t_i,h      (alpha as defined above, incl. 1e-16).
 * up is 4, 8, 12 or 16; D = C/H must be a multiple of the 16-byte vector width with D/vec a power of two <= 16.
 * lse (optional, f32 [n_dst, H]): the softmax normaliser max + log(sum exp + 1e-16) per destination and head, i.e.
 * alpha_ij = exp(s_ij - lse_i); what the backward needs to rebuild alpha in one sweep.  NULL: not written.
 */
int anemoi_gt_edge_attention_folded(int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                    const void* x_r, int64_t ldr, const void* u, int64_t ldu, const float* edge_attr,
                                    int up, const int32_t* rowptr, const int32_t* col, void* out, int64_t ldo, float* lse,
                                    int64_t n_dst, int C, int H, anemoi_stream_t stream);

/*
 * The folded edge phase for sources given as the RAW rows they are embedded from (bf16; the encoder's grid nodes):
 * with k_j,h = rstd_j A_k,h x_j + b_k,h and v_j,h = rstd_j A_v,h x_j + b_v,h (embedding and LayerNorm folded into the
 * k | v weights, the mean removed algebraically), both products move to the destination side:
 *   s_ij,h = (rstd_j qt_i,h . x_j + u_i,h . a'_ij) / sqrt(D)      qt_i,h = A_k,h^T q_i,h  (Ks values; q . b_k is constant
 *                                                                over a destination's in-edges and drops out of alpha)
 *   g_i,h  = sum_j alpha_ij,h rstd_j x_j                          -> sum_j alpha v_j,h = A_v,h g_i,h + b_v,h sum_j alpha
 * qt [n_dst, H, Ks] (ldqt) and g [n_dst, H, Ks] (ldg) bracket the kernel; x [n_src, Ks] (ldx) are the raw rows,
 * src_stats [n_src, 2] f32 their {rstd, -mean rstd} (anemoi_row_stats layout; only rstd is read).  Column sum_col of
 * every head of g (a column where x is zero; -1: none) receives sum_j alpha_ij,h (1, or 0 without in-edges), so that
 * b_v rides as one more weight column of the product that follows.  u, edge_attr, up, rowptr, col and t [n_dst, H, up]
 * (ldt) = sum_j alpha a'_ij as in anemoi_gt_edge_attention_folded; alpha includes the 1e-16 of the normaliser.
 * H = 16, Ks = 64, 128 or 256, up = 4, 8, 12 or 16; qt, x, g 16-byte aligned rows.  One wave per destination on MFMA, no
 * atomics, run-to-run bit-identical.
 */
int anemoi_gt_edge_attention_raw(const void* qt, int64_t ldqt, const void* x, int64_t ldx, const float* src_stats,
                                 const void* u, int64_t ldu, const float* edge_attr, int up, const int32_t* rowptr,
                                 const int32_t* col, void* g, int64_t ldg, void* t, int64_t ldt, int64_t n_dst, int H,
                                 int Ks, int D, int sum_col, anemoi_stream_t stream);

/*
 * anemoi_gt_edge_attention_folded on a graph whose destinations all have exactly three in-edges, stored as CSR with
 * rowptr[d] = 3 d (the mesh -> grid decoder of the reference, layers/mapper.py:348-418, on anemoi-graphs' 3-nearest-neighbour
 * edges): consecutive destinations fed by the SAME three sources form a run and share one gather of the three k / v rows.
 *   run_ptr  int32 [n_runs + 1]  first destination of every run (ascending, run_ptr[n_runs] = n_dst)
 *   run_perm int32 [n_runs]      6 bits per destination d = 0, 1 of the run (runs hold at most TWO); bits 6 d + 2 s .. + 1 =
 *                                position (0 .. 2) inside that destination's CSR segment of its edge to the s-th source in
 *                                ascending source order; all destinations of a run have the same source set
 * Same result as the plain entry point up to the f32 rounding of another summation order (deterministic).  bf16, head sizes
 * 64 / 32; other shapes, or run_ptr == NULL, run the plain kernel.  anemoi_models_amd/runtime.py::EdgePlan.runs3 builds the lists.
 */
int anemoi_gt_edge_attention_folded_runs(int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                         const void* x_r, int64_t ldr, const void* u, int64_t ldu, const float* edge_attr,
                                         int up, const int32_t* rowptr, const int32_t* col, const int32_t* run_ptr,
                                         const int32_t* run_perm, int64_t n_runs, void* out, int64_t ldo, float* lse,
                                         int64_t n_dst, int C, int H, anemoi_stream_t stream);

/*
 * The same launch on GROUPS: every destination fed by the same three sources -- the grid points of one mesh triangle, wherever
 * they lie in the grid's own order (5.4 per triangle at N320 -> ico-6, against runs of 1.5 consecutive ones) -- is walked
 * by one wave behind one gather of the three k / v row slices:
 *   grp_ptr  int32 [n_groups + 1]  group g = entries grp_ptr[g] .. grp_ptr[g + 1] - 1 (1 .. 8 of them) of
 *   grp_dst  int32 [n_dst]         the destinations, each exactly once (sorted by source triple)
 *   grp_perm int32 [n_dst]         per entry, bits 2 s .. 2 s + 1 = CSR position of its edge to the s-th source, ascending
 * n_src = rows of k / v.  Results equal anemoi_gt_edge_attention_folded_runs bit for bit (same per-destination arithmetic).
 * bf16, head size 64 / 32, every matrix below 4 GiB; anything else, or grp_ptr == NULL, runs the plain kernel.
 * anemoi_models_amd/runtime.py::EdgePlan.runs3 builds the lists (reference layers/mapper.py:348-418 on 3-NN decoder edges).
 */
int anemoi_gt_edge_attention_folded_groups(int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                           const void* x_r, int64_t ldr, const void* u, int64_t ldu, const float* edge_attr,
                                           int up, const int32_t* rowptr, const int32_t* col, const int32_t* grp_ptr,
                                           const int32_t* grp_dst, const int32_t* grp_perm, int64_t n_groups, int64_t n_src,
                                           void* out, int64_t ldo, float* lse, int64_t n_dst, int C, int H,
                                           anemoi_stream_t stream);

/*
 * anemoi_gt_edge_attention_folded with a DESTINATION SCHEDULE (round 5): the same result bit for bit -- same arithmetic,
 * same per-destination summation order -- from a launch in which
 *   - a host-built static schedule names the destinations every wave slot walks.  At any step the slots of an XCD work on
 *     one contiguous group of destinations (same L2 window as the plain kernel), but inside the group the destinations
 *     with many in-edges go to the slots with the least work so far: on a multi-scale icosahedral mesh (in-degree 6 ... 36)
 *     the plain round-robin leaves the busiest wave with 1.6 x the mean work, and the launch lasts as long as that wave;
 *   - schedule entry -> row pointers -> source ids are resolved by scalar loads one destination AHEAD each, and all of a
 *     destination's first loads (2 U row gathers, attribute rows, q / u / x_r) are in flight under one wait.
 * sched: int32 [8][slots][steps], XCD x's lists hold every destination of [n_dst x / 8, n_dst (x + 1) / 8) exactly once,
 * each list ends with at least three -1; slots / steps as anemoi_edge_schedule_shape returns them for (dtype, n_dst, C).
 * bf16 with 32- or 64-channel heads and every operand matrix -- the attribute matrix [n_edges, up] f32 included, n_edges =
 * rowptr[n_dst] stated by the caller -- below 4 GiB; other cases (or sched == NULL, or n_edges <= 0) run the plain kernel.
 * anemoi_models_amd/runtime.py::EdgePlan.schedule builds the lists.
 */
int anemoi_edge_schedule_shape(int dtype, int64_t n_dst, int C, int* slots, int* steps);
int anemoi_gt_edge_attention_folded_sched(int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                          const void* x_r, int64_t ldr, const void* u, int64_t ldu, const float* edge_attr,
                                          int up, const int32_t* rowptr, const int32_t* col, const int32_t* sched, int slots,
                                          int steps, int64_t n_src, int64_t n_edges, void* out, int64_t ldo, float* lse,
                                          int64_t n_dst, int C, int H, anemoi_stream_t stream);

/*
 * anemoi_gt_edge_attention_folded on LDS TILES (round 6): the same result bit for bit -- same arithmetic, same
 * per-destination summation order -- from a launch that stages every source row ONCE per tile instead of gathering it once
 * per edge.  A tile is a run of <= 32 consecutive destinations (an internal order that keeps graph neighbours together is
 * what makes it pay: the mesh's Morton order) whose in-edges name <= src_cap distinct sources and <= edge_cap edges; a
 * workgroup takes one tile x one 128-channel slice, copies the k | v slices of the tile's sources, the tile's attribute rows
 * and the per-edge LDS slot bytes into LDS, and a wave then walks four destinations at a time (one per 16-lane row) reading
 * its sources from LDS.  Lists (host-built, anemoi_models_amd/runtime.py::EdgeTiles; all on the device):
 *   tile_hdr  int32 [n_tiles][8]      first CSR slot e0, edge count, offset into tile_src, source count, offset into
 *                                     tile_slot (a multiple of 16), destination count, 0, 0
 *   tile_dst  int32 [n_tiles][32][2]  per (pass of four, row): destination id (-1: none), (first edge - e0) << 8 | in-degree
 *   tile_src  int32 [...]             the tiles' distinct sources
 *   tile_slot uint8 [...]             per tile, per edge in CSR order: index of its source in the tile's list
 *   tile_xcd  int32 [9]               tile index range of each of the 8 XCDs (destinations [n_dst x / 8, n_dst (x + 1) / 8))
 * bf16, 32- or 64-channel heads, C a multiple of 128, up in {4, 8, 12, 16}, every operand matrix below 2 GiB; other cases
 * (or tile_hdr == NULL) run the plain kernel.  Reference: layers/conv.py:98-142 (+ PyG propagate / softmax / scatter).
 */
int anemoi_gt_edge_attention_folded_tiles(int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                          const void* x_r, int64_t ldr, const void* u, int64_t ldu, const float* edge_attr,
                                          int up, const int32_t* rowptr, const int32_t* col, const int32_t* tile_hdr,
                                          const int32_t* tile_dst, const int32_t* tile_src, const uint8_t* tile_slot,
                                          const int32_t* tile_xcd, int max_tiles_per_xcd, int src_cap, int edge_cap,
                                          int64_t n_src, int64_t n_edges, void* out, int64_t ldo, float* lse, int64_t n_dst,
                                          int C, int H, anemoi_stream_t stream);

/*
 * GraphTransformerConv with explicit per-edge features (the callable the reference exposes, layers/conv.py:98-142):
 *   s_ij = q_i . (k_j + e_ij) / sqrt(D),  alpha = softmax over the in-edges of i (+1e-16),  out_i = sum_j alpha (v_j + e_ij)
 * q [n_dst, C], k / v [n_src, C], edges [E, C] in the CSR order of (rowptr, col) (= lin_edge(edge_attr)[perm]), all in
 * the activation dtype; x_r (optional) is added to the result, lse (optional f32 [n_dst, H]) receives the softmax
 * normaliser for the backward.  The block mirrors fold lin_edge away (see above) and come here only for edge_dim values
 * the folded / fused kernels do not cover (any edge_dim works on this route).
 * Backward (same structure as the folded backward below, with k + e, v + e in place of k, v):
 *   _dst: alpha, w [E, H], dsum [n_dst, H] (f32), dq;   _src: dk, dv and d edges [E, C] (CSR order) = alpha dout_i + scale ds q_i.
 * dropout_p / dropout_seed / dropout_seed_dev (ABI v41): the conv's `dropout` argument in training mode (reference
 * layers/conv.py:89,140 -- `dropout(alpha, p, training)` on alpha [E, H]): out_i = sum_j alpha keep / (1 - p) (v_j + e_ij) with
 * one counter-based keep decision per (CSR edge position, head) and seed (no mask tensor; the two backward entry points
 * take the same three arguments and rebuild it).  dropout_seed_dev: optional device word whose low 32 bits the kernels add
 * to the seed when they run (what a captured training step advances; NULL otherwise).  dropout_p = 0: the plain kernels.
 */
int anemoi_gt_conv(int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* edges,
                   int64_t lde, const void* x_r, int64_t ldr, const int32_t* rowptr, const int32_t* col, void* out,
                   int64_t ldo, float* lse, int64_t n_dst, int C, int H, float dropout_p, uint32_t dropout_seed,
                   const void* dropout_seed_dev, anemoi_stream_t stream);
int anemoi_gt_conv_backward_dst(int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                const void* edges, int64_t lde, const void* dout, int64_t ldd, const float* lse,
                                const int32_t* rowptr, const int32_t* col, float* alpha, float* w, float* dsum, void* dq,
                                int64_t lddq, int64_t n_dst, int C, int H, float dropout_p, uint32_t dropout_seed,
                                const void* dropout_seed_dev, anemoi_stream_t stream);
int anemoi_gt_conv_backward_src(int dtype, const void* q, int64_t ldq, const void* dout, int64_t ldd, const float* alpha,
                                const float* w, const float* dsum, const int32_t* rowptr_t, const int32_t* eid_t,
                                const int32_t* dst_t, void* dk, void* dv, int64_t ldg, void* dedges, int64_t ldde,
                                int64_t n_src, int C, int H, float dropout_p, uint32_t dropout_seed,
                                const void* dropout_seed_dev, anemoi_stream_t stream);

/*
 * Input assembly (I/O glue K9): rows (b, ens, g) of
 *   out = [ x[b, 0..T-1, ens, g, 0..V-1] (time-major) | latlons[g, 0:n_ll] | trainable[g, 0:n_tr] | 0-pad ]
 * x is f32 [B, T, Ens, G, V] contiguous; out is `dtype` with leading dimension ldo >= T*V + n_ll + n_tr.
 * Replaces einops.rearrange + NamedNodesAttributes + torch.cat, models/encoder_processor_decoder.py:173-181.
 * With x == NULL (T = 0) it produces the hidden-node attribute matrix of line :181.
 * in_mul / in_add (both NULL or both [V] f32): x is the RAW state and `x * in_mul[v] + in_add[v]` -- the
 * InputNormalizer's transform (preprocessing/normalizer.py:134-164) -- is applied while it is read.
 */
int anemoi_assemble_nodes(int dtype, const float* x, int B, int T, int Ens, int64_t G, int V, const float* latlons,
                          int n_ll, const float* trainable, int n_tr, void* out, int64_t ldo, const float* in_mul,
                          const float* in_add, anemoi_stream_t stream);

/*
 * The same for a LIST of grid nodes (batch 1, ensemble 1): out row i is the row of node rows[i] (int64 [n_rows], any order,
 * repeats allowed).  A rank of a node-partitioned run (models/encoder_processor_decoder.py:168-181 under a model group)
 * assembles only the grid rows its encoder reads and its decoder writes instead of the whole grid.
 */
int anemoi_assemble_node_rows(int dtype, const float* x, int T, int64_t G, int V, const float* latlons, int n_ll,
                              const float* trainable, int n_tr, const int64_t* rows, int64_t n_rows, void* out,
                              int64_t ldo, const float* in_mul, const float* in_add, anemoi_stream_t stream);

/*
 * One pass over the f32 output [B, Ens, G, V_out] that ends AnemoiModelInterface.predict_step on a raw input state:
 *   y[.., c] += normalised x[b, T-1, ens, g, src[c]]      where src[c] >= 0 (prognostic residual,
 *                                                          models/encoder_processor_decoder.py:227; src int32 [V_out])
 *   y[.., c]  = (y[.., c] - out_add[c]) / out_mul[c]       (InputNormalizer.inverse_transform,
 *                                                          preprocessing/normalizer.py:166-205; NULL/NULL = skipped)
 * with normalised x = x * in_mul[v] + in_add[v] (NULL/NULL: x is already normalised).
 */
int anemoi_finalize_output(float* y, int V_out, const float* x, int B, int T, int Ens, int64_t G, int V_in,
                           const int32_t* src, const float* in_mul, const float* in_add, const float* out_mul,
                           const float* out_add, anemoi_stream_t stream);

/*
 * The same on the rows a rank decodes (batch 1, ensemble 1): y is [n_rows, V_out], row i belongs to grid node rows[i]
 * (int64 [n_rows]) -- the residual and the de-normalisation are row-local, so a node-partitioned run finishes its own rows
 * BEFORE the final all-gather (models/encoder_processor_decoder.py:223-233, layers/mapper.py:99-102).
 */
int anemoi_finalize_output_rows(float* y, int V_out, const float* x, int T, int64_t G, int V_in, const int32_t* src,
                                const int64_t* rows, int64_t n_rows, const float* in_mul, const float* in_add,
                                const float* out_mul, const float* out_add, anemoi_stream_t stream);

/*
 * Output boundings, in place on the f32 output rows [rows, V_out] (rows = B * Ens * G) after the prognostic residual:
 * replaces the chained ReluBounding / HardtanhBounding / FractionBounding modules of
 * models/encoder_processor_decoder.py:229-231 (layers/bounding.py:60-124).  Every row applies, IN ORDER i = 0..n_ops-1,
 *   y[col[i]] = clamp(y[col[i]], lo[i], hi[i]) * (mul[i] >= 0 ? y[mul[i]] : 1)
 * (ReLU: lo = 0, hi = +inf; Hardtanh: lo = min_val, hi = max_val; the fraction step: lo = -inf, hi = +inf, mul = column
 * of total_var; NaN stays NaN), then de-normalises the n_fin columns fin_col[j]: y = (y - fin_add[j]) / fin_mul[j]
 * (InputNormalizer.inverse_transform of the columns the boundings had to see normalised; n_fin = 0: none).
 * All lists are device arrays (int32 / f32).
 */
int anemoi_bound_output(float* y, int V_out, int64_t rows, int n_ops, const int32_t* op_col, const float* op_lo,
                        const float* op_hi, const int32_t* op_mul, int n_fin, const int32_t* fin_col,
                        const float* fin_mul, const float* fin_add, anemoi_stream_t stream);

/*
 * NaN imputation folded into the three I/O kernels above (preprocessing/imputer.py: InputImputer / ConstantImputer and
 * their Dynamic forms between AnemoiModelInterface.predict_step and the model).  The kernels are the same templates with
 * a compile-time flag; the plain entry points above keep launching the instantiations without it.  Additive: no existing
 * signature changes and the ABI version is unchanged.
 *
 * anemoi_assemble_nodes_imputed: the arguments of anemoi_assemble_nodes plus
 *   fill_val  f32   [V]       value written when a point is imputed, ALREADY in the space the model sees (imputer before
 *                             normaliser: replacement * in_mul + in_add; normaliser before imputer: replacement)
 *   fill_src  int32 [V]       column of the NaN map for this input column, -1: the column is not imputed
 *   nan_map   uint8 [G, W]    row-major static NaN map (the imputer's nan_locations), or NULL: dynamic imputer
 *   W         int             width of the NaN map
 * For the state column c = t * V + v of row (b, ens, g):
 *   raw  = x[b, t, ens, g, v]
 *   pick = fill_src[v] >= 0 && (nan_map ? nan_map[g * W + fill_src[v]] != 0 : isnan(raw))
 *   val  = pick ? fill_val[v] : (in_mul ? raw * in_mul[v] + in_add[v] : raw)
 * The same map row serves every b, t, ens (_expand_subset_mask, preprocessing/imputer.py:106-108).  A static imputer
 * overwrites a mapped point whether or not it is NaN today and leaves a NaN outside the map alone; a dynamic one tests the
 * value it has just loaded.  Checks: fill_val / fill_src both NULL (nothing imputed: the call is anemoi_assemble_nodes) or
 * both given; nan_map needs them and W > 0; fill_src[v] < W and the G rows of the map are the caller's to guarantee.
 */
int anemoi_assemble_nodes_imputed(int dtype, const float* x, int B, int T, int Ens, int64_t G, int V, const float* latlons,
                                  int n_ll, const float* trainable, int n_tr, void* out, int64_t ldo, const float* in_mul,
                                  const float* in_add, const float* fill_val, const int32_t* fill_src,
                                  const uint8_t* nan_map, int W, anemoi_stream_t stream);

/*
 * anemoi_finalize_output_imputed: the arguments of anemoi_finalize_output plus fill_val / fill_src / nan_map / W as above --
 * the prognostic residual reads the last time slice of the RAW state and adds the imputed value there, not a NaN -- and
 *   out_nan_src int32 [V_out]  map column whose NaNs output column c gets back, -1: none (NULL: none at all)
 * After the residual and the de-normalisation: y[b, ens, g, c] = NaN where nan_map[g * W + out_nan_src[c]] != 0 (the
 * imputer's inverse_transform).  A dynamic imputer restores nothing: with nan_map == NULL out_nan_src is ignored.
 */
int anemoi_finalize_output_imputed(float* y, int V_out, const float* x, int B, int T, int Ens, int64_t G, int V_in,
                                   const int32_t* src, const float* in_mul, const float* in_add, const float* out_mul,
                                   const float* out_add, const float* fill_val, const int32_t* fill_src,
                                   const uint8_t* nan_map, int W, const int32_t* out_nan_src, anemoi_stream_t stream);

/*
 * anemoi_bound_output_imputed: the arguments of anemoi_bound_output plus the grid size G (rows % G == 0), nan_map, W and
 *   fin_nan_src int32 [n_fin]  map column whose NaNs column fin_col[j] gets back, -1: none
 * After the op list and the de-normalisation of fin_col[j]: y[row, fin_col[j]] = NaN where
 * nan_map[(row % G) * W + fin_nan_src[j]] != 0.  The rule between the two kernels: A COLUMN'S NaNs ARE RESTORED BY THE
 * KERNEL THAT DE-NORMALISES IT, AFTER IT HAS DONE SO -- the columns the boundings read or write stay finite until every
 * bounding op has run, as in the reference, where the boundings run inside the model and the imputer's inverse runs last.
 * nan_map == NULL (dynamic imputer): the call is anemoi_bound_output.
 */
int anemoi_bound_output_imputed(float* y, int V_out, int64_t rows, int n_ops, const int32_t* op_col, const float* op_lo,
                                const float* op_hi, const int32_t* op_mul, int n_fin, const int32_t* fin_col,
                                const float* fin_mul, const float* fin_add, int64_t G, const uint8_t* nan_map, int W,
                                const int32_t* fin_nan_src, anemoi_stream_t stream);

/*
 * Boundings with a slope (layers/bounding.py: NormalizedReluBounding and the Leaky* classes of current anemoi-models).
 * Additive: no existing signature changes and the ABI version is unchanged.  One op i becomes, with s = op_slope[i],
 *   f_i(v) = v < lo[i] ? lo[i] + s (v - lo[i]) : v > hi[i] ? hi[i] + s (v - hi[i]) : v
 *   y[col[i]] = f_i(y[col[i]]) * (mul[i] >= 0 ? y[mul[i]] : 1)
 * (comparisons: a NaN stays a NaN; s = 0 is the hard op of anemoi_bound_output, bit for bit).  Leaky ReLU: lo = 0, hi = +inf,
 * s = 0.01; leaky hardtanh / fraction: lo = min_val, hi = max_val, s = 0.01; (leaky) normalised ReLU: lo = the variable's
 * threshold in normalised space, hi = +inf, s = 0 (0.01).
 *
 * anemoi_bound_output_leaky: the arguments of anemoi_bound_output_imputed plus op_slope (f32 [n_ops], not NULL).  The same
 * kernel template with a second compile-time flag; anemoi_bound_output / _imputed keep launching the instantiations without
 * it.  nan_map == NULL: no NaN is restored (G, W and fin_nan_src are then ignored).
 */
int anemoi_bound_output_leaky(float* y, int V_out, int64_t rows, int n_ops, const int32_t* op_col, const float* op_lo,
                              const float* op_hi, const int32_t* op_mul, int n_fin, const int32_t* fin_col,
                              const float* fin_mul, const float* fin_add, int64_t G, const uint8_t* nan_map, int W,
                              const int32_t* fin_nan_src, const float* op_slope, anemoi_stream_t stream);

/*
 * The bounding list of the TRAINING forward as a differentiable pair (csrc/bounding.hip), one launch each way.
 *
 * anemoi_bound_output_train: the op walk above, in place on y [rows, V_out] (f32, no de-normalisation), which also writes the
 * TAPE the backward needs: walking i = 0..n_ops-1, the value op i read and, when mul[i] >= 0, the multiplier it read, one
 * entry each, entry e of row r at tape[e * rows + r].  n_tape = n_ops + the number of ops with mul[i] >= 0 (the caller counts
 * them; entries at or past n_tape are neither written nor read).  Column indices within [0, V_out) are the caller's to
 * guarantee, as for anemoi_bound_output.
 *
 * anemoi_bound_output_backward: dx [rows, V_out] (a buffer of its own: g is read only, the two must not overlap) from the
 * incoming gradient g [rows, V_out], the tape and the same op lists.  dx = g, then for i = n_ops-1..0 on every row:
 *   go = dx[col[i]];  dx[col[i]] = go * f_i'(v) * ym;  if mul[i] >= 0: dx[mul[i]] += go * f_i(v)
 * (v, ym: the tape's entries of op i; ym = 1 without a multiplier).  f_i'(v) = 1 strictly inside (lo[i], hi[i]) and s
 * elsewhere, the bounds included: the convention of torch's relu / hardtanh / leaky_relu backward at the kinks.
 *
 * Both: no atomics, no workspace, nothing read back (capturable), the same bits on every run.
 */
int anemoi_bound_output_train(float* y, int V_out, int64_t rows, int n_ops, const int32_t* op_col, const float* op_lo,
                              const float* op_hi, const int32_t* op_mul, const float* op_slope, float* tape, int n_tape,
                              anemoi_stream_t stream);
int anemoi_bound_output_backward(const float* g, float* dx, int V_out, int64_t rows, int n_ops, const int32_t* op_col,
                                 const float* op_lo, const float* op_hi, const int32_t* op_mul, const float* op_slope,
                                 const float* tape, int n_tape, anemoi_stream_t stream);

/*
 * Remappers folded into predict_step's I/O kernels (csrc/remap.hip; preprocessing/monomapper.py, multimapper.py: log1p,
 * sqrt, boxcox with lambda 1/2, cos_sin).  A remapper is a per-column function of the raw state whose internal layout
 * may be wider than the raw one (V_int != V_raw).  Additive: no existing signature changes and the ABI version is unchanged.
 *
 * One op code per column, one device function for the three kernels:
 *   ANEMOI_REMAP_COPY u | _LOG1P log1p(u) | _SQRT sqrt(u) | _BOXCOX (sqrt(u) - 1) / 0.5 | _COS cos(u pi / 180) |
 *   _SIN sin(u pi / 180) | _EXPM1 expm1(u) | _SQUARE u u | _INV_BOXCOX (0.5 u + 1)^2 |
 *   _ATAN2DEG remainder(atan2(u1, u) 180 / pi, 360), in [0, 360], of TWO source columns (u the cosine, u1 the sine)
 * Forward, internal input column j < V_int, from raw column src[j]:
 *   f_j(x) = post_mul[j] * op_j(pre_mul[j] * x + pre_add[j]) + post_add[j]                    op_j in COPY .. SIN
 * Inverse, raw output column c < V_out, from internal output column(s) s0[c] (and s1[c] for ATAN2DEG):
 *   u = (y[s0[c]] - post_add[s0[c]]) / post_mul[s0[c]],  u1 likewise from s1[c]
 *   z = (op_c(u, u1) - pre_add[c]) / pre_mul[c]                      op_c in COPY, EXPM1, SQUARE, INV_BOXCOX, ATAN2DEG
 * The InputNormalizer is the pre pair when it runs before the remapper and the post pair when it runs after; a pair given as
 * NULL / NULL is the identity and costs nothing.  NaN and values outside a converter's domain follow the C library (log1p of
 * a value below -1 and sqrt of a negative one are NaN, NaN stays NaN).
 *
 * All tables are device arrays.  h_* are HOST copies of the integer tables of the same name: the entry point checks them --
 * src / s0 / s1 / res inside their range, op codes inside the list above -- and returns ANEMOI_ERR_INVALID before anything is
 * launched; it reads no device memory and is capturable.  Every output element is written by one thread, no atomics.
 *
 * anemoi_assemble_nodes_remapped: anemoi_assemble_nodes whose feature column c = t * V_int + j holds
 * f_j(x[b, t, ens, g, src[j]]), x being f32 [B, T, Ens, G, V_raw]; same row layout [x | latlons | trainable | 0-pad], dtypes
 * and ldo rule (ldo >= T * V_int + n_ll + n_tr; eight columns per thread when ldo % 8 == 0 and out is 16-byte aligned).
 *
 * anemoi_residual_remapped: in place on the f32 internal output y [B, Ens, G, V_int_out],
 *   y[.., c] += f_j(x[b, T-1, ens, g, src[j]])   for j = res[c] >= 0     (res int32 [V_int_out], -1: none)
 * -- the prognostic residual on the remapped, normalised input; nothing is de-normalised here.
 *
 * anemoi_unmap_output: y f32 [rows, V_int_out] -> out f32 [rows, V_out] (another buffer), one thread per output element,
 * the inverse above; pre tables have V_out entries, post tables V_int_out.
 */
enum {
  ANEMOI_REMAP_COPY = 0, ANEMOI_REMAP_LOG1P = 1, ANEMOI_REMAP_SQRT = 2, ANEMOI_REMAP_BOXCOX = 3, ANEMOI_REMAP_COS = 4,
  ANEMOI_REMAP_SIN = 5, ANEMOI_REMAP_EXPM1 = 6, ANEMOI_REMAP_SQUARE = 7, ANEMOI_REMAP_INV_BOXCOX = 8,
  ANEMOI_REMAP_ATAN2DEG = 9
};
int anemoi_assemble_nodes_remapped(int dtype, const float* x, int B, int T, int Ens, int64_t G, int V_raw, int V_int,
                                   const float* latlons, int n_ll, const float* trainable, int n_tr, void* out, int64_t ldo,
                                   const int32_t* src, const int32_t* op, const float* pre_mul, const float* pre_add,
                                   const float* post_mul, const float* post_add, const int32_t* h_src, const int32_t* h_op,
                                   anemoi_stream_t stream);
int anemoi_residual_remapped(float* y, int V_int_out, const float* x, int B, int T, int Ens, int64_t G, int V_raw, int V_int,
                             const int32_t* res, const int32_t* src, const int32_t* op, const float* pre_mul,
                             const float* pre_add, const float* post_mul, const float* post_add, const int32_t* h_res,
                             const int32_t* h_src, const int32_t* h_op, anemoi_stream_t stream);
int anemoi_unmap_output(const float* y, int V_int_out, float* out, int V_out, int64_t rows, const int32_t* s0,
                        const int32_t* s1, const int32_t* op, const float* pre_mul, const float* pre_add,
                        const float* post_mul, const float* post_add, const int32_t* h_s0, const int32_t* h_s1,
                        const int32_t* h_op, anemoi_stream_t stream);

/*
 * Prognostic residual (models/encoder_processor_decoder.py:227), in place on the f32 output:
 *   y[b, ens, g, out_idx[p]] += x[b, T-1, ens, g, in_idx[p]]   for p < n_prog.
 */
int anemoi_prognostic_residual(float* y, int V_out, const float* x, int B, int T, int Ens, int64_t G, int V_in,
                               const int32_t* out_idx, const int32_t* in_idx, int n_prog, anemoi_stream_t stream);

/*
 * Autoregressive rollout: next model input from the current one and the prediction, in place on x (f32
 * [B, T, Ens, G, V_in]):  x[:, t] <- x[:, t+1] for t < T-1, then for the last time slice
 *   colmap[v] >= 0  : x[b, T-1, ens, g, v] = y[b, ens, g, colmap[v]]            (prognostic variables)
 *   colmap[v] <= -2 : x[b, T-1, ens, g, v] = forcing[b, ens, g, -2 - colmap[v]]  (forcings of the new time; skipped
 *                     when forcing == NULL: the previous value persists)
 *   colmap[v] == -1 : the previous value persists.
 * The reference repository stops at one step (interface/__init__.py:97-123); this is the caller's loop
 * (anemoi-training `advance_input`: roll the time axis, write the prognostic outputs, write the new forcings), i.e.
 * BASELINE config 4.  y is f32 [B, Ens, G, V_out], forcing f32 [B, Ens, G, F] or NULL.
 */
int anemoi_advance_input(float* x, int B, int T, int Ens, int64_t G, int V_in, const float* y, int V_out,
                         const float* forcing, int F, const int32_t* colmap, anemoi_stream_t stream);

/*
 * Rollout training (ABI v47, csrc/rollout.hip): the differentiable state advance between two steps of a training rollout
 * (anemoi-training sums a loss over the steps and lets the gradient flow through `advance_input`), the input gradients of
 * the one-pass I/O kernels above, and the rollout loss (anemoi_weighted_mse below, csrc/losses.hip).  Every output element is
 * owned by exactly one thread: no atomics, the same bits on every run.  Outputs named "in full" are written completely (no
 * zero-fill by the caller).
 *
 * anemoi_advance_state: the out-of-place form of anemoi_advance_input -- x_out (f32 [B, T, Ens, G, V_in], must not overlap
 * x_in) receives what anemoi_advance_input would leave in a copy of x_in; same colmap / forcing / persist semantics, the
 * same bits.
 */
int anemoi_advance_state(const float* x_in, float* x_out, int B, int T, int Ens, int64_t G, int V_in, const float* y,
                         int V_out, const float* forcing, int F, const int32_t* colmap, anemoi_stream_t stream);

/*
 * Its backward.  dx_out is the gradient of x_out; dx_in (f32 [B, T, Ens, G, V_in], must not overlap dx_out) and dy (f32
 * [B, Ens, G, V_out]) are written in full:
 *   dx_in[:, 0] = 0 (T > 1);  dx_in[:, t] = dx_out[:, t-1] for t >= 1;
 *   dx_in[:, T-1, .., v] += dx_out[:, T-1, .., v] in the persisting columns: colmap[v] == -1, or colmap[v] <= -2 when the
 *   forward ran without forcing (has_forcing == 0);  with T == 1 only that term remains;
 *   dy[.., m] = dx_out[:, T-1, .., inv_colmap[m]] where inv_colmap[m] >= 0, else 0.
 * inv_colmap is int32 [V_out]: the input column v with colmap[v] == m, or -1 -- built once by the host, which refuses a
 * colmap whose non-negative entries repeat.
 */
int anemoi_advance_state_backward(const float* dx_out, float* dx_in, float* dy, int B, int T, int Ens, int64_t G,
                                  int V_in, int V_out, const int32_t* colmap, const int32_t* inv_colmap,
                                  int has_forcing, anemoi_stream_t stream);

/*
 * Input gradient of anemoi_assemble_nodes: dx[b, t, ens, g, v] = float(grad[(b, ens, g), t * V + v]) -- the leading T * V
 * columns of the gradient of its output (`dtype`, leading dimension ldg >= T * V).  dx is f32 [B, T, Ens, G, V], in full.
 */
int anemoi_assemble_nodes_backward(int dtype, const void* grad, int64_t ldg, float* dx, int B, int T, int Ens, int64_t G,
                                   int V, anemoi_stream_t stream);

/*
 * Input gradient of the prognostic residual of anemoi_finalize_output (src int32 [V_out] as there, no affine maps): dx (f32
 * [B, T, Ens, G, V_in], in full) is zero except dx[:, T-1, .., src[c]] = dy[.., c] where src[c] >= 0 (an input column that
 * feeds several output columns receives their sum, in output-column order).  dy is f32 [B, Ens, G, V_out].  V_in <= 1024.
 */
int anemoi_prognostic_residual_backward(const float* dy, int V_out, float* dx, int B, int T, int Ens, int64_t G, int V_in,
                                        const int32_t* src, anemoi_stream_t stream);

/*
 * Truncated residual connection (ABI v52, csrc/truncation.hip): current anemoi-models adds A_up (A_down x[:, -1]) -- the last
 * input state projected to a coarser grid and back by two sparse interpolation matrices -- to the decoder output instead of
 * the state itself.  One CSR projection serves both products and, on the transposed matrices, their backward:
 *   out[s, i, cols_out[p]]  (= or +=)  sum_{k = indptr[i] .. indptr[i+1]-1} val[k] * x'[s, idx[k], cols_in[p]]     p < P
 *   x' = x * in_mul[cols_in[p]] + in_add[cols_in[p]]        (both NULL: x' = x)
 * x and out are f32 with unit-stride columns and rows ldx / ldo elements apart; indptr int64 [n_out + 1], idx int32 (< n_in),
 * val f32; cols_in / cols_out int32 [P], NULL = 0..P-1.  Slab s = so * n_inner + si (so < n_outer, si < n_inner) of x starts
 * at x + so * xs_outer + si * xs_inner and of out at out + so * os_outer + si * os_inner (element strides; the caller adds
 * the base, e.g. time slice T-1): the down-projection reads x [B, T, Ens, G, V_in] -- or a transposed view of it -- in place
 * for every (b, ens), the up-projection accumulates straight into y [B, Ens, G, V_out].  accumulate = 0 stores (an empty row
 * writes 0), 1 adds to out (an empty row leaves it untouched).  Each output element is owned by one thread that adds the
 * terms of its row in ascending CSR position with one f32 FMA each: no atomics, no workspace, the same bits on every run.
 * Negative sizes or strides, P <= 0, a row pitch below P under NULL columns and overlapping output slabs are
 * ANEMOI_ERR_INVALID before any launch; more than 65535 slabs is ANEMOI_ERR_UNSUPPORTED.  x must not overlap out.
 */
int anemoi_csr_project(const float* x, int64_t ldx, int64_t xs_outer, int64_t xs_inner, float* out, int64_t ldo,
                       int64_t os_outer, int64_t os_inner, int n_outer, int n_inner, int64_t n_in, int64_t n_out,
                       const int64_t* indptr, const int32_t* idx, const float* val, const int32_t* cols_in,
                       const int32_t* cols_out, int P, const float* in_mul, const float* in_add, int accumulate,
                       anemoi_stream_t stream);

/*
 * The rollout loss (csrc/losses.hip, with the loss family below): node-weighted, variable-scaled, masked squared error over
 * pred / target (f32 [rows, V] contiguous; rows is a multiple of G and row r belongs to grid node r % G, so a stack of rollout
 * steps, batch and ensemble members is one call):
 *   loss = scale * sum_{r, v} keep(r, v) ? row_w[r % G] * col_w[v] * (pred - target)^2 : 0
 * row_w f32 [G], col_w f32 [V], mask f32 [G, V] or NULL, keep = mask[r % G, v] != 0.  The mask is a SELECT: a masked element
 * contributes exactly 0 even where pred or target is NaN (imputed values); an unmasked NaN propagates.  Two deterministic
 * stages: one f32 partial per workgroup in `workspace` (anemoi_weighted_mse_workspace_floats(rows, V) floats -- the workgroup
 * count is a function of rows * V alone, never of the device), then one workgroup sums the partials in a fixed order into
 * loss (device f32 scalar).  rows == 0: loss = 0 by a memset.
 */
int64_t anemoi_weighted_mse_workspace_floats(int64_t rows, int V);
int anemoi_weighted_mse(const float* pred, const float* target, int64_t rows, int V, int64_t G, const float* row_w,
                        const float* col_w, const float* mask, float scale, float* loss, float* workspace,
                        int64_t workspace_floats, anemoi_stream_t stream);

/*
 * Its gradient: dpred = upstream * scale * 2 * row_w * col_w * (pred - target) where kept, exactly 0 where masked.
 * `upstream` is a DEVICE pointer to the f32 scalar gradient of loss: no host synchronisation (graph capture safe).
 */
int anemoi_weighted_mse_backward(const float* pred, const float* target, int64_t rows, int V, int64_t G,
                                 const float* row_w, const float* col_w, const float* mask, float scale,
                                 const float* upstream, float* dpred, anemoi_stream_t stream);

/*
 * The loss family (ABI v48, csrc/losses.hip): per-variable node-weighted error over pred / target (f32 [rows, V] contiguous),
 * one value per group of rows and variable.  rows = n_groups * rows_per_group with rows_per_group a multiple of G; group l is
 * the rows [l * rows_per_group, (l + 1) * rows_per_group) (a rollout step; n_groups = 1: the whole tensor), row r is grid node r % G:
 *   out[l, v] = scale * sum_{r in group l} keep(r, v) ? row_w[r % G] * col_w[v] * f(c[v] * (pred[r, v] - target[r, v])) : 0
 * row_w f32 [G]; col_w f32 [V] or NULL (ones); mask f32 [G, V] or NULL, keep = mask[r % G, v] != 0, a SELECT as in
 * anemoi_weighted_mse; diff_scale c f32 [V] or NULL (ones): the per-variable scale of the difference (de-normalisation).
 * `kind` selects f (d = c * (pred - target)):
 *   ANEMOI_LOSS_MSE      f = d^2                                                   f' = 2 d
 *   ANEMOI_LOSS_MAE      f = |d|                                                   f' = sign(d), 0 at d = 0
 *   ANEMOI_LOSS_HUBER    f = 0.5 d^2 if |d| <= delta else delta (|d| - 0.5 delta)  f' = d if |d| <= delta else delta sign(d)
 *   ANEMOI_LOSS_LOGCOSH  f = |d| + log1p(exp(-2 |d|)) - ln 2                       f' = tanh(d)
 * (`delta` is read by ANEMOI_LOSS_HUBER only and must be positive there.)  Two deterministic stages without atomics: every
 * workgroup of stage 1 belongs to one group, reduces a contiguous chunk of its rows and writes one [V] partial to `workspace`
 * (anemoi_weighted_error_workspace_floats(n_groups, rows_per_group, V) floats: the workgroup count and the chunks are functions
 * of these three numbers alone); stage 2 adds the partials of a group per variable in ascending workgroup order and applies
 * `scale`.  out is f32 [n_groups, V].  rows == 0: out = 0 by a memset.  n_groups <= 65535.
 */
#define ANEMOI_LOSS_MSE 0
#define ANEMOI_LOSS_MAE 1
#define ANEMOI_LOSS_HUBER 2
#define ANEMOI_LOSS_LOGCOSH 3
int64_t anemoi_weighted_error_workspace_floats(int64_t n_groups, int64_t rows_per_group, int V);
int anemoi_weighted_error(int kind, float delta, const float* pred, const float* target, int64_t rows, int V, int64_t G,
                          int64_t n_groups, const float* row_w, const float* col_w, const float* mask,
                          const float* diff_scale, float scale, float* out, float* workspace, int64_t workspace_floats,
                          anemoi_stream_t stream);

/*
 * Its gradient, one element-wise kernel:
 *   dpred[r, v] = keep ? (scale * upstream[l, v] * row_w[r % G] * col_w[v] * c[v]) * f'(c[v] * (pred - target)) : 0
 * `upstream` is a DEVICE pointer to the f32 [n_groups, V] gradient of out: no host synchronisation (graph capture safe).
 * The gradient of target is -dpred.
 */
int anemoi_weighted_error_backward(int kind, float delta, const float* pred, const float* target, int64_t rows, int V,
                                   int64_t G, int64_t n_groups, const float* row_w, const float* col_w, const float* mask,
                                   const float* diff_scale, float scale, const float* upstream, float* dpred,
                                   anemoi_stream_t stream);

/*
 * Ensemble scores (ABI v49, csrc/ensemble.hip): per-variable node-weighted scores of an E-member ensemble against one target,
 * one value per group of points and variable.  target is f32 [rows, V] contiguous with rows = n_groups * B * G (no ensemble
 * axis; group l is the rows [l * B * G, (l + 1) * B * G), a rollout step; row r is grid node r % G); pred is f32 [rows * E, V]
 * contiguous, member e of point (l, b, g) in row ((l * B + b) * E + e) * G + g:
 *   out[l, v] = scale * sum_{b, g} keep(g, v) ? row_w[g] * col_w[v] * S(c[v] x_1 .. c[v] x_E, c[v] y) : 0
 * row_w f32 [G]; col_w f32 [V] or NULL (ones); mask f32 [G, V] or NULL, keep = mask[g, v] != 0, a SELECT as in
 * anemoi_weighted_error (a masked point contributes exactly 0 even where the target is NaN or a member Inf); diff_scale c f32
 * [V] or NULL (ones).  `kind` selects S:
 *   ANEMOI_ENS_AFCRPS    S = 1/E sum_j |x_j - y| - (1 - eps) / (2 E (E - 1)) sum_{j != k} |x_j - x_k|,  eps = (1 - alpha) / E
 *                        (the almost-fair kernel CRPS; alpha = 1: the fair CRPS, alpha = 0: the ensemble CRPS with 1 / (2 E^2))
 *   ANEMOI_ENS_MEAN_SE   S = (mean_j x_j - y)^2
 *   ANEMOI_ENS_VARIANCE  S = 1 / (E - 1) sum_j (x_j - mean)^2  (the mean first, then the squares)
 * evaluated on e_j = c (x_j - y), which S takes the same value on; the CRPS as the sum over the pairs j < k of the non-negative
 * 2 |med3(e_j, e_k, 0)| + eps |e_j - e_k| (= |e_j| + |e_k| - (1 - eps) |e_j - e_k|) over E (E - 1).  2 <= E <= 16 (E < 2:
 * ANEMOI_ERR_INVALID, E > 16: ANEMOI_ERR_UNSUPPORTED); alpha in [0, 1] for every kind (read by ANEMOI_ENS_AFCRPS only).
 * Every member is read once and held in registers.  Two deterministic stages without atomics: every workgroup of stage 1
 * belongs to one group, reduces a contiguous chunk of its points (members ascending, pairs ascending in (j, k)) and writes one
 * [V] partial to `workspace`
 * (anemoi_ensemble_score_workspace_floats(n_groups, B * G, V, E) floats: the workgroup count and the chunks are functions of
 * these four numbers alone); stage 2 adds the partials of a group per variable in ascending workgroup order and applies
 * `scale`.  out is f32 [n_groups, V].  rows == 0: out = 0 by a memset.  n_groups <= 65535, G * V < 2^31.
 */
#define ANEMOI_ENS_AFCRPS 0
#define ANEMOI_ENS_MEAN_SE 1
#define ANEMOI_ENS_VARIANCE 2
int64_t anemoi_ensemble_score_workspace_floats(int64_t n_groups, int64_t points_per_group, int V, int E);
int anemoi_ensemble_score(int kind, float alpha, const float* pred, const float* target, int64_t rows, int V, int64_t G, int E,
                          int64_t n_groups, const float* row_w, const float* col_w, const float* mask,
                          const float* diff_scale, float scale, float* out, float* workspace, int64_t workspace_floats,
                          anemoi_stream_t stream);

/*
 * The gradient of ANEMOI_ENS_AFCRPS for the members (the other kinds: ANEMOI_ERR_UNSUPPORTED; the target gets none), one
 * thread per point and variable writing its E values:
 *   dpred[e] = keep ? scale * upstream[l, v] * row_w[g] * col_w[v] * |c[v]|
 *                     * (sgn(x_e - y) / E - (1 - eps) / (E (E - 1)) sum_k sgn(x_e - x_k)) : 0
 * sgn is taken by comparing the raw members, so equal values give exactly 0 (torch's convention for |.|).  `upstream` is a
 * DEVICE pointer to the f32 [n_groups, V] gradient of out: no host synchronisation (graph capture safe).  dpred is f32
 * [rows * E, V].
 */
int anemoi_ensemble_score_backward(int kind, float alpha, const float* pred, const float* target, int64_t rows, int V,
                                   int64_t G, int E, int64_t n_groups, const float* row_w, const float* col_w,
                                   const float* mask, const float* diff_scale, float scale, const float* upstream,
                                   float* dpred, anemoi_stream_t stream);

/*
 * Conditional LayerNorm (the processor LayerNorm of an ensemble model: scale and shift are linear in a per-row condition):
 *   y[r, c] = xhat[r, c] * (1 + cond[r, :] . Ws[c, :] + bs[c]) + (cond[r, :] . Wb[c, :] + bb[c])
 * x, y: [rows, C] in `dtype` (f32 or bf16); cond: f32 [rows, K] with leading dimension ldc; Ws, Wb: f32 [C, K] (an
 * nn.Linear(K, C).weight) with leading dimension ldw; bs, bb: f32 [C].  The caller pads K to KP = 4, 8, 16 or 32 columns
 * (the next of these): ldc, ldw >= KP and multiples of 4, cond / Ws / Wb 16-byte aligned (ANEMOI_ERR_INVALID otherwise),
 * columns K .. KP - 1 zero (the contents are the caller's) -- the kernels read KP columns with 16-byte loads and have one
 * code path per KP.  xhat = (x - mean) * rstd with the statistics of anemoi_layer_norm -- the same order of every sum: with
 * zero weights y is bit for bit anemoi_layer_norm(gamma = 1, beta = 0) -- and stats[r] = { rstd_r, -mean_r * rstd_r } as
 * anemoi_row_stats leaves them (stats may be NULL).  Neither [rows, C] product exists in memory.  1 <= K <= 32 (K < 1:
 * ANEMOI_ERR_INVALID; K > 32: ANEMOI_ERR_UNSUPPORTED, the caller composes the operation from a Linear and a LayerNorm); every
 * C of anemoi_layer_norm.
 */
int anemoi_cond_layer_norm(int dtype, const void* x, int64_t ldx, const float* cond, int64_t ldc, int K, const float* Ws,
                           int64_t ldw, const float* bs, const float* Wb, const float* bb, void* y, int64_t ldy, float* stats,
                           int64_t rows, int C, float eps, anemoi_stream_t stream);

/*
 * Its backward.  With ds = dy * xhat and g = dy * (1 + s):
 *   dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat))       dcond[r, k] = sum_c ds * Ws[c, k] + dy * Wb[c, k]
 *   dWs[c, k] = sum_r ds * cond[r, k]    dbs[c] = sum_r ds      dWb[c, k] = sum_r dy * cond[r, k]    dbb[c] = sum_r dy
 * (dx in `dtype`, everything else f32; cond, Ws, Wb padded as in the forward; dcond [rows, K], dWs and dWb [C, K] contiguous).
 * Deterministic, no atomics: the column sums are taken over fixed chunks of rows, one [2 K + 2, C] partial per chunk in
 * `workspace` (anemoi_cond_layer_norm_backward_workspace_floats(rows, C, K) floats; the chunks are a function of `rows`
 * alone), and added in ascending chunk order.
 */
int64_t anemoi_cond_layer_norm_backward_workspace_floats(int64_t rows, int C, int K);
int anemoi_cond_layer_norm_backward(int dtype, const void* dy, int64_t ldd, const void* x, int64_t ldx, const float* stats,
                                    const float* cond, int64_t ldc, int K, const float* Ws, int64_t ldw, const float* bs,
                                    const float* Wb, void* dx, int64_t ldo, float* dcond, float* dWs, float* dbs, float* dWb,
                                    float* dbb, int64_t rows, int C, float* workspace, int64_t workspace_floats,
                                    anemoi_stream_t stream);

/*
 * out[rows, K] (f32, contiguous) = std * z, z ~ N(0, 1), counter-based: element i = row * K + k is a function of
 * (seed + *seed_dev, i) alone, whatever `rows` and the launch.  Philox4x32-10 with counter (i / 4, (i / 4) >> 32, 0, 0) and
 * key (seed + *seed_dev, 0x6E6F6973) yields the words w0..w3 of the elements 4 q .. 4 q + 3; a pair (wa, wb) gives
 *   u1 = ((wa >> 8) + 1) / 2^24,  u2 = (wb >> 8) / 2^24,  (z, z') = sqrt(-2 ln u1) * (cos 2 pi u2, sin 2 pi u2)
 * -- (w0, w1) the elements 4 q and 4 q + 1, (w2, w3) the next two -- so |z| <= sqrt(48 ln 2) ~ 5.77.  `seed_dev`: NULL or a
 * device word added to the seed by the kernel (what a captured training step advances, as for the dropout kernels).
 */
int anemoi_gaussian_noise(float* out, int64_t rows, int K, float std, uint32_t seed, const void* seed_dev,
                          anemoi_stream_t stream);

/*
 * qk_norm: the bias-free LayerNorm over the head dimension of queries and keys, between the q|k|v product and the attention
 * kernel.  x, y: [rows, groups * H * D] views in `dtype` (f32 or bf16) with leading dimensions ldx, ldy; w: f32 [groups, D]
 * (q | k adjacent in one matrix: groups = 2 and the weights of q_norm and k_norm stacked; a single q or k: groups = 1):
 *   y[r, (g H + h) D + d] = (x - mean) * rstd * w[g, d],  mean and the biased variance over the D elements of the head, in f32,
 *   rstd = 1 / sqrt(var + eps); the result is rounded once, to `dtype`.
 * y == x is the in-place form (inference: no copy of the product's output); otherwise x and y must not overlap.  `stats` (may be
 * NULL): f32 [rows, groups * H, 2] = { rstd, -mean * rstd }, the convention of anemoi_layer_norm_stats.  One read and one write
 * of the addressed columns, no other column of a row is touched.  16-byte accesses when x, y, ldx, ldy and D * sizeof(elem) are
 * multiples of 16 bytes, element accesses otherwise.  1 <= D <= 128 (D < 1: ANEMOI_ERR_INVALID; D > 128:
 * ANEMOI_ERR_UNSUPPORTED).
 */
int anemoi_head_norm(int dtype, const void* x, int64_t ldx, const float* w, void* y, int64_t ldy, float* stats, int64_t rows,
                     int groups, int H, int D, float eps, anemoi_stream_t stream);

/*
 * Its backward from the pre-norm x and the forward's statistics.  With g = dy * w and xhat = x * rstd + (-mean * rstd):
 *   dx = rstd * (g - mean_d(g) - xhat * mean_d(g * xhat))       dw[g, d] = sum_{r, h} dy * xhat       (no division by w)
 * dy, x, dx: [rows, groups * H * D] views in `dtype` (ldd, ldx, ldo); dw: f32 [groups, D] contiguous.  Deterministic, no atomics:
 * the column sums are taken over fixed chunks of rows (a function of `rows` alone), one [groups * H * D] partial per chunk in
 * `workspace` (anemoi_head_norm_backward_workspace_floats(rows, groups, H, D) floats), added in ascending chunk order, then
 * the heads of a group in ascending order.
 */
int64_t anemoi_head_norm_backward_workspace_floats(int64_t rows, int groups, int H, int D);
int anemoi_head_norm_backward(int dtype, const void* dy, int64_t ldd, const void* x, int64_t ldx, const float* stats,
                              const float* w, void* dx, int64_t ldo, float* dw, int64_t rows, int groups, int H, int D,
                              float* workspace, int64_t workspace_floats, anemoi_stream_t stream);

/* dtype conversion / K-padding copy: dst[r, 0:cols] = src[r, 0:cols], dst[r, cols:ld_dst] = 0. */
int anemoi_convert_pad(int src_dtype, const void* src, int64_t ld_src, int dst_dtype, void* dst, int64_t ld_dst,
                       int64_t rows, int cols, anemoi_stream_t stream);

/* y = a + b elementwise over [rows, cols] slices (processor skip, models/encoder_processor_decoder.py:204). */
int anemoi_add(int dtype, const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t ldy, int64_t rows,
               int cols, anemoi_stream_t stream);

/*
 * GNN edge phase, part 1 (K5): out[e, :] = act(t[e, :] + p_dst[dst[e], :] + p_src[src[e], :]).
 * With t = e W1c^T + b1, p_dst = x W1a^T, p_src = x W1b^T this is the first Linear + activation of the edge MLP applied
 * to cat[x_i, x_j, e] (layers/conv.py:68-69, layers/mlp.py:74) without materialising the [E, 3C] concatenation.
 * dst / src: int32 [E] node index per edge (CSR order: dst ascending).
 */
int anemoi_gather_add_act(int dtype, const void* t, int64_t ldt, const void* p_dst, int64_t ldpd, const void* p_src,
                          int64_t ldps, const int32_t* dst, const int32_t* src, void* out, int64_t ldo,
                          int64_t n_edges, int C, int act, anemoi_stream_t stream);

/*
 * GNN edge phase, part 2: out[i, :] = sum of v[e, :] over the CSR row i (edges sorted by destination), f32 accumulation
 * in CSR order.  Replaces torch_geometric scatter(reduce="sum") at layers/conv.py:73-76.
 */
int anemoi_segment_sum(int dtype, const void* v, int64_t ldv, const int32_t* rowptr, void* out, int64_t ldo,
                       int64_t n_dst, int C, anemoi_stream_t stream);

/*
 * The same pass producing the node MLP's input of a GNN block, out[i, :] = [ x[i, 0:C] | sum of v[e, :] over CSR row i ]
 * (out is [n_dst, ldo >= 2C]): torch.cat([x, aggregated], dim=1) at layers/block.py:217, 276 without a separate copy of x.
 */
int anemoi_segment_sum_cat(int dtype, const void* v, int64_t ldv, const int32_t* rowptr, const void* x, int64_t ldx,
                           void* out, int64_t ldo, int64_t n_dst, int C, anemoi_stream_t stream);

/*
 * Mesh-node multi-head self attention (K7): out[b*S + i, h*D:(h+1)*D] = softmax_j(q_i . k_j / sqrt(D)) v_j per head,
 * flash style, on the fused lin_qkv output qkv [B*S, 3C] = q | k | v (leading dimension ld), C = H*D.
 * Replaces the rearranges + flash_attn_func / scaled_dot_product_attention of layers/attention.py:76-108.
 * window < 0: global attention (the reference's SDPA fallback); window >= 0: flash-attn sliding window |i - j| <= window.
 * bf16 with D = 64 or 32 runs on MFMA and needs `workspace` of anemoi_mhsa_workspace_bytes() bytes (V transposed);
 * other cases use a VALU kernel (workspace may be NULL).
 * dropout_p in [0, 1] (attention dropout of the reference in training mode, layers/attention.py:90): probabilities are
 * dropped AFTER normalisation by a counter-based hash of (batch, head, query, key) and `dropout_seed`, kept ones scaled
 * by 1 / (1 - p); the backward rebuilds the same mask from the same seed.  One 32-bit hash decides the key pair
 * (2 j, 2 j + 1) of a query, 16 bits each (p is resolved to 2^-16).  The MFMA kernels apply the mask to their packed
 * probabilities (0 < p < 1, B x heads x S < 2^32); p = 1 takes the VALU kernel.  `dropout_h0` / `dropout_h_total`: the
 * GLOBAL index of head 0 of this call and the head count of the whole attention (0 = H) -- a head-sharded call
 * (sequence-parallel attention, distributed/transformer.py:85-130) then draws exactly the mask of the unsharded one.
 * `dropout_seed_dev` (may be NULL): a 4-byte aligned DEVICE word whose value every kernel of the call adds to
 * `dropout_seed` when it starts -- the part of the seed a captured HIP graph can advance between replays (kernel arguments
 * are frozen at capture; anemoi_models_amd/runtime.py::DeviceDropout).  The backward must be given the same word, holding
 * the value the forward saw.
 * Route.  The MFMA kernels take a call with dtype bf16, D = 64 or 32, dropout_p < 1, B x heads x S < 2^32 (heads =
 * dropout_h_total, or H where that is 0), `qkv` 16-byte and `out` 8-byte aligned, ld a multiple of 8 and ldo a multiple of
 * 4 elements; such a call without a workspace is refused (ANEMOI_ERR_INVALID).  D = 64 with window < 0 and
 * S x ld x 2 < 2^31 bytes runs the four-wave kernel (the eight-wave one behind its device-side fallback flag), every other
 * MFMA call the eight-wave kernel; the 1 .. 16 rows behind the last whole 512-row block of an S > 512 go to the key-split
 * tail kernels.  Every other call takes the VALU kernel: D <= 128, B x S x H / 4 < 2^31 workgroups
 * (ANEMOI_ERR_UNSUPPORTED beyond either).  anemoi_mhsa_route (below) answers which of these a call takes.
 */
int64_t anemoi_mhsa_workspace_bytes(int dtype, int B, int S, int H, int D);
int anemoi_mhsa(int dtype, const void* qkv, int64_t ld, void* out, int64_t ldo, void* workspace, float* lse, int B, int S,
                int H, int D, int window, float dropout_p, uint32_t dropout_seed, const void* dropout_seed_dev,
                int dropout_h0, int dropout_h_total, anemoi_stream_t stream);

/*
 * Backward of anemoi_mhsa (what torch autograd derives for the reference's scaled_dot_product_attention call,
 * layers/attention.py:99-105, when anemoi-training calls .backward()).  `lse` f32 [B, H, S] is the forward's optional
 * output (natural-log sum-exp of the scaled scores per query and head; pass NULL to the forward when not training), `out`
 * the forward's result, `dout` its gradient; writes dqkv [B*S, 3C] = dq | dk | dv in `dtype`.  `delta` f32 [B, H, S] is
 * scratch.  Probabilities are recomputed from lse (nothing of size S x S is stored); no atomics.  bf16 with D = 64 / 32
 * and dropout_p < 1: MFMA kernels (one pass with the keys stationary for dK / dV, one with the queries stationary for dQ)
 * on a `workspace` of anemoi_mhsa_backward_workspace_bytes() bytes (Q^T, K^T, dO^T and the padded lse / delta rows the
 * dK / dV kernel streams); otherwise VALU kernels, O(S^2 D) on the vector pipe (workspace may be NULL).
 * Route.  D <= 128 and B x S x H / 4 < 2^31 hold for every call (ANEMOI_ERR_UNSUPPORTED otherwise).  The MFMA kernels
 * take a call with dtype bf16, D = 64 or 32, dropout_p < 1, B x heads x S < 2^32, B x S, ld and lddo < 2^31, a non-NULL
 * 16-byte aligned `workspace`, `qkv` and `dout` 16-byte, `dqkv` 8-byte and `out` 2-byte aligned, ld and lddo multiples of
 * 8 and lddq a multiple of 4 elements.  A call that misses any of these -- a NULL or misaligned workspace included --
 * is NOT refused: it runs the VALU kernels, which compute the same gradients and are orders of magnitude slower at
 * mesh sizes (46 s per layer at S = 40 962).  Withholding the workspace is the supported way to ask for them (the
 * tests' yardstick); a caller that wants the MFMA kernels asks anemoi_mhsa_route what its call takes.
 */
int64_t anemoi_mhsa_backward_workspace_bytes(int dtype, int B, int S, int H, int D);
int anemoi_mhsa_backward(int dtype, const void* qkv, int64_t ld, const void* out, int64_t ldo, const void* dout,
                         int64_t lddo, const float* lse, float* delta, void* dqkv, int64_t lddq, void* workspace, int B,
                         int S, int H, int D, int window, float dropout_p, uint32_t dropout_seed,
                         const void* dropout_seed_dev, int dropout_h0, int dropout_h_total, anemoi_stream_t stream);

/*
 * Route query of self attention (tests and diagnostics; nothing on the hot path calls it).  anemoi_mhsa and
 * anemoi_mhsa_backward gather their arguments in an anemoi_mhsa_args, validate them, plan an anemoi_mhsa_route_info and
 * execute it; anemoi_mhsa_route runs the same validation and the same plan on the same two types, launches nothing,
 * touches no memory and needs no device, and returns the status the entry point would return before its first launch.
 * Pointers are looked at for NULL and alignment only.  Fields the forward does not have (dout, delta, dqkv, lddo, lddq)
 * stay 0 / NULL.  `struct_bytes` of both blocks must be their sizeof (layout check across the FFI).
 */
enum { ANEMOI_MHSA_ENTRY_FORWARD = 0, ANEMOI_MHSA_ENTRY_BACKWARD = 1 };
enum {
  ANEMOI_MHSA_KERNEL_GENERIC = 0, /* the VALU kernels, forward or backward */
  ANEMOI_MHSA_KERNEL_W8 = 1,      /* forward: the eight-wave MFMA kernel */
  ANEMOI_MHSA_KERNEL_W4 = 2,      /* forward: the four-wave MFMA kernel, the eight-wave one behind its flag */
  ANEMOI_MHSA_KERNEL_BWD_MFMA = 3 /* backward: the dK / dV and dQ MFMA kernels */
};

typedef struct anemoi_mhsa_args {
  int64_t struct_bytes;
  int32_t entry, dtype;
  const void* qkv;
  void* out;       /* the forward's result (the backward reads it) */
  float* lse;      /* forward: optional output; backward: input */
  const void* dout;
  float* delta;
  void* dqkv;
  void* workspace;
  const void* dropout_seed_dev;
  int64_t ld, ldo, lddo, lddq;
  int32_t B, S, H, D, window;
  float dropout_p;
  uint32_t dropout_seed;
  int32_t dropout_h0, dropout_h_total, reserved;
} anemoi_mhsa_args;

typedef struct anemoi_mhsa_workspace_layout { /* byte offsets into `workspace`, and its size */
  int64_t vt, tail, flag;                     /* forward: V^T, the tail rows' partial states, the four-wave kernel's flag */
  int64_t qt, kt, dot, lse2p, deltap;         /* backward: Q^T, K^T, dO^T, the padded lse (log2 units) and delta rows */
  int64_t total;                              /* = anemoi_mhsa[_backward]_workspace_bytes() */
} anemoi_mhsa_workspace_layout;

typedef struct anemoi_mhsa_route_info {
  int64_t struct_bytes;
  int32_t kernel;     /* ANEMOI_MHSA_KERNEL_* */
  int32_t drop;       /* a mask is hashed (0 < dropout_p < 1 after rounding to 15 bits): the MFMA kernels' DROP argument */
  int32_t win;        /* backward MFMA kernels' WIN argument (window >= 0); 0 elsewhere */
  int32_t dmax;       /* the VALU kernels' DMAX (32, 64 or 128); 0 on the MFMA routes */
  int32_t S_pad;      /* MFMA routes: S rounded up to 64, the row length of the transposed operands */
  int32_t tail_rows, tail_splits, tail_chunk; /* forward MFMA: rows of the key-split tail pair, key chunks, keys per chunk */
  uint32_t grid[3];   /* workgroups of the main launch (forward kernel; dK / dV and dQ kernels; VALU kernels) */
  int32_t reserved;
  anemoi_mhsa_workspace_layout layout; /* MFMA routes; all 0 on the VALU route, which uses no workspace */
} anemoi_mhsa_route_info;

int anemoi_mhsa_route(const anemoi_mhsa_args* args, anemoi_mhsa_route_info* route);

/* ------------------------------------------------------------------------------------------------------------------
 * Backward pass, dense half (first step): the pieces the autograd of the fused Linear and of
 * LayerNorm needs besides the forward GEMM entry points (anemoi_models_amd/autograd.py):
 *   dX = dpre W (anemoi_linear on dpre and W^T), dW = dpre^T X (anemoi_linear on the two transposes, f32 result),
 *   db = column sums of dpre, dpre = dy * act'(pre).  What torch.autograd derives from nn.Linear / nn.GELU / nn.SiLU /
 *   nn.LayerNorm in layers/block.py:504-508,631-633 and layers/mlp.py:74-84 when anemoi-training calls .backward().
 * No atomics: gradients are reproducible bit for bit.
 * ------------------------------------------------------------------------------------------------------------------ */

/* dst[c, r] = src[r, c]; dst has leading dimension ld_dst >= rows, its columns rows..ld_dst-1 are zero filled. */
int anemoi_transpose(int dtype, const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int cols,
                     anemoi_stream_t stream);

/* Chunked form: rows [s * chunk_rows, (s + 1) * chunk_rows) of src become slab s of dst = [chunks, cols, ld_dst]
 * (ld_dst >= chunk_rows, zero filled behind the chunk's rows).  colsum_partial (optional, bf16 sources, cols % 4 == 0):
 * f32 [anemoi_transpose_colsum_rows(rows, chunk_rows), cols] -- every 64-row tile leaves the column sums of its source
 * rows there; their sum over the rows (anemoi_col_sum) is the column sum of src (the bias gradient, without a second pass
 * over dpre). */
int64_t anemoi_transpose_colsum_rows(int64_t rows, int64_t chunk_rows);
int anemoi_transpose_chunked(int dtype, const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int cols,
                             int64_t chunk_rows, float* colsum_partial, anemoi_stream_t stream);

/* Weight gradient without transposed copies (bf16): partial[c] [N, K] f32 (contiguous, c = 0 .. ceil(M / chunk_rows) - 1)
 * <- sum over the rows m of chunk c of dy[m, :N]^T x[m, :K]; bias_partial (optional) [chunks, N] f32 <- the column sums of
 * dy over the chunk (the bias gradient, out of the same pass).  partial_stride / bias_stride: floats between the chunks of
 * either (>= N * K / >= N) -- both may live in one [chunks, N * K + N] buffer that one anemoi_col_sum reduces.  dy [M, ldy], x [M, ldx] row-major, 16-byte aligned, pitches
 * and N, K multiples of 8; chunk_rows a multiple of 64, >= 128, chunk_rows * pitch * 2 < 2 GiB.  The caller adds the
 * chunks (anemoi_col_sum).  Replaces autograd's grad_output.t() @ input of every nn.Linear under
 * models/encoder_processor_decoder.py:167-233 (training). */
int anemoi_weight_grad_tn(const void* dy, int64_t ldy, const void* x, int64_t ldx, void* partial, int64_t partial_stride,
                          void* bias_partial, int64_t bias_stride, int64_t M, int N, int K, int chunk_rows,
                          anemoi_stream_t stream);

/* `batch` independent products y[b] = x[b] w[b]^T (strides in elements; no bias / activation): the weight-gradient GEMMs
 * split their long reduction over the rows into `batch` chunks this way and add the partial [N, K] results with
 * anemoi_col_sum -- deterministic, and a small result still fills the chip. */
int anemoi_linear_batched(int dtype, int out_dtype, const void* x, int64_t ldx, int64_t stride_x, const void* w,
                          int64_t stride_w, void* y, int64_t ldy, int64_t stride_y, int batch, int64_t M, int N, int K,
                          anemoi_stream_t stream);

/* out[c] = sum_r x[r, c] (f32 result, two deterministic stages; workspace: anemoi_col_sum_workspace_floats floats). */
int64_t anemoi_col_sum_workspace_floats(int64_t rows, int cols);
int anemoi_col_sum(int dtype, const void* x, int64_t ldx, int64_t rows, int cols, float* out, float* workspace,
                   int64_t workspace_floats, anemoi_stream_t stream);

/* out[r] = sum_c a[r, c] * (b[r, c] - shift[c]) in f32 (shift optional: f32 [cols]).  The training route's folded
 * "embedding -> LayerNorm -> Linear" product y = rstd * (x F^T) + b' needs d rstd[r] = sum_c dy[r, c] (y[r, c] - b'[c]) / rstd[r]
 * (anemoi_models_amd/autograd.py::_ScaledLinear; reference layers/mapper.py:322-331 + layers/block.py:516-528 under autograd). */
int anemoi_row_dot(int dtype, const void* a, int64_t lda, const void* b, int64_t ldb, const float* shift, float* out,
                   int64_t rows, int cols, anemoi_stream_t stream);

/* out[r, c] = alpha * s[r] * x[r, c] (s: f32 per row; out in x's dtype, may alias x): the row scalings of the same folded
 * product's backward (dx = rstd (dy F), dF = dy^T (rstd x)) and of its variance term x^T (A^T A / C) x. */
int anemoi_row_scale(int dtype, const void* x, int64_t ldx, const float* s, float alpha, void* out, int64_t ldo,
                     int64_t rows, int cols, anemoi_stream_t stream);

/* out[r, 0:cols] = stats[r, 0] * x[r, :] (f32 product, one rounding), out[r, cols:2 cols] = x[r, :] -- stats the [rows, 2] f32
 * LayerNorm statistics {rstd, -mean rstd} of the rows.  The two raw-row blocks the decoder's projection product reads behind
 * out | t of the folded edge phase when x_r and the embedded grid rows are folded into it (layers/block.py::_native_dec_fold,
 * DESIGN.md section 4.2).  Whole 16-byte pieces only (cols, ldx, ldo multiples of 16 bytes, aligned pointers), ldo >= 2 cols;
 * anything else is ANEMOI_ERR_UNSUPPORTED before any launch.  Additive: the ABI version is unchanged. */
int anemoi_raw_row_tail(int dtype, const void* x, int64_t ldx, const float* stats, void* out, int64_t ldo, int64_t rows,
                        int cols, anemoi_stream_t stream);

/* out = act(pre) (+ residual): the differentiable forward keeps `pre` for act' and applies the activation in one pass. */
int anemoi_act_forward(int dtype, int act, const void* pre, int64_t ldp, const void* residual, int64_t ldr, void* out,
                       int64_t ldo, int64_t rows, int cols, anemoi_stream_t stream);

/* out = dy * act'(pre), pre = the Linear's result before its activation (ANEMOI_ACT_*; exact erf GELU derivative). */
int anemoi_act_backward(int dtype, int act, const void* pre, int64_t ldp, const void* dy, int64_t ldd, void* out,
                        int64_t ldo, int64_t rows, int cols, anemoi_stream_t stream);

/*
 * Training forward of Linear + activation: y = act(x W^T + b) and pre = x W^T + b (rounded to the activation dtype) from
 * ONE launch (the backward multiplies by act'(pre); nn.Linear + nn.GELU of layers/mlp.py:74-84, layers/block.py:504-508
 * under autograd).  bf16 only, M = a multiple of 256 plus at most 8 rows (the mesh sizes 10 * 4^k + 2: the last rows are
 * computed by the same launch), N >= 256, K >= 128 (multiple of 64), 16-byte aligned operands; ANEMOI_ERR_UNSUPPORTED
 * otherwise -- the caller then runs anemoi_linear followed by anemoi_act_forward.
 */
int anemoi_linear_dual(int dtype, const void* x, int64_t ldx, const void* w, const float* bias, void* pre, int64_t ldp,
                       void* y, int64_t ldy, int64_t M, int N, int K, int act, anemoi_stream_t stream);

/*
 * Backward counterpart: y = (x W^T) * act'(pre) in one launch -- with x = dy and W = W2^T this is the dX GEMM of the
 * Linear BEHIND an activation delivering d pre of the Linear in front of it (what autograd derives for
 * Linear -> GELU -> Linear, layers/mlp.py:74-84), without a separate act' pass.  GELU': degree-8 polynomial in x^2 of the
 * exact derivative, |error| < 5.5e-4.  Same shape rules / fallback as anemoi_linear_dual.
 */
int anemoi_linear_actgrad(int dtype, const void* x, int64_t ldx, const void* w, const void* pre, int64_t ldp, void* y,
                          int64_t ldy, int64_t M, int N, int K, int act, anemoi_stream_t stream);

/*
 * Route query of the fused Linear family (tests and diagnostics; nothing on the hot path calls it).  Every entry point
 * above gathers its arguments in an anemoi_linear_args, validates them, plans an anemoi_linear_route_info and executes it;
 * anemoi_linear_route runs the same validation and the same plan on the same two types, launches nothing and touches no
 * device, and returns the status the entry point would return before its first launch.  Pointers are looked at for NULL
 * and alignment only.  Fields an entry point does not have stay 0 / NULL.  `struct_bytes` of both blocks must be their
 * sizeof (layout check across the FFI).
 */
enum {
  ANEMOI_LINEAR_ENTRY_LINEAR = 0,
  ANEMOI_LINEAR_ENTRY_LN = 1,
  ANEMOI_LINEAR_ENTRY_STATS = 2,
  ANEMOI_LINEAR_ENTRY_DUAL = 3,
  ANEMOI_LINEAR_ENTRY_ACTGRAD = 4,
  ANEMOI_LINEAR_ENTRY_BATCHED = 5
};
enum { ANEMOI_LINEAR_KERNEL_NONE = 0, ANEMOI_LINEAR_KERNEL_128 = 1, ANEMOI_LINEAR_KERNEL_PERSISTENT = 2 };
enum {
  ANEMOI_LINEAR_REST_NONE = 0,
  ANEMOI_LINEAR_REST_IN_LAUNCH = 1, /* the persistent kernel's own skinny pass */
  ANEMOI_LINEAR_REST_SKINNY = 2,    /* the stand-alone skinny kernel */
  ANEMOI_LINEAR_REST_128 = 3        /* a launch of the 128 x 128 kernel */
};

typedef struct anemoi_linear_args {
  int64_t struct_bytes;
  int32_t entry, dtype, out_dtype, act;
  const void* x;
  const void* w;
  const float* bias;
  const float* colsum; /* LayerNorm fold (_ln, _stats) */
  const float* stats;
  const void* residual; /* the residual; `pre` of _dual (an output) and _actgrad (an input), ldr = ldp */
  void* y;
  int64_t ldx, ldr, ldy, M;
  int32_t N, K;
  void* workspace; /* _stats */
  int64_t workspace_bytes;
  float* stats_out;
  int64_t stride_x, stride_w, stride_y; /* _batched */
  int32_t batch, reserved;
} anemoi_linear_args;

typedef struct anemoi_linear_route_launch { /* one launch of the persistent kernel */
  int64_t row0, rows, tiles;                 /* first row, rows, tiles of 32 mh x 256 (all problems of a batched call) */
  int32_t mh, blocks, tail_rows;             /* tile height / 32; workgroups; rows behind `rows` on the in-launch skinny pass */
  int32_t stagger_phases, stagger_unit, reserved;
} anemoi_linear_route_launch;

typedef struct anemoi_linear_route_info {
  int64_t struct_bytes;
  int32_t kernel;     /* ANEMOI_LINEAR_KERNEL_*: what computes rows 0 .. main_rows (NONE: M = 0, nothing to do) */
  int32_t n_launches; /* persistent kernel: 1 or 2 */
  anemoi_linear_route_launch launch[2];
  int64_t main_rows;
  int32_t rest; /* ANEMOI_LINEAR_REST_*: what computes the rest_rows rows from rest_row0 on */
  int32_t nt;   /* persistent kernel: column tiles of 256 */
  int64_t rest_row0, rest_rows;
  int64_t rs_rows; /* leading rows whose row-sum partials the launches leave in the workspace (_stats); 0: none */
  int32_t vec_ok;  /* the epilogue's vector path (the kernel family's own rule) */
  int32_t split;   /* the launches are the half-tile split: [256-row tiles,] 128-row tiles of the remainder round */
  int32_t model;   /* the tile-height cost model ran */
  int32_t reserved;
} anemoi_linear_route_info;

int anemoi_linear_route(const anemoi_linear_args* args, anemoi_linear_route_info* route);

/*
 * Thin Linear (csrc/gemm_thin.hip): y[M, N] = epilogue(x[M, K] W^T + b) for bf16 x and W whose weight is small enough to stay
 * in the four waves' registers for the whole launch, while the rows of x stream through once (global -> VGPR in the MFMA
 * operand layout, no LDS staging).  It is NOT part of the fused Linear family above: nothing of it goes through that
 * family's plan, and anemoi_linear_route knows nothing of it.  Shapes (N, K) taken: (256, 64), (64, 256), (256, 256),
 * (80, 1024), (16, 1024), (16, 256), (256, 128); any M >= 1.  Every other shape, and every combination named below as not taken, returns
 * ANEMOI_ERR_UNSUPPORTED before anything is launched -- the caller then keeps the fused Linear family's route.
 *
 *   batch > 1: `batch` independent problems; problem b reads x + b stride_x, w + b stride_w, residual + b stride_r,
 *     bias + b N and writes y + b stride_y (strides in elements: column blocks of one row-major matrix, as
 *     anemoi_linear_batched takes them).  Not with colsum / stats / stats_out, and only for the shapes with K <= 256.
 *   colsum + stats: the LayerNorm fold of anemoi_linear_ln, acc * stats[m].x + stats[m].y * colsum[n], before the bias.
 *   residual (bf16): added after the result was rounded to bf16 when out_dtype is bf16 (round, add, round: the persistent
 *     kernel's order); added in f32 when out_dtype is f32.
 *   stats_out != NULL ("statistics only"): nothing is stored to y (y may be NULL); stats_out[m] = { rstd, -mean rstd } of
 *     row m of the result as it WOULD be stored in out_dtype, by the two-pass formula of anemoi_row_stats with `eps`.
 *     Not with a residual.
 * Alignment: x, w, y, residual 16 bytes; ldx, stride_x, stride_w multiples of 8; ldy, stride_y (and ldr, stride_r)
 * multiples of 8 (bf16) or 4 (f32); bias, colsum 16 bytes.  ANEMOI_ERR_INVALID otherwise.  x is read up to row M - 1 only
 * and y written up to row M - 1 only.  No atomics: two calls give the same bits.  `struct_bytes` must be sizeof.
 */
typedef struct anemoi_linear_thin_args {
  int64_t struct_bytes;
  int32_t out_dtype; /* ANEMOI_BF16 / ANEMOI_F32 */
  int32_t batch;     /* 0 or 1: one problem */
  const void* x;
  const void* w;
  const float* bias;
  const float* colsum;
  const float* stats;
  const void* residual;
  void* y;
  float* stats_out;
  int64_t ldx, ldr, ldy, M;
  int32_t N, K;
  int64_t stride_x, stride_w, stride_y, stride_r;
  float eps;
  int32_t reserved;
} anemoi_linear_thin_args;

int anemoi_linear_thin(const anemoi_linear_thin_args* args, anemoi_stream_t stream);

/*
 * LayerNorm backward from the forward's row statistics (stats [rows, 2] = { rstd, -mean * rstd }, anemoi_row_stats):
 *   dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)), g = dy * gamma, xhat = x * rstd - mean * rstd;
 *   dgamma[c] = sum_r dy * xhat, dbeta[c] = sum_r dy (f32).  workspace: anemoi_layer_norm_backward_workspace_floats.
 *   dres (optional, [rows, ldr] in x's dtype): added to dx before the store -- the gradient that reaches x through the skip
 *   connection around the LayerNorm (layers/block.py:504-508, 614-635: x + mlp(norm(x))), instead of a separate add pass.
 */
int64_t anemoi_layer_norm_backward_workspace_floats(int64_t rows, int C);
int anemoi_layer_norm_backward(int dtype, const void* x, int64_t ldx, const float* stats, const float* gamma,
                               const void* dy, int64_t ldd, const void* dres, int64_t ldr, void* dx, int64_t ldo,
                               int64_t rows, int C, float* dgamma, float* dbeta, float* workspace,
                               int64_t workspace_floats, anemoi_stream_t stream);

/*
 * Backward of anemoi_gt_edge_attention_folded (the edge half of SURVEY.md section 8f-1; what torch.autograd derives from
 * GraphTransformerConv.message / softmax / aggregate, layers/conv.py:98-142, plus lin_edge through the fold).
 * With s_e = scale (q_i.k_j + u_i.a_e), alpha_e = exp(s_e - lse_i) (lse: the forward's optional output), out_i = sum alpha
 * v_j (+ x_r), t_i = sum alpha a_e, and for the incoming gradients dout [n_dst, C] and dt [n_dst, H*up]:
 *   w_e = alpha_e (dout_i,h.v_j,h + dt_i,h.a_e),   dsum[i, h] = sum_e w_e,   ds_e = w_e - alpha_e dsum[i, h]
 *   _dst  (forward CSR, ONE sweep over the in-edges):  alpha[E, H], w[E, H], dsum[n_dst, H] (f32);
 *                            dq_i = scale sum_e ds k_j,  du_i = scale sum_e ds a_e   (activation dtype, any leading dim)
 *   _src  (transposed CSR):  dk_j = scale sum_{e from j} ds q_i,  dv_j = sum_{e from j} alpha dout_i
 *   anemoi_gt_edge_attr_grad: dattr[e, a] = sum_h (scale ds[e, h] u[dst(e), h, a] + alpha[e, h] dt[dst(e), h, a]), the
 *                            gradient of the edge attributes [E, up] (CSR order; trainable edge tensor columns included)
 * (rowptr_t [n_src+1], eid_t [E] = position of the edge in the forward CSR, dst_t [E] = its destination; u / dt / du are
 * [n_dst, H*up] column ranges in the activation dtype, dst_of_edge [E] the destination of every CSR slot).  dsum is
 * accumulated in f32 over the edges, never rebuilt from the forward's rounded output.  No atomics.
 * dxr (optional, [n_dst, lddxr]): _dst also leaves a copy of dout there -- the gradient of the self term x_r of
 * out = sum alpha v + x_r -- so that a caller who keeps x_r | q | k | v | u in one matrix fills d x_r without a pass of its own.
 */
int anemoi_gt_edge_attention_folded_backward_dst(int dtype, const void* q, int64_t ldq, const void* k, const void* v,
                                                 int64_t ldkv, const void* dout, int64_t ldd, const void* u, int64_t ldu,
                                                 const void* dt, int64_t lddt, const float* lse, const float* edge_attr,
                                                 int up, const int32_t* rowptr, const int32_t* col, float* alpha,
                                                 float* w, float* dsum, void* dq, int64_t lddq, void* du, int64_t lddu,
                                                 void* dxr, int64_t lddxr, int64_t n_dst, int C, int H,
                                                 anemoi_stream_t stream);
int anemoi_gt_edge_attention_folded_backward_src(int dtype, const void* q, int64_t ldq, const void* dout, int64_t ldd,
                                                 const float* alpha, const float* w, const float* dsum,
                                                 const int32_t* rowptr_t, const int32_t* eid_t, const int32_t* dst_t,
                                                 void* dk, void* dv, int64_t ldg, int64_t n_src, int C, int H,
                                                 anemoi_stream_t stream);
int anemoi_gt_edge_attr_grad(int dtype, const float* alpha, const float* w, const float* dsum, const void* u, int64_t ldu,
                             const void* dt, int64_t lddt, const int32_t* dst_of_edge, float* dattr, int64_t n_edges,
                             int H, int up, int D, anemoi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Block-level entry points ("gt_block_fwd(x, ln / lin weights, edge attributes, csr, ..., out,
 * stream)"): a whole GraphTransformer block's launch sequence from ONE call on the caller's stream -- what
 * GraphTransformerProcessorBlock.forward (reference layers/block.py:602-635) and the back half of
 * GraphTransformerMapperBlock.forward (layers/block.py:516-550) do, on the bf16 LayerNorm-folded route: the host mirror
 * pays one FFI call per block instead of five or six (host enqueue of a forward: 2.6 -> 0.6 ms).  Weights arrive packed
 * as the op-level entry points above take them (LayerNorm folded in by the caller: W' = W * gamma, column sums of W',
 * b' = b + W beta; lin_edge folded into W_in / W_proj); every buffer -- workspaces included -- is the caller's.
 *
 *   anemoi_gt_block_tail              out = mlp(LN(y)) + y,  y = projection(edge_phase(q, k, v, u) + x_r | t) + res
 *                                     (edge phase = anemoi_gt_edge_attention_folded; projection = anemoi_linear_stats
 *                                     with the node MLP's LayerNorm statistics in its epilogue; mlp = LayerNorm-folded
 *                                     Linear + activation (anemoi_linear_ln), Linear + y (anemoi_linear_stats, or
 *                                     anemoi_linear when out_stats is NULL))
 *   anemoi_gt_processor_block_forward the x_r | q | k | v | u product of LayerNorm(x) first (anemoi_linear_ln into
 *                                     `sq`, whose column ranges then ARE q, k, v, x_r, u), then the tail with res = x.
 * `struct_bytes` must be sizeof(anemoi_gt_block_args) (layout check across the FFI).  Status codes as everywhere.
 */
typedef struct anemoi_gt_block_args {
  int64_t struct_bytes;
  int64_t n_dst;           /* destination rows (processor block: all rows)                                       */
  int32_t dtype;           /* ANEMOI_BF16                                                                        */
  int32_t C, H, up;        /* channels, heads, folded edge width per head                                        */
  int32_t hidden, act;     /* node MLP: hidden width, activation code                                            */
  int32_t k_proj, n_in;    /* projection K (= ld of att: C + H * up, slab padded); columns of the input product  */
  float eps_mlp, eps_out;  /* epsilon of the node MLP's LayerNorm; of the LayerNorm that consumes `out` next     */
  /* LayerNorm-folded input product (anemoi_gt_processor_block_forward only) */
  const void* x; int64_t ldx; const float* x_stats;                 /* [n_dst, C], its row statistics            */
  const void* w_in; const float* b_in; const float* cs_in;          /* [n_in, C] = x_r | q | k | v | u rows      */
  void* sq; int64_t ld_sq;                                          /* [n_dst, n_in] workspace                   */
  /* edge phase (the processor entry point overwrites these with column ranges of sq) */
  const void* q; const void* k; const void* v; const void* x_r; const void* u;
  int64_t ldq, ldkv, ldr, ldu;
  const float* edge_attr; const int32_t* rowptr; const int32_t* col; /* [E, up] f32 CSR order, int32 CSR           */
  void* att; int64_t ld_att;                                        /* [n_dst, k_proj] workspace; the caller has */
                                                                    /* ZEROED its columns >= C + H * up (K pad)  */
  /* projection (+ res) -> y and the statistics of the node MLP's LayerNorm */
  const void* w_proj; const float* b_proj; const void* res; int64_t ld_res; void* y; float* y_stats;
  /* node MLP */
  const void* w_fc1; const float* b_fc1; const float* cs_fc1; void* h;  /* [hidden, C] LayerNorm-folded; [n_dst, hidden] */
  const void* w_fc2; const float* b_fc2; void* out; float* out_stats;   /* [C, hidden]; out [n_dst, C]; NULL: no stats   */
  void* stats_ws; int64_t stats_ws_bytes;                           /* >= n_dst * max(C / 128, 1) * 8 bytes      */
  /* optional (NULL / 0: plain edge kernel): the runs of a uniform-degree-3 graph, anemoi_gt_edge_attention_folded_runs */
  const int32_t* run_ptr; const int32_t* run_perm; int64_t n_runs;
  /* optional (NULL: none; ignored when runs are given): the destination schedule of anemoi_gt_edge_attention_folded_sched */
  const int32_t* sched; int32_t sched_slots, sched_steps; int64_t n_src;
  /* optional (NULL: run_ptr / run_perm are the consecutive runs above): run_ptr / run_perm / run_dst are the GROUP lists of
   * anemoi_gt_edge_attention_folded_groups (groups of 1 .. 8 destinations out of run_dst, run_perm per destination; n_src set) */
  const int32_t* run_dst;
  /* rowptr[n_dst], stated by the caller: the scheduled kernel addresses attribute rows by 32-bit byte offsets and is taken
   * only when n_edges * up * 4 < 2^32 (<= 0: not stated, plain kernel) */
  int64_t n_edges;
  /* optional (NULL: none; taken before the schedule, ignored when runs are given): the tile lists of
   * anemoi_gt_edge_attention_folded_tiles (n_src, n_edges set) */
  const int32_t* tile_hdr; const int32_t* tile_dst; const int32_t* tile_src; const uint8_t* tile_slot; const int32_t* tile_xcd;
  int32_t tile_max_per_xcd, tile_src_cap, tile_edge_cap, tile_pad;
} anemoi_gt_block_args;
int anemoi_gt_block_tail(const anemoi_gt_block_args* args, anemoi_stream_t stream);
int anemoi_gt_processor_block_forward(const anemoi_gt_block_args* args, anemoi_stream_t stream);

/*
 * anemoi_transformer_block_forward: TransformerProcessorBlock.forward (reference layers/block.py:99-105 over
 * layers/attention.py:67-112) from one call, f32 or bf16 --
 *     y   = x + projection(attention(lin_qkv(layer_norm1(x))))
 *     out = y + mlp(layer_norm2(y)),    mlp = Linear -> activation -> Linear
 * as the launch sequence anemoi_layer_norm, anemoi_linear, anemoi_mhsa, anemoi_linear (+ x), anemoi_layer_norm,
 * anemoi_linear (+ activation), anemoi_linear (+ y) on the caller's stream.  Weights [out, K] in `dtype`, K zero padded to
 * the slab multiple as for anemoi_linear (C itself must be a multiple); LayerNorm parameters and biases f32 (biases may be
 * NULL); `qkv` / `att` / `y` / `h_ln` / `h` are the caller's workspaces, `mhsa_ws` of anemoi_mhsa_workspace_bytes() bytes;
 * window / dropout arguments as anemoi_mhsa.  `out` may not alias `x`.
 */
typedef struct anemoi_tfm_block_args {
  int64_t struct_bytes;
  int64_t rows;              /* B * S node rows                                                                    */
  int32_t dtype;             /* ANEMOI_F32 or ANEMOI_BF16                                                          */
  int32_t B, S, C, H;        /* batch, sequence length (rows = B * S), channels, heads                             */
  int32_t hidden, act;       /* MLP hidden width, activation code                                                  */
  int32_t window;            /* < 0: global attention                                                              */
  float eps1, eps2;          /* epsilon of layer_norm1 / layer_norm2                                               */
  float dropout_p; uint32_t dropout_seed; const void* dropout_seed_dev; int32_t dropout_h0, dropout_h_total;
  const void* x; int64_t ldx;                                       /* [rows, C]                                   */
  const float* ln1_w; const float* ln1_b; const float* ln2_w; const float* ln2_b;
  const void* w_qkv; const float* b_qkv;                            /* [3 C, C]                                    */
  const void* w_proj; const float* b_proj;                          /* [C, C]                                      */
  const void* w_fc1; const float* b_fc1;                            /* [hidden, C]                                 */
  const void* w_fc2; const float* b_fc2;                            /* [C, hidden]                                 */
  void* h_ln;                                                       /* [rows, C]      layer_norm1 / layer_norm2 out */
  void* qkv;                                                        /* [rows, 3 C]                                 */
  void* att;                                                        /* [rows, C]                                   */
  void* y;                                                          /* [rows, C]                                   */
  void* h;                                                          /* [rows, hidden]                              */
  void* mhsa_ws;                                                    /* anemoi_mhsa_workspace_bytes (may be NULL)   */
  void* out;                                                        /* [rows, C]                                   */
} anemoi_tfm_block_args;
int anemoi_transformer_block_forward(const anemoi_tfm_block_args* args, anemoi_stream_t stream);

/*
 * MXFP8 (OCP MX v1.0, E4M3 elements) -- opt-in inference format of csrc/mx.hip.
 *   block    32 consecutive K-elements of one row.
 *   scale    amax = max |v| over the block; e = floor(log2(amax)) - 8 clamped to [-127, 127] (so amax 2^-e lies in
 *            [256, 512)); stored as the E8M0 byte e + 127.  An all-zero block has scale byte 0 and zero elements.
 *   element  v 2^-e rounded to nearest-even into e4m3fn; |v 2^-e| > 448 saturates to +-448 (never NaN).
 *   padding  K is padded with zero bytes (scale byte 0) up to Kp, a multiple of 128.
 *   layout   elements [rows, Kp] uint8 (ldq bytes per row), scales [rows, Kp / 32] uint8 (lds bytes per row).
 * The scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) reads this layout directly: lane l of a 16-row operand tile holds
 * row l & 15, K bytes [16 (l >> 4), +16) and [64 + 16 (l >> 4), +16) of the 128-byte slab, and the scale of block l >> 4
 * of row l & 15 (measured with exact data: profiles/r07_mxfp8.md).  No other internal layout exists.
 */

/* LayerNorm (optional) + MXFP8 quantisation of x [rows, K] (ldx, `dtype`) in one row pass: q [rows, Kp] (ldq), s [rows,
 * Kp / 32] (lds).  gamma / beta f32 [K], both NULL for no LayerNorm (statistics in f32, two-pass, biased variance, eps inside
 * the sqrt, as anemoi_layer_norm).  Kp a multiple of 128 with K <= Kp <= 4096; ldq a multiple of 16 and >= Kp, lds >= Kp / 32;
 * columns K .. Kp-1 are written as zero bytes with scale byte 0. */
int anemoi_mx_quantize(int dtype, const void* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                       uint8_t* q, int64_t ldq, uint8_t* s, int64_t lds, int64_t rows, int K, int Kp,
                       anemoi_stream_t stream);

/* y = act(dequant(xq) dequant(wq)^T + bias) + residual on the scaled MFMA, f32 accumulation.
 *   xq [M, K] (ldxq) / xs [M, K / 32] (ldxs): MXFP8 activations; wq [N, K] / ws [N, K / 32]: MXFP8 weights, contiguous.
 *   bias f32 [N] or NULL; residual bf16 [M, N] (ldr) or NULL; act an ANEMOI_ACT_* code.
 *   out_mx = 0: y bf16 [M, N] (ldy), ys unused.
 *   out_mx = 1: the result quantised to MXFP8 as anemoi_mx_quantize would from its f32 value: y uint8 [M, round_up(N, 128)]
 *               (ldy bytes), ys [M, round_up(N, 128) / 32] (ldys); the padding columns are written as zeros, so the
 *               output is the next Linear's input as it stands.
 * Any M >= 0 (ragged tails included).  N a multiple of 16 (32 with out_mx) and K a multiple of 128, else
 * ANEMOI_ERR_UNSUPPORTED.  ldxq a multiple of 16 and ldxs of 4; ldy a multiple of 8 (bf16) or 16 (out_mx); ldr a multiple
 * of 8; operands 16-byte (scales 4-byte) aligned, else ANEMOI_ERR_INVALID. */
int anemoi_linear_mx(const uint8_t* xq, int64_t ldxq, const uint8_t* xs, int64_t ldxs, const uint8_t* wq,
                     const uint8_t* ws, const float* bias, const void* residual, int64_t ldr, int out_mx, void* y,
                     int64_t ldy, uint8_t* ys, int64_t ldys, int64_t M, int N, int K, int act, anemoi_stream_t stream);

/*
 * Split-bf16 ("bf16x3") Linear -- opt-in arithmetic of the f32 inference route (csrc/gemm_split.hip) and, through
 * anemoi_weight_grad_split below, of f32 training.
 *   split    v = hi + lo (+ a remainder below 2^-16 |v|): hi = bf16(v), lo = bf16(v - float(hi)), round to nearest even both.
 *   product  x W^T ~= x_hi W_hi^T + x_hi W_lo^T + x_lo W_hi^T on the bf16 MFMA, one f32 accumulator (x_lo W_lo^T dropped):
 *            ~4e-6 rms relative error per Linear (exact f32 kernel 3e-7, bf16 operands 2e-3).
 *   domain   finite values with |v| < 2^126: bf16(v) of a value next to the f32 maximum is infinite and v - hi then NaN, and
 *            +-infinity in x or W gives NaN where anemoi_linear gives +-infinity.  NaN in -> NaN out holds.
 */

/* The two bf16 planes w_hi, w_lo [N, K] (contiguous) of the f32 weight w [N, K] (ldw).  K a multiple of 32 (the f32 route's
 * K padding), w and the planes 16-byte aligned, ldw a multiple of 4, else ANEMOI_ERR_INVALID.  N = 0 is a no-op. */
int anemoi_split_weight(const float* w, int64_t ldw, void* w_hi, void* w_lo, int64_t N, int K, anemoi_stream_t stream);

/* y = act(x W^T + bias) + residual with the split product above.  x f32 [M, K] (ldx) is split inside the kernel; w_hi / w_lo
 * are the planes of anemoi_split_weight; bias f32 [N] or NULL; residual f32 [M, N] (ldr) or NULL; y f32 [M, N] (ldy); act an
 * ANEMOI_ACT_* code (GELU in the erf form of the f32 kernel).  Any M >= 0 and N > 0 (ragged tiles included); K a multiple of
 * 32, x and the planes 16-byte aligned and ldx a multiple of 4, else ANEMOI_ERR_INVALID (checked before any launch). */
int anemoi_linear_split(const float* x, int64_t ldx, const void* w_hi, const void* w_lo, const float* bias,
                        const float* residual, int64_t ldr, float* y, int64_t ldy, int64_t M, int N, int K, int act,
                        anemoi_stream_t stream);

/* Split-bf16 weight gradient (csrc/weight_grad_split.hip): the training counterpart of anemoi_linear_split, switched on by
 * ANEMOI_AMD_F32_TRAIN_LINEAR=bf16x3.
 *   partial[c][n * K + k] = sum over the rows m of chunk c of dy[m, n] * x[m, k]      (c = 0 .. ceil(M / chunk_rows) - 1)
 * with BOTH f32 operands split inside the kernel (hi = bf16(v), lo = bf16(v - hi)) and each product formed as
 * dy_hi^T x_hi + (dy_hi^T x_lo + dy_lo^T x_hi) on the bf16 MFMA with one f32 accumulator.  dy f32 [M, N] (ldy) and
 * x f32 [M, >= K] (ldx) are row-major and read as they lie (no transposed copies, no planes in HBM); rows at and behind M
 * and columns at and behind N / K are never read.  Chunk c covers rows c * chunk_rows .. min(M, (c + 1) * chunk_rows) - 1
 * and starts partial_stride floats behind chunk c - 1; the caller sums the chunks (anemoi_col_sum over
 * [chunks, partial_stride]): no atomics, the same bits on every run.  The bias gradient is not produced here
 * (anemoi_col_sum over dy: exact f32 sums).
 * Checked before any launch, else ANEMOI_ERR_INVALID: non-null pointers (dy / x may be NULL when M = 0); N and K
 * multiples of 4; ldy >= N, ldx >= K, both multiples of 4; dy, x and partial 16-byte aligned; chunk_rows a positive
 * multiple of 32; partial_stride >= N * K and a multiple of 4.  M = 0: partial[0 .. N * K) is zeroed by a memset and
 * nothing is launched. */
int anemoi_weight_grad_split(const float* dy, int64_t ldy, const float* x, int64_t ldx, float* partial,
                             int64_t partial_stride, int64_t M, int N, int K, int chunk_rows, anemoi_stream_t stream);

/*
 * The optimizer step (ABI v54, csrc/optim.hip, DESIGN.md section 7 "8f-10"): multi-tensor kernels over LISTS of f32 tensors.
 * The list is given as HOST arrays of n_tensors device pointers and lengths; the entry point copies them into the argument
 * blocks of its launches (at most anemoi_multi_tensor_max_tensors() tensors per launch, chunks of anemoi_multi_tensor_chunk()
 * elements per workgroup), so the arrays may be freed on return and nothing of them lives in device memory.  A tensor of
 * numel 0 is skipped (its pointers may be NULL); any other pointer need only be 4-byte aligned.  Fields an entry point does not
 * read stay 0 / NULL.  `struct_bytes` must be sizeof of the block (layout check across the FFI).
 * Checked before any launch, else ANEMOI_ERR_INVALID with a message naming the argument: a null block or pointer, a negative
 * count or length, a workspace that is too small, beta1 / beta2 outside [0, 1), eps < 0, lr < 0, weight_decay < 0.
 */
typedef struct anemoi_multi_tensor_args {
  int64_t struct_bytes;
  int64_t n_tensors;
  const int64_t* numel;     /* host [n_tensors] */
  void* const* params;      /* host [n_tensors] of device f32 pointers: anemoi_multi_adamw (read and written) */
  void* const* grads;       /* sumsq, adamw: read only; scale: scaled in place */
  void* const* exp_avg;     /* adamw (read and written) */
  void* const* exp_avg_sq;  /* adamw (read and written) */
  float* workspace;         /* sumsq: device, anemoi_multi_sumsq_workspace_floats(numel, n_tensors) floats */
  int64_t workspace_floats;
  float* sumsq;             /* sumsq: device f32 [1], the result */
  const float* consts;      /* adamw: device, the group's constants block (anemoi_adamw_constants) */
  const float* coef;        /* scale: device f32 [1] */
  double beta1, beta2, eps; /* adamw: as torch takes them; the kernel sees f32(1 - beta1), f32(beta2), f32(1 - beta2), f32(eps) */
} anemoi_multi_tensor_args;

int anemoi_multi_tensor_max_tensors(void);
int anemoi_multi_tensor_chunk(void);

/* sumsq[0] = sum over the list of g^2, two deterministic stages without atomics: one f32 partial per (tensor, chunk) in list
 * order to `workspace`, then one workgroup that adds the partials in f64 and writes the f32-rounded total.  The result is a
 * function of the values and of the ordered list of lengths alone (csrc/optim.hip states every sum order).  An empty list
 * gives 0.  Trail: "sumsq". */
int64_t anemoi_multi_sumsq_workspace_floats(const int64_t* numel, int64_t n_tensors);
int anemoi_multi_sumsq(const anemoi_multi_tensor_args* args, anemoi_stream_t stream);

/*
 * The scalars of one AdamW step, by one tiny kernel; nothing is read back.  consts is device f32 [(1 + n_groups) * 8]:
 *   block 0       norm = sqrt(sumsq), clip = min(1, max_norm / (norm + 1e-6)) (1 without max_norm), finite, skip, 0 ...
 *   block 1 + g   clip, 1 - lr wd, lr / (1 - beta1^t), sqrt(1 - beta2^t), skip, lr, t, 0         t = step[g] + 1
 * (bias corrections and the decay factor evaluated in f64, rounded once).  step: host [n_groups] of device f32 [1] counters,
 * advanced here; lr_dev: NULL, or host [n_groups] of device f32 [1] learning rates, an entry may be NULL: lr[g] by value.
 * sumsq NULL: no norm was taken (clip = 1, finite).  skip_nonfinite with a non-finite norm: no counter is advanced, the device
 * int64 `skipped` (may be NULL) is advanced by one and every block carries skip = 1, which turns anemoi_multi_adamw into a
 * no-op.  n_groups = 0 writes block 0 alone (the stand-alone clip reads its coefficient there).  Trail: "consts".
 */
typedef struct anemoi_adamw_constants_args {
  int64_t struct_bytes;
  int64_t n_groups;
  void* const* step;
  void* const* lr_dev;
  const double* lr;           /* host [n_groups] each */
  const double* beta1;
  const double* beta2;
  const double* weight_decay;
  const float* sumsq;         /* device, or NULL */
  void* skipped;              /* device int64 [1], or NULL */
  float* consts;              /* device f32 [(1 + n_groups) * 8] */
  float max_norm;
  int32_t has_max_norm;
  int32_t skip_nonfinite;
  int32_t reserved;
} anemoi_adamw_constants_args;

int anemoi_adamw_constants(const anemoi_adamw_constants_args* args, anemoi_stream_t stream);

/*
 * One pass over params, grads, exp_avg, exp_avg_sq (16 bytes read, 12 written per element), torch.optim.AdamW's arithmetic
 * with the clip applied on load -- grads are NOT modified:
 *   g' = clip g;  m <- m + (g' - m)(1 - beta1);  v <- beta2 v + (1 - beta2) g'^2
 *   p  <- p (1 - lr wd) - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * in correctly rounded f32 operations (no fast sqrt or division).  `consts` points at the group's block (block 1 + g).  Under
 * its skip flag nothing is read or written.  Trail (only while one is armed): "params[i]", "exp_avg[i]", "exp_avg_sq[i]" per
 * non-empty tensor i of the list, each as [1, numel].
 */
int anemoi_multi_adamw(const anemoi_multi_tensor_args* args, anemoi_stream_t stream);

/* grads[i] <- coef[0] * grads[i] in place, coef on the device.  Trail: "grads[i]" per non-empty tensor. */
int anemoi_multi_scale(const anemoi_multi_tensor_args* args, anemoi_stream_t stream);

/*
 * Weight averaging and the learning-rate schedule on the device (ABI v55, csrc/average.hip, DESIGN.md section 7 "8f-11"), on the
 * multi-tensor frame above: lists as HOST arrays of device f32 pointers and lengths, anemoi_multi_tensor_max_tensors() tensors
 * per launch, a tensor of numel 0 skipped, an empty list launches nothing, any pointer 4-byte aligned.  Each entry point has its
 * own argument block with the `struct_bytes` layout check.
 * Checked before any launch, else ANEMOI_ERR_INVALID with a message naming the argument: a null block or pointer, a negative
 * count or length, decay outside [0, 1), every < 1, start_step < 0, warmup_steps < 0, total_steps < 1, a negative learning
 * rate, more than 32 groups.
 */
#define ANEMOI_AVERAGE_EMA 0
#define ANEMOI_AVERAGE_SWA 1

/*
 * The scalars of one averaging update, by one tiny kernel; nothing is read back.  avg is device f32 [4] = {w, active, copy,
 * n_after}.  n = n_averaged[0] (a device f32 counter, advanced here when active); step (may be NULL): the optimizer's device
 * f32 step counter, steps COMPLETED (read after anemoi_adamw_constants advanced it); skip (may be NULL): the optimizer's
 * list-wide skip flag (consts[3] of anemoi_adamw_constants).
 *   active = !skip && (step == NULL || (t >= start_step && (t - start_step) % every == 0))
 *   inactive: w = 0, n_averaged keeps its value.  Active: n == 0: copy = 1 (w = 1);
 *   EMA: w = 1 - d, d = use_warmup ? min(decay, (1 + n) / (10 + n)) : decay;   SWA: w = 1 / (n + 1)
 * (w evaluated in f64, rounded once).  Trail: "avg".
 */
typedef struct anemoi_average_constants_args {
  int64_t struct_bytes;
  float* n_averaged;  /* device f32 [1] */
  const float* step;  /* device f32 [1], or NULL */
  const float* skip;  /* device f32 [1], or NULL */
  float* avg;         /* device f32 [4] */
  double decay;       /* EMA: in [0, 1) */
  int64_t start_step; /* >= 0 */
  int64_t every;      /* >= 1 */
  int32_t kind;       /* ANEMOI_AVERAGE_EMA / ANEMOI_AVERAGE_SWA */
  int32_t use_warmup;
} anemoi_average_constants_args;

int anemoi_average_constants(const anemoi_average_constants_args* args, anemoi_stream_t stream);

/*
 * shadow[i] <- the average of shadow[i] and params[i] under the block `avg` of anemoi_average_constants, one pass (8 bytes read,
 * 4 written per element; params are only read): inactive: nothing is read or written; copy: shadow <- params bit for bit;
 * else shadow <- fmaf(params - shadow, w, shadow) in correctly rounded f32 (two roundings).  Trail: "shadow[i]" per non-empty
 * tensor i of the list, as [1, numel].
 */
typedef struct anemoi_multi_average_args {
  int64_t struct_bytes;
  int64_t n_tensors;
  const int64_t* numel; /* host [n_tensors] */
  void* const* params;  /* host [n_tensors] of device f32 pointers, read only */
  void* const* shadow;  /* host [n_tensors] of device f32 pointers, read and written */
  const float* avg;     /* device f32 [4] */
} anemoi_multi_average_args;

int anemoi_multi_average(const anemoi_multi_average_args* args, anemoi_stream_t stream);

/* a[i] <-> b[i], element for element and exactly (bit patterns move, no arithmetic); the two lists must not overlap.
 * Trail: "a[i]", then "b[i]", per non-empty tensor. */
typedef struct anemoi_multi_swap_args {
  int64_t struct_bytes;
  int64_t n_tensors;
  const int64_t* numel; /* host [n_tensors] */
  void* const* a;       /* host [n_tensors] of device f32 pointers each */
  void* const* b;
} anemoi_multi_swap_args;

int anemoi_multi_swap(const anemoi_multi_swap_args* args, anemoi_stream_t stream);

/*
 * lr[g][0] <- the schedule of group g at t = step[g][0] (the group's device f32 step counter, steps completed), by one tiny
 * kernel, at most 32 groups; evaluated in f64 and rounded once:
 *   t < warmup_steps:  warmup_start + t (base - warmup_start) / warmup_steps
 *   else, tc = warmup_prefix ? t - warmup_steps : t:   tc < total_steps: lr_min + 0.5 (base - lr_min)(1 + cos(pi tc / total_steps))
 *                                                      else lr_min
 * warmup_prefix = 1 is torch's SequentialLR(LinearLR, CosineAnnealingLR); warmup_prefix = 0 with warmup_start = 0 restates
 * timm's CosineLRScheduler as anemoi-training configures it.  Trail: "lr[g]" per group.
 */
typedef struct anemoi_lr_schedule_args {
  int64_t struct_bytes;
  int64_t n_groups;
  void* const* step;            /* host [n_groups] of device f32 [1], read only */
  void* const* lr;              /* host [n_groups] of device f32 [1], written */
  const double* base;           /* host [n_groups] each; >= 0 */
  const double* lr_min;         /* >= 0 */
  const double* warmup_start;   /* >= 0 */
  const int64_t* warmup_steps;  /* >= 0 */
  const int64_t* total_steps;   /* >= 1 */
  const int32_t* warmup_prefix; /* 0 / 1 */
} anemoi_lr_schedule_args;

int anemoi_lr_schedule(const anemoi_lr_schedule_args* args, anemoi_stream_t stream);

/*
 * Launch trail -- opt-in per-launch output digests (csrc/trail.hip).
 *
 * While a trail is armed on the calling thread, every entry point of this header that writes device memory appends one
 * 32-byte record per OUTPUT buffer it wrote (workspaces are not recorded), computed on the device by a read-only kernel on
 * the entry point's own stream, in call order; the block-level entry points record through the entry points they call.
 * Record i of the buffer given to anemoi_trail_begin, for a [rows, cols] matrix with bit patterns b (zero-extended):
 *   bytes  0.. 7  digest    u64  sum over i = r * cols + c of (b_i + 1) * m(i) mod 2^64,
 *                                m(i) = ((i + 1) * 0x9E3779B97F4A7C15 mod 2^64) | 1   (padding beyond cols is never read)
 *   bytes  8..15  nonfinite u64  number of NaN / +-Inf elements (0 for the integer dtypes)
 *   bytes 16..19  absmax    u32  f32 bits of the largest |x| over the finite elements (bf16 widened), 0 if there is none
 *   bytes 20..31  reserved, zero
 * Integer arithmetic only: a record is the same on every run and can be recomputed on the host.  The records are complete
 * once the streams the entry points ran on have been synchronised.  Unarmed, an entry point pays one thread-local load.
 * Limits: the state is per host thread; launches captured into a HIP graph cannot be recorded (ANEMOI_ERR_UNSUPPORTED).
 */

/* Arm the trail of the calling thread: `records` is a device buffer of capacity * 32 bytes on the device the entry points
 * will run on.  A null buffer, capacity <= 0 or a trail already armed: ANEMOI_ERR_INVALID (checked before any device call). */
int anemoi_trail_begin(void* records, int64_t capacity);

/* Disarm it.  n_written records were written (at most `capacity`); n_dropped further ones were counted and never written.
 * Either pointer may be NULL.  ANEMOI_ERR_INVALID when no trail is armed. */
int anemoi_trail_end(int64_t* n_written, int64_t* n_dropped);

/* Host-side description of record i of this thread's last trail (valid until the next anemoi_trail_begin on the thread):
 * name "<entry point>:<output>", e.g. "anemoi_mhsa:out" and "anemoi_mhsa:lse"; dtype an ANEMOI_F32 / BF16 / I32 / U8 code. */
int anemoi_trail_entry(int64_t i, const char** name, int* dtype, int64_t* rows, int64_t* cols);

/* The hook the entry points use, for callers that want their own buffers on the trail: one record of the [rows, cols]
 * matrix at `ptr` (leading dimension ld elements, aligned to its element size) under `name`.  No trail armed: ANEMOI_OK,
 * nothing is done.  Armed while `stream` is being captured: ANEMOI_ERR_UNSUPPORTED. */
int anemoi_trail_note(const char* name, int dtype, const void* ptr, int64_t ld, int64_t rows, int64_t cols,
                      anemoi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ANEMOI_AMD_H */
