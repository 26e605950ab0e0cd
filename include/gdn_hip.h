/*
 * gdn_hip.h — C ABI of libgdn_hip.so, the MI355X (gfx950) implementation of GDN's
 * graph-attention hot path.
 *
 * The reference (SchlomoFeng/GDN) has no FFI: its boundary is the Python nn.Module
 * `GDN.forward(data, org_edge_index)` (models/GDN.py:122-187).  gdn_amd/model.py keeps
 * that Python API and calls the entry points below through ctypes; each entry point
 * replaces the reference lines cited at its declaration.  INTEGRATION.md shows the
 * binding a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - the caller allocates every output; the library owns nothing and keeps no state
 *     between calls (it caches only immutable device properties);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls only
 *     enqueue work, never synchronise, never allocate: they are hipGraph-capturable;
 *   - return value: GDN_OK (0) or a negative GDN_ERR_* code; nothing is thrown;
 *   - tensors are dense, row-major, fp32 unless stated; "BN rows" means batch*n rows in
 *     window-major order (row = b*n + sensor), the layout of models/GDN.py:130;
 *   - re-entrant across distinct streams.
 *
 * Supported shapes: 1 <= d <= 256; 1 <= w <= 1024; 1 <= k <= n <= 4096 with k+1 <= 1024.
 * Embedding widths other than 16, 32, 64 and 128 (ANY-WIDTH form, gdn_any_width.hip) run the staged fp32 entry points
 *   only, at every n, w, k above: gdn_topk_graph (scalar row reads where d % 4 != 0), gdn_node_terms,
 *   gdn_project_fwd[_wide] / _series, gdn_attn_aggregate_fwd[_wide], gdn_head_fwd, gdn_head_train_* (all four pairs),
 *   gdn_attn_aggregate_bwd[_wide], gdn_project_bwd[_partials], gdn_terms_bwd[_acc] and their workspace queries.  Kernels
 *   run on the padded width (16, 32, 64, 128 or 256) with columns >= d masked; xlin, z and their gradients stay dense
 *   [BN, d].  gdn_tile_fits, gdn_fused_plan_bytes and gdn_train_supported return 0, the fused / bf16 entry points
 *   and gdn_train_finish GDN_ERR_UNSUPPORTED; no projection, aggregate or head kernel takes d > 256.
 * Windows longer than 64 ticks (LONG-WINDOW form, w = 65..1024) run the staged entry points only: gdn_node_terms,
 *   gdn_project_fwd[_wide] / _series (fp32 matrix-core projection, exact fp32, no range limit), gdn_project_bwd[_partials],
 *   gdn_terms_bwd[_acc]; everything after xlin depends on n, d, k only and takes the forms below.  gdn_tile_fits,
 *   gdn_fused_plan_bytes and gdn_train_supported return 0, the fused / bf16 entry points GDN_ERR_UNSUPPORTED.
 * Route table — the kernel FAMILY of every stage of the graph layer, chosen by the library, never by the caller.
 *   gdn_route.hip is the one place that decides it and gdn_kernel_family the query; rules apply in the order written,
 *   inside the supported shapes above (outside them: NONE, and the entry point returns GDN_ERR_UNSUPPORTED).
 *   "dense shape" = n <= 127, d = 64, w <= 32, k <= 63.  Dimensions a stage does not depend on are ignored.
 *     PROJECT (n, w, d)       gdn_project_fwd[_wide|_series|_bf16]:
 *                             BF16: DENSE at a dense shape, else NONE; ANY at d not 16/32/64/128; LONG at w > 64;
 *                             SERIES: LARGE; DENSE at a dense shape unless WIDE; TILE where the xlin tile fits; LARGE.
 *     AGGREGATE (n, d, k)     gdn_attn_aggregate_fwd[_wide|_bf16]: as PROJECT without the LONG and SERIES rules.
 *     ATTN_BWD (n, d, k)      gdn_attn_aggregate_bwd[_wide]: ANY; DENSE at a dense shape unless WIDE; TILE in one of
 *                             three sub-forms (below); LARGE.
 *     PROJECT_BWD (n, w, d)   gdn_project_bwd[_partials]: ANY; LONG; TILE.
 *     TERMS (w, d)            gdn_node_terms, gdn_terms_bwd[_acc]: LONG at w > 64; ANY; TILE (gdn_node_terms runs one
 *                             kernel for ANY and TILE, gdn_terms_bwd one for LONG and ANY).
 *     HEAD (d)                gdn_head_fwd: ANY; TILE.
 *     FUSED (n, w, d, k)      gdn_forward_fused[_series|_bf16|_gated]: NONE at d not 16/32/64/128 or w > 64; DENSE at a
 *                             dense shape (also d = 128) unless WIDE (the _gated forms); TILE where the tile fits
 *                             (SERIES: and the projection runs on the matrix cores); NONE — one launch, no workspace.
 *   The families:
 *   TILE — the window's working set in the 160 KB of LDS of one CU:
 *     forward (staged and fused): the xlin tile (n+1)*dc*4 bytes, dc = d (d = 128: 64, two column slices) —
 *       n up to ~610 at d = 64/128, ~1180 at d = 32, ~2200 at d = 16 (gdn_tile_fits: the fused forward);
 *     backward (gdn_attn_aggregate_bwd), three sub-forms: that tile at full d PLUS two [n, pitch] fp32 tables and the
 *       lists in LDS (GDN_BWD_TABLES_LDS) — n up to ~250 at d = 64 with k = 30; beyond that the tables go through the
 *       caller's workspace and only the tile must fit (GDN_BWD_TABLES_GLOBAL); d = 128 walks two 64-column slices
 *       when the full tile does not fit (GDN_BWD_SLICED);
 *   LARGE — where the tile refuses (n up to 4096): streaming kernels that keep only the window's s_i / s_j and one
 *     list per wave in LDS and gather the source rows of xlin (forward) / d_z (backward) from global memory; fp32 only,
 *     bitwise reproducible;
 *   DENSE — the matrix-core kernels (every factor as two 16-bit terms: the range guard below); the staged
 *     bf16-storage entry points exist only there;
 *   LONG, ANY — the long-window and any-width forms above.
 *   gdn_tile_fits, gdn_train_supported (the tile kernels take every stage of a training step),
 *   gdn_attn_aggregate_bwd_uses_reverse and the two backward workspace queries are reads of this table.
 *   Diagnostic A/B overrides, read once per process: GDN_FUSED_PATH=valu (no DENSE at any stage, bf16 storage aside),
 *   GDN_BWD_PATH=valu (no DENSE at ATTN_BWD), GDN_BWD_SLICED=1 (ATTN_BWD at d = 128: GDN_BWD_SLICED or NONE).
 * anything else returns GDN_ERR_UNSUPPORTED (never a silent fallback).
 */
#ifndef GDN_HIP_H
#define GDN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDN_OK 0
#define GDN_ERR_ARG (-1)          /* null pointer / non-positive dimension                 */
#define GDN_ERR_LAUNCH (-2)       /* hipGetLastError() != hipSuccess after the launch      */
#define GDN_ERR_UNSUPPORTED (-3)  /* shape outside the supported set above                 */

#define GDN_ABI_VERSION 23
int gdn_abi_version(void);

/* Number of u16 slots per neighbour-list row for a given k: (k+1) rounded up to 16. */
int gdn_nbr_pitch(int k);

/* ---- sensor graph -----------------------------------------------------------------
 * Replaces models/GDN.py:148-159 (cosine matrix, top-k) and the per-forward edge-list
 * build :161-165 + get_batch_edge_index :15-24 + the self-loop strip/append of
 * models/graph_layer.py:61-63.  One neighbour list per sensor, shared by every window:
 *   topk_idx[n,k]  int64, descending cosine, ties -> lower index, NaN ranks highest
 *                  (= model.learned_graph);
 *   nbr[n,pitch]   u16: the top-k entries != i in rank order, then i itself, then
 *                  padding = the sentinel index n; pitch = gdn_nbr_pitch(k);
 *   deg[n]         int32: number of valid entries (k, or k+1 when i is not in its own
 *                  top-k);
 *   cos_out[n,n]   optional (may be NULL) cosine matrix for inspection.               */
int gdn_topk_graph(const float* emb, int n, int d, int k,
                   int64_t* topk_idx, uint16_t* nbr, int32_t* deg, float* cos_out, void* stream);

/* Same neighbour-list build from a GIVEN top-k table (kernel-level parity with an
 * injected graph; also lets a caller reuse a graph learned elsewhere).                */
int gdn_graph_from_topk(const int64_t* topk_idx, int n, int k,
                        uint16_t* nbr, int32_t* deg, void* stream);

/* ---- per-forward constants ----------------------------------------------------------
 * The attention logit of models/graph_layer.py:91-103 is separable:
 *   pi(i<-j) = [xlin_i.att_i + v_i.att_em_i] + [xlin_j.att_j + v_j.att_em_j]
 * and xlin = x.lin^T, so each bracket is  x_row . a + c[sensor]  with
 *   a_i = lin^T att_i  [w],  c_i[s] = v_s . att_em_i  [n]   (same for _j).
 * node_terms receives [a_i(P) | a_j(P) | c_i(n) | c_j(n)] (a_* zero padded to P = gdn_terms_pitch(w): 64 for
 * w <= 64, round_up(w, 64) above).                                                                                */
int gdn_node_terms(const float* lin_w, const float* att_i, const float* att_j,
                   const float* att_em_i, const float* att_em_j, const float* emb,
                   int n, int d, int w, float* node_terms, void* stream);

/* gdn_terms_pitch: P of the node-terms layout above (64 for 1 <= w <= 64, round_up(w, 64) for w <= 1024), 0 for an
 * unsupported w.  Host only, no launch.                                                                           */
int gdn_terms_pitch(int w);

/* gdn_topk_graph + gdn_node_terms as ONE launch (w <= 64) (a training step rebuilds both from the parameters it is about
 * to use; they are independent of each other): same outputs, no cos_out.                              */
int gdn_topk_graph_terms(const float* emb, int n, int d, int k, int64_t* topk_idx, uint16_t* nbr,
                         int32_t* deg, const float* lin_w, const float* att_i, const float* att_j,
                         const float* att_em_i, const float* att_em_j, int w, float* node_terms,
                         void* stream);

/* Eval-mode BatchNorm1d folded to y = x*scale + shift (models/GDN.py:77, :179 under
 * model.eval()): scale = weight/sqrt(var+eps), shift = bias - mean*scale.
 * affine receives [scale(c) | shift(c)].                                               */
int gdn_bn_fold(const float* weight, const float* bias, const float* running_mean,
                const float* running_var, float eps, int c, float* affine, void* stream);

/* ---- staged forward (training + inspection path) ------------------------------------
 * gdn_project_fwd: models/graph_layer.py:56 (xlin = x lin^T) plus the two per-node
 * attention scalars.  x[BN,w] -> xlin[BN,d], s_i[BN], s_j[BN].                         */
int gdn_project_fwd(const float* x, const float* lin_w, const float* node_terms,
                    int batch, int n, int w, int d,
                    float* xlin, float* s_i, float* s_j, void* stream);

/* gdn_project_fwd_series: gdn_project_fwd on windows read straight from the raw series[n, series_len] (the
 * layout of gdn_forward_fused_series): window b = series[:, first+b : first+b+w]; requires first + batch - 1 + w
 * <= series_len.  Runs the large-form streaming kernel at every shape (the same bits gdn_project_fwd gives
 * on the same windows where the tile form refuses): the eval path of graphs beyond the tile without a
 * [B, n, w] copy.                                                                                            */
int gdn_project_fwd_series(const float* series, int series_len, int first, const float* lin_w,
                           const float* node_terms, int batch, int n, int w, int d,
                           float* xlin, float* s_i, float* s_j, void* stream);

/* gdn_tile_fits: 1 when the tile form of the forward takes (n, w, d, k) — the one-launch gdn_forward_fused and
 * its plans — 0 when only the staged entry points (large form beyond the tile) do.  Host only, no launch.      */
int gdn_tile_fits(int n, int w, int d, int k);

/* gdn_kernel_family: the route table above as a query (host only, no launch) — the GDN_FAMILY_* that the entry
 * points of `stage` run at (n, w, d, k) under `flags`, in the low 8 bits; for GDN_STAGE_ATTN_BWD with family TILE the
 * GDN_BWD_* sub-form in bits 8 and up (it decides the layout gdn_attn_aggregate_bwd_workspace_bytes sizes).          */
#define GDN_FAMILY_NONE 0
#define GDN_FAMILY_DENSE 1
#define GDN_FAMILY_TILE 2
#define GDN_FAMILY_LARGE 3
#define GDN_FAMILY_LONG 4
#define GDN_FAMILY_ANY 5
#define GDN_STAGE_PROJECT 0
#define GDN_STAGE_AGGREGATE 1
#define GDN_STAGE_ATTN_BWD 2
#define GDN_STAGE_PROJECT_BWD 3
#define GDN_STAGE_TERMS 4
#define GDN_STAGE_HEAD 5
#define GDN_STAGE_FUSED 6
#define GDN_ROUTE_WIDE 1     /* the `_wide` / `_gated` entry points: never DENSE                          */
#define GDN_ROUTE_BF16 2     /* the `_bf16` entry points: x / xlin / z stored as bf16                     */
#define GDN_ROUTE_SERIES 4   /* the `_series` entry points: windows read from the raw series (PROJECT, FUSED) */
#define GDN_BWD_TABLES_LDS 0
#define GDN_BWD_TABLES_GLOBAL 1
#define GDN_BWD_SLICED 2
int gdn_kernel_family(int stage, int n, int w, int d, int k, int flags);

/* gdn_tile_forward_form: the form of the TILE kernel that the staged forward launches at (n, w, d, k), whatever the
 * route says (the `_wide` entry points run TILE at dense shapes).  Host only, no launch; the numbers come from the code
 * that dispatches.  stage = GDN_STAGE_PROJECT (k ignored) or GDN_STAGE_AGGREGATE (w ignored); -1 for any other stage
 * and for a shape the tile refuses (the fused launch depends on the batch and the CU count and is not reported).
 *   bits 0-3    PROJ: the projection form — 0 / 1: fp32 VALU, window padded to 8 / to a multiple of 16 ticks;
 *               2 / 3 / 4: matrix cores, whole window staged (n w <= 8 threads, w <= 16 / above it / w > 16);
 *               5: matrix cores, x in registers, the LDS x tile one row chunk at a time.  AGGREGATE: 1;
 *   bits 4-7    LST: the list form — lists in LDS at pitch 16 (1), 32 (2), 48..80 (5); lists read from global at
 *               pitch <= 80 (6); any longer list (0).  PROJECT: 0;
 *   bits 8-11   threads / 256 (1 or 2);
 *   bit 12      two 64-column slices (d = 128 beyond the full tile);
 *   bit 13      neighbour lists in LDS;
 *   bit 14      lin weights in LDS (fp32 VALU projections of small tiles);
 *   bit 15      x tile chunked: it holds fewer rows than the window has sensors;
 *   bits 16-30  the rows of the x tile (0 for AGGREGATE).
 * GDN_THREADS and GDN_NO_MFMA act on it as on the launch.  Additive diagnostic entry point: the ABI version does not
 * move.                                                                                                           */
int gdn_tile_forward_form(int stage, int n, int w, int d, int k);

/* gdn_attn_aggregate_fwd: models/graph_layer.py:65-74,82-117 + PyG propagate / softmax:
 * LeakyReLU(0.2) logits, softmax over each target's incoming edges (max-subtract, exp,
 * /(sum+1e-16)), alpha-weighted sum of source rows, + bias.
 *   z[BN,d]          aggregate incl. bias (the GraphLayer output);
 *   alpha[BN,pitch]  optional (NULL to skip): attention weight of nbr slot p of each
 *                    target row (0 in padding) — att_weight_1 in dense form.           */
int gdn_attn_aggregate_fwd(const float* xlin, const float* s_i, const float* s_j,
                           const uint16_t* nbr, const int32_t* deg, const float* bias,
                           int batch, int n, int d, int k,
                           float* z, float* alpha, void* stream);

/* gdn_head_fwd: models/GDN.py:77-79 (BN+ReLU), :175-180 (x embedding, BN+ReLU), eval
 * dropout = identity (:182), OutLayer with out_layer_num == 1 (:27-56) = Linear(d->1).
 * bn1_affine / bn2_affine come from gdn_bn_fold.  z[BN,d] -> out[BN].
 * h2 (optional, NULL to skip) receives the [BN,d] input of the OutLayer (needed when
 * out_layer_num > 1: the MLP then runs in gdn_mlp_fwd).                                  */
int gdn_head_fwd(const float* z, const float* emb, const float* bn1_affine,
                 const float* bn2_affine, const float* out_w, const float* out_b,
                 int batch, int n, int d, float* out, float* h2, void* stream);

/* ---- OutLayer MLP, out_layer_num > 1 (models/GDN.py:27-56,:183), eval mode -------------
 * h2[rows, d_in] (the h2 output of gdn_head_fwd) -> [Linear(K->hidden), BatchNorm1d(hidden) with
 * running statistics, ReLU] x (layers-1) -> Linear(hidden->1) -> out[rows], one launch, on the
 * 16-bit matrix cores with the fp32-grade two-term split (activations never leave registers).
 * The weights enter through a PLAN (BatchNorm folded, split, reordered), built once per parameter
 * update: gdn_mlp_plan_layer for hidden layer `layer` = 0 .. layers-2 (weight[hidden, K],
 * K = d_in for layer 0, hidden otherwise; bias[hidden]; the BatchNorm1d behind it), then
 * gdn_mlp_plan_out for the final Linear (weight[hidden], bias[1]).
 * Supported: layers 2..8, hidden <= 256, d_in in {16,32,64,128}; gdn_mlp_plan_bytes returns 0
 * otherwise.                                                                                */
long long gdn_mlp_plan_bytes(int d_in, int hidden, int layers);
int gdn_mlp_plan_layer(const float* weight, const float* bias, const float* bn_weight,
                       const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                       int d_in, int hidden, int layers, int layer, void* plan, void* stream);
int gdn_mlp_plan_out(const float* weight, const float* bias, int d_in, int hidden, int layers,
                     void* plan, void* stream);
int gdn_mlp_fwd(const float* h2, const void* plan, int rows, int d_in, int hidden, int layers,
                float* out, void* stream);

/* gdn_head_mlp_fwd: gdn_head_fwd (the h2 output) and gdn_mlp_fwd as ONE launch: z[BN, d] -> out[BN], BN = batch * n.
 * The head (models/GDN.py:77-79,175-180: BN+ReLU, x embedding row BN % n, BN+ReLU) is computed in registers while
 * the chain's first matrix operand is built, by the operation sequence gdn_head_fwd uses, so h2 never exists in
 * memory and the result equals gdn_mlp_fwd(gdn_head_fwd(z).h2) bit for bit.  The two affine tables (gdn_bn_fold)
 * are staged in LDS once per workgroup; the embedding rows are read per lane.  Same plan and same supported set
 * as gdn_mlp_fwd (gdn_mlp_plan_bytes(d, hidden, layers) != 0), anything else GDN_ERR_UNSUPPORTED; z and emb
 * 16-byte aligned (GDN_ERR_ARG otherwise, like a null pointer or a non-positive size), all before any launch.   */
int gdn_head_mlp_fwd(const float* z, const float* emb, const float* bn1_affine, const float* bn2_affine,
                     const void* plan, int batch, int n, int d, int hidden, int layers,
                     float* out, void* stream);

/* ---- train-mode head (out_layer_num == 1) -------------------------------------------
 * gdn_head_train_fwd: the same chain as gdn_head_fwd under model.train(): both BatchNorms
 * normalise by the statistics of this batch (models/GDN.py:77-79 GNNLayer.bn, :178-180
 * bn_outlayer_in — biased variance over all batch*n rows) and update running_mean /
 * running_var (momentum, unbiased variance) / num_batches_tracked; dropout (:182) is applied
 * as the caller's mask: either mask[BN,d] fp32 multipliers (0 or 1/(1-p)) or keep[BN,d] bytes
 * (1 kept / 0 dropped, multiplier = keep * keep_scale: a quarter of the traffic); both NULL =
 * no dropout; OutLayer Linear(d->1).
 *   stats (out)  gdn_head_train_stats_bytes(d) bytes: the column sums of z, z^2, h1, h1^2 — opaque,
 *                kept for the backward.  Sums across workgroups are EXACT (260-bit fixed point, 64-bit
 *                integer atomics, see gdn_exact_sum): statistics and gradients do not depend on the
 *                order the workgroups finish in.
 *   running_* / batches*     may be NULL (track_running_stats off).
 * Three streaming passes over z; nothing [BN,d]-sized is stored.  batch*n >= 2.             */
long long gdn_head_train_stats_bytes(int d);
/* The accumulator of the training statistics on its own: out[0] = the sum of x[0..count) (device fp64, count <=
 * 2048), exact up to the final conversion to fp64 (values are held to 2^-130, NaN / inf / |x| >= 2^130 give NaN).
 * workspace: gdn_exact_sum_workspace_bytes() bytes, zero on entry, left zero.  Exported for tests.          */
long long gdn_exact_sum_workspace_bytes(void);
int gdn_exact_sum(const double* x, int count, void* workspace, double* out, void* stream);
int gdn_head_train_fwd(const float* z, const float* emb, const float* bn1_w, const float* bn1_b,
                       const float* bn2_w, const float* bn2_b, const float* lin_w,
                       const float* lin_b, const float* mask, const uint8_t* keep,
                       float keep_scale, int batch, int n, int d,
                       float eps1, float eps2, float momentum1, float momentum2,
                       float* running_mean1, float* running_var1, long long* batches1,
                       float* running_mean2, float* running_var2, long long* batches2,
                       double* stats, float* out, void* stream);

/* gdn_head_train_bwd: gradients of gdn_head_train_fwd given d_out[BN] (what autograd derives
 * for models/GDN.py:77-79,:175-184 in training): d_z[BN,d], d_emb[n,d] (the head's share of the
 * embedding gradient), BatchNorm weight/bias gradients [d], OutLayer Linear d_lin_w[d] /
 * d_lin_b[1].  workspace: gdn_head_train_workspace_bytes(n, d) bytes of scratch.            */
long long gdn_head_train_workspace_bytes(int n, int d);
int gdn_head_train_bwd(const float* d_out, const float* z, const float* emb, const float* bn1_w,
                       const float* bn1_b, const float* bn2_w, const float* bn2_b,
                       const float* lin_w, const float* mask, const uint8_t* keep,
                       float keep_scale, const double* stats,
                       int batch, int n, int d, float eps1, float eps2, double* workspace,
                       float* d_z, float* d_emb, float* d_bn1_w, float* d_bn1_b, float* d_bn2_w,
                       float* d_bn2_b, float* d_lin_w, float* d_lin_b, void* stream);

/* The same two passes with the dropout mask of models/GDN.py:114,182 DRAWN INSIDE the kernels instead of
 * read from a tensor: element e of training step t is dropped iff mix32(e, seed, t) < p_drop * 2^32, kept
 * values are scaled by 1/(1-p_drop).  rng_seed_step = {seed, t} (two int64 in device memory); the forward
 * and the backward of one step must see the same pair (gdn_adam_step increments t after the backward).
 * Stateless draw: nothing [BN,d]-sized is written or read for the mask.  It is NOT torch's Philox stream:
 * reproducing a given torch mask needs the mask/keep arguments of the plain entry points.             */
int gdn_head_train_fwd_rng(const float* z, const float* emb, const float* bn1_w, const float* bn1_b,
                           const float* bn2_w, const float* bn2_b, const float* lin_w,
                           const float* lin_b, const long long* rng_seed_step, float p_drop,
                           int batch, int n, int d, float eps1, float eps2, float momentum1,
                           float momentum2, float* running_mean1, float* running_var1,
                           long long* batches1, float* running_mean2, float* running_var2,
                           long long* batches2, double* stats, float* out, int buffers_zeroed,
                           void* stream);
int gdn_head_train_bwd_rng(const float* d_out, const float* z, const float* emb, const float* bn1_w,
                           const float* bn1_b, const float* bn2_w, const float* bn2_b,
                           const float* lin_w, const long long* rng_seed_step, float p_drop,
                           const double* stats, int batch, int n, int d, float eps1, float eps2,
                           double* workspace, float* d_z, float* d_emb, float* d_bn1_w, float* d_bn1_b,
                           float* d_bn2_w, float* d_bn2_b, float* d_lin_w, float* d_lin_b,
                           int buffers_zeroed, void* stream);
/* gdn_head_train_fwd_rng with the loss folded in (train.py:20-23,70-72: F.mse_loss + the first step of
 * loss.backward()): the last forward pass also writes d_out = 2 (out - y) / (batch n) and loss[0] =
 * mean((out - y)^2) — per-workgroup fp64 partials added in a fixed order by the last workgroup to finish, as
 * gdn_mse_loss_grad does, without its launch.  mse_workspace: gdn_head_mse_workspace_bytes(), zero-filled once; every call leaves all of it zero.
 * (Measured on MI355X at 512 windows: 5 us slower than the separate launch — every one of the 512 workgroups
 * pays the block reduction and the ticket; harness.NativeTrainStep uses it only with GDN_FUSE_MSE=1.)        */
long long gdn_head_mse_workspace_bytes(void);
int gdn_head_train_fwd_rng_mse(const float* z, const float* emb, const float* bn1_w, const float* bn1_b,
                               const float* bn2_w, const float* bn2_b, const float* lin_w,
                               const float* lin_b, const long long* rng_seed_step, float p_drop,
                               int batch, int n, int d, float eps1, float eps2, float momentum1,
                               float momentum2, float* running_mean1, float* running_var1,
                               long long* batches1, float* running_mean2, float* running_var2,
                               long long* batches2, double* stats, float* out, const float* y,
                               double* mse_workspace, float* loss, float* d_out, int buffers_zeroed,
                               void* stream);
/* buffers_zeroed (the _rng and _act entry points; bit 1 of gdn_head_train_bwd_rng's: see gdn_train_finish): 0 = the call zero-fills its accumulators itself (a
 * memset launch each in forward and backward); 1 = the caller guarantees `stats` (forward) / the first
 * gdn_head_train_stats_bytes-style block of `workspace` (backward) are zero on entry, and the backward
 * leaves BOTH zeroed again when it finishes — a training loop that zero-fills them once never pays the two
 * memset launches (~5 us each at 512 windows).                                                          */

/* ---- train-mode OutLayer MLP, out_layer_num > 1 (models/GDN.py:27-56 under model.train()) ----------
 * The head passes above end at the [B*n, d] activation after dropout (forward: `act`) / start from its
 * gradient (backward: `d_act`) instead of the fused Linear(d -> 1); mask / keep as in gdn_head_train_fwd,
 * or (both null, rng_seed_step given, p_drop > 0) the in-kernel draw of the _rng entry points.          */
int gdn_head_train_fwd_act(const float* z, const float* emb, const float* bn1_w, const float* bn1_b,
                           const float* bn2_w, const float* bn2_b, const float* mask,
                           const uint8_t* keep, float keep_scale, const long long* rng_seed_step,
                           float p_drop, int batch, int n, int d, float eps1,
                           float eps2, float momentum1, float momentum2, float* running_mean1,
                           float* running_var1, long long* batches1, float* running_mean2,
                           float* running_var2, long long* batches2, double* stats, float* act,
                           int buffers_zeroed, void* stream);
int gdn_head_train_bwd_act(const float* d_act, const float* z, const float* emb, const float* bn1_w,
                           const float* bn1_b, const float* bn2_w, const float* bn2_b,
                           const float* mask, const uint8_t* keep, float keep_scale,
                           const long long* rng_seed_step, float p_drop,
                           const double* stats, int batch, int n, int d, float eps1, float eps2,
                           double* workspace, float* d_z, float* d_emb, float* d_bn1_w, float* d_bn1_b,
                           float* d_bn2_w, float* d_bn2_b, int buffers_zeroed, void* stream);
/* The MLP itself: Y_l = A_l W_l^T + b_l, A_{l+1} = relu(BatchNorm_train(Y_l)) for l = 0..layers-2 (A_0 = act
 * [rows, d_in]), out = A_{layers-1} w_o + b_o — replaces OutLayer.forward (models/GDN.py:47-56) and the
 * autograd graph behind train.py:72.  fp32 matrix cores (exact fp32 products), batch statistics and every
 * reduction in fp64 in a fixed order (bitwise reproducible).  params[4*l .. 4*l+3] = {W_l [hidden, K_l],
 * b_l, gamma_l, beta_l} (K_0 = d_in, K_l = hidden), running[2*l .. 2*l+1] = {running_mean, running_var} (null
 * = not tracked), batches[l] = num_batches_tracked or null; eps[l], momentum[l]: host floats.  The arrays
 * of pointers live in HOST memory and hold device pointers.  `saved` (gdn_mlp_train_saved_bytes) carries the
 * pre-BatchNorm outputs and the batch constants from the forward to the backward; `workspace`
 * (gdn_mlp_train_workspace_bytes) is scratch.  grads[4*l .. 4*l+3] = gradients in the layout of params.
 * Supported: layers 2..8, d_in a multiple of 4 up to 256, hidden 1..512 (widths that are not a multiple of 4
 * stage their operands element by element); else GDN_ERR_UNSUPPORTED and byte counts of 0.                                                                                   */
long long gdn_mlp_train_saved_bytes(int rows, int d_in, int hidden, int layers);
long long gdn_mlp_train_workspace_bytes(int rows, int d_in, int hidden, int layers);
int gdn_mlp_train_fwd(const float* act, const float* const* params, float* const* running,
                      long long* const* batches, const float* eps, const float* momentum,
                      const float* out_w, const float* out_b, int rows, int d_in, int hidden,
                      int layers, void* saved, void* workspace, float* out, void* stream);
int gdn_mlp_train_bwd(const float* d_out, const float* act, const float* const* params,
                      const float* out_w, int rows, int d_in, int hidden, int layers,
                      const void* saved, void* workspace, float* const* grads, float* d_out_w,
                      float* d_out_b, float* d_act, void* stream);

/* gdn_mlp_eval_fwd: the OutLayer MLP under model.eval() (models/GDN.py:45-56: Linear, BatchNorm on the RUNNING
 * statistics, ReLU per hidden layer, Linear(hidden -> 1)) for the widths the one-launch chain gdn_mlp_fwd does not
 * take (hidden > 256; up to 512 = the reference class's default inter_num): one fp32 matrix-core GEMM per hidden
 * layer, the BatchNorm + ReLU folded into the next GEMM's operand staging, a column pass for the last Linear.
 * params / running as gdn_mlp_train_fwd (host arrays of device pointers; running must be non-null here).
 * hidden 1..512, d_in a multiple of 4; workspace: gdn_mlp_eval_workspace_bytes (0 = unsupported shape).    */
long long gdn_mlp_eval_workspace_bytes(int rows, int d_in, int hidden, int layers);
int gdn_mlp_eval_fwd(const float* act, const float* const* params, const float* const* running,
                     const float* eps, const float* out_w, const float* out_b,
                     int rows, int d_in, int hidden, int layers, void* workspace, float* out, void* stream);

/* One launch less at the end of a training step: gdn_head_train_bwd_rng with (buffers_zeroed | 2) leaves out its
 * small finishing launch, gdn_project_bwd_partials is gdn_project_bwd without its reduce launch (*rows_out =
 * partial rows written to `workspace`), and gdn_train_finish runs both reductions as ONE launch (independent
 * workgroups, disjoint outputs).  Same results as the separate forms.                                       */
int gdn_project_bwd_partials(const float* x, const float* d_xlin, const float* d_si, const float* d_sj,
                             int batch, int n, int w, int d, float* workspace, int* rows_out,
                             void* stream);
int gdn_train_finish(double* head_workspace, double* stats, int head_zeroed, int batch, int n, int d,
                     float* d_emb, float* d_bn1_w, float* d_bn1_b, float* d_bn2_w, float* d_bn2_b,
                     float* d_lin_w, float* d_lin_b, const float* proj_workspace, int proj_rows, int w,
                     float* d_proj_w, float* d_a, float* d_c, void* stream);

/* gdn_adam_step: torch.optim.Adam(lr, betas, eps, weight_decay) of train.py:31,73 over ONE flat fp32
 * buffer holding every parameter back to back (params / grads / exp_avg / exp_avg_sq: [count]); step[0] =
 * steps taken so far (device memory), incremented by the call.  grads are multiplied by grad_scale first
 * (1/ranks after a summing all-reduce).  Same update, in the same operation order, as torch's
 * single-tensor Adam (amsgrad and maximize off).  grads[zero_from, zero_from + zero_count) is cleared
 * after use (zero_count = 0: nothing is cleared; gdn_attn_aggregate_bwd WRITES its d_bias since ABI 20). */
int gdn_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                  long long* step, int count, double lr, double beta1, double beta2, double eps,
                  double weight_decay, double grad_scale, int zero_from, int zero_count, void* stream);

/* gdn_mse_loss_grad: train.py:20-23 `F.mse_loss(out, y, reduction='mean')` and the gradient
 * autograd derives for it, d_out = 2 (out - y) / count, in one launch (fp64 accumulation,
 * bitwise reproducible).  workspace: gdn_mse_workspace_bytes() bytes, ZEROED ONCE by the
 * caller when allocated; every call leaves it zeroed.  Calls sharing a workspace must be
 * stream-ordered.  loss[1], d_out[count].                                                   */
long long gdn_mse_workspace_bytes(void);
int gdn_mse_loss_grad(const float* out, const float* y, long long count, double* workspace,
                      float* loss, float* d_out, void* stream);

/* gdn_mse_loss_grad_masked: the loss over the observed targets only (training on a series with missing readings).
 * valid[batch, n] uint8 says which targets are real, row_valid[batch] int32 how many per window (both are
 * gdn_windows_gather_gaps' outputs); m = sum(row_valid).  loss = sum over valid of (out - y)^2 / m;
 * d_out = 2 (out - y) / m where valid, EXACTLY 0.0 where not (a select: a non-finite out or y in a masked slot
 * reaches neither); m = 0: loss 0, d_out all zeros.  One launch: every workgroup adds the `batch` counts itself, then
 * gdn_mse_loss_grad's grid, chains, finish and scale — with every byte set it writes gdn_mse_loss_grad's bits.  Same
 * workspace rules.  m_out (int64[1], may be NULL) receives m.  Additive: the ABI version does not move.          */
int gdn_mse_loss_grad_masked(const float* out, const float* y, const uint8_t* valid, const int* row_valid, int batch,
                             int n, double* workspace, float* loss, float* d_out, int64_t* m_out, void* stream);

/* ---- fused eval forward (the throughput path) ---------------------------------------
 * Everything from x[batch,n,w] to out[batch,n] in one launch (one workgroup per window,
 * xlin tile and neighbour lists resident in LDS): models/GDN.py:122-187 under
 * model.eval() with out_layer_num == 1.  HBM traffic = x in + out.                      */
int gdn_forward_fused(const float* x, const float* lin_w, const float* node_terms,
                      const uint16_t* nbr, const int32_t* deg, const float* gnn_bias,
                      const float* emb, const float* bn1_affine, const float* bn2_affine,
                      const float* out_w, const float* out_b,
                      int batch, int n, int w, int d, int k, float* out, void* stream);

/* Same forward fed from the RAW series instead of materialised windows: series[n, series_len]
 * fp32 (the [node, time] layout of datasets/TimeDataset.py:42); window b of the launch is
 * series[:, first+b : first+b+w] (TimeDataset.py:46-49 with stride 1, the test-mode loop), its
 * target column is first+b+w.  Requires first + batch - 1 + w <= series_len.  Needs d >= 32 and
 * w <= 32 (the matrix-core projection variants); otherwise GDN_ERR_UNSUPPORTED.          */
int gdn_forward_fused_series(const float* series, int series_len, int first, const float* lin_w,
                             const float* node_terms, const uint16_t* nbr, const int32_t* deg,
                             const float* gnn_bias, const float* emb, const float* bn1_affine,
                             const float* bn2_affine, const float* out_w, const float* out_b,
                             int batch, int n, int w, int d, int k, float* out, void* stream);

/* gdn_graph_bank_order: a copy of the neighbour lists with every row's entries permuted inside its two halves
 * (slots [0, pitch/2) and [pitch/2, pitch)) so that the staged matrix-core kernels' per-slot LDS accesses (the
 * s_j gather, the two scatters into the attention image) spread over the banks: softmax and aggregation do not
 * depend on the order of a target's slots, so gdn_attn_aggregate_fwd[_bf16] may be given this table instead of
 * `nbr` whenever the caller does not read alpha in rank order (z is the same to the summation order of the
 * softmax denominator).  Matrix-core shapes only (n <= 127, k <= 63); once per graph, one small launch.      */
int gdn_graph_bank_order(const uint16_t* nbr, int n, int k, uint16_t* nbr_ordered, void* stream);

/* ---- plans: the fused forward with its per-launch constants precomputed -------------
 * For shapes on the matrix-core path (n <= 127, d = 64 or 128, w <= 32, k <= 63) everything a
 * workgroup of gdn_forward_fused derives from the parameters and the sensor graph (list
 * offsets, split weight operands in the k order of the product that consumes them, folded
 * BatchNorm / embedding factors, the C-in table, the x limit) can be computed
 * once per parameter update into a caller-owned device buffer, the PLAN; launches that are
 * given it skip that prologue (~10 us per workgroup), which is most of the time of a
 * single-minibatch launch.  The plan is read-only for the launches and holds no pointers;
 * its layout is private to the library build that wrote it (size: gdn_fused_plan_bytes).
 *   gdn_fused_plan_bytes   size of the plan for this shape (0 = shape not on this path:
 *                          use gdn_forward_fused);
 *   gdn_fused_plan_build   same parameter arguments as gdn_forward_fused;
 *   gdn_forward_fused_plan / _series_plan   = gdn_forward_fused(_bf16) /
 *                          gdn_forward_fused_series on the plan's parameters; x is
 *                          fp32 [batch,n,w] (bf16_storage = 0) or bf16 (1, must match the
 *                          plan).  Results are bit-identical to the plan-less calls.        */
long long gdn_fused_plan_bytes(int n, int w, int d, int k, int bf16_storage);
int gdn_fused_plan_build(const float* lin_w, const float* node_terms, const uint16_t* nbr,
                         const int32_t* deg, const float* gnn_bias, const float* emb,
                         const float* bn1_affine, const float* bn2_affine, const float* out_w,
                         const float* out_b, int n, int w, int d, int k, int bf16_storage,
                         void* plan, void* stream);
int gdn_forward_fused_plan(const void* x, const void* plan, int batch, int n, int w, int d, int k,
                           int bf16_storage, float* out, int* range_guard, void* stream);
int gdn_forward_fused_series_plan(const float* series, int series_len, int first, const void* plan,
                                  int batch, int n, int w, int d, int k, float* out, int* range_guard,
                                  void* stream);

/* ---- range guard ---------------------------------------------------------------------
 * The reference computes in fp32 on whatever the caller feeds it (models/graph_layer.py:56).  The fp32-storage
 * fused matrix-core kernel aggregates the raw window before it projects it: it carries x times 8, and the aggregated
 * row sum_j alpha_ij x_j times 8 (a convex combination of the window's values), as two f16 terms each: values of
 * 65504 and beyond do not exist there.  Every plan therefore holds its X LIMIT, the largest |x| for which both are
 * representable whatever the window: 60000 / 8 = 7500, whatever lin' and C-in are (the projected tile and C-in
 * exist in fp32 only) — or 0 when an entry of the BatchNorm-folded lin' times 8 is itself outside the f16 range
 * (a float at byte gdn_fused_plan_limit_offset(...) of the plan; +inf for bf16 storage, whose terms have
 * fp32's exponent range).  Normalised data (the reference's scripts/process_*.py: MinMax to [0, 1]) sits four
 * orders of magnitude below it; raw engineering units may not.  Two ways to stay exact for ANY input:
 *   (a) known data (a resident series): compare max|x| with the limit once and call the `_gated` entry points
 *       below with guard = null — the fp32 row-gather kernels, fp32's own range — when it is exceeded;
 *   (b) unknown data (GDN.forward on a caller's tensor): pass `range_guard` (2 ints, ZERO before the first
 *       call) to the planned launch — it stores 1 in range_guard[0] when a window holds |x| >= limit or a
 *       NaN — and follow it on the same stream with the gated launch on the same guard: a no-op (every
 *       workgroup returns at once) unless the flag is up, in which case it recomputes the launch's windows
 *       in fp32 and leaves the guard zeroed.  No host synchronisation, hipGraph-capturable; one guard per
 *       stream.  range_guard = null: no detection (the `_keys` launches never detect: use (a)).
 * The staged kernels have `_wide` twins that always take the row-gather path (training on raw-unit data:
 * harness.train / python -m gdn_amd.main compare the data they hold with GDN_WIDE_LIMIT once).          */
long long gdn_fused_plan_limit_offset(int n, int w, int d, int k, int bf16_storage);
int gdn_forward_fused_gated(int* guard, const float* x, const float* lin_w, const float* node_terms,
                            const uint16_t* nbr, const int32_t* deg, const float* gnn_bias,
                            const float* emb, const float* bn1_affine, const float* bn2_affine,
                            const float* out_w, const float* out_b,
                            int batch, int n, int w, int d, int k, float* out, void* stream);
int gdn_forward_fused_series_gated(int* guard, const float* series, int series_len, int first,
                                   const float* lin_w, const float* node_terms, const uint16_t* nbr,
                                   const int32_t* deg, const float* gnn_bias, const float* emb,
                                   const float* bn1_affine, const float* bn2_affine, const float* out_w,
                                   const float* out_b, int batch, int n, int w, int d, int k, float* out,
                                   void* stream);
int gdn_project_fwd_wide(const float* x, const float* lin_w, const float* node_terms,
                         int batch, int n, int w, int d,
                         float* xlin, float* s_i, float* s_j, void* stream);
int gdn_attn_aggregate_fwd_wide(const float* xlin, const float* s_i, const float* s_j,
                                const uint16_t* nbr, const int32_t* deg, const float* bias,
                                int batch, int n, int d, int k,
                                float* z, float* alpha, void* stream);
int gdn_attn_aggregate_bwd_wide(const float* d_z, const float* xlin, const float* alpha,
                                const float* s_i, const float* s_j,
                                const uint16_t* nbr, const uint32_t* rent, const int32_t* rlen,
                                int batch, int n, int d, int k,
                                float* d_xlin, float* d_si, float* d_sj, float* d_bias,
                                float* workspace, void* stream);

/* The two planned launches with the scoring hand-off folded into their epilogue: besides out[B, n] they leave
 * keys[sensor * key_pitch + b] = |out[b][sensor] - gt[b][sensor]| in float64 — the radix keys
 * gdn_score_select consumes (evaluate.py:48-50, util/data.py:75-82), which gdn_score_keys would otherwise
 * produce in a launch of its own (transposing 2 x 4 bytes in, 8 bytes out per value).  key_pitch >= batch;
 * slots batch..key_pitch-1 of every row are left untouched (pre-fill them with the all-ones filler when
 * key_pitch > batch).  Measured on MI355X: the 127 scattered 8-byte stores per window cost the launch more
 * (+40 us per 32768 windows) than the separate transposing kernel (14 us); harness.SeriesEvaluator uses
 * them only on request (GDN_FUSE_KEYS=1).                                                                 */
int gdn_forward_fused_plan_keys(const void* x, const void* plan, const float* gt, double* keys,
                                int key_pitch, int batch, int n, int w, int d, int k, int bf16_storage,
                                float* out, void* stream);
int gdn_forward_fused_series_plan_keys(const float* series, int series_len, int first, const void* plan,
                                       const float* gt, double* keys, int key_pitch, int batch, int n,
                                       int w, int d, int k, float* out, void* stream);

/* ---- bf16 STORAGE variants (BASELINE.json configs[2] / configs[4]) --------------------
 * Same arithmetic as the four forward entry points above with the windowed inputs x, the
 * projected features xlin and the aggregate z held in bfloat16 IN HBM (uint16_t = the raw
 * bf16 bit pattern, round-to-nearest-even where a value is stored); attention scalars,
 * logits, softmax, every accumulation, BatchNorm and the outputs stay fp32
 * (models/graph_layer.py:56,87-117 with 2-byte features).  Semantics, exactly:
 *   x     is given in bf16 (exact);
 *   xlin  = bf16( x . lin^T accumulated in fp32 )            [stored / LDS resident];
 *   s_i, s_j from the UNROUNDED projection (x_row . a + c, fp32);
 *   z     = sum_j alpha_ij xlin_j + bias in fp32; gdn_attn_aggregate_fwd_bf16 stores bf16(z),
 *           gdn_forward_fused_bf16 keeps z on chip in fp32;
 *   head  as gdn_head_fwd.
 * The three staged entry points: matrix-core path only (n <= 127, d = 64, w <= 32,
 * k <= 63; other shapes return GDN_ERR_UNSUPPORTED).  gdn_forward_fused_bf16 takes every
 * shape gdn_forward_fused takes: outside the matrix-core path the fp32 row-gather kernel
 * reads the bf16 windows and rounds its LDS-resident projected tile to bf16 (configs[4]:
 * 512 sensors, top-k 64, W = 30).
 * RANGE: with fp32 STORAGE the matrix-core kernels carry x, and the BatchNorm-folded features
 * 8*(scale1*xlin + shift), as two f16 terms each: values of 65504 and beyond do not exist there.
 * The reference takes any fp32 (models/graph_layer.py:56; its main.py normalises nothing, the
 * offline scripts/process_*.py do), so see "range guard" above: planned launches detect
 * out-of-range windows on the device, the `_wide` / `_gated` entry points are the fp32 row-gather
 * kernels with fp32's own range.  With bf16 storage x is ONE exact bf16 term with fp32's exponent
 * range and the projected tile is rounded to bf16: no such limit.                            */
int gdn_project_fwd_bf16(const uint16_t* x, const float* lin_w, const float* node_terms,
                         int batch, int n, int w, int d,
                         uint16_t* xlin, float* s_i, float* s_j, void* stream);
int gdn_attn_aggregate_fwd_bf16(const uint16_t* xlin, const float* s_i, const float* s_j,
                                const uint16_t* nbr, const int32_t* deg, const float* bias,
                                int batch, int n, int d, int k,
                                uint16_t* z, float* alpha, void* stream);
int gdn_head_fwd_bf16(const uint16_t* z, const float* emb, const float* bn1_affine,
                      const float* bn2_affine, const float* out_w, const float* out_b,
                      int batch, int n, int d, float* out, float* h2, void* stream);
int gdn_forward_fused_bf16(const uint16_t* x, const float* lin_w, const float* node_terms,
                           const uint16_t* nbr, const int32_t* deg, const float* gnn_bias,
                           const float* emb, const float* bn1_affine, const float* bn2_affine,
                           const float* out_w, const float* out_b,
                           int batch, int n, int w, int d, int k, float* out, void* stream);

/* ---- backward (training) -------------------------------------------------------------
 * Gradients of gdn_attn_aggregate_fwd and gdn_project_fwd; the autograd graph of
 * `loss.backward()` at train.py:72 restricted to the GraphLayer.  No gradient flows into
 * the neighbour lists (the graph is built from a detached embedding, models/GDN.py:145).
 *   d_xlin[BN,d]  gradient of the message term (gathered through the reverse lists: no
 *                 scatter atomics, bitwise reproducible);
 *   d_si, d_sj    grads of the per-node scalars;
 *   d_bias[d]     column sums of d_z, WRITTEN (not accumulated): every workgroup leaves one partial row in
 *                 the workspace and the last one to finish adds the rows in row order — no floating-point
 *                 atomics anywhere in the backward, so a training step is bitwise reproducible (the true
 *                 gradient of a bias in front of a train-mode BatchNorm is 0: what arrives here is rounding
 *                 noise, which Adam turns into +-lr steps — with atomics those steps differed run to run).
 *   workspace     gdn_attn_aggregate_bwd_workspace_bytes(batch, n, d, k) bytes, REQUIRED: [16 bytes: the
 *                 ticket, ZERO before the first call, left zero by every call][1024 x d floats: the d_bias
 *                 rows][batch*n*pitch floats of d_pi when the tile plus the two [n, pitch] tables exceed LDS
 *                 (n ~> 250 at d = 64, k = 30; the 512-sensor / k = 64 stress shape) — the tables then go
 *                 through global memory and only the tile must fit: (n+1)*d*4 bytes <= ~155 KB; beyond
 *                 the tile (large form) the same d_pi table carries the softmax gradient from the per-target
 *                 pass to the per-source pass].  One workspace per stream: two concurrent calls must not share one. */
long long gdn_attn_aggregate_bwd_workspace_bytes(int batch, int n, int d, int k);
int gdn_attn_aggregate_bwd(const float* d_z, const float* xlin, const float* alpha,
                           const float* s_i, const float* s_j,
                           const uint16_t* nbr, const uint32_t* rent, const int32_t* rlen,
                           int batch, int n, int d, int k,
                           float* d_xlin, float* d_si, float* d_sj, float* d_bias,
                           float* workspace, void* stream);

/* Shapes on the matrix-core path (n <= 127, d = 64, k <= 63) run the backward as two dense products per
 * window (G = dZ . X^T for d alpha, dX = A^T . dZ for the reverse gather; d_z scaled per window by a power of
 * two, every factor as two f16 terms) and do not read the reverse lists: gdn_attn_aggregate_bwd_uses_reverse
 * returns 0 there, rent / rlen may be null and gdn_graph_reverse need not run.                         */
int gdn_attn_aggregate_bwd_uses_reverse(int n, int d, int k);

/* 1 when every kernel of a training step (gdn_project_fwd, gdn_attn_aggregate_fwd, gdn_attn_aggregate_bwd,
 * gdn_project_bwd, gdn_terms_bwd) takes the shape, 0 otherwise: ask before capturing a step.           */
int gdn_train_supported(int n, int w, int d, int k);

/* Reverse neighbour lists for the backward gather: rent[n, gdn_rev_pitch(n)] u32 holds, for
 * source j, (target << 16 | slot) of every list entry that names j, ascending target;
 * rlen[n] their counts.  Built once per graph.                                           */
int gdn_rev_pitch(int n);
int gdn_graph_reverse(const uint16_t* nbr, const int32_t* deg, int n, int k,
                      uint32_t* rent, int32_t* rlen, void* stream);

/* Backward of gdn_project_fwd, i.e. of `x = self.lin(x)` (models/graph_layer.py:56) and of the
 * folded logit scalars (graph_layer.py:94-104):
 * x[BN,w], d_xlin[BN,d], d_si/d_sj[BN] -> d_lin_w[d,w] (direct term), d_a[2,P] (grads of a_i, a_j, P =
 * gdn_terms_pitch(w), zero padded), d_c[2,n] (grads of c_i, c_j); outputs are written, not accumulated.
 * workspace: gdn_project_bwd_workspace_bytes(n, w, d) bytes (one partial row per workgroup; w > 64: one partial
 * [d+2, w] block per row range, which only gdn_project_bwd reduces — gdn_train_finish refuses w > 64).          */
long long gdn_project_bwd_workspace_bytes(int n, int w, int d);
int gdn_project_bwd(const float* x, const float* d_xlin, const float* d_si, const float* d_sj,
                    int batch, int n, int w, int d, float* workspace,
                    float* d_lin_w, float* d_a, float* d_c, void* stream);

/* gdn_terms_bwd: chain rule through gdn_node_terms (a = lin^T att, c = emb . att_em — the
 * separable form of models/graph_layer.py:90-104): from gdn_project_bwd's d_a[2,P] / d_c[2,n]
 *   d_lin_w[d,w] += att_i (x) d_a[0] + att_j (x) d_a[1]      (in/out: holds the direct term)
 *   d_att_i/j[d]  = lin_w d_a[0/1]     d_att_em_i/j[d] = emb^T d_c[0/1]
 *   d_emb[n,d]    = d_c[0] (x) att_em_i + d_c[1] (x) att_em_j                               */
int gdn_terms_bwd(const float* lin_w, const float* att_i, const float* att_j,
                  const float* att_em_i, const float* att_em_j, const float* emb,
                  const float* d_a, const float* d_c, int n, int d, int w, float* d_lin_w,
                  float* d_att_i, float* d_att_j, float* d_att_em_i, float* d_att_em_j,
                  float* d_emb, void* stream);

/* ---- anomaly scoring -----------------------------------------------------------------
 * evaluate.py:48-68 + util/data.py:75-82 + the max over sensors of evaluate.py:131-139,
 * in float64 like the reference.  pred, gt: fp32 [t,n] (time-major, as test.py returns).
 *   gdn_score_quantiles: per sensor, median and IQR (numpy 'linear' percentiles 25/75)
 *     of |pred-gt| over all t ticks -> med_iqr[n,2] float64.  workspace: device buffer of
 *     gdn_score_workspace_bytes(t, n) bytes (8-byte aligned).
 *   gdn_score_smooth_max: a=(|pred-gt|-med)/(|iqr|+1e-2); 4-tap causal mean (first 3
 *     ticks of the SERIES 0); `first_tick` = series index of row 0 of this shard; when it is
 *     > 0, halo_pred/halo_gt [3,n] hold the 3 rows before it (right aligned; rows that would
 *     precede tick 0 are never read); scores[n,t] float64 (optional, NULL to skip) and
 *     anomaly[t] float64 = max over sensors.                                            */
long long gdn_score_workspace_bytes(int t, int n);
/* The two halves of gdn_score_quantiles, separable for the multi-GPU exchange (each rank builds the
 * keys of its own ticks, rows are exchanged by sensor, the owner selects over every rank's block):
 *   gdn_score_keys:   keys[n, pitch] float64 = |pred-gt| transposed; slots t..pitch-1 hold a filler
 *                     (bit pattern of all ones) that the select ignores.  pitch >= t.
 *   gdn_score_select: keys[blocks, n, pitch] (block r = the rows received from rank r), `total` real
 *                     keys per sensor -> med_iqr[n,2].  The input is not modified.  blocks > 1
 *                     needs pitch % 2048 == 0.  workspace: gdn_score_select_workspace_bytes bytes. */
long long gdn_score_select_workspace_bytes(int blocks, int n, int pitch);
int gdn_score_keys(const float* pred, const float* gt, int t, int n, int pitch, double* keys, void* stream);
int gdn_score_select(const double* keys, int blocks, int n, int pitch, long long total,
                     double* workspace, double* med_iqr, void* stream);
/* gdn_score_select plus a diagnostic (additive entry point, the ABI version does not move): path[n] int32 on the
 * device receives, per sensor, 0 where the one-workgroup select (one block, 2048 < pitch <= 32768) settled the
 * ranks from its sample brackets and 1 where the digit passes ran (always 1 on the other routes).  Same result. */
int gdn_score_select_paths(const double* keys, int blocks, int n, int pitch, long long total,
                           double* workspace, double* med_iqr, int* path, void* stream);
int gdn_score_quantiles(const float* pred, const float* gt, int t, int n,
                        double* workspace, double* med_iqr, void* stream);
int gdn_score_smooth_max(const float* pred, const float* gt, const double* med_iqr,
                         int t, int n, int first_tick, const float* halo_pred,
                         const float* halo_gt, double* scores, double* anomaly, void* stream);

/* gdn_score_smooth_topm: gdn_score_smooth_max that keeps, per tick, the m largest smoothed scores and their sensors
 * (which sensor deviates) instead of the maximum alone: top_scores[t, m] float64 descending, top_sensors[t, m] int32;
 * equal scores come in ascending sensor order (the first 3 ticks of the series, all 0: sensors 0 .. m-1).  Same
 * float64 arithmetic in the same order, same first_tick / halo meaning; with m = 1, top_scores[:, 0] equals the
 * anomaly of gdn_score_smooth_max bit for bit.  The [n, t] table is never written.  1 <= m <= 8 and m <= n, else
 * GDN_ERR_UNSUPPORTED.                                                                                          */
int gdn_score_smooth_topm(const float* pred, const float* gt, const double* med_iqr,
                          int t, int n, int first_tick, const float* halo_pred,
                          const float* halo_gt, int m, double* top_scores, int32_t* top_sensors, void* stream);

/* Resident series with missing readings (opt-in; additive entry points, the ABI version does not move).  The offline
 * counterpart of the streaming detector's "Missing readings" below, under the same three rules: a reading of
 * raw [n, t_raw] is MISSING when its exponent field is all ones (NaN, +inf, -inf); a missing reading is HELD at its
 * sensor's latest earlier real one; its normalised error is exactly 0.0 wherever it is used.  t = t_raw - w ticks are
 * scored, tick j = column w + j; a tick is KEPT for the calibration when all n readings of it are real.
 *   gdn_series_fill      ONCE per series, before any step (two launches, no atomics, no workgroup waits on another):
 *                          filled [n, t_raw]   raw with every missing reading held; a sensor without any earlier real
 *                                              reading gets 0 (raw[:, :w] finite is the caller's duty)
 *                          gt [t, n]           filled[:, w:] time-major: what the forward is scored against
 *                          valid [t, n] uint8  1 for a real reading
 *                          keep [t] uint8      1 where all n readings of the tick are real
 *                          counters [2, n] int64   row 0 missing_total, row 1 missing_run (the run of missing readings
 *                                              that ends at the last tick), both over the t scored ticks
 *                        workspace: gdn_series_fill_workspace_bytes(n, t_raw) bytes, 8-byte aligned (0 for an
 *                        unsupported shape).  filled must not alias raw.  1 <= n <= 4096, w >= 1, t_raw > w: else
 *                        GDN_ERR_UNSUPPORTED; null pointers: GDN_ERR_ARG.  All decided before any launch.
 *   gdn_score_keys_keep  gdn_score_keys that writes the filler into all n keys of a tick whose keep flag is 0 (and into
 *                        slots t .. pitch - 1): gdn_score_select(keys, 1, n, pitch, total = the kept ticks, ...) is then
 *                        the median / IQR table over complete ticks — every sensor has the same `total`.
 *   gdn_score_smooth_max_gaps / gdn_score_smooth_topm_gaps
 *                        gdn_score_smooth_max / _topm with gt = the filled readings and the validity plane valid [t, n]
 *                        (halo_valid [3, n] beside halo_pred / halo_gt when first_tick > 0): the normalised error of a
 *                        missing (tick, sensor) is 0.0 in its own 4-tap mean and in those of the next three ticks;
 *                        operation order, the zero scores of ticks 0-2, the top-m order and the tie rule stay.  With
 *                        every reading valid they write the bits of the plain entry points.  valid == NULL (halo_valid
 *                        == NULL with first_tick > 0): GDN_ERR_ARG.                                                    */
long long gdn_series_fill_workspace_bytes(int n, int t_raw);
int gdn_series_fill(const float* raw, int n, int t_raw, int w, float* filled, float* gt, uint8_t* valid,
                    uint8_t* keep, int64_t* counters, void* workspace, void* stream);
int gdn_score_keys_keep(const float* pred, const float* gt, const uint8_t* keep, int t, int n, int pitch,
                        double* keys, void* stream);
int gdn_score_smooth_max_gaps(const float* pred, const float* gt, const double* med_iqr,
                              int t, int n, int first_tick, const float* halo_pred, const float* halo_gt,
                              double* scores, double* anomaly, const uint8_t* valid, const uint8_t* halo_valid,
                              void* stream);
int gdn_score_smooth_topm_gaps(const float* pred, const float* gt, const double* med_iqr,
                               int t, int n, int first_tick, const float* halo_pred, const float* halo_gt, int m,
                               double* top_scores, int32_t* top_sensors, const uint8_t* valid,
                               const uint8_t* halo_valid, void* stream);

/* ---- attention from raw data -----------------------------------------------------------
 * The attention weights of models/graph_layer.py:91-110 (att_weight_1) without the projection: the logit is
 * separable ("per-forward constants" above), so alpha depends on the raw window, node_terms and the neighbour lists
 * only — not on d, xlin or the head.  fp32 VALU throughout: fp32's own range, no guard.  Arithmetic: s_i / s_j =
 * fp32 dot product of the window row with a_i / a_j, + c_i / c_j; LeakyReLU(0.2); max-subtract, exp, / (sum + 1e-16)
 * over the target's valid slots.  Rows have pitch = gdn_nbr_pitch(k) slots in the order of `nbr` (the top-k ranks
 * without self, then self); padding slots are written as 0.
 * Addressing of x: t_raw > 0: the raw series [n, t_raw], window b = columns first+b .. first+b+w-1 (gdn_attention_at:
 * windows[q] .. windows[q]+w-1); t_raw == 0: windows [batch, n, w] (first must be 0; gdn_attention_at: window index
 * windows[q]).  Both give the same bits on the same windows.
 *   gdn_attention_mean  mean[n, pitch] = sum_b weights[b] alpha_b / sum_b weights[b] over `batch` windows (weights ==
 *                       NULL: the plain mean; a weight sum that is not positive: zeros).  Per-workgroup float64
 *                       partial blocks in `workspace` (gdn_attention_workspace_bytes, no initialisation needed) are
 *                       added in block order by a second launch: no floating-point atomics, bitwise reproducible.
 *   gdn_attention_at    alpha[q, pitch]: one row per pair (windows[q], sensors[q]); a pair outside the data (negative
 *                       window, window past the series, sensor outside [0, n)) gets a row of zeros.
 * 1 <= w <= 1024, 1 <= k <= n <= 4096, k + 1 <= 1024, else GDN_ERR_UNSUPPORTED (workspace bytes: 0); windows that
 * do not fit the series, or first != 0 with t_raw == 0: GDN_ERR_ARG.  All decided before any launch.           */
long long gdn_attention_workspace_bytes(int batch, int n, int w, int k);
int gdn_attention_mean(const float* x, long long t_raw, long long first, const float* weights,
                       const float* node_terms, const uint16_t* nbr, const int32_t* deg,
                       int batch, int n, int w, int k, void* workspace, float* mean, void* stream);
int gdn_attention_at(const float* x, long long t_raw, const int64_t* windows, const int32_t* sensors, int q,
                     const float* node_terms, const uint16_t* nbr, const int32_t* deg,
                     int n, int w, int k, float* alpha, void* stream);

/* gdn_terms_bwd with accumulate_emb != 0: d_emb += (instead of =) — the head's share of the embedding
 * gradient already sits in d_emb (gdn_head_train_bwd), so both land in one gradient slot without an add
 * kernel.                                                                                              */
int gdn_terms_bwd_acc(const float* lin_w, const float* att_i, const float* att_j,
                      const float* att_em_i, const float* att_em_j, const float* emb,
                      const float* d_a, const float* d_c, int n, int d, int w, float* d_lin_w,
                      float* d_att_i, float* d_att_j, float* d_att_em_i, float* d_att_em_j,
                      float* d_emb, int accumulate_emb, void* stream);

/* ---- epochs from the resident series ------------------------------------------------------
 * Training and validation windows cut on the device from the raw series [n, series_len] (datasets/TimeDataset.py:
 * window of target tick t = columns t-w .. t-1, target = column t), so that an epoch is a run of graph replays with
 * no host work between them.  Additive entry points: the ABI version does not move.
 *   gdn_windows_gather   table entry e = first + (cursor ? cursor[0] * batch : 0) + b names tick t = starts[e];
 *                        x_out[b, i, :] = series[i, t-w : t], y_out[b, i] = series[i, t] for b < batch.  An entry with
 *                        e >= count, or a tick outside [w, series_len), gets a window of zeros and reads nothing.
 *                        `cursor` (device, may be NULL) is only read: advancing it is gdn_epoch_advance's launch.
 *                        1 <= w <= 1024, 1 <= n <= 4096 (else GDN_ERR_UNSUPPORTED), any alignment of t; offsets
 *                        into the series are 64-bit.
 *   gdn_epoch_advance    one thread: r = cursor[0]; if (r < table_len) loss_table[r] = loss[0]; cursor[0] = r + 1.
 *                        Stream-ordered after the step whose gather read the cursor.
 *   gdn_mse_batch_means  batch_means[q] = mean((pred - y)^2) over rows [q*batch, min(rows, (q+1)*batch)) of
 *                        pred / y [rows, n] (difference in fp32, accumulation in float64 in a fixed order), for
 *                        q < ceil(rows / batch); mean[0] = their plain average, added in batch order (test.py:
 *                        sum(losses) / len(losses)).  No atomics: bitwise reproducible.  `workspace` is not used
 *                        (may be NULL).
 * Null required pointers, batch < 1, count < 1, rows < 1, table_len < 1: GDN_ERR_ARG; all decided before any launch. */
int gdn_windows_gather(const float* series, int n, long long series_len, const int64_t* starts, long long count,
                       const int64_t* cursor, long long first, int batch, int w, float* x_out, float* y_out,
                       void* stream);
int gdn_epoch_advance(const float* loss, int64_t* cursor, float* loss_table, long long table_len, void* stream);
int gdn_mse_batch_means(const float* pred, const float* y, long long rows, int n, long long batch,
                        double* batch_means, double* mean, void* workspace, void* stream);

/* The same two with the validity plane of a filled series (gdn_series_fill's `valid` [series_len - w, n] uint8, row
 * t - w = tick t): training and validating on a series with missing readings.
 *   gdn_windows_gather_gaps     gdn_windows_gather, and valid_out[b, :] = valid[t - w, :] (n bytes, any alignment, 64-bit
 *                               offset), row_valid[b] = how many of them are set.  An entry beyond the table or a tick
 *                               outside [w, series_len): zeros, valid_out = 0, row_valid = 0.  series_len > w.
 *   gdn_mse_batch_means_masked  gdn_mse_batch_means over the real targets: valid [rows, n] uint8 beside pred / y;
 *                               batch_means[q] = the masked mean of minibatch q (0 when it has no real target),
 *                               batch_counts[q] int64 = its real targets; mean[0] = the average of the means of the
 *                               minibatches that have one, in batch order, 0 when none has.  Same chains and tree.  */
int gdn_windows_gather_gaps(const float* series, int n, long long series_len, const int64_t* starts, long long count,
                            const int64_t* cursor, long long first, int batch, int w, float* x_out, float* y_out,
                            const uint8_t* valid, uint8_t* valid_out, int* row_valid, void* stream);
int gdn_mse_batch_means_masked(const float* pred, const float* y, const uint8_t* valid, long long rows, int n,
                               long long batch, double* batch_means, int64_t* batch_counts, double* mean,
                               void* workspace, void* stream);

/* ---- streaming detector --------------------------------------------------------------------
 * Scoring ticks as they arrive, 1 .. c at a time, against a frozen calibration (median / IQR per sensor and one
 * threshold, both from a period known to be normal), with every piece of stream state on the device so that a push is
 * a fixed run of launches (capturable in a HIP graph).  Additive entry points: the ABI version does not move.
 * State: ONE allocation of gdn_stream_state_bytes(n, w) bytes (8-byte aligned; 0 for an unsupported shape):
 *   int64  ticks      ticks scored so far            (byte 0)
 *   int64  alarms     alarm ticks so far             (byte 8)
 *   int64  logged     log entries written so far     (byte 16)
 *   int64  reserved                                  (byte 24)
 *   double carry[3, n]   normalised errors (|pred - gt| - median) * (1 / (|iqr| + 1e-2)) of the last three scored
 *                        ticks, oldest first; zeros where the stream has no such tick      (byte 32)
 *   float  hist[n, w]    the last w ticks of every sensor, oldest first                    (byte 32 + 24 n)
 * Only gdn_stream_advance writes the state after gdn_stream_init; the other two read it.  A push is, in stream order:
 * gdn_stream_windows, the model's forward on x_out, gdn_stream_score, gdn_stream_advance.  `chunk` [c, n] fp32 is
 * time-major (one row per tick, the layout of pred / gt everywhere else): it is the gt of the score launch itself.
 *   gdn_stream_init     hist = the last w columns of history[n, h]; counters and carry 0 (so the 4-tap mean of the
 *                       first three scored ticks is 0, as at the start of a series).  h < w: GDN_ERR_ARG.
 *   gdn_stream_windows  x_out[b, i, :] for b < count = the w values of sensor i before tick b of the chunk: the first
 *                       max(0, w - b) from hist[i, b:], the rest from chunk[b-w .. b-1, i].  Rows b >= count are not
 *                       written.
 *   gdn_stream_score    gdn_score_smooth_topm over the chunk's `count` rows with first_tick = ticks read from the
 *                       state and the three values before the chunk from carry: the same float64 operations in the
 *                       same order, the same top-m order.  alarm[b] = top_scores[b, 0] > threshold[0] (threshold: one
 *                       float64 on the device; strict, a NaN score never alarms).
 *   gdn_stream_advance  hist = the last w columns of [hist | chunk^T] (a row is loaded whole before any of it is
 *                       stored: count < w is safe); carry = the last three of [carry | the chunk's normalised errors];
 *                       ticks += count; alarms += raised flags; every alarm appended to the log in tick order (ordered
 *                       compaction in one workgroup, no atomics) as log_ticks[e] = its global tick, log_sensors[e, :] =
 *                       its row of top_sensors, while e < log_len; a full log drops entries, alarms keeps counting.
 *                       log_len may be 0 with NULL log pointers.
 * 1 <= w <= 1024, 1 <= n <= 4096, 1 <= m <= 8, m <= n: else GDN_ERR_UNSUPPORTED.  Null required pointers, count < 1,
 * count > c, log_len < 0, log_len > 0 with a NULL log pointer: GDN_ERR_ARG.  All decided before any launch.          */
long long gdn_stream_state_bytes(int n, int w);
int gdn_stream_init(void* state, const float* history, long long h, int n, int w, void* stream);
int gdn_stream_windows(const void* state, const float* chunk, int c, int count, int n, int w, float* x_out,
                       void* stream);
int gdn_stream_score(const void* state, const float* pred, const float* chunk, const double* med_iqr,
                     const double* threshold, int c, int count, int n, int m, double* top_scores,
                     int32_t* top_sensors, int32_t* alarm, void* stream);
int gdn_stream_advance(void* state, const float* chunk, const float* pred, const double* med_iqr,
                       const int32_t* alarm, const int32_t* top_sensors, int c, int count, int n, int w, int m,
                       int64_t* log_ticks, int32_t* log_sensors, long long log_len, void* stream);
/* Missing readings (opt-in; additive entry points, the ABI version does not move).  A reading of the pushed chunk is
 * MISSING when it is not finite (NaN, +inf, -inf: exponent field all ones).  A push is then, in stream order:
 * gdn_stream_fill, gdn_stream_windows on the filled chunk, the forward, gdn_stream_score_gaps, gdn_stream_advance_gaps.
 *   gdn_stream_fill          filled_chunk[b, i] for b < count = raw_chunk[b, i] when it is not missing, else the latest
 *                            earlier reading of sensor i that was not missing: the closest earlier row of the chunk,
 *                            else hist[i, w - 1] (finite by induction when the history the stream began on was finite:
 *                            the caller's duty).  valid[b, i] = 1 for a real reading, 0 for a missing one.
 *                            gap_chunk[0, i] = the missing readings of sensor i in this push, gap_chunk[1, i] = the run
 *                            of missing readings that ends at row count - 1 (= count when every row was missing).
 *                            Rows >= count of filled_chunk and valid are not written.  Reads the state, writes none of
 *                            it.  One launch, no atomics.  filled_chunk must not alias raw_chunk.
 *   gdn_stream_score_gaps    gdn_stream_score with `chunk` = the filled chunk and the validity plane: the normalised
 *                            error of a missing reading is exactly 0.0 (the calibration median) in its own 4-tap mean
 *                            and in those of the next three ticks; nothing else changes.  With every reading valid it
 *                            writes the bits gdn_stream_score writes.
 *   gdn_stream_advance_gaps  gdn_stream_advance with `chunk` = the filled chunk (hist rolls from it): the carry entries
 *                            taken from the chunk are 0.0 where the reading was missing, and the gap counters
 *                            gaps[2, n] int64 (row 0 missing_total, row 1 missing_run; zeroed by the caller before the
 *                            first push) are folded: total += gap_chunk[0], run = gap_chunk[1] == count ? run + count
 *                            : gap_chunk[1].  The only writer of the state and of `gaps`.
 * Shapes and refusals as above (gdn_stream_score_gaps, like gdn_stream_score, has no w); all decided before any launch. */
int gdn_stream_fill(const void* state, const float* raw_chunk, int c, int count, int n, int w, float* filled_chunk,
                    uint8_t* valid, int32_t* gap_chunk, void* stream);
int gdn_stream_score_gaps(const void* state, const float* pred, const float* chunk, const uint8_t* valid,
                          const double* med_iqr, const double* threshold, int c, int count, int n, int m,
                          double* top_scores, int32_t* top_sensors, int32_t* alarm, void* stream);
int gdn_stream_advance_gaps(void* state, const float* chunk, const float* pred, const uint8_t* valid,
                            const int32_t* gap_chunk, const double* med_iqr, const int32_t* alarm,
                            const int32_t* top_sensors, int c, int count, int n, int w, int m, int64_t* log_ticks,
                            int32_t* log_sensors, long long log_len, int64_t* gaps, void* stream);
/* Rolling calibration (opt-in; additive entry points, the ABI version does not move).  A calibration ring keeps the
 * scoring keys |pred - gt| of the last R stream ticks on the device, in the layout gdn_score_select reads as it stands
 * (keys[1, n, pitch = R] holding `total` real keys, the filler in any slot), so that the median / IQR table the score
 * launch reads through a fixed pointer can be recomputed in place from recent ticks, without a recapture.
 * Ring: ONE allocation of gdn_stream_calib_bytes(n, R) = 8 n R + R bytes (rounded up to 8; 0 for an unsupported shape):
 *   double  ring_keys[n, R]   slot j of sensor i: fabs((double)pred - (double)gt) as gdn_score_keys computes it, or
 *                             the filler pattern (all ones)                                  (byte 0)
 *   uint8   ring_keep[R]      1 where slot j holds a kept tick                               (byte 8 n R)
 * An empty ring (the caller's duty before the first push): every key the filler, every keep flag 0.
 *   gdn_stream_calib_write       row b < count of the push is stream tick ticks + b (ticks read from the state) and owns
 *                                slot (ticks + b) mod R, whatever the alarms or the push sizes: the ring holds the last
 *                                R stream ticks.  The tick is KEPT unless exclude_alarms != 0 and alarm[b] != 0; a kept
 *                                tick writes its n keys and keep = 1, a tick that is not kept the filler into all n
 *                                keys and keep = 0 (no older tick survives in its slot).  Rows >= count touch nothing.
 *                                In stream order AFTER the score launch of the push (it wrote `alarm`) and BEFORE the
 *                                advance launch (ticks is still the push's first tick).  Reads the state, pred, chunk
 *                                and alarm; writes the ring only.  One launch, no atomics.
 *   gdn_stream_calib_write_gaps  the same on the filled chunk with the validity plane of gdn_stream_fill: a tick with a
 *                                missing reading in any sensor is not kept either (kept ticks are complete: filled =
 *                                raw there).
 * The table: gdn_score_select(ring_keys, 1, n, R, total = the sum of ring_keep, workspace, med_iqr) — every sensor has
 * the same `total` because keeping is decided per tick.
 * 1 <= n <= 4096, 64 <= R <= 2^20, 8 n R <= 2 GiB: else GDN_ERR_UNSUPPORTED.  Null pointers, count < 1, count > c,
 * c > R (two rows of a push would share a slot): GDN_ERR_ARG.  All decided before any launch.                        */
long long gdn_stream_calib_bytes(int n, int R);
int gdn_stream_calib_write(const void* state, const float* pred, const float* chunk, const int32_t* alarm, int c,
                           int count, int n, int R, int exclude_alarms, double* ring_keys, uint8_t* ring_keep,
                           void* stream);
int gdn_stream_calib_write_gaps(const void* state, const float* pred, const float* chunk, const int32_t* alarm,
                                const uint8_t* valid, int c, int count, int n, int R, int exclude_alarms,
                                double* ring_keys, uint8_t* ring_keep, void* stream);

/* Calibration on each sensor's own readings (opt-in; additive entry points, the ABI version does not move).  The two
 * blocks above keep a tick for the median / IQR table only when all n sensors reported, so that every sensor has one
 * `total`; with many sensors hardly any tick is complete.  Here sensor s's row comes from sensor s's own real readings:
 * the filler sits in single keys, every sensor has its own count, and the select forms ranks, interpolation weights
 * and the median rule per sensor on the device.
 *   gdn_score_keys_valid   gdn_score_keys with valid [t, n] uint8: key (s, tick) is the filler wherever
 *                          valid[tick, s] == 0, and in slots t .. pitch - 1.  With every reading valid it writes the
 *                          bits of gdn_score_keys.  valid == NULL: GDN_ERR_ARG.
 *   gdn_score_key_counts   counts[s] (int32, device) = slots of sensor s in keys[blocks, n, pitch] that do not hold the
 *                          filler.  One launch, integer adds only, no workgroup waits on another.
 *   gdn_score_select_counts
 *                          gdn_score_select where sensor s has counts[s] real keys (device data: nothing is read back).
 *                          counts[s] must be the number of non-filler slots of sensor s.  The ranks, the two gammas and
 *                          the median rule are those gdn_score_select forms on the host from `total`, computed with the
 *                          same float64 operations per sensor, on every route (single slice, one workgroup with its
 *                          brackets, digit passes; GDN_SELECT_MULTI / GDN_SELECT_BRACKET act as they do there): with
 *                          every count equal to T it writes the bits of gdn_score_select(total = T).  A sensor with
 *                          counts[s] < min_count or counts[s] < 1 keeps its med_iqr row as it is.  path may be NULL;
 *                          where given, a sensor that keeps its row on the one-workgroup route keeps its path entry
 *                          too.  Workspace: gdn_score_select_workspace_bytes.  Argument rules of gdn_score_select;
 *                          counts == NULL: GDN_ERR_ARG.
 *   gdn_stream_calib_write_sensor
 *                          gdn_stream_calib_write_gaps' slots and order.  A tick excluded by its alarm writes the
 *                          filler into all n keys and keep = 0; any other tick writes keep = 1, sensor i's key where
 *                          valid[b, i] == 1 and the filler where it is missing.  One launch, no atomics.
 * The table of a ring: gdn_score_key_counts(ring_keys, 1, n, R, counts), then
 * gdn_score_select_counts(ring_keys, 1, n, R, counts, min_count, workspace, med_iqr, NULL).                         */
int gdn_score_keys_valid(const float* pred, const float* gt, const uint8_t* valid, int t, int n, int pitch,
                         double* keys, void* stream);
int gdn_score_key_counts(const double* keys, int blocks, int n, int pitch, int32_t* counts, void* stream);
int gdn_score_select_counts(const double* keys, int blocks, int n, int pitch, const int32_t* counts, int min_count,
                            double* workspace, double* med_iqr, int* path, void* stream);
int gdn_stream_calib_write_sensor(const void* state, const float* pred, const float* chunk, const int32_t* alarm,
                                  const uint8_t* valid, int c, int count, int n, int R, int exclude_alarms,
                                  double* ring_keys, uint8_t* ring_keep, void* stream);

/* ---- Raw readings ----------------------------------------------------------------------------
 * The front of the deployment path (opt-in; additive entry points, the ABI version does not move): raw engineering
 * units at the raw tick rate in, the prepared series the model was trained on out — min-max normalised with a table
 * fitted on the training file, then the median of every `down` raw ticks (the reference's scripts/process_*.py:
 * MinMaxScaler(0, 1) and np.median over groups of 10).
 * Conventions: raw data is tick-major [t_raw, n] (a CSV read; the stream's chunk), fp32 when raw_f64 == 0, float64
 * otherwise.  Every computation is float64 with a multiply and the add after it rounded separately, as numpy does.
 * A reading that is not finite (NaN, +inf, -inf: exponent field all ones) is MISSING, gdn_stream_fill's rule.
 * table[n, 2] float64 = (scale, offset) per sensor: a reading x is normalised as x * scale + offset; for the min-max
 * fit scale = 1 / range and offset = 0 - min * scale (range = 1 where max - min < 10 eps: a constant sensor).
 * No allocation, no synchronisation (capturable), no atomics: results are bitwise reproducible.
 *   gdn_prep_stats   stats[i] = (min, max, mean, count) of sensor i's readings that are not missing, as float64; all
 *                    four 0 for a sensor with none.  The sum runs in a fixed order — rows strided over the four waves
 *                    of a segment, the waves in wave order, the segments in segment order, the number of segments a
 *                    function of (t_raw, n) alone — so it does not depend on the device or on how the grid is
 *                    scheduled.  workspace: gdn_prep_stats_workspace_bytes(t_raw, n) bytes (0: unsupported shape).
 *                    Two launches.
 *   gdn_prep_series  T = t_raw / down prepared ticks (the tail t_raw % down is dropped).  A missing reading is first
 *                    replaced by fill[i] when fill != NULL (fill, then normalise: the reference's order), else it
 *                    stays missing.  series[i, g] (sensor-major [n, T] fp32, the layout of `series` everywhere) = the
 *                    median of the group's normalised readings that are not missing, rounded to fp32: the middle
 *                    value of an odd count, (lo + hi) / 2.0 of the middle pair of an even one, a quiet NaN for a group
 *                    with none (a missing reading to every gaps consumer downstream).  labels_out[g] (float64, may be
 *                    NULL) = rint(max of labels_in[g down .. g down + down - 1]), labels_in float64 [t_raw].  One
 *                    launch; raw is read once, coalesced along sensors, and series is written in 256-byte runs.
 *   gdn_prep_ticks   the stream's front end.  The raw ticks of the launch are [pend_in[:pending] | raw[:r]], pending <
 *                    down a host value; out[g, :] (tick-major fp32, rows of a [c, n] chunk) for g < (pending + r) / down
 *                    by gdn_prep_series' arithmetic with fill == NULL; the last (pending + r) % down raw ticks go to
 *                    pend_out as float64.  pend_in and pend_out are distinct planes of at least down - 1 rows of n
 *                    float64 (the caller alternates them: a launch never reads what it writes).  One launch.
 * 1 <= n <= 4096 and 1 <= down <= 64: else GDN_ERR_UNSUPPORTED.  Null required pointers, t_raw < down, r < 1, pending
 * outside [0, down), pend_in == pend_out, (pending + r) / down > c, labels_out without labels_in: GDN_ERR_ARG.  All
 * decided before any launch.                                                                                        */
long long gdn_prep_stats_workspace_bytes(long long t_raw, int n);
int gdn_prep_stats(const void* raw, long long t_raw, int n, int raw_f64, void* workspace, double* stats, void* stream);
int gdn_prep_series(const void* raw, long long t_raw, int n, int raw_f64, const double* table, const double* fill,
                    int down, const double* labels_in, float* series, double* labels_out, void* stream);
int gdn_prep_ticks(const void* raw, int r, int raw_f64, const double* pend_in, int pending, double* pend_out, int n,
                   int down, const double* table, float* out, int c, void* stream);

/* ---- Alarm episodes --------------------------------------------------------------------------
 * The layer between a score per tick and an event list (opt-in; additive entry points, the ABI version does not move):
 * on-delay, a clear level below the raise level, off-delay, and a table of episodes.  With s_t = top_scores[t, 0],
 * float64 levels lo <= hi and integers on, off >= 1:
 *   above_t = s_t > hi (strict; a NaN score is not above), below_t = !(s_t > lo) (a NaN score is below);
 *   run_hi(t) / run_lo(t) = the length of the run of above / below ticks that ends at t (0: t is not above / below);
 *   set_t = run_hi(t) >= on, reset_t = run_lo(t) >= off; active_t = the latest set-or-reset at or before t is a set.
 *   An episode OPENS where active turns true: start = t - on + 1; it CLOSES where active turns false: end = t - off + 1
 *   (exclusive; end > start); peak = the largest score in [start, end), peak_tick = the first tick that holds it,
 *   sensors[:m] = top_sensors[peak_tick]; an episode still open at the last tick has end = -1 and its peak so far.
 * Episodes are numbered in tick order; the table keeps rows 0 .. E - 1 (start, end, peak_tick int64; peak float64;
 * sensors [E, m] int32) and `count` goes on counting beyond E.  Ticks are global: first_tick + index.  Comparisons and
 * copies only, no floating-point arithmetic, integer max / min atomics on an order-preserving image of the score: the
 * result is deterministic, the same for every grid size, and equal bit for bit between the two forms.
 * Carry: GDN_EPISODES_CARRY_BYTES bytes on the device, 8-byte aligned, all zero for a series that has not begun:
 *   int64 count, active, run_hi, run_lo (saturated at on / off); the peak so far of an above-run that has not raised
 *   (float64 peak, int64 tick, int32 sensors[8]); the open episode (int64 start, float64 peak, int64 peak_tick, int32
 *   sensors[8]); three reserved words.
 *   gdn_episodes_scan    the archive form, parallel over T: scores [T] float64 and top_sensors [T, m] int32 on the
 *                        device.  Five launches — per-tile reduce, a scan of the tile aggregates by one workgroup,
 *                        two apply passes, finish — and no workgroup waits on another.  carry_in (may be NULL: a
 *                        series that begins here) / carry_out (may be NULL; may be carry_in) let a long archive be
 *                        scanned in pieces over ONE table: a call keeps the rows below carry_in's count as they are and
 *                        completes the open one.  count [1] int64.  workspace: gdn_episodes_workspace_bytes(T, E)
 *                        bytes (0: unsupported), 8-byte aligned, need not be cleared.
 *   gdn_episodes_scan_grid  the same with the grid of the tile launches given (0: the library's choice): a diagnostic
 *                        for the claim that the grid does not change a bit.
 *   gdn_stream_events    the stream form, ONE launch of one workgroup in a push: after gdn_stream_score[_gaps] (it wrote
 *                        top_scores [c, m] / top_sensors [c, m]) and before gdn_stream_advance[_gaps] (`ticks` in the
 *                        stream state is still the push's first tick).  hi = threshold[0], the pointer the score launch
 *                        reads; lo = clear[0], a float64 device scalar (a clear level above hi, or NaN, acts as hi).
 *                        Reads the stream state; writes only `events`: ONE allocation of
 *                        gdn_stream_events_bytes(m, E) bytes, zero before the first push = [the carry | start [E] | end
 *                        [E] | peak_tick [E] | peak [E] | sensors [E, m]].  Rows >= count of a short push are ignored.
 *                        The open episode's row is rewritten on every push: a reader sees its peak so far.
 * 1 <= T <= 2^26 (stream: count <= c <= 4096), 1 <= m <= 8, 1 <= on, off <= 4096, 0 <= E <= 2^20: else
 * GDN_ERR_UNSUPPORTED (byte counts: 0).  lo > hi, a NaN level, first_tick < 0, a null required pointer (the table's
 * when E > 0), count < 1, count > c: GDN_ERR_ARG.  All decided before any launch.                                    */
#define GDN_EPISODES_CARRY_BYTES 160
long long gdn_episodes_workspace_bytes(long long T, long long E);
int gdn_episodes_scan(const double* scores, const int32_t* top_sensors, long long T, int m, double hi, double lo,
                      int on, int off, long long first_tick, long long E, const void* carry_in, void* carry_out,
                      int64_t* start, int64_t* end, int64_t* peak_tick, double* peak, int32_t* sensors, int64_t* count,
                      void* workspace, void* stream);
int gdn_episodes_scan_grid(const double* scores, const int32_t* top_sensors, long long T, int m, double hi, double lo,
                           int on, int off, long long first_tick, long long E, const void* carry_in, void* carry_out,
                           int64_t* start, int64_t* end, int64_t* peak_tick, double* peak, int32_t* sensors,
                           int64_t* count, void* workspace, int grid, void* stream);
long long gdn_stream_events_bytes(int m, long long E);
int gdn_stream_events(const void* state, const double* top_scores, const int32_t* top_sensors, const double* threshold,
                      const double* clear, int c, int count, int m, int on, int off, long long E, void* events,
                      void* stream);

/* ---- Alarm tuning ----------------------------------------------------------------------------
 * Which (hi, lo, on, off) to deploy (additive, the ABI version does not move): the episodes of P settings
 * over one scored series, matched against labelled incidents.  scores [T] float64 (s_t, as above), labels [T] uint8
 * (non-zero: the tick lies inside a labelled incident), hi [P], lo [P] float64, on [P], off [P] int32, all on the
 * device.  Incident i = the i-th maximal run of labelled ticks, [a_i, b_i); I of them.  The episodes of setting p are
 * those of "Alarm episodes" with first_tick = 0 and no cap; episode k spans [start_k, end_k), end_k = T while it is
 * open at the last tick, and raise_k = start_k + on - 1 is the tick at which it is first seen.  counts [P, 8] int64:
 *   0 episodes           episodes raised
 *   1 true_episodes      episodes whose span holds a labelled tick
 *   2 incidents_hit      incidents overlapped by at least one span (distinct)
 *   3 delay_sum          sum over the hit incidents of max(0, raise_k(i) - a_i), k(i) = the first episode that overlaps i
 *   4 delay_max          the largest of those delays (0: none hit)
 *   5 alarm_ticks        sum of end_k - start_k
 *   6 alarm_label_ticks  labelled ticks inside spans
 *   7 open               1: the last episode is open at T
 * A row with lo > hi, a NaN level, or on / off outside 1 .. 4096 gets -1 in all eight (decided on the device: no host
 * read).  ONE launch: a lane is a setting, a workgroup one wave that walks the ticks in order (ceil(P / 64)
 * workgroups), no atomics, no workspace; integer counts and comparisons only, so the result is exact.  The time is set
 * by T; below 64 * (number of CUs) settings part of the device idles.
 * 1 <= T <= 2^26, 1 <= P <= 2^20: else GDN_ERR_UNSUPPORTED; a null pointer: GDN_ERR_ARG; decided before the launch.   */
int gdn_alarm_sweep(const double* scores, const uint8_t* labels, long long T, const double* hi, const double* lo,
                    const int32_t* on, const int32_t* off, long long P, int64_t* counts, void* stream);

/* ---- streaming fleet --------------------------------------------------------------------------
 * U units of ONE model — a rack of servers, a line of pumps: the same sensor list, the same trained model, but a
 * median / IQR table, a threshold, a history and an alarm log per unit — scored with one run of launches per push, so
 * that the model's forward sees units x c windows (additive, the ABI version does not move).
 * State: ONE allocation of gdn_fleet_state_bytes(units, n, w) = units * gdn_stream_state_bytes(n, w) bytes; unit u's
 * block, at state + u * gdn_stream_state_bytes(n, w), has exactly the layout of "streaming detector" above.
 * Every tensor of a push gains a leading unit axis:
 *   chunk [U, c, n] fp32    x_out [U, c, n, w] fp32    pred [U, c, n] fp32    med_iqr [U, n, 2] float64
 *   threshold [U] float64   top_scores [U, c, m] float64   top_sensors [U, c, m] int32   alarm [U, c] int32
 *   log_ticks [U, L] int64  log_sensors [U, L, m] int32    counts [U] int32
 * counts[u] = the rows of unit u that are real in this push, ON THE DEVICE: every kernel reads it there and clamps it
 * to 0 .. c.  It is never a launch argument, so one captured graph serves a full push, a short one and one in which
 * some units are silent.  A push is, in stream order: gdn_fleet_windows, the model's forward on x_out viewed as
 * [U * c, n, w], gdn_fleet_score, gdn_fleet_advance.  Per unit every launch does the single-stream launch's work through
 * the same device functions, so a unit's outputs on its real rows, its state block and its log are, bit for bit, those
 * of a single stream pushed that unit's real rows in the same cuts (a push with counts[u] == 0 skipped).
 *   gdn_fleet_init     gdn_stream_init per unit from history [U, n, h]: one launch, grid (spans, U).
 *   gdn_fleet_windows  grid (row b, span, unit).  b < counts[u]: the row gdn_stream_windows writes for that unit.
 *                      b >= counts[u]: zeros, so the forward's input is a function of the states and this push only,
 *                      never of an earlier push (a stale out-of-range row could otherwise hold a guarded forward on
 *                      the fp32 route).
 *   gdn_fleet_score    one wave per (unit, run of 8 ticks): gdn_stream_score's sweep with the unit's first tick and
 *                      carry, its table rows and its threshold.  Writes rows b < counts[u] only.  `w` only places the
 *                      unit's state block.
 *   gdn_fleet_advance  grid (n + 1, unit): gdn_stream_advance per unit with count = counts[u]; the only writer of the
 *                      states and the logs.  counts[u] == 0 leaves every byte of unit u's state and log untouched.
 *                      log_len (L, per unit) may be 0 with NULL log pointers.
 * 1 <= units, units * c <= 4096, 1 <= n <= 4096, 1 <= w <= 1024, 1 <= m <= min(8, n): else GDN_ERR_UNSUPPORTED
 * (gdn_fleet_state_bytes: 0).  A null required pointer, h < w, log_len < 0, log_len > 0 with a NULL log pointer:
 * GDN_ERR_ARG.  All decided before any launch.                                                                        */
long long gdn_fleet_state_bytes(int units, int n, int w);
int gdn_fleet_init(void* state, const float* history, long long h, int units, int n, int w, void* stream);
int gdn_fleet_windows(const void* state, const float* chunk, const int32_t* counts, int units, int c, int n, int w,
                      float* x_out, void* stream);
int gdn_fleet_score(const void* state, const float* pred, const float* chunk, const double* med_iqr,
                    const double* threshold, const int32_t* counts, int units, int c, int n, int w, int m,
                    double* top_scores, int32_t* top_sensors, int32_t* alarm, void* stream);
int gdn_fleet_advance(void* state, const float* chunk, const float* pred, const double* med_iqr, const int32_t* alarm,
                      const int32_t* top_sensors, const int32_t* counts, int units, int c, int n, int w, int m,
                      int64_t* log_ticks, int32_t* log_sensors, long long log_len, void* stream);
/* Missing readings and alarm episodes per unit (opt-in; additive entry points, the ABI version does not
 * move).  Both are the single stream's options ("Missing readings", "Alarm episodes" above) per unit, with counts [U] on
 * the device in the place of `count`, so the one captured graph still serves full, short and silent units.  New tensors:
 *   raw_chunk, filled_chunk [U, c, n] fp32   valid [U, c, n] uint8   gap_chunk [U, 2, n] int32   gaps [U, 2, n] int64
 *   clear [U] float64   events: gdn_fleet_events_bytes(units, m, E) = units * gdn_stream_events_bytes(m, E) bytes, unit
 *   u's block (a single stream's events allocation, zero before the first push) at u * gdn_stream_events_bytes(m, E).
 * A push is, in stream order: gdn_fleet_fill, gdn_fleet_windows on the filled chunk, the forward, gdn_fleet_score_gaps,
 * [gdn_fleet_events,] gdn_fleet_advance_gaps; gdn_fleet_events also sits between the plain score and advance launches.
 *   gdn_fleet_fill          grid (sensor group of 64, unit): gdn_stream_fill on unit u's rows with count = counts[u]
 *                           clamped to 0 .. c; the hold value before the unit's first real reading is its own
 *                           hist[i, w - 1].  Rows at or beyond counts[u] are neither read nor written (a non-finite
 *                           value there is not a missing reading); a unit with count 0 writes nothing, gap_chunk
 *                           included.  The workgroup has 1, 4 or 16 waves by c alone (c <= 8, c <= 32, else), never by
 *                           counts; integer counts and "the right-most real reading wins", so every shape writes the
 *                           same bits.  Reads the states, writes none.  filled_chunk must not alias raw_chunk.
 *   gdn_fleet_score_gaps    gdn_fleet_score with `chunk` = the filled chunk and its validity plane: per unit
 *                           gdn_stream_score_gaps.
 *   gdn_fleet_advance_gaps  gdn_fleet_advance with `chunk` = the filled chunk: per unit gdn_stream_advance_gaps on the
 *                           unit's slices of valid, gap_chunk and gaps.  The only writer of the states, the logs and
 *                           `gaps`; counts[u] == 0 leaves unit u's state, log and gaps rows untouched.
 *   gdn_fleet_events        workgroup u: gdn_stream_events on unit u's rows of top_scores / top_sensors [U, c, m] with
 *                           hi = threshold[u], lo = clear[u], first_tick from unit u's state block and count =
 *                           counts[u] clamped; counts[u] == 0 leaves the unit's events block byte for byte.  After the
 *                           score launch, before the advance launch (it reads the units' tick counters).  The tile is
 *                           256, 1024 or 4096 ticks by c alone; comparisons and copies only, so every tile writes the
 *                           same bits.  Reads the states; writes only `events`.
 * Refusals, all before any launch: a null pointer: GDN_ERR_ARG; the limits of the fleet entry points above (units * c,
 * n, w, m) and of gdn_stream_events (on, off, E): GDN_ERR_UNSUPPORTED (gdn_fleet_events_bytes: 0; units <= 4096).      */
int gdn_fleet_fill(const void* state, const float* raw_chunk, const int32_t* counts, int units, int c, int n, int w,
                   float* filled_chunk, uint8_t* valid, int32_t* gap_chunk, void* stream);
int gdn_fleet_score_gaps(const void* state, const float* pred, const float* chunk, const uint8_t* valid,
                         const double* med_iqr, const double* threshold, const int32_t* counts, int units, int c, int n,
                         int w, int m, double* top_scores, int32_t* top_sensors, int32_t* alarm, void* stream);
int gdn_fleet_advance_gaps(void* state, const float* chunk, const float* pred, const uint8_t* valid,
                           const int32_t* gap_chunk, const double* med_iqr, const int32_t* alarm,
                           const int32_t* top_sensors, const int32_t* counts, int units, int c, int n, int w, int m,
                           int64_t* log_ticks, int32_t* log_sensors, long long log_len, int64_t* gaps, void* stream);
long long gdn_fleet_events_bytes(int units, int m, long long E);
int gdn_fleet_events(const void* state, const double* top_scores, const int32_t* top_sensors, const double* threshold,
                     const double* clear, const int32_t* counts, int units, int c, int n, int w, int m, int on, int off,
                     long long E, void* events, void* stream);
/* Rolling calibration of a fleet (opt-in; additive entry points, the ABI version does not move): the
 * single stream's calibration ring ("Rolling calibration", "Calibration on each sensor's own readings" above) per unit.
 * Rings: ONE allocation of gdn_fleet_calib_bytes(units, n, R) = units * gdn_stream_calib_bytes(n, R) bytes, the keys of
 * all units first and then the keep flags:
 *   ring_keys [U, n, R] float64   unit u's block, a single stream's ring_keys [n, R], at u * n * R;
 *   ring_keep [U, R] uint8        at byte 8 U n R.
 * An empty ring holds the filler in every key and 0 in every keep flag.  Limits (gdn_fleet_calib_bytes: 0 outside):
 * the single stream's per unit (1 <= n <= 4096, 64 <= R <= 2^20), 1 <= units <= 4096, 8 units n R <= 2 GiB.
 *   gdn_fleet_calib_write         gdn_stream_calib_write per unit with count = counts[u] clamped to 0 .. c, read on the
 *                                 device: row b < count of unit u is that unit's stream tick ticks_u + b (ticks_u from
 *                                 the unit's state block) and owns slot (ticks_u + b) mod R of the unit's ring.  Keep
 *                                 rules and key arithmetic are the single stream's.  A unit with count 0 has no byte of
 *                                 its ring touched.  In stream order after gdn_fleet_score (and gdn_fleet_events),
 *                                 before gdn_fleet_advance.  Reads the states, pred, the (filled) chunk, alarm [U, c]
 *                                 and valid; writes the rings only.  ONE launch whose form follows c alone: c < 64 a
 *                                 wave per (unit, row) with its lanes along the sensors, no LDS and no barrier; from 64
 *                                 on the single stream's transposing tile per (row tile, unit).  Both write the same
 *                                 bytes.  No atomics; no workgroup waits on another.
 *   gdn_fleet_calib_write_gaps    the same with gdn_stream_calib_write_gaps' rule: valid [U, c, n] of gdn_fleet_fill.
 *   gdn_fleet_calib_write_sensor  the same with gdn_stream_calib_write_sensor's rule.
 *   gdn_fleet_ring_counts         the per-row counts gdn_score_select_counts(keys = ring_keys, blocks = 1, n = U n
 *                                 rows, pitch = R) takes.  ring_keep != NULL (tick calibration): kept [U] int32 = the sum
 *                                 of each unit's keep flags, counts [U n] int32 = kept[u] for every row of unit u.
 *                                 ring_keep == NULL (per-sensor calibration): counts already holds gdn_score_key_counts
 *                                 over the U n rows and `kept` is not used.  select [U] uint8 on the device may be NULL;
 *                                 a unit with select[u] == 0 gets counts 0 (the select then keeps its rows) and keeps
 *                                 kept[u].  One launch (none when ring_keep and select are both NULL).
 * Refusals, all before any launch: a null required pointer, c > R: GDN_ERR_ARG; units * c, n, w and the ring limits:
 * GDN_ERR_UNSUPPORTED.                                                                                               */
long long gdn_fleet_calib_bytes(int units, int n, int R);
int gdn_fleet_calib_write(const void* state, const float* pred, const float* chunk, const int32_t* alarm,
                          const int32_t* counts, int units, int c, int n, int w, int R, int exclude_alarms,
                          double* ring_keys, uint8_t* ring_keep, void* stream);
int gdn_fleet_calib_write_gaps(const void* state, const float* pred, const float* chunk, const int32_t* alarm,
                               const uint8_t* valid, const int32_t* counts, int units, int c, int n, int w, int R,
                               int exclude_alarms, double* ring_keys, uint8_t* ring_keep, void* stream);
int gdn_fleet_calib_write_sensor(const void* state, const float* pred, const float* chunk, const int32_t* alarm,
                                 const uint8_t* valid, const int32_t* counts, int units, int c, int n, int w, int R,
                                 int exclude_alarms, double* ring_keys, uint8_t* ring_keep, void* stream);
int gdn_fleet_ring_counts(const uint8_t* ring_keep, const uint8_t* select, int units, int n, int R, int32_t* counts,
                          int32_t* kept, void* stream);
/* Threshold from the ring (opt-in; additive entry points, the ABI version does not move): after a
 * recalibration has rewritten a table, the alarm threshold — a number in units of that table — is re-derived from the
 * same ring by the rule of the first calibration: the largest smoothed anomaly score of the period.  A single stream is
 * the fleet of one unit (its state is one state block, its ring one unit's slices): ONE symbol serves both.
 * Per unit, with base = ticks mod R (from the unit's state block: the slot the next tick takes, the oldest of a full
 * ring) and the table med_iqr [n, 2] as it stands when the launch runs (in stream order after the select):
 *   error(s, q)  = (ring_keys[s, q] - median_s) * (1 / (|iqr_s| + 1e-2)), the scorer's expression and reciprocal;
 *                  mode 2 (per-sensor rings): a key that is the filler bit pattern is a missing reading, error 0.0;
 *   score(q)     = max over s of (((error(s, q-3) + error(s, q-2)) + error(s, q-1)) + error(s, q)) / 4.0, slots mod R,
 *                  no FMA contraction; a NaN never wins the maximum;
 *   eligible(q)  = ring_keep is 1 at q, q-1, q-2, q-3 (mod R) and (q - base) mod R >= 3: the ring holds the whole
 *                  window the live scorer would smooth over, and the window does not straddle the seam between the
 *                  newest and the oldest tick;
 *   peak [U] float64 = the largest score of an eligible slot (-inf when there is none), peak_slot [U] int32 the
 *   smallest slot that attains it (-1 when none does), eligible [U] int32 the number of eligible slots: always written.
 *   threshold[u] = peak * margin (one float64 multiply) iff select[u] != 0 (select [U] uint8 may be NULL: every unit),
 *   eligible >= min_eligible and peak is finite and > 0; otherwise it keeps its bits.  clear_frac / clear [U] float64
 *   (both NULL, or both given): clear[u] = the new threshold * clear_frac[u], written with it and only then.
 * mode: 0 or 1 — tick calibration (gdn_*_calib_write / _gaps rings: no filler test), 2 — gdn_*_calib_write_sensor rings.
 * workspace: gdn_fleet_ring_threshold_bytes(units, R) bytes (16 per unit and tile of 61 slots; 0 outside the limits of
 * gdn_fleet_calib_bytes), written and read by the call, nothing carried.  Two launches: a wave per (unit, tile) whose
 * lanes run along the slots, three halo slots taken mod R, the sensors walked with the running maximum in a register;
 * then a workgroup per unit that folds the partials (maximum, ties by the lower slot; integer sums) and applies the
 * rule.  The maximum is exact in any order: no tiling changes a bit.  No atomics; no workgroup waits on another.
 * Refusals, all before any launch: a null required pointer, one of clear_frac / clear without the other, a margin that
 * is not finite or <= 0, min_eligible < 1, another mode: GDN_ERR_ARG; n, w and the ring limits: GDN_ERR_UNSUPPORTED.   */
long long gdn_fleet_ring_threshold_bytes(int units, int R);
int gdn_fleet_ring_threshold(const void* state, const double* ring_keys, const uint8_t* ring_keep, const double* med_iqr,
                             const uint8_t* select, int units, int n, int w, int R, int mode, double margin,
                             int min_eligible, void* workspace, double* threshold, const double* clear_frac,
                             double* clear, double* peak, int32_t* eligible, int32_t* peak_slot, void* stream);
/* Raw readings of a fleet (opt-in; additive entry points, the ABI version does not move): gdn_prep_ticks
 * ("Raw readings" above) per unit in ONE launch, with every unit's open downsample group and its length on the device,
 * so that how many raw ticks a unit hands over — and how many it holds — is data, never a launch argument.
 * Pending state: ONE allocation of gdn_fleet_prep_bytes(units, n, down) bytes (zeroed: no unit holds a raw tick):
 *   ticks   [U, down, n] float64   at byte 0: unit u's open group, raw tick q < pending of sensor i at (u down + q) n + i
 *                                  (the bits of a float64 reading are kept);
 *   pending [U, tiles] int32       at byte 8 U down n, tiles = ceil(n / 64): the length of unit u's open group, one
 *                                  word per tile of 64 sensors, all tiles of a unit equal; padded to 8 bytes.
 *   gdn_fleet_prep_ticks  raw [U, rows, n] fp32 (raw_f64 = 0) or float64, rows <= c down; raw_counts [U] int32 on the
 *                         device, clamped to 0 .. rows: unit u's real raw rows are its first k = raw_counts[u].  With p
 *                         the unit's pending count, groups = (p + k) / down <= c.  out[u, g, :] (out [U, c, n] fp32) =
 *                         the median of raw ticks g down .. g down + down - 1 of [ticks[u, :p] | raw[u, :k]] for g <
 *                         groups, computed as gdn_prep_ticks computes it (table [n, 2] shared by all units; a group with
 *                         no finite reading: the quiet NaN); rows of out at or beyond groups are not written.
 *                         counts[u] = groups (the buffer every later fleet launch reads).  The new open group is the
 *                         last (p + k) mod down of those ticks.  Grid (tile, unit), 64 prep_waves(down) threads: a
 *                         workgroup reads its own count word and its own 64 columns of ticks[u], and after one barrier
 *                         writes them; tile 0 also writes counts[u].  No workgroup reads what another writes: in place,
 *                         no second plane, no atomic.  raw_counts[u] == 0: counts[u] = 0, the unit's pending state
 *                         stays byte for byte.
 *   gdn_fleet_prep_ticks_units   the same launch with tables [U, n, 2] float64: unit u normalises with
 *                         tables[u] — pumps of one model with duty points, hence raw ranges, of their own.  ONE kernel
 *                         body serves both: the per-unit table stride is 2 n doubles here and 0 above; grid, pending
 *                         rule, arithmetic and refusals are those of gdn_fleet_prep_ticks, and unit u's output equals
 *                         gdn_prep_ticks with table = tables[u] on that unit's real rows, bit for bit.
 * Refusals, all before any launch: a null pointer, rows < 1, rows > c down: GDN_ERR_ARG; units * c > 4096, units, c < 1,
 * n outside 1 .. 4096, down outside 1 .. 64: GDN_ERR_UNSUPPORTED (gdn_fleet_prep_bytes: 0; units <= 4096).             */
long long gdn_fleet_prep_bytes(int units, int n, int down);
int gdn_fleet_prep_ticks(const void* raw, int rows, int raw_f64, const int32_t* raw_counts, void* pend, int units,
                         int c, int n, int down, const double* table, float* out, int32_t* counts, void* stream);
int gdn_fleet_prep_ticks_units(const void* raw, int rows, int raw_f64, const int32_t* raw_counts, void* pend, int units,
                               int c, int n, int down, const double* tables, float* out, int32_t* counts, void* stream);
/* Fleet series (opt-in; additive entry points, the ABI version does not move): the archive side of a
 * fleet — U units of one model, each with a resident series of its own, scored in launches that cover all units.  All
 * tensors are stacks of contiguous per-unit planes:
 *   pred, gt [U, t, n] fp32    valid [U, t, n] uint8    keep [U, t] uint8    med_iqr [U, n, 2] float64
 *   gdn_fleet_series_keys         ONE launch: keys [U, n, pitch] float64, unit u's block what gdn_score_keys (keep ==
 *                                 valid == NULL), gdn_score_keys_keep (keep) or gdn_score_keys_valid (valid) writes for
 *                                 that unit's planes, bit for bit, the filler in slots t .. pitch-1 included.  Both keep
 *                                 and valid: GDN_ERR_ARG.  The block is what gdn_score_select_counts takes as blocks = 1,
 *                                 U n sensors (in spans of at most 65535 rows), with counts [U n].
 *   gdn_fleet_series_smooth_max   ONE launch over all units: unit u reads med_iqr[u] and is scored as a series of its own
 *   gdn_fleet_series_smooth_topm  with first_tick = 0 — its ticks 0 - 2 are exactly 0.0, no run of ticks and no
 *                                 predecessor row crosses a unit seam, row clamping stays inside the unit.  anomaly
 *                                 [U, t], scores [U, n, t] (may be NULL), top_scores / top_sensors [U, t, m]: per unit
 *                                 the bits of gdn_score_smooth_max / gdn_score_smooth_topm on that unit's planes.
 *   ..._gaps                      the same with the validity planes: per unit gdn_score_smooth_max_gaps / _topm_gaps.
 * Limits, decided before any launch: 1 <= U <= 4096, 1 <= n <= 4096, 1 <= m <= min(8, n), 8 U n pitch <= 2 GiB (the
 * smooth launches: pitch = t): GDN_ERR_UNSUPPORTED; a null required pointer, t < 1, pitch < t: GDN_ERR_ARG.
 * No floating-point atomics; no workgroup waits on another.                                                          */
int gdn_fleet_series_keys(const float* pred, const float* gt, const uint8_t* keep, const uint8_t* valid, int units,
                          int t, int n, int pitch, double* keys, void* stream);
int gdn_fleet_series_smooth_max(const float* pred, const float* gt, const double* med_iqr, int units, int t, int n,
                                double* scores, double* anomaly, void* stream);
int gdn_fleet_series_smooth_topm(const float* pred, const float* gt, const double* med_iqr, int units, int t, int n,
                                 int m, double* top_scores, int32_t* top_sensors, void* stream);
int gdn_fleet_series_smooth_max_gaps(const float* pred, const float* gt, const double* med_iqr, int units, int t, int n,
                                     double* scores, double* anomaly, const uint8_t* valid, void* stream);
int gdn_fleet_series_smooth_topm_gaps(const float* pred, const float* gt, const double* med_iqr, int units, int t,
                                      int n, int m, double* top_scores, int32_t* top_sensors, const uint8_t* valid,
                                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDN_HIP_H */
