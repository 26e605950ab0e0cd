// Shared device helpers for the gfx950 GDN kernels.  wave = 64 lanes, DPP "row" = 16 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/gdn_hip.h"

#define GDN_NEG_SLOPE 0.2f      // LeakyReLU slope, reference models/graph_layer.py:13
#define GDN_SOFTMAX_EPS 1e-16f  // torch_geometric.utils.softmax 1.5.0 denominator epsilon
#define GDN_MAX_W 64
#define GDN_A_PITCH 64          // a_i / a_j are stored zero padded to 64 floats (w > 64: gdn_terms_pitch(w))
#define GDN_LONG_MAX_W 1024     // longest window: gdn_long_window.hip

#define GDN_FLEET_MAX_ROWS 4096 // units * c: the cap on windows per launch of a streaming fleet (gdn_fleet.hip, gdn_events.hip)
static inline bool gdn_fleet_rows_ok(int units, int c) {
  return units >= 1 && c >= 1 && (long long)units * c <= GDN_FLEET_MAX_ROWS;
}

static inline int gdn_launch_status() {
  return hipGetLastError() == hipSuccess ? GDN_OK : GDN_ERR_LAUNCH;
}

// Immutable device properties, cached per device behind a mutex (gdn_graph.hip): the library is re-entrant
// across threads, streams and devices.  gdn_blocks_per_cu = resident workgroups per CU of kernel `fn` at
// (threads, dynamic LDS bytes); it also raises the kernel's dynamic-LDS limit to the 160 KB of a gfx950 CU.
int gdn_cu_count();
int gdn_blocks_per_cu(const void* fn, int threads, int lds);
// environment knob of a diagnostic A/B run, read ONCE per process at its first use (a function-local static:
// thread-safe initialisation, nothing on the launch path afterwards)
#define GDN_ENV_INT_ONCE(NAME, FALLBACK) \
  ([]() -> int { static const int v = [] { const char* e = getenv(NAME); return e ? atoi(e) : (FALLBACK); }(); return v; }())

// gdn_route.hip: THE kernel-family decision of the staged graph layer (include/gdn_hip.h "route table"): GDN_FAMILY_* of
// `stage` at (n, w, d, k) under GDN_ROUTE_* flags; dimensions a stage does not depend on are ignored.  Pure host
// arithmetic.  *bwd_form (ATTN_BWD, family TILE): GDN_BWD_* below, the sub-form that decides the workspace layout.
int gdn_route(int stage, int n, int w, int d, int k, int flags, int* bwd_form = nullptr);
int gdn_forward_staged_ok(int n, int w, int d, int k);        // the tile kernels take both stages of the staged forward
// the LDS budgets of the tile kernels, asked by gdn_route: make_plan (gdn_forward.hip), bwd_plan and the projection
// backward's staging chunk (gdn_backward.hip)
bool gdn_tile_forward_ok(int stage, int n, int w, int d, int k, bool series);
int gdn_tile_attn_bwd_form(int n, int d, int k, bool force_sliced);   // GDN_BWD_*, or -1 beyond the tile
bool gdn_tile_project_bwd_ok(int n, int w, int d);
// gdn_forward_dense.hip: the matrix-core aggregation path (n <= 127, d = 64); x is fp32 or bf16 bits
bool gdn_dense_supported(int n, int w, int d, int k);         // staged kernels: d = 64
bool gdn_dense_fused_supported(int n, int w, int d, int k);   // fused kernel: d = 64 or 128
int gdn_dense_forward_fused(const void* x, int x_is_bf16, int series_len, int series_first, const float* lin_w,
                            const float* node_terms, const uint16_t* nbr, const float* gnn_bias,
                            const float* emb, const float* bn1, const float* bn2, const float* out_w,
                            const float* out_b, int batch, int n, int w, int d, int k, float* out,
                            hipStream_t stream);
int gdn_dense_attn_aggregate(const void* xlin, int is_bf16, const float* s_i, const float* s_j, const uint16_t* nbr,
                             const float* bias, int batch, int n, int d, int k, void* z, float* alpha,
                             hipStream_t stream);
int gdn_dense_attn_bwd(const float* d_z, const float* xlin, const float* alpha, const float* s_i, const float* s_j,
                       const uint16_t* nbr, int batch, int n, int k, float* d_xlin, float* d_si, float* d_sj,
                       float* d_bias, float* bias_ws, hipStream_t stream);   // matrix-core backward of the gather-aggregate
int gdn_dense_project(const void* x, int is_bf16, const float* lin_w, const float* node_terms, int batch, int n,
                      int w, int d, void* xlin, float* s_i, float* s_j, hipStream_t stream);
// gdn_large.hip: the graph layer beyond the LDS tile (n up to 4096, xlin gathered from global memory): family LARGE,
// where make_plan / bwd_plan refuse the shape.  x rows at xb + b*bstride + s*sstride.
int gdn_large_project(const float* xb, long long bstride, long long sstride, const float* lin_w, const float* terms,
                      int batch, int n, int w, int d, float* xlin, float* s_i, float* s_j, hipStream_t stream);
int gdn_large_aggregate(const float* xlin, const float* s_i, const float* s_j, const uint16_t* nbr, const float* bias,
                        int batch, int n, int d, int k, float* z, float* alpha, hipStream_t stream);
int gdn_large_attn_bwd(const float* d_z, const float* xlin, const float* alpha, const float* s_i, const float* s_j,
                       const uint16_t* nbr, const uint32_t* rent, const int32_t* rlen, int batch, int n, int d, int k,
                       float* d_xlin, float* d_si, float* d_sj, float* d_bias, float* workspace,
                       long long bias_ws_floats, hipStream_t stream);
// gdn_long_window.hip: windows longer than GDN_MAX_W (up to GDN_LONG_MAX_W): family LONG.  Node terms at pitch
// gdn_terms_pitch(w); x rows as gdn_large_project's.
int gdn_long_node_terms(const float* lin_w, const float* att_i, const float* att_j, const float* att_em_i,
                        const float* att_em_j, const float* emb, int n, int d, int w, float* node_terms,
                        hipStream_t stream);
int gdn_long_project(const float* xb, long long bstride, long long sstride, const float* lin_w, const float* terms,
                     int batch, int n, int w, int d, float* xlin, float* s_i, float* s_j, hipStream_t stream);
long long gdn_long_project_bwd_workspace_bytes(int n, int w, int d);
int gdn_long_project_bwd_partials(const float* x, const float* d_xlin, const float* d_si, const float* d_sj, int batch,
                                  int n, int w, int d, float* workspace, int* parts_out, hipStream_t stream);
int gdn_long_terms_bwd(const float* lin_w, const float* att_i, const float* att_j, const float* att_em_i,
                       const float* att_em_j, const float* emb, const float* d_a, const float* d_c, int n, int d, int w,
                       float* d_lin_w, float* d_att_i, float* d_att_j, float* d_att_em_i, float* d_att_em_j,
                       float* d_emb, int accumulate_emb, hipStream_t stream);
int gdn_long_project_reduce(const float* part, int parts, int batch, int n, int w, int d, const float* d_si,
                            const float* d_sj, float* d_lin_w, float* d_a, float* d_c, hipStream_t stream);
// gdn_any_width.hip: embedding widths other than 16 / 32 / 64 / 128 (1 <= d <= GDN_ANY_MAX_D): family ANY, at every
// n, w, k of the envelope.  Dense [B*n, d] rows.
#define GDN_ANY_MAX_D 256
bool gdn_any_width(int d);
int gdn_any_project(const float* xb, long long bstride, long long sstride, const float* lin_w, const float* terms,
                    int batch, int n, int w, int d, float* xlin, float* s_i, float* s_j, hipStream_t stream);
int gdn_any_aggregate(const float* xlin, const float* s_i, const float* s_j, const uint16_t* nbr, const float* bias,
                      int batch, int n, int d, int k, float* z, float* alpha, hipStream_t stream);
int gdn_any_attn_bwd(const float* d_z, const float* xlin, const float* alpha, const float* s_i, const float* s_j,
                     const uint16_t* nbr, const uint32_t* rent, const int32_t* rlen, int batch, int n, int d, int k,
                     float* d_xlin, float* d_si, float* d_sj, float* d_bias, float* workspace,
                     long long bias_ws_floats, hipStream_t stream);
int gdn_any_head(const float* z, const float* emb, const float* bn1_affine, const float* bn2_affine,
                 const float* out_w, const float* out_b, int batch, int n, int d, float* out, float* h2,
                 hipStream_t stream);
long long gdn_any_project_bwd_workspace_bytes(int n, int w, int d);
int gdn_any_project_bwd_partials(const float* x, const float* d_xlin, const float* d_si, const float* d_sj, int batch,
                                 int n, int w, int d, float* workspace, int* parts_out, hipStream_t stream);
// ---- DPP within a 16-lane row ------------------------------------------------------
// dpp_ctrl encodings (gfx9): quad_perm 0x00-0xFF, row_ror:n 0x120+n, row_mirror 0x140,
// row_half_mirror 0x141.
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, dpp_i<CTRL>(__builtin_bit_cast(int, v)));
}
#define GDN_DPP_XOR1 0xB1          // quad_perm [1,0,3,2]
#define GDN_DPP_XOR2 0x4E          // quad_perm [2,3,0,1]
#define GDN_DPP_XOR3 0x1B          // quad_perm [3,2,1,0]
#define GDN_DPP_HALF_MIRROR 0x141  // lane i <-> 7-i inside each 8
#define GDN_DPP_MIRROR 0x140       // lane i <-> 15-i inside each 16
#define GDN_DPP_ROR1 0x121         // rotate the 16-lane row by one lane

// All 16 lanes of a row end with the row's sum / max.
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<GDN_DPP_XOR1>(v);
  v += dpp_f<GDN_DPP_XOR2>(v);
  v += dpp_f<GDN_DPP_HALF_MIRROR>(v);
  v += dpp_f<GDN_DPP_MIRROR>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_f<GDN_DPP_XOR1>(v));
  v = fmaxf(v, dpp_f<GDN_DPP_XOR2>(v));
  v = fmaxf(v, dpp_f<GDN_DPP_HALF_MIRROR>(v));
  v = fmaxf(v, dpp_f<GDN_DPP_MIRROR>(v));
  return v;
}

// LeakyReLU(0.2): max(v, 0.2 v) — v for v > 0, 0.2 v otherwise; -inf stays -inf
__device__ __forceinline__ float leaky(float v) { return fmaxf(v, v * GDN_NEG_SLOPE); }

// 64-lane wave sum through DPP + readlane (used by the small reduction kernels).
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// Fixed-order column sum across the workgroups of a launch, no floating-point atomics: every workgroup stores its
// row of `cols` partial sums (`lds_row`, complete and visible to the workgroup: call after a barrier), takes a
// ticket, and the workgroup that draws the last one adds the rows IN ROW ORDER and writes out[cols].  The result
// depends on the grid size only, never on the order the workgroups finish in: bitwise reproducible.
//   ws: [0..3] = the ticket (u64 + padding; zero on entry, left zero), rows at ws + 4 + row * cols.
// Same memory protocol as gdn_mse_kernel: agent-scope stores acknowledged (vmcnt) before the ticket is drawn, the
// last workgroup reads the rows back with agent-scope loads (no release/acquire fence: each would write back an
// XCD's whole L2).  Must be reached by every thread of every workgroup; `scratch` = blockDim.x floats of LDS.
#define GDN_COLSUM_WS_HEAD 4
#define GDN_COLSUM_MAX_ROWS 1024   // launches that use it keep their grid at or below this
__device__ __forceinline__ void gdn_colsum_ticket(float* __restrict__ ws, const float* lds_row, int cols,
                                                  float* __restrict__ out, float* scratch) {
  __shared__ bool last_wg;
  const int tid = threadIdx.x, nth = blockDim.x;
  float* rows = ws + GDN_COLSUM_WS_HEAD;
  for (int c = tid; c < cols; c += nth)
    __hip_atomic_store(rows + (size_t)blockIdx.x * cols + c, lds_row[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    unsigned long long* ticket = reinterpret_cast<unsigned long long*>(ws);
    const unsigned long long t = __hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_wg = t == (unsigned long long)gridDim.x - 1ull;
    if (last_wg) __hip_atomic_store(ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last_wg) return;
  // lane groups take rows g, g + groups, ...; four independent chains each so the loads overlap
  const int groups = nth / cols > 0 ? nth / cols : 1;
  const int c = tid % cols, g = tid / cols;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (g < groups) {
    const int nrow = (int)gridDim.x;
    int r = g;
    for (; r + 3 * groups < nrow; r += 4 * groups) {
      s0 += __hip_atomic_load(rows + (size_t)r * cols + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s1 += __hip_atomic_load(rows + (size_t)(r + groups) * cols + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s2 += __hip_atomic_load(rows + (size_t)(r + 2 * groups) * cols + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s3 += __hip_atomic_load(rows + (size_t)(r + 3 * groups) * cols + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (; r < nrow; r += groups)
      s0 += __hip_atomic_load(rows + (size_t)r * cols + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  scratch[tid] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (tid < cols) {
    float s = 0.f;
    for (int q = 0; q < groups; ++q) s += scratch[q * cols + tid];
    out[tid] = s;
  }
}

// Sum of the per-workgroup partial rows of gdn_project_bwd ([rows][D*wp + 128 + 2n] -> d_lin_w[D,w], d_a[2,64],
// d_c[2,n]): workgroup `block` sums 16 columns — 16 lane groups take every 16th row (four independent chains
// each, so the loads overlap), then an LDS reduce.  A device function because two kernels run it: the plain
// reduce launch and the training step's combined tail launch (gdn_head_train.hip).
__device__ __forceinline__ void gdn_project_reduce_body(const float* __restrict__ part, int rows, int d, int n, int w,
                                                        int wp, float* __restrict__ d_lin_w, float* __restrict__ d_a,
                                                        float* __restrict__ d_c, int block) {
  __shared__ float red[16][17];
  const int len = d * wp + 128 + 2 * n;
  const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int t = block * 16 + c;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (t < len) {
    int r = g;
    for (; r + 48 < rows; r += 64) {
      s0 += part[(size_t)r * len + t];
      s1 += part[(size_t)(r + 16) * len + t];
      s2 += part[(size_t)(r + 32) * len + t];
      s3 += part[(size_t)(r + 48) * len + t];
    }
    for (; r < rows; r += 16) s0 += part[(size_t)r * len + t];
  }
  red[g][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g != 0 || t >= len) return;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) s += red[q][c];
  if (t < d * wp) {
    const int cc = t / d, r = t - cc * d;     // partial rows hold d_lin_w column-major (c*D + d)
    if (cc < w) d_lin_w[(size_t)r * w + cc] = s;
  } else if (t < d * wp + 128) {
    d_a[t - d * wp] = s;
  } else {
    d_c[t - d * wp - 128] = s;
  }
}
