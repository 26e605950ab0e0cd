// Sliding windows longer than GDN_MAX_W = 64 ticks, up to GDN_LONG_MAX_W = 1024 (include/gdn_hip.h "Supported
// shapes").  The window length enters the graph layer only through the projection x[B*n, w] . lin^T (models/
// graph_layer.py:25,56) and the folded logit terms a = lin^T att; everything after xlin depends on n, d and k only
// and runs on the tile / large-form kernels unchanged.  The entry points of gdn_forward.hip, gdn_backward.hip and
// gdn_graph.hip hand every w > 64 call to the functions at the end of this file before any w <= 64 path runs.
//
// Node terms: a_i / a_j are stored at the pitch P = gdn_terms_pitch(w) = round_up(w, 64) (64 for w <= 64, the
// layout every other kernel reads), so node_terms = [a_i(P) | a_j(P) | c_i(n) | c_j(n)].
//
// Forward projection on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, the result equals a
// k-ordered fmaf chain).  Workgroup = 4 waves = LW_ROWS rows, each wave two 16-row blocks times all D columns.  The
// k axis is walked in chunks of LW_KC: lin^T [KC][D] and the x rows [ROWS][KC] are staged in LDS, and the next
// chunk's global loads are in flight while the matrix cores work on the current one.  s_i / s_j ride along on the
// VALU from the A operand already in registers (per-lane partial sums over k = q mod 4, then a fixed xor
// butterfly).  x rows are read at xb + b*bstride + s*sstride: the materialised windows [B, n, w] and the raw series
// [n, T] share the arithmetic, only the loads differ (16-byte loads where every row start is 16-byte aligned):
// both give the same bits.  No 16-bit operands: no range limit.
//
// Backward: d_lin_w[d, w] and d_a[2, P] are the product G^T X with G = [d_xlin | d_si | d_sj] ([rows, d + 2]).  A
// fixed number of row ranges (LWB_PARTS) each leave one partial [d + 2, w] block in the workspace; the reduce
// launch adds the blocks in range order and d_c[2, n] = sum over windows of d_si / d_sj in window order.  No
// floating-point atomics: bitwise reproducible.
#include "gdn_common.hpp"

namespace {

#define LW_NT 256                  // threads per workgroup: 4 waves
#define LW_ROWS 128                // rows per workgroup: 32 per wave
#define LW_KC 32                   // k chunk
#define LW_XP (LW_KC + 4)          // x tile pitch: 16-byte rows, the 4 k-groups of a read land on different banks
#define LWB_PARTS 64               // row ranges (partial blocks) of the backward
#define LWB_RC 32                  // rows per LDS chunk of the backward

typedef float lw_f32x4 __attribute__((ext_vector_type(4)));

static bool long_shape_ok(int n, int w, int d) {
  return (d == 16 || d == 32 || d == 64 || d == 128) && n <= 4096 && w > GDN_MAX_W && w <= GDN_LONG_MAX_W;
}

// ---- folded logit terms ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gdn_long_node_terms_kernel(
    const float* __restrict__ lin_w, const float* __restrict__ att_i, const float* __restrict__ att_j,
    const float* __restrict__ att_em_i, const float* __restrict__ att_em_j, const float* __restrict__ emb, int n,
    int d, int w, int ap, float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 2 * ap) {
    const int col = t % ap;
    const float* att = t < ap ? att_i : att_j;
    float acc = 0.f;
    if (col < w)
      for (int r = 0; r < d; ++r) acc = fmaf(lin_w[(size_t)r * w + col], att[r], acc);
    out[t] = acc;
  } else if (t < 2 * ap + 2 * n) {
    const int u = t - 2 * ap;
    const int s = u % n;
    const float* att = u < n ? att_em_i : att_em_j;
    float acc = 0.f;
    for (int r = 0; r < d; ++r) acc = fmaf(emb[(size_t)s * d + r], att[r], acc);
    out[t] = acc;
  }
}

// ---- forward projection ---------------------------------------------------------------------------------------
// A operand (16x16x4): lane l holds x[row = l & 15][k = l >> 4]; B: lin^T[k = l >> 4][col = l & 15];
// C/D: register r of lane l = xlin[row 4 (l >> 4) + r][col l & 15].
template <int D, bool VEC>
__global__ __launch_bounds__(LW_NT) void gdn_long_project_kernel(
    const float* __restrict__ xb, long long bstride, long long sstride, const float* __restrict__ lin_w,
    const float* __restrict__ terms, int rows, int n, int w, int ap, float* __restrict__ xlin,
    float* __restrict__ s_i, float* __restrict__ s_j) {
  constexpr int LP = D + 16;                        // lin^T chunk pitch: the 4 k rows of a read on different banks
  constexpr int CB = D / 16;                        // 16-column blocks
  constexpr int XU = LW_ROWS * LW_KC / LW_NT;       // x values per thread per chunk (16)
  constexpr int WU = D * LW_KC / LW_NT;             // lin values per thread per chunk (D / 8)
  __shared__ float4 xs4[LW_ROWS * LW_XP / 4];
  __shared__ float ls[LW_KC * LP];
  __shared__ float as[2 * LW_KC];
  __shared__ long long roff[LW_ROWS];
  float* xs = reinterpret_cast<float*>(xs4);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i16 = lane & 15, q = lane >> 4;
  const int r0 = (int)blockIdx.x * LW_ROWS;
  for (int r = tid; r < LW_ROWS; r += LW_NT) {
    const int row = min(r0 + r, rows - 1);          // rows past the end re-read the last one (never stored)
    const int b = row / n, s = row - b * n;
    roff[r] = b * bstride + s * sstride;
  }
  __syncthreads();

  float xv[XU], lv[WU], avv = 0.f;
  auto load = [&](int k0) {
    if constexpr (VEC) {
#pragma unroll
      for (int u = 0; u < XU / 4; ++u) {
        const int e = tid + u * LW_NT, r = e >> 3, k = k0 + 4 * (e & 7);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < w) v = *reinterpret_cast<const float4*>(xb + roff[r] + k);   // w % 4 == 0: all four inside
        xv[4 * u] = v.x; xv[4 * u + 1] = v.y; xv[4 * u + 2] = v.z; xv[4 * u + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int e = tid + u * LW_NT, r = e >> 5, k = k0 + (e & 31);
        xv[u] = k < w ? xb[roff[r] + k] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < WU; ++u) {
      const int e = tid + u * LW_NT, col = e >> 5, k = k0 + (e & 31);
      lv[u] = k < w ? lin_w[(size_t)col * w + k] : 0.f;
    }
    if (tid < 2 * LW_KC) {
      const int k = k0 + (tid & 31);
      avv = k < w ? terms[(tid >> 5) * ap + k] : 0.f;
    }
  };
  auto store = [&]() {
    if constexpr (VEC) {
#pragma unroll
      for (int u = 0; u < XU / 4; ++u) {
        const int e = tid + u * LW_NT, r = e >> 3, c = 4 * (e & 7);
        xs4[(r * LW_XP + c) / 4] = make_float4(xv[4 * u], xv[4 * u + 1], xv[4 * u + 2], xv[4 * u + 3]);
      }
    } else {
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int e = tid + u * LW_NT;
        xs[(e >> 5) * LW_XP + (e & 31)] = xv[u];
      }
    }
#pragma unroll
    for (int u = 0; u < WU; ++u) {
      const int e = tid + u * LW_NT;
      ls[(e & 31) * LP + (e >> 5)] = lv[u];
    }
    if (tid < 2 * LW_KC) as[tid] = avv;
  };

  lw_f32x4 acc[2][CB];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[rb][cb] = lw_f32x4{0.f, 0.f, 0.f, 0.f};
  float pi[2] = {0.f, 0.f}, pj[2] = {0.f, 0.f};
  const int nch = (w + LW_KC - 1) / LW_KC;
  load(0);
  for (int ch = 0; ch < nch; ++ch) {
    __syncthreads();                                  // the previous chunk is consumed
    store();
    __syncthreads();
    if (ch + 1 < nch) load((ch + 1) * LW_KC);         // in flight during this chunk's MFMAs
#pragma unroll
    for (int kk = 0; kk < LW_KC / 4; ++kk) {
      const int k = 4 * kk + q;
      float a[2];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) a[rb] = xs[(wv * 32 + rb * 16 + i16) * LW_XP + k];
      const float ai = as[k], aj = as[LW_KC + k];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        pi[rb] = fmaf(a[rb], ai, pi[rb]);
        pj[rb] = fmaf(a[rb], aj, pj[rb]);
      }
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const float bv = ls[k * LP + cb * 16 + i16];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb], bv, acc[rb][cb], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int rbase = r0 + wv * 32 + rb * 16;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rbase + 4 * q + r;
        if (row < rows) xlin[(size_t)row * D + cb * 16 + i16] = acc[rb][cb][r];
      }
    float si = pi[rb], sj = pj[rb];                   // the four k-groups of the row, in a fixed order
    si += __shfl_xor(si, 16);
    sj += __shfl_xor(sj, 16);
    si += __shfl_xor(si, 32);
    sj += __shfl_xor(sj, 32);
    const int row = rbase + i16;
    if (q == 0 && row < rows) {
      const int s = row % n;
      s_i[row] = si + terms[2 * ap + s];
      s_j[row] = sj + terms[2 * ap + n + s];
    }
  }
}

// ---- backward: partial blocks [d + 2, w] of G^T X per row range -------------------------------------------------
// Workgroup (range p, 64-column tile): thread = one column k, the 4 waves take the outputs o = wave, wave + 4, ...
// (G values are wave-uniform LDS broadcasts).
template <int D>
__global__ __launch_bounds__(256) void gdn_long_project_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ d_xlin, const float* __restrict__ d_si,
    const float* __restrict__ d_sj, int rows, int w, int per, float* __restrict__ part) {
  constexpr int O = D + 2, NO = (O + 3) / 4;
  __shared__ float gs[LWB_RC * O];
  __shared__ float xs[LWB_RC * 64];
  const int tid = threadIdx.x, col = tid & 63, g = tid >> 6;
  const int p = blockIdx.x, k0 = blockIdx.y * 64;
  const int ra = p * per, rb = min(rows, ra + per);
  float acc[NO];
#pragma unroll
  for (int j = 0; j < NO; ++j) acc[j] = 0.f;
  for (int c0 = ra; c0 < rb; c0 += LWB_RC) {
    const int cnt = min(LWB_RC, rb - c0);
    __syncthreads();
    for (int t = tid; t < cnt * O; t += 256) {
      const int r = t / O, o = t - r * O;
      const size_t row = (size_t)c0 + r;
      gs[t] = o < D ? d_xlin[row * D + o] : (o == D ? d_si[row] : d_sj[row]);
    }
    for (int t = tid; t < cnt * 64; t += 256) {
      const int r = t >> 6, k = k0 + (t & 63);
      xs[t] = k < w ? x[((size_t)c0 + r) * w + k] : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < cnt; ++r) {
      const float xv = xs[r * 64 + col];
      const float* gr = gs + r * O;
#pragma unroll
      for (int j = 0; j < NO; ++j)
        if (g + 4 * j < O) acc[j] = fmaf(gr[g + 4 * j], xv, acc[j]);
    }
  }
  if (k0 + col < w) {
    float* out = part + (size_t)p * O * w;
#pragma unroll
    for (int j = 0; j < NO; ++j)
      if (g + 4 * j < O) out[(size_t)(g + 4 * j) * w + k0 + col] = acc[j];
  }
}

// out = the partial blocks added in range order -> d_lin_w[d, w], d_a[2, ap] (zero padded); d_c[2, n] = sums of
// d_si / d_sj over the windows in window order (d_si == null: d_c is left alone)
__global__ __launch_bounds__(256) void gdn_long_project_reduce_kernel(
    const float* __restrict__ part, int parts, int d, int w, int ap, int n, int batch, const float* __restrict__ d_si,
    const float* __restrict__ d_sj, float* __restrict__ d_lin_w, float* __restrict__ d_a, float* __restrict__ d_c) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int nw = (d + 2) * w, pad = ap - w;
  if (t < nw) {
    float s = 0.f;
    for (int p = 0; p < parts; ++p) s += part[(size_t)p * nw + t];
    const int o = t / w, k = t - o * w;
    if (o < d) d_lin_w[t] = s;
    else d_a[(o - d) * ap + k] = s;
  } else if (t < nw + 2 * pad) {
    const int u = t - nw, which = u / pad;
    d_a[which * ap + w + (u - which * pad)] = 0.f;
  } else if (t < nw + 2 * pad + 2 * n && d_si) {
    const int u = t - nw - 2 * pad, which = u / n, s = u - which * n;
    const float* ds = which ? d_sj : d_si;
    float acc = 0.f;
    for (int b = 0; b < batch; ++b) acc += ds[(size_t)b * n + s];
    d_c[u] = acc;
  }
}

// chain rule through the folded terms at pitch ap (gdn_backward.hip's gdn_terms_bwd_kernel with a = [2, ap])
__global__ __launch_bounds__(1024) void gdn_long_terms_bwd_kernel(
    const float* __restrict__ lin_w, const float* __restrict__ att_i, const float* __restrict__ att_j,
    const float* __restrict__ att_em_i, const float* __restrict__ att_em_j, const float* __restrict__ emb,
    const float* __restrict__ d_a, const float* __restrict__ d_c, int n, int d, int w, int ap,
    float* __restrict__ d_lin_w, float* __restrict__ d_att_i, float* __restrict__ d_att_j,
    float* __restrict__ d_att_em_i, float* __restrict__ d_att_em_j, float* __restrict__ d_emb, int accumulate_emb) {
  const int tid = threadIdx.x;
  constexpr int NT = 1024;
  for (int t = blockIdx.x * NT + tid; t < n * d; t += gridDim.x * NT) {
    const int s = t / d, c = t - s * d;
    const float v = fmaf(d_c[s], att_em_i[c], d_c[n + s] * att_em_j[c]);
    d_emb[t] = accumulate_emb ? d_emb[t] + v : v;
  }
  if (blockIdx.x != 0) return;
  __shared__ float part[4][NT];
  for (int t = tid; t < d * w; t += NT) {
    const int c = t / w, q = t - c * w;
    d_lin_w[t] += fmaf(att_i[c], d_a[q], att_j[c] * d_a[ap + q]);
  }
  const int c = tid % d, g = tid / d, groups = NT / d;
  float si = 0.f, sj = 0.f, ei = 0.f, ej = 0.f;
#pragma unroll 8
  for (int q = g; q < w; q += groups) {
    const float lw = lin_w[c * w + q];
    si = fmaf(lw, d_a[q], si);
    sj = fmaf(lw, d_a[ap + q], sj);
  }
#pragma unroll 8
  for (int s = g; s < n; s += groups) {
    const float ev = emb[(size_t)s * d + c];
    ei = fmaf(ev, d_c[s], ei);
    ej = fmaf(ev, d_c[n + s], ej);
  }
  part[0][tid] = si; part[1][tid] = sj; part[2][tid] = ei; part[3][tid] = ej;
  __syncthreads();
  if (tid < d) {
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < groups; ++q)
#pragma unroll
      for (int v = 0; v < 4; ++v) r[v] += part[v][q * d + tid];
    d_att_i[tid] = r[0];
    d_att_j[tid] = r[1];
    d_att_em_i[tid] = r[2];
    d_att_em_j[tid] = r[3];
  }
}

static int long_bwd_parts(int rows) { return min(LWB_PARTS, (rows + LWB_RC - 1) / LWB_RC); }

}  // namespace

extern "C" int gdn_terms_pitch(int w) {
  if (w <= 0 || w > GDN_LONG_MAX_W) return 0;
  return w <= GDN_A_PITCH ? GDN_A_PITCH : (w + 63) & ~63;
}

int gdn_long_node_terms(const float* lin_w, const float* att_i, const float* att_j, const float* att_em_i,
                        const float* att_em_j, const float* emb, int n, int d, int w, float* node_terms,
                        hipStream_t st) {
  if (w > GDN_LONG_MAX_W) return GDN_ERR_UNSUPPORTED;
  const int ap = gdn_terms_pitch(w), total = 2 * ap + 2 * n;
  hipLaunchKernelGGL(gdn_long_node_terms_kernel, dim3((total + 255) / 256), dim3(256), 0, st, lin_w, att_i, att_j,
                     att_em_i, att_em_j, emb, n, d, w, ap, node_terms);
  return gdn_launch_status();
}

int gdn_long_project(const float* xb, long long bstride, long long sstride, const float* lin_w, const float* terms,
                     int batch, int n, int w, int d, float* xlin, float* s_i, float* s_j, hipStream_t st) {
  if (batch <= 0 || n <= 0 || w <= 0) return GDN_ERR_ARG;
  if (!long_shape_ok(n, w, d)) return GDN_ERR_UNSUPPORTED;
  const long long rows_ll = (long long)batch * n;
  if (rows_ll > 0x7fffffffLL) return GDN_ERR_UNSUPPORTED;
  const int rows = (int)rows_ll, ap = gdn_terms_pitch(w);
  const int grid = (rows + LW_ROWS - 1) / LW_ROWS;
  const bool vec = (w % 4) == 0 && (bstride % 4) == 0 && (sstride % 4) == 0 && ((uintptr_t)xb & 15) == 0;
#define GDN_LWP(DD)                                                                                              \
  case DD:                                                                                                       \
    if (vec)                                                                                                     \
      hipLaunchKernelGGL((gdn_long_project_kernel<DD, true>), dim3(grid), dim3(LW_NT), 0, st, xb, bstride, sstride, \
                         lin_w, terms, rows, n, w, ap, xlin, s_i, s_j);                                          \
    else                                                                                                         \
      hipLaunchKernelGGL((gdn_long_project_kernel<DD, false>), dim3(grid), dim3(LW_NT), 0, st, xb, bstride,      \
                         sstride, lin_w, terms, rows, n, w, ap, xlin, s_i, s_j);                                 \
    break;
  switch (d) {
    GDN_LWP(16)
    GDN_LWP(32)
    GDN_LWP(64)
    GDN_LWP(128)
  }
#undef GDN_LWP
  return gdn_launch_status();
}

long long gdn_long_project_bwd_workspace_bytes(int n, int w, int d) {
  if (!long_shape_ok(n, w, d)) return 0;
  return (long long)LWB_PARTS * (d + 2) * w * (long long)sizeof(float);
}

int gdn_long_project_bwd_partials(const float* x, const float* d_xlin, const float* d_si, const float* d_sj, int batch,
                                  int n, int w, int d, float* workspace, int* parts_out, hipStream_t st) {
  if (!long_shape_ok(n, w, d)) return GDN_ERR_UNSUPPORTED;
  const long long rows_ll = (long long)batch * n;
  if (rows_ll > 0x7fffffffLL) return GDN_ERR_UNSUPPORTED;
  const int rows = (int)rows_ll, parts = long_bwd_parts(rows), per = (rows + parts - 1) / parts;
  const dim3 grid(parts, (w + 63) / 64);
#define GDN_LWB(DD)                                                                                              \
  case DD:                                                                                                       \
    hipLaunchKernelGGL((gdn_long_project_bwd_kernel<DD>), grid, dim3(256), 0, st, x, d_xlin, d_si, d_sj, rows, w, \
                       per, workspace);                                                                          \
    break;
  switch (d) {
    GDN_LWB(16)
    GDN_LWB(32)
    GDN_LWB(64)
    GDN_LWB(128)
  }
#undef GDN_LWB
  *parts_out = parts;
  return gdn_launch_status();
}

// the partial blocks added in range order (also the reduce of gdn_any_width.hip's projection backward, any w)
int gdn_long_project_reduce(const float* part, int parts, int batch, int n, int w, int d, const float* d_si,
                            const float* d_sj, float* d_lin_w, float* d_a, float* d_c, hipStream_t st) {
  const int ap = gdn_terms_pitch(w);
  const int total = (d + 2) * w + 2 * (ap - w) + 2 * n;
  hipLaunchKernelGGL(gdn_long_project_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, part, parts, d,
                     w, ap, n, batch, d_si, d_sj, d_lin_w, d_a, d_c);
  return gdn_launch_status();
}

int gdn_long_terms_bwd(const float* lin_w, const float* att_i, const float* att_j, const float* att_em_i,
                       const float* att_em_j, const float* emb, const float* d_a, const float* d_c, int n, int d, int w,
                       float* d_lin_w, float* d_att_i, float* d_att_j, float* d_att_em_i, float* d_att_em_j,
                       float* d_emb, int accumulate_emb, hipStream_t st) {
  // any d <= 256: a workgroup's 1024 threads hold 1024 / d whole column groups (the rest idle)
  if (w > GDN_LONG_MAX_W || d > 256 || (!gdn_any_width(d) && (256 % d) != 0)) return GDN_ERR_UNSUPPORTED;
  int grid = (n * d + 1024 * 2 - 1) / (1024 * 2);
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(gdn_long_terms_bwd_kernel, dim3(grid), dim3(1024), 0, st, lin_w, att_i, att_j, att_em_i,
                     att_em_j, emb, d_a, d_c, n, d, w, gdn_terms_pitch(w), d_lin_w, d_att_i, d_att_j, d_att_em_i,
                     d_att_em_j, d_emb, accumulate_emb);
  return gdn_launch_status();
}
