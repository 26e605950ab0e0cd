// Graph layer beyond the LDS tile (include/gdn_hip.h "Supported shapes", large-graph form): the kernels that
// gdn_project_fwd, gdn_attn_aggregate_fwd and gdn_attn_aggregate_bwd run where the window's projected tile
// (n+1) x d fp32 does not fit the 160 KB of one CU (make_plan / bwd_plan refuse), up to n = 4096.
//
// Nothing [n, d]-sized lives in LDS.  xlin stays in global memory and every target gathers its k + 1 source
// rows from there; a workgroup holds only the window's s_j (<= 16 KB) and, per wave, one target's list entries
// and weights.  Work split: workgroup = (window, block of LARGE_TPB targets), one wave per target at a time.
// Lane layout of a gather: a row of d floats is LPR = d/4 lanes of one float4 each; the NG = 64/LPR lane
// groups of a wave take the list slots p = g, g + NG, ... and meet in a fixed xor butterfly at the end.
//
// Placement: blocks L and L + 8 run on the same XCD (MI355X dispatches workgroups round robin over its 8 XCDs),
// so block L serves window 8 * ((L / 8) / T) + L % 8, target block (L / 8) % T: all T target blocks of a window
// share one XCD and its 4 MiB L2, which then holds that window's xlin (n * d * 4 bytes, 0.25 - 2 MB).
//
// No atomics except the d_bias ticket (gdn_colsum_ticket: integer, fixed-order sum): bitwise reproducible.
#include "gdn_common.hpp"

namespace {

#define LARGE_TPB 64      // targets (sources, in the backward's second pass) per workgroup
#define LARGE_NT 256      // threads per workgroup: 4 waves
#define LARGE_PROJ_ROWS 64

template <int D>
struct LG {
  static constexpr int LPR = D / 4;      // lanes per row
  static constexpr int NG = 64 / LPR;    // lane groups per wave
};

__device__ __forceinline__ float wave_max(float v) {
  v = row16_max(v);
  v = fmaxf(v, __shfl_xor(v, 16));
  v = fmaxf(v, __shfl_xor(v, 32));
  return v;
}

__device__ __forceinline__ void fma4(float a, const float4& x, float4& acc) {
  acc.x = fmaf(a, x.x, acc.x);
  acc.y = fmaf(a, x.y, acc.y);
  acc.z = fmaf(a, x.z, acc.z);
  acc.w = fmaf(a, x.w, acc.w);
}

// sum over the lane groups of a wave (xor butterfly over the lane bits above the row's): every lane ends with
// the same bits (each step adds the same two operands on both sides)
template <int D>
__device__ __forceinline__ void group_sum(float4& acc) {
#pragma unroll
  for (int off = LG<D>::LPR; off < 64; off <<= 1) {
    acc.x += __shfl_xor(acc.x, off);
    acc.y += __shfl_xor(acc.y, off);
    acc.z += __shfl_xor(acc.z, off);
    acc.w += __shfl_xor(acc.w, off);
  }
}

// (window, first target) of this workgroup, or false past the last window
__device__ __forceinline__ bool large_place(int tblocks, int batch, int& b, int& t0) {
  const int L = (int)blockIdx.x, s = L >> 3;
  b = (s / tblocks) * 8 + (L & 7);
  t0 = (s % tblocks) * LARGE_TPB;
  return b < batch;
}

static int large_grid(int batch, int n) {
  const int tblocks = (n + LARGE_TPB - 1) / LARGE_TPB;
  return ((batch + 7) / 8) * 8 * tblocks;
}

// ---- projection: xlin = x lin^T, s_i / s_j, streamed by rows ----------------------------------------------
// Row r = b*n + s of window b reads x at xb + b * bstride + s * sstride + [0, w): bstride = n*w, sstride = w for
// materialised windows [B, n, w], bstride = 1, sstride = series_len for the raw series [n, T] (xb = series +
// first).  One arithmetic for both: the two forms give the same bits.
template <int D>
__global__ __launch_bounds__(LARGE_NT) void gdn_large_project_kernel(
    const float* __restrict__ xb, long long bstride, long long sstride, const float* __restrict__ lin_w,
    const float* __restrict__ terms, int rows, int n, int w, float* __restrict__ xlin, float* __restrict__ s_i,
    float* __restrict__ s_j) {
  constexpr int LPR = LG<D>::LPR;
  __shared__ float4 wt4[GDN_MAX_W * D / 4];                     // lin^T [w][D]
  __shared__ float xs[LARGE_PROJ_ROWS * (GDN_MAX_W + 1)];       // x rows, pitch w + 1
  float* wt = reinterpret_cast<float*>(wt4);
  const int tid = threadIdx.x, xp = w + 1;
  for (int t = tid; t < w * D; t += LARGE_NT) {
    const int c = t / D, col = t - c * D;
    wt[t] = lin_w[(size_t)col * w + c];
  }
  const int r0 = (int)blockIdx.x * LARGE_PROJ_ROWS;
  for (int t = tid; t < LARGE_PROJ_ROWS * w; t += LARGE_NT) {
    const int r = t / w, c = t - r * w, row = r0 + r;
    if (row < rows) {
      const int b = row / n, s = row - b * n;
      xs[r * xp + c] = xb[b * bstride + s * sstride + c];
    }
  }
  __syncthreads();
  const int c0 = (tid % LPR) * 4;
  for (int r = tid / LPR; r < LARGE_PROJ_ROWS; r += LARGE_NT / LPR) {
    const int row = r0 + r;
    if (row >= rows) break;
    const float* xr = xs + r * xp;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < w; ++c) fma4(xr[c], wt4[c * (D / 4) + c0 / 4], acc);
    *reinterpret_cast<float4*>(xlin + (size_t)row * D + c0) = acc;
  }
  if (tid < LARGE_PROJ_ROWS && r0 + tid < rows) {   // the attention scalars: one thread per row
    const int row = r0 + tid, s = row % n;
    const float* xr = xs + tid * xp;
    float pi = 0.f, pj = 0.f;
    for (int c = 0; c < w; ++c) {
      pi = fmaf(xr[c], terms[c], pi);
      pj = fmaf(xr[c], terms[GDN_A_PITCH + c], pj);
    }
    s_i[row] = pi + terms[2 * GDN_A_PITCH + s];
    s_j[row] = pj + terms[2 * GDN_A_PITCH + n + s];
  }
}

// ---- gather-aggregate forward -------------------------------------------------------------------------------
// Per target (one wave): logits LeakyReLU(s_i + s_j[j]) over its list slots, max, exp, sum, 1/(sum + 1e-16)
// as the tile kernel; then z = sum_p alpha_p xlin[j_p] + bias with the source rows read from global memory.
// Padding slots (index n) get weight 0 and are never read: the kernel skips by index, not by degree.
template <int D>
__global__ __launch_bounds__(LARGE_NT) void gdn_large_aggregate_kernel(
    const float* __restrict__ xlin, const float* __restrict__ s_i, const float* __restrict__ s_j,
    const uint16_t* __restrict__ nbr, const float* __restrict__ bias, int batch, int n, int pitch, int tblocks,
    float* __restrict__ z, float* __restrict__ alpha) {
  constexpr int LPR = LG<D>::LPR, NG = LG<D>::NG;
  extern __shared__ float4 smem_l4[];
  float* smem = reinterpret_cast<float*>(smem_l4);
  int b, t0;
  if (!large_place(tblocks, batch, b, t0)) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int npad = (n + 3) & ~3;
  float* sj = smem;
  float* wl = smem + npad + wave * 2 * pitch;             // this wave's weights [pitch]
  int* jl = reinterpret_cast<int*>(wl + pitch);           // and list entries [pitch]
  const size_t row0 = (size_t)b * n;
  for (int t = tid; t < n; t += LARGE_NT) sj[t] = s_j[row0 + t];
  __syncthreads();
  const int g = lane / LPR, c0 = (lane % LPR) * 4;
  const float4 bv = *reinterpret_cast<const float4*>(bias + c0);
  const float* xw = xlin + row0 * D + c0;
  const int t1 = min(n, t0 + LARGE_TPB);
  for (int i = t0 + wave; i < t1; i += LARGE_NT / 64) {
    const float sti = s_i[row0 + i];
    const uint16_t* lst = nbr + (size_t)i * pitch;
    float m = -INFINITY;
    for (int p = lane; p < pitch; p += 64) {
      const int j = lst[p];
      const float e = j < n ? leaky(sti + sj[j]) : -INFINITY;
      wl[p] = e;
      jl[p] = j;
      m = fmaxf(m, e);
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int p = lane; p < pitch; p += 64) {
      const float ex = __expf(wl[p] - m);      // exp(-inf) = 0 in the padding slots
      wl[p] = ex;
      sum += ex;
    }
    sum = wave_sum(sum);
    const float inv = __builtin_amdgcn_rcpf(sum + GDN_SOFTMAX_EPS);
    float* arow = alpha ? alpha + (row0 + i) * pitch : nullptr;
    for (int p = lane; p < pitch; p += 64) {
      const float a = wl[p] * inv;
      wl[p] = a;
      if (arow) arow[p] = a;
    }
    __builtin_amdgcn_wave_barrier();
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int p = g; p < pitch; p += NG) {
      const int j = jl[p];
      if (j < n) fma4(wl[p], *reinterpret_cast<const float4*>(xw + (size_t)j * D), acc);
    }
    group_sum<D>(acc);
    if (g == 0) {
      acc.x += bv.x; acc.y += bv.y; acc.z += bv.z; acc.w += bv.w;
      *reinterpret_cast<float4*>(z + (row0 + i) * D + c0) = acc;
    }
    __builtin_amdgcn_wave_barrier();   // wl / jl are rewritten for the next target
  }
}

// ---- backward, pass 1 (per target) ---------------------------------------------------------------------------
//   d_alpha_p = d_z_i . xlin[j_p]  (the row's LPR lanes add their float4 dots in a butterfly)
//   d_e_p = alpha_p (d_alpha_p - sum_q alpha_q d_alpha_q);  d_pi_p = d_e_p * (pi_p > 0 ? 1 : 0.2)  -> dpi_ws
//   d_s_i = (0.2 - 1) * sum of d_e_p over the negative-logit slots (the tile kernel's form)
template <int D>
__global__ __launch_bounds__(LARGE_NT) void gdn_large_bwd_target_kernel(
    const float* __restrict__ d_z, const float* __restrict__ xlin, const float* __restrict__ alpha,
    const float* __restrict__ s_i, const float* __restrict__ s_j, const uint16_t* __restrict__ nbr, int batch,
    int n, int pitch, int tblocks, float* __restrict__ d_si, float* __restrict__ dpi_ws) {
  constexpr int LPR = LG<D>::LPR, NG = LG<D>::NG;
  extern __shared__ float4 smem_l4[];
  float* smem = reinterpret_cast<float*>(smem_l4);
  int b, t0;
  if (!large_place(tblocks, batch, b, t0)) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int npad = (n + 3) & ~3;
  float* sj = smem;
  float* da = smem + npad + wave * 2 * pitch;             // d_alpha [pitch]
  int* jl = reinterpret_cast<int*>(da + pitch);
  const size_t row0 = (size_t)b * n;
  for (int t = tid; t < n; t += LARGE_NT) sj[t] = s_j[row0 + t];
  __syncthreads();
  const int g = lane / LPR, c0 = (lane % LPR) * 4;
  const float* xw = xlin + row0 * D + c0;
  const int t1 = min(n, t0 + LARGE_TPB);
  for (int i = t0 + wave; i < t1; i += LARGE_NT / 64) {
    const size_t ri = row0 + i;
    const float4 gz = *reinterpret_cast<const float4*>(d_z + ri * D + c0);
    const uint16_t* lst = nbr + (size_t)i * pitch;
    for (int p = g; p < pitch; p += NG) {       // pitch is a multiple of 16: the same trip count for every group
      const int j = lst[p];
      float part = 0.f;
      if (j < n) {
        const float4 x = *reinterpret_cast<const float4*>(xw + (size_t)j * D);
        part = fmaf(gz.x, x.x, fmaf(gz.y, x.y, fmaf(gz.z, x.z, gz.w * x.w)));
      }
#pragma unroll
      for (int off = 1; off < LPR; off <<= 1) part += __shfl_xor(part, off);
      if (lane % LPR == 0) {
        da[p] = part;
        jl[p] = j;
      }
    }
    __builtin_amdgcn_wave_barrier();
    const float* arow = alpha + ri * pitch;
    float dot = 0.f;
    for (int p = lane; p < pitch; p += 64) dot = fmaf(arow[p], da[p], dot);
    dot = wave_sum(dot);
    const float sti = s_i[ri];
    float dsi = 0.f;
    float* drow = dpi_ws + ri * pitch;
    for (int p = lane; p < pitch; p += 64) {
      const int j = jl[p];
      float dpi = 0.f;
      if (j < n) {
        const float de = arow[p] * (da[p] - dot);
        const float pi = sti + sj[j];
        dpi = de * (pi > 0.f ? 1.f : GDN_NEG_SLOPE);
        dsi += pi > 0.f ? 0.f : de;
      }
      drow[p] = dpi;
    }
    dsi = wave_sum(dsi) * (GDN_NEG_SLOPE - 1.f);
    if (lane == 0) d_si[ri] = dsi;
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- backward, pass 2 (per source j, over the reverse lists) ------------------------------------------------
//   d_xlin[j] = sum_(i,p) alpha_ip d_z_i ;  d_s_j[j] = sum_(i,p) d_pi_ip
template <int D>
__global__ __launch_bounds__(LARGE_NT) void gdn_large_bwd_source_kernel(
    const float* __restrict__ d_z, const float* __restrict__ alpha, const float* __restrict__ dpi_ws,
    const uint32_t* __restrict__ rent, const int32_t* __restrict__ rlen, int batch, int n, int pitch, int rpitch,
    int tblocks, float* __restrict__ d_xlin, float* __restrict__ d_sj) {
  constexpr int LPR = LG<D>::LPR, NG = LG<D>::NG;
  int b, t0;
  if (!large_place(tblocks, batch, b, t0)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, c0 = (lane % LPR) * 4;
  const size_t row0 = (size_t)b * n;
  const int t1 = min(n, t0 + LARGE_TPB);
  for (int j = t0 + wave; j < t1; j += LARGE_NT / 64) {
    const int cnt = rlen[j];
    const uint32_t* ents = rent + (size_t)j * rpitch;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float dsj = 0.f;
#pragma unroll 4
    for (int r = g; r < cnt; r += NG) {
      const uint32_t ent = ents[r];
      const size_t ti = row0 + (ent >> 16), p = ent & 0xffffu;
      fma4(alpha[ti * pitch + p], *reinterpret_cast<const float4*>(d_z + ti * D + c0), acc);
      if (lane % LPR == 0) dsj += dpi_ws[ti * pitch + p];
    }
    group_sum<D>(acc);
    dsj = wave_sum(dsj);
    if (g == 0) *reinterpret_cast<float4*>(d_xlin + (row0 + j) * D + c0) = acc;
    if (lane == 0) d_sj[row0 + j] = dsj;
  }
}

// ---- d_bias = column sums of d_z over all B*n rows: a fixed row range per workgroup, then gdn_colsum_ticket -----
template <int D>
__global__ __launch_bounds__(LARGE_NT) void gdn_large_bias_kernel(const float* __restrict__ d_z, int rows,
                                                                  float* __restrict__ d_bias,
                                                                  float* __restrict__ bias_ws) {
  constexpr int LPR = LG<D>::LPR, RG = LARGE_NT / LPR;   // row groups per workgroup
  __shared__ float4 part4[RG * D / 4];
  __shared__ float row[D];
  __shared__ float scratch[LARGE_NT];
  const int tid = threadIdx.x, rg = tid / LPR, c0 = (tid % LPR) * 4;
  const int per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
  const int r0 = (int)blockIdx.x * per, r1 = min(rows, r0 + per);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r = r0 + rg; r < r1; r += RG) {
    const float4 v = *reinterpret_cast<const float4*>(d_z + (size_t)r * D + c0);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  part4[rg * (D / 4) + c0 / 4] = acc;
  __syncthreads();
  const float* part = reinterpret_cast<const float*>(part4);
  if (tid < D) {
    float s = 0.f;
    for (int q = 0; q < RG; ++q) s += part[q * D + tid];
    row[tid] = s;
  }
  __syncthreads();
  gdn_colsum_ticket(bias_ws, row, D, d_bias, scratch);
}

static bool large_shape_ok(int n, int d, int k) {
  if (d != 16 && d != 32 && d != 64 && d != 128) return false;
  if (n > 4096) return false;
  if (k > 0 && (k > n || k + 1 > 1024)) return false;
  return true;
}

// dynamic LDS of the two per-target kernels: s_j of the window + two [pitch] arrays per wave (<= 48 KB at
// n = 4096, k = 1023: below the default limit, no attribute needed)
static int large_lds(int n, int pitch) { return (((n + 3) & ~3) + (LARGE_NT / 64) * 2 * pitch) * 4; }

}  // namespace

int gdn_large_project(const float* xb, long long bstride, long long sstride, const float* lin_w,
                      const float* terms, int batch, int n, int w, int d, float* xlin, float* s_i, float* s_j,
                      hipStream_t st) {
  if (w <= 0 || batch <= 0 || n <= 0) return GDN_ERR_ARG;
  if (w > GDN_MAX_W || !large_shape_ok(n, d, 0)) return GDN_ERR_UNSUPPORTED;
  const int rows = batch * n;
  const int grid = (rows + LARGE_PROJ_ROWS - 1) / LARGE_PROJ_ROWS;
#define GDN_LP(DD)                                                                                           \
  case DD:                                                                                                   \
    hipLaunchKernelGGL(gdn_large_project_kernel<DD>, dim3(grid), dim3(LARGE_NT), 0, st, xb, bstride, sstride, \
                       lin_w, terms, rows, n, w, xlin, s_i, s_j);                                            \
    break;
  switch (d) {
    GDN_LP(16)
    GDN_LP(32)
    GDN_LP(64)
    GDN_LP(128)
  }
#undef GDN_LP
  return gdn_launch_status();
}

int gdn_large_aggregate(const float* xlin, const float* s_i, const float* s_j, const uint16_t* nbr,
                        const float* bias, int batch, int n, int d, int k, float* z, float* alpha, hipStream_t st) {
  if (batch <= 0 || n <= 0 || k <= 0) return GDN_ERR_ARG;
  if (!large_shape_ok(n, d, k)) return GDN_ERR_UNSUPPORTED;
  const int pitch = gdn_nbr_pitch(k), tblocks = (n + LARGE_TPB - 1) / LARGE_TPB;
  const int lds = large_lds(n, pitch), grid = large_grid(batch, n);
#define GDN_LA(DD)                                                                                            \
  case DD:                                                                                                    \
    hipLaunchKernelGGL(gdn_large_aggregate_kernel<DD>, dim3(grid), dim3(LARGE_NT), lds, st, xlin, s_i, s_j, nbr, \
                       bias, batch, n, pitch, tblocks, z, alpha);                                             \
    break;
  switch (d) {
    GDN_LA(16)
    GDN_LA(32)
    GDN_LA(64)
    GDN_LA(128)
  }
#undef GDN_LA
  return gdn_launch_status();
}

// workspace layout as gdn_attn_aggregate_bwd's: [d_bias ticket + rows (bias_ws_floats)][batch*n*pitch d_pi]
int gdn_large_attn_bwd(const float* d_z, const float* xlin, const float* alpha, const float* s_i, const float* s_j,
                       const uint16_t* nbr, const uint32_t* rent, const int32_t* rlen, int batch, int n, int d, int k,
                       float* d_xlin, float* d_si, float* d_sj, float* d_bias, float* workspace,
                       long long bias_ws_floats, hipStream_t st) {
  if (batch <= 0 || n <= 0 || k <= 0 || !rent || !rlen) return GDN_ERR_ARG;
  if (!large_shape_ok(n, d, k)) return GDN_ERR_UNSUPPORTED;
  const int pitch = gdn_nbr_pitch(k), rpitch = (n + 15) & ~15, tblocks = (n + LARGE_TPB - 1) / LARGE_TPB;
  const int lds = large_lds(n, pitch), grid = large_grid(batch, n);
  const int rows = batch * n;
  const int bgrid = min(GDN_COLSUM_MAX_ROWS, (rows + 255) / 256);
  float* dpi_ws = workspace + bias_ws_floats;
#define GDN_LB(DD)                                                                                               \
  case DD:                                                                                                       \
    hipLaunchKernelGGL(gdn_large_bwd_target_kernel<DD>, dim3(grid), dim3(LARGE_NT), lds, st, d_z, xlin, alpha, s_i, \
                       s_j, nbr, batch, n, pitch, tblocks, d_si, dpi_ws);                                        \
    hipLaunchKernelGGL(gdn_large_bwd_source_kernel<DD>, dim3(grid), dim3(LARGE_NT), 0, st, d_z, alpha, dpi_ws,    \
                       rent, rlen, batch, n, pitch, rpitch, tblocks, d_xlin, d_sj);                              \
    hipLaunchKernelGGL(gdn_large_bias_kernel<DD>, dim3(bgrid), dim3(LARGE_NT), 0, st, d_z, rows, d_bias, workspace); \
    break;
  switch (d) {
    GDN_LB(16)
    GDN_LB(32)
    GDN_LB(64)
    GDN_LB(128)
  }
#undef GDN_LB
  return gdn_launch_status();
}
