// Embedding widths other than 16, 32, 64 and 128: any 1 <= d <= 256 (include/gdn_hip.h "Supported shapes").
// The staged entry points of gdn_forward.hip, gdn_backward.hip and gdn_head_train.hip hand every such d to the
// functions at the end of this file before any other path runs; the four tile widths never reach them.
//
// Every kernel here is instantiated on a padded width DP in {16, 32, 64, 128, 256}, the smallest >= d, and takes
// d at run time: columns >= d are read as zero and never stored, so xlin, z and their gradients stay dense
// [B*n, d] in HBM.  Row segments of four columns are read as one float4 where d % 4 == 0 (16-byte aligned rows),
// as two float2 where d % 2 == 0, else column by column (V = 4 / 2 / 1, chosen on the host).
//
// The graph-layer kernels follow gdn_large.hip: nothing [n, d]-sized in LDS, one list and its weights per wave,
// source rows gathered from global memory, a window's target blocks on one XCD (its xlin in that XCD's L2),
// padding slots skipped by index (== n), and no floating-point atomics (d_bias: gdn_colsum_ticket), so results are
// bitwise reproducible.  The projection is gdn_long_window.hip's fp32 matrix-core kernel with lin^T's columns >= d
// zero in LDS, at every w <= 1024 (both addressings, the same bits); its backward the per-range partial blocks and
// the fixed-order reduce of that file.
#include "gdn_common.hpp"

#include <initializer_list>

namespace {

#define AW_TPB 64      // targets (sources) per workgroup of the gather kernels
#define AW_NT 256      // threads per workgroup: 4 waves
#define AW_ROWS 128    // projection: rows per workgroup, 32 per wave
#define AW_KC 32       // projection: k chunk
#define AW_XP (AW_KC + 4)
#define AW_PARTS 64    // projection backward: row ranges
#define AW_RC 32       // projection backward: rows per LDS chunk

typedef float aw_f32x4 __attribute__((ext_vector_type(4)));

template <int DP>
struct AWG {
  static constexpr int LPR = DP / 4;     // lanes per row: four columns each
  static constexpr int NG = 64 / LPR;    // lane groups per wave
};

// columns c0 .. c0 + 3 of a row, zero at and beyond d
template <int V>
__device__ __forceinline__ float4 aw_load(const float* __restrict__ row, int c0, int d) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (V == 4) {
    if (c0 < d) v = *reinterpret_cast<const float4*>(row + c0);   // d % 4 == 0: all four inside
  } else if constexpr (V == 2) {
    if (c0 < d) {
      const float2 a = *reinterpret_cast<const float2*>(row + c0);
      v.x = a.x; v.y = a.y;
    }
    if (c0 + 2 < d) {
      const float2 b = *reinterpret_cast<const float2*>(row + c0 + 2);
      v.z = b.x; v.w = b.y;
    }
  } else {
    if (c0 < d) v.x = row[c0];
    if (c0 + 1 < d) v.y = row[c0 + 1];
    if (c0 + 2 < d) v.z = row[c0 + 2];
    if (c0 + 3 < d) v.w = row[c0 + 3];
  }
  return v;
}

template <int V>
__device__ __forceinline__ void aw_store(float* __restrict__ row, int c0, int d, const float4& v) {
  if constexpr (V == 4) {
    if (c0 < d) *reinterpret_cast<float4*>(row + c0) = v;
  } else if constexpr (V == 2) {
    if (c0 < d) *reinterpret_cast<float2*>(row + c0) = make_float2(v.x, v.y);
    if (c0 + 2 < d) *reinterpret_cast<float2*>(row + c0 + 2) = make_float2(v.z, v.w);
  } else {
    if (c0 < d) row[c0] = v.x;
    if (c0 + 1 < d) row[c0 + 1] = v.y;
    if (c0 + 2 < d) row[c0 + 2] = v.z;
    if (c0 + 3 < d) row[c0 + 3] = v.w;
  }
}

__device__ __forceinline__ float aw_wave_max(float v) {
  v = row16_max(v);
  v = fmaxf(v, __shfl_xor(v, 16));
  v = fmaxf(v, __shfl_xor(v, 32));
  return v;
}

__device__ __forceinline__ void aw_fma4(float a, const float4& x, float4& acc) {
  acc.x = fmaf(a, x.x, acc.x);
  acc.y = fmaf(a, x.y, acc.y);
  acc.z = fmaf(a, x.z, acc.z);
  acc.w = fmaf(a, x.w, acc.w);
}

// sum over the lane groups of a wave (fixed xor butterfly: every lane ends with the same bits)
template <int DP>
__device__ __forceinline__ void aw_group_sum(float4& acc) {
#pragma unroll
  for (int off = AWG<DP>::LPR; off < 64; off <<= 1) {
    acc.x += __shfl_xor(acc.x, off);
    acc.y += __shfl_xor(acc.y, off);
    acc.z += __shfl_xor(acc.z, off);
    acc.w += __shfl_xor(acc.w, off);
  }
}

// (window, first target) of this workgroup: blocks L and L + 8 share an XCD, so all target blocks of a window do
__device__ __forceinline__ bool aw_place(int tblocks, int batch, int& b, int& t0) {
  const int L = (int)blockIdx.x, s = L >> 3;
  b = (s / tblocks) * 8 + (L & 7);
  t0 = (s % tblocks) * AW_TPB;
  return b < batch;
}

static int aw_grid(int batch, int n) { return ((batch + 7) / 8) * 8 * ((n + AW_TPB - 1) / AW_TPB); }
static int aw_lds(int n, int pitch) { return (((n + 3) & ~3) + (AW_NT / 64) * 2 * pitch) * 4; }

// ---- projection: xlin = x lin^T and s_i / s_j on the fp32 matrix cores ---------------------------------------------
// gdn_long_project_kernel with D -> DP and lin^T columns >= d zero: A operand (16x16x4) lane l = x[row l & 15][k
// l >> 4], B = lin^T[k l >> 4][col l & 15], C/D register r of lane l = xlin[row 4 (l >> 4) + r][col l & 15].  The
// result of a column is a k-ordered fmaf chain (exact fp32 products), the same for both addressings of x.
template <int DP, bool VEC>
__global__ __launch_bounds__(AW_NT) void gdn_any_project_kernel(
    const float* __restrict__ xb, long long bstride, long long sstride, const float* __restrict__ lin_w,
    const float* __restrict__ terms, int rows, int n, int w, int d, int ap, float* __restrict__ xlin,
    float* __restrict__ s_i, float* __restrict__ s_j) {
  constexpr int LP = DP + 16;
  constexpr int CB = DP / 16;
  constexpr int XU = AW_ROWS * AW_KC / AW_NT;
  constexpr int WU = DP * AW_KC / AW_NT;
  __shared__ float4 xs4[AW_ROWS * AW_XP / 4];
  __shared__ float ls[AW_KC * LP];
  __shared__ float as[2 * AW_KC];
  __shared__ long long roff[AW_ROWS];
  float* xs = reinterpret_cast<float*>(xs4);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i16 = lane & 15, q = lane >> 4;
  const int r0 = (int)blockIdx.x * AW_ROWS;
  for (int r = tid; r < AW_ROWS; r += AW_NT) {
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
        const int e = tid + u * AW_NT, r = e >> 3, k = k0 + 4 * (e & 7);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < w) v = *reinterpret_cast<const float4*>(xb + roff[r] + k);
        xv[4 * u] = v.x; xv[4 * u + 1] = v.y; xv[4 * u + 2] = v.z; xv[4 * u + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int e = tid + u * AW_NT, r = e >> 5, k = k0 + (e & 31);
        xv[u] = k < w ? xb[roff[r] + k] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < WU; ++u) {
      const int e = tid + u * AW_NT, col = e >> 5, k = k0 + (e & 31);
      lv[u] = (k < w && col < d) ? lin_w[(size_t)col * w + k] : 0.f;
    }
    if (tid < 2 * AW_KC) {
      const int k = k0 + (tid & 31);
      avv = k < w ? terms[(tid >> 5) * ap + k] : 0.f;
    }
  };
  auto store = [&]() {
    if constexpr (VEC) {
#pragma unroll
      for (int u = 0; u < XU / 4; ++u) {
        const int e = tid + u * AW_NT, r = e >> 3, c = 4 * (e & 7);
        xs4[(r * AW_XP + c) / 4] = make_float4(xv[4 * u], xv[4 * u + 1], xv[4 * u + 2], xv[4 * u + 3]);
      }
    } else {
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int e = tid + u * AW_NT;
        xs[(e >> 5) * AW_XP + (e & 31)] = xv[u];
      }
    }
#pragma unroll
    for (int u = 0; u < WU; ++u) {
      const int e = tid + u * AW_NT;
      ls[(e & 31) * LP + (e >> 5)] = lv[u];
    }
    if (tid < 2 * AW_KC) as[tid] = avv;
  };

  aw_f32x4 acc[2][CB];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[rb][cb] = aw_f32x4{0.f, 0.f, 0.f, 0.f};
  float pi[2] = {0.f, 0.f}, pj[2] = {0.f, 0.f};
  const int nch = (w + AW_KC - 1) / AW_KC;
  const int cbn = (d + 15) >> 4;                      // column blocks that hold a column < d (wave-uniform)
  load(0);
  for (int ch = 0; ch < nch; ++ch) {
    __syncthreads();
    store();
    __syncthreads();
    if (ch + 1 < nch) load((ch + 1) * AW_KC);
#pragma unroll
    for (int kk = 0; kk < AW_KC / 4; ++kk) {
      const int k = 4 * kk + q;
      float a[2];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) a[rb] = xs[(wv * 32 + rb * 16 + i16) * AW_XP + k];
      const float ai = as[k], aj = as[AW_KC + k];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        pi[rb] = fmaf(a[rb], ai, pi[rb]);
        pj[rb] = fmaf(a[rb], aj, pj[rb]);
      }
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        if (cb < cbn) {                               // blocks wholly beyond d: no matrix-core work
          const float bv = ls[k * LP + cb * 16 + i16];
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
            acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb], bv, acc[rb][cb], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int rbase = r0 + wv * 32 + rb * 16;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int col = cb * 16 + i16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rbase + 4 * q + r;
        if (row < rows && col < d) xlin[(size_t)row * d + col] = acc[rb][cb][r];
      }
    }
    float si = pi[rb], sj = pj[rb];
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

// ---- gather-aggregate forward (gdn_large_aggregate_kernel at run-time d) --------------------------------------------
template <int DP, int V>
__global__ __launch_bounds__(AW_NT) void gdn_any_aggregate_kernel(
    const float* __restrict__ xlin, const float* __restrict__ s_i, const float* __restrict__ s_j,
    const uint16_t* __restrict__ nbr, const float* __restrict__ bias, int batch, int n, int d, int pitch,
    int tblocks, float* __restrict__ z, float* __restrict__ alpha) {
  constexpr int LPR = AWG<DP>::LPR, NG = AWG<DP>::NG;
  extern __shared__ float4 smem_aw4[];
  float* smem = reinterpret_cast<float*>(smem_aw4);
  int b, t0;
  if (!aw_place(tblocks, batch, b, t0)) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int npad = (n + 3) & ~3;
  float* sj = smem;
  float* wl = smem + npad + wave * 2 * pitch;
  int* jl = reinterpret_cast<int*>(wl + pitch);
  const size_t row0 = (size_t)b * n;
  for (int t = tid; t < n; t += AW_NT) sj[t] = s_j[row0 + t];
  __syncthreads();
  const int g = lane / LPR, c0 = (lane % LPR) * 4;
  const float4 bv = aw_load<V>(bias, c0, d);
  const float* xw = xlin + row0 * d;
  const int t1 = min(n, t0 + AW_TPB);
  for (int i = t0 + wave; i < t1; i += AW_NT / 64) {
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
    m = aw_wave_max(m);
    float sum = 0.f;
    for (int p = lane; p < pitch; p += 64) {
      const float ex = __expf(wl[p] - m);
      wl[p] = ex;
      sum += ex;
    }
    sum = wave_sum(sum);
    const float inv = __builtin_amdgcn_rcpf(sum + GDN_SOFTMAX_EPS);
    float* arow = alpha ? alpha + (row0 + i) * pitch : nullptr;
    for (int p = lane; p < pitch; p += 64) {
      const float a = wl[p] * inv;
      wl[p] = a;
      if (arow) arow[p] = a;       // rank order: slot p of the list
    }
    __builtin_amdgcn_wave_barrier();
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int p = g; p < pitch; p += NG) {
      const int j = jl[p];
      if (j < n) aw_fma4(wl[p], aw_load<V>(xw + (size_t)j * d, c0, d), acc);
    }
    aw_group_sum<DP>(acc);
    if (g == 0) {
      acc.x += bv.x; acc.y += bv.y; acc.z += bv.z; acc.w += bv.w;
      aw_store<V>(z + (row0 + i) * d, c0, d, acc);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- backward pass 1, per target: d_alpha, the softmax / LeakyReLU chain -> d_pi table, d_s_i -------------------
template <int DP, int V>
__global__ __launch_bounds__(AW_NT) void gdn_any_bwd_target_kernel(
    const float* __restrict__ d_z, const float* __restrict__ xlin, const float* __restrict__ alpha,
    const float* __restrict__ s_i, const float* __restrict__ s_j, const uint16_t* __restrict__ nbr, int batch,
    int n, int d, int pitch, int tblocks, float* __restrict__ d_si, float* __restrict__ dpi_ws) {
  constexpr int LPR = AWG<DP>::LPR, NG = AWG<DP>::NG;
  extern __shared__ float4 smem_aw4[];
  float* smem = reinterpret_cast<float*>(smem_aw4);
  int b, t0;
  if (!aw_place(tblocks, batch, b, t0)) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int npad = (n + 3) & ~3;
  float* sj = smem;
  float* da = smem + npad + wave * 2 * pitch;
  int* jl = reinterpret_cast<int*>(da + pitch);
  const size_t row0 = (size_t)b * n;
  for (int t = tid; t < n; t += AW_NT) sj[t] = s_j[row0 + t];
  __syncthreads();
  const int g = lane / LPR, c0 = (lane % LPR) * 4;
  const float* xw = xlin + row0 * d;
  const int t1 = min(n, t0 + AW_TPB);
  for (int i = t0 + wave; i < t1; i += AW_NT / 64) {
    const size_t ri = row0 + i;
    const float4 gz = aw_load<V>(d_z + ri * d, c0, d);
    const uint16_t* lst = nbr + (size_t)i * pitch;
    for (int p = g; p < pitch; p += NG) {       // pitch is a multiple of 16: the same trip count for every group
      const int j = lst[p];
      float part = 0.f;
      if (j < n) {
        const float4 x = aw_load<V>(xw + (size_t)j * d, c0, d);
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

// ---- backward pass 2, per source j over the reverse lists: d_xlin[j], d_s_j[j] --------------------------------------
template <int DP, int V>
__global__ __launch_bounds__(AW_NT) void gdn_any_bwd_source_kernel(
    const float* __restrict__ d_z, const float* __restrict__ alpha, const float* __restrict__ dpi_ws,
    const uint32_t* __restrict__ rent, const int32_t* __restrict__ rlen, int batch, int n, int d, int pitch,
    int rpitch, int tblocks, float* __restrict__ d_xlin, float* __restrict__ d_sj) {
  constexpr int LPR = AWG<DP>::LPR, NG = AWG<DP>::NG;
  int b, t0;
  if (!aw_place(tblocks, batch, b, t0)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / LPR, c0 = (lane % LPR) * 4;
  const size_t row0 = (size_t)b * n;
  const int t1 = min(n, t0 + AW_TPB);
  for (int j = t0 + wave; j < t1; j += AW_NT / 64) {
    const int cnt = rlen[j];
    const uint32_t* ents = rent + (size_t)j * rpitch;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float dsj = 0.f;
#pragma unroll 4
    for (int r = g; r < cnt; r += NG) {
      const uint32_t ent = ents[r];
      const size_t ti = row0 + (ent >> 16), p = ent & 0xffffu;
      aw_fma4(alpha[ti * pitch + p], aw_load<V>(d_z + ti * d, c0, d), acc);
      if (lane % LPR == 0) dsj += dpi_ws[ti * pitch + p];
    }
    aw_group_sum<DP>(acc);
    dsj = wave_sum(dsj);
    if (g == 0) aw_store<V>(d_xlin + (row0 + j) * d, c0, d, acc);
    if (lane == 0) d_sj[row0 + j] = dsj;
  }
}

// ---- d_bias = column sums of d_z: a fixed row range per workgroup, then gdn_colsum_ticket ----------------------------
template <int DP, int V>
__global__ __launch_bounds__(AW_NT) void gdn_any_bias_kernel(const float* __restrict__ d_z, int rows, int d,
                                                             float* __restrict__ d_bias, float* __restrict__ bias_ws) {
  constexpr int LPR = AWG<DP>::LPR, RG = AW_NT / LPR;
  __shared__ float4 part4[RG * DP / 4];
  __shared__ float row[DP];
  __shared__ float scratch[AW_NT];
  const int tid = threadIdx.x, rg = tid / LPR, c0 = (tid % LPR) * 4;
  const int per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
  const int r0 = (int)blockIdx.x * per, r1 = min(rows, r0 + per);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r = r0 + rg; r < r1; r += RG) {
    const float4 v = aw_load<V>(d_z + (size_t)r * d, c0, d);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  part4[rg * (DP / 4) + c0 / 4] = acc;
  __syncthreads();
  const float* part = reinterpret_cast<const float*>(part4);
  if (tid < d) {
    float s = 0.f;
    for (int q = 0; q < RG; ++q) s += part[q * DP + tid];
    row[tid] = s;
  }
  __syncthreads();
  gdn_colsum_ticket(bias_ws, row, d, d_bias, scratch);
}

// ---- eval head: BN+ReLU, x embedding, BN+ReLU, Linear(d -> 1) (gdn_head_kernel at run-time d) ---------------------
// 16 lanes per row, CPL = DP / 16 consecutive columns per lane; columns >= d contribute nothing.
template <int DP>
__global__ __launch_bounds__(256) void gdn_any_head_kernel(const float* __restrict__ z, const float* __restrict__ emb,
                                                           const float* __restrict__ bn1, const float* __restrict__ bn2,
                                                           const float* __restrict__ out_w,
                                                           const float* __restrict__ out_b, int rows, int n, int d,
                                                           float* __restrict__ out, float* __restrict__ h2) {
  constexpr int CPL = DP / 16;
  const int l16 = threadIdx.x & 15;
  const int d0 = l16 * CPL;
  float sc1[CPL], sh1[CPL], sc2[CPL], sh2[CPL], wo[CPL];
#pragma unroll
  for (int v = 0; v < CPL; ++v) {
    const bool in = d0 + v < d;
    sc1[v] = in ? bn1[d0 + v] : 0.f; sh1[v] = in ? bn1[d + d0 + v] : 0.f;
    sc2[v] = in ? bn2[d0 + v] : 0.f; sh2[v] = in ? bn2[d + d0 + v] : 0.f;
    wo[v] = in ? out_w[d0 + v] : 0.f;
  }
  const float ob = out_b[0];
  const int rpb = blockDim.x >> 4;
  constexpr int U = 4;
  for (int row0 = (blockIdx.x * rpb + (threadIdx.x >> 4)) * U; row0 < rows; row0 += gridDim.x * rpb * U) {
    float zv[U][CPL], ev[U][CPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = min(row0 + u, rows - 1);
      const int s = row % n;
#pragma unroll
      for (int v = 0; v < CPL; ++v) {
        const bool in = d0 + v < d;
        zv[u][v] = in ? z[(size_t)row * d + d0 + v] : 0.f;
        ev[u][v] = in ? emb[(size_t)s * d + d0 + v] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = row0 + u;
      float part = 0.f;
#pragma unroll
      for (int v = 0; v < CPL; ++v) {
        float h = fmaxf(fmaf(zv[u][v], sc1[v], sh1[v]), 0.f);
        h *= ev[u][v];
        h = fmaxf(fmaf(h, sc2[v], sh2[v]), 0.f);
        if (h2 && row < rows && d0 + v < d) h2[(size_t)row * d + d0 + v] = h;
        part = fmaf(h, wo[v], part);
      }
      part = row16_sum(part);
      if (l16 == 0 && row < rows) out[row] = part + ob;
    }
  }
}

// ---- projection backward: partial [d + 2, w] blocks of G^T X per row range (gdn_long_project_bwd_kernel, run-time d)
template <int DP>
__global__ __launch_bounds__(256) void gdn_any_project_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ d_xlin, const float* __restrict__ d_si,
    const float* __restrict__ d_sj, int rows, int w, int d, int per, float* __restrict__ part) {
  constexpr int NO = (DP + 2 + 3) / 4;
  __shared__ float gs[AW_RC * (DP + 2)];
  __shared__ float xs[AW_RC * 64];
  const int O = d + 2;
  const int tid = threadIdx.x, col = tid & 63, g = tid >> 6;
  const int p = blockIdx.x, k0 = blockIdx.y * 64;
  const int ra = p * per, rb = min(rows, ra + per);
  float acc[NO];
#pragma unroll
  for (int j = 0; j < NO; ++j) acc[j] = 0.f;
  for (int c0 = ra; c0 < rb; c0 += AW_RC) {
    const int cnt = min(AW_RC, rb - c0);
    __syncthreads();
    for (int t = tid; t < cnt * O; t += 256) {
      const int r = t / O, o = t - r * O;
      const size_t row = (size_t)c0 + r;
      gs[t] = o < d ? d_xlin[row * d + o] : (o == d ? d_si[row] : d_sj[row]);
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

static int aw_parts(int rows) { return min(AW_PARTS, (rows + AW_RC - 1) / AW_RC); }

// float4 / float2 / scalar row segments: every pointer must be aligned to the segment
static int aw_vec(int d, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  if (d % 4 == 0 && (bits & 15) == 0) return 4;
  if (d % 2 == 0 && (bits & 7) == 0) return 2;
  return 1;
}

}  // namespace

bool gdn_any_width(int d) { return d >= 1 && d <= GDN_ANY_MAX_D && d != 16 && d != 32 && d != 64 && d != 128; }

// padded width DP of the kernels above
static int aw_dp(int d) { return d <= 16 ? 16 : d <= 32 ? 32 : d <= 64 ? 64 : d <= 128 ? 128 : 256; }

#define GDN_AW_DP_SWITCH(DPV, BODY) \
  switch (DPV) {                    \
    case 16: { constexpr int DP = 16; BODY; } break;   \
    case 32: { constexpr int DP = 32; BODY; } break;   \
    case 64: { constexpr int DP = 64; BODY; } break;   \
    case 128: { constexpr int DP = 128; BODY; } break;  \
    default: { constexpr int DP = 256; BODY; } break;   \
  }
#define GDN_AW_V_SWITCH(VV, BODY) \
  switch (VV) {                   \
    case 4: { constexpr int V = 4; BODY; } break;  \
    case 2: { constexpr int V = 2; BODY; } break;  \
    default: { constexpr int V = 1; BODY; } break; \
  }

int gdn_any_project(const float* xb, long long bstride, long long sstride, const float* lin_w, const float* terms,
                    int batch, int n, int w, int d, float* xlin, float* s_i, float* s_j, hipStream_t st) {
  if (batch <= 0 || n <= 0 || w <= 0) return GDN_ERR_ARG;
  if (!gdn_any_width(d) || n > 4096 || w > GDN_LONG_MAX_W) return GDN_ERR_UNSUPPORTED;
  const long long rows_ll = (long long)batch * n;
  if (rows_ll > 0x7fffffffLL) return GDN_ERR_UNSUPPORTED;
  const int rows = (int)rows_ll, ap = gdn_terms_pitch(w);
  const int grid = (rows + AW_ROWS - 1) / AW_ROWS;
  const bool vec = (w % 4) == 0 && (bstride % 4) == 0 && (sstride % 4) == 0 && ((uintptr_t)xb & 15) == 0;
  GDN_AW_DP_SWITCH(aw_dp(d), {
    if (vec)
      hipLaunchKernelGGL((gdn_any_project_kernel<DP, true>), dim3(grid), dim3(AW_NT), 0, st, xb, bstride, sstride,
                         lin_w, terms, rows, n, w, d, ap, xlin, s_i, s_j);
    else
      hipLaunchKernelGGL((gdn_any_project_kernel<DP, false>), dim3(grid), dim3(AW_NT), 0, st, xb, bstride, sstride,
                         lin_w, terms, rows, n, w, d, ap, xlin, s_i, s_j);
  })
  return gdn_launch_status();
}

int gdn_any_aggregate(const float* xlin, const float* s_i, const float* s_j, const uint16_t* nbr, const float* bias,
                      int batch, int n, int d, int k, float* z, float* alpha, hipStream_t st) {
  if (batch <= 0 || n <= 0 || k <= 0) return GDN_ERR_ARG;
  if (!gdn_any_width(d) || n > 4096 || k > n || k + 1 > 1024) return GDN_ERR_UNSUPPORTED;
  const int pitch = gdn_nbr_pitch(k), tblocks = (n + AW_TPB - 1) / AW_TPB;
  const int lds = aw_lds(n, pitch), grid = aw_grid(batch, n);
  const int vv = aw_vec(d, {xlin, bias, z});
  GDN_AW_DP_SWITCH(aw_dp(d), GDN_AW_V_SWITCH(vv, {
    hipLaunchKernelGGL((gdn_any_aggregate_kernel<DP, V>), dim3(grid), dim3(AW_NT), lds, st, xlin, s_i, s_j, nbr,
                       bias, batch, n, d, pitch, tblocks, z, alpha);
  }))
  return gdn_launch_status();
}

// workspace as gdn_attn_aggregate_bwd's: [d_bias ticket + rows (bias_ws_floats)][batch*n*pitch d_pi]
int gdn_any_attn_bwd(const float* d_z, const float* xlin, const float* alpha, const float* s_i, const float* s_j,
                     const uint16_t* nbr, const uint32_t* rent, const int32_t* rlen, int batch, int n, int d, int k,
                     float* d_xlin, float* d_si, float* d_sj, float* d_bias, float* workspace,
                     long long bias_ws_floats, hipStream_t st) {
  if (batch <= 0 || n <= 0 || k <= 0 || !rent || !rlen) return GDN_ERR_ARG;
  if (!gdn_any_width(d) || n > 4096 || k > n || k + 1 > 1024) return GDN_ERR_UNSUPPORTED;
  const int pitch = gdn_nbr_pitch(k), rpitch = (n + 15) & ~15, tblocks = (n + AW_TPB - 1) / AW_TPB;
  const int lds = aw_lds(n, pitch), grid = aw_grid(batch, n);
  const int rows = batch * n;
  const int bgrid = min(GDN_COLSUM_MAX_ROWS, (rows + 255) / 256);
  float* dpi_ws = workspace + bias_ws_floats;
  const int vv = aw_vec(d, {d_z, xlin, d_xlin});
  GDN_AW_DP_SWITCH(aw_dp(d), GDN_AW_V_SWITCH(vv, {
    hipLaunchKernelGGL((gdn_any_bwd_target_kernel<DP, V>), dim3(grid), dim3(AW_NT), lds, st, d_z, xlin, alpha, s_i,
                       s_j, nbr, batch, n, d, pitch, tblocks, d_si, dpi_ws);
    hipLaunchKernelGGL((gdn_any_bwd_source_kernel<DP, V>), dim3(grid), dim3(AW_NT), 0, st, d_z, alpha, dpi_ws, rent,
                       rlen, batch, n, d, pitch, rpitch, tblocks, d_xlin, d_sj);
    hipLaunchKernelGGL((gdn_any_bias_kernel<DP, V>), dim3(bgrid), dim3(AW_NT), 0, st, d_z, rows, d, d_bias, workspace);
  }))
  return gdn_launch_status();
}

int gdn_any_head(const float* z, const float* emb, const float* bn1_affine, const float* bn2_affine,
                 const float* out_w, const float* out_b, int batch, int n, int d, float* out, float* h2,
                 hipStream_t st) {
  if (!z || !emb || !bn1_affine || !bn2_affine || !out_w || !out_b || !out || batch <= 0 || n <= 0)
    return GDN_ERR_ARG;
  if (!gdn_any_width(d)) return GDN_ERR_UNSUPPORTED;
  const int rows = batch * n;
  const int grid = min((rows + 63) / 64, gdn_cu_count() * 8);
  GDN_AW_DP_SWITCH(aw_dp(d), {
    hipLaunchKernelGGL((gdn_any_head_kernel<DP>), dim3(grid), dim3(256), 0, st, z, emb, bn1_affine, bn2_affine, out_w,
                       out_b, rows, n, d, out, h2);
  })
  return gdn_launch_status();
}

long long gdn_any_project_bwd_workspace_bytes(int n, int w, int d) {
  if (!gdn_any_width(d) || n > 4096 || w > GDN_LONG_MAX_W) return 0;
  return (long long)AW_PARTS * (d + 2) * w * (long long)sizeof(float);
}

int gdn_any_project_bwd_partials(const float* x, const float* d_xlin, const float* d_si, const float* d_sj, int batch,
                                 int n, int w, int d, float* workspace, int* parts_out, hipStream_t st) {
  if (!gdn_any_width(d) || n > 4096 || w > GDN_LONG_MAX_W) return GDN_ERR_UNSUPPORTED;
  const long long rows_ll = (long long)batch * n;
  if (rows_ll > 0x7fffffffLL) return GDN_ERR_UNSUPPORTED;
  const int rows = (int)rows_ll, parts = aw_parts(rows), per = (rows + parts - 1) / parts;
  const dim3 grid(parts, (w + 63) / 64);
  GDN_AW_DP_SWITCH(aw_dp(d), {
    hipLaunchKernelGGL((gdn_any_project_bwd_kernel<DP>), grid, dim3(256), 0, st, x, d_xlin, d_si, d_sj, rows, w, d,
                       per, workspace);
  })
  *parts_out = parts;
  return gdn_launch_status();
}

