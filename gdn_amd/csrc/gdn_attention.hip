// Attention from raw data: the attention weights of the graph layer (models/graph_layer.py:91-110) without the
// projection.  The logit is separable (include/gdn_hip.h "per-forward constants"): pi(i<-j) = LeakyReLU(s_i + s_j)
// with s = x_row . a + c[sensor], and a / c are folded into node_terms — so attention needs the raw window, the
// node terms and the neighbour lists only, at every n, w, k of the envelope and for any embedding width or head.
// fp32 VALU throughout (no 16-bit operands: fp32's own range, no guard).
//   gdn_attention_at    one attention row per (window, sensor) pair;
//   gdn_attention_mean  the weighted mean of the attention rows over a run of windows.
// Both addressings of x (the raw series [n, t_raw] / materialised windows [batch, n, w]) go through ONE row
// pointer and one dot-product routine: the same bits from either.
#include "gdn_common.hpp"

#include <algorithm>

namespace {

constexpr int ATT_NT = 512;                 // threads of a gdn_attention_mean workgroup
constexpr int ATT_MAX_RUN = 64;             // windows a workgroup stages at once
constexpr int ATT_LDS_BUDGET = 128 * 1024;  // bytes of s_i / s_j per workgroup
constexpr int ATT_MAX_PARTS = 512;          // workgroups = partial blocks of a launch
constexpr long long ATT_PART_BUDGET = 64ll << 20;   // bytes of partial blocks in the workspace
constexpr int ATT_UNROLL = 4;               // windows in flight per softmax step (independent chains)

// x rows: row(b, i) = x + b * win_stride + i * row_stride  (series: 1 / t_raw, from column `first`; windows: n*w / w)
struct AttRows {
  const float* x;
  long long win_stride, row_stride;
};

// the two attention scalars of one row, without the per-sensor constants: a serial fmaf chain in tick order
__device__ __forceinline__ void att_dots(const float* __restrict__ row, const float* __restrict__ a_i,
                                         const float* __restrict__ a_j, int w, float* u, float* v) {
  float su = 0.f, sv = 0.f;
  for (int t = 0; t < w; ++t) {
    const float xv = row[t];
    su = fmaf(xv, a_i[t], su);
    sv = fmaf(xv, a_j[t], sv);
  }
  *u = su;
  *v = sv;
}

// max / sum over the L lanes (16, 32 or 64, aligned) that share a target
template <int L>
__device__ __forceinline__ float seg_max(float v) {
  v = row16_max(v);
  if (L >= 32) v = fmaxf(v, __shfl_xor(v, 16));
  if (L >= 64) v = fmaxf(v, __shfl_xor(v, 32));
  return v;
}
template <int L>
__device__ __forceinline__ float seg_sum(float v) {
  v = row16_sum(v);
  if (L >= 32) v += __shfl_xor(v, 16);
  if (L >= 64) v += __shfl_xor(v, 32);
  return v;
}

struct MeanPlan {
  int run;        // windows staged per step
  int ns;         // row stride of the s tables (odd: lanes along the windows hit distinct banks)
  int parts;      // workgroups
  int runs_per;   // steps per workgroup
};

MeanPlan mean_plan(int batch, int n, int k) {
  MeanPlan p;
  p.ns = n | 1;
  p.run = std::min(ATT_MAX_RUN, std::max(1, ATT_LDS_BUDGET / (8 * p.ns)));
  const long long runs = ((long long)batch + p.run - 1) / p.run;
  const long long block = (long long)n * gdn_nbr_pitch(k) * 8;
  long long parts = std::min(runs, (long long)ATT_MAX_PARTS);
  parts = std::min(parts, std::max(1ll, ATT_PART_BUDGET / block));
  p.runs_per = (int)((runs + parts - 1) / parts);
  p.parts = (int)((runs + p.runs_per - 1) / p.runs_per);
  return p;
}

// Workgroup g owns windows [g * runs_per * run, ...) and one partial block part[g][n][pitch] (float64).  Per step:
//   phase S  s_i / s_j of (window, sensor) for `run` windows into LDS, one pair per thread;
//   phase A  L lanes per target (a slot each, NS slots per lane beyond 64): softmax over the target's valid slots
//            per window, weight * alpha summed over the step's windows in float64 registers, then added to the
//            workgroup's own partial block (the same lane owns a cell in every step: plain loads and stores).
// No atomics: gdn_attention_reduce_kernel adds the blocks in block order.
template <int L, int NS>
__global__ __launch_bounds__(ATT_NT) void gdn_attention_mean_kernel(
    const AttRows rows, const float* __restrict__ weights, const float* __restrict__ terms, int tp,
    const uint16_t* __restrict__ nbr, const int32_t* __restrict__ deg, int batch, int n, int w, int pitch,
    const MeanPlan pl, int lanes_along_windows, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float att_lds[];
  float* sI = att_lds;
  float* sJ = att_lds + (size_t)pl.run * pl.ns;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* a_i = terms;
  const float* a_j = terms + tp;
  const float* c_i = terms + 2 * tp;
  const float* c_j = c_i + n;
  double* mine = part + (size_t)blockIdx.x * n * pitch;
  constexpr int TPW = 64 / L;                       // targets per wave
  const int sub = lane % L, tslot = lane / L;
  const int groups = (n + TPW - 1) / TPW;
  for (int r = 0; r < pl.runs_per; ++r) {
    const long long b0 = ((long long)blockIdx.x * pl.runs_per + r) * pl.run;
    const int cnt = (int)min((long long)pl.run, (long long)batch - b0);     // <= 0: nothing left for this step
    __syncthreads();                                // the previous step's readers are done with the tables
    for (int p = tid; p < cnt * n; p += ATT_NT) {
      int b, i;
      if (lanes_along_windows) { b = p % cnt; i = p / cnt; }
      else { i = p % n; b = p / n; }
      float u, v;
      att_dots(rows.x + (b0 + b) * rows.win_stride + (long long)i * rows.row_stride, a_i, a_j, w, &u, &v);
      sI[b * pl.ns + i] = u + c_i[i];
      sJ[b * pl.ns + i] = v + c_j[i];
    }
    __syncthreads();
    for (int g = wv; g < groups; g += ATT_NT / 64) {
      const int i = g * TPW + tslot;
      const bool live = i < n;
      const int dg = live ? deg[i] : 0;
      int src[NS];
      bool valid[NS];
      double acc[NS];
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        const int p = sub + q * L;
        valid[q] = p < dg;
        src[q] = valid[q] ? (int)nbr[(size_t)i * pitch + p] : 0;
        acc[q] = 0.0;
      }
      const int ii = live ? i : 0;
      for (int bb = 0; bb < cnt; bb += ATT_UNROLL) {
        float e[ATT_UNROLL][NS], mx[ATT_UNROLL], sm[ATT_UNROLL], wt[ATT_UNROLL];
#pragma unroll
        for (int c = 0; c < ATT_UNROLL; ++c) {
          const int b = min(bb + c, cnt - 1);
          wt[c] = bb + c < cnt ? (weights ? weights[b0 + b] : 1.f) : 0.f;
          const float si = sI[b * pl.ns + ii];
          mx[c] = -INFINITY;
#pragma unroll
          for (int q = 0; q < NS; ++q) {
            e[c][q] = valid[q] ? leaky(si + sJ[b * pl.ns + src[q]]) : -INFINITY;
            mx[c] = fmaxf(mx[c], e[c][q]);
          }
        }
#pragma unroll
        for (int c = 0; c < ATT_UNROLL; ++c) mx[c] = seg_max<L>(mx[c]);
#pragma unroll
        for (int c = 0; c < ATT_UNROLL; ++c) {
          sm[c] = 0.f;
#pragma unroll
          for (int q = 0; q < NS; ++q) {
            e[c][q] = valid[q] ? __expf(e[c][q] - mx[c]) : 0.f;
            sm[c] += e[c][q];
          }
        }
#pragma unroll
        for (int c = 0; c < ATT_UNROLL; ++c) sm[c] = seg_sum<L>(sm[c]);
#pragma unroll
        for (int c = 0; c < ATT_UNROLL; ++c) {       // windows in order: a fixed summation order
          const float inv = 1.f / (sm[c] + GDN_SOFTMAX_EPS);
#pragma unroll
          for (int q = 0; q < NS; ++q) acc[q] += (double)(wt[c] * (e[c][q] * inv));
        }
      }
      if (live) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          const int p = sub + q * L;
          if (p < pitch) {
            double* cell = mine + (size_t)i * pitch + p;
            *cell = r == 0 ? acc[q] : *cell + acc[q];
          }
        }
      }
    }
  }
}

// mean[c] = sum over the partial blocks (in block order) / sum of the weights (in a fixed order); zeros when the
// weight sum is not positive
__global__ __launch_bounds__(256) void gdn_attention_reduce_kernel(const double* __restrict__ part, int parts,
                                                                   long long cells, const float* __restrict__ weights,
                                                                   int batch, float* __restrict__ mean) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double wsum = (double)batch;
  if (weights) {
    double s = 0.0;
    for (int b = tid; b < batch; b += 256) s += (double)weights[b];
    red[tid] = s;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    wsum = red[0];
  }
  const long long c = (long long)blockIdx.x * 256 + tid;
  if (c >= cells) return;
  double s = 0.0;
  for (int g = 0; g < parts; ++g) s += part[(size_t)g * cells + c];
  mean[c] = wsum > 0.0 ? (float)(s / wsum) : 0.f;
}

// One 64-thread workgroup per (window, sensor) pair: s_i of the target, s_j of its sources (a slot per lane, strided),
// softmax over the valid slots.  A pair outside the data (window < 0, past the series, sensor outside [0, n)) gets a
// row of zeros: nothing is read for it.
__global__ __launch_bounds__(64) void gdn_attention_at_kernel(
    const float* __restrict__ x, long long t_raw, const int64_t* __restrict__ windows,
    const int32_t* __restrict__ sensors, const float* __restrict__ terms, int tp, const uint16_t* __restrict__ nbr,
    const int32_t* __restrict__ deg, int n, int w, int pitch, float* __restrict__ alpha) {
  __shared__ float lg[1024];
  const int lane = threadIdx.x;
  const long long b = windows[blockIdx.x];
  const int i = sensors[blockIdx.x];
  float* out = alpha + (size_t)blockIdx.x * pitch;
  const bool inside = i >= 0 && i < n && b >= 0 && (t_raw == 0 || b + w <= t_raw);
  if (!inside) {
    for (int p = lane; p < pitch; p += 64) out[p] = 0.f;
    return;
  }
  const long long win_stride = t_raw > 0 ? 1 : (long long)n * w, row_stride = t_raw > 0 ? t_raw : w;
  const float* base = x + b * win_stride;
  const float* a_i = terms;
  const float* a_j = terms + tp;
  const float* c_i = terms + 2 * tp;
  const float* c_j = c_i + n;
  const int dg = deg[i];
  float u, v;
  att_dots(base + (long long)i * row_stride, a_i, a_j, w, &u, &v);
  const float si = u + c_i[i];
  float mx = -INFINITY;
  for (int p = lane; p < dg; p += 64) {
    const int j = nbr[(size_t)i * pitch + p];
    att_dots(base + (long long)j * row_stride, a_i, a_j, w, &u, &v);
    const float l = leaky(si + (v + c_j[j]));
    lg[p] = l;
    mx = fmaxf(mx, l);
  }
  mx = seg_max<64>(mx);
  float sm = 0.f;
  for (int p = lane; p < dg; p += 64) {
    const float e = __expf(lg[p] - mx);
    lg[p] = e;
    sm += e;
  }
  sm = seg_sum<64>(sm);
  const float inv = 1.f / (sm + GDN_SOFTMAX_EPS);
  for (int p = lane; p < pitch; p += 64) out[p] = p < dg ? lg[p] * inv : 0.f;
}

bool att_shape_ok(int n, int w, int k) {
  return w >= 1 && w <= GDN_LONG_MAX_W && k >= 1 && k <= n && n <= 4096 && k + 1 <= 1024;
}

template <int L, int NS>
int launch_mean(const AttRows& rows, const float* weights, const float* terms, int tp, const uint16_t* nbr,
                const int32_t* deg, int batch, int n, int w, int pitch, const MeanPlan& pl, int along,
                double* part, hipStream_t st) {
  const int lds = 2 * pl.run * pl.ns * (int)sizeof(float);
  (void)gdn_blocks_per_cu((const void*)gdn_attention_mean_kernel<L, NS>, ATT_NT, lds);   // raises the LDS limit
  hipLaunchKernelGGL((gdn_attention_mean_kernel<L, NS>), dim3(pl.parts), dim3(ATT_NT), lds, st, rows, weights, terms,
                     tp, nbr, deg, batch, n, w, pitch, pl, along, part);
  return gdn_launch_status();
}

}  // namespace

extern "C" long long gdn_attention_workspace_bytes(int batch, int n, int w, int k) {
  if (batch <= 0 || n <= 0 || !att_shape_ok(n, w, k)) return 0;
  const MeanPlan pl = mean_plan(batch, n, k);
  return (long long)pl.parts * n * gdn_nbr_pitch(k) * 8;
}

extern "C" int gdn_attention_mean(const float* x, long long t_raw, long long first, const float* weights,
                                  const float* node_terms, const uint16_t* nbr, const int32_t* deg, int batch, int n,
                                  int w, int k, void* workspace, float* mean, void* stream) {
  if (!x || !node_terms || !nbr || !deg || !workspace || !mean || batch <= 0 || n <= 0 || t_raw < 0 || first < 0)
    return GDN_ERR_ARG;
  if (!att_shape_ok(n, w, k)) return GDN_ERR_UNSUPPORTED;
  if (t_raw == 0 && first != 0) return GDN_ERR_ARG;
  if (t_raw > 0 && first + batch + w - 1 > t_raw) return GDN_ERR_ARG;     // the last window must fit
  const int pitch = gdn_nbr_pitch(k), tp = gdn_terms_pitch(w);
  const MeanPlan pl = mean_plan(batch, n, k);
  AttRows rows;
  rows.x = t_raw > 0 ? x + first : x;
  rows.win_stride = t_raw > 0 ? 1 : (long long)n * w;
  rows.row_stride = t_raw > 0 ? t_raw : w;
  const int along = t_raw > 0 ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(workspace);
  int rc;
#define GDN_ATT(LL, NN) \
  rc = launch_mean<LL, NN>(rows, weights, node_terms, tp, nbr, deg, batch, n, w, pitch, pl, along, part, st)
  if (pitch <= 16) GDN_ATT(16, 1);
  else if (pitch <= 32) GDN_ATT(32, 1);
  else if (pitch <= 64) GDN_ATT(64, 1);
  else if (pitch <= 128) GDN_ATT(64, 2);
  else if (pitch <= 256) GDN_ATT(64, 4);
  else if (pitch <= 512) GDN_ATT(64, 8);
  else GDN_ATT(64, 16);
#undef GDN_ATT
  if (rc != GDN_OK) return rc;
  const long long cells = (long long)n * pitch;
  hipLaunchKernelGGL(gdn_attention_reduce_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, part,
                     pl.parts, cells, weights, batch, mean);
  return gdn_launch_status();
}

extern "C" int gdn_attention_at(const float* x, long long t_raw, const int64_t* windows, const int32_t* sensors, int q,
                                const float* node_terms, const uint16_t* nbr, const int32_t* deg, int n, int w, int k,
                                float* alpha, void* stream) {
  if (!x || !windows || !sensors || !node_terms || !nbr || !deg || !alpha || q <= 0 || n <= 0 || t_raw < 0)
    return GDN_ERR_ARG;
  if (!att_shape_ok(n, w, k)) return GDN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gdn_attention_at_kernel, dim3(q), dim3(64), 0, (hipStream_t)stream, x, t_raw, windows, sensors,
                     node_terms, gdn_terms_pitch(w), nbr, deg, n, w, gdn_nbr_pitch(k), alpha);
  return gdn_launch_status();
}
