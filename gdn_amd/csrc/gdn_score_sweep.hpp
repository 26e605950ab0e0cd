// The scoring sweep "normalise, smooth over 4 ticks, reduce over sensors", ONE source for the three kernels that run
// it: score_smooth_max_kernel and score_smooth_topm_kernel (gdn_score.hip) and gdn_stream_score_kernel
// (gdn_stream.hip), plus the small pieces the key, ring and carry kernels share with them.  The kernels are compared
// bit for bit (top_scores[:, 0] is anomaly; a stream cut into any pushes writes the evaluator's bits; gaps with nothing
// missing writes the plain bits): every float64 expression that must agree stands here once and nowhere else.
//
// One wave owns a run of RUN consecutive ticks; lane l owns sensors s0 + l and s0 + 64 + l of a sweep and slides a
// 4-deep window of normalised errors down the run, so each (tick, sensor) value is computed once.  smoothed = mean of
// the value at the tick and its 3 predecessors (0 for the first 3 ticks of the SERIES).  What differs between the
// kernels is handed in:
//   the source   where pred / gt / valid of row t0 - 3 + u come from, and what the three predecessors of t0 are
//                (SeriesSource below: halo rows, zeros before the series; StreamSource in gdn_stream.hip:
//                the float64 carry).  The two predecessor rules are different rules, not cases of one.
//   the sink     what a tick does with the two smoothed scores of the lane (maximum, top-m merge, score table).
// GAPS: `valid` (1 = a real reading) travels as one bit per loaded row and the normalised error of a missing reading is
// 0.0 wherever it is used.  Without GAPS the validity rows are never asked for.
//
// numpy evaluates (x - m) * r and the 4-term sum as separate roundings: no FMA contraction in any unit that includes
// this header.
#pragma once
#pragma clang fp contract(off)
#include "gdn_common.hpp"

namespace gdn_sweep {

constexpr int RUN = 8;             // ticks per wave (short runs: thousands of waves keep loads in flight)
constexpr int TOPM_MAX = 8;
constexpr int NONE = 0x7fffffff;   // sensor of a masked / missing top-m candidate (score -inf)
// key of a slot that holds no reading (all ones: larger than every real key, the select never counts it)
constexpr unsigned long long FILLER = ~0ull;

// grid of a sweep launch over `ticks` ticks: four runs (waves) per workgroup, at most 8 workgroups per CU
inline int sweep_grid(int ticks) {
  const int runs = (ticks + RUN - 1) / RUN;
  return min((runs + 3) / 4, gdn_cu_count() * 8);
}

// the scoring key |pred - gt| in float64 (its bit pattern is the radix key of the select)
__device__ __forceinline__ double score_key(float p, float g) { return fabs((double)p - (double)g); }

__device__ __forceinline__ double filler_key() { return __longlong_as_double((long long)FILLER); }

// (x - median) / (|iqr| + eps), evaluate.py:60-62: the divisor is one number per sensor, so a wave divides ONCE per
// sensor and run and multiplies per tick (a float64 division is ~35 instructions; eleven per sensor and run were a
// third of the sweep).  x * (1/d) is within one ulp of x / d: 2e-16 relative, four orders below the 1e-12 bar of the
// scoring parity tests.
struct Scale {
  double med, inv_den;
};
__device__ __forceinline__ Scale sensor_scale(const double* __restrict__ med_iqr, int s) {
  return {med_iqr[2 * s], 1.0 / (fabs(med_iqr[2 * s + 1]) + 1e-2)};
}

// the normalised error of one reading; GAPS: 0.0 unless bit u of ok_bits says the reading is real
template <bool GAPS>
__device__ __forceinline__ double norm(float p, float g, double med, double inv_den, unsigned ok_bits, int u) {
  const double a = (score_key(p, g) - med) * inv_den;
  if constexpr (GAPS) return ((ok_bits >> u) & 1u) ? a : 0.0;
  return a;
}

// the two sensors of a lane in the sweep at s0: live flags, and indices clamped so that every load is unconditional
struct Lanes {
  int sa, sb, ca, cb;
  bool la, lb;
  __device__ __forceinline__ Lanes(int s0, int lane, int n)
      : sa(s0 + lane), sb(s0 + 64 + lane), ca(sa < n ? sa : n - 1), cb(sb < n ? sb : n - 1), la(sa < n), lb(sb < n) {}
};

// One sweep of one run: ticks [t0, t1) of sensors l.sa / l.sb; sink(u, tick, sma, smb) for every tick, in order.
// Source:  pred_row(tt) / gt_row(tt) / valid_row(tt)   row tt = t0 - 3 .. t0 + RUN - 1 (the source clamps)
//          before(t0, l, a, b, na, nb)                  a[k] / b[k] = normalised error 3 - k ticks before t0 of
//                                                      sensor l.ca / l.cb; na(k) / nb(k) = that of loaded row k
// first_tick: the series position of tick 0 (int or long long, as the kernel holds it).
template <bool GAPS, typename Source, typename Tick, typename Sink>
__device__ __forceinline__ void score_sweep(const Source& src, const double* __restrict__ med_iqr, const Lanes& l,
                                            int t0, int t1, Tick first_tick, Sink&& sink) {
  const Scale A = sensor_scale(med_iqr, l.ca), B = sensor_scale(med_iqr, l.cb);
  // ALL 4 x (3 + RUN) values of the run are fetched before the first is used (clamped row indices: the loads are
  // unconditional, rows that do not exist are masked afterwards) — fetched inside the tick loop they were a chain of
  // dependent round trips and the kernel ran at 2.2 TB/s
  float pa[RUN + 3], ga[RUN + 3], pb[RUN + 3], gb[RUN + 3];
  unsigned oka = 0u, okb = 0u;                   // GAPS: bit u = the reading of row u is real
#pragma unroll
  for (int u = 0; u < RUN + 3; ++u) {
    const int tt = t0 - 3 + u;
    const float* pp = src.pred_row(tt);
    const float* gg = src.gt_row(tt);
    pa[u] = pp[l.ca]; ga[u] = gg[l.ca]; pb[u] = pp[l.cb]; gb[u] = gg[l.cb];
    if constexpr (GAPS) {
      const unsigned char* vv = src.valid_row(tt);
      oka |= (vv[l.ca] ? 1u : 0u) << u;
      okb |= (vv[l.cb] ? 1u : 0u) << u;
    }
  }
  auto na = [&](int u) -> double { return norm<GAPS>(pa[u], ga[u], A.med, A.inv_den, oka, u); };
  auto nb = [&](int u) -> double { return norm<GAPS>(pb[u], gb[u], B.med, B.inv_den, okb, u); };
  double a[3], b[3];                             // three, two, one tick before t0
  src.before(t0, l, a, b, na, nb);
  double a3 = a[0], a2 = a[1], a1 = a[2], b3 = b[0], b2 = b[1], b1 = b[2];
#pragma unroll
  for (int u = 0; u < RUN; ++u) {
    const int tick = t0 + u;
    if (tick >= t1) continue;                    // (wave uniform)
    const double a0 = na(3 + u), b0 = nb(3 + u);
    double sma = 0.0, smb = 0.0;
    if (first_tick + tick >= 3) {                // numpy sums the 4 values left to right
      sma = (((a3 + a2) + a1) + a0) / 4.0;
      smb = (((b3 + b2) + b1) + b0) / 4.0;
    }
    a3 = a2; a2 = a1; a1 = a0;
    b3 = b2; b2 = b1; b1 = b0;
    sink(u, tick, sma, smb);
  }
}

// The source of a resident series (gdn_score.hip; per unit with first_tick = 0 in gdn_fleet_series.hip).
// Rows before this shard's first tick come from the halo [3][n] when the series has them (first_tick > 0); otherwise
// row 0 stands in (its values only feed ticks whose series index is < 3, which are forced to 0).  Rows past the shard
// are clamped to its last.  The 3 predecessors of t0 are 0.0 where the series has no such tick.
struct SeriesSource {
  const float *pred, *gt, *halo_pred, *halo_gt;
  const unsigned char *valid, *halo_valid;
  int t, n, first_tick;
  template <typename T>
  __device__ __forceinline__ const T* row(const T* body, const T* halo, int tt) const {
    const bool before = tt < 0;                  // halo row 3 + tt
    const int r = before ? (first_tick > 0 ? 3 + tt : 0) : min(tt, t - 1);
    return (before && first_tick > 0 ? halo : body) + (size_t)r * n;
  }
  __device__ __forceinline__ const float* pred_row(int tt) const { return row(pred, halo_pred, tt); }
  __device__ __forceinline__ const float* gt_row(int tt) const { return row(gt, halo_gt, tt); }
  __device__ __forceinline__ const unsigned char* valid_row(int tt) const { return row(valid, halo_valid, tt); }
  template <typename FA, typename FB>
  __device__ __forceinline__ void before(int t0, const Lanes&, double (&a)[3], double (&b)[3], FA&& na,
                                         FB&& nb) const {
    const int g0 = first_tick + t0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[k] = g0 >= 3 - k ? na(k) : 0.0;
      b[k] = g0 >= 3 - k ? nb(k) : 0.0;
    }
  }
};

// Top m: a tick keeps its m largest smoothed scores WITH their sensors.  The lane's two values of the sweep and the
// list carried over from earlier sweeps (entry r in lane r: cs / ci) are the candidates; m rounds of "wave maximum of
// (score, sensor), the owner masks it out" leave the new list, again entry r in lane r.  Order: larger score first,
// equal scores by the lower sensor (sensors are unique among the candidates, so every round has one owner).  A run
// starts from the empty list: every cs = -inf, every ci = NONE.
__device__ __forceinline__ void topm_merge(const Lanes& l, int lane, int m, double sma, double smb, double& cs,
                                           int& ci) {
  double v0 = l.la ? sma : -INFINITY, v1 = l.lb ? smb : -INFINITY, v2 = cs;
  int i0 = l.la ? l.sa : NONE, i1 = l.lb ? l.sb : NONE, i2 = ci;
  double ns = -INFINITY;
  int ni = NONE;
  for (int r = 0; r < m; ++r) {                  // (m is wave uniform)
    double bs = v0;
    int bi = i0;
    if (v1 > bs || (v1 == bs && i1 < bi)) { bs = v1; bi = i1; }
    if (v2 > bs || (v2 == bs && i2 < bi)) { bs = v2; bi = i2; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const double os = __shfl_xor(bs, d);
      const int oi = __shfl_xor(bi, d);
      if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
    }
    if (bi != NONE) {                            // the owner masks its candidate out
      if (i0 == bi) { v0 = -INFINITY; i0 = NONE; }
      if (i1 == bi) { v1 = -INFINITY; i1 = NONE; }
      if (i2 == bi) { v2 = -INFINITY; i2 = NONE; }
    }
    if (lane == r) { ns = bs; ni = bi; }
  }
  cs = ns;
  ci = ni;
}

// the lists of ticks [t0, t1): top_scores[t, m] descending, top_sensors[t, m]
__device__ __forceinline__ void topm_store(const double (&cs)[RUN], const int (&ci)[RUN], int lane, int m, int t0,
                                           int t1, double* __restrict__ top_scores, int* __restrict__ top_sensors) {
  if (lane < m) {
#pragma unroll
    for (int u = 0; u < RUN; ++u) {
      if (t0 + u < t1) {
        top_scores[(size_t)(t0 + u) * m + lane] = cs[u];
        top_sensors[(size_t)(t0 + u) * m + lane] = ci[u];
      }
    }
  }
}

// max over the 64 lanes for all 8 ticks together: a butterfly that also transposes — each step a lane keeps half of its
// ticks and hands the other half to its partner (8 + 4 + 2 exchanges), then three plain steps on the one tick left:
// 20 64-bit exchanges instead of 8 x 6 = 48 (max is exact in any order).  Lanes 0, 8, .., 56 end with the maximum of
// tick butterfly_tick(lane).
__device__ __forceinline__ double butterfly_max(const double (&mt)[RUN], int lane) {
  static_assert(RUN == 8, "the transposing reduction is written for 8 ticks");
  double k4[4], k2[2], k1;
  {
    const bool up = (lane & 32) != 0;
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2) {
      const double mine = up ? mt[4 + i2] : mt[i2], send = up ? mt[i2] : mt[4 + i2];
      k4[i2] = fmax(mine, __shfl_xor(send, 32));
    }
  }
  {
    const bool up = (lane & 16) != 0;
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2) {
      const double mine = up ? k4[2 + i2] : k4[i2], send = up ? k4[i2] : k4[2 + i2];
      k2[i2] = fmax(mine, __shfl_xor(send, 16));
    }
  }
  {
    const bool up = (lane & 8) != 0;
    const double mine = up ? k2[1] : k2[0], send = up ? k2[0] : k2[1];
    k1 = fmax(mine, __shfl_xor(send, 8));
  }
  k1 = fmax(k1, __shfl_xor(k1, 4));
  k1 = fmax(k1, __shfl_xor(k1, 2));
  k1 = fmax(k1, __shfl_xor(k1, 1));
  return k1;
}
__device__ __forceinline__ int butterfly_tick(int lane) {
  return ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);
}

}  // namespace gdn_sweep
