// The archive side of a fleet (include/gdn_hip.h "fleet series"): U units of ONE model, each with a
// resident series of its own, scored in launches that cover all units.  Every tensor is a stack of per-unit planes
// (pred / gt [U, t, n], valid [U, t, n], keep [U, t], med_iqr [U, n, 2], keys [U, n, pitch]) and unit u's plane is
// written bit for bit as the single-series entry points of gdn_score.hip / gdn_series_gaps.hip write it:
//   keys    the transposing tile of score_keys_kernel per (tick tile, sensor tile, unit), with the keep flags or the
//           validity plane deciding where the filler goes;
//   smooth  the sweep of gdn_score_sweep.hpp over the U * ceil(t / RUN) runs of all units.  A run belongs to ONE unit and
//           reads through that unit's SeriesSource with first_tick = 0: rows clamp inside the unit's plane and the three
//           predecessors of the unit's tick 0 are zeros, so nothing crosses a unit seam in either direction.
// No floating-point atomics, no workgroup waits on another.
#include "gdn_score_sweep.hpp"

namespace {

using namespace gdn_sweep;

enum KeyMode { KEYS_PLAIN = 0, KEYS_KEEP = 1, KEYS_VALID = 2 };

// Workgroup (tick tile, sensor tile, unit): keys[u][s][tick] = |pred[u][tick][s] - gt[u][tick][s]| through the LDS tile
// of score_keys_kernel.  KEYS_VALID: a missing reading's tile entry is the filler itself (score_keys_valid_kernel);
// KEYS_KEEP: a tick whose flag is 0 gets the filler in all n keys (score_keys_keep_kernel).  Slots t .. pitch-1: filler.
template <int MODE>
__global__ __launch_bounds__(256) void fleet_series_keys_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ gt,
                                                                const unsigned char* __restrict__ mask, int t, int n,
                                                                int pitch, double* __restrict__ keys) {
  __shared__ double tile[64][65];
  const int t0 = blockIdx.x * 64, s0 = blockIdx.y * 64;
  const size_t u = blockIdx.z;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t plane = u * (size_t)t * n;
  for (int r = wv; r < 64; r += 4) {
    const int tick = t0 + r, s = s0 + lane;
    if (tick < t && s < n) {
      const size_t o = plane + (size_t)tick * n + s;
      const double e = score_key(pred[o], gt[o]);
      if constexpr (MODE == KEYS_VALID) tile[r][lane] = mask[o] != 0 ? e : filler_key();
      else tile[r][lane] = e;
    }
  }
  __syncthreads();
  const int tick = t0 + lane;
  bool real = tick < t;
  if constexpr (MODE == KEYS_KEEP) real = real && mask[u * (size_t)t + tick] != 0;
  double* __restrict__ out = keys + u * (size_t)n * pitch;
  for (int r = wv; r < 64; r += 4) {
    const int s = s0 + r;
    if (s < n && tick < pitch) out[(size_t)s * pitch + tick] = real ? tile[lane][r] : filler_key();
  }
}

// the planes of unit u as a series of its own: no halo, first_tick = 0
__device__ __forceinline__ SeriesSource unit_source(const float* pred, const float* gt, const unsigned char* valid,
                                                    size_t u, int t, int n) {
  const size_t plane = u * (size_t)t * n;
  return {pred + plane, gt + plane, nullptr, nullptr, valid ? valid + plane : nullptr, nullptr, t, n, 0};
}

// score_smooth_max_kernel over the runs of all units: anomaly [U, t], `scores` (optional) [U, n, t].
template <bool GAPS>
__global__ __launch_bounds__(256) void fleet_series_smooth_max_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt, const double* __restrict__ med_iqr_all, int units,
    int t, int n, double* __restrict__ scores_all, double* __restrict__ anomaly_all,
    const unsigned char* __restrict__ valid) {
  __shared__ double best[4][RUN];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int nruns = (t + RUN - 1) / RUN, total = units * nruns;
  for (int job = blockIdx.x * wpb + wv; job < total; job += gridDim.x * wpb) {
    const int u = job / nruns, run = job - u * nruns;      // (wave uniform)
    const int t0 = run * RUN, t1 = min(t, t0 + RUN);
    const SeriesSource src = unit_source(pred, gt, valid, u, t, n);
    const double* __restrict__ med_iqr = med_iqr_all + (size_t)u * 2 * n;
    double* __restrict__ scores = scores_all ? scores_all + (size_t)u * n * t : nullptr;
    for (int s0 = 0; s0 < n; s0 += 128) {
      const Lanes l(s0, lane, n);
      double mt[RUN];
#pragma unroll
      for (int k = 0; k < RUN; ++k) mt[k] = -INFINITY;
      score_sweep<GAPS>(src, med_iqr, l, t0, t1, 0, [&](int k, int tick, double sma, double smb) {
        if (scores) {
          if (l.la) scores[(size_t)l.sa * t + tick] = sma;
          if (l.lb) scores[(size_t)l.sb * t + tick] = smb;
        }
        mt[k] = fmax(l.la ? sma : -INFINITY, l.lb ? smb : -INFINITY);
      });
      const double k1 = butterfly_max(mt, lane);
      if ((lane & 7) == 0) {
        const int k = butterfly_tick(lane);
        best[wv][k] = s0 == 0 ? k1 : fmax(best[wv][k], k1);
      }
    }
    // (LDS writes above and reads below are by the same wave, in program order)
    if (lane < t1 - t0) anomaly_all[(size_t)u * t + t0 + lane] = best[wv][lane];
  }
}

// score_smooth_topm_kernel over the runs of all units: top_scores / top_sensors [U, t, m].
template <bool GAPS>
__global__ __launch_bounds__(256) void fleet_series_smooth_topm_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt, const double* __restrict__ med_iqr_all, int units,
    int t, int n, int m, double* __restrict__ top_scores, int* __restrict__ top_sensors,
    const unsigned char* __restrict__ valid) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int nruns = (t + RUN - 1) / RUN, total = units * nruns;
  for (int job = blockIdx.x * wpb + wv; job < total; job += gridDim.x * wpb) {
    const int u = job / nruns, run = job - u * nruns;      // (wave uniform)
    const int t0 = run * RUN, t1 = min(t, t0 + RUN);
    const SeriesSource src = unit_source(pred, gt, valid, u, t, n);
    const double* __restrict__ med_iqr = med_iqr_all + (size_t)u * 2 * n;
    double cs[RUN];
    int ci[RUN];
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
      cs[k] = -INFINITY;
      ci[k] = NONE;
    }
    for (int s0 = 0; s0 < n; s0 += 128) {
      const Lanes l(s0, lane, n);
      score_sweep<GAPS>(src, med_iqr, l, t0, t1, 0, [&](int k, int, double sma, double smb) {
        topm_merge(l, lane, m, sma, smb, cs[k], ci[k]);
      });
    }
    topm_store(cs, ci, lane, m, t0, t1, top_scores + (size_t)u * t * m, top_sensors + (size_t)u * t * m);
  }
}

// The limits of every entry point here, decided before any launch: 1 <= units, n <= 4096, t >= 1 and a key block
// [units, n, pitch] float64 (the smooth launches: pitch = t) of at most 2 GiB, which also keeps every job and tick
// count of the kernels inside an int.
int fleet_series_shape(int units, int t, int n, int pitch) {
  if (t < 1 || pitch < t) return GDN_ERR_ARG;
  if (units < 1 || units > 4096 || n < 1 || n > 4096) return GDN_ERR_UNSUPPORTED;
  if (8ll * units * n * (long long)pitch > (2ll << 30)) return GDN_ERR_UNSUPPORTED;
  return GDN_OK;
}

// grid of a smooth launch: sweep_grid over the runs of all units (units * ceil(t / RUN) * RUN <= 2^28 + 8 * 4096)
int fleet_sweep_grid(int units, int t) { return sweep_grid(units * ((t + RUN - 1) / RUN) * RUN); }

template <bool GAPS>
int fleet_smooth_max(const float* pred, const float* gt, const double* med_iqr, int units, int t, int n,
                     double* scores, double* anomaly, const uint8_t* valid, void* stream) {
  if (!pred || !gt || !med_iqr || !anomaly || (GAPS && !valid)) return GDN_ERR_ARG;
  const int rc = fleet_series_shape(units, t, n, t);
  if (rc != GDN_OK) return rc;
  hipLaunchKernelGGL(fleet_series_smooth_max_kernel<GAPS>, dim3(fleet_sweep_grid(units, t)), dim3(256), 0,
                     (hipStream_t)stream, pred, gt, med_iqr, units, t, n, scores, anomaly, valid);
  return gdn_launch_status();
}

template <bool GAPS>
int fleet_smooth_topm(const float* pred, const float* gt, const double* med_iqr, int units, int t, int n, int m,
                      double* top_scores, int32_t* top_sensors, const uint8_t* valid, void* stream) {
  if (!pred || !gt || !med_iqr || !top_scores || !top_sensors || (GAPS && !valid)) return GDN_ERR_ARG;
  const int rc = fleet_series_shape(units, t, n, t);
  if (rc != GDN_OK) return rc;
  if (m < 1 || m > TOPM_MAX || m > n) return GDN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fleet_series_smooth_topm_kernel<GAPS>, dim3(fleet_sweep_grid(units, t)), dim3(256), 0,
                     (hipStream_t)stream, pred, gt, med_iqr, units, t, n, m, top_scores, top_sensors, valid);
  return gdn_launch_status();
}

}  // namespace

extern "C" int gdn_fleet_series_keys(const float* pred, const float* gt, const uint8_t* keep, const uint8_t* valid,
                                     int units, int t, int n, int pitch, double* keys, void* stream) {
  if (!pred || !gt || !keys || (keep && valid)) return GDN_ERR_ARG;
  const int rc = fleet_series_shape(units, t, n, pitch);
  if (rc != GDN_OK) return rc;
  const dim3 grid((pitch + 63) / 64, (n + 63) / 64, units);
  const hipStream_t st = (hipStream_t)stream;
  if (valid) hipLaunchKernelGGL(fleet_series_keys_kernel<KEYS_VALID>, grid, dim3(256), 0, st, pred, gt, valid, t, n, pitch, keys);
  else if (keep) hipLaunchKernelGGL(fleet_series_keys_kernel<KEYS_KEEP>, grid, dim3(256), 0, st, pred, gt, keep, t, n, pitch, keys);
  else hipLaunchKernelGGL(fleet_series_keys_kernel<KEYS_PLAIN>, grid, dim3(256), 0, st, pred, gt, nullptr, t, n, pitch, keys);
  return gdn_launch_status();
}

extern "C" int gdn_fleet_series_smooth_max(const float* pred, const float* gt, const double* med_iqr, int units, int t,
                                           int n, double* scores, double* anomaly, void* stream) {
  return fleet_smooth_max<false>(pred, gt, med_iqr, units, t, n, scores, anomaly, nullptr, stream);
}

extern "C" int gdn_fleet_series_smooth_max_gaps(const float* pred, const float* gt, const double* med_iqr, int units,
                                                int t, int n, double* scores, double* anomaly, const uint8_t* valid,
                                                void* stream) {
  return fleet_smooth_max<true>(pred, gt, med_iqr, units, t, n, scores, anomaly, valid, stream);
}

extern "C" int gdn_fleet_series_smooth_topm(const float* pred, const float* gt, const double* med_iqr, int units, int t,
                                            int n, int m, double* top_scores, int32_t* top_sensors, void* stream) {
  return fleet_smooth_topm<false>(pred, gt, med_iqr, units, t, n, m, top_scores, top_sensors, nullptr, stream);
}

extern "C" int gdn_fleet_series_smooth_topm_gaps(const float* pred, const float* gt, const double* med_iqr, int units,
                                                 int t, int n, int m, double* top_scores, int32_t* top_sensors,
                                                 const uint8_t* valid, void* stream) {
  return fleet_smooth_topm<true>(pred, gt, med_iqr, units, t, n, m, top_scores, top_sensors, valid, stream);
}
