// Raw readings in (include/gdn_hip.h "Raw readings"): the front of the deployment path.  A plant delivers raw
// engineering units at the raw tick rate; the model reads [0, 1] medians of `down` raw ticks.  Three entry points:
// gdn_prep_stats (min / max / mean / count per sensor over its finite readings: what a min-max fit and a mean fill
// need), gdn_prep_series (a resident raw file -> the prepared sensor-major series) and gdn_prep_ticks (the stream's
// front end: raw ticks and the pending tail of the push before -> tick-major model ticks and the new tail).
// gdn_fleet_prep_ticks ("Raw readings of a fleet") is that front end per unit of a streaming fleet in one launch, the
// open groups and their lengths on the device; gdn_fleet_prep_ticks_units is the same launch with a table per unit.
// Raw data is tick-major [t_raw, n], fp32 or float64 (one template parameter); lanes run along sensors, so every
// row read is coalesced.  All arithmetic is float64, every product and sum an operation of its own.  Plain loads,
// compares and stores: no inline assembly, no atomics, no allocation, no synchronisation.
#include "gdn_common.hpp"

// numpy rounds x * scale and then + offset: no contraction of the pair into one fused multiply-add
#pragma clang fp contract(off)

namespace {

#define GDN_PREP_MAX_DOWN 64
#define GDN_PREP_THREADS 256
#define GDN_PREP_DEPTH 8             // row loads in flight per lane
#define GDN_PREP_COL_DOUBLES 4096    // LDS doubles for the waves' value columns: [waves][down][64] with waves * down <= 64
#define GDN_PREP_SEG_ROWS 256        // rows of a stats segment while there are fewer than the cap of segments

// "Missing" is decided on the bit pattern (exponent field all ones: NaN, +inf, -inf), gdn_stream_fill's rule; a
// float's NaN / inf converts to a double's.
__device__ inline bool prep_missing(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

bool prep_shape_ok(int n, int down) { return n >= 1 && n <= 4096 && down >= 1 && down <= GDN_PREP_MAX_DOWN; }

// waves of a workgroup of the median kernels: every wave owns a [down][64] float64 column block in LDS
int prep_waves(int down) { return down <= 16 ? 4 : down <= 32 ? 2 : 1; }

// segments of the stats sum: a function of the shape alone (never of the device), so the order of the sum is fixed
int prep_segments(long long t_raw, int n) {
  const int tiles = (n + 63) / 64;
  int cap = 2048 / tiles;
  cap = cap < 16 ? 16 : cap > 1024 ? 1024 : cap;
  const long long want = (t_raw + GDN_PREP_SEG_ROWS - 1) / GDN_PREP_SEG_ROWS;
  return (int)(want < 1 ? 1 : want > cap ? cap : want);
}

// Workgroup (tile, s): sensors [64 tile, 64 tile + 64), one per lane, rows [s * seg, (s + 1) * seg) ^ [0, t_raw).  Wave v
// walks rows r0 + v, r0 + v + 4, .. (DEPTH loads in flight) and keeps (min, max, sum, count) of the finite ones; the
// four waves meet in LDS and wave 0 folds them in wave order into partial[s, i, 0..3].
template <typename RAW>
__global__ __launch_bounds__(GDN_PREP_THREADS) void gdn_prep_stats_kernel(
    const RAW* __restrict__ raw, long long t_raw, int n, long long seg, double* __restrict__ partial) {
  __shared__ double part[GDN_PREP_THREADS / 64][4][64];
  constexpr int WAVES = GDN_PREP_THREADS / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const int ic = i < n ? i : n - 1;                                  // a dead lane reads sensor n - 1, writes nothing
  const long long r0 = (long long)blockIdx.y * seg, r1 = min(t_raw, r0 + seg);
  double mn = 0.0, mx = 0.0, sum = 0.0, cnt = 0.0;
  for (long long b = r0 + wv; b < r1; b += WAVES * GDN_PREP_DEPTH) {
    double v[GDN_PREP_DEPTH];
#pragma unroll
    for (int u = 0; u < GDN_PREP_DEPTH; ++u) {
      const long long row = b + (long long)u * WAVES;
      v[u] = (double)raw[(size_t)(row < r1 ? row : r1 - 1) * n + ic];
    }
#pragma unroll
    for (int u = 0; u < GDN_PREP_DEPTH; ++u) {
      if (b + (long long)u * WAVES < r1 && !prep_missing(v[u])) {
        if (cnt == 0.0) { mn = v[u]; mx = v[u]; }
        mn = v[u] < mn ? v[u] : mn;
        mx = v[u] > mx ? v[u] : mx;
        sum = sum + v[u];
        cnt = cnt + 1.0;
      }
    }
  }
  part[wv][0][lane] = mn;
  part[wv][1][lane] = mx;
  part[wv][2][lane] = sum;
  part[wv][3][lane] = cnt;
  __syncthreads();
  if (wv == 0 && i < n) {
    mn = 0.0; mx = 0.0; sum = 0.0; cnt = 0.0;
    for (int v = 0; v < WAVES; ++v) {
      const double c = part[v][3][lane];
      if (c == 0.0) continue;
      const double a = part[v][0][lane], z = part[v][1][lane];
      if (cnt == 0.0) { mn = a; mx = z; }
      mn = a < mn ? a : mn;
      mx = z > mx ? z : mx;
      sum = sum + part[v][2][lane];
      cnt = cnt + c;
    }
    double* __restrict__ o = partial + ((size_t)blockIdx.y * n + i) * 4;
    o[0] = mn; o[1] = mx; o[2] = sum; o[3] = cnt;
  }
}

// One thread per sensor folds the segments in segment order: stats[i] = (min, max, sum / count, count), all 0 for a
// sensor with no finite reading.
__global__ __launch_bounds__(GDN_PREP_THREADS) void gdn_prep_stats_finish_kernel(
    const double* __restrict__ partial, int segments, int n, double* __restrict__ stats) {
  const int i = blockIdx.x * GDN_PREP_THREADS + threadIdx.x;
  if (i >= n) return;
  double mn = 0.0, mx = 0.0, sum = 0.0, cnt = 0.0;
  for (int s = 0; s < segments; ++s) {
    const double* __restrict__ p = partial + ((size_t)s * n + i) * 4;
    const double c = p[3];
    if (c == 0.0) continue;
    if (cnt == 0.0) { mn = p[0]; mx = p[1]; }
    mn = p[0] < mn ? p[0] : mn;
    mx = p[1] > mx ? p[1] : mx;
    sum = sum + p[2];
    cnt = cnt + c;
  }
  stats[4 * (size_t)i + 0] = mn;
  stats[4 * (size_t)i + 1] = mx;
  stats[4 * (size_t)i + 2] = cnt == 0.0 ? 0.0 : sum / cnt;
  stats[4 * (size_t)i + 3] = cnt;
}

// The median of one group of `down` raw ticks of this lane's sensor, normalised: raw_at(j) is raw tick j of the group
// as float64.  A missing reading is replaced by `fillv` when have_fill, else left out; the others go as
// x * scale + offset into this lane's column of `col` [down][64] (bank = 2 lane mod 64 whatever the row: conflict
// free), packed from row 0.  Rank by counting (ties by position): the values of rank (cnt - 1) / 2 and cnt / 2 are the
// middle pair; their mean, or the middle value of an odd count, rounded to fp32; a quiet NaN for an empty group.
// Only the lane itself reads its column: no barrier.
template <class F>
__device__ inline float prep_group_median(F&& raw_at, int down, double scale, double offset, bool have_fill,
                                          double fillv, double* __restrict__ col, int lane) {
  int cnt = 0;
  for (int j0 = 0; j0 < down; j0 += GDN_PREP_DEPTH) {
    double v[GDN_PREP_DEPTH];
#pragma unroll
    for (int u = 0; u < GDN_PREP_DEPTH; ++u) v[u] = raw_at(min(j0 + u, down - 1));
#pragma unroll
    for (int u = 0; u < GDN_PREP_DEPTH; ++u) {
      if (j0 + u < down) {                                           // (wave uniform)
        double x = v[u];
        if (have_fill && prep_missing(x)) x = fillv;
        if (!prep_missing(x)) {
          col[cnt * 64 + lane] = x * scale + offset;
          ++cnt;
        }
      }
    }
  }
  if (cnt == 0) return __uint_as_float(0x7fc00000u);
  const int lo_rank = (cnt - 1) >> 1, hi_rank = cnt >> 1;
  double lo = 0.0, hi = 0.0;
  for (int j = 0; j < cnt; ++j) {
    const double vj = col[j * 64 + lane];
    int rank = 0;
    for (int k = 0; k < cnt; ++k) {
      const double vk = col[k * 64 + lane];
      rank += (vk < vj || (vk == vj && k < j)) ? 1 : 0;
    }
    if (rank == lo_rank) lo = vj;
    if (rank == hi_rank) hi = vj;
  }
  return (float)((cnt & 1) ? lo : (lo + hi) / 2.0);
}

// Workgroup (gt, tile): groups [64 gt, 64 gt + 64) of sensors [64 tile, 64 tile + 64).  Wave v takes groups v, v + waves,
// .. of the tile, lane = sensor (coalesced row reads), and leaves the medians in the padded LDS tile; after the barrier
// the lanes run along the groups and every wave writes whole 256-byte runs of series[i, :] (no 4-byte scattered
// stores).  The workgroups of tile 0 also reduce the labels of their 64 groups (one thread per group).
template <typename RAW>
__global__ __launch_bounds__(GDN_PREP_THREADS) void gdn_prep_series_kernel(
    const RAW* __restrict__ raw, int n, const double* __restrict__ table, const double* __restrict__ fill, int down,
    const double* __restrict__ labels_in, long long T, float* __restrict__ series, double* __restrict__ labels_out) {
  __shared__ double cols[GDN_PREP_COL_DOUBLES];
  __shared__ float tile[64][65];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const long long g0 = (long long)blockIdx.x * 64;
  const int s0 = blockIdx.y * 64;
  const int i = s0 + lane;
  const int ic = i < n ? i : n - 1;
  const double scale = table[2 * ic], offset = table[2 * ic + 1];
  const bool have_fill = fill != nullptr;
  const double fillv = have_fill ? fill[ic] : 0.0;
  double* __restrict__ col = cols + (size_t)wv * down * 64;
  for (int gl = wv; gl < 64; gl += waves) {
    const long long g = g0 + gl;
    if (g >= T) break;                                               // (wave uniform)
    const RAW* __restrict__ base = raw + (size_t)g * down * n + ic;
    tile[lane][gl] = prep_group_median([&](int j) { return (double)base[(size_t)j * n]; }, down, scale, offset,
                                       have_fill, fillv, col, lane);
  }
  __syncthreads();
  const long long g = g0 + lane;                                     // now the lane runs along the groups
  if (g < T) {
    for (int s = wv; s < 64; s += waves)
      if (s0 + s < n) series[(size_t)(s0 + s) * T + g] = tile[s][lane];
    if (labels_out != nullptr && blockIdx.y == 0 && wv == 0) {
      const double* __restrict__ lab = labels_in + (size_t)g * down;
      double m = lab[0];
      for (int j = 1; j < down; ++j) {
        const double v = lab[j];
        if (v > m || v != v) m = v;                                  // np.max: a NaN label wins
      }
      labels_out[g] = rint(m);                                       // np.round: half to even
    }
  }
}

// The stream's front end.  The raw ticks of the launch are [pend_in[:pending] | raw[:r]] (tick q < pending from the
// float64 plane, else row q - pending of raw).  Workgroup (tile, y < gy): wave v takes group y * waves + v, lane =
// sensor, and writes out[g, i]: tick-major, coalesced as it stands.  Workgroup (tile, gy): the tail, ticks
// groups * down .. pending + r - 1, goes to pend_out as float64 (bits of a float64 reading kept, NaN payload included).
template <typename RAW>
__global__ __launch_bounds__(GDN_PREP_THREADS) void gdn_prep_ticks_kernel(
    const RAW* __restrict__ raw, int r, const double* __restrict__ pend_in, int pending,
    double* __restrict__ pend_out, int n, int down, const double* __restrict__ table, float* __restrict__ out,
    int groups, int gy) {
  __shared__ double cols[GDN_PREP_COL_DOUBLES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const int ic = i < n ? i : n - 1;
  auto tick = [&](int q) -> double {
    return q < pending ? pend_in[(size_t)q * n + ic] : (double)raw[(size_t)(q - pending) * n + ic];
  };
  if ((int)blockIdx.y == gy) {
    const int first = groups * down, tail = pending + r - first;    // tail < down
    for (int j = wv; j < tail; j += waves) {
      const double v = tick(first + j);
      if (i < n) pend_out[(size_t)j * n + i] = v;
    }
    return;
  }
  const int g = blockIdx.y * waves + wv;
  if (g >= groups) return;                                           // (wave uniform; no barrier below)
  const float med = prep_group_median([&](int j) { return tick(g * down + j); }, down, table[2 * ic],
                                      table[2 * ic + 1], false, 0.0, cols + (size_t)wv * down * 64, lane);
  if (i < n) out[(size_t)g * n + i] = med;
}

// The fleet's front end (include/gdn_hip.h "Raw readings of a fleet"): gdn_prep_ticks per unit, with the unit's open
// group and its count kept ON THE DEVICE.  Workgroup (tile, u): sensors [64 tile, 64 tile + 64) of unit u, lane = sensor.
// k = raw_counts[u] clamped to 0 .. rows, p = this tile's own count word; the raw ticks of the unit are
// [pend_ticks[u, :p] | raw[u, :k]].  Wave v takes groups v, v + waves, .. < groups = (p + k) / down and writes
// out[u, g, i] (coalesced).  After ONE barrier (every read of the pending rows lies before it) the workgroup writes
// the new tail into ITS OWN 64 columns of pend_ticks[u], then its own count word; tile 0 also writes counts[u].  A
// workgroup reads nothing that another workgroup of the launch writes (a dead lane reads column n - 1: its own tile's),
// so the state is updated in place with no second plane, no host parity and no atomic.  k == 0: counts[u] = 0 and
// nothing else.  A count word outside 0 .. down - 1 (never written by this kernel) is clamped: no index leaves a buffer.
// table_stride: doubles between two units' tables: 0 (gdn_fleet_prep_ticks: one table [n, 2] for all units) or 2 n
// (gdn_fleet_prep_ticks_units: tables [U, n, 2]); the workgroup reads its own 64 rows of unit u's table either way.
template <typename RAW>
__global__ __launch_bounds__(GDN_PREP_THREADS) void gdn_fleet_prep_ticks_kernel(
    const RAW* __restrict__ raw, int rows, const int* __restrict__ raw_counts, double* __restrict__ pend_ticks,
    int* __restrict__ pend_counts, int c, int n, int down, const double* __restrict__ table, size_t table_stride,
    float* __restrict__ out, int* __restrict__ counts) {
  __shared__ double cols[GDN_PREP_COL_DOUBLES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int tile = blockIdx.x, u = blockIdx.y;
  const int k = min(max(raw_counts[u], 0), rows);
  if (k == 0) {                                                      // (workgroup uniform, ahead of the barrier)
    if (tile == 0 && threadIdx.x == 0) counts[u] = 0;
    return;
  }
  int* __restrict__ word = pend_counts + (size_t)u * gridDim.x + tile;
  const int p = min(max(*word, 0), down - 1);
  const int groups = (p + k) / down;                                 // <= c: p < down, k <= rows <= c down
  const int i = tile * 64 + lane;
  const int ic = i < n ? i : n - 1;
  const RAW* __restrict__ ru = raw + (size_t)u * rows * n;
  double* __restrict__ pu = pend_ticks + (size_t)u * down * n;
  auto tick = [&](int q) -> double { return q < p ? pu[(size_t)q * n + ic] : (double)ru[(size_t)(q - p) * n + ic]; };
  const double* __restrict__ tu = table + (size_t)u * table_stride;
  const double scale = tu[2 * ic], offset = tu[2 * ic + 1];
  double* __restrict__ col = cols + (size_t)wv * down * 64;
  float* __restrict__ ou = out + (size_t)u * c * n;
  for (int g = wv; g < groups; g += waves) {
    const float med = prep_group_median([&](int j) { return tick(g * down + j); }, down, scale, offset, false, 0.0,
                                        col, lane);
    if (i < n) ou[(size_t)g * n + i] = med;
  }
  __syncthreads();
  // groups >= 1: the tail lies in raw alone (groups * down >= down > p); else the k new rows go behind the p that stay
  const int first = groups ? groups * down - p : 0, at = groups ? 0 : p, tail = groups ? p + k - groups * down : k;
  for (int j = wv; j < tail; j += waves) {
    const double v = (double)ru[(size_t)(first + j) * n + ic];
    if (i < n) pu[(size_t)(at + j) * n + i] = v;
  }
  if (threadIdx.x == 0) {
    *word = at + tail;
    if (tile == 0) counts[u] = groups;
  }
}

template <typename RAW>
int prep_stats(const void* raw, long long t_raw, int n, double* workspace, double* stats, hipStream_t stream) {
  const int segments = prep_segments(t_raw, n);
  const long long seg = (t_raw + segments - 1) / segments;
  hipLaunchKernelGGL(gdn_prep_stats_kernel<RAW>, dim3(((unsigned)n + 63) / 64, (unsigned)segments),
                     dim3(GDN_PREP_THREADS), 0, stream, static_cast<const RAW*>(raw), t_raw, n, seg, workspace);
  hipLaunchKernelGGL(gdn_prep_stats_finish_kernel, dim3(((unsigned)n + GDN_PREP_THREADS - 1) / GDN_PREP_THREADS),
                     dim3(GDN_PREP_THREADS), 0, stream, workspace, segments, n, stats);
  return gdn_launch_status();
}

template <typename RAW>
int prep_series(const void* raw, int n, const double* table, const double* fill, int down, const double* labels_in,
                long long T, float* series, double* labels_out, hipStream_t stream) {
  hipLaunchKernelGGL(gdn_prep_series_kernel<RAW>, dim3((unsigned)((T + 63) / 64), ((unsigned)n + 63) / 64),
                     dim3(64 * prep_waves(down)), 0, stream, static_cast<const RAW*>(raw), n, table, fill, down,
                     labels_in, T, series, labels_out);
  return gdn_launch_status();
}

template <typename RAW>
int prep_ticks(const void* raw, int r, const double* pend_in, int pending, double* pend_out, int n, int down,
               const double* table, float* out, int groups, hipStream_t stream) {
  const int waves = prep_waves(down), gy = (groups + waves - 1) / waves;
  hipLaunchKernelGGL(gdn_prep_ticks_kernel<RAW>, dim3(((unsigned)n + 63) / 64, (unsigned)gy + 1), dim3(64 * waves), 0,
                     stream, static_cast<const RAW*>(raw), r, pend_in, pending, pend_out, n, down, table, out, groups,
                     gy);
  return gdn_launch_status();
}

template <typename RAW>
int fleet_prep_ticks(const void* raw, int rows, const int32_t* raw_counts, void* pend, int units, int c, int n, int down,
                     const double* table, size_t table_stride, float* out, int32_t* counts, hipStream_t stream) {
  const unsigned tiles = ((unsigned)n + 63) / 64;
  double* ticks = static_cast<double*>(pend);
  int* words = reinterpret_cast<int*>(ticks + (size_t)units * down * n);
  hipLaunchKernelGGL(gdn_fleet_prep_ticks_kernel<RAW>, dim3(tiles, (unsigned)units), dim3(64 * prep_waves(down)), 0,
                     stream, static_cast<const RAW*>(raw), rows, raw_counts, ticks, words, c, n, down, table,
                     table_stride, out, counts);
  return gdn_launch_status();
}

}  // namespace

extern "C" long long gdn_prep_stats_workspace_bytes(long long t_raw, int n) {
  if (t_raw < 1 || n < 1 || n > 4096) return 0;
  return 32ll * prep_segments(t_raw, n) * n;
}

extern "C" int gdn_prep_stats(const void* raw, long long t_raw, int n, int raw_f64, void* workspace, double* stats,
                              void* stream) {
  if (!raw || !workspace || !stats || t_raw < 1) return GDN_ERR_ARG;
  if (n < 1 || n > 4096) return GDN_ERR_UNSUPPORTED;
  return raw_f64 ? prep_stats<double>(raw, t_raw, n, static_cast<double*>(workspace), stats, (hipStream_t)stream)
                 : prep_stats<float>(raw, t_raw, n, static_cast<double*>(workspace), stats, (hipStream_t)stream);
}

extern "C" int gdn_prep_series(const void* raw, long long t_raw, int n, int raw_f64, const double* table,
                               const double* fill, int down, const double* labels_in, float* series,
                               double* labels_out, void* stream) {
  if (!raw || !table || !series || (labels_out && !labels_in)) return GDN_ERR_ARG;
  if (!prep_shape_ok(n, down)) return GDN_ERR_UNSUPPORTED;
  const long long T = t_raw / down;
  if (t_raw < 1 || T < 1 || (T + 63) / 64 > 0x7fffffffll) return GDN_ERR_ARG;
  return raw_f64 ? prep_series<double>(raw, n, table, fill, down, labels_in, T, series, labels_out, (hipStream_t)stream)
                 : prep_series<float>(raw, n, table, fill, down, labels_in, T, series, labels_out, (hipStream_t)stream);
}

extern "C" int gdn_prep_ticks(const void* raw, int r, int raw_f64, const double* pend_in, int pending,
                              double* pend_out, int n, int down, const double* table, float* out, int c,
                              void* stream) {
  if (!raw || !pend_in || !pend_out || !table || !out || pend_in == pend_out) return GDN_ERR_ARG;
  if (!prep_shape_ok(n, down)) return GDN_ERR_UNSUPPORTED;
  if (r < 1 || c < 1 || pending < 0 || pending >= down) return GDN_ERR_ARG;
  const long long groups = ((long long)pending + r) / down;
  if (groups > c) return GDN_ERR_ARG;
  return raw_f64 ? prep_ticks<double>(raw, r, pend_in, pending, pend_out, n, down, table, out, (int)groups,
                                      (hipStream_t)stream)
                 : prep_ticks<float>(raw, r, pend_in, pending, pend_out, n, down, table, out, (int)groups,
                                     (hipStream_t)stream);
}

// pend: the pending ticks of all units first ([U, down, n] float64), then one int32 count per (unit, tile of 64 sensors)
// ([U, tiles]), rounded up to 8 bytes.
extern "C" long long gdn_fleet_prep_bytes(int units, int n, int down) {
  if (units < 1 || units > GDN_FLEET_MAX_ROWS || !prep_shape_ok(n, down)) return 0;
  return 8ll * units * down * n + ((4ll * units * ((n + 63) / 64) + 7) & ~7ll);
}

// the two entry points of the fleet's front end: one body, the table stride apart
static int fleet_prep_ticks_any(const void* raw, int rows, int raw_f64, const int32_t* raw_counts, void* pend, int units,
                                int c, int n, int down, const double* table, size_t table_stride, float* out,
                                int32_t* counts, void* stream) {
  if (!raw || !raw_counts || !pend || !table || !out || !counts) return GDN_ERR_ARG;
  if (!gdn_fleet_rows_ok(units, c) || !prep_shape_ok(n, down)) return GDN_ERR_UNSUPPORTED;
  if (rows < 1 || rows > c * down) return GDN_ERR_ARG;
  return raw_f64 ? fleet_prep_ticks<double>(raw, rows, raw_counts, pend, units, c, n, down, table, table_stride, out,
                                            counts, (hipStream_t)stream)
                 : fleet_prep_ticks<float>(raw, rows, raw_counts, pend, units, c, n, down, table, table_stride, out,
                                           counts, (hipStream_t)stream);
}

extern "C" int gdn_fleet_prep_ticks(const void* raw, int rows, int raw_f64, const int32_t* raw_counts, void* pend,
                                    int units, int c, int n, int down, const double* table, float* out,
                                    int32_t* counts, void* stream) {
  return fleet_prep_ticks_any(raw, rows, raw_f64, raw_counts, pend, units, c, n, down, table, 0, out, counts, stream);
}

extern "C" int gdn_fleet_prep_ticks_units(const void* raw, int rows, int raw_f64, const int32_t* raw_counts, void* pend,
                                          int units, int c, int n, int down, const double* tables, float* out,
                                          int32_t* counts, void* stream) {
  return fleet_prep_ticks_any(raw, rows, raw_f64, raw_counts, pend, units, c, n, down, tables, n > 0 ? 2 * (size_t)n : 0,
                              out, counts, stream);
}
