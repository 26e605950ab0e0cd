// The streaming fleet (include/gdn_hip.h "streaming fleet"): U units of ONE model, each with a stream state, a median /
// IQR table, a threshold and an alarm log of its own, pushed together so that the model's forward sees units x c
// windows.  Unit u's state is a single stream's state (gdn_stream_state_bytes(n, w) bytes) at state + u * that many
// bytes, and every launch here is the single-stream launch's work per unit: the steps are the __device__ functions of
// gdn_stream_steps.hpp that the single-stream kernels call, so a unit is written bit for bit as a stream is.
// counts [U] int32 lives on the device: how many rows of unit u are real in this push.  Every kernel reads it there and
// clamps it to 0 .. c; it is never a launch argument, so one captured graph serves a full push, a short one and one in
// which some units are silent.  Only gdn_fleet_advance writes the states; a unit with counts[u] == 0 is not touched.
// Missing readings (opt-in): gdn_fleet_fill leads the push and the score / advance kernels have a GAPS
// instantiation each, per unit the single stream's; the plain instantiations never read the trailing parameters.  (The
// episodes launch of a fleet, gdn_fleet_events, lives with the tile code in gdn_events.hip.)
// Plain copy, sweep and scan kernels: no inline assembly, no floating-point atomics, no workgroup waits on another.
#include "gdn_stream_steps.hpp"

// (float64 scoring: gdn_score_sweep.hpp switches FMA contraction off for this unit)

namespace {

using namespace gdn_stream_steps;

__device__ __forceinline__ int fleet_count(const int* __restrict__ counts, int u, int c) {
  return min(max(counts[u], 0), c);
}
__device__ __forceinline__ void* fleet_state(void* state, int u, int n, int w) {
  return reinterpret_cast<char*>(state) + (size_t)u * (size_t)stream_state_size(n, w);
}
__device__ __forceinline__ const void* fleet_state(const void* state, int u, int n, int w) {
  return reinterpret_cast<const char*>(state) + (size_t)u * (size_t)stream_state_size(n, w);
}

// Workgroup (span, u): gdn_stream_init of unit u from history[u].
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_fleet_init_kernel(
    void* __restrict__ state, const float* __restrict__ history, long long h, int n, int w) {
  const int u = blockIdx.y;
  stream_seed_span(fleet_state(state, u, n, w), history + (size_t)u * n * h, h, n, w, blockIdx.x, threadIdx.x);
}

// Workgroup (b, span, u): a real row (b < counts[u]) is the single stream's window; any other row is zeros, so the
// forward's input depends on the states and this push alone.
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_fleet_windows_kernel(
    const void* __restrict__ state, const float* __restrict__ chunk, const int* __restrict__ counts, int c, int n,
    int w, float* __restrict__ x_out) {
  const int b = blockIdx.x, u = blockIdx.z;
  const unsigned nw = (unsigned)n * (unsigned)w;
  float* __restrict__ xb = x_out + ((size_t)u * c + b) * nw;
  if (b < fleet_count(counts, u, c)) {                       // (workgroup uniform)
    stream_window_span(fleet_state(state, u, n, w), chunk + (size_t)u * c * n, n, w, b, blockIdx.y, threadIdx.x, xb);
    return;
  }
  const unsigned f0 = blockIdx.y * GDN_STREAM_SPAN + threadIdx.x;
#pragma unroll
  for (int j = 0; j < GDN_STREAM_PER_THREAD; ++j) {
    const unsigned f = f0 + j * GDN_STREAM_THREADS;
    if (f < nw) xb[f] = 0.f;
  }
}

// Workgroup (g, u) of WAVES waves: gdn_stream_fill's workgroup g on unit u's rows with count = counts[u]; 0 writes
// nothing, gap_chunk included.  WAVES comes from c on the host (fleet_fill below), never from counts.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gdn_fleet_fill_kernel(
    const void* __restrict__ state, const float* __restrict__ raw, const int* __restrict__ counts, int c, int n, int w,
    float* __restrict__ filled, unsigned char* __restrict__ valid, int* __restrict__ gap_chunk) {
  const int u = blockIdx.y;
  const int count = fleet_count(counts, u, c);
  if (count == 0) return;                                    // (workgroup uniform, ahead of the barrier)
  const size_t row0 = (size_t)u * c * n;
  stream_fill_group<WAVES>(fleet_state(state, u, n, w), raw + row0, count, n, w, filled + row0, valid + row0,
                           gap_chunk + (size_t)u * 2 * n, blockIdx.x, threadIdx.x);
}

// One wave per (unit, run of RUN ticks): runs = ceil(c / RUN) per unit; a run at or past counts[u] writes nothing.
// GAPS: `gt` is the filled chunk and valid [U, c, n] its plane; the plain instantiation never reads `valid`.
template <bool GAPS>
__global__ __launch_bounds__(256) void gdn_fleet_score_kernel(
    const void* __restrict__ state, const float* __restrict__ pred, const float* __restrict__ gt,
    const double* __restrict__ med_iqr, const double* __restrict__ threshold, const int* __restrict__ counts, int units,
    int c, int n, int w, int m, double* __restrict__ top_scores, int* __restrict__ top_sensors,
    int* __restrict__ alarm, const unsigned char* __restrict__ valid) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nruns = (c + RUN - 1) / RUN;
  const int at = blockIdx.x * (blockDim.x >> 6) + wv;        // (wave uniform) <= 4096 + 3
  const int u = at / nruns, run = at - u * nruns;
  if (u >= units) return;
  const int t = fleet_count(counts, u, c);
  if (run * RUN >= t) return;
  const void* st = fleet_state(state, u, n, w);
  const long long first_tick = reinterpret_cast<const long long*>(st)[0];
  const size_t row0 = (size_t)u * c;
  const unsigned char* vu = nullptr;
  if constexpr (GAPS) vu = valid + row0 * n;
  const StreamSource src{pred + row0 * n, gt + row0 * n, vu, stream_carry(st), t, n};
  stream_score_run<GAPS>(src, med_iqr + (size_t)u * 2 * n, threshold[u], first_tick, run, lane, m,
                         top_scores + row0 * m, top_sensors + row0 * m, alarm + row0);
}

// Workgroup (i, u): gdn_stream_advance's workgroup i of unit u with count = counts[u]; 0 leaves the unit as it is.
// GAPS: `chunk` is the filled chunk; valid [U, c, n], gap_chunk [U, 2, n] and gaps [U, 2, n] are unit u's slices of
// what gdn_stream_advance_gaps takes (a silent unit's gaps row stays).  The plain instantiation reads none of the three.
template <bool GAPS>
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_fleet_advance_kernel(
    void* __restrict__ state, const float* __restrict__ chunk, const float* __restrict__ pred,
    const double* __restrict__ med_iqr, const int* __restrict__ alarm, const int* __restrict__ top_sensors,
    const int* __restrict__ counts, int c, int n, int w, int m, long long* __restrict__ log_ticks,
    int* __restrict__ log_sensors, long long log_len, const unsigned char* __restrict__ valid,
    const int* __restrict__ gap_chunk, long long* __restrict__ gaps) {
  const int u = blockIdx.y;
  const int count = fleet_count(counts, u, c);
  if (count == 0) return;                                    // (workgroup uniform, ahead of every barrier)
  void* st = fleet_state(state, u, n, w);
  const size_t row0 = (size_t)u * c;
  if ((int)blockIdx.x < n) {
    stream_roll_row(st, chunk + row0 * n, count, n, w, blockIdx.x, threadIdx.x);
    return;
  }
  const unsigned char* vu = nullptr;
  const int* gu = nullptr;
  long long* au = nullptr;
  if constexpr (GAPS) {
    vu = valid + row0 * n;
    gu = gap_chunk + (size_t)u * 2 * n;
    au = gaps + (size_t)u * 2 * n;
  }
  stream_carry_log<GAPS>(st, chunk + row0 * n, pred + row0 * n, med_iqr + (size_t)u * 2 * n, alarm + row0,
                         top_sensors + row0 * m, count, n, m, log_ticks + (size_t)u * log_len,
                         log_sensors + (size_t)u * log_len * m, log_len, threadIdx.x, vu, gu, au);
}

template <int WAVES>
void fleet_fill_launch(const void* state, const float* raw, const int32_t* counts, int units, int c, int n, int w,
                       float* filled, uint8_t* valid, int32_t* gap_chunk, hipStream_t stream) {
  hipLaunchKernelGGL(gdn_fleet_fill_kernel<WAVES>, dim3(((unsigned)n + 63) / 64, (unsigned)units), dim3(WAVES * 64), 0,
                     stream, state, raw, counts, c, n, w, filled, valid, gap_chunk);
}

template <bool GAPS>
int fleet_score(const void* state, const float* pred, const float* chunk, const uint8_t* valid, const double* med_iqr,
                const double* threshold, const int32_t* counts, int units, int c, int n, int w, int m,
                double* top_scores, int32_t* top_sensors, int32_t* alarm, void* stream) {
  if (!state || !pred || !chunk || (GAPS && !valid) || !med_iqr || !threshold || !counts || !top_scores ||
      !top_sensors || !alarm)
    return GDN_ERR_ARG;
  if (!gdn_fleet_rows_ok(units, c) || !stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  if (m < 1 || m > TOPM_MAX || m > n) return GDN_ERR_UNSUPPORTED;
  const unsigned waves = (unsigned)units * (((unsigned)c + RUN - 1) / RUN);          // <= 4096
  hipLaunchKernelGGL(gdn_fleet_score_kernel<GAPS>, dim3((waves + 3) / 4), dim3(256), 0, (hipStream_t)stream, state,
                     pred, chunk, med_iqr, threshold, counts, units, c, n, w, m, top_scores, top_sensors, alarm, valid);
  return gdn_launch_status();
}

template <bool GAPS>
int fleet_advance(void* state, const float* chunk, const float* pred, const uint8_t* valid, const int32_t* gap_chunk,
                  const double* med_iqr, const int32_t* alarm, const int32_t* top_sensors, const int32_t* counts,
                  int units, int c, int n, int w, int m, int64_t* log_ticks, int32_t* log_sensors, long long log_len,
                  int64_t* gaps, void* stream) {
  if (!state || !chunk || !pred || !med_iqr || !alarm || !top_sensors || !counts ||
      (GAPS && (!valid || !gap_chunk || !gaps)))
    return GDN_ERR_ARG;
  if (log_len < 0 || (log_len > 0 && (!log_ticks || !log_sensors))) return GDN_ERR_ARG;
  if (!gdn_fleet_rows_ok(units, c) || !stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  if (m < 1 || m > TOPM_MAX || m > n) return GDN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gdn_fleet_advance_kernel<GAPS>, dim3((unsigned)n + 1, (unsigned)units), dim3(GDN_STREAM_THREADS),
                     0, (hipStream_t)stream, state, chunk, pred, med_iqr, alarm, top_sensors, counts, c, n, w, m,
                     reinterpret_cast<long long*>(log_ticks), log_sensors, log_len, valid, gap_chunk,
                     reinterpret_cast<long long*>(gaps));
  return gdn_launch_status();
}

}  // namespace

extern "C" long long gdn_fleet_state_bytes(int units, int n, int w) {
  if (units < 1 || !stream_shape_ok(n, w)) return 0;
  return (long long)units * stream_state_size(n, w);
}

extern "C" int gdn_fleet_init(void* state, const float* history, long long h, int units, int n, int w, void* stream) {
  if (!state || !history) return GDN_ERR_ARG;
  if (units < 1 || units > GDN_FLEET_MAX_ROWS || !stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  if (h < w) return GDN_ERR_ARG;                   // a cold start: the caller buffers w ticks first
  const unsigned nw = (unsigned)n * (unsigned)w;
  const dim3 grid((nw + GDN_STREAM_SPAN - 1) / GDN_STREAM_SPAN, (unsigned)units);
  hipLaunchKernelGGL(gdn_fleet_init_kernel, grid, dim3(GDN_STREAM_THREADS), 0, (hipStream_t)stream, state, history, h,
                     n, w);
  return gdn_launch_status();
}

extern "C" int gdn_fleet_windows(const void* state, const float* chunk, const int32_t* counts, int units, int c, int n,
                                 int w, float* x_out, void* stream) {
  if (!state || !chunk || !counts || !x_out) return GDN_ERR_ARG;
  if (!gdn_fleet_rows_ok(units, c) || !stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  const unsigned nw = (unsigned)n * (unsigned)w;
  const dim3 grid((unsigned)c, (nw + GDN_STREAM_SPAN - 1) / GDN_STREAM_SPAN, (unsigned)units);
  hipLaunchKernelGGL(gdn_fleet_windows_kernel, grid, dim3(GDN_STREAM_THREADS), 0, (hipStream_t)stream, state, chunk,
                     counts, c, n, w, x_out);
  return gdn_launch_status();
}

// (w is not used by the arithmetic: it places unit u's state block)
extern "C" int gdn_fleet_score(const void* state, const float* pred, const float* chunk, const double* med_iqr,
                               const double* threshold, const int32_t* counts, int units, int c, int n, int w, int m,
                               double* top_scores, int32_t* top_sensors, int32_t* alarm, void* stream) {
  return fleet_score<false>(state, pred, chunk, nullptr, med_iqr, threshold, counts, units, c, n, w, m, top_scores,
                            top_sensors, alarm, stream);
}

extern "C" int gdn_fleet_advance(void* state, const float* chunk, const float* pred, const double* med_iqr,
                                 const int32_t* alarm, const int32_t* top_sensors, const int32_t* counts, int units,
                                 int c, int n, int w, int m, int64_t* log_ticks, int32_t* log_sensors,
                                 long long log_len, void* stream) {
  return fleet_advance<false>(state, chunk, pred, nullptr, nullptr, med_iqr, alarm, top_sensors, counts, units, c, n, w,
                              m, log_ticks, log_sensors, log_len, nullptr, stream);
}

// The workgroup shape follows c alone (known on the host, captured): up to DEPTH rows one wave walks them in one round
// of loads, up to 4 * DEPTH four waves do, beyond that the single stream's 16.  Every shape writes the same bits.
extern "C" int gdn_fleet_fill(const void* state, const float* raw_chunk, const int32_t* counts, int units, int c, int n,
                              int w, float* filled_chunk, uint8_t* valid, int32_t* gap_chunk, void* stream) {
  if (!state || !raw_chunk || !counts || !filled_chunk || !valid || !gap_chunk) return GDN_ERR_ARG;
  if (!gdn_fleet_rows_ok(units, c) || !stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  const hipStream_t s = (hipStream_t)stream;
  if (c <= GDN_FILL_DEPTH)
    fleet_fill_launch<1>(state, raw_chunk, counts, units, c, n, w, filled_chunk, valid, gap_chunk, s);
  else if (c <= 4 * GDN_FILL_DEPTH)
    fleet_fill_launch<4>(state, raw_chunk, counts, units, c, n, w, filled_chunk, valid, gap_chunk, s);
  else
    fleet_fill_launch<GDN_FILL_WAVES>(state, raw_chunk, counts, units, c, n, w, filled_chunk, valid, gap_chunk, s);
  return gdn_launch_status();
}

extern "C" int gdn_fleet_score_gaps(const void* state, const float* pred, const float* chunk, const uint8_t* valid,
                                    const double* med_iqr, const double* threshold, const int32_t* counts, int units,
                                    int c, int n, int w, int m, double* top_scores, int32_t* top_sensors,
                                    int32_t* alarm, void* stream) {
  return fleet_score<true>(state, pred, chunk, valid, med_iqr, threshold, counts, units, c, n, w, m, top_scores,
                           top_sensors, alarm, stream);
}

extern "C" int gdn_fleet_advance_gaps(void* state, const float* chunk, const float* pred, const uint8_t* valid,
                                      const int32_t* gap_chunk, const double* med_iqr, const int32_t* alarm,
                                      const int32_t* top_sensors, const int32_t* counts, int units, int c, int n,
                                      int w, int m, int64_t* log_ticks, int32_t* log_sensors, long long log_len,
                                      int64_t* gaps, void* stream) {
  return fleet_advance<true>(state, chunk, pred, valid, gap_chunk, med_iqr, alarm, top_sensors, counts, units, c, n, w,
                             m, log_ticks, log_sensors, log_len, gaps, stream);
}
