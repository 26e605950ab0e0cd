// The streaming detector (include/gdn_hip.h "streaming detector"): one device allocation holds the stream's state —
// tick / alarm / log counters, the float64 smoothing carry and the last w ticks of every sensor — and four launches
// make a push of 1 .. c ticks: cut the windows, (the model's forward,) score with the carried smoothing state,
// advance the state.  Only gdn_stream_advance writes the state; the other two read it, and stream order makes a push
// race-free.  Plain copy, sweep and scan kernels: no inline assembly, no floating-point atomics.
// Missing readings (opt-in, include/gdn_hip.h "Missing readings"): gdn_stream_fill leads the push and holds every
// non-finite reading at its sensor's latest real one; the score and advance kernels have a GAPS instantiation each that
// reads the validity plane and takes the normalised error of a missing reading as 0.0.  The plain instantiations are
// the kernels they were: the extra parameters trail the argument list and are never read.
// Rolling calibration (opt-in, include/gdn_hip.h "Rolling calibration"): gdn_stream_calib_write sits between the score
// and the advance launch and keeps |pred - gt| of the last R stream ticks in a ring that gdn_score_select reads as it
// stands; it reads the state and writes the ring only.
#include "gdn_stream_steps.hpp"

// (float64 scoring: gdn_score_sweep.hpp switches FMA contraction off for this unit)
// The window cut, the score of a run, the hist roll and the carry / log / counters are the __device__ steps of
// gdn_stream_steps.hpp, which the fleet kernels (gdn_fleet.hip) call too; the kernels here keep their launch shapes.

namespace {

using namespace gdn_stream_steps;

// hist = the last w columns of history[n, h]; counters and carry zero.  Lanes along the flat [i, w] index.
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_stream_init_kernel(
    void* __restrict__ state, const float* __restrict__ history, long long h, int n, int w) {
  stream_seed_span(state, history, h, n, w, blockIdx.x, threadIdx.x);
}

// Workgroup (b, span): elements [span * SPAN, (span + 1) * SPAN) of window b's flat [i, c] index.
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_stream_windows_kernel(
    const void* __restrict__ state, const float* __restrict__ chunk, int n, int w, float* __restrict__ x_out) {
  const int b = blockIdx.x;
  stream_window_span(state, chunk, n, w, b, blockIdx.y, threadIdx.x, x_out + (size_t)b * ((unsigned)n * (unsigned)w));
}

// Hold missing readings (stream_fill_group, gdn_stream_steps.hpp): workgroup g of GDN_FILL_WAVES waves owns sensors
// [64 g, 64 g + 64), each wave a contiguous segment of the chunk's rows.  Reads the state, writes none of it; no
// workgroup waits on another.
__global__ __launch_bounds__(GDN_FILL_WAVES * 64) void gdn_stream_fill_kernel(
    const void* __restrict__ state, const float* __restrict__ raw, int count, int n, int w,
    float* __restrict__ filled, unsigned char* __restrict__ valid, int* __restrict__ gap_chunk) {
  stream_fill_group<GDN_FILL_WAVES>(state, raw, count, n, w, filled, valid, gap_chunk, blockIdx.x, threadIdx.x);
}

// Normalise, smooth, top m, flag (stream_score_run): a wave per run of RUN ticks, grid-stride over the runs.
template <bool GAPS>
__global__ __launch_bounds__(256) void gdn_stream_score_kernel(
    const void* __restrict__ state, const float* __restrict__ pred, const float* __restrict__ gt,
    const double* __restrict__ med_iqr, const double* __restrict__ threshold, int t, int n, int m,
    double* __restrict__ top_scores, int* __restrict__ top_sensors, int* __restrict__ alarm,
    const unsigned char* __restrict__ valid) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int nruns = (t + RUN - 1) / RUN;
  const long long first_tick = reinterpret_cast<const long long*>(state)[0];
  const StreamSource src{pred, gt, valid, stream_carry(state), t, n};
  const double thr = threshold[0];
  for (int run = blockIdx.x * wpb + wv; run < nruns; run += gridDim.x * wpb)
    stream_score_run<GAPS>(src, med_iqr, thr, first_tick, run, lane, m, top_scores, top_sensors, alarm);
}

// The one launch that writes the state.  Workgroup i < n rolls row i of hist (stream_roll_row); workgroup n: the
// carry, the alarm log and, last, the counters (stream_carry_log).
// GAPS: `chunk` is the filled chunk; a carry entry taken from the chunk is 0.0 where valid says the reading was
// missing, and the push's gap_chunk [2, n] is folded into gaps [2, n] (missing_total, missing_run): this launch is the
// only writer of both.  Without GAPS the three trailing parameters are not read.
template <bool GAPS>
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_stream_advance_kernel(
    void* __restrict__ state, const float* __restrict__ chunk, const float* __restrict__ pred,
    const double* __restrict__ med_iqr, const int* __restrict__ alarm, const int* __restrict__ top_sensors, int count,
    int n, int w, int m, long long* __restrict__ log_ticks, int* __restrict__ log_sensors, long long log_len,
    const unsigned char* __restrict__ valid, const int* __restrict__ gap_chunk, long long* __restrict__ gaps) {
  if ((int)blockIdx.x < n) {
    stream_roll_row(state, chunk, count, n, w, blockIdx.x, threadIdx.x);
    return;
  }
  stream_carry_log<GAPS>(state, chunk, pred, med_iqr, alarm, top_sensors, count, n, m, log_ticks, log_sensors, log_len,
                         threadIdx.x, valid, gap_chunk, gaps);
}

// The calibration ring (include/gdn_hip.h "Rolling calibration"): row b < count of the push is stream tick
// ticks + b and owns slot (ticks + b) mod R of ring_keys [n, R] / ring_keep [R] (c <= R: no two rows of a push share
// a slot).  Workgroup g: rows [64 g, 64 g + 64) of the push through ring_write_tile (gdn_stream_steps.hpp), which
// states the keep rule and the key of each MODE (plain, gaps, per-sensor calibration) once, for a fleet's units too.
// Runs between the score launch (which wrote `alarm`) and the advance launch (`ticks` is still the push's first
// tick); reads the state, writes the ring only.
#define GDN_CALIB_MIN_R 64
#define GDN_CALIB_MAX_R (1 << 20)

template <int MODE>
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_stream_calib_write_kernel(
    const void* __restrict__ state, const float* __restrict__ pred, const float* __restrict__ chunk,
    const int* __restrict__ alarm, const unsigned char* __restrict__ valid, int count, int n, int R,
    int exclude_alarms, double* __restrict__ ring_keys, unsigned char* __restrict__ ring_keep) {
  const RingSource rs{pred, chunk, alarm, valid, ring_keys, ring_keep, ring_base(state, R)};
  ring_write_tile<MODE>(rs, blockIdx.x * 64, count, n, R, exclude_alarms, threadIdx.x);
}

bool calib_shape_ok(int n, int R) {
  return n >= 1 && n <= 4096 && R >= GDN_CALIB_MIN_R && R <= GDN_CALIB_MAX_R && 8ll * n * R <= (2ll << 30);
}

template <int MODE>
int calib_write(const void* state, const float* pred, const float* chunk, const int32_t* alarm, const uint8_t* valid,
                int c, int count, int n, int R, int exclude_alarms, double* ring_keys, uint8_t* ring_keep,
                void* stream) {
  if (!state || !pred || !chunk || !alarm || !ring_keys || !ring_keep || (MODE != CALIB_PLAIN && !valid))
    return GDN_ERR_ARG;
  if (count < 1 || count > c) return GDN_ERR_ARG;
  if (!calib_shape_ok(n, R)) return GDN_ERR_UNSUPPORTED;
  if (c > R) return GDN_ERR_ARG;                   // two rows of one push would share a slot
  hipLaunchKernelGGL(gdn_stream_calib_write_kernel<MODE>, dim3(((unsigned)count + 63) / 64), dim3(GDN_STREAM_THREADS),
                     0, (hipStream_t)stream, state, pred, chunk, alarm, valid, count, n, R, exclude_alarms, ring_keys,
                     ring_keep);
  return gdn_launch_status();
}

template <bool GAPS>
int stream_score(const void* state, const float* pred, const float* chunk, const uint8_t* valid, const double* med_iqr,
                 const double* threshold, int c, int count, int n, int m, double* top_scores, int32_t* top_sensors,
                 int32_t* alarm, void* stream) {
  if (!state || !pred || !chunk || (GAPS && !valid) || !med_iqr || !threshold || !top_scores || !top_sensors || !alarm ||
      count < 1 || count > c) return GDN_ERR_ARG;
  if (n < 1 || n > 4096) return GDN_ERR_UNSUPPORTED;
  if (m < 1 || m > TOPM_MAX || m > n) return GDN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gdn_stream_score_kernel<GAPS>, dim3(sweep_grid(count)), dim3(256), 0, (hipStream_t)stream, state, pred, chunk,
                     med_iqr, threshold, count, n, m, top_scores, top_sensors, alarm, valid);
  return gdn_launch_status();
}

template <bool GAPS>
int stream_advance(void* state, const float* chunk, const float* pred, const uint8_t* valid, const int32_t* gap_chunk,
                   const double* med_iqr, const int32_t* alarm, const int32_t* top_sensors, int c, int count, int n,
                   int w, int m, int64_t* log_ticks, int32_t* log_sensors, long long log_len, int64_t* gaps,
                   void* stream) {
  if (!state || !chunk || !pred || !med_iqr || !alarm || !top_sensors || (GAPS && (!valid || !gap_chunk || !gaps)))
    return GDN_ERR_ARG;
  if (count < 1 || count > c || log_len < 0 || (log_len > 0 && (!log_ticks || !log_sensors))) return GDN_ERR_ARG;
  if (!stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  if (m < 1 || m > TOPM_MAX || m > n) return GDN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gdn_stream_advance_kernel<GAPS>, dim3((unsigned)n + 1), dim3(GDN_STREAM_THREADS), 0,
                     (hipStream_t)stream, state, chunk, pred, med_iqr, alarm, top_sensors, count, n, w, m,
                     reinterpret_cast<long long*>(log_ticks), log_sensors, log_len, valid, gap_chunk,
                     reinterpret_cast<long long*>(gaps));
  return gdn_launch_status();
}

}  // namespace

extern "C" long long gdn_stream_calib_bytes(int n, int R) {
  if (!calib_shape_ok(n, R)) return 0;
  return (8ll * n * R + R + 7) & ~7ll;
}

extern "C" int gdn_stream_calib_write(const void* state, const float* pred, const float* chunk, const int32_t* alarm,
                                      int c, int count, int n, int R, int exclude_alarms, double* ring_keys,
                                      uint8_t* ring_keep, void* stream) {
  return calib_write<CALIB_PLAIN>(state, pred, chunk, alarm, nullptr, c, count, n, R, exclude_alarms, ring_keys,
                                  ring_keep, stream);
}

extern "C" int gdn_stream_calib_write_gaps(const void* state, const float* pred, const float* chunk,
                                           const int32_t* alarm, const uint8_t* valid, int c, int count, int n, int R,
                                           int exclude_alarms, double* ring_keys, uint8_t* ring_keep, void* stream) {
  return calib_write<CALIB_GAPS>(state, pred, chunk, alarm, valid, c, count, n, R, exclude_alarms, ring_keys,
                                 ring_keep, stream);
}

extern "C" int gdn_stream_calib_write_sensor(const void* state, const float* pred, const float* chunk,
                                             const int32_t* alarm, const uint8_t* valid, int c, int count, int n,
                                             int R, int exclude_alarms, double* ring_keys, uint8_t* ring_keep,
                                             void* stream) {
  return calib_write<CALIB_SENSOR>(state, pred, chunk, alarm, valid, c, count, n, R, exclude_alarms, ring_keys,
                                   ring_keep, stream);
}

extern "C" long long gdn_stream_state_bytes(int n, int w) {
  if (!stream_shape_ok(n, w)) return 0;
  return stream_state_size(n, w);
}

extern "C" int gdn_stream_init(void* state, const float* history, long long h, int n, int w, void* stream) {
  if (!state || !history) return GDN_ERR_ARG;
  if (!stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  if (h < w) return GDN_ERR_ARG;                   // a cold start: the caller buffers w ticks first
  const unsigned nw = (unsigned)n * (unsigned)w;
  hipLaunchKernelGGL(gdn_stream_init_kernel, dim3((nw + GDN_STREAM_SPAN - 1) / GDN_STREAM_SPAN),
                     dim3(GDN_STREAM_THREADS), 0, (hipStream_t)stream, state, history, h, n, w);
  return gdn_launch_status();
}

extern "C" int gdn_stream_windows(const void* state, const float* chunk, int c, int count, int n, int w, float* x_out,
                                  void* stream) {
  if (!state || !chunk || !x_out) return GDN_ERR_ARG;
  if (count < 1 || count > c) return GDN_ERR_ARG;
  if (!stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  const unsigned nw = (unsigned)n * (unsigned)w;
  const dim3 grid((unsigned)count, (nw + GDN_STREAM_SPAN - 1) / GDN_STREAM_SPAN);
  hipLaunchKernelGGL(gdn_stream_windows_kernel, grid, dim3(GDN_STREAM_THREADS), 0, (hipStream_t)stream, state, chunk, n,
                     w, x_out);
  return gdn_launch_status();
}

extern "C" int gdn_stream_score(const void* state, const float* pred, const float* chunk, const double* med_iqr,
                                const double* threshold, int c, int count, int n, int m, double* top_scores,
                                int32_t* top_sensors, int32_t* alarm, void* stream) {
  return stream_score<false>(state, pred, chunk, nullptr, med_iqr, threshold, c, count, n, m, top_scores, top_sensors,
                             alarm, stream);
}

extern "C" int gdn_stream_advance(void* state, const float* chunk, const float* pred, const double* med_iqr,
                                  const int32_t* alarm, const int32_t* top_sensors, int c, int count, int n, int w,
                                  int m, int64_t* log_ticks, int32_t* log_sensors, long long log_len, void* stream) {
  return stream_advance<false>(state, chunk, pred, nullptr, nullptr, med_iqr, alarm, top_sensors, c, count, n, w, m,
                               log_ticks, log_sensors, log_len, nullptr, stream);
}

extern "C" int gdn_stream_fill(const void* state, const float* raw_chunk, int c, int count, int n, int w,
                               float* filled_chunk, uint8_t* valid, int32_t* gap_chunk, void* stream) {
  if (!state || !raw_chunk || !filled_chunk || !valid || !gap_chunk) return GDN_ERR_ARG;
  if (count < 1 || count > c) return GDN_ERR_ARG;
  if (!stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gdn_stream_fill_kernel, dim3(((unsigned)n + 63) / 64), dim3(GDN_FILL_WAVES * 64), 0,
                     (hipStream_t)stream, state, raw_chunk, count, n, w, filled_chunk, valid, gap_chunk);
  return gdn_launch_status();
}

extern "C" int gdn_stream_score_gaps(const void* state, const float* pred, const float* chunk, const uint8_t* valid,
                                     const double* med_iqr, const double* threshold, int c, int count, int n, int m,
                                     double* top_scores, int32_t* top_sensors, int32_t* alarm, void* stream) {
  return stream_score<true>(state, pred, chunk, valid, med_iqr, threshold, c, count, n, m, top_scores, top_sensors,
                            alarm, stream);
}

extern "C" int gdn_stream_advance_gaps(void* state, const float* chunk, const float* pred, const uint8_t* valid,
                                       const int32_t* gap_chunk, const double* med_iqr, const int32_t* alarm,
                                       const int32_t* top_sensors, int c, int count, int n, int w, int m,
                                       int64_t* log_ticks, int32_t* log_sensors, long long log_len, int64_t* gaps,
                                       void* stream) {
  return stream_advance<true>(state, chunk, pred, valid, gap_chunk, med_iqr, alarm, top_sensors, c, count, n, w, m,
                              log_ticks, log_sensors, log_len, gaps, stream);
}
