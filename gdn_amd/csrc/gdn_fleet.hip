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
// Rolling calibration (opt-in): gdn_fleet_calib_write* sits between the score and the advance launch and
// writes a single stream's calibration ring per unit; gdn_fleet_ring_counts turns the keep flags into the per-row
// counts of gdn_score_select_counts, so a fleet recalibrates with no host read.  gdn_fleet_ring_threshold (opt-in,
// DESIGN §3.8l) re-derives every unit's threshold from its ring under the table just written; a single stream calls it
// with units = 1.
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

// The calibration rings of a fleet (include/gdn_hip.h "Rolling calibration of a fleet"): ring_keys [U, n, R] float64,
// ring_keep [U, R] uint8, unit u's slices a single stream's ring.  Row b < counts[u] of unit u is that unit's stream
// tick ticks_u + b and owns slot (ticks_u + b) mod R of the unit's ring.  The keep rule and the key of each MODE
// (CALIB_PLAIN / _GAPS / _SENSOR) and the tile step are gdn_stream_steps.hpp's, the ones gdn_stream_calib_write /
// _gaps / _sensor run: a kernel here only says which unit's rows, ring and count.
// Reads the states, writes the rings only; a unit with counts[u] == 0 has no byte of its ring touched.
#define GDN_FLEET_CALIB_TILE_C 64    // from this many rows per unit on, the transposing tile form

__device__ __forceinline__ RingSource fleet_ring(const void* state, const float* pred, const float* chunk,
                                                 const int* alarm, const unsigned char* valid, int u, int c, int n,
                                                 int w, int R, double* ring_keys, unsigned char* ring_keep) {
  const size_t row0 = (size_t)u * c;
  return RingSource{pred + row0 * n, chunk + row0 * n, alarm + row0, valid ? valid + row0 * n : nullptr,
                    ring_keys + (size_t)u * n * R, ring_keep + (size_t)u * R,
                    ring_base(fleet_state(state, u, n, w), R)};
}

// The direct form (small c): one wave per (unit, row), lanes along the sensors, every lane stores its key at
// ring_keys[u][s][slot].  8-byte stores at stride 8 R: as uncoalesced as the tile form's at c of 1 to a few rows (one
// slot per sensor row either way), but every lane of the wave carries one, and there is no LDS and no barrier.
template <int MODE>
__global__ __launch_bounds__(256) void gdn_fleet_calib_direct_kernel(
    const void* __restrict__ state, const float* __restrict__ pred, const float* __restrict__ chunk,
    const int* __restrict__ alarm, const unsigned char* __restrict__ valid, const int* __restrict__ counts, int units,
    int c, int n, int w, int R, int exclude_alarms, double* __restrict__ ring_keys,
    unsigned char* __restrict__ ring_keep) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int at = blockIdx.x * (blockDim.x >> 6) + wv;        // (wave uniform) <= 4096 + 3
  const int u = at / c, b = at - u * c;
  if (u >= units || b >= fleet_count(counts, u, c)) return;
  const RingSource rs = fleet_ring(state, pred, chunk, alarm, valid, u, c, n, w, R, ring_keys, ring_keep);
  const unsigned slot = calib_slot(rs.base, b, R);
  const bool keep = ring_keep_row<MODE>(rs, b, n, exclude_alarms, lane);
  if (lane == 0) rs.keep[slot] = keep ? 1 : 0;
  for (int s = lane; s < n; s += 64)
    rs.keys[(size_t)s * R + slot] = ring_key<MODE>(rs, (size_t)b * n + s, keep);
}

// The tile form, workgroup (row tile g, unit): the single stream's workgroup g on unit u's rows with count = counts[u]
// (ring_write_tile, the step that workgroup runs).
template <int MODE>
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_fleet_calib_tile_kernel(
    const void* __restrict__ state, const float* __restrict__ pred, const float* __restrict__ chunk,
    const int* __restrict__ alarm, const unsigned char* __restrict__ valid, const int* __restrict__ counts, int c,
    int n, int w, int R, int exclude_alarms, double* __restrict__ ring_keys, unsigned char* __restrict__ ring_keep) {
  const int u = blockIdx.y, b0 = blockIdx.x * 64;
  const int count = fleet_count(counts, u, c);
  if (b0 >= count) return;                                   // (workgroup uniform, ahead of every barrier)
  const RingSource rs = fleet_ring(state, pred, chunk, alarm, valid, u, c, n, w, R, ring_keys, ring_keep);
  ring_write_tile<MODE>(rs, b0, count, n, R, exclude_alarms, threadIdx.x);
}

// Workgroup u, tick mode: kept[u] = the sum of unit u's keep flags (integer adds: any order gives the same number),
// broadcast into counts[u n .. u n + n).  A unit with select[u] == 0 gets counts 0 and keeps kept[u].
__global__ __launch_bounds__(256) void gdn_fleet_ring_counts_kernel(
    const unsigned char* __restrict__ ring_keep, const unsigned char* __restrict__ select, int n, int R,
    int* __restrict__ counts, int* __restrict__ kept) {
  __shared__ int wave_sum[4];
  const int u = blockIdx.x, tid = threadIdx.x;
  int* __restrict__ cu = counts + (size_t)u * n;
  if (select && select[u] == 0) {                            // (workgroup uniform, ahead of the barrier)
    for (int s = tid; s < n; s += 256) cu[s] = 0;
    return;
  }
  const unsigned char* __restrict__ ku = ring_keep + (size_t)u * R;
  int sum = 0;
  for (int i = tid; i < R; i += 256) sum += ku[i] != 0 ? 1 : 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = sum;
  __syncthreads();
  const int total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
  for (int s = tid; s < n; s += 256) cu[s] = total;
  if (tid == 0) kept[u] = total;
}

// Sensor mode: counts [U n] is gdn_score_key_counts' over the rings; the rows of a unit with select[u] == 0 become 0.
__global__ __launch_bounds__(256) void gdn_fleet_counts_mask_kernel(const unsigned char* __restrict__ select, int n,
                                                                    long long rows, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < rows && select[i / n] == 0) counts[i] = 0;
}

// The threshold from the rings (include/gdn_hip.h "Threshold from the ring").  Two launches, no atomics,
// no workgroup waits on another: the tile kernel leaves one RingPeak per (unit, tile of 61 slots) in the workspace
// [U, ring_tiles(R)], the finisher folds a unit's row and applies the rule.  A single stream is the fleet of one unit.
// Wave (unit u, tile t): ring_peak_tile, the step of gdn_stream_steps.hpp, on unit u's ring, table and base.
template <int MODE>
__global__ __launch_bounds__(256) void gdn_fleet_ring_peak_kernel(
    const void* __restrict__ state, const double* __restrict__ ring_keys, const unsigned char* __restrict__ ring_keep,
    const double* __restrict__ med_iqr, int n, int w, int R, RingPeak* __restrict__ partials) {
  const int lane = threadIdx.x & 63, u = blockIdx.y, tiles = ring_tiles(R);
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);         // (wave uniform)
  if (t >= tiles) return;
  const RingPeak p = ring_peak_tile<MODE>(ring_keys + (size_t)u * n * R, ring_keep + (size_t)u * R,
                                          med_iqr + (size_t)u * n * 2, ring_base(fleet_state(state, u, n, w), R), n, R,
                                          t, lane);
  if (lane == 0) partials[(size_t)u * tiles + t] = p;
}

// Workgroup u: the maximum (ties by slot) and the eligible sum of the unit's partials, then the rule: the threshold is
// rewritten as peak * margin (ONE multiply) iff the unit is selected, eligible >= min_eligible and peak is finite and
// > 0; with episodes, clear = the new threshold * clear_frac in the same step.  peak, eligible and peak_slot (-1: no
// eligible slot) are written either way.
__global__ __launch_bounds__(256) void gdn_fleet_ring_threshold_kernel(
    const RingPeak* __restrict__ partials, const unsigned char* __restrict__ select, int tiles, double margin,
    int min_eligible, double* __restrict__ threshold, const double* __restrict__ clear_frac,
    double* __restrict__ clear, double* __restrict__ peak, int* __restrict__ eligible, int* __restrict__ peak_slot) {
  __shared__ RingPeak wave_part[4];
  const int u = blockIdx.x, tid = threadIdx.x;
  const RingPeak* __restrict__ row = partials + (size_t)u * tiles;
  RingPeak acc{-INFINITY, NONE, 0};
  for (int t = tid; t < tiles; t += 256) {
    const RingPeak p = row[t];
    ring_peak_merge(acc.peak, acc.slot, p.peak, p.slot);
    acc.eligible += p.eligible;
  }
  ring_peak_wave(acc.peak, acc.slot);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc.eligible += __shfl_xor(acc.eligible, d);
  if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
  __syncthreads();
  if (tid != 0) return;
  for (int v = 1; v < 4; ++v) {
    ring_peak_merge(acc.peak, acc.slot, wave_part[v].peak, wave_part[v].slot);
    acc.eligible += wave_part[v].eligible;
  }
  peak[u] = acc.peak;
  eligible[u] = acc.eligible;
  peak_slot[u] = acc.slot == NONE ? -1 : acc.slot;
  const bool selected = !select || select[u] != 0;
  if (selected && acc.eligible >= min_eligible && acc.peak > 0.0 && acc.peak < INFINITY) {
    const double thr = acc.peak * margin;
    threshold[u] = thr;
    if (clear) clear[u] = thr * clear_frac[u];
  }
}

template <int MODE>
void fleet_ring_peak_launch(const void* state, const double* ring_keys, const uint8_t* ring_keep,
                            const double* med_iqr, int units, int n, int w, int R, RingPeak* partials, hipStream_t s) {
  const unsigned tiles = (unsigned)ring_tiles(R);            // <= 17190
  hipLaunchKernelGGL(gdn_fleet_ring_peak_kernel<MODE>, dim3((tiles + 3) / 4, (unsigned)units), dim3(256), 0, s, state,
                     ring_keys, ring_keep, med_iqr, n, w, R, partials);
}

// diagnostic knob: GDN_FLEET_CALIB_TILE=1 keeps the ring write on the tile form at every c (comparisons)
bool force_calib_tile() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("GDN_FLEET_CALIB_TILE");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}

// The form follows c alone (known on the host, captured), never counts; both forms write the same bytes.
template <int MODE>
int fleet_calib_write(const void* state, const float* pred, const float* chunk, const int32_t* alarm,
                      const uint8_t* valid, const int32_t* counts, int units, int c, int n, int w, int R,
                      int exclude_alarms, double* ring_keys, uint8_t* ring_keep, void* stream) {
  if (!state || !pred || !chunk || !alarm || !counts || !ring_keys || !ring_keep || (MODE != CALIB_PLAIN && !valid))
    return GDN_ERR_ARG;
  if (!gdn_fleet_rows_ok(units, c) || !stream_shape_ok(n, w)) return GDN_ERR_UNSUPPORTED;
  if (gdn_fleet_calib_bytes(units, n, R) <= 0) return GDN_ERR_UNSUPPORTED;
  if (c > R) return GDN_ERR_ARG;                   // two rows of one push would share a slot
  const hipStream_t s = (hipStream_t)stream;
  if (c < GDN_FLEET_CALIB_TILE_C && !force_calib_tile()) {
    const unsigned waves = (unsigned)units * (unsigned)c;                            // <= 4096
    hipLaunchKernelGGL(gdn_fleet_calib_direct_kernel<MODE>, dim3((waves + 3) / 4), dim3(256), 0, s, state, pred, chunk,
                       alarm, valid, counts, units, c, n, w, R, exclude_alarms, ring_keys, ring_keep);
  } else {
    hipLaunchKernelGGL(gdn_fleet_calib_tile_kernel<MODE>, dim3(((unsigned)c + 63) / 64, (unsigned)units),
                       dim3(GDN_STREAM_THREADS), 0, s, state, pred, chunk, alarm, valid, counts, c, n, w, R,
                       exclude_alarms, ring_keys, ring_keep);
  }
  return gdn_launch_status();
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

// units x the single stream's ring, keys of all units first ([U, n, R] float64), then the keep flags ([U, R] uint8).
extern "C" long long gdn_fleet_calib_bytes(int units, int n, int R) {
  const long long one = gdn_stream_calib_bytes(n, R);        // 0: outside the single stream's limits
  if (one <= 0 || units < 1 || units > GDN_FLEET_MAX_ROWS || 8ll * units * n * R > (2ll << 30)) return 0;
  return (long long)units * one;
}

extern "C" int gdn_fleet_calib_write(const void* state, const float* pred, const float* chunk, const int32_t* alarm,
                                     const int32_t* counts, int units, int c, int n, int w, int R, int exclude_alarms,
                                     double* ring_keys, uint8_t* ring_keep, void* stream) {
  return fleet_calib_write<CALIB_PLAIN>(state, pred, chunk, alarm, nullptr, counts, units, c, n, w, R, exclude_alarms,
                                        ring_keys, ring_keep, stream);
}

extern "C" int gdn_fleet_calib_write_gaps(const void* state, const float* pred, const float* chunk,
                                          const int32_t* alarm, const uint8_t* valid, const int32_t* counts, int units,
                                          int c, int n, int w, int R, int exclude_alarms, double* ring_keys,
                                          uint8_t* ring_keep, void* stream) {
  return fleet_calib_write<CALIB_GAPS>(state, pred, chunk, alarm, valid, counts, units, c, n, w, R, exclude_alarms,
                                       ring_keys, ring_keep, stream);
}

extern "C" int gdn_fleet_calib_write_sensor(const void* state, const float* pred, const float* chunk,
                                            const int32_t* alarm, const uint8_t* valid, const int32_t* counts,
                                            int units, int c, int n, int w, int R, int exclude_alarms,
                                            double* ring_keys, uint8_t* ring_keep, void* stream) {
  return fleet_calib_write<CALIB_SENSOR>(state, pred, chunk, alarm, valid, counts, units, c, n, w, R, exclude_alarms,
                                         ring_keys, ring_keep, stream);
}

// ring_keep != NULL (tick mode): the keep sums into kept [U] and counts [U n].  ring_keep == NULL (sensor mode): counts
// holds gdn_score_key_counts' numbers and only the mask is applied (select == NULL: nothing to do, no launch).
extern "C" int gdn_fleet_ring_counts(const uint8_t* ring_keep, const uint8_t* select, int units, int n, int R,
                                     int32_t* counts, int32_t* kept, void* stream) {
  if (!counts || (ring_keep && !kept)) return GDN_ERR_ARG;
  if (gdn_fleet_calib_bytes(units, n, R) <= 0) return GDN_ERR_UNSUPPORTED;
  if (ring_keep) {
    hipLaunchKernelGGL(gdn_fleet_ring_counts_kernel, dim3((unsigned)units), dim3(256), 0, (hipStream_t)stream,
                       ring_keep, select, n, R, counts, kept);
  } else if (select) {
    const long long rows = (long long)units * n;             // <= 2^24
    hipLaunchKernelGGL(gdn_fleet_counts_mask_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, select, n, rows, counts);
  } else {
    return GDN_OK;
  }
  return gdn_launch_status();
}

// One RingPeak (16 bytes) per unit and tile of 61 slots.
extern "C" long long gdn_fleet_ring_threshold_bytes(int units, int R) {
  if (gdn_fleet_calib_bytes(units, 1, R) <= 0) return 0;
  return (long long)sizeof(RingPeak) * units * ring_tiles(R);
}

// mode: the CALIB_* of the ring's writer (PLAIN and GAPS are tick calibration: no filler test; SENSOR has it).
extern "C" int gdn_fleet_ring_threshold(const void* state, const double* ring_keys, const uint8_t* ring_keep,
                                        const double* med_iqr, const uint8_t* select, int units, int n, int w, int R,
                                        int mode, double margin, int min_eligible, void* workspace, double* threshold,
                                        const double* clear_frac, double* clear, double* peak, int32_t* eligible,
                                        int32_t* peak_slot, void* stream) {
  if (!state || !ring_keys || !ring_keep || !med_iqr || !workspace || !threshold || !peak || !eligible || !peak_slot ||
      (clear_frac == nullptr) != (clear == nullptr))
    return GDN_ERR_ARG;
  if (!(margin > 0.0 && margin < INFINITY) || min_eligible < 1) return GDN_ERR_ARG;       // (a NaN margin compares false)
  if (mode != CALIB_PLAIN && mode != CALIB_GAPS && mode != CALIB_SENSOR) return GDN_ERR_ARG;
  if (!stream_shape_ok(n, w) || gdn_fleet_calib_bytes(units, n, R) <= 0) return GDN_ERR_UNSUPPORTED;
  const hipStream_t s = (hipStream_t)stream;
  RingPeak* partials = reinterpret_cast<RingPeak*>(workspace);
  if (mode == CALIB_SENSOR)
    fleet_ring_peak_launch<CALIB_SENSOR>(state, ring_keys, ring_keep, med_iqr, units, n, w, R, partials, s);
  else
    fleet_ring_peak_launch<CALIB_PLAIN>(state, ring_keys, ring_keep, med_iqr, units, n, w, R, partials, s);
  hipLaunchKernelGGL(gdn_fleet_ring_threshold_kernel, dim3((unsigned)units), dim3(256), 0, s, partials, select,
                     ring_tiles(R), margin, min_eligible, threshold, clear_frac, clear, peak, eligible, peak_slot);
  return gdn_launch_status();
}
