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
#include "gdn_score_sweep.hpp"

// (float64 scoring: gdn_score_sweep.hpp switches FMA contraction off for this unit)

namespace {

using namespace gdn_sweep;

#define GDN_STREAM_HEADER 4          // int64 words ahead of the carry: ticks, alarms, logged, (reserved)
#define GDN_STREAM_THREADS 256
#define GDN_STREAM_PER_THREAD 4      // flat elements per thread, GDN_STREAM_THREADS apart (gdn_windows_gather's shape)
#define GDN_STREAM_SPAN (GDN_STREAM_THREADS * GDN_STREAM_PER_THREAD)

__host__ __device__ inline const double* stream_carry(const void* state) {
  return reinterpret_cast<const double*>(state) + GDN_STREAM_HEADER;
}
__host__ __device__ inline double* stream_carry(void* state) {
  return reinterpret_cast<double*>(state) + GDN_STREAM_HEADER;
}
__host__ __device__ inline const float* stream_hist(const void* state, int n) {
  return reinterpret_cast<const float*>(stream_carry(state) + 3 * (size_t)n);
}
__host__ __device__ inline float* stream_hist(void* state, int n) {
  return reinterpret_cast<float*>(stream_carry(state) + 3 * (size_t)n);
}

// hist = the last w columns of history[n, h]; counters and carry zero.  Lanes along the flat [i, w] index.
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_stream_init_kernel(
    void* __restrict__ state, const float* __restrict__ history, long long h, int n, int w) {
  const unsigned nw = (unsigned)n * (unsigned)w;
  const unsigned f0 = blockIdx.x * GDN_STREAM_SPAN + threadIdx.x;
  float* __restrict__ hist = stream_hist(state, n);
#pragma unroll
  for (int j = 0; j < GDN_STREAM_PER_THREAD; ++j) {
    const unsigned f = f0 + j * GDN_STREAM_THREADS;
    if (f >= nw) break;
    const unsigned i = f / (unsigned)w, c = f - i * (unsigned)w;
    hist[f] = history[(long long)i * h + (h - w) + c];
  }
  if (blockIdx.x == 0) {
    long long* __restrict__ head = reinterpret_cast<long long*>(state);
    double* __restrict__ carry = stream_carry(state);
    if (threadIdx.x < GDN_STREAM_HEADER) head[threadIdx.x] = 0;
    for (int f = threadIdx.x; f < 3 * n; f += GDN_STREAM_THREADS) carry[f] = 0.0;
  }
}

// Workgroup (b, span): elements [span * SPAN, (span + 1) * SPAN) of window b's flat [i, c] index: the w values of
// sensor i before tick b of the chunk.  Position b - w + c of the stream relative to the chunk's first tick: negative
// = column w + (b - w + c) = b + c of hist, else that row of the (time-major) chunk.
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_stream_windows_kernel(
    const void* __restrict__ state, const float* __restrict__ chunk, int n, int w, float* __restrict__ x_out) {
  const int b = blockIdx.x;
  const unsigned nw = (unsigned)n * (unsigned)w;     // <= 4096 * 1024
  const float* __restrict__ hist = stream_hist(state, n);
  float* __restrict__ xb = x_out + (size_t)b * nw;
  const unsigned f0 = blockIdx.y * GDN_STREAM_SPAN + threadIdx.x;
#pragma unroll
  for (int j = 0; j < GDN_STREAM_PER_THREAD; ++j) {
    const unsigned f = f0 + j * GDN_STREAM_THREADS;
    if (f >= nw) break;
    const unsigned i = f / (unsigned)w, c = f - i * (unsigned)w;
    const int pos = b - w + (int)c;
    xb[f] = pos < 0 ? hist[(size_t)i * w + (unsigned)(b + (int)c)] : chunk[(size_t)pos * n + i];
  }
}

// Hold missing readings.  "Missing" is decided on the bit pattern (exponent field all ones: NaN, +inf, -inf), so it
// does not depend on how floating-point comparisons with NaN are compiled.
#define GDN_FILL_WAVES 16            // waves of a workgroup: each owns a contiguous segment of the chunk's rows
#define GDN_FILL_DEPTH 8             // row loads in flight per lane
__device__ inline bool stream_missing(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// Workgroup g: sensors [64 g, 64 g + 64), one per lane (a row of the time-major chunk is contiguous along sensors:
// coalesced).  Wave v walks rows [v * seg, (v + 1) * seg) ^ [0, count), DEPTH loads at a time, and reduces them to
// (latest real reading, found one, missing readings, missing readings after the latest real one = the whole segment
// when there is none).  "The right-most real reading wins" is associative: the segments meet in LDS, every wave takes
// the latest real reading before its segment (hist[i, w - 1] when no earlier segment has one) and walks its rows a
// second time, writing.  Wave 0 folds the counts.  Reads the state, writes none of it; no workgroup waits on another.
__global__ __launch_bounds__(GDN_FILL_WAVES * 64) void gdn_stream_fill_kernel(
    const void* __restrict__ state, const float* __restrict__ raw, int count, int n, int w,
    float* __restrict__ filled, unsigned char* __restrict__ valid, int* __restrict__ gap_chunk) {
  __shared__ float seg_last[GDN_FILL_WAVES][64];
  __shared__ int seg_found[GDN_FILL_WAVES][64];
  __shared__ int seg_missing[GDN_FILL_WAVES][64];
  __shared__ int seg_trail[GDN_FILL_WAVES][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < n;
  const int ic = live ? i : n - 1;                                   // a dead lane reads sensor n - 1, writes nothing
  const int seg = (count + GDN_FILL_WAVES - 1) / GDN_FILL_WAVES;
  const int r0 = min(count, wv * seg), r1 = min(count, r0 + seg);
  float last = 0.f;
  int found = 0, missing = 0, trail = 0;
  for (int b = r0; b < r1; b += GDN_FILL_DEPTH) {
    float v[GDN_FILL_DEPTH];
#pragma unroll
    for (int u = 0; u < GDN_FILL_DEPTH; ++u) v[u] = raw[(size_t)min(b + u, r1 - 1) * n + ic];
#pragma unroll
    for (int u = 0; u < GDN_FILL_DEPTH; ++u) {
      if (b + u < r1) {                                              // (wave uniform)
        if (stream_missing(v[u])) { ++missing; ++trail; }
        else { last = v[u]; found = 1; trail = 0; }
      }
    }
  }
  seg_last[wv][lane] = last;
  seg_found[wv][lane] = found;
  seg_missing[wv][lane] = missing;
  seg_trail[wv][lane] = trail;
  __syncthreads();
  float hold = stream_hist(state, n)[(size_t)ic * w + (w - 1)];
  for (int v = 0; v < wv; ++v)
    if (seg_found[v][lane]) hold = seg_last[v][lane];
  for (int b = r0; b < r1; b += GDN_FILL_DEPTH) {
    float v[GDN_FILL_DEPTH];
#pragma unroll
    for (int u = 0; u < GDN_FILL_DEPTH; ++u) v[u] = raw[(size_t)min(b + u, r1 - 1) * n + ic];
#pragma unroll
    for (int u = 0; u < GDN_FILL_DEPTH; ++u) {
      if (b + u < r1) {
        const bool gone = stream_missing(v[u]);
        if (!gone) hold = v[u];
        if (live) {
          filled[(size_t)(b + u) * n + i] = hold;
          valid[(size_t)(b + u) * n + i] = gone ? 0 : 1;
        }
      }
    }
  }
  if (wv == 0 && live) {
    int total = 0, run = 0;
    for (int v = 0; v < GDN_FILL_WAVES; ++v) total += seg_missing[v][lane];
    for (int v = GDN_FILL_WAVES - 1; v >= 0; --v) {                  // from the last row back to the latest real reading
      run += seg_trail[v][lane];
      if (seg_found[v][lane]) break;
    }
    gap_chunk[i] = total;
    gap_chunk[n + i] = run;
  }
}

// Normalise, smooth, top m, flag: the sweep of gdn_score_sweep.hpp with top-m lists, as score_smooth_topm_kernel
// (gdn_score.hip) runs it, over a push.  Here: the series position of the chunk's first tick is read from the state,
// and only the run at tick 0 reaches back: its three predecessors are the carry (rows 0, 1, 2 = three, two, one tick
// before; zeros where the series has no such tick, GAPS: 0.0 for a missing reading, through gdn_stream_advance).

// Rows before the chunk are never used as values (row 0 stands in for the loads); rows past it are clamped.
struct StreamSource {
  const float *pred, *gt;
  const unsigned char* valid;
  const double* carry;
  int t, n;
  __device__ __forceinline__ size_t at(int tt) const { return (size_t)(tt < 0 ? 0 : min(tt, t - 1)) * n; }
  __device__ __forceinline__ const float* pred_row(int tt) const { return pred + at(tt); }
  __device__ __forceinline__ const float* gt_row(int tt) const { return gt + at(tt); }
  __device__ __forceinline__ const unsigned char* valid_row(int tt) const { return valid + at(tt); }
  template <typename FA, typename FB>
  __device__ __forceinline__ void before(int t0, const Lanes& l, double (&a)[3], double (&b)[3], FA&& na,
                                         FB&& nb) const {
    if (t0 == 0) {                                 // (wave uniform) all six loads in one block: one round trip
      a[0] = carry[l.ca]; a[1] = carry[(size_t)n + l.ca]; a[2] = carry[2 * (size_t)n + l.ca];
      b[0] = carry[l.cb]; b[1] = carry[(size_t)n + l.cb]; b[2] = carry[2 * (size_t)n + l.cb];
    } else {
      a[0] = na(0); a[1] = na(1); a[2] = na(2);
      b[0] = nb(0); b[1] = nb(1); b[2] = nb(2);
    }
  }
};

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
  for (int run = blockIdx.x * wpb + wv; run < nruns; run += gridDim.x * wpb) {
    const int t0 = run * RUN, t1 = min(t, t0 + RUN);
    double cs[RUN];                               // the carried list: entry `lane` of every tick of the run
    int ci[RUN];
#pragma unroll
    for (int u = 0; u < RUN; ++u) {
      cs[u] = -INFINITY;
      ci[u] = NONE;
    }
    for (int s0 = 0; s0 < n; s0 += 128) {
      const Lanes l(s0, lane, n);
      score_sweep<GAPS>(src, med_iqr, l, t0, t1, first_tick, [&](int u, int, double sma, double smb) {
        topm_merge(l, lane, m, sma, smb, cs[u], ci[u]);
      });
    }
    topm_store(cs, ci, lane, m, t0, t1, top_scores, top_sensors);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < RUN; ++u)
        if (t0 + u < t1) alarm[t0 + u] = cs[u] > thr ? 1 : 0;      // strict; a NaN score compares false
    }
  }
}

// The one launch that writes the state.  Workgroup i < n rolls row i of hist: every thread loads its (up to 4)
// columns of the NEW row — from the old row where the column survives, else from the chunk — then a barrier, then the
// stores: no column is read after it has been overwritten, whatever count is.  Workgroup n: the carry (one thread per
// sensor: its three old entries are read before any is written), the alarm log (an ordered compaction: ballot and
// popcount inside a wave, four wave totals through LDS, 256 flags a round in tick order) and, last, the counters.
// GAPS: `chunk` is the filled chunk; a carry entry taken from the chunk is 0.0 where valid says the reading was
// missing, and the carry thread of sensor s folds the push's gap_chunk [2, n] into gaps [2, n] (missing_total,
// missing_run): this launch is the only writer of both.  Without GAPS the three trailing parameters are not read.
template <bool GAPS>
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_stream_advance_kernel(
    void* __restrict__ state, const float* __restrict__ chunk, const float* __restrict__ pred,
    const double* __restrict__ med_iqr, const int* __restrict__ alarm, const int* __restrict__ top_sensors, int count,
    int n, int w, int m, long long* __restrict__ log_ticks, int* __restrict__ log_sensors, long long log_len,
    const unsigned char* __restrict__ valid, const int* __restrict__ gap_chunk, long long* __restrict__ gaps) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < n) {
    const int i = blockIdx.x;
    float* __restrict__ row = stream_hist(state, n) + (size_t)i * w;
    float v[GDN_STREAM_PER_THREAD];
#pragma unroll
    for (int j = 0; j < GDN_STREAM_PER_THREAD; ++j) {
      const int c = tid + j * GDN_STREAM_THREADS;             // w <= 1024 = PER_THREAD * THREADS
      v[j] = 0.f;
      if (c < w) {
        const long long src = (long long)c + count;           // column of [hist | chunk^T]
        v[j] = src < w ? row[src] : chunk[(size_t)(src - w) * n + i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < GDN_STREAM_PER_THREAD; ++j) {
      const int c = tid + j * GDN_STREAM_THREADS;
      if (c < w) row[c] = v[j];
    }
    return;
  }
  __shared__ int wave_total[GDN_STREAM_THREADS / 64];
  long long* __restrict__ head = reinterpret_cast<long long*>(state);
  double* __restrict__ carry = stream_carry(state);
  // carry: the last three of [carry0, carry1, carry2, a(chunk row 0), .., a(chunk row count - 1)]
  for (int s = tid; s < n; s += GDN_STREAM_THREADS) {
    const Scale sc = sensor_scale(med_iqr, s);
    double next[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int q = count + j;                                 // position in the 3 + count values above
      if (q < 3) {
        next[j] = carry[(size_t)q * n + s];
      } else {
        const size_t at = (size_t)(q - 3) * n + s;
        unsigned ok = 0u;
        if constexpr (GAPS) ok = valid[at] ? 1u : 0u;
        next[j] = norm<GAPS>(pred[at], chunk[at], sc.med, sc.inv_den, ok, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) carry[(size_t)j * n + s] = next[j];
    if constexpr (GAPS) {
      const int trail = gap_chunk[n + s];
      gaps[s] += gap_chunk[s];
      gaps[(size_t)n + s] = trail == count ? gaps[(size_t)n + s] + count : trail;
    }
  }
  // alarm log
  const long long ticks = head[0], logged = head[2];
  const int lane = tid & 63, wv = tid >> 6;
  long long raised = 0;                                        // flags in the rounds before this one
  for (int base = 0; base < count; base += GDN_STREAM_THREADS) {
    const int b = base + tid;
    const bool flag = b < count && alarm[b] != 0;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) wave_total[wv] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int v = 0; v < GDN_STREAM_THREADS / 64; ++v) {
      if (v < wv) before += wave_total[v];
      total += wave_total[v];
    }
    __syncthreads();                                           // wave_total is rewritten next round
    const long long slot = logged + raised + before;
    if (flag && slot < log_len) {
      log_ticks[slot] = ticks + b;
      for (int r = 0; r < m; ++r) log_sensors[slot * m + r] = top_sensors[(size_t)b * m + r];
    }
    raised += total;
  }
  if (tid == 0) {
    head[0] = ticks + count;
    head[1] += raised;
    const long long want = logged + raised, room = log_len > logged ? log_len : logged;
    head[2] = want < room ? want : room;                       // a full log drops entries; `alarms` keeps counting
  }
}

// The calibration ring (include/gdn_hip.h "Rolling calibration"): row b < count of the push is stream tick
// ticks + b and owns slot (ticks + b) mod R of ring_keys [n, R] / ring_keep [R].  A kept tick writes its n keys
// score_key(pred, chunk) and keep = 1; a tick that is not kept (its
// alarm flag under exclude_alarms; GAPS: a missing reading in any sensor) writes the filler into all n keys and
// keep = 0, so no older tick survives in its slot.  Workgroup g: rows [64 g, 64 g + 64) of the push, sensor tiles of
// 64 transposed through the padded LDS tile of score_keys_kernel: fp32 reads along sensors, fp64 writes along slots.
// The slot is computed per row: a tile may wrap the ring's end once (c <= R: no two rows of a push share a slot).
// Runs between the score launch (which wrote `alarm`) and the advance launch (`ticks` is still the push's first
// tick); reads the state, writes the ring only.  GAPS first walks the tiles once to AND every row's validity bytes.
#define GDN_CALIB_MIN_R 64
#define GDN_CALIB_MAX_R (1 << 20)

template <bool GAPS>
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_stream_calib_write_kernel(
    const void* __restrict__ state, const float* __restrict__ pred, const float* __restrict__ chunk,
    const int* __restrict__ alarm, const unsigned char* __restrict__ valid, int count, int n, int R,
    int exclude_alarms, double* __restrict__ ring_keys, unsigned char* __restrict__ ring_keep) {
  __shared__ double tile[64][65];
  __shared__ int keep_row[64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b0 = blockIdx.x * 64;
  const unsigned base = (unsigned)(reinterpret_cast<const long long*>(state)[0] % (long long)R);   // < R <= 2^20
  auto slot_of = [&](int b) -> unsigned {                    // b < count <= c <= R: one wrap at the most
    const unsigned at = base + (unsigned)b;
    return at >= (unsigned)R ? at - (unsigned)R : at;
  };
  for (int r = wv; r < 64; r += GDN_STREAM_THREADS / 64) {   // wave wv owns rows wv, wv + 4, ..: (wave uniform)
    const int b = b0 + r;
    if (b >= count) break;
    bool keep = !(exclude_alarms && alarm[b] != 0);
    if constexpr (GAPS) {
      bool real = true;
      for (int s0 = 0; s0 < n; s0 += 64) {
        const int s = s0 + lane;
        real = real && (s >= n || valid[(size_t)b * n + s] != 0);
      }
      keep = keep && __all(real);
    }
    if (lane == 0) {
      keep_row[r] = keep ? 1 : 0;
      ring_keep[slot_of(b)] = keep ? 1 : 0;
    }
  }
  __syncthreads();
  for (int s0 = 0; s0 < n; s0 += 64) {
    for (int r = wv; r < 64; r += GDN_STREAM_THREADS / 64) {
      const int b = b0 + r, s = s0 + lane;
      if (b < count && s < n) {
        const size_t o = (size_t)b * n + s;
        tile[r][lane] = score_key(pred[o], chunk[o]);
      }
    }
    __syncthreads();
    const int b = b0 + lane;                                 // now the lane runs along the push's rows = ring slots
    if (b < count) {
      const unsigned slot = slot_of(b);
      const bool keep = keep_row[lane] != 0;
      for (int r = wv; r < 64; r += GDN_STREAM_THREADS / 64) {
        const int s = s0 + r;
        if (s < n)
          ring_keys[(size_t)s * R + slot] = keep ? tile[lane][r] : filler_key();
      }
    }
    __syncthreads();                                         // the tile is rewritten by the next sensor tile
  }
}

// The ring write of per-sensor calibration (gdn_stream_calib_write_sensor; include/gdn_hip.h "Calibration on each
// sensor's own readings").  Slots and order are those of the kernel above.  A tick excluded by its alarm writes the
// filler into all n keys and keep = 0; any other tick writes keep = 1 and sensor i's key where valid[b, i] == 1, the
// filler where it is missing: the validity byte is read next to the value and the tile carries the filler pattern in
// the key's place.  A kernel of its own, so the two instantiations above stay as they are.
__global__ __launch_bounds__(GDN_STREAM_THREADS) void gdn_stream_calib_write_sensor_kernel(
    const void* __restrict__ state, const float* __restrict__ pred, const float* __restrict__ chunk,
    const int* __restrict__ alarm, const unsigned char* __restrict__ valid, int count, int n, int R,
    int exclude_alarms, double* __restrict__ ring_keys, unsigned char* __restrict__ ring_keep) {
  __shared__ double tile[64][65];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b0 = blockIdx.x * 64;
  const unsigned base = (unsigned)(reinterpret_cast<const long long*>(state)[0] % (long long)R);   // < R <= 2^20
  auto slot_of = [&](int b) -> unsigned {                    // b < count <= c <= R: one wrap at the most
    const unsigned at = base + (unsigned)b;
    return at >= (unsigned)R ? at - (unsigned)R : at;
  };
  if (threadIdx.x < 64) {
    const int b = b0 + (int)threadIdx.x;
    if (b < count) ring_keep[slot_of(b)] = (exclude_alarms && alarm[b] != 0) ? 0 : 1;
  }
  for (int s0 = 0; s0 < n; s0 += 64) {
    for (int r = wv; r < 64; r += GDN_STREAM_THREADS / 64) {
      const int b = b0 + r, s = s0 + lane;
      if (b < count && s < n) {
        const size_t o = (size_t)b * n + s;
        const bool keep = !(exclude_alarms && alarm[b] != 0) && valid[o] != 0;
        const double e = score_key(pred[o], chunk[o]);
        tile[r][lane] = keep ? e : filler_key();
      }
    }
    __syncthreads();
    const int b = b0 + lane;                                 // now the lane runs along the push's rows = ring slots
    if (b < count) {
      const unsigned slot = slot_of(b);
      for (int r = wv; r < 64; r += GDN_STREAM_THREADS / 64) {
        const int s = s0 + r;
        if (s < n) ring_keys[(size_t)s * R + slot] = tile[lane][r];
      }
    }
    __syncthreads();                                         // the tile is rewritten by the next sensor tile
  }
}

bool stream_shape_ok(int n, int w) { return w >= 1 && w <= GDN_LONG_MAX_W && n >= 1 && n <= 4096; }

bool calib_shape_ok(int n, int R) {
  return n >= 1 && n <= 4096 && R >= GDN_CALIB_MIN_R && R <= GDN_CALIB_MAX_R && 8ll * n * R <= (2ll << 30);
}

template <bool GAPS>
int calib_write(const void* state, const float* pred, const float* chunk, const int32_t* alarm, const uint8_t* valid,
                int c, int count, int n, int R, int exclude_alarms, double* ring_keys, uint8_t* ring_keep,
                void* stream) {
  if (!state || !pred || !chunk || !alarm || !ring_keys || !ring_keep || (GAPS && !valid)) return GDN_ERR_ARG;
  if (count < 1 || count > c) return GDN_ERR_ARG;
  if (!calib_shape_ok(n, R)) return GDN_ERR_UNSUPPORTED;
  if (c > R) return GDN_ERR_ARG;                   // two rows of one push would share a slot
  hipLaunchKernelGGL(gdn_stream_calib_write_kernel<GAPS>, dim3(((unsigned)count + 63) / 64), dim3(GDN_STREAM_THREADS),
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
  return calib_write<false>(state, pred, chunk, alarm, nullptr, c, count, n, R, exclude_alarms, ring_keys, ring_keep,
                            stream);
}

extern "C" int gdn_stream_calib_write_gaps(const void* state, const float* pred, const float* chunk,
                                           const int32_t* alarm, const uint8_t* valid, int c, int count, int n, int R,
                                           int exclude_alarms, double* ring_keys, uint8_t* ring_keep, void* stream) {
  return calib_write<true>(state, pred, chunk, alarm, valid, c, count, n, R, exclude_alarms, ring_keys, ring_keep,
                           stream);
}

extern "C" int gdn_stream_calib_write_sensor(const void* state, const float* pred, const float* chunk,
                                             const int32_t* alarm, const uint8_t* valid, int c, int count, int n,
                                             int R, int exclude_alarms, double* ring_keys, uint8_t* ring_keep,
                                             void* stream) {
  if (!state || !pred || !chunk || !alarm || !valid || !ring_keys || !ring_keep) return GDN_ERR_ARG;
  if (count < 1 || count > c) return GDN_ERR_ARG;
  if (!calib_shape_ok(n, R)) return GDN_ERR_UNSUPPORTED;
  if (c > R) return GDN_ERR_ARG;                   // two rows of one push would share a slot
  hipLaunchKernelGGL(gdn_stream_calib_write_sensor_kernel, dim3(((unsigned)count + 63) / 64),
                     dim3(GDN_STREAM_THREADS), 0, (hipStream_t)stream, state, pred, chunk, alarm, valid, count, n, R,
                     exclude_alarms, ring_keys, ring_keep);
  return gdn_launch_status();
}

extern "C" long long gdn_stream_state_bytes(int n, int w) {
  if (!stream_shape_ok(n, w)) return 0;
  const long long bytes = 8ll * GDN_STREAM_HEADER + 8ll * 3 * n + 4ll * n * w;
  return (bytes + 7) & ~7ll;
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
