// The steps of a stream push as __device__ functions, ONE source for the single-stream kernels (gdn_stream.hip) and
// the fleet kernels (gdn_fleet.hip): the layout of a stream state, the seeding of hist, the window cut, the score of a
// run of ticks with the carried smoothing state, the hist roll, and the carry / ordered log compaction / counters.
// A kernel decides which state, which rows and which count a workgroup works on and calls the step; a fleet is a
// stream per unit, so a unit's state block is written bit for bit as the single stream writes it.  The hold of
// missing readings (stream_fill_group), the write of the calibration ring (ring_write_tile) and the threshold a ring
// supports (ring_peak_tile) are steps like the others.
// The float64 scoring arithmetic is gdn_score_sweep.hpp's (no FMA contraction in a unit that includes this header).
#pragma once
#include "gdn_score_sweep.hpp"

namespace gdn_stream_steps {

using namespace gdn_sweep;

#define GDN_STREAM_HEADER 4          // int64 words ahead of the carry: ticks, alarms, logged, (reserved)
#define GDN_STREAM_THREADS 256
#define GDN_STREAM_PER_THREAD 4      // flat elements per thread, GDN_STREAM_THREADS apart (gdn_windows_gather's shape)
#define GDN_STREAM_SPAN (GDN_STREAM_THREADS * GDN_STREAM_PER_THREAD)

__host__ __device__ inline bool stream_shape_ok(int n, int w) {
  return w >= 1 && w <= GDN_LONG_MAX_W && n >= 1 && n <= 4096;
}
// bytes of one stream state (header, carry[3, n] float64, hist[n, w] fp32; rounded up to 8): a supported shape only
__host__ __device__ inline long long stream_state_size(int n, int w) {
  const long long bytes = 8ll * GDN_STREAM_HEADER + 8ll * 3 * n + 4ll * n * w;
  return (bytes + 7) & ~7ll;
}

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

// Span `span` of the flat [i, w] index: hist = the last w columns of history[n, h]; span 0 also zeroes the counters
// and the carry.
__device__ __forceinline__ void stream_seed_span(void* __restrict__ state, const float* __restrict__ history,
                                                 long long h, int n, int w, unsigned span, int tid) {
  const unsigned nw = (unsigned)n * (unsigned)w;
  const unsigned f0 = span * GDN_STREAM_SPAN + tid;
  float* __restrict__ hist = stream_hist(state, n);
#pragma unroll
  for (int j = 0; j < GDN_STREAM_PER_THREAD; ++j) {
    const unsigned f = f0 + j * GDN_STREAM_THREADS;
    if (f >= nw) break;
    const unsigned i = f / (unsigned)w, c = f - i * (unsigned)w;
    hist[f] = history[(long long)i * h + (h - w) + c];
  }
  if (span == 0) {
    long long* __restrict__ head = reinterpret_cast<long long*>(state);
    double* __restrict__ carry = stream_carry(state);
    if (tid < GDN_STREAM_HEADER) head[tid] = 0;
    for (int f = tid; f < 3 * n; f += GDN_STREAM_THREADS) carry[f] = 0.0;
  }
}

// Elements [span * SPAN, (span + 1) * SPAN) of window b's flat [i, c] index, into xb = x_out[b]: the w values of
// sensor i before tick b of the chunk.  Position b - w + c of the stream relative to the chunk's first tick: negative
// = column w + (b - w + c) = b + c of hist, else that row of the (time-major) chunk.
__device__ __forceinline__ void stream_window_span(const void* __restrict__ state, const float* __restrict__ chunk,
                                                   int n, int w, int b, unsigned span, int tid,
                                                   float* __restrict__ xb) {
  const unsigned nw = (unsigned)n * (unsigned)w;     // <= 4096 * 1024
  const float* __restrict__ hist = stream_hist(state, n);
  const unsigned f0 = span * GDN_STREAM_SPAN + tid;
#pragma unroll
  for (int j = 0; j < GDN_STREAM_PER_THREAD; ++j) {
    const unsigned f = f0 + j * GDN_STREAM_THREADS;
    if (f >= nw) break;
    const unsigned i = f / (unsigned)w, c = f - i * (unsigned)w;
    const int pos = b - w + (int)c;
    xb[f] = pos < 0 ? hist[(size_t)i * w + (unsigned)(b + (int)c)] : chunk[(size_t)pos * n + i];
  }
}

// The slot rule of a calibration ring (include/gdn_hip.h "Rolling calibration"): row b of a push whose first tick sits
// in slot base = ticks mod R owns slot (base + b) mod R.  b < c <= R, so one wrap at the most.
__device__ __forceinline__ unsigned calib_slot(unsigned base, int b, int R) {
  const unsigned at = base + (unsigned)b;
  return at >= (unsigned)R ? at - (unsigned)R : at;
}

// The ring write of a push (include/gdn_hip.h "Rolling calibration"), ONE source for a stream and for a unit of a
// fleet.  Row b is stream tick ticks + b; which of its keys are real follows the MODE:
//   PLAIN   a tick is kept unless it alarmed under exclude_alarms; a tick not kept writes the filler and keep = 0;
//   GAPS    ... or unless a reading of it was missing (valid);
//   SENSOR  keep = the alarm rule alone; the key of a missing reading is the filler, the tick's others are real.
// A kept tick writes score_key(pred, chunk) per sensor and keep = 1; a tick not kept leaves no older tick in its slot.
enum { CALIB_PLAIN = 0, CALIB_GAPS = 1, CALIB_SENSOR = 2 };

// What one stream's (one unit's) ring write reads and writes: the push's rows, the ring, and base = ticks mod R.
struct RingSource {
  const float *pred, *chunk;
  const int* alarm;
  const unsigned char* valid;        // PLAIN: not read
  double* keys;                      // [n, R]
  unsigned char* keep;               // [R]
  unsigned base;
};
__device__ __forceinline__ unsigned ring_base(const void* state, int R) {
  return (unsigned)(reinterpret_cast<const long long*>(state)[0] % (long long)R);       // < R <= 2^20
}
// does tick b count?  All 64 lanes of a wave call it (GAPS: an __all over the row's validity bytes).
template <int MODE>
__device__ __forceinline__ bool ring_keep_row(const RingSource& rs, int b, int n, int exclude_alarms, int lane) {
  bool keep = !(exclude_alarms && rs.alarm[b] != 0);
  if constexpr (MODE == CALIB_GAPS) {
    bool real = true;
    for (int s0 = 0; s0 < n; s0 += 64) {
      const int s = s0 + lane;
      real = real && (s >= n || rs.valid[(size_t)b * n + s] != 0);
    }
    keep = keep && __all(real);
  }
  return keep;
}
// the key of reading o = b * n + s of a tick whose keep flag is `keep`
template <int MODE>
__device__ __forceinline__ double ring_key(const RingSource& rs, size_t o, bool keep) {
  if constexpr (MODE == CALIB_SENSOR) keep = keep && rs.valid[o] != 0;
  const double e = score_key(rs.pred[o], rs.chunk[o]);
  return keep ? e : filler_key();
}

// A workgroup of GDN_STREAM_THREADS threads, rows [b0, min(b0 + 64, count)) of the push: the keep flags (wave wv owns
// rows wv, wv + 4, ..), then sensor tiles of 64 transposed through the padded LDS tile of score_keys_kernel: fp32 reads
// along sensors, fp64 writes along slots.  The slot is computed per row: a tile may wrap the ring's end once.  Every
// thread of the workgroup must call it (barriers inside); b0 < count.
template <int MODE>
__device__ __forceinline__ void ring_write_tile(const RingSource& rs, int b0, int count, int n, int R,
                                                int exclude_alarms, int tid) {
  __shared__ double tile[64][65];
  __shared__ int keep_row[64];
  const int lane = tid & 63, wv = tid >> 6;
  // PLAIN, GAPS: a tick is kept or not as a whole; the flag travels through LDS to the store phase, where the lane
  // runs along the rows, and the tile carries every key.  SENSOR: the flag is the alarm rule alone, a thread per row
  // writes it, and the tile carries the filler in the place of a key (no keep_row, one barrier fewer: measured).
  constexpr bool BY_ROW = MODE != CALIB_SENSOR;
  if constexpr (BY_ROW) {
    for (int r = wv; r < 64; r += GDN_STREAM_THREADS / 64) { // (wave uniform)
      const int b = b0 + r;
      if (b >= count) break;
      const bool keep = ring_keep_row<MODE>(rs, b, n, exclude_alarms, lane);
      if (lane == 0) {
        keep_row[r] = keep ? 1 : 0;
        rs.keep[calib_slot(rs.base, b, R)] = keep ? 1 : 0;
      }
    }
    __syncthreads();
  } else {
    const int b = b0 + tid;
    if (tid < 64 && b < count)
      rs.keep[calib_slot(rs.base, b, R)] = ring_keep_row<MODE>(rs, b, n, exclude_alarms, lane) ? 1 : 0;
  }
  for (int s0 = 0; s0 < n; s0 += 64) {
    for (int r = wv; r < 64; r += GDN_STREAM_THREADS / 64) {
      const int b = b0 + r, s = s0 + lane;
      if (b < count && s < n)
        tile[r][lane] = ring_key<MODE>(rs, (size_t)b * n + s,
                                       BY_ROW || ring_keep_row<MODE>(rs, b, n, exclude_alarms, lane));
    }
    __syncthreads();
    const int b = b0 + lane;                                 // now the lane runs along the push's rows = ring slots
    if (b < count) {
      const unsigned slot = calib_slot(rs.base, b, R);
      const bool keep = !BY_ROW || keep_row[lane] != 0;
      for (int r = wv; r < 64; r += GDN_STREAM_THREADS / 64) {
        const int s = s0 + r;
        if (s < n) rs.keys[(size_t)s * R + slot] = keep ? tile[lane][r] : filler_key();
      }
    }
    __syncthreads();                                         // the tile is rewritten by the next sensor tile
  }
}

// The threshold a ring supports (include/gdn_hip.h "Threshold from the ring"), ONE source for a stream
// and for a unit of a fleet: the largest smoothed score, under the table in force, among the slots whose four-tick
// window the ring holds whole.  The rule per slot stands here once:
//   ring_norm      the normalised error of one key: norm's expression on a key that is already |pred - gt|; SENSOR:
//                  the filler is a missing reading, error exactly 0.0 (tick modes never read a filler in an eligible
//                  window: a tick not kept holds the filler in every key and makes its window ineligible);
//   ring_smooth    the scorer's left-to-right 4-term mean;
//   ring_eligible  keep at q, q - 1, q - 2, q - 3 (mod R) and (q - base) mod R >= 3: the window neither holds a tick
//                  that was left out nor straddles the seam between the newest tick (base - 1) and the oldest (base).
template <int MODE>
__device__ __forceinline__ double ring_norm(double key, double med, double inv_den) {
  const double a = (key - med) * inv_den;
  if constexpr (MODE == CALIB_SENSOR) return (unsigned long long)__double_as_longlong(key) == FILLER ? 0.0 : a;
  return a;
}
__device__ __forceinline__ double ring_smooth(double e3, double e2, double e1, double e0) {
  return (((e3 + e2) + e1) + e0) / 4.0;
}
__device__ __forceinline__ bool ring_eligible(bool k3, bool k2, bool k1, bool k0, unsigned q, unsigned base, int R) {
  const unsigned age = q >= base ? q - base : q + (unsigned)R - base;        // 0: the oldest tick of a full ring
  return k3 && k2 && k1 && k0 && age >= 3u;
}

// What a run of slots, a unit's ring or a fleet's workspace row reduces to.  slot == NONE: no eligible slot (peak is
// then -inf).  Larger peak first, equal peaks by the lower slot: exact in any order, so no tiling changes a bit.
struct RingPeak {
  double peak;
  int slot, eligible;
};
__device__ __forceinline__ void ring_peak_merge(double& peak, int& slot, double op, int os) {
  if (op > peak || (op == peak && os < slot)) { peak = op; slot = os; }
}
__device__ __forceinline__ void ring_peak_wave(double& peak, int& slot) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double op = __shfl_xor(peak, d);
    const int os = __shfl_xor(slot, d);
    ring_peak_merge(peak, slot, op, os);
  }
}

#define GDN_RING_TILE 61             // slots a wave owns: its 64 lanes hold them and the 3 slots before (mod R)
__host__ __device__ inline int ring_tiles(int R) { return (R + GDN_RING_TILE - 1) / GDN_RING_TILE; }

// One wave, tile t < ring_tiles(R) of one ring (keys [n, R], keep [R], the table med_iqr [n, 2] in force): lane l holds
// slot (61 t - 3 + l) mod R — lanes 0, 1, 2 the halo, taken mod R and never clamped, lanes 3 .. 63 the slots the wave
// owns (those below R).  The lanes run along the slots (R is contiguous: one coalesced 8-byte load per lane and
// sensor); the three predecessors of a slot come from the lanes below (__shfl_up), never from memory again.  The wave
// walks the sensors, four loads in flight, and keeps the running maximum per slot in a register (fmax: a NaN error
// never wins, as in the scorer).  sensor_scale runs once per sensor and wave — 64 sensors at a time, a lane each, then
// broadcast — so the float64 division is off the per-slot path.  Returns, in every lane, the wave's masked maximum
// with its slot and its eligible count.  All 64 lanes call it; no LDS, no barrier.
template <int MODE>
__device__ __forceinline__ RingPeak ring_peak_tile(const double* __restrict__ keys,
                                                   const unsigned char* __restrict__ keep,
                                                   const double* __restrict__ med_iqr, unsigned base, int n, int R,
                                                   int t, int lane) {
  const int at = t * GDN_RING_TILE - 3 + lane;               // < R + 64 <= 2 R
  const unsigned q = (unsigned)(at < 0 ? at + R : (at >= R ? at - R : at));
  const bool owned = lane >= 3 && at < R;
  const int k0 = keep[q] != 0 ? 1 : 0;
  const int k1 = __shfl_up(k0, 1), k2 = __shfl_up(k0, 2), k3 = __shfl_up(k0, 3);
  const bool ok = owned && ring_eligible(k3 != 0, k2 != 0, k1 != 0, k0 != 0, q, base, R);
  double best = -INFINITY;
  for (int s0 = 0; s0 < n; s0 += 64) {
    const Scale mine = sensor_scale(med_iqr, min(s0 + lane, n - 1));
    const int cnt = min(64, n - s0);                         // (wave uniform)
    for (int j0 = 0; j0 < cnt; j0 += 4) {
      double key[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)                            // past the last sensor: the last one again (max is idempotent)
        key[i] = keys[(size_t)(s0 + min(j0 + i, cnt - 1)) * R + q];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = min(j0 + i, cnt - 1);
        const double e0 = ring_norm<MODE>(key[i], __shfl(mine.med, j), __shfl(mine.inv_den, j));
        const double e1 = __shfl_up(e0, 1), e2 = __shfl_up(e0, 2), e3 = __shfl_up(e0, 3);
        best = fmax(best, ring_smooth(e3, e2, e1, e0));
      }
    }
  }
  RingPeak out{ok ? best : -INFINITY, ok ? (int)q : NONE, (int)__popcll(__ballot(ok))};
  ring_peak_wave(out.peak, out.slot);
  return out;
}

// Hold missing readings.  "Missing" is decided on the bit pattern (exponent field all ones: NaN, +inf, -inf), so it
// does not depend on how floating-point comparisons with NaN are compiled.
#define GDN_FILL_WAVES 16            // waves of the single stream's workgroup (a fleet picks 1, 4 or 16 from c)
#define GDN_FILL_DEPTH 8             // row loads in flight per lane
__device__ inline bool stream_missing(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// A workgroup of WAVES waves, sensor group g: sensors [64 g, 64 g + 64), one per lane (a row of the time-major chunk is
// contiguous along sensors: coalesced).  Wave v walks rows [v * seg, (v + 1) * seg) ^ [0, count), DEPTH loads at a
// time, and reduces them to (latest real reading, found one, missing readings, missing readings after the latest real
// one = the whole segment when there is none).  "The right-most real reading wins" is associative: the segments meet in
// LDS, every wave takes the latest real reading before its segment (hist[i, w - 1] when no earlier segment has one) and
// walks its rows a second time, writing.  Wave 0 folds the counts.  Integer counts and copies only, so every WAVES
// gives the same bits.  Reads the state, writes none of it; rows at or beyond `count` are neither read nor written.
// Every thread of the workgroup must call it (a barrier inside); count >= 1.
template <int WAVES>
__device__ __forceinline__ void stream_fill_group(const void* __restrict__ state, const float* __restrict__ raw,
                                                  int count, int n, int w, float* __restrict__ filled,
                                                  unsigned char* __restrict__ valid, int* __restrict__ gap_chunk,
                                                  int g, int tid) {
  __shared__ float seg_last[WAVES][64];
  __shared__ int seg_found[WAVES][64];
  __shared__ int seg_missing[WAVES][64];
  __shared__ int seg_trail[WAVES][64];
  const int lane = tid & 63, wv = tid >> 6;
  const int i = g * 64 + lane;
  const bool live = i < n;
  const int ic = live ? i : n - 1;                                   // a dead lane reads sensor n - 1, writes nothing
  const int seg = (count + WAVES - 1) / WAVES;
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
    for (int v = 0; v < WAVES; ++v) total += seg_missing[v][lane];
    for (int v = WAVES - 1; v >= 0; --v) {                           // from the last row back to the latest real reading
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
// before; zeros where the series has no such tick, GAPS: 0.0 for a missing reading, through the advance step).

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

// One wave, one run: ticks [run * RUN, min(t, run * RUN + RUN)) of a push of t rows; lists and flags of those rows.
template <bool GAPS>
__device__ __forceinline__ void stream_score_run(const StreamSource& src, const double* __restrict__ med_iqr,
                                                 double thr, long long first_tick, int run, int lane, int m,
                                                 double* __restrict__ top_scores, int* __restrict__ top_sensors,
                                                 int* __restrict__ alarm) {
  const int t = src.t, n = src.n;
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

// A whole workgroup rolls row i of hist by `count` ticks: every thread loads its (up to 4) columns of the NEW row —
// from the old row where the column survives, else from the chunk — then a barrier, then the stores: no column is
// read after it has been overwritten, whatever count is.
__device__ __forceinline__ void stream_roll_row(void* __restrict__ state, const float* __restrict__ chunk, int count,
                                                int n, int w, int i, int tid) {
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
}

// One workgroup per stream: the carry (one thread per sensor: its three old entries are read before any is written),
// the alarm log (an ordered compaction: ballot and popcount inside a wave, four wave totals through LDS, 256 flags a
// round in tick order) and, last, the counters.
// GAPS: `chunk` is the filled chunk; a carry entry taken from the chunk is 0.0 where valid says the reading was
// missing, and the carry thread of sensor s folds the push's gap_chunk [2, n] into gaps [2, n] (missing_total,
// missing_run).  Without GAPS the three trailing parameters are not read.
template <bool GAPS>
__device__ __forceinline__ void stream_carry_log(void* __restrict__ state, const float* __restrict__ chunk,
                                                 const float* __restrict__ pred, const double* __restrict__ med_iqr,
                                                 const int* __restrict__ alarm, const int* __restrict__ top_sensors,
                                                 int count, int n, int m, long long* __restrict__ log_ticks,
                                                 int* __restrict__ log_sensors, long long log_len, int tid,
                                                 const unsigned char* __restrict__ valid,
                                                 const int* __restrict__ gap_chunk, long long* __restrict__ gaps) {
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

}  // namespace gdn_stream_steps
