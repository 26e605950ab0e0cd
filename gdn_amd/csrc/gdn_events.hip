// Alarm episodes (include/gdn_hip.h "Alarm episodes"): on-delay, hysteresis, off-delay and an episode
// table, as an archive scan that is parallel over T (gdn_episodes_scan) and as one launch of a stream push
// (gdn_stream_events; gdn_fleet_events: the same per unit of a fleet).  Comparisons and copies only: no floating-point arithmetic, so both forms and the sequential
// definition agree bit for bit.
//
// Both forms run the same tile code (EvTile): a workgroup of 256 threads owns a tile of 256 * TPT consecutive ticks,
// a thread TPT consecutive ones.  Inside a tile
//   run_hi / run_lo   = position - (running max of the last position that was not above / not below),
//   active            = the kind of the running max over (position, kind) of the set / reset ticks,
//   an episode's row  = an ordered prefix count of the opens,
//   "will this run of above ticks raise?" = (running min, from the right, of the next tick that is not above) - (the
//                       run's first tick) >= on,
// each a wave scan by shuffles plus four wave totals through LDS.  What a tile needs from its neighbours:
//   - the run lengths at its first tick: it looks back over at most max(on, off) <= 4096 ticks itself;
//   - whether a run that leaves it unraised goes on to raise: it looks ahead over at most on ticks itself;
//   - `active` and the number of opens before it: one aggregate per tile (kind of the first and of the last set / reset
//     tick, opens after the first) and ONE workgroup that scans the aggregates in a launch of its own.
// So the archive form is five launches — reduce, scan of the tile aggregates, apply (peak keys), apply (peak ticks),
// finish — and no workgroup ever waits on another.  The number of tiles depends on T alone and a workgroup strides
// over tiles, so every grid size gives the same bits.
// Peaks: only a tick above `hi` can be an episode's peak.  Such a tick knows its row; it folds an order-preserving
// 64-bit image of its score into the row's key with an integer atomic max, and in the second apply launch the ticks
// whose image equals the key fold their tick with an integer atomic min: the first tick that holds the largest score.
// Both are order independent.  A wave whose lanes all aim at one row reduces by shuffles and issues one atomic.  The
// peak's bits and its sensors are then copied from that tick's own row of the input (so -0.0 stays -0.0).
// The stream form keeps keys and ticks of its (at most 2049) rows in LDS and is one workgroup.
#include "gdn_common.hpp"

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_TPT = 8;                                  // archive: ticks per thread
constexpr int EV_TILE = EV_THREADS * EV_TPT;               // 2048 ticks per tile
constexpr int EV_STREAM_TPT = 16;                          // stream: ONE tile of 4096 ticks
constexpr int EV_STREAM_MAX = EV_THREADS * EV_STREAM_TPT;
constexpr int EV_MAX_RUN = 4096;
constexpr long long EV_MAX_T = 1ll << 26;
constexpr long long EV_MAX_E = 1ll << 20;
constexpr int EV_NONE = -(1 << 30);
constexpr int EV_FAR = 1 << 30;
constexpr unsigned long long EV_NO_TICK = ~0ull;
constexpr int EV_CARRY_WORDS = GDN_EPISODES_CARRY_BYTES / 8;
constexpr int EV_INFO_WORDS = 12;                          // workspace words after the carry copy (EvInfo)
constexpr int EV_TILE_INTS = 7;                            // per-tile ints of the workspace

// The carried state (GDN_EPISODES_CARRY_BYTES; all zero = a series that has not begun).  run_hi / run_lo saturate at
// on / off.  cand_*: the peak so far of a run of above ticks that has not raised yet (!active && run_hi > 0).
struct EvCarry {
  long long count, active, run_hi, run_lo;
  double cand_peak;
  long long cand_tick;
  int cand_sensors[8];
  long long open_start;
  double open_peak;
  long long open_peak_tick;
  int open_sensors[8];
  long long reserved[3];
};
static_assert(sizeof(EvCarry) == GDN_EPISODES_CARRY_BYTES, "carry layout");

struct EvInfo {                                            // written by the scan launch, read by the later ones
  long long count_out, active_out, run_hi_out, run_lo_out, spans, open_start, reserved[6];
};
static_assert(sizeof(EvInfo) == 8 * EV_INFO_WORDS, "info layout");

struct EvParams {
  const double* scores;
  long long stride;                                        // doubles between two ticks' scores
  long long T, first_tick, E;
  double hi, lo;
  int on, off, m;
};

// order-preserving image of a score that is not NaN; -0.0 and +0.0 share one image (they compare equal)
__device__ __forceinline__ unsigned long long ev_image(double s) {
  unsigned long long b = (unsigned long long)__double_as_longlong(s);
  if ((b << 1) == 0ull) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct EvMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct EvMin { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };
struct EvSum { __device__ int operator()(int a, int b) const { return a + b; } };

// Exclusive scan of one int per thread over the workgroup's 256 threads (commutative op), from the left or — REVERSE —
// from the right; `total` = the whole workgroup's.  sc: 4 ints of LDS.  Every thread must call it.
template <bool REVERSE, class Op>
__device__ __forceinline__ int ev_block_scan(int v, int ident, Op op, int* sc, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = REVERSE ? __shfl_down(inc, d) : __shfl_up(inc, d);
    if (REVERSE ? lane + d < 64 : lane >= d) inc = op(inc, o);
  }
  if (lane == (REVERSE ? 0 : 63)) sc[wv] = inc;
  __syncthreads();
  int pre = ident;
  total = ident;
#pragma unroll
  for (int q = 0; q < EV_THREADS / 64; ++q) {
    if (REVERSE ? q > wv : q < wv) pre = op(pre, sc[q]);
    total = op(total, sc[q]);
  }
  int ex = REVERSE ? __shfl_down(inc, 1) : __shfl_up(inc, 1);
  if (lane == (REVERSE ? 63 : 0)) ex = ident;
  __syncthreads();                                         // sc is rewritten by the next scan
  return op(pre, ex);
}

// The run lengths at tick `pos` (the runs of above / below ticks that end at pos - 1), saturated at on / off, from at
// most max(on, off) ticks before it; a run that reaches the first tick goes on into the carried run.  *spans: the
// above-run reached the first tick.
__device__ void ev_lookback(const EvParams& P, long long pos, long long carry_hi, long long carry_lo, int* sc,
                            int& rhi, int& rlo, int* spans = nullptr) {
  const int window = P.on > P.off ? P.on : P.off;
  int dh = EV_FAR, dl = EV_FAR;
  for (int d = threadIdx.x; d < window; d += EV_THREADS) {
    const long long gi = pos - 1 - d;
    if (gi < 0) break;
    const double sv = P.scores[gi * P.stride];
    if (!(sv > P.hi) && d < dh) dh = d;
    if ((sv > P.lo) && d < dl) dl = d;
  }
  int th, tl;
  ev_block_scan<false>(dh, EV_FAR, EvMin(), sc, th);
  ev_block_scan<false>(dl, EV_FAR, EvMin(), sc, tl);
  const long long avail = pos < window ? pos : window;
  long long h = th < EV_FAR ? th : avail + (avail == pos ? carry_hi : 0);
  long long l = tl < EV_FAR ? tl : avail + (avail == pos ? carry_lo : 0);
  rhi = (int)(h < P.on ? h : P.on);
  rlo = (int)(l < P.off ? l : P.off);
  if (spans) *spans = (th == EV_FAR && avail == pos) ? 1 : 0;
}

// Ticks from `pos` to the first one at or after it that is not above, looking at no more than `on` ticks: `on` when
// all of them are above, T - pos when the series ends first.
__device__ int ev_lookahead(const EvParams& P, long long pos, int* sc) {
  int dh = EV_FAR;
  for (int d = threadIdx.x; d < P.on; d += EV_THREADS) {
    const long long gi = pos + d;
    if (gi >= P.T) break;
    if (!(P.scores[gi * P.stride] > P.hi) && d < dh) dh = d;
  }
  int th;
  ev_block_scan<false>(dh, EV_FAR, EvMin(), sc, th);
  if (th < EV_FAR) return th;
  const long long left = P.T - pos;
  return (int)(left < P.on ? left : P.on);
}

// One tile's ticks in registers.  Bit u of a mask = this thread's tick u (tile position threadIdx.x * TPT + u).
template <int TPT>
struct EvTile {
  double s[TPT];
  unsigned above, below;          // above: s > hi; below: !(s > lo); a tick at or after T is neither
  unsigned setm, openm, closem, actm;   // set ticks; opens; closes; active AFTER the tick
  int Lh0;                        // the last position before this thread's ticks that is not above (< 0: before the tile)
  int Lh_tot, Ll_tot;             // ... of the whole tile (EV_NONE: none inside the tile)
  int opens_excl, opens_total;    // opens before this thread's ticks / in the tile
  int first_code, last_code;      // (position << 2 | kind) of the tile's first / last set (2) or reset (1) tick
};

// rhi0 / rlo0: the run lengths at the tile's first tick; a0: `active` before it.
template <int TPT, bool WANT_FIRST>
__device__ __forceinline__ void ev_tile_events(EvTile<TPT>& t, const EvParams& P, long long tile0, int rhi0, int rlo0,
                                               int a0, int* sc) {
  const int p0 = threadIdx.x * TPT;
  t.above = t.below = 0u;
  int la = EV_NONE, lb = EV_NONE;
#pragma unroll
  for (int u = 0; u < TPT; ++u) {
    const long long gi = tile0 + p0 + u;
    const bool valid = gi < P.T;
    const double sv = valid ? P.scores[gi * P.stride] : 0.0;
    t.s[u] = sv;
    const bool ab = valid && sv > P.hi, be = valid && !(sv > P.lo);
    t.above |= (ab ? 1u : 0u) << u;
    t.below |= (be ? 1u : 0u) << u;
    if (valid && !ab) la = p0 + u;
    if (valid && !be) lb = p0 + u;
  }
  const int eh = ev_block_scan<false>(la, EV_NONE, EvMax(), sc, t.Lh_tot);
  const int el = ev_block_scan<false>(lb, EV_NONE, EvMax(), sc, t.Ll_tot);
  t.Lh0 = eh > -1 - rhi0 ? eh : -1 - rhi0;
  int Lh = t.Lh0, Ll = el > -1 - rlo0 ? el : -1 - rlo0;
  unsigned rstm = 0u;
  t.setm = 0u;
  int le = -1, fe = EV_FAR;
#pragma unroll
  for (int u = 0; u < TPT; ++u) {
    const int p = p0 + u;
    int kind = 0;
    if ((t.above >> u) & 1u) {
      if (p - Lh >= P.on) kind = 2;
    } else {
      Lh = p;
    }
    if ((t.below >> u) & 1u) {
      if (p - Ll >= P.off) kind = 1;
    } else {
      Ll = p;
    }
    if (kind) {
      if (kind == 2) t.setm |= 1u << u; else rstm |= 1u << u;
      le = (p << 2) | kind;
      if (fe == EV_FAR) fe = le;
    }
  }
  const int pe = ev_block_scan<false>(le, -1, EvMax(), sc, t.last_code);
  t.first_code = EV_FAR;
  if constexpr (WANT_FIRST) ev_block_scan<false>(fe, EV_FAR, EvMin(), sc, t.first_code);
  int a = pe < 0 ? a0 : ((pe & 3) == 2 ? 1 : 0);
  t.openm = t.closem = t.actm = 0u;
  int opens = 0;
#pragma unroll
  for (int u = 0; u < TPT; ++u) {
    if ((t.setm >> u) & 1u) {
      if (!a) { t.openm |= 1u << u; ++opens; }
      a = 1;
    } else if ((rstm >> u) & 1u) {
      if (a) t.closem |= 1u << u;
      a = 0;
    }
    t.actm |= (unsigned)a << u;
  }
  t.opens_excl = ev_block_scan<false>(opens, 0, EvSum(), sc, t.opens_total);
}

// What an above tick folds its score into, relative to the rows of its tile: rel[u] = j >= 0: the episode that is the
// j-th open counted from the tile's first tick (0: the one open before the tile); -1: nothing (a run that ends
// unraised); -2: the candidate (a run that reaches the end of the series unraised).  `ahead`: ev_lookahead at the
// tile's end (0 when the series ends inside the tile).
template <int TPT>
__device__ __forceinline__ void ev_tile_targets(const EvTile<TPT>& t, const EvParams& P, long long tile0, int ahead,
                                                int* sc, int (&rel)[TPT]) {
  const int p0 = threadIdx.x * TPT;
  int fa = EV_FAR;
#pragma unroll
  for (int u = TPT - 1; u >= 0; --u)
    if (!((t.above >> u) & 1u)) fa = p0 + u;
  int unused;
  int N = ev_block_scan<true>(fa, EV_FAR, EvMin(), sc, unused);
  const int beyond = EV_THREADS * TPT + ahead;
  if (N > beyond) N = beyond;
  int first[TPT];                                          // the first position of the above-run a tick is in
  int Lh = t.Lh0;
#pragma unroll
  for (int u = 0; u < TPT; ++u) {
    if (!((t.above >> u) & 1u)) Lh = p0 + u;
    first[u] = Lh + 1;
  }
#pragma unroll
  for (int u = TPT - 1; u >= 0; --u) {
    rel[u] = -1;
    if (!((t.above >> u) & 1u)) {
      N = p0 + u;
      continue;
    }
    const int oi = t.opens_excl + __popc(t.openm & ((2u << u) - 1u));
    if ((t.actm >> u) & 1u) rel[u] = oi;
    else if (N - first[u] >= P.on) rel[u] = oi + 1;
    else if (tile0 + N >= P.T) rel[u] = -2;
  }
}

// Fold `val` into slots[slot] (slot < 0 or val == the identity: nothing).  IS_MAX: atomic max, else atomic min.  A wave
// whose folding lanes all aim at one slot reduces by shuffles and issues one atomic.  Every lane of the wave calls it.
template <bool IS_MAX>
__device__ __forceinline__ void ev_fold(unsigned long long* slots, long long slot, unsigned long long val) {
  const unsigned long long ident = IS_MAX ? 0ull : EV_NO_TICK;
  const bool has = slot >= 0 && val != ident;
  const unsigned long long mask = __ballot(has);
  if (!mask) return;
  const int leader = __ffsll((long long)mask) - 1;
  const long long s0 = __shfl(slot, leader);
  if (__ballot(has && slot == s0) == mask) {
    unsigned long long v = has ? val : ident;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(v, d);
      v = IS_MAX ? (o > v ? o : v) : (o < v ? o : v);
    }
    if ((int)(threadIdx.x & 63) == leader) {
      if (IS_MAX) atomicMax(&slots[s0], v); else atomicMin(&slots[s0], v);
    }
  } else if (has) {
    if (IS_MAX) atomicMax(&slots[slot], val); else atomicMin(&slots[slot], val);
  }
}

// A thread's TPT (slot, value) pairs: one fold when every thread of the wave has a single slot, else TPT folds.
template <int TPT, bool IS_MAX>
__device__ __forceinline__ void ev_fold_thread(unsigned long long* slots, const long long (&slot)[TPT],
                                               const unsigned long long (&val)[TPT]) {
  const unsigned long long ident = IS_MAX ? 0ull : EV_NO_TICK;
  long long one = -1;
  unsigned long long v = ident;
  bool single = true;
#pragma unroll
  for (int u = 0; u < TPT; ++u) {
    if (slot[u] < 0 || val[u] == ident) continue;
    if (one >= 0 && slot[u] != one) single = false;
    one = slot[u];
    v = IS_MAX ? (val[u] > v ? val[u] : v) : (val[u] < v ? val[u] : v);
  }
  if (__all(single)) {
    ev_fold<IS_MAX>(slots, one, v);
  } else {
#pragma unroll
    for (int u = 0; u < TPT; ++u) ev_fold<IS_MAX>(slots, slot[u], val[u]);
  }
}

// ---- archive form ---------------------------------------------------------------------------------------------------
struct EvWorkspace {
  EvCarry* carry;                 // the scan launch's copy of carry_in (zeros without one)
  EvInfo* info;
  unsigned long long* key;        // [E + 2]: rows 0 .. E - 1, E = the episode open at the end when its row >= E,
  unsigned long long* ptick;      //          E + 1 = the candidate run
  int* tile;                      // [EV_TILE_INTS][tiles]: rhi0, rlo0, ahead, first << 2 | last, opens, active_in, opens_before
  long long tiles;
};

__host__ __device__ inline EvWorkspace ev_workspace(void* ws, long long T, long long E) {
  EvWorkspace w;
  long long* words = reinterpret_cast<long long*>(ws);
  w.carry = reinterpret_cast<EvCarry*>(words);
  w.info = reinterpret_cast<EvInfo*>(words + EV_CARRY_WORDS);
  w.key = reinterpret_cast<unsigned long long*>(words + EV_CARRY_WORDS + EV_INFO_WORDS);
  w.ptick = w.key + (E + 2);
  w.tile = reinterpret_cast<int*>(w.ptick + (E + 2));
  w.tiles = (T + EV_TILE - 1) / EV_TILE;
  return w;
}

// Launch 1.  Per tile: its look-back and look-ahead and, with `active` taken as 0 before it, the aggregate (kind of
// the first and last set / reset tick, opens after the first).  All threads of the grid also clear the rows this call
// can reach: end = -1, key = 0, ptick = none for rows [base, base + T / 2 + 2) below E, and the two extra slots.
__global__ __launch_bounds__(EV_THREADS) void gdn_episodes_reduce_kernel(EvParams P, const EvCarry* __restrict__ carry_in,
                                                                         void* __restrict__ ws_raw,
                                                                         long long* __restrict__ end) {
  __shared__ int sc[EV_THREADS / 64];
  const EvWorkspace W = ev_workspace(ws_raw, P.T, P.E);
  const long long c_hi = carry_in ? carry_in->run_hi : 0, c_lo = carry_in ? carry_in->run_lo : 0;
  const long long base = carry_in ? carry_in->count - (carry_in->active ? 1 : 0) : 0;
  const long long reach = P.T / 2 + 2;
  for (long long r = (long long)blockIdx.x * EV_THREADS + threadIdx.x; r < reach + 2; r += (long long)gridDim.x * EV_THREADS) {
    const long long row = r < reach ? base + r : P.E + (r - reach);
    if (r < reach && row >= P.E) continue;
    W.key[row] = 0ull;
    W.ptick[row] = EV_NO_TICK;
    if (r < reach) end[row] = -1;
  }
  for (long long tile = blockIdx.x; tile < W.tiles; tile += gridDim.x) {
    const long long tile0 = tile * EV_TILE;
    int rhi0, rlo0;
    ev_lookback(P, tile0, c_hi, c_lo, sc, rhi0, rlo0);
    const int ahead = tile0 + EV_TILE < P.T ? ev_lookahead(P, tile0 + EV_TILE, sc) : 0;
    EvTile<EV_TPT> t;
    ev_tile_events<EV_TPT, true>(t, P, tile0, rhi0, rlo0, 0, sc);
    if (threadIdx.x == 0) {
      const int first = t.first_code == EV_FAR ? 0 : (t.first_code & 3), last = t.last_code < 0 ? 0 : (t.last_code & 3);
      W.tile[0 * W.tiles + tile] = rhi0;
      W.tile[1 * W.tiles + tile] = rlo0;
      W.tile[2 * W.tiles + tile] = ahead;
      W.tile[3 * W.tiles + tile] = (first << 2) | last;
      W.tile[4 * W.tiles + tile] = t.opens_total - (first == 2 ? 1 : 0);
    }
  }
}

// Launch 2, ONE workgroup.  Thread q owns the tiles [q * per, (q + 1) * per): the exclusive scan of the aggregates
// gives every tile `active` before it and the opens before it; the totals, the run lengths after the last tick and a
// copy of carry_in go to the workspace.
__global__ __launch_bounds__(EV_THREADS) void gdn_episodes_scan_kernel(EvParams P, const EvCarry* __restrict__ carry_in,
                                                                       void* __restrict__ ws_raw) {
  __shared__ int sc[EV_THREADS / 64];
  const EvWorkspace W = ev_workspace(ws_raw, P.T, P.E);
  const int tid = threadIdx.x;
  EvCarry c;
  long long* cw = reinterpret_cast<long long*>(&c);
#pragma unroll
  for (int q = 0; q < EV_CARRY_WORDS; ++q) cw[q] = carry_in ? reinterpret_cast<const long long*>(carry_in)[q] : 0ll;
  const int a_in = c.active ? 1 : 0;
  const long long per = (W.tiles + EV_THREADS - 1) / EV_THREADS;
  const long long q0 = tid * per, q1 = q0 + per < W.tiles ? q0 + per : W.tiles;
  const int* fl = W.tile + 3 * W.tiles;
  const int* oi = W.tile + 4 * W.tiles;
  int last = 0;
  for (long long q = q0; q < q1; ++q)
    if (fl[q] & 3) last = fl[q] & 3;
  int tot_code;
  const int pe = ev_block_scan<false>(last ? ((tid << 2) | last) : -1, -1, EvMax(), sc, tot_code);
  const int a_thread = pe < 0 ? a_in : ((pe & 3) == 2 ? 1 : 0);
  int a = a_thread, opens = 0;
  for (long long q = q0; q < q1; ++q) {
    const int first = fl[q] >> 2, lst = fl[q] & 3;
    opens += oi[q] + (first == 2 && !a ? 1 : 0);
    if (lst) a = lst == 2 ? 1 : 0;
  }
  int tot_opens;
  int before = ev_block_scan<false>(opens, 0, EvSum(), sc, tot_opens);
  a = a_thread;
  for (long long q = q0; q < q1; ++q) {
    const int first = fl[q] >> 2, lst = fl[q] & 3;
    W.tile[5 * W.tiles + q] = a;
    W.tile[6 * W.tiles + q] = before;
    before += oi[q] + (first == 2 && !a ? 1 : 0);
    if (lst) a = lst == 2 ? 1 : 0;
  }
  int rhi, rlo, spans;
  ev_lookback(P, P.T, c.run_hi, c.run_lo, sc, rhi, rlo, &spans);
  if (tid == 0) {
    *W.carry = c;
    EvInfo info = {};
    info.count_out = c.count + tot_opens;
    info.active_out = tot_code < 0 ? a_in : ((tot_code & 3) == 2 ? 1 : 0);
    info.run_hi_out = rhi;
    info.run_lo_out = rlo;
    info.spans = spans;
    info.open_start = c.open_start;
    *W.info = info;
  }
}

// Launches 3 (PASS 0) and 4 (PASS 1).  PASS 0: opens write `start`, closes write `end`, above ticks fold their image
// into their row's key.  PASS 1: the above ticks whose image is the key fold their tick into the row's ptick.
template <int PASS>
__global__ __launch_bounds__(EV_THREADS) void gdn_episodes_apply_kernel(EvParams P, void* __restrict__ ws_raw,
                                                                        long long* __restrict__ start,
                                                                        long long* __restrict__ end) {
  __shared__ int sc[EV_THREADS / 64];
  const EvWorkspace W = ev_workspace(ws_raw, P.T, P.E);
  const long long count0 = W.carry->count;
  const long long open_row = W.info->active_out ? W.info->count_out - 1 : -1;
  for (long long tile = blockIdx.x; tile < W.tiles; tile += gridDim.x) {
    const long long tile0 = tile * EV_TILE;
    EvTile<EV_TPT> t;
    ev_tile_events<EV_TPT, false>(t, P, tile0, W.tile[tile], W.tile[W.tiles + tile], W.tile[5 * W.tiles + tile], sc);
    int rel[EV_TPT];
    ev_tile_targets<EV_TPT>(t, P, tile0, W.tile[2 * W.tiles + tile], sc, rel);
    const long long row0 = count0 - 1 + W.tile[6 * W.tiles + tile];      // the row of rel == 0
    const int p0 = threadIdx.x * EV_TPT;
    long long slot[EV_TPT];
    unsigned long long val[EV_TPT];
#pragma unroll
    for (int u = 0; u < EV_TPT; ++u) {
      const long long tick = P.first_tick + tile0 + p0 + u;
      const long long row = row0 + t.opens_excl + __popc(t.openm & ((2u << u) - 1u));   // of an open / a close here
      if (PASS == 0 && ((t.openm >> u) & 1u)) {
        if (row < P.E) start[row] = tick - P.on + 1;
        if (row == open_row) W.info->open_start = tick - P.on + 1;
      }
      if (PASS == 0 && ((t.closem >> u) & 1u) && row < P.E) end[row] = tick - P.off + 1;
      slot[u] = -1;
      val[u] = PASS == 0 ? 0ull : EV_NO_TICK;
      if (rel[u] == -1) continue;
      const long long r = rel[u] == -2 ? -1 : row0 + rel[u];
      slot[u] = rel[u] == -2 ? P.E + 1 : (r < P.E ? r : (r == open_row ? P.E : -1));
      const unsigned long long img = ev_image(t.s[u]);
      if (PASS == 0) val[u] = img;
      else if (slot[u] >= 0 && img == W.key[slot[u]]) val[u] = (unsigned long long)tick;
    }
    ev_fold_thread<EV_TPT, PASS == 0>(PASS == 0 ? W.key : W.ptick, slot, val);
  }
}

// What a slot holds, merged with what the carry knew of the same run: the carried open episode (`from_open`) or the
// carried candidate run (`from_cand`) wins unless a tick of this call is strictly larger.
struct EvPeak {
  double peak;
  long long tick;
  int sensors[8];
};

__device__ inline EvPeak ev_peak_of(const EvParams& P, const int* __restrict__ top_sensors, unsigned long long ptick,
                                    const EvCarry& c, bool from_open, bool from_cand) {
  EvPeak r = {};
  const bool have = ptick != EV_NO_TICK;
  if (have) {
    const long long at = (long long)ptick - P.first_tick;
    r.peak = P.scores[at * P.stride];
    r.tick = (long long)ptick;
    for (int j = 0; j < P.m; ++j) r.sensors[j] = top_sensors[at * P.m + j];
  }
  if (from_open && (!have || !(r.peak > c.open_peak))) {
    r.peak = c.open_peak;
    r.tick = c.open_peak_tick;
    for (int j = 0; j < 8; ++j) r.sensors[j] = c.open_sensors[j];
  } else if (from_cand && (!have || !(r.peak > c.cand_peak))) {
    r.peak = c.cand_peak;
    r.tick = c.cand_tick;
    for (int j = 0; j < 8; ++j) r.sensors[j] = c.cand_sensors[j];
  }
  return r;
}

// Launch 5.  One thread per row this call touched: the peak's bits and sensors from the peak tick's own input row.  The
// last workgroup's thread 0 writes the carry out and the count.
__global__ __launch_bounds__(EV_THREADS) void gdn_episodes_finish_kernel(
    EvParams P, const int* __restrict__ top_sensors, void* __restrict__ ws_raw, const long long* __restrict__ start,
    long long* __restrict__ peak_tick, double* __restrict__ peak, int* __restrict__ sensors, EvCarry* __restrict__ carry_out,
    long long* __restrict__ count) {
  const EvWorkspace W = ev_workspace(ws_raw, P.T, P.E);
  const EvCarry c = *W.carry;
  const EvInfo info = *W.info;
  const bool active0 = c.active != 0, cand0 = !active0 && c.run_hi > 0;
  const long long base = c.count - (active0 ? 1 : 0);
  if (blockIdx.x + 1 < gridDim.x) {
    const long long row = base + (long long)blockIdx.x * EV_THREADS + threadIdx.x;
    if (row >= P.E || row >= info.count_out) return;
    const bool from_open = active0 && row == c.count - 1;
    const bool from_cand = cand0 && row == c.count && start[row] < P.first_tick;
    const EvPeak r = ev_peak_of(P, top_sensors, W.ptick[row], c, from_open, from_cand);
    peak[row] = r.peak;
    peak_tick[row] = r.tick;
    for (int j = 0; j < P.m; ++j) sensors[row * P.m + j] = r.sensors[j];
    return;
  }
  if (threadIdx.x != 0) return;
  if (count) count[0] = info.count_out;
  if (!carry_out) return;
  EvCarry o = {};
  o.count = info.count_out;
  o.active = info.active_out;
  o.run_hi = info.run_hi_out;
  o.run_lo = info.run_lo_out;
  if (info.active_out) {
    const long long row = info.count_out - 1;
    const bool from_open = active0 && row == c.count - 1;
    const bool from_cand = cand0 && row == c.count && info.open_start < P.first_tick;
    const EvPeak r = ev_peak_of(P, top_sensors, W.ptick[row < P.E ? row : P.E], c, from_open, from_cand);
    o.open_start = info.open_start;
    o.open_peak = r.peak;
    o.open_peak_tick = r.tick;
    for (int j = 0; j < 8; ++j) o.open_sensors[j] = r.sensors[j];
  } else if (info.run_hi_out > 0) {
    const EvPeak r = ev_peak_of(P, top_sensors, W.ptick[P.E + 1], c, false, cand0 && info.spans);
    o.cand_peak = r.peak;
    o.cand_tick = r.tick;
    for (int j = 0; j < 8; ++j) o.cand_sensors[j] = r.sensors[j];
  }
  *carry_out = o;
}

// ---- stream form ----------------------------------------------------------------------------------------------------
// One workgroup, one tile of up to 256 * TPT ticks (ev_stream_push).  events = [EvCarry | start[E] | end[E] |
// peak_tick[E] | peak[E] | sensors[E, m]]; the carry is read whole before any of it is written.  Local slot j: the
// episode that is the j-th open of the push (0: the one open before it); SLOTS - 1: the candidate run.  SLOTS = the
// carried episode, at most 256 * TPT / 2 opens, the candidate.  The single stream runs TPT = 16 (4096 ticks, about
// 49 KB of slots); a fleet, whose c is small, instantiates smaller tiles as well (gdn_fleet_events_kernel).
// Comparisons and copies only, so every TPT that covers `count` writes the same bits.  first_tick: state[0].
template <int TPT>
__device__ __forceinline__ void ev_stream_push(const void* __restrict__ state, const double* __restrict__ top_scores,
                                               const int* __restrict__ top_sensors, const double* __restrict__ threshold,
                                               const double* __restrict__ clear, int count, int m, int on, int off,
                                               long long E, long long* __restrict__ events) {
  constexpr int SLOTS = EV_THREADS * TPT / 2 + 2;
  __shared__ unsigned long long key[SLOTS], ptick[SLOTS];
  __shared__ long long lstart[SLOTS];
  __shared__ long long carry_words[EV_CARRY_WORDS];
  __shared__ int sc[EV_THREADS / 64];
  const int tid = threadIdx.x;
  if (tid < EV_CARRY_WORDS) carry_words[tid] = events[tid];
  for (int j = tid; j < SLOTS; j += EV_THREADS) {
    key[j] = 0ull;
    ptick[j] = EV_NO_TICK;
    lstart[j] = 0;
  }
  __syncthreads();
  const EvCarry c = *reinterpret_cast<const EvCarry*>(carry_words);
  long long* __restrict__ t_start = events + EV_CARRY_WORDS;
  long long* __restrict__ t_end = t_start + E;
  long long* __restrict__ t_ptick = t_end + E;
  double* __restrict__ t_peak = reinterpret_cast<double*>(t_ptick + E);
  int* __restrict__ t_sensors = reinterpret_cast<int*>(t_peak + E);
  EvParams P;
  P.scores = top_scores;
  P.stride = m;
  P.T = count;
  P.first_tick = reinterpret_cast<const long long*>(state)[0];
  P.E = E;
  P.hi = threshold[0];
  P.lo = clear[0];
  if (!(P.lo <= P.hi)) P.lo = P.hi;                      // a clear level above the raise level (or NaN) is the raise level
  P.on = on;
  P.off = off;
  P.m = m;
  const bool active0 = c.active != 0, cand0 = !active0 && c.run_hi > 0;
  EvTile<TPT> t;
  ev_tile_events<TPT, false>(t, P, 0, (int)c.run_hi, (int)c.run_lo, active0 ? 1 : 0, sc);
  int rel[TPT];
  ev_tile_targets<TPT>(t, P, 0, 0, sc, rel);
  const long long row0 = c.count - 1;
  const int p0 = tid * TPT;
  const bool active_out = t.last_code < 0 ? active0 : (t.last_code & 3) == 2;
  if (tid == 0 && active0) lstart[0] = c.open_start;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < TPT; ++u) {
    const long long tick = P.first_tick + p0 + u;
    const int j = t.opens_excl + __popc(t.openm & ((2u << u) - 1u));
    if ((t.openm >> u) & 1u) {
      lstart[j] = tick - on + 1;
      if (row0 + j < E) {
        t_start[row0 + j] = tick - on + 1;
        t_end[row0 + j] = -1;
      }
    }
    if (rel[u] != -1) atomicMax(&key[rel[u] == -2 ? SLOTS - 1 : rel[u]], ev_image(t.s[u]));
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < TPT; ++u) {
    const long long tick = P.first_tick + p0 + u;
    const int j = t.opens_excl + __popc(t.openm & ((2u << u) - 1u));
    if (((t.closem >> u) & 1u) && row0 + j < E) t_end[row0 + j] = tick - off + 1;      // (after its open's end = -1)
    if (rel[u] != -1) {
      const int slot = rel[u] == -2 ? SLOTS - 1 : rel[u];
      if (ev_image(t.s[u]) == key[slot]) atomicMin(&ptick[slot], (unsigned long long)tick);
    }
  }
  __syncthreads();
  const int rhi_out = (int)min((long long)on, (long long)(count - 1) - max(t.Lh_tot, -1 - (int)c.run_hi));
  const int rlo_out = (int)min((long long)off, (long long)(count - 1) - max(t.Ll_tot, -1 - (int)c.run_lo));
  EvCarry* __restrict__ out = reinterpret_cast<EvCarry*>(events);
  for (int j = tid; j <= t.opens_total; j += EV_THREADS) {
    if (j == 0 && !active0) continue;
    const long long row = row0 + j;
    const bool from_open = j == 0;
    const bool from_cand = cand0 && j == 1 && lstart[1] < P.first_tick;
    const EvPeak r = ev_peak_of(P, top_sensors, ptick[j], c, from_open, from_cand);
    if (row < E) {
      t_peak[row] = r.peak;
      t_ptick[row] = r.tick;
      for (int q = 0; q < m; ++q) t_sensors[row * m + q] = r.sensors[q];
    }
    if (active_out && j == t.opens_total) {
      out->open_start = lstart[j];
      out->open_peak = r.peak;
      out->open_peak_tick = r.tick;
      for (int q = 0; q < 8; ++q) out->open_sensors[q] = r.sensors[q];
    }
  }
  if (tid == 0) {
    out->count = c.count + t.opens_total;
    out->active = active_out ? 1 : 0;
    out->run_hi = rhi_out;
    out->run_lo = rlo_out;
    EvPeak r = {};
    if (!active_out && rhi_out > 0)
      r = ev_peak_of(P, top_sensors, ptick[SLOTS - 1], c, false, cand0 && t.Lh_tot == EV_NONE);
    out->cand_peak = r.peak;
    out->cand_tick = r.tick;
    for (int q = 0; q < 8; ++q) out->cand_sensors[q] = r.sensors[q];
    if (!active_out) {                                     // (active_out: the loop above wrote the open episode)
      out->open_start = 0;
      out->open_peak = 0.0;
      out->open_peak_tick = 0;
      for (int q = 0; q < 8; ++q) out->open_sensors[q] = 0;
    }
  }
}

__global__ __launch_bounds__(EV_THREADS) void gdn_stream_events_kernel(
    const void* __restrict__ state, const double* __restrict__ top_scores, const int* __restrict__ top_sensors,
    const double* __restrict__ threshold, const double* __restrict__ clear, int count, int m, int on, int off,
    long long E, long long* __restrict__ events) {
  ev_stream_push<EV_STREAM_TPT>(state, top_scores, top_sensors, threshold, clear, count, m, on, off, E, events);
}

// Workgroup u: gdn_stream_events on unit u of a fleet (include/gdn_hip.h "streaming fleet"): its rows of top_scores /
// top_sensors [U, c, m], its threshold and clear level, first_tick from its state block, count = counts[u] clamped to
// 0 .. c (0: the unit's events block is not touched), its block at events + u * ev_words.  TPT: the smallest tile of
// the instantiated ones that covers c, chosen on the host from c alone.
template <int TPT>
__global__ __launch_bounds__(EV_THREADS) void gdn_fleet_events_kernel(
    const void* __restrict__ state, long long state_bytes, const double* __restrict__ top_scores,
    const int* __restrict__ top_sensors, const double* __restrict__ threshold, const double* __restrict__ clear,
    const int* __restrict__ counts, int c, int m, int on, int off, long long E, long long* __restrict__ events,
    long long ev_words) {
  const int u = blockIdx.x;
  const int count = min(max(counts[u], 0), c);
  if (count == 0) return;                                  // (workgroup uniform, ahead of every barrier)
  const size_t row0 = (size_t)u * c * m;
  ev_stream_push<TPT>(reinterpret_cast<const char*>(state) + (size_t)u * (size_t)state_bytes, top_scores + row0,
                      top_sensors + row0, threshold + u, clear + u, count, m, on, off, E, events + (size_t)u * ev_words);
}

bool ev_shape_ok(long long T, int m, int on, int off, long long E) {
  return T >= 1 && T <= EV_MAX_T && m >= 1 && m <= 8 && on >= 1 && on <= EV_MAX_RUN && off >= 1 && off <= EV_MAX_RUN &&
         E >= 0 && E <= EV_MAX_E;
}

template <int TPT>
void fleet_events_launch(const void* state, long long state_bytes, const double* top_scores, const int32_t* top_sensors,
                         const double* threshold, const double* clear, const int32_t* counts, int units, int c, int m,
                         int on, int off, long long E, void* events, long long ev_words, hipStream_t stream) {
  static_assert(TPT <= EV_STREAM_TPT, "no tile beyond the stream's");
  hipLaunchKernelGGL(gdn_fleet_events_kernel<TPT>, dim3((unsigned)units), dim3(EV_THREADS), 0, stream, state, state_bytes,
                     top_scores, top_sensors, threshold, clear, counts, c, m, on, off, E,
                     reinterpret_cast<long long*>(events), ev_words);
}

int episodes_scan(const double* scores, const int32_t* top_sensors, long long T, int m, double hi, double lo, int on,
                  int off, long long first_tick, long long E, const void* carry_in, void* carry_out, int64_t* start,
                  int64_t* end, int64_t* peak_tick, double* peak, int32_t* sensors, int64_t* count, void* workspace,
                  int grid, void* stream) {
  if (!scores || !top_sensors || !workspace || !count) return GDN_ERR_ARG;
  if (!ev_shape_ok(T, m, on, off, E)) return GDN_ERR_UNSUPPORTED;
  if (E > 0 && (!start || !end || !peak_tick || !peak || !sensors)) return GDN_ERR_ARG;
  if (!(lo <= hi) || first_tick < 0 || grid < 0) return GDN_ERR_ARG;      // (a NaN level compares false)
  EvParams P;
  P.scores = scores;
  P.stride = 1;
  P.T = T;
  P.first_tick = first_tick;
  P.E = E;
  P.hi = hi;
  P.lo = lo;
  P.on = on;
  P.off = off;
  P.m = m;
  const long long tiles = (T + EV_TILE - 1) / EV_TILE;
  const long long most = (long long)gdn_cu_count() * 8;
  const unsigned g = (unsigned)(grid > 0 ? (grid < tiles ? grid : tiles) : (tiles < most ? tiles : most));
  const long long reach = T / 2 + 2, rows = reach < E ? reach : E;
  const hipStream_t s = (hipStream_t)stream;
  const EvCarry* cin = reinterpret_cast<const EvCarry*>(carry_in);
  long long* st = reinterpret_cast<long long*>(start);
  long long* en = reinterpret_cast<long long*>(end);
  hipLaunchKernelGGL(gdn_episodes_reduce_kernel, dim3(g), dim3(EV_THREADS), 0, s, P, cin, workspace, en);
  hipLaunchKernelGGL(gdn_episodes_scan_kernel, dim3(1), dim3(EV_THREADS), 0, s, P, cin, workspace);
  hipLaunchKernelGGL(gdn_episodes_apply_kernel<0>, dim3(g), dim3(EV_THREADS), 0, s, P, workspace, st, en);
  hipLaunchKernelGGL(gdn_episodes_apply_kernel<1>, dim3(g), dim3(EV_THREADS), 0, s, P, workspace, st, en);
  hipLaunchKernelGGL(gdn_episodes_finish_kernel, dim3((unsigned)((rows + EV_THREADS - 1) / EV_THREADS) + 1),
                     dim3(EV_THREADS), 0, s, P, top_sensors, workspace, st, reinterpret_cast<long long*>(peak_tick), peak,
                     sensors, reinterpret_cast<EvCarry*>(carry_out), reinterpret_cast<long long*>(count));
  return gdn_launch_status();
}

}  // namespace

extern "C" long long gdn_episodes_workspace_bytes(long long T, long long E) {
  if (T < 1 || T > EV_MAX_T || E < 0 || E > EV_MAX_E) return 0;
  const long long tiles = (T + EV_TILE - 1) / EV_TILE;
  const long long bytes = 8ll * (EV_CARRY_WORDS + EV_INFO_WORDS + 2 * (E + 2)) + 4ll * EV_TILE_INTS * tiles;
  return (bytes + 7) & ~7ll;
}

extern "C" int gdn_episodes_scan(const double* scores, const int32_t* top_sensors, long long T, int m, double hi,
                                 double lo, int on, int off, long long first_tick, long long E, const void* carry_in,
                                 void* carry_out, int64_t* start, int64_t* end, int64_t* peak_tick, double* peak,
                                 int32_t* sensors, int64_t* count, void* workspace, void* stream) {
  return episodes_scan(scores, top_sensors, T, m, hi, lo, on, off, first_tick, E, carry_in, carry_out, start, end,
                       peak_tick, peak, sensors, count, workspace, 0, stream);
}

extern "C" int gdn_episodes_scan_grid(const double* scores, const int32_t* top_sensors, long long T, int m, double hi,
                                      double lo, int on, int off, long long first_tick, long long E,
                                      const void* carry_in, void* carry_out, int64_t* start, int64_t* end,
                                      int64_t* peak_tick, double* peak, int32_t* sensors, int64_t* count,
                                      void* workspace, int grid, void* stream) {
  return episodes_scan(scores, top_sensors, T, m, hi, lo, on, off, first_tick, E, carry_in, carry_out, start, end,
                       peak_tick, peak, sensors, count, workspace, grid, stream);
}

extern "C" long long gdn_stream_events_bytes(int m, long long E) {
  if (m < 1 || m > 8 || E < 0 || E > EV_MAX_E) return 0;
  const long long bytes = GDN_EPISODES_CARRY_BYTES + 32ll * E + 4ll * E * m;
  return (bytes + 7) & ~7ll;
}

extern "C" int gdn_stream_events(const void* state, const double* top_scores, const int32_t* top_sensors,
                                 const double* threshold, const double* clear, int c, int count, int m, int on, int off,
                                 long long E, void* events, void* stream) {
  if (!state || !top_scores || !top_sensors || !threshold || !clear || !events || count < 1 || count > c)
    return GDN_ERR_ARG;
  if (c > EV_STREAM_MAX || !ev_shape_ok(count, m, on, off, E)) return GDN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gdn_stream_events_kernel, dim3(1), dim3(EV_THREADS), 0, (hipStream_t)stream, state, top_scores,
                     top_sensors, threshold, clear, count, m, on, off, E, reinterpret_cast<long long*>(events));
  return gdn_launch_status();
}

extern "C" long long gdn_fleet_events_bytes(int units, int m, long long E) {
  if (units < 1 || units > GDN_FLEET_MAX_ROWS) return 0;
  return (long long)units * gdn_stream_events_bytes(m, E);
}

// The tile follows c alone (known on the host, captured): 256, 1024 or the stream's 4096 ticks.
extern "C" int gdn_fleet_events(const void* state, const double* top_scores, const int32_t* top_sensors,
                                const double* threshold, const double* clear, const int32_t* counts, int units, int c,
                                int n, int w, int m, int on, int off, long long E, void* events, void* stream) {
  if (!state || !top_scores || !top_sensors || !threshold || !clear || !counts || !events) return GDN_ERR_ARG;
  const long long state_bytes = gdn_stream_state_bytes(n, w);                    // 0: no such stream shape
  if (!gdn_fleet_rows_ok(units, c) || state_bytes <= 0) return GDN_ERR_UNSUPPORTED;
  if (!ev_shape_ok(c, m, on, off, E)) return GDN_ERR_UNSUPPORTED;
  const long long ev_words = gdn_stream_events_bytes(m, E) / 8;
  const hipStream_t s = (hipStream_t)stream;
  if (c <= EV_THREADS)
    fleet_events_launch<1>(state, state_bytes, top_scores, top_sensors, threshold, clear, counts, units, c, m, on, off,
                           E, events, ev_words, s);
  else if (c <= EV_THREADS * 4)
    fleet_events_launch<4>(state, state_bytes, top_scores, top_sensors, threshold, clear, counts, units, c, m, on, off,
                           E, events, ev_words, s);
  else
    fleet_events_launch<EV_STREAM_TPT>(state, state_bytes, top_scores, top_sensors, threshold, clear, counts, units, c,
                                       m, on, off, E, events, ev_words, s);
  return gdn_launch_status();
}
