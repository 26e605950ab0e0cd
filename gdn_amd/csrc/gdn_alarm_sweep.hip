// Alarm tuning (include/gdn_hip.h "Alarm tuning"): the episodes of P alarm settings (hi, lo, on, off)
// over ONE scored series, each matched against the labelled incidents and reduced to eight integer counters.
// Comparisons and integer counts only, so the result equals the sequential definition bit for bit.
//
// One launch.  A lane is a setting, a workgroup is one wave, and the wave walks the ticks in order with the tick index
// uniform: a score or a label is one uniform read shared by the 64 settings, the incident bookkeeping (the current
// incident's id and begin tick, the running count of labelled ticks) is scalar, and a setting's state lives in
// registers.  No workgroup waits on another; no atomics, no workspace.  The per-tick update is selects only: the lanes
// of a wave hold different `on` / `off`, so their events fall on different ticks.
//
// An episode's span is backdated at both ends — it starts on - 1 ticks before the raise and ends off - 1 ticks before
// the clear — which a constant-size state per lane carries:
//   rh / rl         the runs of above / below ticks (not saturated: a run is at most T < 2^31 ticks long);
//   hi_base/lo_base the number of labelled ticks up to the last tick that was not above / not below, so that
//                   labelled(span) = labels_upto(end - 1) - labels_upto(start - 1) needs no prefix array;
//   the tentative tallies of the ticks whose membership is not decided yet — while idle the current above-run (it is in
//   the span iff it goes on to raise), while active the current below-run (it is in the span iff it breaks before
//   `off`): incidents touched for the first time (t_cnt), the sum of their delays so far (t_delay, aged by t_cnt every
//   tick), the earliest of their begins (t_first) and the id of the last incident seen (seen);
//   last_hit        the id of the last incident counted for good: incident ids ascend, so "id > last_hit" is "new".
// The tallies are committed at the raise and at every active tick that is not below; they are dropped when an idle
// run breaks and when the episode clears.  An incident first met after the raise began after it: its delay is 0.
// alarm_ticks needs no per-episode arithmetic: the ticks with `active` set, plus (on - 1) per episode, minus (off - 1)
// per cleared episode.
#include "gdn_common.hpp"

namespace {

constexpr int AS_LANES = 64;
constexpr int AS_UNROLL = 8;                               // ticks per iteration: 64 B of scores, 8 B of labels
constexpr int AS_MAX_RUN = 4096;
constexpr long long AS_MAX_T = 1ll << 26;
constexpr long long AS_MAX_P = 1ll << 20;
constexpr int AS_NO_BEGIN = 0x7fffffff;

struct AsUniform {                // the same in every lane: the labels' side of a tick
  int prev;                       // the previous tick was labelled
  int inc;                        // id of the latest incident that has begun (-1: none yet)
  int begin;                      // its first tick
  int labelled;                   // labelled ticks so far, this one included
};

struct AsLane {                   // one setting
  double hi, lo;
  int on, off;
  int rh, rl, active;
  int hi_base, lo_base, ep_base;
  int t_cnt, t_delay, t_first, seen, last_hit;
  int episodes, true_episodes, hit, delay_max, active_ticks, label_ticks, cleared;
  long long delay_sum;
};

__device__ __forceinline__ void as_tick(AsLane& s, AsUniform& u, int t, double score, int label) {
  if (label && !u.prev) {
    ++u.inc;
    u.begin = t;
  }
  u.prev = label;
  u.labelled += label;
  const bool above = score > s.hi, below = !(score > s.lo);
  const bool was = s.active != 0;
  s.rh = above ? s.rh + 1 : 0;
  s.rl = below ? s.rl + 1 : 0;
  const bool set = !was & (s.rh >= s.on), rst = was & (s.rl >= s.off);   // (& and |: mask logic, no branch)
  const bool commit = (was & !below) | set;
  const bool keep = (was & below & !rst) | (!was & above & !set);
  s.hi_base = above ? s.hi_base : u.labelled;
  s.lo_base = below ? s.lo_base : u.labelled;
  // the tentative tallies: every incident in them is one tick older, then this tick's own incident
  s.t_delay += s.t_cnt;
  if (label) {                                             // (uniform)
    const bool touch = (was | above) & (u.inc > s.seen);
    s.t_cnt += touch ? 1 : 0;
    s.t_delay += touch ? t - u.begin : 0;
    s.t_first = touch ? min(s.t_first, u.begin) : s.t_first;
    s.seen = touch ? u.inc : s.seen;
  }
  s.hit += commit ? s.t_cnt : 0;
  s.last_hit = commit ? s.seen : s.last_hit;
  s.delay_sum += set ? (long long)(unsigned)s.t_delay : 0ll;
  s.delay_max = set ? max(s.delay_max, t - s.t_first) : s.delay_max;
  s.t_cnt = keep ? s.t_cnt : 0;
  s.t_delay = keep ? s.t_delay : 0;
  s.t_first = keep ? s.t_first : AS_NO_BEGIN;
  s.seen = keep ? s.seen : s.last_hit;
  // the episode table's side: a raise opens at the labelled count before the run, a clear closes at the one before it
  s.episodes += set ? 1 : 0;
  s.ep_base = set ? s.hi_base : s.ep_base;
  s.label_ticks += set ? -s.hi_base : (rst ? s.lo_base : 0);
  s.true_episodes += (rst & (s.lo_base > s.ep_base)) ? 1 : 0;
  s.cleared += rst ? 1 : 0;
  s.active = set ? 1 : (rst ? 0 : s.active);
  s.active_ticks += s.active;
}

__global__ __launch_bounds__(AS_LANES) void gdn_alarm_sweep_kernel(
    const double* __restrict__ scores, const uint8_t* __restrict__ labels, int T, const double* __restrict__ hi,
    const double* __restrict__ lo, const int* __restrict__ on, const int* __restrict__ off, long long P,
    long long* __restrict__ counts) {
  const long long p = (long long)blockIdx.x * AS_LANES + threadIdx.x;
  const long long row = p < P ? p : P - 1;                 // a lane beyond P repeats the last setting and stores nothing
  AsLane s = {};
  s.hi = hi[row];
  s.lo = lo[row];
  s.on = on[row];
  s.off = off[row];
  s.t_first = AS_NO_BEGIN;
  s.seen = s.last_hit = -1;
  const bool valid = s.lo <= s.hi && s.on >= 1 && s.on <= AS_MAX_RUN && s.off >= 1 && s.off <= AS_MAX_RUN;
  AsUniform u = {0, -1, 0, 0};
  // single ticks up to the first one whose label byte is 8-byte aligned, then AS_UNROLL ticks per iteration, then the rest
  const int lead = (int)((0 - (unsigned long long)(uintptr_t)labels) & 7ull);
  int t = 0;
  const int head = lead < T ? lead : T;
  for (; t < head; ++t) as_tick(s, u, t, scores[t], labels[t] != 0);
  const int blocks = (T - t) / AS_UNROLL;
  for (int b = 0; b < blocks; ++b, t += AS_UNROLL) {
    const unsigned long long lw = *reinterpret_cast<const unsigned long long*>(labels + t);
    double sv[AS_UNROLL];
#pragma unroll
    for (int q = 0; q < AS_UNROLL; ++q) sv[q] = scores[t + q];
#pragma unroll
    for (int q = 0; q < AS_UNROLL; ++q) as_tick(s, u, t + q, sv[q], ((lw >> (8 * q)) & 0xffull) != 0ull);
  }
  for (; t < T; ++t) as_tick(s, u, t, scores[t], labels[t] != 0);
  if (p >= P) return;
  // an episode open at the last tick ends at T: its trailing below-run and everything labelled up to T are in the span
  const int open = s.active;
  long long out[8];
  out[0] = s.episodes;
  out[1] = s.true_episodes + ((open && u.labelled > s.ep_base) ? 1 : 0);
  out[2] = s.hit + (open ? s.t_cnt : 0);
  out[3] = s.delay_sum;
  out[4] = s.delay_max;
  out[5] = (long long)s.active_ticks + (long long)s.episodes * (s.on - 1) - (long long)s.cleared * (s.off - 1);
  out[6] = s.label_ticks + (open ? u.labelled : 0);
  out[7] = open;
#pragma unroll
  for (int q = 0; q < 8; ++q) counts[p * 8 + q] = valid ? out[q] : -1ll;
}

}  // namespace

extern "C" int gdn_alarm_sweep(const double* scores, const uint8_t* labels, long long T, const double* hi,
                               const double* lo, const int32_t* on, const int32_t* off, long long P, int64_t* counts,
                               void* stream) {
  if (!scores || !labels || !hi || !lo || !on || !off || !counts) return GDN_ERR_ARG;
  if (T < 1 || T > AS_MAX_T || P < 1 || P > AS_MAX_P) return GDN_ERR_UNSUPPORTED;
  const unsigned grid = (unsigned)((P + AS_LANES - 1) / AS_LANES);
  hipLaunchKernelGGL(gdn_alarm_sweep_kernel, dim3(grid), dim3(AS_LANES), 0, (hipStream_t)stream, scores, labels, (int)T,
                     hi, lo, on, off, P, reinterpret_cast<long long*>(counts));
  return gdn_launch_status();
}
