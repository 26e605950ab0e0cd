// Anomaly scoring on device, float64 like the reference (evaluate.py:48-68, util/data.py:75-82,
// evaluate.py:131-139).  numpy evaluates  a + d*t  and  (x - m) / (|r| + eps)  as separate
// roundings, so FMA contraction is switched off for this file.
#pragma clang fp contract(off)
#include "gdn_score_sweep.hpp"

#include <stdlib.h>

namespace {

using namespace gdn_sweep;

constexpr int NQ = 6;  // order statistics per sensor: median lo/hi, q25 lo/hi, q75 lo/hi

struct SelectArgs {
  int rank[NQ];      // 0-based ranks in the ascending order of |pred-gt|
  double gamma[2];   // interpolation weights of the 25th / 75th percentile (numpy 'linear')
  int median_pair;   // 1: t even, median = mean of two middle values
  int total;         // real keys per sensor
  int bracket;       // the one-workgroup flat select first tries the sample brackets (select_onewg_kernel): 0 no,
                     // 1 the three-interval tier only, 2 the one-span tier in front of it
};

// Ranks, interpolation weights and median rule of a sensor with t >= 1 real keys.  ONE function for the host
// (make_select_args: the same t for every sensor) and the device (gdn_score_select_counts: t = counts[s]): the same
// float64 operations in the same order, no contraction in this file, hence the same bits.
__host__ __device__ inline void fill_select_args(SelectArgs& sa, long long t) {
  // np.median: middle value, or the mean of the two middle values when t is even
  sa.median_pair = (t % 2 == 0);
  sa.rank[0] = (int)(sa.median_pair ? t / 2 - 1 : (t - 1) / 2);
  sa.rank[1] = (int)(sa.median_pair ? t / 2 : (t - 1) / 2);
  // np.percentile(method='linear'): virtual index n*q + (alpha + q*(1-alpha-beta)) - 1, alpha=beta=1
  const double qs[2] = {25.0 / 100.0, 75.0 / 100.0};
  for (int h = 0; h < 2; ++h) {
    const double vi = (double)t * qs[h] + (1.0 + qs[h] * (1.0 - 1.0 - 1.0)) - 1.0;
    const double lo = floor(vi);
    long long ilo = (long long)lo, ihi = ilo + 1;
    if (ilo < 0) ilo = 0;
    if (ihi > t - 1) ihi = t - 1;
    if (ilo > t - 1) ilo = t - 1;
    sa.rank[2 + 2 * h] = (int)ilo;
    sa.rank[3 + 2 * h] = (int)ihi;
    sa.gamma[h] = vi - lo;
  }
  sa.total = (int)t;
}

// gdn_score_select_counts: what the kernels get in SelectArgs' place.  Sensor s has counts[s] real keys; its
// SelectArgs are formed on the device by select_args_for (one thread, handed to the workgroup through LDS: a
// workgroup is one sensor, so every test on them stays uniform).  A sensor with fewer than max(min_count, 1) real keys
// keeps its med_iqr row: total = 0 marks it.
struct CountArgs {
  const int* counts;   // [n] on the device
  int min_count;
  int bracket;
};

// The kernels below take their rank arguments as a template type: SelectArgs (the instantiations behind
// gdn_score_select / _paths / gdn_score_quantiles: the kernel argument itself, nothing added) or CountArgs.
__device__ __forceinline__ const SelectArgs& select_args_for(const SelectArgs& sa, int) { return sa; }
template <typename ARGS> constexpr bool kPerSensor = false;
template <> constexpr bool kPerSensor<CountArgs> = true;

__device__ __forceinline__ const SelectArgs& select_args_for(const CountArgs& ca, int s) {
  __shared__ SelectArgs sh;
  if (threadIdx.x == 0) {
    const int c = ca.counts[s];
    if (c >= 1 && c >= ca.min_count) {
      fill_select_args(sh, c);
    } else {
      for (int q = 0; q < 6; ++q) sh.rank[q] = 0;
      sh.gamma[0] = sh.gamma[1] = 0.0;
      sh.median_pair = 0;
      sh.total = 0;
    }
    sh.bracket = ca.bracket;
  }
  __syncthreads();
  return sh;
}

// keys[s][tick] = |pred[tick][s] - gt[tick][s]| in float64 (bit pattern = radix key), transposed
// through LDS so that both the fp32 reads (along sensors) and the fp64 writes (along ticks) are
// coalesced.  Row pitch >= t; slots t..pitch-1 get the FILLER pattern (gdn_score_sweep.hpp).

__global__ __launch_bounds__(256) void score_keys_kernel(const float* __restrict__ pred,
                                                         const float* __restrict__ gt, int t, int n, int pitch,
                                                         double* __restrict__ keys) {
  __shared__ double tile[64][65];
  const int t0 = blockIdx.x * 64, s0 = blockIdx.y * 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int r = wv; r < 64; r += 4) {
    const int tick = t0 + r, s = s0 + lane;
    if (tick < t && s < n) {
      const size_t o = (size_t)tick * n + s;
      tile[r][lane] = score_key(pred[o], gt[o]);
    }
  }
  __syncthreads();
  for (int r = wv; r < 64; r += 4) {
    const int s = s0 + r, tick = t0 + lane;
    if (s < n && tick < pitch)
      keys[(size_t)s * pitch + tick] = tick < t ? tile[lane][r] : filler_key();
  }
}

// score_keys_kernel with a validity plane (gdn_score_keys_valid): key (s, tick) is the filler wherever
// valid[tick, s] == 0.  The validity byte is read next to the value and travels through the tile AS the value: a
// missing reading's tile entry is the filler pattern itself, so the second half is score_keys_kernel's.
__global__ __launch_bounds__(256) void score_keys_valid_kernel(const float* __restrict__ pred,
                                                               const float* __restrict__ gt,
                                                               const unsigned char* __restrict__ valid, int t, int n,
                                                               int pitch, double* __restrict__ keys) {
  __shared__ double tile[64][65];
  const int t0 = blockIdx.x * 64, s0 = blockIdx.y * 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int r = wv; r < 64; r += 4) {
    const int tick = t0 + r, s = s0 + lane;
    if (tick < t && s < n) {
      const size_t o = (size_t)tick * n + s;
      const double e = score_key(pred[o], gt[o]);
      tile[r][lane] = valid[o] != 0 ? e : filler_key();
    }
  }
  __syncthreads();
  for (int r = wv; r < 64; r += 4) {
    const int s = s0 + r, tick = t0 + lane;
    if (s < n && tick < pitch)
      keys[(size_t)s * pitch + tick] = tick < t ? tile[lane][r] : filler_key();
  }
}

// counts[s] = slots of sensor s that do not hold the filler (gdn_score_key_counts).  A workgroup per sensor walks the
// sensor's `blocks` rows; register adds, a wave reduction, one integer LDS add per wave, one store.
__global__ __launch_bounds__(256) void score_key_counts_kernel(const unsigned long long* __restrict__ keys, int blocks,
                                                               int n, int pitch, int* __restrict__ counts) {
  __shared__ int total;
  const int s = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) total = 0;
  __syncthreads();
  int mine = 0;
  for (int b = 0; b < blocks; ++b) {
    const unsigned long long* row = keys + ((size_t)b * n + s) * pitch;
    for (int i = tid; i < pitch; i += 256) mine += row[i] != FILLER ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
  if ((tid & 63) == 0) atomicAdd(&total, mine);
  __syncthreads();
  if (tid == 0) counts[s] = total;
}

// ------------------------------------------------------------------ radix select
// Exact order statistics by an MSB-first 8-bit radix select of NQ ranks per sensor (non-negative
// doubles order like their bit patterns), spread over the whole chip.
//
// Input layout: keys[blocks][n][pitch] — `blocks` row blocks as they arrive from `blocks` ranks in
// the multi-GPU exchange (one block, pitch = t, on a single GPU); sensor s owns blocks*pitch SLOTS,
// of which `total` hold real keys and the rest the FILLER.  The input is never written.
//
// Digits 0-1 (the exponent bytes) and 2: one launch per digit, grid = (2048-slot slices, sensors);
// a block keeps its slice in registers (8 keys per thread), histograms the digit of the keys that
// still match some rank's prefix in LDS (a wave landing in one bin adds 64 at once), adds its
// non-empty bins to the sensor's global histogram and takes a ticket; the LAST block of a sensor
// (no spinning, no fences: every consumed value is an agent-scope atomic) locates every rank's bin
// and extends the prefixes for the next launch.  The digit-2 launch also compacts the matching keys
// (normally a few percent) into the workspace, and one single-block finisher launch per sensor does
// digits 3-7 on those.
constexpr int SLICE = 2048;

struct SelState {
  unsigned long long prefix[NQ];
  int rem[NQ];
  int rep[NQ];
  unsigned int hist[NQ][256];
  unsigned int arrive;
  unsigned int cnt_b;     // keys compacted into the workspace buffer
  unsigned int digits_done;   // digits the prefixes hold: pass 0 also settles digit 1 when it can (see select_pass_kernel)
  unsigned int pad1;
};

struct KeyLayout {
  const unsigned long long* keys;   // [blocks][n][pitch]
  unsigned long long* bufb;         // [n][blocks*pitch] compacted survivors
  int blocks, n, pitch;
};

template <typename ARGS>
__global__ void select_init_kernel(SelState* __restrict__ state, const ARGS args) {
  SelState& st = state[blockIdx.x];
  const SelectArgs& sa = select_args_for(args, blockIdx.x);
  for (int i = threadIdx.x; i < NQ * 256; i += blockDim.x) (&st.hist[0][0])[i] = 0u;
  if (threadIdx.x < NQ) {
    st.prefix[threadIdx.x] = 0ull;
    st.rem[threadIdx.x] = sa.rank[threadIdx.x];
    st.rep[threadIdx.x] = 0;
  }
  if (threadIdx.x == 0) {
    st.arrive = 0u;
    st.cnt_b = 0u;
    st.digits_done = 0u;
  }
}

// wave q's lanes find the bin of rank q in a 256-bin histogram; returns through npf / nrem
__device__ __forceinline__ void locate_bin(const unsigned int* h, int left0, unsigned long long pf, int shift,
                                           int lane, unsigned long long* npf, int* nrem) {
  const uint4 c4 = *reinterpret_cast<const uint4*>(h + 4 * lane);
  const int mine = (int)(c4.x + c4.y + c4.z + c4.w);
  int incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  const int excl = incl - mine;
  if (left0 >= excl && left0 < incl) {
    int left = left0 - excl, bin = 0;
    const int c[4] = {(int)c4.x, (int)c4.y, (int)c4.z, (int)c4.w};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (bin == j && left >= c[j]) {
        left -= c[j];
        bin = j + 1;
      }
    }
    *npf = pf | ((unsigned long long)(4 * lane + bin) << shift);
    *nrem = left;
  }
}

// the same over 512 bins (8 per lane) for the bracket path of select_onewg_kernel: a wave finds the bin that holds
// position left0 and writes code0 + bin and the position inside the bin; NOTHING is written when left0 lies outside
// [0, sum of h): that is how a rank outside its bracket shows
__device__ __forceinline__ void locate_bin512(const unsigned int* h, int left0, unsigned int code0, int lane,
                                              unsigned int* code, int* nrem) {
  const uint4 a = *reinterpret_cast<const uint4*>(h + 8 * lane);
  const uint4 b = *reinterpret_cast<const uint4*>(h + 8 * lane + 4);
  const int c[8] = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y, (int)b.z, (int)b.w};
  int mine = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) mine += c[j];
  int incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  const int excl = incl - mine;
  if (left0 >= excl && left0 < incl) {
    int left = left0 - excl, bin = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      if (bin == j && left >= c[j]) {
        left -= c[j];
        bin = j + 1;
      }
    }
    *code = code0 + (unsigned int)(8 * lane + bin);
    *nrem = left;
  }
}

// the same over the 2048 bins of the one-span tier (32 per lane): the lane that holds position left0 first walks its
// eight 4-bin groups, then the four bins of the group (one more LDS read); code = the bin, nothing written outside
__device__ __forceinline__ void locate_bin2048(const unsigned int* h, int left0, int lane, unsigned int* code,
                                               int* nrem) {
  int g[8];
  int mine = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint4 a = *reinterpret_cast<const uint4*>(h + 32 * lane + 4 * j);
    g[j] = (int)(a.x + a.y + a.z + a.w);
    mine += g[j];
  }
  int incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  const int excl = incl - mine;
  if (left0 >= excl && left0 < incl) {
    int left = left0 - excl, grp = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      if (grp == j && left >= g[j]) {
        left -= g[j];
        grp = j + 1;
      }
    }
    const uint4 a = *reinterpret_cast<const uint4*>(h + 32 * lane + 4 * grp);
    const int c[4] = {(int)a.x, (int)a.y, (int)a.z, (int)a.w};
    int bin = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (bin == j && left >= c[j]) {
        left -= c[j];
        bin = j + 1;
      }
    }
    *code = (unsigned int)(32 * lane + 4 * grp + bin);
    *nrem = left;
  }
}

__device__ __forceinline__ void write_result(const unsigned long long* prefix, const SelectArgs& sa, int s,
                                             double* __restrict__ med_iqr) {
  double v[NQ];
  for (int q = 0; q < NQ; ++q) v[q] = __longlong_as_double((long long)prefix[q]);
  const double med = sa.median_pair ? (v[0] + v[1]) / 2.0 : v[0];
  double qv[2];
  for (int h = 0; h < 2; ++h) {   // numpy _lerp
    const double a = v[2 + 2 * h], b = v[3 + 2 * h], gm = sa.gamma[h];
    const double diff = b - a;
    double r = a + diff * gm;
    if (gm >= 0.5) r = b - diff * (1.0 - gm);
    qv[h] = r;
  }
  med_iqr[2 * s] = med;
  med_iqr[2 * s + 1] = qv[1] - qv[0];
}

// FROM_B: read the compacted workspace buffer (flat) instead of the blocked input.
// COMPACT: also write the matching keys to the workspace buffer.
template <bool FROM_B, bool COMPACT>
__global__ __launch_bounds__(256) void select_pass_kernel(const KeyLayout kl, SelState* __restrict__ state,
                                                          int pass) {
  __shared__ unsigned int hist[NQ][256];
  __shared__ unsigned long long stage[COMPACT ? SLICE : 1];
  __shared__ unsigned int n_stage, out_base, ticket_s;
  __shared__ unsigned long long npf[NQ];
  __shared__ int nrem[NQ];
  const int s = blockIdx.y, g = blockIdx.x, G = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  SelState& st = state[s];
  // Pass 0 usually settles TWO digits: the errors of a sensor almost always share the top byte of their keys (sign
  // + 7 exponent bits), so next to the histogram of byte 0 it histograms byte 1 of the keys whose byte 0 equals that
  // of the sensor's first key; if every quantile's rank falls into that byte-0 bin the last workgroup locates
  // digit 1 as well and the pass-1 launch returns at once (it is still launched: the sequence is captured in
  // graphs).  One streaming pass over the keys less: 14.5 -> ~5 us of an 86 us select at the 8-rank shape.
  if (!FROM_B && !COMPACT && pass == 1 && st.digits_done >= 2u) return;
  const unsigned int slots = (unsigned int)kl.blocks * (unsigned int)kl.pitch;
  const unsigned int cnt = FROM_B ? st.cnt_b : slots;
  unsigned long long* outb = kl.bufb + (size_t)s * slots;
  const int shift = 56 - 8 * pass;
  const bool two = !FROM_B && !COMPACT && pass == 0;                    // uniform
  const unsigned int dref = two ? (unsigned int)(kl.keys[(size_t)s * kl.pitch] >> 56) : 0u;   // block 0, slot 0
  unsigned long long pf[NQ];
  bool active[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    pf[q] = st.prefix[q];
    active[q] = st.rep[q] == q;
  }
  for (int i = tid; i < NQ * 256; i += 256) (&hist[0][0])[i] = 0u;
  if (tid == 0) n_stage = 0u;
  __syncthreads();

  // a block walks slices g, g+G, ... (any count stays correct when fewer blocks are launched)
  for (unsigned int base = (unsigned int)g * SLICE; base < cnt; base += (unsigned int)G * SLICE) {
    // slice -> memory: blocked input (a slice never straddles two blocks: pitch % SLICE == 0 when
    // blocks > 1) or the flat workspace buffer
    const unsigned long long* in;
    unsigned int lim;   // valid slots of this slice's row, from `base`
    if (FROM_B) {
      in = outb + base;
      lim = cnt - base;
    } else {
      const unsigned int blk = base / (unsigned int)kl.pitch, off = base - blk * (unsigned int)kl.pitch;
      in = kl.keys + ((size_t)blk * kl.n + s) * kl.pitch + off;
      lim = (unsigned int)kl.pitch - off;
    }
    unsigned long long key[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned int i = tid + u * 256;
      key[u] = i < lim ? in[i] : FILLER;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool real = key[u] != FILLER;
      const unsigned int digit = (unsigned int)(key[u] >> shift) & 255u;
      const unsigned int d0 = __builtin_amdgcn_readfirstlane(digit);
      bool any = false;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (!active[q]) continue;   // uniform
        const bool match = real && (pass == 0 ? true : ((key[u] ^ pf[q]) >> (shift + 8)) == 0ull);
        any |= match;
        if (__all(match && digit == d0)) {
          if (lane == 0) atomicAdd(&hist[q][d0], 64u);
        } else if (match) {
          atomicAdd(&hist[q][digit], 1u);
        }
      }
      if constexpr (COMPACT) {
        if (any) stage[atomicAdd(&n_stage, 1u)] = key[u];
      }
      if (two && real && digit == dref) atomicAdd(&hist[1][(unsigned int)(key[u] >> 48) & 255u], 1u);
    }
    if constexpr (COMPACT) {
      __syncthreads();
      if (tid == 0) out_base = n_stage ? atomicAdd(&st.cnt_b, n_stage) : 0u;
      __syncthreads();
      for (unsigned int i = tid; i < n_stage; i += 256) outb[out_base + i] = stage[i];
      __syncthreads();
      if (tid == 0) n_stage = 0u;
      __syncthreads();
    }
  }
  __syncthreads();
  for (int i = tid; i < NQ * 256; i += 256) {
    const unsigned int c = (&hist[0][0])[i];
    if (c) atomicAdd(&(&st.hist[0][0])[i], c);
  }
  // Hand-off without fences: every value the last block consumes (histogram bins, survivor count)
  // is an agent-scope ATOMIC performed at the device coherence point; each wave waits for its own
  // atomics to be acknowledged, the barrier orders all waves before the ticket, and the last block
  // reads the totals back with atomic exchanges (which also re-zero them).  The compacted keys are
  // plain stores: only the NEXT launch reads them.  (A __threadfence() here costs a full L2
  // write-back per block: 150 us per pass with 2000 blocks.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) ticket_s = atomicAdd(&st.arrive, 1u);
  __syncthreads();
  if (ticket_s != (unsigned int)(G - 1)) return;

  // ---- last block of this sensor
  for (int i = tid; i < NQ * 256; i += 256) (&hist[0][0])[i] = atomicExch(&(&st.hist[0][0])[i], 0u);
  __syncthreads();
  for (int q = wv; q < NQ; q += 4) locate_bin(hist[st.rep[q]], st.rem[q], pf[q], shift, lane, &npf[q], &nrem[q]);
  __syncthreads();
  unsigned int done = (unsigned int)pass + 1u;
  if (two) {
    bool inside = dref != 255u;                                  // (255: the filler's byte)
    for (int q = 0; q < NQ; ++q) inside = inside && (unsigned int)(npf[q] >> 56) == dref;
    if (inside) {                                                // uniform: digit 1 from the conditional histogram
      __shared__ unsigned long long npf2[NQ];
      __shared__ int nrem2[NQ];
      for (int q = wv; q < NQ; q += 4) locate_bin(hist[1], nrem[q], npf[q], shift - 8, lane, &npf2[q], &nrem2[q]);
      __syncthreads();
      if (tid < NQ) {
        npf[tid] = npf2[tid];
        nrem[tid] = nrem2[tid];
      }
      __syncthreads();
      done = 2u;
    }
  }
  if (tid < NQ) {
    st.prefix[tid] = npf[tid];
    st.rem[tid] = nrem[tid];
    int r = tid;
    for (int q = tid - 1; q >= 0; --q)
      if (npf[q] == npf[tid]) r = q;
    st.rep[tid] = r;
  }
  if (tid == 0) {
    st.digits_done = done;
    atomicExch(&st.arrive, 0u);
  }
}

// 1024 threads x 32 keys: up to 32768 survivors stay in registers.  With 8 ranks a sensor has 262144 keys and a 16-bit
// prefix bin keeps ~3 % of them per quantile: ~24 k survivors, which the 256-thread / 4096-key form re-read from
// memory in each of its five passes (176 us of a 230 us select; 18 us now: tools/probe_select_sharded.py).
constexpr int FIN_NT = 1024;
// Finisher: digits first_pass..7 of every rank in ONE launch, one block per sensor, no global
// hand-offs.  Reads the compacted buffer (FROM_B) — normally a handful of keys, <= 2048 stay in
// registers (<= 4096), more (e.g. thousands of identical values) are re-read per digit — or, for inputs of a
// single slice, the flat input itself.
template <bool FROM_B, typename ARGS>
__global__ __launch_bounds__(FIN_NT) void select_finish_kernel(const KeyLayout kl, SelState* __restrict__ state,
                                                            int first_pass, const ARGS args,
                                                            double* __restrict__ med_iqr) {
  __shared__ unsigned int hist[NQ][256];
  __shared__ unsigned long long prefix[NQ];
  __shared__ int rem[NQ];
  __shared__ int rep[NQ];
  const int s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const SelectArgs& sa = select_args_for(args, s);
  if constexpr (kPerSensor<ARGS>) {
    if (sa.total < 1) return;                // (uniform) too few real keys: the row stays as it is
  }
  SelState& st = state[s];
  const unsigned int slots = (unsigned int)kl.blocks * (unsigned int)kl.pitch;
  const unsigned int cnt = FROM_B ? st.cnt_b : slots;
  const unsigned long long* in = FROM_B ? kl.bufb + (size_t)s * slots : kl.keys + (size_t)s * kl.pitch;
  if (tid < NQ) {
    prefix[tid] = st.prefix[tid];
    rem[tid] = st.rem[tid];
  }
  constexpr int FK = 32;                      // keys per thread the finisher keeps in registers
  const bool resident = cnt <= FK * FIN_NT;
  unsigned long long key[FK];
  if (resident) {
#pragma unroll
    for (int u = 0; u < FK; ++u) {
      const unsigned int i = tid + u * FIN_NT;
      key[u] = i < cnt ? in[i] : FILLER;
    }
  }
  __syncthreads();
  for (int pass = first_pass; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    if (tid < NQ) {
      int r = tid;
      for (int q = tid - 1; q >= 0; --q)
        if (prefix[q] == prefix[tid]) r = q;
      rep[tid] = r;
    }
    for (int i = tid; i < NQ * 256; i += FIN_NT) (&hist[0][0])[i] = 0u;
    __syncthreads();
    unsigned long long pf[NQ];
    bool active[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      pf[q] = prefix[q];
      active[q] = rep[q] == q;
    }
    // returns false when the key matches no rank's prefix any more (it never will again)
    auto tally = [&](unsigned long long k) -> bool {
      if (k == FILLER) return false;
      const unsigned int digit = (unsigned int)(k >> shift) & 255u;
      bool any = false;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (!active[q]) continue;
        if (pass == 0 || ((k ^ pf[q]) >> (shift + 8)) == 0ull) {
          atomicAdd(&hist[q][digit], 1u);
          any = true;
        }
      }
      return any;
    };
    if (resident) {
      // a key that matched nothing is dropped from the register set: the later passes skip it with one compare
      // (24 k survivors x 6 ranks x 5 passes of 64-bit shifts were 60 of the finisher's 67 us)
#pragma unroll
      for (int u = 0; u < FK; ++u)
        if (!tally(key[u])) key[u] = FILLER;
    } else {
      for (unsigned int i = tid; i < cnt; i += FIN_NT) tally(in[i]);
    }
    __syncthreads();
    for (int q = wv; q < NQ; q += FIN_NT / 64) locate_bin(hist[rep[q]], rem[q], pf[q], shift, lane, &prefix[q], &rem[q]);
    __syncthreads();
  }
  if (tid == 0) write_result(prefix, sa, s, med_iqr);
}

// Whole select in ONE workgroup per sensor, for sensors whose slots fit the register file of a
// 1024-thread workgroup (32 keys per thread = 32768 slots: the single-GPU series of the bench).  No global
// histograms, no tickets, no inter-block hand-offs, one launch instead of five:
//   digits 0-1 over the keys in registers (read from HBM once; 32-bit math on the high word);
//   keys matching some rank's 16-bit prefix (a few percent) are compacted into LDS, digit 2 runs on those;
//   keys matching a 24-bit prefix (a handful) are compacted again and every rank is finished by
//   COUNTING: a thread per candidate counts the smaller / equal candidates of its bucket.
// Inputs that defeat the compaction (e.g. a constant sensor: every key matches) fall back to digit
// passes over LDS or registers, still inside this launch.
constexpr int ONE_NT = 1024;
constexpr int ONE_FK = 32;
constexpr int ONE_CAP = 8192;   // 16-bit-prefix survivors kept in LDS (64 KB)
constexpr int ONE_CAP2 = 1024;  // 24-bit-prefix survivors finished by counting

//
// BRACKET PATH (flat rows with >= 4 * BR_S real keys; every test below is uniform over the workgroup and a failed one
// runs the digit passes above unchanged, in the same launch):
//   sample    BR_S hi words at the fixed stride slots / BR_S (slot floor(j * slots / BR_S)), loaded BEFORE the row so
//             that their bitonic sort (in-wave exchanges by lane shuffles, the ten cross-wave stages through LDS) runs
//             while the row's 32 loads per thread are in flight; the filler sorts last, m = real samples.
//   brackets  per rank pair (q25, median, q75) the sample order statistics d positions below the pair's scaled
//             position r * m / total and d above it.  For i.i.d. keys the number X of sample keys <= the rank's key
//             is hypergeometric, no wider than Binomial(m, p): sigma <= sqrt(m) / 2.  A side misses when X deviates by
//             d; with d = 5.24 sigma = BR_C * sqrt(m), BR_C = 2.62, the normal tail is 8e-8 per side and 12 sides
//             (6 ranks x 2) stay below 1e-6 per sensor.  Brackets are hi-word ranges (the enclosing hi-word values),
//             overlapping ones are merged: at most three disjoint intervals, ~17 % of the row each at m = 1024.
//   one pass  over the hi words in registers: per interval the keys strictly below it (register adds, wave
//             reduction, one LDS atomic per wave and counter) and a 512-bin histogram of the keys inside it (bin =
//             (hi - lo) >> shift: monotone in the key) -- the brackets of a 1024-key sample are thousands of keys wide,
//             far too many to finish by counting, so each rank is first located in a bin of ~15 keys.
//   finish    a rank outside [below, below + inside) of its interval -> fallback.  The keys of the ranks' bins
//             (~50-100) are staged as slot numbers, re-read in full (> ONE_CAP2 of them -> fallback) and every rank
//             is finished by the counting finisher: full 64-bit keys, the same bits as the digit passes give.
constexpr int BR_S = ONE_NT;      // sample size: one key per thread
constexpr float BR_C = 2.62f;     // margin in units of sqrt(m) sample positions (see above)
constexpr unsigned int BR_NONE = 0xffffu;   // bin code of a key outside every interval
//
// ONE-SPAN TIER, in front of the three intervals (rows like the bench's: the brackets lie close together): ONE
// histogram of SPAN_BINS bins over the single hi-word span from the q25 bracket's lower edge to the q75 bracket's upper
// edge.  Per key one subtract, one unsigned compare, one shift, one LDS atomic and ONE below-counter instead of three
// interval tests and three counters; the staging pass is three range tests on the hi word instead of a second
// code_of and six compares.  The tiers run in this order in the same launch, every decision uniform: the one-span
// tier is chosen from the sorted sample alone (the rule stands where it is evaluated) and falls through to the
// three-interval tier when the rule rejects it, a rank lies outside the span or more than ONE_CAP2 keys share the
// ranks' bins; the three-interval tier falls back to the digit passes as before.  SelectArgs::bracket: 0 digit passes
// only, 1 the three-interval tier only (GDN_SELECT_SPAN=0), 2 both tiers.
//
// LDS MAP of select_onewg_kernel (static, no larger than before the one-span tier: its words alias `stage`):
//   hist[6][256]   digit passes: a 256-bin histogram per rank | bracket path: three intervals x 512 bins
//   sbuf[2048]     bracket path: the sample, two exchange buffers of its sort; the sorted sample ends in the first
//   stage[8192]    digit passes: full keys of the 16-bit-prefix survivors (written from pass 1 on) | bracket path,
//                  as 32-bit words: [0, SPAN_BINS) the one-span histogram, [SPAN_BELOW] keys below the span,
//                  [SPAN_CODE + q] bin of rank q -- idle there until a fallback, which rewrites it
//   stage2[1024]   full keys of the candidates of the counting finisher (every path)
//   sidx[8192]     slot numbers of staged keys; the bracket path keeps the candidates' bins there after the re-read
constexpr int SPAN_BINS = 2048;
constexpr int SPAN_BELOW = SPAN_BINS;
constexpr int SPAN_CODE = SPAN_BINS + 1;

template <bool FLAT, typename ARGS>
__global__ __launch_bounds__(ONE_NT) void select_onewg_kernel(const KeyLayout kl, const ARGS args,
                                                              double* __restrict__ med_iqr, int* __restrict__ path) {
  __shared__ unsigned int hist[NQ][256];
  __shared__ unsigned int sbuf[2 * BR_S];    // bracket path: the sample (two exchange buffers of the sort)
  __shared__ unsigned int br_below[3], br_code[NQ], br_m;
  __shared__ unsigned long long prefix[NQ];
  __shared__ unsigned long long stage[ONE_CAP];
  __shared__ unsigned long long stage2[ONE_CAP2];
  __shared__ unsigned short sidx[ONE_CAP];   // slot numbers of the 16-bit-prefix survivors
  __shared__ int rem[NQ];
  __shared__ int rep[NQ];
  __shared__ unsigned int n_stage, n_stage2, dref;
  __shared__ unsigned int cnt0[2];
  const int s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const SelectArgs& sa = select_args_for(args, s);
  if constexpr (kPerSensor<ARGS>) {
    if (sa.total < 1) return;                // (uniform) too few real keys: the row stays as it is
  }
  const unsigned int slots = (unsigned int)kl.blocks * (unsigned int)kl.pitch;
#ifdef GDN_SELECT_TIMING
  const long long tick_start = wall_clock64();
#endif
  // Only the HIGH words stay in registers (digits 0-2 and both compactions look at nothing else): 32 VGPRs
  // instead of 64 — with the full keys the kernel spilled 47 VGPRs + 172 SGPRs at its 128-register budget
  // (4 waves per SIMD) and every pass paid scratch traffic.  The few keys that survive the 16-bit compaction
  // are re-read in full (L2-resident: the sensor's row was just streamed).
  constexpr bool flat = FLAT;                              // blocks == 1 (single GPU): the sensor's row is contiguous
  // flat rows go through a buffer descriptor: per-thread offset in ONE register, the slot offset u*8 KB a
  // scalar (64-bit pointers per slot cost 64 VGPRs and spilled); reads past the row return 0
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned long long*>(kl.keys + (size_t)s * kl.pitch), 0, flat ? kl.pitch * 8 : 0, 0x00020000);
  auto key_full = [&](int u) -> unsigned long long {
    if constexpr (flat) {
      typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
      const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, tid * 8, u * (ONE_NT * 8), 0);
      return ((unsigned long long)v.y << 32) | v.x;
    } else {
      const unsigned int i = tid + u * ONE_NT;
      const unsigned int blk = i / (unsigned int)kl.pitch, off = i - blk * (unsigned int)kl.pitch;
      return kl.keys[((size_t)blk * kl.n + s) * kl.pitch + off];
    }
  };
  auto key_slot = [&](unsigned int i) -> unsigned long long {     // slot number -> full key
    if constexpr (flat) {
      return kl.keys[(size_t)s * kl.pitch + i];
    } else {
      const unsigned int blk = i / (unsigned int)kl.pitch, off = i - blk * (unsigned int)kl.pitch;
      return kl.keys[((size_t)blk * kl.n + s) * kl.pitch + off];
    }
  };
  const bool try_bracket = flat && sa.bracket != 0 && sa.total >= 4 * BR_S;    // uniform
  unsigned int smp = 0xffffffffu;
  if constexpr (flat) {
    if (try_bracket) smp = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (((unsigned int)tid * slots) / BR_S) * 8 + 4, 0, 0);
  }
  unsigned int khi[ONE_FK];
#pragma unroll
  for (int u = 0; u < ONE_FK; ++u) {
    unsigned int hi;
    if constexpr (flat) hi = __builtin_amdgcn_raw_buffer_load_b32(rsrc, tid * 8 + 4, u * (ONE_NT * 8), 0);
    else hi = tid + u * ONE_NT < slots ? (unsigned int)(key_full(u) >> 32) : 0u;
    if constexpr (flat) khi[u] = hi;                         // (slots past the row: below, after the sample's sort)
    else khi[u] = tid + u * ONE_NT < slots ? hi : 0xffffffffu;   // filler: never a real key
  }
  // survivors (bit u of keep: my key u) first as SLOT NUMBERS in sidx, to be re-read in full by all threads at once
  // (a load inside the per-slot branch would pay one L2 round trip per survivor, serially); one LDS atomic per
  // WAVE: lanes scan their survivor counts, the last lane reserves the range.  Returns the survivors' number.
  // (Forced inline: with three call sites one instantiation otherwise gets a real call, a stack and scratch.)
  auto stage_slots = [&](unsigned int keep) __attribute__((always_inline)) -> unsigned int {
    const int mine = __popc(keep);
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    unsigned int base = 0u;
    if (lane == 63) base = atomicAdd(&n_stage, (unsigned int)incl);
    base = __shfl(base, 63);
    unsigned int pos = base + (unsigned int)(incl - mine);
    unsigned int t1 = tid;
    asm volatile("" : "+v"(t1));     // keeps the 32 slot numbers from being precomputed outside the pass loop
#pragma unroll
    for (int u = 0; u < ONE_FK; ++u) {
      if ((keep >> u) & 1u) {
        if (pos < (unsigned int)ONE_CAP) sidx[pos] = (unsigned short)(t1 + u * ONE_NT);   // slots <= 32768
        ++pos;
      }
    }
    __syncthreads();
    return n_stage;
  };
  // every rank finished by COUNTING: a thread per candidate counts the smaller / equal candidates of its bucket
  // (bucket_of(j): candidate j's bucket, rank_bucket(q): the bucket that holds rank q at position rem[q])
  auto finish_by_counting = [&](const unsigned long long* cand, unsigned int n, auto bucket_of, auto rank_bucket) {
    if ((unsigned int)tid < n) {
      const unsigned long long k = cand[tid];
      const auto mine = bucket_of((unsigned int)tid);
      bool wanted = false;
#pragma unroll
      for (int q = 0; q < NQ; ++q) wanted |= rank_bucket(q) == mine;
      if (wanted) {
        int less = 0, equal = 0;
        for (unsigned int j = 0; j < n; ++j) {
          const unsigned long long o = cand[j];
          if (bucket_of(j) != mine) continue;
          less += o < k ? 1 : 0;
          equal += o == k ? 1 : 0;
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int want = rem[q];                    // 0-based position inside the bucket
          if (rank_bucket(q) == mine && less <= want && want < less + equal) prefix[q] = k;   // equal keys write the same value
        }
      }
    }
    __syncthreads();
  };
#ifdef GDN_SELECT_TIMING
  long long tick[12], btick[6] = {0, 0, 0, 0, 0, 0};   // sort | span pass, span stage | interval pass, stage | finish
  int nt = 0;
  int br_tier = 2;           // 0: the one-span tier staged the candidates, 1: it ran and fell through, 2: it did not run
  unsigned int br_n = 0u;
#endif
  bool bracketed = false;
  if constexpr (flat) {
    if (try_bracket) {
      unsigned int* hflat = &hist[0][0];     // three intervals x 512 bins
      for (int i = tid; i < 3 * 512; i += ONE_NT) hflat[i] = 0u;
      unsigned int* shist = reinterpret_cast<unsigned int*>(stage);   // the one-span tier's words (see the LDS map)
      shist[tid] = 0u;
      shist[tid + ONE_NT] = 0u;
      if (tid == 0) shist[SPAN_BELOW] = 0u;
      if (tid < NQ) shist[SPAN_CODE + tid] = ~0u;
      if (tid < 3) br_below[tid] = 0u;
      if (tid < NQ) br_code[tid] = ~0u;
      if (tid == 0) {
        br_m = 0u;
        n_stage = 0u;
      }
      // bitonic sort of the sample, one key per thread; buffers alternate, so one barrier per cross-wave stage
      unsigned int v = smp;
      int pp = 0;
#pragma unroll
      for (int k = 2; k <= BR_S; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
          unsigned int o;
          if (j >= 64) {
            sbuf[pp * BR_S + tid] = v;
            __syncthreads();
            o = sbuf[pp * BR_S + (tid ^ j)];
            pp ^= 1;
          } else {
            o = (unsigned int)__shfl_xor((int)v, j);
          }
          const bool take_min = ((tid & j) == 0) == ((tid & k) == 0);
          v = take_min ? min(v, o) : max(v, o);
        }
      }
      static_assert(BR_S == 1024, "the sorted sample ends in the first exchange buffer after ten cross-wave stages");
      sbuf[tid] = v;
      __syncthreads();
      if (v != 0xffffffffu && (tid == BR_S - 1 || sbuf[tid + 1] == 0xffffffffu)) br_m = (unsigned int)(tid + 1);
      __syncthreads();
#ifdef GDN_SELECT_TIMING
      btick[0] = wall_clock64();
#endif
    }
  }
  // the row's hi words are first needed here: the sort above ran while their loads were in flight
  if constexpr (flat) {
#pragma unroll
    for (int u = 0; u < ONE_FK; ++u) khi[u] = tid + u * ONE_NT < slots ? khi[u] : 0xffffffffu;   // filler: never a real key
  }
  if constexpr (flat) {
    if (try_bracket) {
      unsigned int* hflat = &hist[0][0];
      const unsigned int* sorted = sbuf;
      const int m = (int)br_m;                 // real keys in the sample (the filler sorted last)
      if (m >= BR_S / 2) {
        const float fm = (float)m, ft = (float)sa.total;
        const int margin = (int)(BR_C * sqrtf(fm)) + 2;
        unsigned int lo[3], hi[3];             // q25, median, q75: ascending
        const int first[3] = {2, 0, 4};
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          const int li = (int)((float)sa.rank[first[g]] * fm / ft) - margin;
          const int ui = (int)((float)sa.rank[first[g] + 1] * fm / ft) + 1 + margin;
          lo[g] = li < 0 ? 0u : sorted[li];
          hi[g] = ui >= m ? 0x7fffffffu : sorted[ui];
        }
        // merge overlapping brackets into disjoint intervals [L, L + W]; an unused one matches no key (no key has
        // the hi word 0x80000000: keys are non-negative, the filler is all ones)
        unsigned int L0 = lo[0], H0 = hi[0], L1 = 0x80000000u, H1 = 0x80000000u, L2 = 0x80000000u, H2 = 0x80000000u;
        int iv_med, iv_q75;
        if (lo[1] <= H0) { H0 = hi[1]; iv_med = 0; } else { L1 = lo[1]; H1 = hi[1]; iv_med = 1; }
        if (iv_med == 0) {
          if (lo[2] <= H0) { H0 = hi[2]; iv_q75 = 0; } else { L1 = lo[2]; H1 = hi[2]; iv_q75 = 1; }
        } else {
          if (lo[2] <= H1) { H1 = hi[2]; iv_q75 = 1; } else { L2 = lo[2]; H2 = hi[2]; iv_q75 = 2; }
        }
        L0 = __builtin_amdgcn_readfirstlane(L0);
        L1 = __builtin_amdgcn_readfirstlane(L1);
        L2 = __builtin_amdgcn_readfirstlane(L2);
        const unsigned int W0 = __builtin_amdgcn_readfirstlane(H0 - L0), W1 = __builtin_amdgcn_readfirstlane(H1 - L1),
                           W2 = __builtin_amdgcn_readfirstlane(H2 - L2);
        const unsigned int S0 = W0 < 512u ? 0u : 23u - (unsigned int)__clz((int)W0),   // (hi - L) >> S < 512
                           S1 = W1 < 512u ? 0u : 23u - (unsigned int)__clz((int)W1),
                           S2 = W2 < 512u ? 0u : 23u - (unsigned int)__clz((int)W2);
        // interval * 512 + bin of a hi word, BR_NONE outside every interval (the filler and unused intervals included)
        auto code_of = [&](unsigned int h) __attribute__((always_inline)) -> unsigned int {
          const unsigned int d0 = h - L0, d1 = h - L1, d2 = h - L2;
          unsigned int c = BR_NONE;
          if (d2 <= W2) c = 1024u + (d2 >> S2);
          if (d1 <= W1) c = 512u + (d1 >> S1);
          if (d0 <= W0) c = d0 >> S0;
          return c;
        };
        // ONE-SPAN TIER.  One monotone histogram of SPAN_BINS bins over [LS, LS + WS]: from the lower edge of the q25
        // bracket to the upper edge of the q75 bracket.  Chosen from the sorted sample alone: the span's bins must be
        // at most 4 x as wide as the bins of the finest interval (SS <= min S + 2) -- a bin of the three-interval
        // tier holds ~15 keys, so six span bins stay far below ONE_CAP2 where the key density between the brackets
        // is like that inside them; rows whose brackets lie far apart (a level shift, two clusters) fail the rule
        // and do not pay the pass.  A span of one hi word (WS == 0) cannot separate anything.
        const int n_iv = iv_q75 + 1;                                     // intervals in use
        unsigned int Smin = S0;
        if (n_iv > 1) Smin = min(Smin, S1);
        if (n_iv > 2) Smin = min(Smin, S2);
        const unsigned int LS = L0;
        const unsigned int WS = __builtin_amdgcn_readfirstlane(hi[2] - lo[0]);
        const unsigned int SS = WS < (unsigned int)SPAN_BINS ? 0u : 21u - (unsigned int)__clz((int)WS);   // WS >> SS < 2048
        const bool use_span = sa.bracket >= 2 && WS != 0u && SS <= Smin + 2u;   // uniform
        unsigned int code[NQ];                 // the ranks' bins (of whichever tier staged the candidates)
        unsigned int n_cand = 0u;
        bool have = false, by_span = false;    // candidates staged in sidx, at most ONE_CAP2 of them
        if (use_span) {
          unsigned int* shist = reinterpret_cast<unsigned int*>(stage);
          unsigned int below = 0u;
          unsigned int ssv = SS, one = 1u;     // in vector registers: as scalars they are re-read from a spill lane per key
          asm volatile("" : "+v"(ssv), "+v"(one));
#pragma unroll
          for (int u = 0; u < ONE_FK; ++u) {
            const unsigned int h = khi[u];     // the filler: h - LS >= 0x80000000 > WS
            const unsigned int d = h - LS;
            below += h < LS ? 1u : 0u;
            if (d <= WS) atomicAdd(&shist[d >> ssv], one);
          }
#pragma unroll
          for (int d = 32; d >= 1; d >>= 1) below += __shfl_xor(below, d);
          if (lane == 0) atomicAdd(&shist[SPAN_BELOW], below);
          __syncthreads();
#ifdef GDN_SELECT_TIMING
          btick[1] = wall_clock64();
#endif
          if (wv < NQ) locate_bin2048(shist, sa.rank[wv] - (int)shist[SPAN_BELOW], lane, &shist[SPAN_CODE + wv], &rem[wv]);
          __syncthreads();
          bool inside = true;
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            code[q] = __builtin_amdgcn_readfirstlane(shist[SPAN_CODE + q]);
            inside = inside && code[q] != ~0u; // nothing written: the rank is outside the span
          }
          if (inside) {
            // the six ranks are three adjacent pairs and the bins between a pair's two bins are empty: one range
            // test per pair, on the hi word itself (bins c_lo..c_hi are the hi words LS + (c_lo << SS) ..
            // LS + min(((c_hi + 1) << SS) - 1, WS): no key past the span, none was counted)
            unsigned int r_lo[3], r_w[3];
            const int first[3] = {2, 0, 4};
#pragma unroll
            for (int g = 0; g < 3; ++g) {
              const unsigned int d_lo = code[first[g]] << SS, d_hi = min(((code[first[g] + 1] + 1u) << SS) - 1u, WS);
              r_lo[g] = LS + d_lo;
              r_w[g] = d_hi - d_lo;
            }
            unsigned int keep = 0u;
#pragma unroll
            for (int u = 0; u < ONE_FK; ++u) {
              const unsigned int h = khi[u];
              const bool any = (h - r_lo[0] <= r_w[0]) | (h - r_lo[1] <= r_w[1]) | (h - r_lo[2] <= r_w[2]);
              keep |= any ? (1u << u) : 0u;
            }
            asm volatile("" : "+v"(keep));     // ONE register of bits: 32 compare masks kept as scalar pairs spill
            n_cand = stage_slots(keep);
            have = by_span = n_cand <= (unsigned int)ONE_CAP2;
            if (!have) {                       // (uniform) every thread has read n_stage: start the next tier at 0
              __syncthreads();
              if (tid == 0) n_stage = 0u;
            }
          }
#ifdef GDN_SELECT_TIMING
          btick[2] = wall_clock64();
          br_tier = have ? 0 : 1;
#endif
        }
        if (!have) {
          // THREE-INTERVAL TIER
          unsigned int b01 = 0u, b2 = 0u;      // keys below interval 0 | below interval 1 << 16, below interval 2
#pragma unroll
          for (int u = 0; u < ONE_FK; ++u) {
            const unsigned int h = khi[u];     // the filler (all ones) is below nothing and inside nothing
            b01 += (h < L0 ? 1u : 0u) + (h < L1 ? 0x10000u : 0u);
            b2 += h < L2 ? 1u : 0u;
            const unsigned int c = code_of(h);
            if (c != BR_NONE) atomicAdd(&hflat[c], 1u);
          }
#pragma unroll
          for (int d = 32; d >= 1; d >>= 1) {  // <= 2048 per wave and counter: the packed halves do not carry
            b01 += __shfl_xor(b01, d);
            b2 += __shfl_xor(b2, d);
          }
          if (lane == 0) {
            atomicAdd(&br_below[0], b01 & 0xffffu);
            atomicAdd(&br_below[1], b01 >> 16);
            atomicAdd(&br_below[2], b2);
          }
          __syncthreads();
#ifdef GDN_SELECT_TIMING
          btick[3] = wall_clock64();
#endif
          if (wv < NQ) {                       // wave q: rank q's bin inside its interval
            const int iv = wv < 2 ? iv_med : (wv < 4 ? 0 : iv_q75);
            locate_bin512(hflat + 512 * iv, sa.rank[wv] - (int)br_below[iv], 512u * (unsigned int)iv, lane,
                          &br_code[wv], &rem[wv]);
          }
          __syncthreads();
          bool inside = true;
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            code[q] = __builtin_amdgcn_readfirstlane(br_code[q]);
            inside = inside && code[q] != ~0u; // nothing written: the rank is outside its bracket
          }
          if (inside) {
            unsigned int keep = 0u;
#pragma unroll
            for (int u = 0; u < ONE_FK; ++u) {
              const unsigned int c = code_of(khi[u]);
              bool any = false;
#pragma unroll
              for (int q = 0; q < NQ; ++q) any |= c == code[q];
              keep |= any ? (1u << u) : 0u;
            }
            n_cand = stage_slots(keep);
            have = n_cand <= (unsigned int)ONE_CAP2;
          }
#ifdef GDN_SELECT_TIMING
          btick[4] = wall_clock64();
#endif
        }
#ifdef GDN_SELECT_TIMING
        br_n = n_cand;
#endif
        if (have) {
          // both tiers: the candidates re-read in full, their bin kept beside them, every rank finished by counting
          if ((unsigned int)tid < n_cand) {
            const unsigned long long k = key_slot(sidx[tid]);
            const unsigned int hk = (unsigned int)(k >> 32);
            stage2[tid] = k;
            sidx[tid] = (unsigned short)(by_span ? (hk - LS) >> SS : code_of(hk));   // the slot number is consumed
          }
          __syncthreads();
          finish_by_counting(stage2, n_cand, [&](unsigned int j) { return (unsigned int)sidx[j]; },
                             [&](int q) { return code[q]; });
          bracketed = true;
        }
      }
      if (!bracketed) __syncthreads();         // the counters read above are reset below
#ifdef GDN_SELECT_TIMING
      btick[5] = wall_clock64();
#endif
    }
  }
  if (!bracketed) {
    if (tid < NQ) {
      prefix[tid] = 0ull;
      rem[tid] = sa.rank[tid];
    }
    if (tid == 0) {
      n_stage = 0u;
      n_stage2 = 0u;
    }
    __syncthreads();
  }
#ifdef GDN_SELECT_TIMING
  tick[nt++] = wall_clock64();
#endif
  bool in_lds = false;       // digits >= 2 read the compacted survivors
  bool done = bracketed;     // the digit passes run only when the brackets did not settle the ranks
  unsigned int n_keep = 0u;
  for (int pass = 0; pass < 8 && !done; ++pass) {
    const int shift = 56 - 8 * pass;
    if (tid < NQ) {
      int r = tid;
      for (int q = tid - 1; q >= 0; --q)
        if (prefix[q] == prefix[tid]) r = q;
      rep[tid] = r;
    }
    for (int i = tid; i < NQ * 256; i += ONE_NT) (&hist[0][0])[i] = 0u;
    if (pass == 0 && tid == 0) {
      cnt0[0] = cnt0[1] = 0u;
      dref = khi[0] >> 24;                 // top byte of tick 0's key: the bin of (nearly) every key
    }
    __syncthreads();
    if (pass == 0) {
      // Digit 0 without a histogram: errors of one sensor almost always share the top byte (sign + 7
      // exponent bits), so COUNT the keys below / inside the reference bin (compares and adds in registers,
      // one LDS atomic pair per wave); if every rank falls inside it the digit is known.  Otherwise (ranks in
      // several bins) the generic histogram below runs.
      const unsigned int dr = dref;
      unsigned int less = 0u, same = 0u;
#pragma unroll
      for (int u = 0; u < ONE_FK; ++u) {
        const unsigned int hi = khi[u];
        const unsigned int digit = hi >> 24;             // the filler's digit is 255: never less, never same
        less += digit < dr ? 1u : 0u;
        same += digit == dr ? 1u : 0u;
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        less += __shfl_xor(less, d);
        same += __shfl_xor(same, d);
      }
      if (lane == 0) {
        atomicAdd(&cnt0[0], less);
        atomicAdd(&cnt0[1], same);
      }
      __syncthreads();
      const unsigned int tl = cnt0[0], ts = cnt0[1];
      bool inside = dr != 255u;
#pragma unroll
      for (int q = 0; q < NQ; ++q) inside = inside && (unsigned int)sa.rank[q] >= tl && (unsigned int)sa.rank[q] < tl + ts;
      if (inside) {                                        // uniform
        if (tid < NQ) {
          prefix[tid] = (unsigned long long)dr << 56;
          rem[tid] = sa.rank[tid] - (int)tl;
        }
        __syncthreads();
#ifdef GDN_SELECT_TIMING
        tick[nt++] = wall_clock64();
#endif
        continue;
      }
    }
    // One REAL loop over the ranks (not unrolled: with the 32 key slots unrolled inside six copies of every
    // branch the kernel was 34 k instructions and spilled ~110 SGPRs); ranks that share their prefix with an
    // earlier one are skipped (uniform).
    if (!in_lds && pass < 3) {
      // digits 0-2 live in the HIGH word of the key: 32-bit shifts and compares
      const unsigned int sh = 24u - 8u * (unsigned int)pass;
#pragma nounroll
      for (int q = 0; q < NQ; ++q) {
        if (rep[q] != q) continue;
        const unsigned int pfh = (unsigned int)(prefix[q] >> 32);
        unsigned int* hq = hist[q];
#pragma unroll
        for (int u = 0; u < ONE_FK; ++u) {
          const unsigned int hi = khi[u];
          const bool real = (int)hi >= 0;               // keys are non-negative doubles; the filler is all ones
          const unsigned int digit = (hi >> sh) & 255u;
          if (pass == 0) {                              // (only when the counting path above gave up)
            const unsigned int d0 = __builtin_amdgcn_readfirstlane(digit);
            if (__all(real && digit == d0)) {           // a whole wave in one bin: one add
              if (lane == 0) atomicAdd(&hq[d0], 64u);
            } else if (real) {
              atomicAdd(&hq[digit], 1u);
            }
          } else if (real && ((hi ^ pfh) >> (sh + 8u)) == 0u) {
            atomicAdd(&hq[digit], 1u);
          }
        }
      }
    } else if (!in_lds) {
#pragma nounroll
      for (int q = 0; q < NQ; ++q) {
        if (rep[q] != q) continue;
        const unsigned long long pfq = prefix[q];
        unsigned int* hq = hist[q];
#pragma unroll 4
        for (int u = 0; u < ONE_FK; ++u) {      // compaction defeated (rare): full keys re-read per digit
          const bool real = (int)khi[u] >= 0;
          const unsigned long long k = real ? key_full(u) : FILLER;
          const unsigned int digit = (unsigned int)(k >> shift) & 255u;
          if (real && ((k ^ pfq) >> (shift + 8)) == 0ull) atomicAdd(&hq[digit], 1u);
        }
      }
    } else {
#pragma nounroll
      for (int q = 0; q < NQ; ++q) {
        if (rep[q] != q) continue;
        const unsigned long long pfq = prefix[q];
        unsigned int* hq = hist[q];
        for (unsigned int i = tid; i < n_keep; i += ONE_NT) {
          const unsigned long long k = stage[i];
          const unsigned int digit = (unsigned int)(k >> shift) & 255u;
          if (((k ^ pfq) >> (shift + 8)) == 0ull) atomicAdd(&hq[digit], 1u);
        }
      }
    }
    __syncthreads();
    for (int q = wv; q < NQ; q += ONE_NT / 64)
      locate_bin(hist[rep[q]], rem[q], prefix[q], shift, lane, &prefix[q], &rem[q]);
    __syncthreads();
    if (pass == 1) {
      // compact the keys that still match some rank's 16-bit prefix; stay in registers if they do not fit
      unsigned int p16[NQ];                            // distinct 16-bit prefixes as scalars; 0x10000 = unused
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        p16[q] = __builtin_amdgcn_readfirstlane((unsigned int)(prefix[q] >> 48));
#pragma unroll
        for (int r = 0; r < q; ++r)
          if (p16[r] == p16[q]) p16[q] = 0x10000u;
      }
      unsigned int keep = 0u;                          // bit u: my key u survives
#pragma unroll
      for (int u = 0; u < ONE_FK; ++u) {
        const unsigned int h16 = khi[u] >> 16;   // the filler (0xffff) never equals a prefix
        bool any = false;
#pragma unroll
        for (int q = 0; q < NQ; ++q) any |= h16 == p16[q];
        keep |= any ? (1u << u) : 0u;
      }
      n_keep = stage_slots(keep);
      in_lds = n_keep <= (unsigned int)ONE_CAP;
      if (in_lds) {
        for (unsigned int i = tid; i < n_keep; i += ONE_NT) stage[i] = key_slot(sidx[i]);
        __syncthreads();
      }
    }
    if (pass == 2 && in_lds) {
      // second compaction (24-bit prefixes), then finish every rank by counting inside its bucket
      for (unsigned int i = tid; i < n_keep; i += ONE_NT) {
        const unsigned long long k = stage[i];
        bool any = false;
#pragma unroll
        for (int q = 0; q < NQ; ++q) any |= ((k ^ prefix[q]) >> 40) == 0ull;
        if (any) {
          const unsigned int at = atomicAdd(&n_stage2, 1u);
          if (at < (unsigned int)ONE_CAP2) stage2[at] = k;
        }
      }
      __syncthreads();
      const unsigned int n2 = n_stage2;
      if (n2 <= (unsigned int)ONE_CAP2) {
        // (a finished rank's prefix becomes a key of its own bucket: the 24-bit bucket it names does not change)
        finish_by_counting(stage2, n2, [&](unsigned int j) { return stage2[j] >> 40; },
                           [&](int q) { return prefix[q] >> 40; });
        done = true;
      }
    }
#ifdef GDN_SELECT_TIMING
    tick[nt++] = wall_clock64();
#endif
  }
#ifdef GDN_SELECT_TIMING
  if (tid == 0 && s == 1 && bracketed && br_tier == 0)
    printf("onewg bracket ticks(10ns): sample sort (under the row load) %lld count+histogram %lld locate+stage %lld "
           "re-read+finish %lld candidates %u tier one-span\n",
           btick[0] - tick_start, btick[1] - btick[0], btick[2] - btick[1], btick[5] - btick[2], br_n);
  else if (tid == 0 && s == 1 && bracketed)
    printf("onewg bracket ticks(10ns): sample sort (under the row load) %lld count+histogram %lld locate+stage %lld "
           "re-read+finish %lld candidates %u tier three-interval (one-span before it: %lld)\n",
           btick[0] - tick_start, btick[3] - (br_tier == 1 ? btick[2] : btick[0]), btick[4] - btick[3],
           btick[5] - btick[4], br_n, br_tier == 1 ? btick[2] - btick[0] : 0ll);
  else if (tid == 0 && s == 1)
    printf("onewg ticks(10ns): load %lld p0 %lld p1+compact %lld p2+finish %lld (passes run %d) survivors %u / %u\n",
           tick[0] - tick_start, tick[1] - tick[0], tick[2] - tick[1], tick[3] - tick[2], nt - 1, n_keep, n_stage2);
#endif
  if (tid == 0) {
    write_result(prefix, sa, s, med_iqr);
    if (path) path[s] = bracketed ? 0 : 1;
  }
}

// Normalise, smooth, reduce over sensors: the sweep of gdn_score_sweep.hpp (the one full description).  Here: the two
// reductions over a resident shard (its rows come from gdn_sweep::SeriesSource).

// anomaly = max over sensors (the transposing butterfly); `scores` (optional) gets the [n, t] table.
template <bool GAPS>
__global__ __launch_bounds__(256) void score_smooth_max_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt, const double* __restrict__ med_iqr,
    int t, int n, int first_tick, const float* __restrict__ halo_pred, const float* __restrict__ halo_gt,
    double* __restrict__ scores, double* __restrict__ anomaly, const unsigned char* __restrict__ valid,
    const unsigned char* __restrict__ halo_valid) {
  __shared__ double best[4][RUN];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int nruns = (t + RUN - 1) / RUN;
  const SeriesSource src{pred, gt, halo_pred, halo_gt, valid, halo_valid, t, n, first_tick};
  for (int run = blockIdx.x * wpb + wv; run < nruns; run += gridDim.x * wpb) {
    const int t0 = run * RUN, t1 = min(t, t0 + RUN);
    for (int s0 = 0; s0 < n; s0 += 128) {          // two sensors per lane per sweep
      const Lanes l(s0, lane, n);
      double mt[RUN];                             // this lane's max over its sensors, per tick of the run
#pragma unroll
      for (int u = 0; u < RUN; ++u) mt[u] = -INFINITY;
      score_sweep<GAPS>(src, med_iqr, l, t0, t1, first_tick, [&](int u, int tick, double sma, double smb) {
        if (scores) {
          if (l.la) scores[(size_t)l.sa * t + tick] = sma;
          if (l.lb) scores[(size_t)l.sb * t + tick] = smb;
        }
        mt[u] = fmax(l.la ? sma : -INFINITY, l.lb ? smb : -INFINITY);
      });
      const double k1 = butterfly_max(mt, lane);
      if ((lane & 7) == 0) {
        const int u = butterfly_tick(lane);
        best[wv][u] = s0 == 0 ? k1 : fmax(best[wv][u], k1);
      }
    }
    // (LDS writes above and reads below are by the same wave, in program order)
    if (lane < t1 - t0) anomaly[t0 + lane] = best[wv][lane];
  }
}

// The m largest scores of every tick with their sensors (topm_merge).  The [n, t] table is never written.
template <bool GAPS>
__global__ __launch_bounds__(256) void score_smooth_topm_kernel(
    const float* __restrict__ pred, const float* __restrict__ gt, const double* __restrict__ med_iqr,
    int t, int n, int first_tick, const float* __restrict__ halo_pred, const float* __restrict__ halo_gt,
    int m, double* __restrict__ top_scores, int* __restrict__ top_sensors, const unsigned char* __restrict__ valid,
    const unsigned char* __restrict__ halo_valid) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int nruns = (t + RUN - 1) / RUN;
  const SeriesSource src{pred, gt, halo_pred, halo_gt, valid, halo_valid, t, n, first_tick};
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
  }
}

}  // namespace

namespace {

// diagnostic knobs: GDN_SELECT_BRACKET=0 keeps the one-workgroup select on its digit passes, GDN_SELECT_SPAN=0 keeps
// its bracket path on the three-interval tier (comparisons).  The value of SelectArgs::bracket / CountArgs::bracket.
int bracket_mode() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("GDN_SELECT_BRACKET");
    const char* sp = getenv("GDN_SELECT_SPAN");
    v = (e && e[0] == '0') ? 0 : ((sp && sp[0] == '0') ? 1 : 2);
  }
  return v;
}

SelectArgs make_select_args(long long t) {
  SelectArgs sa;
  fill_select_args(sa, t);
  sa.bracket = bracket_mode();
  return sa;
}

// diagnostic knob: GDN_SELECT_MULTI=1 forces the multi-launch path at every size (tests, comparisons)
bool force_multi_block() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("GDN_SELECT_MULTI");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}

__global__ void select_path_fill_kernel(int* __restrict__ path, int n, int value) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) path[i] = value;
}

// path (optional, [n] int32 on the device): 0 where a sensor's ranks were settled by the sample brackets of
// select_onewg_kernel, 1 where the digit passes ran (every sensor on the other routes)
template <typename ARGS>
int run_select(const double* keys, int blocks, int n, int pitch, const ARGS sa, double* workspace,
               double* med_iqr, int* path, hipStream_t st) {
  const long long slots = (long long)blocks * pitch;
  KeyLayout kl;
  kl.keys = reinterpret_cast<const unsigned long long*>(keys);
  kl.bufb = reinterpret_cast<unsigned long long*>(workspace);
  kl.blocks = blocks; kl.n = n; kl.pitch = pitch;
  SelState* state = reinterpret_cast<SelState*>(kl.bufb + (size_t)slots * n);
  const int slices = (int)((slots + SLICE - 1) / SLICE);
  if (slices > 1 && slots <= (long long)ONE_NT * ONE_FK && !force_multi_block()) {
    // the whole sensor fits one workgroup's registers: one launch, no global state
    if (kl.blocks == 1) hipLaunchKernelGGL((select_onewg_kernel<true, ARGS>), dim3(n), dim3(ONE_NT), 0, st, kl, sa, med_iqr, path);
    else hipLaunchKernelGGL((select_onewg_kernel<false, ARGS>), dim3(n), dim3(ONE_NT), 0, st, kl, sa, med_iqr, path);
    return gdn_launch_status();
  }
  if (path) hipLaunchKernelGGL(select_path_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, path, n, 1);
  hipLaunchKernelGGL(select_init_kernel<ARGS>, dim3(n), dim3(256), 0, st, state, sa);
  if (slices == 1) {   // tiny input: everything in the finisher, straight from the input
    hipLaunchKernelGGL((select_finish_kernel<false, ARGS>), dim3(n), dim3(FIN_NT), 0, st, kl, state, 0, sa, med_iqr);
    return gdn_launch_status();
  }
  hipLaunchKernelGGL((select_pass_kernel<false, false>), dim3(slices, n), dim3(256), 0, st, kl, state, 0);
  hipLaunchKernelGGL((select_pass_kernel<false, false>), dim3(slices, n), dim3(256), 0, st, kl, state, 1);
  hipLaunchKernelGGL((select_pass_kernel<false, true>), dim3(slices, n), dim3(256), 0, st, kl, state, 2);
  // digits 3-7 on the survivors (normally a few percent of the keys) in one launch per sensor
  hipLaunchKernelGGL((select_finish_kernel<true, ARGS>), dim3(n), dim3(FIN_NT), 0, st, kl, state, 3, sa, med_iqr);
  return gdn_launch_status();
}

}  // namespace

// select workspace: compacted-key buffer [n][blocks*pitch] + one SelState per sensor
extern "C" long long gdn_score_select_workspace_bytes(int blocks, int n, int pitch) {
  if (blocks <= 0 || n <= 0 || pitch <= 0) return 0;
  return (long long)blocks * pitch * n * 8 + (long long)n * (long long)sizeof(SelState) + 256;
}

// quantiles workspace: the key buffer [n][t] + the select workspace
extern "C" long long gdn_score_workspace_bytes(int t, int n) {
  if (t <= 0 || n <= 0) return 0;
  return (long long)t * n * 8 + gdn_score_select_workspace_bytes(1, n, t);
}

extern "C" int gdn_score_keys(const float* pred, const float* gt, int t, int n, int pitch, double* keys,
                              void* stream) {
  if (!pred || !gt || !keys || t <= 0 || n <= 0 || pitch < t) return GDN_ERR_ARG;
  hipLaunchKernelGGL(score_keys_kernel, dim3((pitch + 63) / 64, (n + 63) / 64), dim3(256), 0,
                     (hipStream_t)stream, pred, gt, t, n, pitch, keys);
  return gdn_launch_status();
}

extern "C" int gdn_score_select(const double* keys, int blocks, int n, int pitch, long long total,
                                double* workspace, double* med_iqr, void* stream) {
  if (!keys || !workspace || !med_iqr || blocks <= 0 || n <= 0 || pitch <= 0 || total <= 0) return GDN_ERR_ARG;
  if (total > (long long)blocks * pitch || (long long)blocks * pitch > 0x7fffffffll) return GDN_ERR_ARG;
  if (blocks > 1 && pitch % SLICE != 0) return GDN_ERR_UNSUPPORTED;   // slices must not straddle blocks
  return run_select(keys, blocks, n, pitch, make_select_args(total), workspace, med_iqr, nullptr, (hipStream_t)stream);
}

// gdn_score_select that also records, per sensor, which path settled its ranks (see run_select)
extern "C" int gdn_score_select_paths(const double* keys, int blocks, int n, int pitch, long long total,
                                      double* workspace, double* med_iqr, int* path, void* stream) {
  if (!keys || !workspace || !med_iqr || !path || blocks <= 0 || n <= 0 || pitch <= 0 || total <= 0) return GDN_ERR_ARG;
  if (total > (long long)blocks * pitch || (long long)blocks * pitch > 0x7fffffffll) return GDN_ERR_ARG;
  if (blocks > 1 && pitch % SLICE != 0) return GDN_ERR_UNSUPPORTED;
  return run_select(keys, blocks, n, pitch, make_select_args(total), workspace, med_iqr, path, (hipStream_t)stream);
}

// Calibration on each sensor's own readings (include/gdn_hip.h): keys with a validity plane, the per-sensor count of
// real keys, and the select with per-sensor counts.
extern "C" int gdn_score_keys_valid(const float* pred, const float* gt, const uint8_t* valid, int t, int n, int pitch,
                                    double* keys, void* stream) {
  if (!pred || !gt || !valid || !keys || t <= 0 || n <= 0 || pitch < t) return GDN_ERR_ARG;
  hipLaunchKernelGGL(score_keys_valid_kernel, dim3((pitch + 63) / 64, (n + 63) / 64), dim3(256), 0,
                     (hipStream_t)stream, pred, gt, valid, t, n, pitch, keys);
  return gdn_launch_status();
}

extern "C" int gdn_score_key_counts(const double* keys, int blocks, int n, int pitch, int32_t* counts, void* stream) {
  if (!keys || !counts || blocks <= 0 || n <= 0 || pitch <= 0) return GDN_ERR_ARG;
  if ((long long)blocks * pitch > 0x7fffffffll) return GDN_ERR_ARG;
  hipLaunchKernelGGL(score_key_counts_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(keys), blocks, n, pitch, counts);
  return gdn_launch_status();
}

// gdn_score_select where sensor s has counts[s] real keys (device data: no host read); a sensor with fewer than
// max(min_count, 1) keeps its med_iqr row (and its path entry on the one-workgroup route).  counts[s] must be the
// number of non-filler slots of sensor s (gdn_score_key_counts computes it).
extern "C" int gdn_score_select_counts(const double* keys, int blocks, int n, int pitch, const int32_t* counts,
                                       int min_count, double* workspace, double* med_iqr, int* path, void* stream) {
  if (!keys || !counts || !workspace || !med_iqr || blocks <= 0 || n <= 0 || pitch <= 0) return GDN_ERR_ARG;
  if ((long long)blocks * pitch > 0x7fffffffll) return GDN_ERR_ARG;
  if (blocks > 1 && pitch % SLICE != 0) return GDN_ERR_UNSUPPORTED;
  CountArgs ca;
  ca.counts = counts;
  ca.min_count = min_count;
  ca.bracket = bracket_mode();
  return run_select(keys, blocks, n, pitch, ca, workspace, med_iqr, path, (hipStream_t)stream);
}

extern "C" int gdn_score_quantiles(const float* pred, const float* gt, int t, int n, double* workspace,
                                   double* med_iqr, void* stream) {
  if (!pred || !gt || !workspace || !med_iqr || t <= 0 || n <= 0) return GDN_ERR_ARG;
  double* keys = workspace;
  const int rc = gdn_score_keys(pred, gt, t, n, t, keys, stream);
  if (rc != GDN_OK) return rc;
  return run_select(keys, 1, n, t, make_select_args(t), workspace + (size_t)t * n, med_iqr, nullptr, (hipStream_t)stream);
}

namespace {

template <bool GAPS>
int smooth_max(const float* pred, const float* gt, const double* med_iqr, int t, int n, int first_tick,
               const float* halo_pred, const float* halo_gt, double* scores, double* anomaly, const uint8_t* valid,
               const uint8_t* halo_valid, void* stream) {
  if (!pred || !gt || !med_iqr || !anomaly || t <= 0 || n <= 0 || first_tick < 0) return GDN_ERR_ARG;
  if (first_tick > 0 && (!halo_pred || !halo_gt)) return GDN_ERR_ARG;
  if (GAPS && (!valid || (first_tick > 0 && !halo_valid))) return GDN_ERR_ARG;
  hipLaunchKernelGGL(score_smooth_max_kernel<GAPS>, dim3(sweep_grid(t)), dim3(256), 0, (hipStream_t)stream, pred, gt,
                     med_iqr, t, n, first_tick, halo_pred, halo_gt, scores, anomaly, valid, halo_valid);
  return gdn_launch_status();
}

template <bool GAPS>
int smooth_topm(const float* pred, const float* gt, const double* med_iqr, int t, int n, int first_tick,
                const float* halo_pred, const float* halo_gt, int m, double* top_scores, int32_t* top_sensors,
                const uint8_t* valid, const uint8_t* halo_valid, void* stream) {
  if (!pred || !gt || !med_iqr || !top_scores || !top_sensors || t <= 0 || n <= 0 || first_tick < 0)
    return GDN_ERR_ARG;
  if (first_tick > 0 && (!halo_pred || !halo_gt)) return GDN_ERR_ARG;
  if (GAPS && (!valid || (first_tick > 0 && !halo_valid))) return GDN_ERR_ARG;
  if (m < 1 || m > TOPM_MAX || m > n) return GDN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(score_smooth_topm_kernel<GAPS>, dim3(sweep_grid(t)), dim3(256), 0, (hipStream_t)stream, pred, gt, med_iqr,
                     t, n, first_tick, halo_pred, halo_gt, m, top_scores, top_sensors, valid, halo_valid);
  return gdn_launch_status();
}

}  // namespace

extern "C" int gdn_score_smooth_max(const float* pred, const float* gt, const double* med_iqr, int t, int n,
                                    int first_tick, const float* halo_pred, const float* halo_gt,
                                    double* scores, double* anomaly, void* stream) {
  return smooth_max<false>(pred, gt, med_iqr, t, n, first_tick, halo_pred, halo_gt, scores, anomaly, nullptr, nullptr,
                           stream);
}

// gdn_score_smooth_max with the m largest scores of every tick and their sensors instead of the maximum alone
// (1 <= m <= 8, m <= n): top_scores[t, m] descending, top_sensors[t, m]; equal scores by the lower sensor.  Same
// arithmetic, first_tick and halo as gdn_score_smooth_max: with m = 1, top_scores[:, 0] is its anomaly bit for bit.
extern "C" int gdn_score_smooth_topm(const float* pred, const float* gt, const double* med_iqr, int t, int n,
                                     int first_tick, const float* halo_pred, const float* halo_gt, int m,
                                     double* top_scores, int32_t* top_sensors, void* stream) {
  return smooth_topm<false>(pred, gt, med_iqr, t, n, first_tick, halo_pred, halo_gt, m, top_scores, top_sensors,
                            nullptr, nullptr, stream);
}

// The two sweeps with a validity plane (include/gdn_hip.h "Resident series with missing readings"): the normalised
// error of a missing (tick, sensor) is exactly 0.0 wherever it is used; with every reading valid they write the bits
// of the plain entry points.
extern "C" int gdn_score_smooth_max_gaps(const float* pred, const float* gt, const double* med_iqr, int t, int n,
                                         int first_tick, const float* halo_pred, const float* halo_gt,
                                         double* scores, double* anomaly, const uint8_t* valid,
                                         const uint8_t* halo_valid, void* stream) {
  return smooth_max<true>(pred, gt, med_iqr, t, n, first_tick, halo_pred, halo_gt, scores, anomaly, valid, halo_valid,
                          stream);
}

extern "C" int gdn_score_smooth_topm_gaps(const float* pred, const float* gt, const double* med_iqr, int t, int n,
                                          int first_tick, const float* halo_pred, const float* halo_gt, int m,
                                          double* top_scores, int32_t* top_sensors, const uint8_t* valid,
                                          const uint8_t* halo_valid, void* stream) {
  return smooth_topm<true>(pred, gt, med_iqr, t, n, first_tick, halo_pred, halo_gt, m, top_scores, top_sensors, valid,
                           halo_valid, stream);
}
