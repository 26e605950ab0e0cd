// Missing readings in a resident series (include/gdn_hip.h "Resident series with missing readings"): the offline
// counterpart of gdn_stream_fill.  gdn_series_fill holds every non-finite reading of raw [n, t_raw] at its sensor's
// latest earlier real one, ONCE, before any step: two launches, no workgroup waits on another, integer bookkeeping
// only.  gdn_score_keys_keep is gdn_score_keys with the filler in every key of a tick that is not complete, so that
// gdn_score_select (total = the kept ticks) calibrates on complete ticks only.  Plain C++: no inline assembly, no
// atomics.  (The scoring launches of a step are the GAPS instantiations of the two sweeps in gdn_score.hip.)
#pragma clang fp contract(off)
#include "gdn_score_sweep.hpp"

namespace {

using gdn_sweep::filler_key;
using gdn_sweep::score_key;

#define GDN_SERIES_BLOCK 64          // ticks per block = lanes of a wave: raw column c sits in block c / 64, lane c % 64
#define GDN_SERIES_WAVES 4

// "Missing" is decided on the bit pattern (exponent field all ones: NaN, +inf, -inf), as gdn_stream_fill decides it.
__device__ inline bool series_missing(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// The carry table, one entry per (sensor, block), three planes of n * blocks words in the workspace:
//   col  int32   raw column of the block's last real reading, -1 when it has none
//   val  fp32    that reading
//   miss int32   missing readings of the block among the scored columns (c >= w)
struct CarryTable {
  int* col;
  float* val;
  int* miss;
};

__host__ __device__ inline CarryTable carry_table(void* workspace, int n, int blocks) {
  const size_t plane = (size_t)n * blocks;
  CarryTable tb;
  tb.col = reinterpret_cast<int*>(workspace);
  tb.val = reinterpret_cast<float*>(workspace) + plane;
  tb.miss = reinterpret_cast<int*>(workspace) + 2 * plane;
  return tb;
}

// Launch 1.  Workgroup b: block b of every sensor, one wave per sensor row (lanes along time: coalesced), one ballot
// of "real" per row.  Writes the carry table only.
__global__ __launch_bounds__(GDN_SERIES_WAVES * 64) void series_carry_kernel(
    const float* __restrict__ raw, int n, int t_raw, int w, int blocks, CarryTable tb) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.x, c = b * GDN_SERIES_BLOCK + lane;
  const bool inside = c < t_raw;
  for (int i = wv; i < n; i += GDN_SERIES_WAVES) {                   // (wave uniform)
    const float v = inside ? raw[(size_t)i * t_raw + c] : 0.f;
    const bool real = inside && !series_missing(v);
    const unsigned long long mask = __ballot(real);
    const unsigned long long gone = __ballot(inside && !real && c >= w);
    const int top = mask ? 63 - __clzll((long long)mask) : 0;
    const float last = __shfl(v, top);
    if (lane == 0) {
      const size_t at = (size_t)i * blocks + b;
      tb.col[at] = mask ? b * GDN_SERIES_BLOCK + top : -1;
      tb.val[at] = last;
      tb.miss[at] = __popcll(gone);
    }
  }
}

// Launch 2.  Workgroup b: block b again, sensor tiles of 64.  A row whose first reading is missing looks back through
// the carry table for the nearest earlier block that has a real reading (64 blocks a round: a run of any length); the
// hold inside the block is "highest set bit of the ballot at or below my lane", one __shfl.  filled goes out along time
// as it was read; gt and valid are time-major, so the tile is transposed through score_keys_kernel's padded LDS tile and
// written along sensors.  A tick is kept when every sensor's ballot has its bit: the waves AND their rows' ballots over
// all tiles.  The workgroup of the LAST block also folds the counters of every sensor: the sum of its blocks' missing
// readings and the distance from its latest real reading to the last column.
__global__ __launch_bounds__(GDN_SERIES_WAVES * 64) void series_fill_kernel(
    const float* __restrict__ raw, int n, int t_raw, int w, int blocks, CarryTable tb, float* __restrict__ filled,
    float* __restrict__ gt, unsigned char* __restrict__ valid, unsigned char* __restrict__ keep,
    long long* __restrict__ counters) {
  __shared__ float tile[64][65];
  __shared__ unsigned long long row_mask[64];
  __shared__ unsigned long long wave_keep[GDN_SERIES_WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.x, c0 = b * GDN_SERIES_BLOCK, c = c0 + lane;
  const bool inside = c < t_raw;
  const int t = t_raw - w;
  unsigned long long kept = ~0ull;                                   // (wave uniform)
  for (int s0 = 0; s0 < n; s0 += 64) {
    for (int r = wv; r < 64; r += GDN_SERIES_WAVES) {
      const int i = s0 + r;
      if (i >= n) break;                                             // (wave uniform)
      const float v = inside ? raw[(size_t)i * t_raw + c] : 0.f;
      const bool real = inside && !series_missing(v);
      const unsigned long long mask = __ballot(real);
      // the latest real reading before this block: only a row that begins on a missing reading (or, for the
      // counters, the last block's row without any real reading) asks
      int before_col = -1;
      float before_val = 0.f;
      if (!(mask & 1ull)) {
        for (int base = b - 1; base >= 0; base -= 64) {
          const int bb = base - lane;
          const size_t at = (size_t)i * blocks + (bb >= 0 ? bb : 0);
          const int col = bb >= 0 ? tb.col[at] : -1;
          const float val = tb.val[at];
          const unsigned long long found = __ballot(col >= 0);
          if (found) {
            const int src = __ffsll((long long)found) - 1;           // the lowest lane = the nearest block
            before_col = __shfl(col, src);
            before_val = __shfl(val, src);
            break;
          }
        }
      }
      const unsigned long long upto = mask & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
      const int src = upto ? 63 - __clzll((long long)upto) : lane;
      const float held = __shfl(v, src);
      const float out = upto ? held : before_val;                    // (no real reading at all so far: 0, caller's duty)
      if (inside) filled[(size_t)i * t_raw + c] = out;
      tile[r][lane] = out;
      if (lane == 0) row_mask[r] = mask;
      kept &= mask;
      if (b == blocks - 1) {
        int total = 0;
        for (int bb = lane; bb < blocks; bb += 64) total += tb.miss[(size_t)i * blocks + bb];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) total += __shfl_xor(total, d);
        const int last_col = mask ? c0 + 63 - __clzll((long long)mask) : before_col;
        const int run = min(t, t_raw - 1 - last_col);
        if (lane == 0) {
          counters[i] = total;
          counters[(size_t)n + i] = run;
        }
      }
    }
    __syncthreads();
    const int s = s0 + lane;                                         // now the lane runs along the sensors
    if (s < n) {
      const unsigned long long mask = row_mask[lane];
      for (int r = wv; r < 64; r += GDN_SERIES_WAVES) {
        const int j = c0 + r - w;                                    // the scored tick of column c0 + r
        if (j >= 0 && j < t) {
          gt[(size_t)j * n + s] = tile[lane][r];
          valid[(size_t)j * n + s] = (unsigned char)((mask >> r) & 1ull);
        }
      }
    }
    __syncthreads();                                                 // the tile is rewritten by the next sensor tile
  }
  if (lane == 0) wave_keep[wv] = kept;
  __syncthreads();
  if (wv == 0) {
    unsigned long long all = ~0ull;
#pragma unroll
    for (int v = 0; v < GDN_SERIES_WAVES; ++v) all &= wave_keep[v];
    const int j = c - w;
    if (j >= 0 && j < t) keep[j] = (unsigned char)((all >> lane) & 1ull);
  }
}

// score_keys_kernel (gdn_score.hip) with the keep flags: a tick that is not kept gets the filler in all n keys.
__global__ __launch_bounds__(256) void score_keys_keep_kernel(const float* __restrict__ pred,
                                                              const float* __restrict__ gt,
                                                              const unsigned char* __restrict__ keep, int t, int n,
                                                              int pitch, double* __restrict__ keys) {
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
  const int tick = t0 + lane;
  const bool real = tick < t && keep[tick] != 0;
  for (int r = wv; r < 64; r += 4) {
    const int s = s0 + r;
    if (s < n && tick < pitch)
      keys[(size_t)s * pitch + tick] = real ? tile[lane][r] : filler_key();
  }
}

bool series_shape_ok(int n, int t_raw, int w) { return n >= 1 && n <= 4096 && w >= 1 && t_raw > w; }

int series_blocks(int t_raw) { return (t_raw + GDN_SERIES_BLOCK - 1) / GDN_SERIES_BLOCK; }

}  // namespace

extern "C" long long gdn_series_fill_workspace_bytes(int n, int t_raw) {
  if (!series_shape_ok(n, t_raw, 1)) return 0;
  return (12ll * n * series_blocks(t_raw) + 7) & ~7ll;
}

extern "C" int gdn_series_fill(const float* raw, int n, int t_raw, int w, float* filled, float* gt, uint8_t* valid,
                               uint8_t* keep, int64_t* counters, void* workspace, void* stream) {
  if (!raw || !filled || !gt || !valid || !keep || !counters || !workspace || filled == raw) return GDN_ERR_ARG;
  if (!series_shape_ok(n, t_raw, w)) return GDN_ERR_UNSUPPORTED;
  const int blocks = series_blocks(t_raw);
  const CarryTable tb = carry_table(workspace, n, blocks);
  hipLaunchKernelGGL(series_carry_kernel, dim3(blocks), dim3(GDN_SERIES_WAVES * 64), 0, (hipStream_t)stream, raw, n,
                     t_raw, w, blocks, tb);
  const int rc = gdn_launch_status();
  if (rc != GDN_OK) return rc;
  hipLaunchKernelGGL(series_fill_kernel, dim3(blocks), dim3(GDN_SERIES_WAVES * 64), 0, (hipStream_t)stream, raw, n,
                     t_raw, w, blocks, tb, filled, gt, valid, keep, reinterpret_cast<long long*>(counters));
  return gdn_launch_status();
}

extern "C" int gdn_score_keys_keep(const float* pred, const float* gt, const uint8_t* keep, int t, int n, int pitch,
                                   double* keys, void* stream) {
  if (!pred || !gt || !keep || !keys || t <= 0 || n <= 0 || pitch < t) return GDN_ERR_ARG;
  hipLaunchKernelGGL(score_keys_keep_kernel, dim3((pitch + 63) / 64, (n + 63) / 64), dim3(256), 0,
                     (hipStream_t)stream, pred, gt, keep, t, n, pitch, keys);
  return gdn_launch_status();
}
