// Training epochs from the resident series (include/gdn_hip.h "epochs from the resident series"): the window gather
// of a training step (with the validity bytes of its targets when the series has missing readings), the cursor /
// loss-table bookkeeping between two steps of a captured epoch, and the validation loss (plain and masked).  Plain copy and reduction kernels: no LDS staging of the data, no inline assembly, no floating-point atomics.
#include "gdn_common.hpp"

namespace {

#define GDN_GATHER_THREADS 256
#define GDN_GATHER_PER_THREAD 4      // flat elements per thread, GDN_GATHER_THREADS apart: four loads in flight
#define GDN_GATHER_SPAN (GDN_GATHER_THREADS * GDN_GATHER_PER_THREAD)

// Workgroup (b, chunk): elements [chunk * SPAN, (chunk + 1) * SPAN) of window b's flat [i, c] index.  Lanes run
// along that index: stores are consecutive floats, loads are runs of w consecutive floats of one sensor row.  The
// thread that holds a row's last column also fetches the row's target value: y needs no pass of its own.
// Every offset into `series` is 64-bit (n * series_len exceeds 2^31 elements for long recordings at 4096 sensors).
// GAPS (gdn_windows_gather_gaps): workgroup (b, chunk 0) also copies the n validity bytes of the target tick — one
// contiguous row of the time-major plane `vplane` [series_len - w, n], at a 64-bit byte offset and of any alignment,
// so byte by byte — into valid_out[b, :] and stores how many of them are set into row_valid[b] (a block reduction over
// at most 4096 bytes).  The plain instantiation has none of this: its code and resource figures are the former kernel's.
template <bool GAPS>
__global__ __launch_bounds__(GDN_GATHER_THREADS) void gdn_windows_gather_kernel(
    const float* __restrict__ series, int n, long long series_len, const long long* __restrict__ starts, long long count,
    const long long* __restrict__ cursor, long long first, int batch, int w, float* __restrict__ x_out,
    float* __restrict__ y_out, const unsigned char* __restrict__ vplane, unsigned char* __restrict__ valid_out,
    int* __restrict__ row_valid) {
  const int b = blockIdx.x;
  const long long e = first + (cursor ? cursor[0] * (long long)batch : 0ll) + b;
  long long t = -1;
  if (e >= 0 && e < count) t = starts[e];
  const bool valid = t >= w && t < series_len;       // an entry or a tick outside the data: zeros, nothing is read
  const unsigned nw = (unsigned)n * (unsigned)w;     // <= 4096 * 1024
  float* __restrict__ xb = x_out + (size_t)b * nw;
  float* __restrict__ yb = y_out + (size_t)b * n;
  const unsigned f0 = blockIdx.y * GDN_GATHER_SPAN + threadIdx.x;
#pragma unroll
  for (int j = 0; j < GDN_GATHER_PER_THREAD; ++j) {
    const unsigned f = f0 + j * GDN_GATHER_THREADS;
    if (f >= nw) break;
    const unsigned i = f / (unsigned)w, c = f - i * (unsigned)w;
    const bool last = c == (unsigned)w - 1u;
    if (!valid) {
      xb[f] = 0.f;
      if (last) yb[i] = 0.f;
      continue;
    }
    const float* __restrict__ row = series + (long long)i * series_len + (t - w);
    xb[f] = row[c];
    if (last) yb[i] = row[w];
  }
  if constexpr (GAPS) {
    if (blockIdx.y != 0) return;                     // the validity row is written once per window
    __shared__ int cnt[GDN_GATHER_THREADS];
    const unsigned char* __restrict__ vrow = vplane + (valid ? (t - w) * (long long)n : 0ll);
    unsigned char* __restrict__ vb = valid_out + (size_t)b * n;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += GDN_GATHER_THREADS) {
      const unsigned char v = valid ? vrow[i] : (unsigned char)0;
      vb[i] = v;
      c += v != 0;
    }
    cnt[threadIdx.x] = c;
    __syncthreads();
    for (int s = GDN_GATHER_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) cnt[threadIdx.x] += cnt[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) row_valid[b] = cnt[0];
  }
}

// One thread between two steps of an epoch: the step's loss into its row of the table, the cursor on.  A launch of
// its own, stream-ordered after the step: every workgroup of the step's gather has read the cursor by then.
__global__ void gdn_epoch_advance_kernel(const float* __restrict__ loss, long long* __restrict__ cursor,
                                         float* __restrict__ loss_table, long long table_len) {
  const long long r = cursor[0];
  if (r >= 0 && r < table_len) loss_table[r] = loss[0];
  cursor[0] = r + 1;
}

// Workgroup q: mean((pred - y)^2) over the rows of logical minibatch q (the last one ragged).  The difference in
// fp32 (F.mse_loss forms it in the tensors' type), squares accumulated in float64: per-thread strided chains, then
// an LDS tree — a fixed order, so two runs give the same bits.
__global__ __launch_bounds__(256) void gdn_mse_batch_means_kernel(const float* __restrict__ pred,
                                                                  const float* __restrict__ y, long long rows, int n,
                                                                  long long batch, double* __restrict__ batch_means) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * batch;
  const long long r1 = r0 + batch < rows ? r0 + batch : rows;
  const long long lo = r0 * n, hi = r1 * n;
  double acc = 0.0;
  for (long long i = lo + tid; i < hi; i += 256) {
    const float df = pred[i] - y[i];
    acc = fma((double)df, (double)df, acc);
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) batch_means[blockIdx.x] = red[0] / (double)(hi - lo);
}

// test.py's `sum(losses) / len(losses)`: the batch means added in batch order by one thread
__global__ void gdn_mse_mean_of_means_kernel(const double* __restrict__ batch_means, long long batches,
                                             double* __restrict__ mean) {
  double s = 0.0;
  for (long long q = 0; q < batches; ++q) s += batch_means[q];
  mean[0] = s / (double)batches;
}

// gdn_mse_batch_means_kernel with the validity bytes of the targets: the squares of the real targets and their number
// go through the same strided chains and the same LDS tree; a masked slot is SELECTED out (its pred / y may hold
// anything).  A minibatch without a real target has mean 0 and count 0.
__global__ __launch_bounds__(256) void gdn_mse_batch_means_masked_kernel(
    const float* __restrict__ pred, const float* __restrict__ y, const unsigned char* __restrict__ valid, long long rows,
    int n, long long batch, double* __restrict__ batch_means, long long* __restrict__ batch_counts) {
  __shared__ double red[256];
  __shared__ long long cnt[256];
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * batch;
  const long long r1 = r0 + batch < rows ? r0 + batch : rows;
  const long long lo = r0 * n, hi = r1 * n;
  double acc = 0.0;
  long long c = 0;
  for (long long i = lo + tid; i < hi; i += 256) {
    const bool v = valid[i] != 0;
    const float df = pred[i] - y[i];
    acc = v ? fma((double)df, (double)df, acc) : acc;
    c += v;
  }
  red[tid] = acc;
  cnt[tid] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      cnt[tid] += cnt[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    batch_means[blockIdx.x] = cnt[0] ? red[0] / (double)cnt[0] : 0.0;
    batch_counts[blockIdx.x] = cnt[0];
  }
}

// sum(losses) / len(losses) over the minibatches that have a real target, in batch order; 0 when none has
__global__ void gdn_mse_mean_of_means_masked_kernel(const double* __restrict__ batch_means,
                                                    const long long* __restrict__ batch_counts, long long batches,
                                                    double* __restrict__ mean) {
  double s = 0.0;
  long long used = 0;
  for (long long q = 0; q < batches; ++q)
    if (batch_counts[q] > 0) {
      s += batch_means[q];
      ++used;
    }
  mean[0] = used ? s / (double)used : 0.0;
}

}  // namespace

extern "C" int gdn_windows_gather(const float* series, int n, long long series_len, const int64_t* starts,
                                  long long count, const int64_t* cursor, long long first, int batch, int w,
                                  float* x_out, float* y_out, void* stream) {
  if (!series || !starts || !x_out || !y_out) return GDN_ERR_ARG;
  if (batch < 1 || count < 1 || series_len < 1 || first < 0) return GDN_ERR_ARG;
  if (w < 1 || w > GDN_LONG_MAX_W || n < 1 || n > 4096) return GDN_ERR_UNSUPPORTED;
  const unsigned nw = (unsigned)n * (unsigned)w;
  const dim3 grid((unsigned)batch, (nw + GDN_GATHER_SPAN - 1) / GDN_GATHER_SPAN);
  hipLaunchKernelGGL(gdn_windows_gather_kernel<false>, grid, dim3(GDN_GATHER_THREADS), 0, (hipStream_t)stream, series,
                     n, series_len, reinterpret_cast<const long long*>(starts), count,
                     reinterpret_cast<const long long*>(cursor), first, batch, w, x_out, y_out,
                     (const unsigned char*)nullptr, (unsigned char*)nullptr, (int*)nullptr);
  return gdn_launch_status();
}

extern "C" int gdn_windows_gather_gaps(const float* series, int n, long long series_len, const int64_t* starts,
                                       long long count, const int64_t* cursor, long long first, int batch, int w,
                                       float* x_out, float* y_out, const uint8_t* valid, uint8_t* valid_out,
                                       int* row_valid, void* stream) {
  if (!series || !starts || !x_out || !y_out || !valid || !valid_out || !row_valid) return GDN_ERR_ARG;
  if (batch < 1 || count < 1 || series_len < 1 || first < 0) return GDN_ERR_ARG;
  if (w < 1 || w > GDN_LONG_MAX_W || n < 1 || n > 4096) return GDN_ERR_UNSUPPORTED;
  if (series_len <= w) return GDN_ERR_ARG;          // the plane has series_len - w rows
  const unsigned nw = (unsigned)n * (unsigned)w;
  const dim3 grid((unsigned)batch, (nw + GDN_GATHER_SPAN - 1) / GDN_GATHER_SPAN);
  hipLaunchKernelGGL(gdn_windows_gather_kernel<true>, grid, dim3(GDN_GATHER_THREADS), 0, (hipStream_t)stream, series,
                     n, series_len, reinterpret_cast<const long long*>(starts), count,
                     reinterpret_cast<const long long*>(cursor), first, batch, w, x_out, y_out, valid, valid_out,
                     row_valid);
  return gdn_launch_status();
}

extern "C" int gdn_epoch_advance(const float* loss, int64_t* cursor, float* loss_table, long long table_len,
                                 void* stream) {
  if (!loss || !cursor || !loss_table || table_len < 1) return GDN_ERR_ARG;
  hipLaunchKernelGGL(gdn_epoch_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss,
                     reinterpret_cast<long long*>(cursor), loss_table, table_len);
  return gdn_launch_status();
}

extern "C" int gdn_mse_batch_means(const float* pred, const float* y, long long rows, int n, long long batch,
                                   double* batch_means, double* mean, void* workspace, void* stream) {
  (void)workspace;      // the two launches below hand over through batch_means alone
  if (!pred || !y || !batch_means || !mean) return GDN_ERR_ARG;
  if (rows < 1 || batch < 1) return GDN_ERR_ARG;
  if (n < 1 || n > 4096) return GDN_ERR_UNSUPPORTED;
  const long long batches = (rows + batch - 1) / batch;
  if (batches > 0x7fffffffll) return GDN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gdn_mse_batch_means_kernel, dim3((unsigned)batches), dim3(256), 0, st, pred, y, rows, n, batch,
                     batch_means);
  hipLaunchKernelGGL(gdn_mse_mean_of_means_kernel, dim3(1), dim3(1), 0, st, batch_means, batches, mean);
  return gdn_launch_status();
}

extern "C" int gdn_mse_batch_means_masked(const float* pred, const float* y, const uint8_t* valid, long long rows, int n,
                                          long long batch, double* batch_means, int64_t* batch_counts, double* mean,
                                          void* workspace, void* stream) {
  (void)workspace;
  if (!pred || !y || !valid || !batch_means || !batch_counts || !mean) return GDN_ERR_ARG;
  if (rows < 1 || batch < 1) return GDN_ERR_ARG;
  if (n < 1 || n > 4096) return GDN_ERR_UNSUPPORTED;
  const long long batches = (rows + batch - 1) / batch;
  if (batches > 0x7fffffffll) return GDN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gdn_mse_batch_means_masked_kernel, dim3((unsigned)batches), dim3(256), 0, st, pred, y, valid, rows,
                     n, batch, batch_means, reinterpret_cast<long long*>(batch_counts));
  hipLaunchKernelGGL(gdn_mse_mean_of_means_masked_kernel, dim3(1), dim3(1), 0, st, batch_means,
                     reinterpret_cast<const long long*>(batch_counts), batches, mean);
  return gdn_launch_status();
}
