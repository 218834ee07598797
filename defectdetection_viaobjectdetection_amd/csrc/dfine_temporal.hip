// The temporal head of the D-FINE trainers: what lies between the temporal encoder / context GRU and the loss or the
// post-processing, besides the nn.Linear heads (torch GEMMs) and the guarded box decode (dfine_kernels.hip, dfine_backward.hip).
// fp32, contiguous tensors, no float atomics, every reduction in a fixed order: bitwise reproducible.
//
//   temporal_fuse     out[t, q, :] = fused[t, q, :] * softmax_t(scores[:, q])[t] (+ context[t, q, :]).  Forward: a block per (query
//                     column, chunk of 16 frames); every block forms the column's max and log-sum itself, in one order, so a column
//                     does not depend on the grid or on the other columns.  Backward: ONE block owns a column: d_fused = g * w,
//                     dw[t] = sum_d g * fused into LDS, then d_scores = w * (dw - sum_t w * dw).  w is formed again from the scores
//                     and the saved (max, log-sum), as the attention kernel does.  D % 4 != 0 or a base that is not 16-byte aligned
//                     takes the 4-byte instance of the same template.
//   guard_logits      nan_to_num(clamp(cls (+ anomaly on all but the last column), -bound, bound)); one rounding per element, torch's
//                     gradient mask (-bound <= v <= bound passes).
//   noobject_loss     out[t] = mean_q (logsumexp(x[t, q, :]) - x[t, q, cls]): a block per frame; backward g[t] / Q * (softmax - onehot)
//                     over all rows, nothing read but the logits.
//   consistency_loss  (1 / (T - 1)) sum_{t >= 1} mean((a[t] - a[t - 1])^2): per (frame, chunk of 4096) partial sums into a workspace,
//                     then one wave adds them in a fixed order; backward one elementwise launch.
// The launchers validate nothing (dfine_entries.hip does).  Compiled with -ffp-contract=off: one rounding per written operation.
#include <math.h>

#include "common.h"
#include "device_prims.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int TF_THREADS = 256, TF_WAVES = TF_THREADS / 64;
constexpr int TF_ROWS = 4;                      // frames per wave in flight
constexpr int TF_CHUNK = TF_WAVES * TF_ROWS;    // frames per forward block
constexpr int TFB_THREADS = 512, TFB_WAVES = TFB_THREADS / 64;
constexpr int TF_MAX_T = 1024;
constexpr int EW_THREADS = 256;
constexpr int CL_CHUNK = 4096;                  // elements per consistency partial: a function of the shape alone
constexpr int NO_MAX_Q = 2048;

int ew_grid(long n) {   // blocks of EW_THREADS for a grid-stride loop over n elements: 16 per CU at the most
  const int cus = num_cus();
  if (cus <= 0) return -1;
  const long need = (n + EW_THREADS - 1) / EW_THREADS, cap = (long)cus * 16;
  return (int)(need < 1 ? 1 : (need < cap ? need : cap));
}

__device__ __forceinline__ float dot4(float4v a, float4v b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }
__device__ __forceinline__ float dot4(float a, float b) { return a * b; }

// (max, log of the sum of exp(s - max)) of column q of scores (T, Q): lane-strided passes and xor butterflies, so every lane of
// every wave of every block that asks ends with the same bits
__device__ __forceinline__ float2 column_stats(const float* __restrict__ scores, int T, int Q, int q, int lane) {
  float m = -INFINITY;
  for (int t = lane; t < T; t += 64) m = fmaxf(m, scores[(size_t)t * Q + q]);
  m = wave_max(m);
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += expf(scores[(size_t)t * Q + q] - m);
  s = wave_sum(s);
  return make_float2(m, logf(s));
}
__device__ __forceinline__ float column_weight(float score, float2 st) { return expf((score - st.x) - st.y); }

// V = float4v: 16-byte accesses (every base 16-byte aligned, D % 4 == 0), V = float: 4-byte accesses.  grid (Q, chunks of T)
template <class V>
__global__ __launch_bounds__(TF_THREADS) void dfine_tfuse_fwd_kernel(const float* __restrict__ fused, const float* __restrict__ scores,
                                                                      const float* __restrict__ ctx, float* __restrict__ out,
                                                                      float* __restrict__ stats, int T, int Q, int D) {
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float2 st = column_stats(scores, T, Q, q, lane);
  if (stats && blockIdx.y == 0 && threadIdx.x == 0) {
    stats[q] = st.x;
    stats[(size_t)Q + q] = st.y;
  }
  const int units = D / (int)(sizeof(V) / sizeof(float));
  const int t0 = blockIdx.y * TF_CHUNK + wave * TF_ROWS;
  float w[TF_ROWS];
  size_t row[TF_ROWS];
#pragma unroll
  for (int j = 0; j < TF_ROWS; ++j) {   // a frame past the end reads the last frame and stores nothing
    const int t = min(t0 + j, T - 1);
    w[j] = column_weight(scores[(size_t)t * Q + q], st);
    row[j] = ((size_t)t * Q + q) * D;
  }
  for (int u = lane; u < units; u += 64) {
    V f[TF_ROWS], c[TF_ROWS];
#pragma unroll
    for (int j = 0; j < TF_ROWS; ++j) {
      f[j] = ((const V*)(fused + row[j]))[u];
      c[j] = ctx ? ((const V*)(ctx + row[j]))[u] : V{};
    }
#pragma unroll
    for (int j = 0; j < TF_ROWS; ++j)
      if (t0 + j < T) ((V*)(out + row[j]))[u] = ctx ? f[j] * w[j] + c[j] : f[j] * w[j];
  }
}

// One block per query column.  d_fused and d_scores may each be nullptr; `fused` is read for d_scores only.
template <class V>
__global__ __launch_bounds__(TFB_THREADS) void dfine_tfuse_bwd_kernel(const float* __restrict__ g, const float* __restrict__ fused,
                                                                       const float* __restrict__ scores, const float* __restrict__ stats,
                                                                       float* __restrict__ d_fused, float* __restrict__ d_scores, int T,
                                                                       int Q, int D) {
  __shared__ float dw[TF_MAX_T];
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float2 st = make_float2(stats[q], stats[(size_t)Q + q]);
  const int units = D / (int)(sizeof(V) / sizeof(float));
  for (int t0 = wave * TF_ROWS; t0 < T; t0 += TFB_WAVES * TF_ROWS) {   // wave-uniform trip count: the butterflies are whole
    float w[TF_ROWS], acc[TF_ROWS];
    size_t row[TF_ROWS];
#pragma unroll
    for (int j = 0; j < TF_ROWS; ++j) {
      const int t = min(t0 + j, T - 1);
      w[j] = column_weight(scores[(size_t)t * Q + q], st);
      row[j] = ((size_t)t * Q + q) * D;
      acc[j] = 0.f;
    }
    for (int u = lane; u < units; u += 64) {
      V gv[TF_ROWS], f[TF_ROWS];
#pragma unroll
      for (int j = 0; j < TF_ROWS; ++j) {
        gv[j] = ((const V*)(g + row[j]))[u];
        f[j] = d_scores ? ((const V*)(fused + row[j]))[u] : V{};
      }
#pragma unroll
      for (int j = 0; j < TF_ROWS; ++j) {
        if (d_fused && t0 + j < T) ((V*)(d_fused + row[j]))[u] = gv[j] * w[j];
        acc[j] += dot4(gv[j], f[j]);
      }
    }
    if (d_scores) {
#pragma unroll
      for (int j = 0; j < TF_ROWS; ++j) {
        const float s = wave_sum(acc[j]);
        if (lane == 0 && t0 + j < T) dw[t0 + j] = s;
      }
    }
  }
  if (!d_scores) return;   // uniform for the block
  __syncthreads();
  float dot = 0.f;         // sum_t w dw: every wave forms it, in one order
  for (int t = lane; t < T; t += 64) dot += column_weight(scores[(size_t)t * Q + q], st) * dw[t];
  dot = wave_sum(dot);
  for (int t = threadIdx.x; t < T; t += TFB_THREADS)
    d_scores[(size_t)t * Q + q] = column_weight(scores[(size_t)t * Q + q], st) * (dw[t] - dot);
}

// v = cls[r, c] (+ anomaly[r, c] for c < C1 - 1): what torch's clamp and nan_to_num see
__device__ __forceinline__ float guard_value(const float* __restrict__ cls, const float* __restrict__ an, long i, int C1) {
  float v = cls[i];
  if (an) {
    const long r = i / C1;
    const int c = (int)(i - r * C1);
    if (c < C1 - 1) v += an[r * (C1 - 1) + c];
  }
  return v;
}
__global__ __launch_bounds__(EW_THREADS) void dfine_guard_logits_fwd_kernel(const float* __restrict__ cls, const float* __restrict__ an,
                                                                             float* __restrict__ out, long n, int C1, float bound) {
  for (long i = (long)blockIdx.x * EW_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * EW_THREADS) {
    const float v = guard_value(cls, an, i, C1);
    out[i] = v != v ? 0.f : (v < -bound ? -bound : (v > bound ? bound : v));
  }
}
__global__ __launch_bounds__(EW_THREADS) void dfine_guard_logits_bwd_kernel(const float* __restrict__ g, const float* __restrict__ cls,
                                                                             const float* __restrict__ an, float* __restrict__ d_cls,
                                                                             float* __restrict__ d_an, long n, int C1, float bound) {
  for (long i = (long)blockIdx.x * EW_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * EW_THREADS) {
    const float v = guard_value(cls, an, i, C1);
    const float d = (v >= -bound && v <= bound) ? g[i] : 0.f;   // false for NaN and +-inf
    if (d_cls) d_cls[i] = d;
    if (d_an) {
      const long r = i / C1;
      const int c = (int)(i - r * C1);
      if (c < C1 - 1) d_an[r * (C1 - 1) + c] = d;
    }
  }
}

// (max, sum of exp(x - max)) of a row of C floats that L lanes (a power of two, lanes sub .. of one wave) share
__device__ __forceinline__ float2 row_softmax_stats(const float* __restrict__ x, int C, int sub, int L) {
  float m = -INFINITY;
  for (int c = sub; c < C; c += L) m = fmaxf(m, x[c]);
  for (int o = L >> 1; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float s = 0.f;
  for (int c = sub; c < C; c += L) s += expf(x[c] - m);
  for (int o = L >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return make_float2(m, s);
}

// one block per frame: the Q row losses into LDS, then wave 0 adds them in a fixed order
__global__ __launch_bounds__(EW_THREADS) void dfine_noobject_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int Q, int C,
                                                                         int cls, int L) {
  __shared__ float loss[NO_MAX_Q];
  const int t = blockIdx.x, sub = threadIdx.x & (L - 1), group = threadIdx.x / L, G = EW_THREADS / L;
  const float* frame = x + (size_t)t * Q * C;
  for (int q0 = 0; q0 < Q; q0 += G) {   // block-uniform trip count; a row past the end reads the last row and stores nothing
    const int q = min(q0 + group, Q - 1);
    const float* row = frame + (size_t)q * C;
    const float2 st = row_softmax_stats(row, C, sub, L);
    if (sub == 0 && q0 + group < Q) loss[q] = logf(st.y) - (row[cls] - st.x);
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = 0.f;
    for (int q = threadIdx.x; q < Q; q += 64) s += loss[q];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[t] = s / (float)Q;
  }
}
// every row of (T Q, C): d x = g[t] / Q * (softmax - onehot)
__global__ __launch_bounds__(EW_THREADS) void dfine_noobject_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                         float* __restrict__ dx, long rows, int Q, int C, int cls, int L) {
  const int sub = threadIdx.x & (L - 1), G = EW_THREADS / L;
  const long group = (long)blockIdx.x * G + threadIdx.x / L, step = (long)gridDim.x * G;
  for (long r0 = 0; r0 < rows; r0 += step) {   // grid-uniform trip count
    const long r = min(r0 + group, rows - 1);
    const float* row = x + (size_t)r * C;
    const float2 st = row_softmax_stats(row, C, sub, L);
    const float k = g[r / Q] / (float)Q;
    if (r0 + group < rows)
      for (int c = sub; c < C; c += L) dx[(size_t)r * C + c] = k * (expf(row[c] - st.x) / st.y - (c == cls ? 1.f : 0.f));
  }
}

// grid (T - 1, chunks): the sum of (a[t] - a[t - 1])^2 over one chunk of the frame's N elements
__global__ __launch_bounds__(EW_THREADS) void dfine_consistency_partial_kernel(const float* __restrict__ a, float* __restrict__ part, long N) {
  __shared__ float ws[EW_THREADS / 64];
  const long base = (long)(blockIdx.x + 1) * N, e0 = (long)blockIdx.y * CL_CHUNK;
  const long e1 = e0 + CL_CHUNK < N ? e0 + CL_CHUNK : N;
  float s = 0.f;
  for (long e = e0 + threadIdx.x; e < e1; e += EW_THREADS) {
    const float d = a[base + e] - a[base - N + e];
    s += d * d;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = ws[0];
    for (int w = 1; w < EW_THREADS / 64; ++w) tot += ws[w];
    part[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = tot;
  }
}
// one wave: frame f's chunks in order, / N, the frames lane-strided and a butterfly, / (T - 1)
__global__ __launch_bounds__(64) void dfine_consistency_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int frames,
                                                                    int chunks, float n) {
  float s = 0.f;
  for (int f = threadIdx.x; f < frames; f += 64) {
    float m = 0.f;
    for (int j = 0; j < chunks; ++j) m += part[(size_t)f * chunks + j];
    s += m / n;
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) out[0] = s / (float)frames;
}
// d a[t] = g k ((a[t] - a[t - 1]) [t >= 1] - (a[t + 1] - a[t]) [t < T - 1]), k = 2 / ((T - 1) N)
__global__ __launch_bounds__(EW_THREADS) void dfine_consistency_bwd_kernel(const float* __restrict__ g, const float* __restrict__ a,
                                                                            float* __restrict__ da, long total, long N, float k) {
  const float gk = g[0] * k;
  for (long i = (long)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * EW_THREADS) {
    const float x = a[i];
    float d = 0.f;
    if (i >= N) d = x - a[i - N];
    if (i + N < total) d -= a[i + N] - x;
    da[i] = gk * d;
  }
}

}  // namespace

int dfine_tfuse_max_t() { return TF_MAX_T; }
int dfine_noobject_max_q() { return NO_MAX_Q; }

int launch_dfine_tfuse_forward(const float* fused, const float* scores, const float* ctx, int T, int Q, int D, float* out, float* stats,
                               hipStream_t s) {
  const dim3 grid((unsigned)Q, (unsigned)((T + TF_CHUNK - 1) / TF_CHUNK));
  if (D % 4 == 0 && aligned16(fused) && aligned16(ctx) && aligned16(out))   // nullptr counts as aligned: it is not read
    hipLaunchKernelGGL(dfine_tfuse_fwd_kernel<float4v>, grid, dim3(TF_THREADS), 0, s, fused, scores, ctx, out, stats, T, Q, D);
  else
    hipLaunchKernelGGL(dfine_tfuse_fwd_kernel<float>, grid, dim3(TF_THREADS), 0, s, fused, scores, ctx, out, stats, T, Q, D);
  return (int)hipGetLastError();
}
int launch_dfine_tfuse_backward(const float* g, const float* fused, const float* scores, const float* stats, int T, int Q, int D,
                                float* d_fused, float* d_scores, hipStream_t s) {
  if (D % 4 == 0 && aligned16(g) && aligned16(fused) && aligned16(d_fused))
    hipLaunchKernelGGL(dfine_tfuse_bwd_kernel<float4v>, dim3((unsigned)Q), dim3(TFB_THREADS), 0, s, g, fused, scores, stats, d_fused,
                       d_scores, T, Q, D);
  else
    hipLaunchKernelGGL(dfine_tfuse_bwd_kernel<float>, dim3((unsigned)Q), dim3(TFB_THREADS), 0, s, g, fused, scores, stats, d_fused,
                       d_scores, T, Q, D);
  return (int)hipGetLastError();
}

int launch_dfine_guard_logits(const float* cls, const float* an, long rows, int C1, float bound, float* out, hipStream_t s) {
  const long n = rows * C1;
  const int grid = ew_grid(n);
  if (grid < 0) return -2;
  hipLaunchKernelGGL(dfine_guard_logits_fwd_kernel, dim3(grid), dim3(EW_THREADS), 0, s, cls, an, out, n, C1, bound);
  return (int)hipGetLastError();
}
int launch_dfine_guard_logits_backward(const float* g, const float* cls, const float* an, long rows, int C1, float bound, float* d_cls,
                                       float* d_an, hipStream_t s) {
  const long n = rows * C1;
  const int grid = ew_grid(n);
  if (grid < 0) return -2;
  hipLaunchKernelGGL(dfine_guard_logits_bwd_kernel, dim3(grid), dim3(EW_THREADS), 0, s, g, cls, an, d_cls, d_an, n, C1, bound);
  return (int)hipGetLastError();
}

int launch_dfine_noobject_forward(const float* x, int T, int Q, int C, int cls, float* out, hipStream_t s) {
  hipLaunchKernelGGL(dfine_noobject_fwd_kernel, dim3((unsigned)T), dim3(EW_THREADS), 0, s, x, out, Q, C, cls, lanes_per_row(C));
  return (int)hipGetLastError();
}
int launch_dfine_noobject_backward(const float* g, const float* x, int T, int Q, int C, int cls, float* dx, hipStream_t s) {
  const int L = lanes_per_row(C);
  const long rows = (long)T * Q;
  const int grid = ew_grid(rows * L);
  if (grid < 0) return -2;
  hipLaunchKernelGGL(dfine_noobject_bwd_kernel, dim3(grid), dim3(EW_THREADS), 0, s, g, x, dx, rows, Q, C, cls, L);
  return (int)hipGetLastError();
}

int dfine_consistency_chunks(long N) { return (int)((N + CL_CHUNK - 1) / CL_CHUNK); }
size_t dfine_consistency_workspace_bytes(int T, long N) {
  return T < 2 || N < 1 ? 0 : (size_t)(T - 1) * (size_t)dfine_consistency_chunks(N) * sizeof(float);
}
int launch_dfine_consistency_forward(const float* a, int T, long N, float* work, float* out, hipStream_t s) {
  const int chunks = dfine_consistency_chunks(N);
  hipLaunchKernelGGL(dfine_consistency_partial_kernel, dim3((unsigned)(T - 1), (unsigned)chunks), dim3(EW_THREADS), 0, s, a, work, N);
  hipLaunchKernelGGL(dfine_consistency_sum_kernel, dim3(1), dim3(64), 0, s, work, out, T - 1, chunks, (float)N);
  return (int)hipGetLastError();
}
int launch_dfine_consistency_backward(const float* g, const float* a, int T, long N, float* da, hipStream_t s) {
  const long total = (long)T * N;
  const int grid = ew_grid(total);
  if (grid < 0) return -2;
  const float k = (float)(2.0 / ((double)(T - 1) * (double)N));
  hipLaunchKernelGGL(dfine_consistency_bwd_kernel, dim3(grid), dim3(EW_THREADS), 0, s, g, a, da, total, N, k);
  return (int)hipGetLastError();
}

}  // namespace m355
