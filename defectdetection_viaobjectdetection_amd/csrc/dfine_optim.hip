// The end of the D-FINE trainers' step (include/mi355yolo.h: m355_dfine_grad_sumsq_launch, _clip_scale_launch, _adam_launch):
// torch.nn.utils.clip_grad_norm_ and the Adam / AdamW update of a whole parameter list, each pass ONE launch over all tensors.
// fp32 tensors, no float atomics, every sum in an order that the table alone decides: bitwise reproducible.  The squared norm and
// the clip coefficient are formed in double (dfine_grad_norm_kernel says why).
//
// The kernels work from a device table, one m355_dfine_optim_row per tensor.  A tensor is cut into chunks of kChunk elements and a
// block takes one chunk: the row's chunk0 is the number of chunks of the rows before it (the caller builds that prefix, the entry
// checks it), and a block finds the last row with chunk0 <= blockIdx.x by bisection.  The loads of that search depend on blockIdx
// alone, so they are scalar loads of a table that stays in L2.
//
// Alignment.  kChunk is a multiple of 4, so every chunk of a tensor starts at the tensor's own offset from 16 bytes.  Where all
// pointers of a pass (g; or p, g, m, v) share that offset the chunk is [head of <= 3 elements | float4 body | tail of <= 3]
// with 16-byte accesses in the body; where they differ (a parameter that is a 4-byte-aligned view of a flat buffer, its gradient
// and moments allocated on their own) every access of the chunk is 4 bytes wide, still contiguous across the wave.
//
// Arithmetic.  This file is compiled with -ffp-contract=off: every written operation rounds once, a fused multiply-add is written
// as fmaf.  sqrtf and the divisions are hipcc's default correctly rounded ones (no -ffast-math, no
// -fno-hip-fp32-correctly-rounded-divide-sqrt).  The update is torch 2.10's _multi_tensor_adam pass by pass, one rounding where a
// pass stores its result, fmaf where a pass computes a + s * b.
#include "../../include/mi355yolo.h"
#include "common.h"

namespace m355 {
namespace {

using Row = m355_dfine_optim_row;
constexpr int kThreads = 256;
constexpr int kChunk = M355_DFINE_OPTIM_CHUNK;
static_assert(sizeof(Row) == 96 && kChunk % 4 == 0, "the table layout that dfine.py writes");

struct Span {
  int row;
  long start;   // first element of the chunk in its tensor
  int len;      // 1 .. kChunk
};

// The chunk of this block.  Rows without elements own no chunk and share the chunk0 of the row after them: the LAST row with
// chunk0 <= chunk is the one that has it.
__device__ __forceinline__ Span find_span(const Row* __restrict__ table, int count) {
  const int chunk = blockIdx.x;
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
  }
  Span s;
  s.row = lo;
  s.start = (long)(chunk - table[lo].chunk0) * kChunk;
  const long left = table[lo].numel - s.start;
  s.len = left < kChunk ? (int)left : kChunk;
  return s;
}

__device__ __forceinline__ unsigned off16(const void* p) { return (unsigned)((uintptr_t)p & 15u); }
// elements in front of the first 16-byte boundary of a chunk that starts at p and has len elements
__device__ __forceinline__ int head_of(const void* p, int len) {
  const int h = (int)(((16u - off16(p)) & 15u) >> 2);
  return h < len ? h : len;
}

// the block's sum of one value per thread: wave shuffles, then the four wave sums in wave order.  Valid in thread 0.
__device__ __forceinline__ double block_sum(double s) {
  __shared__ double wsum[kThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// partials[chunk] = sum of g^2 over the chunk, added in double (every square is exact there) and rounded once.  A thread adds its
// elements in the order head, body, tail.
__global__ __launch_bounds__(kThreads) void dfine_grad_sumsq_kernel(const Row* __restrict__ table, int count,
                                                                    float* __restrict__ partials) {
  const Span sp = find_span(table, count);
  const float* g = table[sp.row].g + sp.start;
  const int tid = threadIdx.x;
  const int head = head_of(g, sp.len), nvec = (sp.len - head) >> 2, tail0 = head + 4 * nvec;
  double s = 0.0;
  auto add = [&s](float x) { s += (double)x * (double)x; };
  if (tid < head) add(g[tid]);
  const float4* gv = reinterpret_cast<const float4*>(g + head);
  for (int i = tid; i < nvec; i += kThreads) {
    const float4 x = gv[i];
    add(x.x); add(x.y); add(x.z); add(x.w);
  }
  if (tail0 + tid < sp.len) add(g[tail0 + tid]);
  const double total = block_sum(s);
  if (tid == 0) partials[blockIdx.x] = (float)total;
}

// The norm and the clip coefficient from the n partials, in double: out[0] = (float)norm, norm = sqrt(sum), out[1] = (float)c and
// the double at out + 2 = c = min(1, max_norm / (norm + 1e-6)), NaN kept as torch.clamp keeps it.  The kernels that apply c
// multiply in double and round once, so the clip adds no error of its own to a gradient.  One block: thread t adds partials
// t, t + 256, ... in that order, then the 256 sums fold in halves.  The order depends on n alone.
__global__ __launch_bounds__(kThreads) void dfine_grad_norm_kernel(const float* __restrict__ partials, int n, float max_norm,
                                                                   float* __restrict__ out) {
  __shared__ double ts[kThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) s += (double)partials[i];
  ts[threadIdx.x] = s;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) ts[threadIdx.x] += ts[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double norm = sqrt(ts[0]);
    double c = (double)max_norm / (norm + 1e-6);
    c = c > 1.0 ? 1.0 : c;
    out[0] = (float)norm;
    out[1] = (float)c;
    reinterpret_cast<double*>(out)[1] = c;
  }
}

__device__ __forceinline__ double clip_of(const float* coef) { return reinterpret_cast<const double*>(coef)[1]; }
__device__ __forceinline__ float clipped(float g, double c) { return (float)((double)g * c); }

// g = g c in place, c the double of dfine_grad_norm_kernel.  A coefficient of exactly 1 gives every bit back; the pass runs all the
// same, as torch's does: its time does not depend on the data.
__global__ __launch_bounds__(kThreads) void dfine_clip_scale_kernel(const Row* __restrict__ table, int count,
                                                                    const float* __restrict__ coef) {
  const double c = clip_of(coef);
  const Span sp = find_span(table, count);
  float* g = table[sp.row].g + sp.start;
  const int tid = threadIdx.x;
  const int head = head_of(g, sp.len), nvec = (sp.len - head) >> 2, tail0 = head + 4 * nvec;
  if (tid < head) g[tid] = clipped(g[tid], c);
  float4* gv = reinterpret_cast<float4*>(g + head);
  for (int i = tid; i < nvec; i += kThreads) {
    float4 x = gv[i];
    x.x = clipped(x.x, c); x.y = clipped(x.y, c); x.z = clipped(x.z, c); x.w = clipped(x.w, c);
    gv[i] = x;
  }
  if (tail0 + tid < sp.len) g[tail0 + tid] = clipped(g[tail0 + tid], c);
}

struct Scalars {
  float wd, beta2, eps, neg_step_size, bc2_sqrt, omb1, omb2, decay;
  double clip;
  bool clip_on, small_weight;
};

// One element of torch's update.  ADAMW: p *= 1 - lr wd; else g += wd p.  Then m = lerp(m, g, 1 - beta1),
// v = v beta2 + (1 - beta2) (g g), p += -step_size * (m / (sqrt(v) / bc2_sqrt + eps)).
template <bool ADAMW>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const Scalars& s) {
  if (s.clip_on) g = clipped(g, s.clip);
  if (s.wd != 0.f) {
    if (ADAMW) p = p * s.decay; else g = fmaf(s.wd, p, g);
  }
  const float diff = g - m;
  m = s.small_weight ? fmaf(s.omb1, diff, m) : g - diff * (1.f - s.omb1);   // at::native::lerp
  v = fmaf(s.omb2, g * g, v * s.beta2);
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = fmaf(s.neg_step_size, m / denom, p);
}

template <bool ADAMW>
__global__ __launch_bounds__(kThreads) void dfine_adam_kernel(const Row* __restrict__ table, int count,
                                                              const float* __restrict__ coef) {
  const Span sp = find_span(table, count);
  const Row& r = table[sp.row];
  float* p = r.p + sp.start;
  const float* g = r.g + sp.start;
  float* m = r.m + sp.start;
  float* v = r.v + sp.start;
  Scalars s;
  s.wd = r.weight_decay; s.beta2 = r.beta2; s.eps = r.eps; s.neg_step_size = -r.step_size; s.bc2_sqrt = r.bc2_sqrt;
  s.omb1 = r.one_minus_beta1; s.omb2 = r.one_minus_beta2; s.decay = r.decay;
  s.clip_on = coef != nullptr;
  s.clip = s.clip_on ? clip_of(coef) : 1.0;
  s.small_weight = fabsf(s.omb1) < 0.5f;
  const int tid = threadIdx.x;
  auto one = [&](int i) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_update<ADAMW>(pi, g[i], mi, vi, s);
    p[i] = pi; m[i] = mi; v[i] = vi;
  };
  const unsigned o = off16(p);
  if (off16(g) != o || off16(m) != o || off16(v) != o) {   // no common 16-byte phase: 4-byte accesses throughout
    for (int i = tid; i < sp.len; i += kThreads) one(i);
    return;
  }
  const int head = head_of(p, sp.len), nvec = (sp.len - head) >> 2, tail0 = head + 4 * nvec;
  if (tid < head) one(tid);
  if (tail0 + tid < sp.len) one(tail0 + tid);
  float4* pv = reinterpret_cast<float4*>(p + head);
  const float4* gv = reinterpret_cast<const float4*>(g + head);
  float4* mv = reinterpret_cast<float4*>(m + head);
  float4* vv = reinterpret_cast<float4*>(v + head);
  for (int i = tid; i < nvec; i += kThreads) {
    float4 pi = pv[i], mi = mv[i], vi = vv[i];
    const float4 gi = gv[i];
    adam_update<ADAMW>(pi.x, gi.x, mi.x, vi.x, s);
    adam_update<ADAMW>(pi.y, gi.y, mi.y, vi.y, s);
    adam_update<ADAMW>(pi.z, gi.z, mi.z, vi.z, s);
    adam_update<ADAMW>(pi.w, gi.w, mi.w, vi.w, s);
    pv[i] = pi; mv[i] = mi; vv[i] = vi;
  }
}

}  // namespace

int launch_dfine_grad_sumsq(const void* d_table, int count, int chunks, float* partials, hipStream_t s) {
  hipLaunchKernelGGL(dfine_grad_sumsq_kernel, dim3(chunks), dim3(kThreads), 0, s, (const Row*)d_table, count, partials);
  return (int)hipGetLastError();
}

int launch_dfine_grad_norm(const float* partials, int chunks, float max_norm, float* norm, hipStream_t s) {
  hipLaunchKernelGGL(dfine_grad_norm_kernel, dim3(1), dim3(kThreads), 0, s, partials, chunks, max_norm, norm);
  return (int)hipGetLastError();
}

int launch_dfine_clip_scale(const void* d_table, int count, int chunks, const float* norm, hipStream_t s) {
  hipLaunchKernelGGL(dfine_clip_scale_kernel, dim3(chunks), dim3(kThreads), 0, s, (const Row*)d_table, count, norm);
  return (int)hipGetLastError();
}

int launch_dfine_adam(const void* d_table, int count, int chunks, bool adamw, const float* norm, hipStream_t s) {
  if (adamw) hipLaunchKernelGGL(dfine_adam_kernel<true>, dim3(chunks), dim3(kThreads), 0, s, (const Row*)d_table, count, norm);
  else hipLaunchKernelGGL(dfine_adam_kernel<false>, dim3(chunks), dim3(kThreads), 0, s, (const Row*)d_table, count, norm);
  return (int)hipGetLastError();
}

}  // namespace m355
