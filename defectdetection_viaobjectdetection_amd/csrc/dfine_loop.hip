// The loop of a D-FINE decoder (transformers' DFineDecoder.forward) around its layers, between its GEMMs:
//   qp_fwd / qp_bwd (+ qp_reduce)   relu(ref @ weight.T + bias), the first Linear (K = 4) + ReLU of query_pos_head
//   rr_fwd / rr_bwd                 sigmoid(delta + inverse_sigmoid(ref)), the reference points of layer 0
//   rb_fwd / rb_bwd                 pred_corners = delta + prev and boxes = distance2bbox(points, integral(pred_corners)), per layer
// fp32 in, fp32 out, fp32 accumulation; no atomics: every sum has one owner and a fixed order, so results and gradients are
// bitwise reproducible.  Every per-row result (out, dref; the reference points; pred_corners, boxes, gcorners, gpoints) depends on
// its own row alone.  No workgroup waits on another.
//
// rb_*: a block owns RB_ROWS consecutive rows, one contiguous range of RB_ROWS * 4 * nb1 floats of each logit tensor.  It moves
// that range with 16-byte accesses, lane i next to lane i + 1, and stages it in LDS with one padded segment (nb1 | 1 floats: an
// odd stride, so the 32 lanes of a half wave read 32 banks) per box side; then thread t owns side t & 3 of row t >> 2, walks its
// segment serially (the order of dfine_decode_kernel: max, then sum and dot in one pass) and trades the four distances of its
// row inside its quad of lanes.  Boxes and gpoints leave as one float per lane, again contiguous across the wave.
#include <math.h>

#include "common.h"
#include "device_prims.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int QP_THREADS = 256;
constexpr int QP_ROWS = 4;          // forward: rows per thread, which keeps its 4 weight rows and biases in registers
constexpr int QP_SLAB_ROWS = 64;    // backward: rows of one block's slab while the slabs number QP_MAX_SLABS at the most
constexpr int QP_MAX_SLABS = 256;   // partial rows of dweight | dbias
constexpr int QP_REDUCE_THREADS = 64;   // one wave per block: 5 H / 64 blocks spread the columns over the CUs
constexpr int RB_THREADS = 128;
constexpr int RB_ROWS = RB_THREADS / 4;

__device__ __forceinline__ float relu_f(float v) { return v <= 0.f ? 0.f : v; }   // keeps NaN, as torch.relu
__device__ __forceinline__ float dot4b(const float4 x, const float4 w, float b) { return b + x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w; }

// thread = (group of QP_ROWS rows, 4 consecutive columns); consecutive lanes hold consecutive column groups of a row
__global__ __launch_bounds__(QP_THREADS) void qp_fwd_kernel(const float* ref, const float* w, const float* b, float* out, long N, int H4) {
  const long i = (long)blockIdx.x * QP_THREADS + threadIdx.x;
  const long g = i / H4;
  const int c = (int)(i - g * H4);
  if (g * QP_ROWS >= N) return;
  const float4* w4 = (const float4*)w + 4 * c;   // rows 4 c .. 4 c + 3 of weight (H, 4)
  const float4 w0 = w4[0], w1 = w4[1], w2 = w4[2], w3 = w4[3], bb = ((const float4*)b)[c];
#pragma unroll
  for (int r = 0; r < QP_ROWS; ++r) {
    const long n = g * QP_ROWS + r;
    if (n >= N) break;
    const float4 x = ((const float4*)ref)[n];
    float4 o;
    o.x = relu_f(dot4b(x, w0, bb.x)); o.y = relu_f(dot4b(x, w1, bb.y));
    o.z = relu_f(dot4b(x, w2, bb.z)); o.w = relu_f(dot4b(x, w3, bb.w));
    ((float4*)out)[n * H4 + c] = o;
  }
}

struct QpBwdArgs {
  const float *g, *out, *ref, *w;   // (N, H), (N, H): the forward's output, (N, 4), (H, 4)
  float* dref;                      // (N, 4) or nullptr
  float* part;                      // (slabs, 5 H): per slab dweight (H, 4) flat, then dbias (H); or nullptr
  long N;
  int H, H4, slab_rows;
};

// Block = one slab of rows; wave v takes rows v, v + 4, .. of it, lane l the 4 columns of column group c0 + l, chunk after chunk
// of 64 groups.  Per chunk a thread sums its 16 dweight and 4 dbias terms over its rows in row order, the four waves' sums are
// added in wave order into the slab's partial row.  dref of a row: the lanes' dots over their columns, a wave butterfly, and lane
// 0 adds the chunk's sum to what the chunks before it left (chunk order: fixed by H alone).
__global__ __launch_bounds__(QP_THREADS) void qp_bwd_kernel(const QpBwdArgs a) {
  __shared__ float red[4][64][21];   // 21: an odd stride between lanes
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * a.slab_rows;
  const long r1 = r0 + a.slab_rows < a.N ? r0 + a.slab_rows : a.N;
  const float4* g4 = (const float4*)a.g;
  const float4* o4 = (const float4*)a.out;
  for (int c0 = 0; c0 < a.H4; c0 += 64) {
    const int c = c0 + lane;
    const bool live = c < a.H4;
    float acc[20];
#pragma unroll
    for (int j = 0; j < 20; ++j) acc[j] = 0.f;
    float4 w0 = {0.f, 0.f, 0.f, 0.f}, w1 = w0, w2 = w0, w3 = w0;
    if (a.dref && live) {
      const float4* w4 = (const float4*)a.w + 4 * c;
      w0 = w4[0]; w1 = w4[1]; w2 = w4[2]; w3 = w4[3];
    }
    for (long n = r0 + wave; n < r1; n += 4) {
      float4 gm = {0.f, 0.f, 0.f, 0.f};
      if (live) {
        const float4 gv = g4[n * a.H4 + c], ov = o4[n * a.H4 + c];
        gm.x = ov.x <= 0.f ? 0.f : gv.x; gm.y = ov.y <= 0.f ? 0.f : gv.y;   // torch's threshold_backward on the result
        gm.z = ov.z <= 0.f ? 0.f : gv.z; gm.w = ov.w <= 0.f ? 0.f : gv.w;
      }
      const float4 x = ((const float4*)a.ref)[n];
      const float gmv[4] = {gm.x, gm.y, gm.z, gm.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[4 * j] += gmv[j] * x.x; acc[4 * j + 1] += gmv[j] * x.y; acc[4 * j + 2] += gmv[j] * x.z; acc[4 * j + 3] += gmv[j] * x.w;
        acc[16 + j] += gmv[j];
      }
      if (a.dref) {
        float4 d;
        d.x = wave_sum(gm.x * w0.x + gm.y * w1.x + gm.z * w2.x + gm.w * w3.x);
        d.y = wave_sum(gm.x * w0.y + gm.y * w1.y + gm.z * w2.y + gm.w * w3.y);
        d.z = wave_sum(gm.x * w0.z + gm.y * w1.z + gm.z * w2.z + gm.w * w3.z);
        d.w = wave_sum(gm.x * w0.w + gm.y * w1.w + gm.z * w2.w + gm.w * w3.w);
        if (lane == 0) {
          float4* p = (float4*)a.dref + n;
          if (c0) { const float4 o = *p; d.x = o.x + d.x; d.y = o.y + d.y; d.z = o.z + d.z; d.w = o.w + d.w; }
          *p = d;
        }
      }
    }
    if (a.part) {
#pragma unroll
      for (int j = 0; j < 20; ++j) red[wave][lane][j] = acc[j];
      __syncthreads();
      float* row = a.part + (long)blockIdx.x * 5 * a.H;
      for (int t = threadIdx.x; t < 64 * 20; t += QP_THREADS) {
        const int l = t / 20, j = t - l * 20, cc = c0 + l;
        if (cc < a.H4) {
          const float s = ((red[0][l][j] + red[1][l][j]) + red[2][l][j]) + red[3][l][j];
          row[j < 16 ? 16 * cc + j : 4 * a.H + 4 * cc + (j - 16)] = s;
        }
      }
      __syncthreads();
    }
  }
}

// dweight | dbias [t] = the slabs' partial rows added in slab order; 16 loads are in flight before the first add (one load per
// add made the launch a chain of 235 memory latencies at 15 000 rows: 55 us)
__global__ __launch_bounds__(QP_REDUCE_THREADS) void qp_reduce_kernel(const float* part, int slabs, int H, float* dweight, float* dbias) {
  const int t = blockIdx.x * QP_REDUCE_THREADS + threadIdx.x;
  if (t >= 5 * H) return;
  float* dst = t < 4 * H ? dweight : dbias;
  if (!dst) return;
  const float* col = part + t;
  const long step = 5L * H;
  float s = 0.f;
  int i = 0;
  for (; i + 16 <= slabs; i += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = col[(i + j) * step];
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j];
  }
  for (; i < slabs; ++i) s += col[i * step];
  dst[t < 4 * H ? t : t - 4 * H] = s;
}

int qp_slabs(long N) {
  const long s = (N + QP_SLAB_ROWS - 1) / QP_SLAB_ROWS;
  return (int)(s < QP_MAX_SLABS ? s : QP_MAX_SLABS);
}

// upstream's inverse_sigmoid, operation for operation (clamp keeps NaN), then the add and the sigmoid
__global__ __launch_bounds__(256) void rr_fwd_kernel(const float* delta, const float* ref, float* out, long n, float eps) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float x = ref[i];
  x = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
  const float x1 = x < eps ? eps : x;
  const float om = 1.f - x;
  const float x2 = om < eps ? eps : om;
  const float z = delta[i] + logf(x1 / x2);
  out[i] = 1.f / (1.f + expf(-z));
}
// torch's sigmoid_backward on the saved output
__global__ __launch_bounds__(256) void rr_bwd_kernel(const float* gout, const float* out, float* gdelta, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float y = out[i];
  gdelta[i] = gout[i] * (1.f - y) * y;
}

struct RbArgs {
  const float *corners, *prev;      // forward: delta and prev (or nullptr); backward: pred_corners, nullptr
  const float *project, *points;    // (nb1), (N, 4)
  float *pred, *boxes;              // forward: (N, 4 nb1), written when prev is given; (N, 4)
  const float *gpred, *gboxes;      // backward: (N, 4 nb1) or nullptr, (N, 4)
  float *gcorners, *gpoints;        // backward: (N, 4 nb1), (N, 4) or nullptr
  long N;
  int nb1;
  float rs;                         // |reg_scale|
};

// float4 i of the block's range holds flat elements 4 i .. 4 i + 3; element e is bin e % nb1 of side e / nb1
__device__ __forceinline__ void rb_scatter(float* z, int i, int nb1, int stride, const float4 v) {
  int s = 4 * i / nb1, k = 4 * i - s * nb1;
  const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    z[s * stride + k] = vv[j];
    if (++k == nb1) { k = 0; ++s; }
  }
}
__device__ __forceinline__ float4 rb_gather(const float* z, int i, int nb1, int stride) {
  int s = 4 * i / nb1, k = 4 * i - s * nb1;
  float vv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    vv[j] = z[s * stride + k];
    if (++k == nb1) { k = 0; ++s; }
  }
  return {vv[0], vv[1], vv[2], vv[3]};
}
// the side's expectation in dfine_decode_kernel's order; mx and sum for the backward
__device__ __forceinline__ float rb_expect(const float* zs, const float* project, int nb1, float& mx, float& sum) {
  float m = zs[0];
  for (int k = 1; k < nb1; ++k) m = fmaxf(m, zs[k]);
  float sm = 0.f, dot = 0.f;
  for (int k = 0; k < nb1; ++k) {
    const float e = expf(zs[k] - m);
    sm += e;
    dot += e * project[k];
  }
  mx = m; sum = sm;
  return dot / sm;
}

__global__ __launch_bounds__(RB_THREADS) void rb_fwd_kernel(const RbArgs a) {
  extern __shared__ float4 rb_smem4[];
  float* z = (float*)rb_smem4;
  const int nb1 = a.nb1, stride = nb1 | 1;
  const long row0 = (long)blockIdx.x * RB_ROWS;
  const int rows = a.N - row0 < RB_ROWS ? (int)(a.N - row0) : RB_ROWS;
  const int n4 = rows * nb1;   // 16-byte words of the block's range
  const float4* d4 = (const float4*)(a.corners + row0 * 4 * nb1);
  const float4* p4 = a.prev ? (const float4*)(a.prev + row0 * 4 * nb1) : nullptr;
  float4* o4 = a.prev ? (float4*)(a.pred + row0 * 4 * nb1) : nullptr;
  for (int i = threadIdx.x; i < n4; i += RB_THREADS) {
    float4 v = d4[i];
    if (p4) {
      const float4 p = p4[i];
      v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;   // torch's add: one rounding
      o4[i] = v;
    }
    rb_scatter(z, i, nb1, stride, v);
  }
  __syncthreads();
  const int t = threadIdx.x;
  const bool live = t < 4 * rows;
  float d = 0.f, mx, sum;
  if (live) d = rb_expect(z + t * stride, a.project, nb1, mx, sum);
  const int q = t & 60;   // the quad's first lane in its wave
  const float d0 = __shfl(d, q, 64), d1 = __shfl(d, q + 1, 64), d2 = __shfl(d, q + 2, 64), d3 = __shfl(d, q + 3, 64);
  if (!live) return;
  const long row = row0 + (t >> 2);
  const float4 pt = ((const float4*)a.points)[row];
  const float rs = a.rs;
  const float x0 = pt.x - (0.5f * rs + d0) * (pt.z / rs), y0 = pt.y - (0.5f * rs + d1) * (pt.w / rs);
  const float x1 = pt.x + (0.5f * rs + d2) * (pt.z / rs), y1 = pt.y + (0.5f * rs + d3) * (pt.w / rs);
  const int s = t & 3;
  a.boxes[row * 4 + s] = s == 0 ? (x0 + x1) / 2.f : (s == 1 ? (y0 + y1) / 2.f : (s == 2 ? x1 - x0 : y1 - y0));
}

// gcorners = gpred + p_k (project_k - d) gd, gd the gradient of the side's distance (dfine_decode_bwd_kernel's expressions)
__global__ __launch_bounds__(RB_THREADS) void rb_bwd_kernel(const RbArgs a) {
  extern __shared__ float4 rb_smem4[];
  float* z = (float*)rb_smem4;
  const int nb1 = a.nb1, stride = nb1 | 1;
  const long row0 = (long)blockIdx.x * RB_ROWS;
  const int rows = a.N - row0 < RB_ROWS ? (int)(a.N - row0) : RB_ROWS;
  const int n4 = rows * nb1;
  const float4* c4 = (const float4*)(a.corners + row0 * 4 * nb1);
  for (int i = threadIdx.x; i < n4; i += RB_THREADS) rb_scatter(z, i, nb1, stride, c4[i]);
  __syncthreads();
  const int t = threadIdx.x;
  const bool live = t < 4 * rows;
  float d = 0.f, mx = 0.f, sum = 1.f;
  float* zs = z + t * stride;
  if (live) d = rb_expect(zs, a.project, nb1, mx, sum);
  const int q = t & 60;
  const float d0 = __shfl(d, q, 64), d1 = __shfl(d, q + 1, 64), d2 = __shfl(d, q + 2, 64), d3 = __shfl(d, q + 3, 64);
  if (live) {
    const long row = row0 + (t >> 2);
    const float4 pt = ((const float4*)a.points)[row];
    const float4 go = ((const float4*)a.gboxes)[row];
    const float rs = a.rs;
    // (x0 + x1) / 2, x1 - x0
    const float gx0 = go.x * 0.5f - go.z, gx1 = go.x * 0.5f + go.z;
    const float gy0 = go.y * 0.5f - go.w, gy1 = go.y * 0.5f + go.w;
    const int s = t & 3;
    const float gd = s == 0 ? -gx0 * (pt.z / rs) : (s == 1 ? -gy0 * (pt.w / rs) : (s == 2 ? gx1 * (pt.z / rs) : gy1 * (pt.w / rs)));
    if (a.gpoints)
      a.gpoints[row * 4 + s] = s == 0 ? gx0 + gx1 : (s == 1 ? gy0 + gy1 : (s == 2 ? (gx1 * (0.5f * rs + d2) - gx0 * (0.5f * rs + d0)) / rs
                                                                                  : (gy1 * (0.5f * rs + d3) - gy0 * (0.5f * rs + d1)) / rs));
    for (int k = 0; k < nb1; ++k) zs[k] = expf(zs[k] - mx) / sum * (a.project[k] - d) * gd;
  }
  __syncthreads();
  const float4* gp4 = a.gpred ? (const float4*)(a.gpred + row0 * 4 * nb1) : nullptr;
  float4* o4 = (float4*)(a.gcorners + row0 * 4 * nb1);
  for (int i = threadIdx.x; i < n4; i += RB_THREADS) {
    float4 v = rb_gather(z, i, nb1, stride);
    if (gp4) {
      const float4 g = gp4[i];
      v.x = g.x + v.x; v.y = g.y + v.y; v.z = g.z + v.z; v.w = g.w + v.w;
    }
    o4[i] = v;
  }
}

size_t rb_lds_bytes(int nb1) { return (size_t)RB_THREADS * (nb1 | 1) * sizeof(float); }   // 33 280 bytes at nb1 = 64

}  // namespace

int launch_dfine_query_pos_forward(const float* ref, const float* w, const float* b, long N, int H, float* out, hipStream_t s) {
  const int H4 = H / 4;
  const long threads = (N + QP_ROWS - 1) / QP_ROWS * H4;
  hipLaunchKernelGGL(qp_fwd_kernel, dim3((unsigned)((threads + QP_THREADS - 1) / QP_THREADS)), dim3(QP_THREADS), 0, s, ref, w, b, out, N, H4);
  return (int)hipGetLastError();
}

size_t dfine_query_pos_workspace_bytes(long N, int H) {
  if (N < 1 || H < 1) return 0;
  return (size_t)qp_slabs(N) * 5 * H * sizeof(float);
}

int launch_dfine_query_pos_backward(const float* gout, const float* out, const float* ref, const float* w, long N, int H, float* dref,
                                    float* dweight, float* dbias, float* work, hipStream_t s) {
  QpBwdArgs a{};
  a.g = gout; a.out = out; a.ref = ref; a.w = w; a.dref = dref; a.part = (dweight || dbias) ? work : nullptr;
  a.N = N; a.H = H; a.H4 = H / 4;
  const int slabs = qp_slabs(N);
  a.slab_rows = (int)((N + slabs - 1) / slabs);
  hipLaunchKernelGGL(qp_bwd_kernel, dim3(slabs), dim3(QP_THREADS), 0, s, a);
  if (a.part)
    hipLaunchKernelGGL(qp_reduce_kernel, dim3((5 * H + QP_REDUCE_THREADS - 1) / QP_REDUCE_THREADS), dim3(QP_REDUCE_THREADS), 0, s, work,
                       slabs, H, dweight, dbias);
  return (int)hipGetLastError();
}

int launch_dfine_refine_reference_forward(const float* delta, const float* ref, long n, float eps, float* out, hipStream_t s) {
  hipLaunchKernelGGL(rr_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, delta, ref, out, n, eps);
  return (int)hipGetLastError();
}

int launch_dfine_refine_reference_backward(const float* gout, const float* out, long n, float* gdelta, hipStream_t s) {
  hipLaunchKernelGGL(rr_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gout, out, gdelta, n);
  return (int)hipGetLastError();
}

int launch_dfine_refine_boxes_forward(const float* delta, const float* prev, const float* project, const float* points, long N, int nb1,
                                      float reg_scale, float* pred, float* boxes, hipStream_t s) {
  RbArgs a{};
  a.corners = delta; a.prev = prev; a.project = project; a.points = points; a.pred = pred; a.boxes = boxes;
  a.N = N; a.nb1 = nb1; a.rs = fabsf(reg_scale);
  hipLaunchKernelGGL(rb_fwd_kernel, dim3((unsigned)((N + RB_ROWS - 1) / RB_ROWS)), dim3(RB_THREADS), rb_lds_bytes(nb1), s, a);
  return (int)hipGetLastError();
}

int launch_dfine_refine_boxes_backward(const float* gpred, const float* gboxes, const float* pred, const float* project,
                                       const float* points, long N, int nb1, float reg_scale, float* gcorners, float* gpoints,
                                       hipStream_t s) {
  RbArgs a{};
  a.corners = pred; a.project = project; a.points = points; a.gpred = gpred; a.gboxes = gboxes; a.gcorners = gcorners; a.gpoints = gpoints;
  a.N = N; a.nb1 = nb1; a.rs = fabsf(reg_scale);
  hipLaunchKernelGGL(rb_bwd_kernel, dim3((unsigned)((N + RB_ROWS - 1) / RB_ROWS)), dim3(RB_THREADS), rb_lds_bytes(nb1), s, a);
  return (int)hipGetLastError();
}

}  // namespace m355
