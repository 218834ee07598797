// The row LayerNorms of the D-FINE layers: LayerNorm(z) over the last axis of an (M, D) tensor whose rows z come from a "row source":
//   AddSrc<DROP, false>   z = x + dropout(y)                                  the encoder layers (nn.TransformerEncoderLayer, post-norm)
//   AddSrc<false, true>   z = clamp(x + y, lo, hi)                            the decoder layer's LayerNorm after its FFN
//   GateSrc               z = sigmoid(g[:, :D]) x1 + sigmoid(g[:, D:]) x2     DFineGate, g (M, 2 D) the output of its nn.Linear
// One forward and one backward kernel template serve all of them: the statistics, the normalised row, the dz expression, the
// column sums of dweight | dbias and their order are written once.  A source supplies what differs:
//   Elem                             what the backward keeps per float4 between forming z and scattering dz
//   load(row, D, v, Elem&) -> z      float4 number v of row `row`
//   scatter(row, D, v, dz, Elem)     dz to the gradients of the source's inputs that were asked for
//   wants_rows()                     false: no per-row gradient was asked for, the backward only needs the column sums
// fp32 in, fp32 out, fp32 accumulation; no float atomics: every sum has one owner and a fixed order, so results and gradients
// are bitwise reproducible and a row does not depend on the batch around it.  Every dropout mask comes from dropout_keep4
// (device_prims.h) and is recomputed in the backward; none is stored.
//
// One wave per row; a lane holds float4 number lane + 64 t of the row, t < LN_MAXV (D <= 1024), in registers.  The forward keeps
// mean and rstd per row and nothing else; the backward forms z again from the source's inputs with the forward's expressions
// (the same bits).  The backward's blocks own contiguous row ranges and leave partial column sums of dweight | dbias that
// rowln_reduce_kernel adds in block order.
#include <math.h>

#include "common.h"
#include "device_prims.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_WAVES = LN_THREADS / 64;
constexpr int LN_MAXV = 4;
constexpr int LN_MAX_D = 256 * LN_MAXV;
constexpr int LN_MAX_BLOCKS = 256;   // partial rows of the backward's column sums

// what every form has beside its source
struct RowArgs {
  const float *w, *b;    // (D)
  float* out;            // forward: (M, D)
  float *mean, *rstd;    // (M): written by the forward, read by the backward
  const float* gout;     // backward: (M, D)
  float* part;           // backward: (blocks, 2, D) partial column sums of dweight | dbias, or nullptr
  long M;
  int D;
  long rows_per_block;   // backward
  float eps;
};

// torch.clamp of one element, NaN kept; `inside` = lo <= z <= hi, the elements that torch's clamp backward lets through
__device__ __forceinline__ float clamp1(float z, float lo, float hi, bool& inside) {
  inside = z >= lo && z <= hi;
  return z < lo ? lo : (z > hi ? hi : z);
}
// bit c of the result: component c of z was inside [lo, hi]
__device__ __forceinline__ unsigned ln_clamp4(float4& z, float lo, float hi) {
  bool ix, iy, iz, iw;
  z = make_float4(clamp1(z.x, lo, hi, ix), clamp1(z.y, lo, hi, iy), clamp1(z.z, lo, hi, iz), clamp1(z.w, lo, hi, iw));
  return (unsigned)ix | (unsigned)iy << 1 | (unsigned)iz << 2 | (unsigned)iw << 3;
}

// z = x + dropout(y), or z = clamp(x + y, lo, hi); x, y (M, D); dx, dy (M, D), either may be nullptr
template <bool DROP, bool CLAMP>
struct AddSrc {
  const float *x, *y;
  float *dx, *dy;
  float lo, hi;
  DropArgs d;
  struct Elem {
    unsigned keep, inside;   // bit c: component c was kept by the dropout / not moved by the clamp
  };
  __device__ __forceinline__ bool wants_rows() const { return true; }
  __device__ __forceinline__ float4 load(long row, int D, int v, Elem& q) const {
    const long e = row * D + 4L * v;
    const float4 xv = *(const float4*)(x + e);
    float4 yv = *(const float4*)(y + e);
    q.keep = 0xfu;
    if (DROP) {
      q.keep = dropout_keep4(d, (unsigned long long)e >> 2);
      yv.x = q.keep & 1u ? yv.x * d.scale : 0.f; yv.y = q.keep & 2u ? yv.y * d.scale : 0.f;
      yv.z = q.keep & 4u ? yv.z * d.scale : 0.f; yv.w = q.keep & 8u ? yv.w * d.scale : 0.f;
    }
    float4 z = make_float4(xv.x + yv.x, xv.y + yv.y, xv.z + yv.z, xv.w + yv.w);
    q.inside = 0xfu;
    if (CLAMP) q.inside = ln_clamp4(z, lo, hi);
    return z;
  }
  __device__ __forceinline__ void scatter(long row, int D, int v, float4 dz, const Elem& q) const {
    if (CLAMP) {   // no gradient through an element that the clamp moved
      dz.x = q.inside & 1u ? dz.x : 0.f; dz.y = q.inside & 2u ? dz.y : 0.f;
      dz.z = q.inside & 4u ? dz.z : 0.f; dz.w = q.inside & 8u ? dz.w : 0.f;
    }
    if (dx) *(float4*)(dx + row * D + 4L * v) = dz;
    if (dy) {
      float4 dyv = dz;
      if (DROP) {
        dyv.x = q.keep & 1u ? dz.x * d.scale : 0.f; dyv.y = q.keep & 2u ? dz.y * d.scale : 0.f;
        dyv.z = q.keep & 4u ? dz.z * d.scale : 0.f; dyv.w = q.keep & 8u ? dz.w * d.scale : 0.f;
      }
      *(float4*)(dy + row * D + 4L * v) = dyv;
    }
  }
};

// s = sigmoid(g) and ds = s (1 - s) from e = exp(-|g|), r = 1 / (1 + e): s = r or e r, ds = e r r.  No cancellation at either
// end: a saturated gate keeps a relative-accuracy derivative instead of 1 - s rounding to 0.
__device__ __forceinline__ void sigmoid1(float g, float& s, float& ds) {
  const float e = expf(-fabsf(g)), r = 1.f / (1.f + e), er = e * r;
  s = g >= 0.f ? r : er;
  ds = er * r;
}
__device__ __forceinline__ void sigmoid4(const float4 g, float4& s, float4& ds) {
  sigmoid1(g.x, s.x, ds.x); sigmoid1(g.y, s.y, ds.y); sigmoid1(g.z, s.z, ds.z); sigmoid1(g.w, s.w, ds.w);
}

// z = sigmoid(g1) x1 + sigmoid(g2) x2; g (M, 2 D) = g1 | g2; x1, x2 (M, D); dg (M, 2 D), dx1, dx2 (M, D), each may be nullptr
struct GateSrc {
  const float *g, *x1, *x2;
  float *dg, *dx1, *dx2;
  struct Elem {
    float4 x1, x2, s1, s2, d1, d2;
  };
  __device__ __forceinline__ bool wants_rows() const { return dg || dx1 || dx2; }
  __device__ __forceinline__ float4 load(long row, int D, int v, Elem& e) const {
    const long o = row * D + 4L * v, og = row * 2 * D + 4L * v;
    e.x1 = *(const float4*)(x1 + o);
    e.x2 = *(const float4*)(x2 + o);
    sigmoid4(*(const float4*)(g + og), e.s1, e.d1);
    sigmoid4(*(const float4*)(g + og + D), e.s2, e.d2);
    return make_float4(e.s1.x * e.x1.x + e.s2.x * e.x2.x, e.s1.y * e.x1.y + e.s2.y * e.x2.y, e.s1.z * e.x1.z + e.s2.z * e.x2.z,
                       e.s1.w * e.x1.w + e.s2.w * e.x2.w);
  }
  __device__ __forceinline__ void scatter(long row, int D, int v, const float4 dz, const Elem& q) const {
    if (dx1) *(float4*)(dx1 + row * D + 4L * v) = make_float4(dz.x * q.s1.x, dz.y * q.s1.y, dz.z * q.s1.z, dz.w * q.s1.w);
    if (dx2) *(float4*)(dx2 + row * D + 4L * v) = make_float4(dz.x * q.s2.x, dz.y * q.s2.y, dz.z * q.s2.z, dz.w * q.s2.w);
    if (dg) {
      float* p = dg + row * 2 * D + 4L * v;
      *(float4*)p = make_float4(dz.x * q.x1.x * q.d1.x, dz.y * q.x1.y * q.d1.y, dz.z * q.x1.z * q.d1.z, dz.w * q.x1.w * q.d1.w);
      *(float4*)(p + D) = make_float4(dz.x * q.x2.x * q.d2.x, dz.y * q.x2.y * q.d2.y, dz.z * q.x2.z * q.d2.z, dz.w * q.x2.w * q.d2.w);
    }
  }
};

template <class Src>
__global__ __launch_bounds__(LN_THREADS) void rowln_fwd_kernel(const RowArgs a, const Src src) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nv = a.D >> 2;
  const long row = (long)blockIdx.x * LN_WAVES + wave;
  if (row >= a.M) return;   // no barrier in this kernel
  float4 z[LN_MAXV];
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < LN_MAXV; ++t) {
    const int v = lane + 64 * t;
    z[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (v < nv) {
      typename Src::Elem e;
      z[t] = src.load(row, a.D, v, e);
      sum += (z[t].x + z[t].y) + (z[t].z + z[t].w);
    }
  }
  const float inv_d = 1.f / (float)a.D;
  const float mean = wave_sum(sum) * inv_d;
  float sq = 0.f;
#pragma unroll
  for (int t = 0; t < LN_MAXV; ++t) {
    if (lane + 64 * t < nv) {
      const float dx = z[t].x - mean, dy = z[t].y - mean, dz = z[t].z - mean, dw = z[t].w - mean;
      sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float rstd = 1.f / sqrtf(wave_sum(sq) * inv_d + a.eps);
#pragma unroll
  for (int t = 0; t < LN_MAXV; ++t) {
    const int v = lane + 64 * t;
    if (v < nv) {
      const float4 w = *(const float4*)(a.w + 4 * v), bb = *(const float4*)(a.b + 4 * v);
      *(float4*)(a.out + row * a.D + 4L * v) = make_float4((z[t].x - mean) * rstd * w.x + bb.x, (z[t].y - mean) * rstd * w.y + bb.y,
                                                           (z[t].z - mean) * rstd * w.z + bb.z, (z[t].w - mean) * rstd * w.w + bb.w);
    }
  }
  if (lane == 0) { a.mean[row] = mean; a.rstd[row] = rstd; }
}

// Block `blk` owns rows [blk * rows_per_block, ...): wave w takes every fourth of them in ascending order and keeps its column
// sums of gout * zhat and gout in registers; the four waves' sums are added in wave order into partial row `blk`.
template <class Src>
__global__ __launch_bounds__(LN_THREADS) void rowln_bwd_kernel(const RowArgs a, const Src src) {
  __shared__ float part[LN_WAVES][2][LN_MAX_D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nv = a.D >> 2;
  const long r0 = (long)blockIdx.x * a.rows_per_block;
  const long r1 = r0 + a.rows_per_block < a.M ? r0 + a.rows_per_block : a.M;
  const float inv_d = 1.f / (float)a.D;
  float4 dw[LN_MAXV], db[LN_MAXV], w[LN_MAXV];
#pragma unroll
  for (int t = 0; t < LN_MAXV; ++t) {
    dw[t] = db[t] = w[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane + 64 * t < nv) w[t] = *(const float4*)(a.w + 4 * (lane + 64 * t));
  }
  for (long row = r0 + wave; row < r1; row += LN_WAVES) {
    const float mean = a.mean[row], rstd = a.rstd[row];
    float4 zh[LN_MAXV], gw[LN_MAXV];
    typename Src::Elem e[LN_MAXV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < LN_MAXV; ++t) {
      const int v = lane + 64 * t;
      zh[t] = gw[t] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (v < nv) {
        const float4 z = src.load(row, a.D, v, e[t]);
        const float4 g = *(const float4*)(a.gout + row * a.D + 4L * v);
        zh[t] = make_float4((z.x - mean) * rstd, (z.y - mean) * rstd, (z.z - mean) * rstd, (z.w - mean) * rstd);
        gw[t] = make_float4(g.x * w[t].x, g.y * w[t].y, g.z * w[t].z, g.w * w[t].w);
        s1 += (gw[t].x + gw[t].y) + (gw[t].z + gw[t].w);
        s2 += (gw[t].x * zh[t].x + gw[t].y * zh[t].y) + (gw[t].z * zh[t].z + gw[t].w * zh[t].w);
        dw[t].x = fmaf(g.x, zh[t].x, dw[t].x); dw[t].y = fmaf(g.y, zh[t].y, dw[t].y);
        dw[t].z = fmaf(g.z, zh[t].z, dw[t].z); dw[t].w = fmaf(g.w, zh[t].w, dw[t].w);
        db[t].x += g.x; db[t].y += g.y; db[t].z += g.z; db[t].w += g.w;
      }
    }
    if (!src.wants_rows()) continue;   // wave-uniform: only the column sums were asked for
    const float c1 = wave_sum(s1) * inv_d, c2 = wave_sum(s2) * inv_d;
#pragma unroll
    for (int t = 0; t < LN_MAXV; ++t) {
      const int v = lane + 64 * t;
      if (v < nv) {
        const float4 dz = make_float4(rstd * (gw[t].x - c1 - zh[t].x * c2), rstd * (gw[t].y - c1 - zh[t].y * c2),
                                      rstd * (gw[t].z - c1 - zh[t].z * c2), rstd * (gw[t].w - c1 - zh[t].w * c2));
        src.scatter(row, a.D, v, dz, e[t]);
      }
    }
  }
  if (!a.part) return;   // uniform over the grid: neither dweight nor dbias was asked for (the gate; the add forms always pass it)
#pragma unroll
  for (int t = 0; t < LN_MAXV; ++t) {
    const int v = lane + 64 * t;
    if (v < nv) {
      *(float4*)&part[wave][0][4 * v] = dw[t];
      *(float4*)&part[wave][1][4 * v] = db[t];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * a.D; c += LN_THREADS) {
    const int which = c >= a.D, col = c - which * a.D;
    float s = part[0][which][col];
#pragma unroll
    for (int wv = 1; wv < LN_WAVES; ++wv) s += part[wv][which][col];
    a.part[(long)blockIdx.x * 2 * a.D + c] = s;
  }
}

// dweight | dbias [c] = the partial rows added in block order
__global__ __launch_bounds__(256) void rowln_reduce_kernel(const float* part, int nblocks, int D, float* dweight, float* dbias) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * D) return;
  float s = 0.f;
  for (int k = 0; k < nblocks; ++k) s += part[(long)k * 2 * D + c];
  if (c < D) { if (dweight) dweight[c] = s; }
  else if (dbias) dbias[c - D] = s;
}

long rows_per_block(long M) {
  long blocks = (M + LN_WAVES - 1) / LN_WAVES;
  if (blocks > LN_MAX_BLOCKS) blocks = LN_MAX_BLOCKS;
  const long rpb = (M + blocks - 1) / blocks;
  return (rpb + LN_WAVES - 1) / LN_WAVES * LN_WAVES;
}

template <class Src>
int launch_fwd(const Src& src, const float* w, const float* b, long M, int D, float eps, float* out, float* mean, float* rstd,
               hipStream_t s) {
  RowArgs a{};
  a.w = w; a.b = b; a.out = out; a.mean = mean; a.rstd = rstd; a.M = M; a.D = D; a.eps = eps;
  hipLaunchKernelGGL(rowln_fwd_kernel<Src>, dim3((unsigned)((M + LN_WAVES - 1) / LN_WAVES)), dim3(LN_THREADS), 0, s, a, src);
  return (int)hipGetLastError();
}

// part: where the blocks leave their partial rows, or nullptr when neither dweight nor dbias is asked for and the form allows
// skipping them; the partial rows are added up only when dweight or dbias is asked for
template <class Src>
int launch_bwd(const Src& src, const float* gout, const float* w, const float* mean, const float* rstd, long M, int D, float* part,
               float* dweight, float* dbias, hipStream_t s) {
  RowArgs a{};
  a.gout = gout; a.w = w; a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.part = part;
  a.M = M; a.D = D; a.rows_per_block = rows_per_block(M);
  const int blocks = (int)((M + a.rows_per_block - 1) / a.rows_per_block);
  hipLaunchKernelGGL(rowln_bwd_kernel<Src>, dim3(blocks), dim3(LN_THREADS), 0, s, a, src);
  const int rc = (int)hipGetLastError();
  if (rc != 0 || (!dweight && !dbias)) return rc;
  hipLaunchKernelGGL(rowln_reduce_kernel, dim3((2 * D + 255) / 256), dim3(256), 0, s, part, blocks, D, dweight, dbias);
  return (int)hipGetLastError();
}

}  // namespace

int dfine_addln_max_d() { return LN_MAX_D; }

size_t dfine_addln_workspace_bytes(long M, int D) {
  if (M < 1 || D < 1) return 0;
  const long rpb = rows_per_block(M);
  return (size_t)((M + rpb - 1) / rpb) * 2 * (size_t)D * sizeof(float);
}

int launch_dfine_addln_forward(const float* x, const float* y, const float* w, const float* b, long M, int D, float eps, float p,
                               unsigned long long seed, int site, float* out, float* mean, float* rstd, hipStream_t s) {
  const DropArgs d = drop_args(p, seed, site);
  if (p > 0.f) return launch_fwd(AddSrc<true, false>{x, y, nullptr, nullptr, 0.f, 0.f, d}, w, b, M, D, eps, out, mean, rstd, s);
  return launch_fwd(AddSrc<false, false>{x, y, nullptr, nullptr, 0.f, 0.f, d}, w, b, M, D, eps, out, mean, rstd, s);
}

int launch_dfine_addln_backward(const float* g, const float* x, const float* y, const float* w, const float* mean, const float* rstd,
                                long M, int D, float p, unsigned long long seed, int site, float* dx, float* dy, float* dweight,
                                float* dbias, float* work, hipStream_t s) {
  const DropArgs d = drop_args(p, seed, site);
  if (p > 0.f) return launch_bwd(AddSrc<true, false>{x, y, dx, dy, 0.f, 0.f, d}, g, w, mean, rstd, M, D, work, dweight, dbias, s);
  return launch_bwd(AddSrc<false, false>{x, y, dx, dy, 0.f, 0.f, d}, g, w, mean, rstd, M, D, work, dweight, dbias, s);
}

int launch_dfine_addln_clamp_forward(const float* x, const float* y, const float* w, const float* b, long M, int D, float eps, float lo,
                                     float hi, float* out, float* mean, float* rstd, hipStream_t s) {
  return launch_fwd(AddSrc<false, true>{x, y, nullptr, nullptr, lo, hi, DropArgs{}}, w, b, M, D, eps, out, mean, rstd, s);
}

int launch_dfine_addln_clamp_backward(const float* g, const float* x, const float* y, const float* w, const float* mean,
                                      const float* rstd, long M, int D, float lo, float hi, float* dx, float* dy, float* dweight,
                                      float* dbias, float* work, hipStream_t s) {
  return launch_bwd(AddSrc<false, true>{x, y, dx, dy, lo, hi, DropArgs{}}, g, w, mean, rstd, M, D, work, dweight, dbias, s);
}

int launch_dfine_gate_ln_forward(const float* g, const float* x1, const float* x2, const float* w, const float* b, long M, int D,
                                 float eps, float* out, float* mean, float* rstd, hipStream_t s) {
  return launch_fwd(GateSrc{g, x1, x2, nullptr, nullptr, nullptr}, w, b, M, D, eps, out, mean, rstd, s);
}

int launch_dfine_gate_ln_backward(const float* gout, const float* g, const float* x1, const float* x2, const float* w, const float* mean,
                                  const float* rstd, long M, int D, float* dg, float* dx1, float* dx2, float* dweight, float* dbias,
                                  float* work, hipStream_t s) {
  return launch_bwd(GateSrc{g, x1, x2, dg, dx1, dx2}, gout, w, mean, rstd, M, D, dweight || dbias ? work : nullptr, dweight, dbias, s);
}

}  // namespace m355
