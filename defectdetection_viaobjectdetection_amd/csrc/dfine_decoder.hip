// A D-FINE decoder layer (transformers' DFineDecoderLayer) and its quality head (DFineLQE) between their GEMMs:
//   gate_ln_fwd / gate_ln_bwd   LayerNorm(sigmoid(g[:, :D]) x1 + sigmoid(g[:, D:]) x2), g the output of DFineGate's nn.Linear
//   lqe_fwd / lqe_bwd           per box side: softmax over the bins + 1 logits, the k largest probabilities, their mean
// (the third op, LayerNorm(clamp(x + y)), is the CLAMP instance of the add-LayerNorm kernels in dfine_encoder.hip.)
// fp32 in, fp32 out, fp32 accumulation; no float atomics: every sum has one owner and a fixed order, so results and gradients
// are bitwise reproducible.  Every kernel is row-wise: a row's result does not depend on the batch around it, no workgroup
// waits on another, no barrier except the one before a block writes its partial column sums.
//
// gate_ln has the mapping of the add-LayerNorm: one wave per row, a lane holds float4 number lane + 64 t of the row in
// registers (D <= 1024); the backward's blocks own contiguous row ranges and leave partial column sums of dweight | dbias that
// launch_dfine_addln_reduce adds in block order.  The forward keeps mean and rstd per row and nothing else; the backward forms
// the sigmoids and the normalised row again from g, x1, x2 with the forward's expressions (the same bits).
// lqe: one wave per (row, side), lane i holds bin i (bins + 1 <= 64).  The k rounds of the selection are wave-wide arg-max
// butterflies over (probability, bin) pairs that prefer the lower bin on an exact tie; every lane ends with the same pair.
#include <math.h>

#include "common.h"
#include "device_prims.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int GL_THREADS = 256;
constexpr int GL_WAVES = GL_THREADS / 64;
constexpr int GL_MAXV = 4;
constexpr int GL_MAX_D = 256 * GL_MAXV;

struct GateArgs {
  const float *g, *x1, *x2, *w, *b;   // g (M, 2 D); x1, x2 (M, D); w, b (D)
  float* out;                         // forward: (M, D)
  float *mean, *rstd;                 // (M): written by the forward, read by the backward
  const float* gout;                  // backward: (M, D)
  float *dg, *dx1, *dx2;              // backward: (M, 2 D), (M, D), (M, D); each may be nullptr
  float* part;                        // backward: (blocks, 2, D) partial column sums of dweight | dbias, or nullptr
  long M;
  int D;
  long rows_per_block;                // backward
  float eps;
};

__device__ __forceinline__ float wave_sum(float x) {   // a butterfly: the same bits in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

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

// float4 number v of row `row`: z = sigmoid(g1) x1 + sigmoid(g2) x2, and what the backward needs beside it
struct GateElem {
  float4 x1, x2, s1, s2, d1, d2;
};
__device__ __forceinline__ float4 gate_load_z(const GateArgs& a, long row, int v, GateElem& e) {
  const long o = row * a.D + 4L * v, og = row * 2 * a.D + 4L * v;
  e.x1 = *(const float4*)(a.x1 + o);
  e.x2 = *(const float4*)(a.x2 + o);
  sigmoid4(*(const float4*)(a.g + og), e.s1, e.d1);
  sigmoid4(*(const float4*)(a.g + og + a.D), e.s2, e.d2);
  return make_float4(e.s1.x * e.x1.x + e.s2.x * e.x2.x, e.s1.y * e.x1.y + e.s2.y * e.x2.y, e.s1.z * e.x1.z + e.s2.z * e.x2.z,
                     e.s1.w * e.x1.w + e.s2.w * e.x2.w);
}

__global__ __launch_bounds__(GL_THREADS) void gate_ln_fwd_kernel(const GateArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nv = a.D >> 2;
  const long row = (long)blockIdx.x * GL_WAVES + wave;
  if (row >= a.M) return;   // no barrier in this kernel
  float4 z[GL_MAXV];
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < GL_MAXV; ++t) {
    const int v = lane + 64 * t;
    z[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (v < nv) {
      GateElem e;
      z[t] = gate_load_z(a, row, v, e);
      sum += (z[t].x + z[t].y) + (z[t].z + z[t].w);
    }
  }
  const float inv_d = 1.f / (float)a.D;
  const float mean = wave_sum(sum) * inv_d;
  float sq = 0.f;
#pragma unroll
  for (int t = 0; t < GL_MAXV; ++t) {
    if (lane + 64 * t < nv) {
      const float dx = z[t].x - mean, dy = z[t].y - mean, dz = z[t].z - mean, dw = z[t].w - mean;
      sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float rstd = 1.f / sqrtf(wave_sum(sq) * inv_d + a.eps);
#pragma unroll
  for (int t = 0; t < GL_MAXV; ++t) {
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
__global__ __launch_bounds__(GL_THREADS) void gate_ln_bwd_kernel(const GateArgs a) {
  __shared__ float part[GL_WAVES][2][GL_MAX_D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nv = a.D >> 2;
  const long r0 = (long)blockIdx.x * a.rows_per_block;
  const long r1 = r0 + a.rows_per_block < a.M ? r0 + a.rows_per_block : a.M;
  const float inv_d = 1.f / (float)a.D;
  float4 dw[GL_MAXV], db[GL_MAXV], w[GL_MAXV];
#pragma unroll
  for (int t = 0; t < GL_MAXV; ++t) {
    dw[t] = db[t] = w[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane + 64 * t < nv) w[t] = *(const float4*)(a.w + 4 * (lane + 64 * t));
  }
  for (long row = r0 + wave; row < r1; row += GL_WAVES) {
    const float mean = a.mean[row], rstd = a.rstd[row];
    float4 zh[GL_MAXV], gw[GL_MAXV];
    GateElem e[GL_MAXV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < GL_MAXV; ++t) {
      const int v = lane + 64 * t;
      zh[t] = gw[t] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (v < nv) {
        const float4 z = gate_load_z(a, row, v, e[t]);
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
    if (!a.dg && !a.dx1 && !a.dx2) continue;   // wave-uniform: only the column sums were asked for
    const float c1 = wave_sum(s1) * inv_d, c2 = wave_sum(s2) * inv_d;
#pragma unroll
    for (int t = 0; t < GL_MAXV; ++t) {
      const int v = lane + 64 * t;
      if (v < nv) {
        const float4 dz = make_float4(rstd * (gw[t].x - c1 - zh[t].x * c2), rstd * (gw[t].y - c1 - zh[t].y * c2),
                                      rstd * (gw[t].z - c1 - zh[t].z * c2), rstd * (gw[t].w - c1 - zh[t].w * c2));
        const GateElem& q = e[t];
        if (a.dx1) *(float4*)(a.dx1 + row * a.D + 4L * v) = make_float4(dz.x * q.s1.x, dz.y * q.s1.y, dz.z * q.s1.z, dz.w * q.s1.w);
        if (a.dx2) *(float4*)(a.dx2 + row * a.D + 4L * v) = make_float4(dz.x * q.s2.x, dz.y * q.s2.y, dz.z * q.s2.z, dz.w * q.s2.w);
        if (a.dg) {
          float* p = a.dg + row * 2 * a.D + 4L * v;
          *(float4*)p = make_float4(dz.x * q.x1.x * q.d1.x, dz.y * q.x1.y * q.d1.y, dz.z * q.x1.z * q.d1.z, dz.w * q.x1.w * q.d1.w);
          *(float4*)(p + a.D) = make_float4(dz.x * q.x2.x * q.d2.x, dz.y * q.x2.y * q.d2.y, dz.z * q.x2.z * q.d2.z, dz.w * q.x2.w * q.d2.w);
        }
      }
    }
  }
  if (!a.part) return;   // uniform over the grid: neither dweight nor dbias was asked for
#pragma unroll
  for (int t = 0; t < GL_MAXV; ++t) {
    const int v = lane + 64 * t;
    if (v < nv) {
      *(float4*)&part[wave][0][4 * v] = dw[t];
      *(float4*)&part[wave][1][4 * v] = db[t];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * a.D; c += GL_THREADS) {
    const int which = c >= a.D, col = c - which * a.D;
    float s = part[0][which][col];
#pragma unroll
    for (int wv = 1; wv < GL_WAVES; ++wv) s += part[wv][which][col];
    a.part[(long)blockIdx.x * 2 * a.D + c] = s;
  }
}

// ---- LQE statistics --------------------------------------------------------------------------------------------------------
constexpr int LQ_THREADS = 256;   // four waves: the four sides of one row

struct LqeArgs {
  const float* corners;       // (M, 4 nb1)
  float* stat;                // forward: (M, 4 (k + 1)): per side the k probabilities in descending order, then their mean
  unsigned char* idx;         // forward: (M, 4, k) chosen bins, or nullptr; the backward reads it
  const float* gstat;         // backward: (M, 4 (k + 1))
  float* gcorners;            // backward: (M, 4 nb1)
  long M;
  int nb1, k;
};

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
  return x;
}

// softmax over the nb1 logits of (row, side), bin `lane` in lane `lane`; 0 in the lanes past nb1.  Forward and backward call
// this one function: the backward's probabilities have the forward's bits.
__device__ __forceinline__ float lqe_prob(const float* corners, long rs, int nb1, int lane) {
  const bool live = lane < nb1;
  const float x = live ? corners[rs * nb1 + lane] : -INFINITY;
  const float mx = wave_max(x);
  const float e = live ? expf(x - mx) : 0.f;
  return e / wave_sum(e);
}

__global__ __launch_bounds__(LQ_THREADS) void lqe_fwd_kernel(const LqeArgs a) {
  const int lane = threadIdx.x & 63;
  const long rs = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // (row, side); the grid is exactly M blocks
  const float p = lqe_prob(a.corners, rs, a.nb1, lane);
  float v = lane < a.nb1 ? p : -1.f;                           // -1: not a candidate (past the bins, or already taken)
  float sum = 0.f, mine = 0.f;
  int mine_i = 0;
  for (int j = 0; j < a.k; ++j) {                              // k <= nb1: a live candidate is left in every round
    float bv = v;
    int bi = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == bi) v = -1.f;
    sum += bv;
    if (lane == j) { mine = bv; mine_i = bi; }
  }
  float* st = a.stat + rs * (a.k + 1);
  if (lane < a.k) {
    st[lane] = mine;
    if (a.idx) a.idx[rs * a.k + lane] = (unsigned char)mine_i;
  }
  if (lane == a.k) st[a.k] = sum / (float)a.k;
}

// d logits = p * (dp - sum(dp * p)), dp_i = sum over the chosen slots j with bin i of (gstat_j + gstat_mean / k)
__global__ __launch_bounds__(LQ_THREADS) void lqe_bwd_kernel(const LqeArgs a) {
  const int lane = threadIdx.x & 63;
  const long rs = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const float p = lqe_prob(a.corners, rs, a.nb1, lane);
  const float* gs = a.gstat + rs * (a.k + 1);
  const float gm = gs[a.k] / (float)a.k;
  float dp = 0.f;
  for (int j = 0; j < a.k; ++j)
    if ((int)a.idx[rs * a.k + j] == lane) dp += gs[j] + gm;    // the k bins of a side are distinct: at most one term per lane
  const float dot = wave_sum(dp * p);
  if (lane < a.nb1) a.gcorners[rs * a.nb1 + lane] = p * (dp - dot);
}

}  // namespace

int launch_dfine_gate_ln_forward(const float* g, const float* x1, const float* x2, const float* w, const float* b, long M, int D,
                                 float eps, float* out, float* mean, float* rstd, hipStream_t s) {
  GateArgs a{};
  a.g = g; a.x1 = x1; a.x2 = x2; a.w = w; a.b = b; a.out = out; a.mean = mean; a.rstd = rstd; a.M = M; a.D = D; a.eps = eps;
  hipLaunchKernelGGL(gate_ln_fwd_kernel, dim3((unsigned)((M + GL_WAVES - 1) / GL_WAVES)), dim3(GL_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_gate_ln_backward(const float* gout, const float* g, const float* x1, const float* x2, const float* w, const float* mean,
                                  const float* rstd, long M, int D, float* dg, float* dx1, float* dx2, float* dweight, float* dbias,
                                  float* work, hipStream_t s) {
  GateArgs a{};
  a.gout = gout; a.g = g; a.x1 = x1; a.x2 = x2; a.w = w; a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd);
  a.dg = dg; a.dx1 = dx1; a.dx2 = dx2; a.part = dweight || dbias ? work : nullptr;
  a.M = M; a.D = D; a.rows_per_block = dfine_addln_rows_per_block(M);
  const int blocks = (int)((M + a.rows_per_block - 1) / a.rows_per_block);
  hipLaunchKernelGGL(gate_ln_bwd_kernel, dim3(blocks), dim3(GL_THREADS), 0, s, a);
  const int rc = (int)hipGetLastError();
  if (rc != 0 || !a.part) return rc;
  return launch_dfine_addln_reduce(work, blocks, D, dweight, dbias, s);
}

int launch_dfine_lqe_forward(const float* corners, long M, int nb1, int k, float* stat, unsigned char* idx, hipStream_t s) {
  LqeArgs a{};
  a.corners = corners; a.stat = stat; a.idx = idx; a.M = M; a.nb1 = nb1; a.k = k;
  hipLaunchKernelGGL(lqe_fwd_kernel, dim3((unsigned)M), dim3(LQ_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_lqe_backward(const float* gstat, const float* corners, const unsigned char* idx, long M, int nb1, int k,
                              float* gcorners, hipStream_t s) {
  LqeArgs a{};
  a.corners = corners; a.gstat = gstat; a.idx = const_cast<unsigned char*>(idx); a.gcorners = gcorners; a.M = M; a.nb1 = nb1; a.k = k;
  hipLaunchKernelGGL(lqe_bwd_kernel, dim3((unsigned)M), dim3(LQ_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace m355
