// The temporal encoder of the D-FINE trainers (nn.TransformerEncoderLayer, post-norm, ReLU, head dim 32) between its GEMMs:
//   attn_fwd / attn_bwd          softmax(q k^T / sqrt(32)) [dropout] v on the packed in-projection output (B, S, 3 D)
//   addln_fwd / addln_bwd        LayerNorm(x + dropout(y)), with the fixed-order column sums of dweight / dbias; their CLAMP
//                                instances are LayerNorm(clamp(x + y, lo, hi)) of the D-FINE decoder layer (dfine_decoder.hip)
//   relu_drop_fwd / relu_drop_bwd  dropout(relu(h))
// All fp32 in, fp32 out, fp32 accumulation.  No float atomics anywhere: every sum has one owner and a fixed order, so the
// results are bitwise reproducible and frame b does not depend on the batch.
// Every dropout mask comes from dropout_keep4 (device_prims.h) and is recomputed in the backward; none is stored.
//
// Attention forward: one wave per 32 queries of a (frame, head), both products on the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32), operands straight from memory, no LDS (see attn_fwd_kernel).
// Attention backward, on VALU FMA chains: a block of 256 threads owns 64 rows (queries in the dQ role, keys in the dKV role)
// of one (frame, head); FOUR lanes share a row.  The other axis streams through LDS in tiles of 64 rows x 32 floats (K and V,
// or Q and dO); of each tile the four lanes of a row take 16 consecutive rows each and keep partial sums, merged by two quad
// butterflies at the end, whose order does not depend on the lane.  The row's 32-float vectors (q, dO, dq / k, v, dk, dv) live
// in registers.  The S x S scores exist only in registers, in either direction.
#include <math.h>

#include "common.h"
#include "device_prims.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int AT_THREADS = 256;
constexpr int AT_ROWS = 64;      // rows a block owns = rows of a streamed tile
constexpr int AT_PER_LANE = 16;  // streamed rows per lane and tile (4 lanes per owned row)
constexpr float AT_SCALE = 0.17677669529663687f;             // 1 / sqrt(32)
constexpr float AT_SCALE_LOG2E = 0.25503486237899584f;       // log2(e) / sqrt(32): the logits are kept in base 2

struct AttnArgs {
  const float* qkv;    // (B, S, 3 D): q | k | v, head h at columns h * 32 of each
  float* out;          // forward: (B, S, D)
  float* lse;          // forward: (B, H, S, 2) or nullptr (nothing saved): the row's log-sum-exp of the base-2 logits as the pair
                       // (running maximum m, log2 of the sum of exp2(s - m)), not added up: s - m is (nearly) exact for the keys
                       // that matter, so the backward's exp2((s - m) - log2 sum) is the forward's probability to an ulp or two
  const float* gout;   // backward: (B, S, D)
  const float* o;      // backward: the forward's output
  const float* lse_in; // backward
  float* gqkv;         // backward: (B, S, 3 D), every element written
  int S, H;
  DropArgs d;
};

// LDS image of a tile of 64 rows x 8 float4: the four lanes of a quad read rows r, r + 16, r + 32, r + 48 at the same
// column group g, which a plain 128-byte row pitch would put in the same banks; rotating the groups by 2 per 16 rows puts the
// four 16-byte reads in four different bank groups.
__device__ __forceinline__ int tile_slot(int r, int g) { return r * 8 + ((g + 2 * (r >> 4)) & 7); }

// rows [r0, r0 + 64) of the (S x 32) matrix at `base` (row pitch ld floats), times f, into `lds`; rows past S as zeros
__device__ __forceinline__ void stage_tile(float4* lds, const float* base, long ld, int r0, int S, int tid, float f = 1.f) {
#pragma unroll
  for (int e = tid; e < AT_ROWS * 8; e += AT_THREADS) {
    const int r = e >> 3, g = e & 7;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < S) v = *(const float4*)(base + (long)(r0 + r) * ld + 4 * g);
    lds[tile_slot(r, g)] = make_float4(v.x * f, v.y * f, v.z * f, v.w * f);
  }
}

__device__ __forceinline__ void load_row32(float (&x)[32], const float* p) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const float4 v = *(const float4*)(p + 4 * g);
    x[4 * g] = v.x; x[4 * g + 1] = v.y; x[4 * g + 2] = v.z; x[4 * g + 3] = v.w;
  }
}

__device__ __forceinline__ float dot_tile_row(const float (&x)[32], const float4* lds, int r) {
  float acc = 0.f;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const float4 v = lds[tile_slot(r, g)];
    acc = fmaf(x[4 * g], v.x, acc); acc = fmaf(x[4 * g + 1], v.y, acc);
    acc = fmaf(x[4 * g + 2], v.z, acc); acc = fmaf(x[4 * g + 3], v.w, acc);
  }
  return acc;
}

__device__ __forceinline__ void axpy_tile_row(float (&y)[32], float a, const float4* lds, int r) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const float4 v = lds[tile_slot(r, g)];
    y[4 * g] = fmaf(a, v.x, y[4 * g]); y[4 * g + 1] = fmaf(a, v.y, y[4 * g + 1]);
    y[4 * g + 2] = fmaf(a, v.z, y[4 * g + 2]); y[4 * g + 3] = fmaf(a, v.w, y[4 * g + 3]);
  }
}

// sum over the four lanes of a quad; (x0 + x1) + (x2 + x3) in every lane, whichever lane asks
__device__ __forceinline__ float quad_sum(float x) {
  x += __shfl_xor(x, 1, 64);
  x += __shfl_xor(x, 2, 64);
  return x;
}
__device__ __forceinline__ float quad_max(float x) {
  x = fmaxf(x, __shfl_xor(x, 1, 64));
  return fmaxf(x, __shfl_xor(x, 2, 64));
}

// the eight channels 8 sub .. 8 sub + 7 of a 32-vector, times f, as two 16-byte stores at p
__device__ __forceinline__ void store_slice8(float* p, const float (&x)[32], int sub, float f) {
  float w[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) w[t] = (sub == 0 ? x[t] : sub == 1 ? x[8 + t] : sub == 2 ? x[16 + t] : x[24 + t]) * f;
  *(float4*)(p + 8 * sub) = make_float4(w[0], w[1], w[2], w[3]);
  *(float4*)(p + 8 * sub + 4) = make_float4(w[4], w[5], w[6], w[7]);
}

// keep bits of the 16 consecutive elements that start at flat index f0: five Philox calls cover any alignment
__device__ __forceinline__ unsigned keep16(const DropArgs& d, unsigned long long f0) {
  const unsigned long long g0 = f0 >> 2;
  unsigned bits = 0u, hi = 0u;
#pragma unroll
  for (int t = 0; t < 4; ++t) bits |= dropout_keep4(d, g0 + t) << (4 * t);
  hi = dropout_keep4(d, g0 + 4);
  const unsigned sh = (unsigned)(f0 & 3ull);
  return ((bits >> sh) | (hi << (16 - sh))) & 0xffffu;
}

// ---- forward: one wave owns 32 queries, both products on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered FMA chain) --------
// S^T = K Q^T puts the queries on the lanes (column = lane & 31) and the 32 keys of a tile in the 16 accumulator registers of
// the two lane halves, so a query's softmax is 16 registers of one lane plus one exchange with the other half, and P^T in
// that layout IS the B operand of O^T = V^T P^T: no transpose, no LDS.  Row of accumulator register t in lane half h:
constexpr int MF_ROWS = 32;
__device__ __forceinline__ int acc_row(int t, int h) { return (t & 3) + 8 * (t >> 2) + 4 * h; }

// channels h, 2 + h, 4 + h, ... of a 32-float row: a lane's A (or B) operands of the sixteen k-steps of a product over channels
__device__ __forceinline__ void load_row_parity(float (&x)[16], const float* p, int h) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const float4 v = *(const float4*)(p + 4 * g);
    x[2 * g] = h ? v.y : v.x;
    x[2 * g + 1] = h ? v.w : v.z;
  }
}

template <bool DROP>
__global__ __launch_bounds__(64) void attn_fwd_kernel(const AttnArgs a) {
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const int S = a.S, H = a.H, D = 32 * H;
  const int b = blockIdx.z, h = blockIdx.y, i = blockIdx.x * MF_ROWS + r;
  const long ld = 3L * D;
  const float* base = a.qkv + (long)b * S * ld + 32 * h;
  const bool valid = i < S;
  const int ic = valid ? i : S - 1;   // a lane past the end computes row S - 1 again and stores nothing
  float qb[16];
  load_row_parity(qb, base + (long)ic * ld, hh);
#pragma unroll
  for (int s = 0; s < 16; ++s) qb[s] *= AT_SCALE_LOG2E;   // the backward forms q * (log2 e / sqrt 32) the same way
  float16v o;                                             // O^T: channel acc_row(t, hh) of query i
#pragma unroll
  for (int t = 0; t < 16; ++t) o[t] = 0.f;
  float m = -INFINITY, l = 0.f;                           // m is common to the two halves, l is this half's part of the sum
  const unsigned long long rowbase = (((unsigned long long)b * H + h) * S + ic) * (unsigned long long)S;
  const bool aligned = (S & 3) == 0;                      // every run of four keys is one Philox group

  for (int k0 = 0; k0 < S; k0 += MF_ROWS) {
    float ka[16];
    load_row_parity(ka, base + D + (long)min(k0 + r, S - 1) * ld, hh);
    float16v st;
#pragma unroll
    for (int t = 0; t < 16; ++t) st[t] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[s], qb[s], st, 0, 0, 0);   // channels 2 s, 2 s + 1
    float va[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) va[t] = base[2 * D + (long)min(k0 + acc_row(t, hh), S - 1) * ld + r];
    float mt = m;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (k0 + acc_row(t, hh) >= S) st[t] = -INFINITY;
      mt = fmaxf(mt, st[t]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));   // key k0 is real and lies in half 0: finite in both halves from the first tile on
    unsigned keep = 0xffffu;
    if (DROP) {
      keep = 0u;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {        // keys k0 + 8 q4 + 4 hh .. + 3 are registers 4 q4 .. 4 q4 + 3
        const unsigned long long f0 = rowbase + (unsigned long long)(k0 + 8 * q4 + 4 * hh);
        unsigned bits = dropout_keep4(a.d, f0 >> 2);
        if (!aligned) {
          const unsigned sh = (unsigned)(f0 & 3ull);
          bits = ((bits >> sh) | (dropout_keep4(a.d, (f0 >> 2) + 1) << (4 - sh))) & 15u;
        }
        keep |= bits << (4 * q4);
      }
    }
    const float alpha = __builtin_amdgcn_exp2f(m - mt);   // m = -inf the first time: 0
    l *= alpha;
#pragma unroll
    for (int t = 0; t < 16; ++t) o[t] *= alpha;
    float pt[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float p = __builtin_amdgcn_exp2f(st[t] - mt);   // a masked key: exp2(-inf) = 0
      l += p;
      pt[t] = DROP ? ((keep >> t) & 1u ? p * a.d.scale : 0.f) : p;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) o = __builtin_amdgcn_mfma_f32_32x32x2f32(va[t], pt[t], o, 0, 0, 0);   // keys acc_row(t, 0), acc_row(t, 1)
    m = mt;
  }
  const float lall = l + __shfl_xor(l, 32, 64);
  if (valid) {
    const float inv = 1.f / lall;
    float* op = a.out + ((long)b * S + i) * D + 32 * h + 4 * hh;
#pragma unroll
    for (int g = 0; g < 4; ++g) *(float4*)(op + 8 * g) = make_float4(o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv);
    if (a.lse && hh == 0) {
      float* stat = a.lse + 2 * (((long)b * H + h) * S + i);
      stat[0] = m;
      stat[1] = __builtin_amdgcn_logf(lall);   // v_log_f32 is log2
    }
  }
}

// dQ role: the block owns 64 queries; K and V stream.  dq_i = scale * sum_j ds_ij k_j, ds_ij = p_ij (dp_ij - delta_i),
// dp_ij = mask_ij / (1 - p) * (dO_i . v_j), delta_i = dO_i . o_i.
template <bool DROP>
__device__ __forceinline__ void attn_bwd_dq(const AttnArgs& a, float4* T0, float4* T1, int tile) {
  const int tid = threadIdx.x, sub = tid & 3, r = tid >> 2;
  const int S = a.S, H = a.H, D = 32 * H;
  const int b = blockIdx.z, h = blockIdx.y, i = tile * AT_ROWS + r;
  const long ld = 3L * D;
  const float* base = a.qkv + (long)b * S * ld + 32 * h;
  const bool valid = i < S;
  const int ic = valid ? i : S - 1;
  float q[32], go[32], dq[32];
  load_row32(q, base + (long)ic * ld);
  load_row32(go, a.gout + ((long)b * S + ic) * D + 32 * h);
  float delta = 0.f;
  {
    float ov[32];
    load_row32(ov, a.o + ((long)b * S + ic) * D + 32 * h);
#pragma unroll
    for (int c = 0; c < 32; ++c) delta = fmaf(go[c], ov[c], delta);
  }
#pragma unroll
  for (int c = 0; c < 32; ++c) { q[c] *= AT_SCALE_LOG2E; dq[c] = 0.f; }
  const float lse_m = a.lse_in[2 * (((long)b * H + h) * S + ic)], lse_l = a.lse_in[2 * (((long)b * H + h) * S + ic) + 1];
  const unsigned long long rowbase = (((unsigned long long)b * H + h) * S + ic) * (unsigned long long)S;

  for (int k0 = 0; k0 < S; k0 += AT_ROWS) {
    __syncthreads();
    stage_tile(T0, base + D, ld, k0, S, tid);
    stage_tile(T1, base + 2 * D, ld, k0, S, tid);
    __syncthreads();
    const int j0 = k0 + sub * AT_PER_LANE;
    if (j0 < S) {
      unsigned keep = 0xffffu;
      if (DROP) keep = keep16(a.d, rowbase + j0);
#pragma unroll
      for (int n = 0; n < AT_PER_LANE; ++n) {
        const int row = sub * AT_PER_LANE + n;
        const float s = dot_tile_row(q, T0, row);
        const float p = j0 + n < S ? __builtin_amdgcn_exp2f((s - lse_m) - lse_l) : 0.f;
        float dp = dot_tile_row(go, T1, row);
        if (DROP) dp = (keep >> n) & 1u ? dp * a.d.scale : 0.f;
        axpy_tile_row(dq, p * (dp - delta), T0, row);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 32; ++c) dq[c] = quad_sum(dq[c]);
  if (valid) store_slice8(a.gqkv + ((long)b * S + i) * ld + 32 * h, dq, sub, AT_SCALE);
}

// dKV role: the block owns 64 keys; Q and dO stream, with each query's log-sum-exp and delta beside them.
// dv_j = sum_i pd_ij dO_i, dk_j = scale * sum_i ds_ij q_i.  Q is staged times log2(e) / sqrt(32), as the forward holds it, and the
// dot product runs over the channels in the forward's order: the logit, and with it the probability, has the forward's bits.
template <bool DROP>
__device__ __forceinline__ void attn_bwd_dkv(const AttnArgs& a, float4* T0, float4* T1, float2* lse_s, float* delta_s, int tile) {
  const int tid = threadIdx.x, sub = tid & 3, r = tid >> 2;
  const int S = a.S, H = a.H, D = 32 * H;
  const int b = blockIdx.z, h = blockIdx.y, j = tile * AT_ROWS + r;
  const long ld = 3L * D;
  const float* base = a.qkv + (long)b * S * ld + 32 * h;
  const float* gbase = a.gout + (long)b * S * D + 32 * h;
  const float* obase = a.o + (long)b * S * D + 32 * h;
  const bool valid = j < S;
  const int jc = valid ? j : S - 1;
  float k[32], v[32], dk[32], dv[32];
  load_row32(k, base + D + (long)jc * ld);
  load_row32(v, base + 2 * D + (long)jc * ld);
#pragma unroll
  for (int c = 0; c < 32; ++c) { dk[c] = 0.f; dv[c] = 0.f; }
  const unsigned long long headbase = ((unsigned long long)b * H + h) * S;

  for (int q0 = 0; q0 < S; q0 += AT_ROWS) {
    __syncthreads();
    stage_tile(T0, base, ld, q0, S, tid, AT_SCALE_LOG2E);
    stage_tile(T1, gbase, D, q0, S, tid);
    {   // thread (r, sub): channels 8 sub .. 8 sub + 7 of delta of query q0 + r
      const int i = q0 + r;
      float part = 0.f;
      if (i < S) {
        const float* gp = gbase + (long)i * D + 8 * sub;
        const float* op = obase + (long)i * D + 8 * sub;
        const float4 g0 = *(const float4*)gp, g1 = *(const float4*)(gp + 4), o0 = *(const float4*)op, o1 = *(const float4*)(op + 4);
        part = fmaf(g0.x, o0.x, part); part = fmaf(g0.y, o0.y, part); part = fmaf(g0.z, o0.z, part); part = fmaf(g0.w, o0.w, part);
        part = fmaf(g1.x, o1.x, part); part = fmaf(g1.y, o1.y, part); part = fmaf(g1.z, o1.z, part); part = fmaf(g1.w, o1.w, part);
      }
      part = quad_sum(part);
      if (sub == 0) {
        delta_s[r] = part;
        lse_s[r] = i < S ? *(const float2*)(a.lse_in + 2 * (((long)b * H + h) * S + i)) : make_float2(0.f, 0.f);
      }
    }
    __syncthreads();
    const int i0 = q0 + sub * AT_PER_LANE;
    if (i0 < S) {
#pragma unroll 4
      for (int n = 0; n < AT_PER_LANE; ++n) {
        const int row = sub * AT_PER_LANE + n, i = i0 + n;
        const float s = dot_tile_row(k, T0, row);
        const float2 st = lse_s[row];
        const float p = i < S ? __builtin_amdgcn_exp2f((s - st.x) - st.y) : 0.f;
        float dp = dot_tile_row(v, T1, row);
        float pd = p;
        if (DROP) {
          const unsigned long long flat = (headbase + (unsigned long long)min(i, S - 1)) * (unsigned long long)S + jc;
          const bool kept = (dropout_keep4(a.d, flat >> 2) >> (unsigned)(flat & 3ull)) & 1u;
          dp = kept ? dp * a.d.scale : 0.f;
          pd = kept ? p * a.d.scale : 0.f;
        }
        axpy_tile_row(dv, pd, T1, row);
        axpy_tile_row(dk, p * (dp - delta_s[row]), T0, row);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 32; ++c) { dk[c] = quad_sum(dk[c]); dv[c] = quad_sum(dv[c]); }
  if (valid) {
    float* gp = a.gqkv + ((long)b * S + j) * ld + 32 * h;
    store_slice8(gp + D, dk, sub, AT_SCALE / AT_SCALE_LOG2E);   // the staged q carries log2(e) / sqrt(32)
    store_slice8(gp + 2 * D, dv, sub, 1.f);
  }
}

// blockIdx.x < tiles: the dQ role of query tile blockIdx.x; else the dKV role of key tile blockIdx.x - tiles
template <bool DROP>
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_kernel(const AttnArgs a) {
  __shared__ float4 T0[AT_ROWS * 8], T1[AT_ROWS * 8];
  __shared__ float2 lse_s[AT_ROWS];
  __shared__ float delta_s[AT_ROWS];
  const int tiles = (a.S + AT_ROWS - 1) / AT_ROWS;
  if ((int)blockIdx.x < tiles) attn_bwd_dq<DROP>(a, T0, T1, blockIdx.x);
  else attn_bwd_dkv<DROP>(a, T0, T1, lse_s, delta_s, blockIdx.x - tiles);
}

// ---- LayerNorm(x + dropout(y)) ---------------------------------------------------------------------------------------------
// One wave per row; a lane holds float4 number lane + 64 t of the row, t < LN_MAXV (D <= 1024), in registers.
constexpr int LN_THREADS = 256;
constexpr int LN_WAVES = LN_THREADS / 64;
constexpr int LN_MAXV = 4;
constexpr int LN_MAX_D = 256 * LN_MAXV;
constexpr int LN_MAX_BLOCKS = 256;   // partial rows of the backward's column sums

struct LnArgs {
  const float *x, *y, *w, *b;   // x, y (M, D); w, b (D)
  float* out;                   // forward: (M, D)
  float *mean, *rstd;           // (M): written by the forward, read by the backward
  const float* g;               // backward: (M, D)
  float *dx, *dy;               // backward: (M, D), either may be nullptr
  float* part;                  // backward: (blocks, 2, D) partial column sums of dweight | dbias
  long M;
  int D;
  long rows_per_block;          // backward
  float eps;
  float lo, hi;                 // the CLAMP instances: z = clamp(x + y, lo, hi) before the statistics
  DropArgs d;
};

__device__ __forceinline__ float wave_sum(float x) {   // a butterfly: the same bits in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// z = x + dropout(y) of float4 number v of row `row`
template <bool DROP>
__device__ __forceinline__ float4 ln_load_z(const LnArgs& a, long row, int v, unsigned& keep) {
  const long e = row * a.D + 4L * v;
  const float4 xv = *(const float4*)(a.x + e);
  float4 yv = *(const float4*)(a.y + e);
  keep = 0xfu;
  if (DROP) {
    keep = dropout_keep4(a.d, (unsigned long long)e >> 2);
    yv.x = keep & 1u ? yv.x * a.d.scale : 0.f; yv.y = keep & 2u ? yv.y * a.d.scale : 0.f;
    yv.z = keep & 4u ? yv.z * a.d.scale : 0.f; yv.w = keep & 8u ? yv.w * a.d.scale : 0.f;
  }
  return make_float4(xv.x + yv.x, xv.y + yv.y, xv.z + yv.z, xv.w + yv.w);
}

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

template <bool DROP, bool CLAMP = false>
__global__ __launch_bounds__(LN_THREADS) void addln_fwd_kernel(const LnArgs a) {
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
      unsigned keep;
      z[t] = ln_load_z<DROP>(a, row, v, keep);
      if (CLAMP) ln_clamp4(z[t], a.lo, a.hi);
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

// Block `blk` owns rows [blk * rows_per_block, ...): wave w takes every fourth of them in ascending order and keeps its
// column sums of g * zhat and g in registers; the four waves' sums are added in wave order into partial row `blk`.
template <bool DROP, bool CLAMP = false>
__global__ __launch_bounds__(LN_THREADS) void addln_bwd_kernel(const LnArgs a) {
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
    unsigned keep[LN_MAXV], inside[LN_MAXV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < LN_MAXV; ++t) {
      const int v = lane + 64 * t;
      zh[t] = gw[t] = make_float4(0.f, 0.f, 0.f, 0.f);
      keep[t] = 0u;
      inside[t] = 0xfu;
      if (v < nv) {
        float4 z = ln_load_z<DROP>(a, row, v, keep[t]);
        if (CLAMP) inside[t] = ln_clamp4(z, a.lo, a.hi);
        const float4 g = *(const float4*)(a.g + row * a.D + 4L * v);
        zh[t] = make_float4((z.x - mean) * rstd, (z.y - mean) * rstd, (z.z - mean) * rstd, (z.w - mean) * rstd);
        gw[t] = make_float4(g.x * w[t].x, g.y * w[t].y, g.z * w[t].z, g.w * w[t].w);
        s1 += (gw[t].x + gw[t].y) + (gw[t].z + gw[t].w);
        s2 += (gw[t].x * zh[t].x + gw[t].y * zh[t].y) + (gw[t].z * zh[t].z + gw[t].w * zh[t].w);
        dw[t].x = fmaf(g.x, zh[t].x, dw[t].x); dw[t].y = fmaf(g.y, zh[t].y, dw[t].y);
        dw[t].z = fmaf(g.z, zh[t].z, dw[t].z); dw[t].w = fmaf(g.w, zh[t].w, dw[t].w);
        db[t].x += g.x; db[t].y += g.y; db[t].z += g.z; db[t].w += g.w;
      }
    }
    const float c1 = wave_sum(s1) * inv_d, c2 = wave_sum(s2) * inv_d;
#pragma unroll
    for (int t = 0; t < LN_MAXV; ++t) {
      const int v = lane + 64 * t;
      if (v < nv) {
        float4 dz = make_float4(rstd * (gw[t].x - c1 - zh[t].x * c2), rstd * (gw[t].y - c1 - zh[t].y * c2),
                                rstd * (gw[t].z - c1 - zh[t].z * c2), rstd * (gw[t].w - c1 - zh[t].w * c2));
        if (CLAMP) {   // no gradient through an element that the clamp moved
          dz.x = inside[t] & 1u ? dz.x : 0.f; dz.y = inside[t] & 2u ? dz.y : 0.f;
          dz.z = inside[t] & 4u ? dz.z : 0.f; dz.w = inside[t] & 8u ? dz.w : 0.f;
        }
        if (a.dx) *(float4*)(a.dx + row * a.D + 4L * v) = dz;
        if (a.dy) {
          float4 dyv = dz;
          if (DROP) {
            dyv.x = keep[t] & 1u ? dz.x * a.d.scale : 0.f; dyv.y = keep[t] & 2u ? dz.y * a.d.scale : 0.f;
            dyv.z = keep[t] & 4u ? dz.z * a.d.scale : 0.f; dyv.w = keep[t] & 8u ? dz.w * a.d.scale : 0.f;
          }
          *(float4*)(a.dy + row * a.D + 4L * v) = dyv;
        }
      }
    }
  }
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
__global__ __launch_bounds__(256) void addln_reduce_kernel(const float* part, int nblocks, int D, float* dweight, float* dbias) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * D) return;
  float s = 0.f;
  for (int k = 0; k < nblocks; ++k) s += part[(long)k * 2 * D + c];
  if (c < D) { if (dweight) dweight[c] = s; }
  else if (dbias) dbias[c - D] = s;
}

// ---- dropout(relu(h)), its backward, and the mask itself -------------------------------------------------------------------
// One thread per group of four elements (the Philox call's four words); the last group of a tensor may be shorter.
template <bool DROP, bool BWD>
__global__ __launch_bounds__(256) void relu_drop_kernel(const float* in, const float* saved, float* out, long n, const DropArgs d) {
  const long grp = (long)blockIdx.x * 256 + threadIdx.x, e = grp * 4;
  if (e >= n) return;
  unsigned keep = 0xfu;
  if (DROP) keep = dropout_keep4(d, (unsigned long long)grp);
  const float scale = DROP ? d.scale : 1.f;
  float x[4], sv[4], y[4];
  const bool full = e + 4 <= n;
  if (full) {
    const float4 v = *(const float4*)(in + e);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    if (BWD) { const float4 u = *(const float4*)(saved + e); sv[0] = u.x; sv[1] = u.y; sv[2] = u.z; sv[3] = u.w; }
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      x[t] = e + t < n ? in[e + t] : 0.f;
      if (BWD) sv[t] = e + t < n ? saved[e + t] : 0.f;
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const bool kept = (keep >> t) & 1u;
    if (BWD) y[t] = kept && sv[t] > 0.f ? (DROP ? x[t] * scale : x[t]) : 0.f;   // in = grad_out, saved = the forward's output
    else y[t] = kept && x[t] > 0.f ? (DROP ? x[t] * scale : x[t]) : 0.f;
  }
  if (full) *(float4*)(out + e) = make_float4(y[0], y[1], y[2], y[3]);
  else {
#pragma unroll
    for (int t = 0; t < 4; ++t) if (e + t < n) out[e + t] = y[t];
  }
}

__global__ __launch_bounds__(256) void keep_mask_kernel(unsigned char* mask, long n, const DropArgs d) {
  const long grp = (long)blockIdx.x * 256 + threadIdx.x, e = grp * 4;
  if (e >= n) return;
  const unsigned keep = dropout_keep4(d, (unsigned long long)grp);
#pragma unroll
  for (int t = 0; t < 4; ++t) if (e + t < n) mask[e + t] = (unsigned char)((keep >> t) & 1u);
}

DropArgs drop_args(float p, unsigned long long seed, int site) {
  DropArgs d{};
  d.seed = seed;
  d.site = (unsigned)site;
  d.thr = (unsigned)((double)p * 4294967296.0);   // p in [0, 1): below 2^32
  d.scale = (float)(1.0 / (1.0 - (double)p));
  return d;
}

}  // namespace

int launch_dfine_attn_forward(const float* qkv, int B, int S, int H, float p, unsigned long long seed, int site, float* out,
                              float* lse, hipStream_t s) {
  AttnArgs a{};
  a.qkv = qkv; a.out = out; a.lse = lse; a.S = S; a.H = H; a.d = drop_args(p, seed, site);
  const dim3 grid((S + MF_ROWS - 1) / MF_ROWS, H, B);
  if (p > 0.f) hipLaunchKernelGGL(attn_fwd_kernel<true>, grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL(attn_fwd_kernel<false>, grid, dim3(64), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_attn_backward(const float* gout, const float* qkv, const float* out, const float* lse, int B, int S, int H, float p,
                               unsigned long long seed, int site, float* gqkv, hipStream_t s) {
  AttnArgs a{};
  a.qkv = qkv; a.gout = gout; a.o = out; a.lse_in = lse; a.gqkv = gqkv; a.S = S; a.H = H; a.d = drop_args(p, seed, site);
  const dim3 grid(2 * ((S + AT_ROWS - 1) / AT_ROWS), H, B);
  if (p > 0.f) hipLaunchKernelGGL(attn_bwd_kernel<true>, grid, dim3(AT_THREADS), 0, s, a);
  else hipLaunchKernelGGL(attn_bwd_kernel<false>, grid, dim3(AT_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int dfine_addln_max_d() { return LN_MAX_D; }

long dfine_addln_rows_per_block(long M) {
  long blocks = (M + LN_WAVES - 1) / LN_WAVES;
  if (blocks > LN_MAX_BLOCKS) blocks = LN_MAX_BLOCKS;
  const long rpb = (M + blocks - 1) / blocks;
  return (rpb + LN_WAVES - 1) / LN_WAVES * LN_WAVES;
}

size_t dfine_addln_workspace_bytes(long M, int D) {
  if (M < 1 || D < 1) return 0;
  const long rpb = dfine_addln_rows_per_block(M);
  return (size_t)((M + rpb - 1) / rpb) * 2 * (size_t)D * sizeof(float);
}

int launch_dfine_addln_forward(const float* x, const float* y, const float* w, const float* b, long M, int D, float eps, float p,
                               unsigned long long seed, int site, float* out, float* mean, float* rstd, hipStream_t s) {
  LnArgs a{};
  a.x = x; a.y = y; a.w = w; a.b = b; a.out = out; a.mean = mean; a.rstd = rstd; a.M = M; a.D = D; a.eps = eps;
  a.d = drop_args(p, seed, site);
  const dim3 grid((unsigned)((M + LN_WAVES - 1) / LN_WAVES));
  if (p > 0.f) hipLaunchKernelGGL(addln_fwd_kernel<true>, grid, dim3(LN_THREADS), 0, s, a);
  else hipLaunchKernelGGL(addln_fwd_kernel<false>, grid, dim3(LN_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_addln_backward(const float* g, const float* x, const float* y, const float* w, const float* mean, const float* rstd,
                                long M, int D, float p, unsigned long long seed, int site, float* dx, float* dy, float* dweight,
                                float* dbias, float* work, hipStream_t s) {
  LnArgs a{};
  a.x = x; a.y = y; a.w = w; a.g = g; a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.dx = dx; a.dy = dy;
  a.part = work; a.M = M; a.D = D; a.rows_per_block = dfine_addln_rows_per_block(M);
  a.d = drop_args(p, seed, site);
  const int blocks = (int)((M + a.rows_per_block - 1) / a.rows_per_block);
  if (p > 0.f) hipLaunchKernelGGL(addln_bwd_kernel<true>, dim3(blocks), dim3(LN_THREADS), 0, s, a);
  else hipLaunchKernelGGL(addln_bwd_kernel<false>, dim3(blocks), dim3(LN_THREADS), 0, s, a);
  int rc = (int)hipGetLastError();
  if (rc != 0 || (!dweight && !dbias)) return rc;
  return launch_dfine_addln_reduce(work, blocks, D, dweight, dbias, s);
}

int launch_dfine_addln_reduce(const float* part, int blocks, int D, float* dweight, float* dbias, hipStream_t s) {
  hipLaunchKernelGGL(addln_reduce_kernel, dim3((2 * D + 255) / 256), dim3(256), 0, s, part, blocks, D, dweight, dbias);
  return (int)hipGetLastError();
}

// LayerNorm(clamp(x + y, lo, hi)): the CLAMP instances of the same device code, without dropout
int launch_dfine_addln_clamp_forward(const float* x, const float* y, const float* w, const float* b, long M, int D, float eps, float lo,
                                     float hi, float* out, float* mean, float* rstd, hipStream_t s) {
  LnArgs a{};
  a.x = x; a.y = y; a.w = w; a.b = b; a.out = out; a.mean = mean; a.rstd = rstd; a.M = M; a.D = D; a.eps = eps; a.lo = lo; a.hi = hi;
  hipLaunchKernelGGL((addln_fwd_kernel<false, true>), dim3((unsigned)((M + LN_WAVES - 1) / LN_WAVES)), dim3(LN_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_addln_clamp_backward(const float* g, const float* x, const float* y, const float* w, const float* mean,
                                      const float* rstd, long M, int D, float lo, float hi, float* dx, float* dy, float* dweight,
                                      float* dbias, float* work, hipStream_t s) {
  LnArgs a{};
  a.x = x; a.y = y; a.w = w; a.g = g; a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.dx = dx; a.dy = dy;
  a.part = work; a.M = M; a.D = D; a.rows_per_block = dfine_addln_rows_per_block(M); a.lo = lo; a.hi = hi;
  const int blocks = (int)((M + a.rows_per_block - 1) / a.rows_per_block);
  hipLaunchKernelGGL((addln_bwd_kernel<false, true>), dim3(blocks), dim3(LN_THREADS), 0, s, a);
  const int rc = (int)hipGetLastError();
  if (rc != 0 || (!dweight && !dbias)) return rc;
  return launch_dfine_addln_reduce(work, blocks, D, dweight, dbias, s);
}

int launch_dfine_relu_dropout(const float* in, const float* saved, float* out, long n, float p, unsigned long long seed, int site,
                              hipStream_t s) {
  const DropArgs d = drop_args(p, seed, site);
  const dim3 grid((unsigned)(((n + 3) / 4 + 255) / 256));
  if (saved) {
    if (p > 0.f) hipLaunchKernelGGL((relu_drop_kernel<true, true>), grid, dim3(256), 0, s, in, saved, out, n, d);
    else hipLaunchKernelGGL((relu_drop_kernel<false, true>), grid, dim3(256), 0, s, in, saved, out, n, d);
  } else {
    if (p > 0.f) hipLaunchKernelGGL((relu_drop_kernel<true, false>), grid, dim3(256), 0, s, in, saved, out, n, d);
    else hipLaunchKernelGGL((relu_drop_kernel<false, false>), grid, dim3(256), 0, s, in, saved, out, n, d);
  }
  return (int)hipGetLastError();
}

int launch_dfine_keep_mask(unsigned char* mask, long n, float p, unsigned long long seed, int site, hipStream_t s) {
  hipLaunchKernelGGL(keep_mask_kernel, dim3((unsigned)(((n + 3) / 4 + 255) / 256)), dim3(256), 0, s, mask, n, drop_args(p, seed, site));
  return (int)hipGetLastError();
}

}  // namespace m355
