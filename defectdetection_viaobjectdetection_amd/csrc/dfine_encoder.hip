// The temporal encoder of the D-FINE trainers (nn.TransformerEncoderLayer, post-norm, ReLU, head dim 32) between its GEMMs:
//   attn_fwd / attn_bwd          softmax(q k^T / sqrt(32)) [dropout] v on the packed in-projection output (B, S, 3 D)
//   relu_drop_fwd / relu_drop_bwd  dropout(relu(h))
// (the layer's LayerNorm(x + dropout(y)) is a source of the row-LayerNorm kernels in dfine_rowln.hip.)
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
