// YOLO11 C2PSA attention core (gfx950): for every head h of the PSABlock's Attention, over the N = H * W tokens of the map,
//   o[h 64 + c, i] = sum_j v[c, j] softmax_j(sum_d q[d, i] k[d, j] / sqrt(32)) + pe(v)[h 64 + c, i]
// where head h's qkv channels are [q 32 | k 32 | v 64] at offset 128 h (upstream's view(B, nh, 2 kd + hd, N)) and pe is the
// depthwise 3x3 conv + folded BN (no activation) over v laid out as (B, heads 64, H, W).  One launch for all heads; the fp16
// result goes straight into the slice attn.proj reads.
//
// Grid = (query tiles of 64, heads, B); a block = 4 waves, wave w owns 16 queries.  K (64 keys x 32) and V (64 keys x 64,
// stored transposed: [channel][key]) stream through LDS in 64-key tiles -- a whole map does not fit (1024 x 1024 input:
// N = 1024, K + V of one head = 192 KB > 160 KB).
//
// Orientation: the scores are computed transposed, S^T = K Q^T (A = 16 keys x 32, B = Q^T: the lane's own query as 8 d
// values), one v_mfma_f32_16x16x32_f16 per 16 x 16 block.  Lane l (query l & 15, lane group g = l >> 4) then holds the scores
// of ITS query for keys 16 kb + 4 g + r (kb = 0..3, r = 0..3), so the online softmax is per lane plus one reduction over the
// four lane groups (two xor shuffles).  The output is also computed transposed, O^T = V^T P^T (A = 16 channels x 32 keys from
// the transposed V tile, B = P^T), so the P registers are the B operand as they stand: k-slot j of lane group g in step t is
// key 32 t + 4 g + j (j < 4) or 32 t + 16 + 4 g + j - 4 (j >= 4), and the V^T operand reads the same two 4-key runs.  O^T's
// accumulator holds, per lane, channels 16 cb + 4 g + r of the lane's query: the per-query statistics never leave the lane.
//
// Softmax: fp32, exp2 with scale * log2(e) folded into the scores, keys >= N masked to -inf.  Textbook order per tile: row max,
// m_new = max(m, tile max), alpha = exp2(m - m_new) scales O and l (nothing at the new scale exists yet), then P = exp2(s - m_new)
// and P V.  The first tile always holds key 0, so m is finite from then on and no inf - inf arises.  Epilogue: O / l + pe bias +
// the 3 x 3 neighbourhood of v (read from the qkv tensor), one rounding to fp16.
#include <math.h>
#include <stdio.h>

#include "common.h"
#include "device_prims.h"

namespace m355 {
namespace {

constexpr int PA_KEYS = 64;        // keys per LDS tile
constexpr int PA_QUERIES = 64;     // queries per block (16 per wave)
constexpr int PA_KP = 40;          // K tile pitch (fp16): 80 bytes, 16-byte aligned rows
constexpr int PA_VP = 72;          // V^T tile pitch (fp16): 144 bytes, 8-byte aligned runs

__global__ __launch_bounds__(256) void psa_attn_kernel(PsaArgs a) {
  __shared__ __attribute__((aligned(16))) half_t ks[PA_KEYS * PA_KP];
  __shared__ __attribute__((aligned(16))) half_t vt[64 * PA_VP];
  const int N = a.H * a.W;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
  const half_t* base = a.qkv + (long)b * a.q_bstride + 128 * h;
  const int qi = blockIdx.x * PA_QUERIES + 16 * wave + l15;
  const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const half8 qf = qi < N ? *(const half8*)(base + (long)qi * a.ldq + 8 * g) : zero8;

  float4v o[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) o[cb] = float4v{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  const int ntiles = (N + PA_KEYS - 1) / PA_KEYS;
#pragma unroll 1
  for (int kt = 0; kt < ntiles; ++kt) {
    const int k0 = kt * PA_KEYS;
    __syncthreads();   // the previous tile's readers are done
    {
      const int key = tid >> 2, part = tid & 3, jj = k0 + key;
      *(half8*)(ks + key * PA_KP + 8 * part) = jj < N ? *(const half8*)(base + (long)jj * a.ldq + 32 + 8 * part) : zero8;
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + 256 * it, key = idx & 63, part = idx >> 6, jj = k0 + key;
      const half8 v = jj < N ? *(const half8*)(base + (long)jj * a.ldq + 64 + 8 * part) : zero8;
#pragma unroll
      for (int e = 0; e < 8; ++e) vt[(8 * part + e) * PA_VP + key] = v[e];
    }
    __syncthreads();

    float4v s[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const half8 kf = *(const half8*)(ks + (16 * kb + l15) * PA_KP + 8 * g);
      s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, float4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = (k0 + 16 * kb + 4 * g + r) < N ? s[kb][r] * a.scale_log2e : -INFINITY;
        s[kb][r] = v;
        tmax = fmaxf(tmax, v);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mn = fmaxf(m, tmax);                 // finite: every tile but the masked tail of the last holds a real key
    const float alpha = __builtin_amdgcn_exp2f(m - mn);   // m = -inf before the first tile: alpha = 0 on zeros
    m = mn;
    l *= alpha;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) o[cb] *= alpha;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(s[kb][r] - mn);
        s[kb][r] = p;
        l += p;
      }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      half8 pf;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pf[j] = (half_t)s[2 * t][j];
        pf[4 + j] = (half_t)s[2 * t + 1][j];
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const half_t* vr = vt + (16 * cb + l15) * PA_VP + 32 * t + 4 * g;
        const half4 lo = *(const half4*)vr, hi = *(const half4*)(vr + 16);
        const half8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[cb], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qi >= N) return;
  const float inv = 1.0f / l;
  const int py = qi / a.W, px = qi - py * a.W;
  half_t* yp = a.y + (long)b * a.y_bstride + (long)qi * a.ldy + 64 * h;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int c = 16 * cb + 4 * g;              // this lane's 4 channels of the head
    const int ch = 64 * h + c;                  // ... of the pe conv
    float acc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = py + dy, xx = px + dx;
        if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) continue;
        const half4 v = *(const half4*)(base + ((long)yy * a.W + xx) * a.ldq + 64 + c);
        const half4 w = *(const half4*)(a.pe_w + (long)((dy + 1) * 3 + dx + 1) * a.C + ch);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = __builtin_fmaf((float)w[r], (float)v[r], acc[r]);
      }
    half4 out;
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = m355_to_half(o[cb][r] * inv + (acc[r] + a.pe_b[ch + r]));
    *(half4*)(yp + c) = out;
  }
}

}  // namespace

bool psa_attn_ok(const PsaArgs& a) {
  if (!a.qkv || !a.pe_w || !a.pe_b || !a.y) return false;
  if (a.B < 1 || a.B > 65535 || a.H < 1 || a.W < 1 || a.heads < 1 || a.heads > 64 || a.C != 64 * a.heads) return false;
  if (a.ldq < 128 * a.heads || a.ldq % 8 || a.ldy < a.C || a.ldy % 4) return false;
  if (((uintptr_t)a.qkv & 15) || ((uintptr_t)a.y & 7) || ((uintptr_t)a.pe_w & 7)) return false;
  const long N = (long)a.H * a.W;
  if (N > (1L << 24) || a.q_bstride < (N - 1) * a.ldq + 128 * a.heads || a.y_bstride < (N - 1) * a.ldy + a.C) return false;
  return true;
}

int launch_psa_attn(const PsaArgs& a, hipStream_t s) {
  if (!psa_attn_ok(a)) return -1;
  const int N = a.H * a.W;
  const dim3 grid((N + PA_QUERIES - 1) / PA_QUERIES, a.heads, a.B);
  hipLaunchKernelGGL(psa_attn_kernel, grid, dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace m355
