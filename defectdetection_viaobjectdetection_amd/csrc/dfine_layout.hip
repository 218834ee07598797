// D-FINE layout kernels: NCHW feature maps <-> token rows, and the exact GELU of the AIFI layer's MLP.
//   maps_to_tokens: L <= 8 contiguous maps (B, D, h_l, w_l) -> tokens (B, S, D), S = sum h_l w_l, level l's pixel (y, x) at token
//     start_l + y w_l + x, and optionally a second output from the same read: tokens + pos (S, D) or mask (S) * tokens.
//   tokens_to_maps: its adjoint, map_l[b, c, y, x] = tokens[b, s, c] (+ extra[b, s, c] (* mask[s])).
// Both are one launch for all levels: a tiled transpose through LDS, LT_P tokens x LT_C channels per block.  The map side has lanes
// along the pixels of one channel (contiguous in NCHW), the token side has lanes along the channels as 16-byte accesses.  A map row
// starts at element (b D + c) h w + p0, which is 16-byte aligned only when h w is a multiple of 4 (p0 is a multiple of LT_P): such
// a level takes 16-byte map accesses, every other level 4-byte ones.  The tile is token-major with the odd stride LT_C + 1, and the
// lane -> element maps below put the 32 lanes of a half wave on 32 different banks in every LDS access of either side.
// The block -> (level, image, token tile, channel tile) map is the host-built prefix blk0 (as the MSDA backward's block starts).
// Every element offset is 64-bit.  No atomics, one writer per element, one rounding per written operation (-ffp-contract=off).
#include "common.h"

namespace m355 {

namespace {

constexpr int LT_P = 64;              // tokens (pixels of one level) per tile
constexpr int LT_C = 64;              // channels per tile
constexpr int LT_STRIDE = LT_C + 1;   // floats between the tile's token rows
constexpr int LT_THREADS = 256;

struct LayoutArgs {
  const float* src[8];   // maps_to_tokens: the maps
  float* dst[8];         // tokens_to_maps: the maps
  int hw[8], start[8], npt[8], blk0[9];   // per level: pixels, first token, token tiles; blocks before the level
  int L, D, S, nct;      // nct: channel tiles
  const float* tokens_in;   // tokens_to_maps: may be nullptr when extra is given
  const float* extra_in;    // tokens_to_maps: may be nullptr
  float* tokens;
  float* extra;          // maps_to_tokens: nullptr without pos and mask
  const float* pos;
  const float* mask;
};

struct TilePos { int l, b, p0, c0; };

__device__ inline TilePos locate(const LayoutArgs& a) {
  const int blk = (int)blockIdx.x;
  int l = 0;
  while (l + 1 < a.L && blk >= a.blk0[l + 1]) ++l;
  int r = blk - a.blk0[l];
  TilePos t;
  t.l = l;
  t.c0 = (r % a.nct) * LT_C; r /= a.nct;
  t.p0 = (r % a.npt[l]) * LT_P;
  t.b = r / a.npt[l];
  return t;
}

// token side: unit u of the tile's LT_P x LT_C / 4 float4s -> (token, first channel).  32 consecutive units are 4 tokens x 8 channel
// quads: LDS word p LT_STRIDE + 4 q + j lies on bank (p + 4 q + j) mod 32, all different; 8 lanes share 128 contiguous bytes of a row
__device__ inline void token_unit(int u, int& p, int& c) {
  c = 4 * ((u & 7) + 8 * ((u >> 5) & 1));
  p = ((u >> 3) & 3) + 4 * (u >> 6);
}
// map side, 16-byte form: unit u -> (first pixel, channel).  32 consecutive units are 8 pixel quads x 4 channels: word
// (4 i + k) LT_STRIDE + c lies on bank (4 i + k + c) mod 32, all different; 8 lanes share 128 contiguous bytes of a channel row
__device__ inline void map_unit4(int u, int& p, int& c) {
  p = 4 * ((u & 7) + 8 * ((u >> 5) & 1));
  c = ((u >> 3) & 3) + 4 * (u >> 6);
}

__global__ __launch_bounds__(LT_THREADS) void maps_to_tokens_kernel(const LayoutArgs a) {
  __shared__ float tile[LT_P * LT_STRIDE];
  const TilePos t = locate(a);
  const int hw = a.hw[t.l], D = a.D, tid = threadIdx.x;
  const float* src = a.src[t.l] + ((long)t.b * D + t.c0) * hw + t.p0;   // tile origin: channel c0, pixel p0 of image b
  const int np = min(LT_P, hw - t.p0), nc = min(LT_C, D - t.c0);
  if ((hw & 3) == 0) {
#pragma unroll
    for (int it = 0; it < LT_P * LT_C / 4 / LT_THREADS; ++it) {
      int p, c;
      map_unit4(tid + it * LT_THREADS, p, c);
      if (p < np && c < nc) {   // hw and p0 are multiples of 4: a quad is inside or outside as a whole
        const float4 v = *(const float4*)(src + (long)c * hw + p);
        float* w = tile + p * LT_STRIDE + c;
        w[0] = v.x; w[LT_STRIDE] = v.y; w[2 * LT_STRIDE] = v.z; w[3 * LT_STRIDE] = v.w;
      }
    }
  } else {
#pragma unroll 4
    for (int it = 0; it < LT_P * LT_C / LT_THREADS; ++it) {
      const int u = tid + it * LT_THREADS, p = u & (LT_P - 1), c = u / LT_P;
      if (p < np && c < nc) tile[p * LT_STRIDE + c] = src[(long)c * hw + p];
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < LT_P * LT_C / 4 / LT_THREADS; ++it) {
    int p, c;
    token_unit(tid + it * LT_THREADS, p, c);
    if (p >= np || c >= nc) continue;   // D is a multiple of 4
    const float* r = tile + p * LT_STRIDE + c;
    const float4 v = make_float4(r[0], r[1], r[2], r[3]);
    const long s = (long)a.start[t.l] + t.p0 + p;
    const long o = ((long)t.b * a.S + s) * D + t.c0 + c;
    *(float4*)(a.tokens + o) = v;
    if (a.pos) {
      const float4 q = *(const float4*)(a.pos + s * D + t.c0 + c);
      *(float4*)(a.extra + o) = make_float4(v.x + q.x, v.y + q.y, v.z + q.z, v.w + q.w);
    } else if (a.mask) {
      const float m = a.mask[s];   // a true multiply: 0 * inf is NaN and 0 * -x is -0, as torch's valid_mask * source_flatten
      *(float4*)(a.extra + o) = make_float4(m * v.x, m * v.y, m * v.z, m * v.w);
    }
  }
}

__global__ __launch_bounds__(LT_THREADS) void tokens_to_maps_kernel(const LayoutArgs a) {
  __shared__ float tile[LT_P * LT_STRIDE];
  const TilePos t = locate(a);
  const int hw = a.hw[t.l], D = a.D, tid = threadIdx.x;
  const int np = min(LT_P, hw - t.p0), nc = min(LT_C, D - t.c0);
#pragma unroll
  for (int it = 0; it < LT_P * LT_C / 4 / LT_THREADS; ++it) {
    int p, c;
    token_unit(tid + it * LT_THREADS, p, c);
    if (p >= np || c >= nc) continue;
    const long s = (long)a.start[t.l] + t.p0 + p;
    const long o = ((long)t.b * a.S + s) * D + t.c0 + c;
    float4 v;
    if (a.extra_in) {
      float4 e = *(const float4*)(a.extra_in + o);
      if (a.mask) { const float m = a.mask[s]; e = make_float4(m * e.x, m * e.y, m * e.z, m * e.w); }
      if (a.tokens_in) {
        const float4 k = *(const float4*)(a.tokens_in + o);
        v = make_float4(k.x + e.x, k.y + e.y, k.z + e.z, k.w + e.w);
      } else v = e;
    } else v = *(const float4*)(a.tokens_in + o);
    float* w = tile + p * LT_STRIDE + c;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  }
  __syncthreads();
  float* dst = a.dst[t.l] + ((long)t.b * D + t.c0) * hw + t.p0;
  if ((hw & 3) == 0) {
#pragma unroll
    for (int it = 0; it < LT_P * LT_C / 4 / LT_THREADS; ++it) {
      int p, c;
      map_unit4(tid + it * LT_THREADS, p, c);
      if (p < np && c < nc) {
        const float* r = tile + p * LT_STRIDE + c;
        *(float4*)(dst + (long)c * hw + p) = make_float4(r[0], r[LT_STRIDE], r[2 * LT_STRIDE], r[3 * LT_STRIDE]);
      }
    }
  } else {
#pragma unroll 4
    for (int it = 0; it < LT_P * LT_C / LT_THREADS; ++it) {
      const int u = tid + it * LT_THREADS, p = u & (LT_P - 1), c = u / LT_P;
      if (p < np && c < nc) dst[(long)c * hw + p] = tile[p * LT_STRIDE + c];
    }
  }
}

// ---- exact (erf) GELU and its backward from the saved input -------------------------------------------------------------------
// torch's expressions (aten GeluCUDAKernelImpl, approximate = "none"): x * 0.5 * (1 + erf(x / sqrt(2))) and
// g * (cdf + x * pdf), cdf = 0.5 * (1 + erf(x / sqrt(2))), pdf = exp(-x^2 / 2) / sqrt(2 pi); the last sum as one fused multiply-add.
constexpr float kSqrtHalf = 0.70710678118654752440f;
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;   // 2 / sqrt(pi) * sqrt(1 / 2) * 0.5

template <bool BWD>
__device__ inline float gelu_one(float x, float g) {
  const float cdf1 = 1.f + erff(x * kSqrtHalf);
  if (!BWD) return x * 0.5f * cdf1;
  const float pdf = expf(-0.5f * x * x) * kInvSqrt2Pi;
  return g * fmaf(x, pdf, 0.5f * cdf1);
}

// One thread per group of four elements; the last group of a tensor may be shorter.  BWD: in = grad_out, saved = the forward's input
template <bool BWD>
__global__ __launch_bounds__(256) void gelu_kernel(const float* in, const float* saved, float* out, long n) {
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= n) return;
  if (e + 4 <= n) {
    const float4 v = *(const float4*)(in + e);
    float4 h = v;
    if (BWD) h = *(const float4*)(saved + e);
    *(float4*)(out + e) = make_float4(gelu_one<BWD>(h.x, v.x), gelu_one<BWD>(h.y, v.y), gelu_one<BWD>(h.z, v.z), gelu_one<BWD>(h.w, v.w));
  } else {
    for (long i = e; i < n; ++i) out[i] = gelu_one<BWD>(BWD ? saved[i] : in[i], in[i]);
  }
}

}  // namespace

long dfine_layout_blocks(const DfineLayoutLevels& lv, int B, int D) {
  const long nct = (D + LT_C - 1) / LT_C;
  long blocks = 0;
  for (int l = 0; l < lv.L; ++l) blocks += (long)B * (((long)lv.hw[l] + LT_P - 1) / LT_P) * nct;
  return blocks;
}

static LayoutArgs layout_args(const DfineLayoutLevels& lv, int B, int D) {
  LayoutArgs a{};
  a.L = lv.L; a.D = D; a.S = (int)lv.S; a.nct = (D + LT_C - 1) / LT_C;
  int blk = 0;
  for (int l = 0; l < lv.L; ++l) {
    a.hw[l] = lv.hw[l]; a.start[l] = lv.start[l]; a.npt[l] = (lv.hw[l] + LT_P - 1) / LT_P;
    a.blk0[l] = blk;
    blk += B * a.npt[l] * a.nct;
  }
  a.blk0[lv.L] = blk;
  return a;
}

int launch_dfine_maps_to_tokens(const float* const* maps, const DfineLayoutLevels& lv, int B, int D, const float* pos, const float* mask,
                                float* tokens, float* extra, hipStream_t s) {
  LayoutArgs a = layout_args(lv, B, D);
  for (int l = 0; l < lv.L; ++l) a.src[l] = maps[l];
  a.tokens = tokens; a.extra = extra; a.pos = pos; a.mask = mask;
  hipLaunchKernelGGL(maps_to_tokens_kernel, dim3((unsigned)a.blk0[lv.L]), dim3(LT_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_tokens_to_maps(const float* tokens, const float* extra, const float* mask, const DfineLayoutLevels& lv, int B, int D,
                                float* const* maps, hipStream_t s) {
  LayoutArgs a = layout_args(lv, B, D);
  for (int l = 0; l < lv.L; ++l) a.dst[l] = maps[l];
  a.tokens_in = tokens; a.extra_in = extra; a.mask = mask;
  hipLaunchKernelGGL(tokens_to_maps_kernel, dim3((unsigned)a.blk0[lv.L]), dim3(LT_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_gelu(const float* in, const float* saved, float* out, long n, hipStream_t s) {
  const dim3 grid((unsigned)(((n + 3) / 4 + 255) / 256));
  if (saved) hipLaunchKernelGGL(gelu_kernel<true>, grid, dim3(256), 0, s, in, saved, out, n);
  else hipLaunchKernelGGL(gelu_kernel<false>, grid, dim3(256), 0, s, in, saved, out, n);
  return (int)hipGetLastError();
}

}  // namespace m355
