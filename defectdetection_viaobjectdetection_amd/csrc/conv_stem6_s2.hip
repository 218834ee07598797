// YOLOv5u model.0: Conv(3 -> C0, 6x6, stride 2, pad 2) + BN (folded) + SiLU on the uint8 letterboxed image (gfx950).
//   y = SiLU(conv6x6_s2_p2(x_u8; w) * (1/255) + b), fp16 NHWC (B, H/2, W/2, C0), C0 in {16, 32, 48}.
// Rounding points as the YOLOv8 stem (conv_stem_s2c32.hip stage A): uint8 -> fp16 is exact, fp16 weights, fp32 sums, then
// x 1/255 and + bias in fp32, SiLU, one rounding to fp16.
//
// K order (kh, kw, c), 108 taps padded to 128 = 4 steps of v_mfma_f32_16x16x32_f16.  For one kernel row kh, the 6 taps x 3
// channels of output pixel wo are the 18 CONSECUTIVE bytes of input row 2 ho - 2 + kh starting at byte 6 wo - 6, and 18 is
// even: every aligned tap pair (k, k + 1) lies inside one kernel row.  So the B operand (8 taps per lane) is four 4-byte LDS
// reads of a fp16 copy of the window -- no byte gathers.
//
// Block = 4 waves = a tile of 4 output rows x 64 output pixels.  The block stages input rows 2 ho0 - 2 .. 2 ho0 + 9 (12 rows),
// bytes [S, S + 416) of each, converted to fp16 in LDS (16-byte global loads, 32-byte LDS stores; S = the window's first byte
// rounded down to 16, so a 16-byte chunk is wholly inside or wholly outside an image row: 3 W is a multiple of 16).  Rows and
// chunks outside the image are zeros: the conv's padding.  Wave w owns output row ho0 + w and walks its 4 groups of 16 pixels.
//
// Output: the host packs the weight rows so that, for each pair of 16-channel tiles, lane group g's 2 x 4 accumulators are the
// 8 consecutive channels 32 p + 8 g .. 32 p + 8 g + 7 (one 16-byte store per lane); a last unpaired tile (C0 = 16, 48) stores
// 4 channels (8 bytes) per lane.
#include <stdio.h>

#include "common.h"
#include "device_prims.h"

namespace m355 {
namespace {

constexpr int S6_TH = 4, S6_TW = 64;           // output tile: rows x pixels (one wave per row)
constexpr int S6_ROWS = 2 * S6_TH + 4;         // 12 staged input rows
constexpr int S6_CHUNKS = 26;                  // 16-byte chunks per staged row: 6 * 63 + 15 + 18 <= 416 bytes
constexpr int S6_RP = S6_CHUNKS * 16 + 8;      // LDS row pitch in fp16 elements (848 bytes: 16-byte aligned)
static_assert(S6_ROWS * S6_RP * 2 == 10176, "window: 10 176 bytes of LDS");

template <int NT>   // 16-channel tiles: C0 / 16
__global__ __launch_bounds__(256) void stem6_s2_kernel(const Stem6Args a) {
  __shared__ __attribute__((aligned(16))) half_t win[S6_ROWS * S6_RP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int Ho = a.H >> 1, Wo = a.W >> 1, rowb = a.W * 3;
  const int wo0 = blockIdx.x * S6_TW, ho0 = blockIdx.y * S6_TH, b = blockIdx.z;
  const int first = 6 * wo0 - 6;                               // first window byte of the tile's first pixel (may be < 0)
  const int S = (first >= 0 ? first : first - 15) / 16 * 16;   // floor to a multiple of 16
  const int D = first - S;                                     // even, 0 .. 14

  // ---- stage the window: 12 rows x 26 chunks, uint8 -> fp16
  const uint8_t* xb = a.x + (long)b * a.H * rowb;
  for (int i = tid; i < S6_ROWS * S6_CHUNKS; i += 256) {
    const int rl = i / S6_CHUNKS, ch = i - rl * S6_CHUNKS;
    const int gr = 2 * ho0 - 2 + rl, gb = S + 16 * ch;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)gr < (unsigned)a.H && gb >= 0 && gb + 16 <= rowb) v = *(const uint4*)(xb + (long)gr * rowb + gb);
    half8 lo, hi;
    const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      lo[j] = (half_t)(float)((wv[j >> 2] >> (8 * (j & 3))) & 0xffu);
      hi[j] = (half_t)(float)((wv[2 + (j >> 2)] >> (8 * (j & 3))) & 0xffu);
    }
    half8* dst = (half8*)(win + rl * S6_RP + 16 * ch);
    dst[0] = lo;
    dst[1] = hi;
  }

  // ---- weights (A operand) and biases in registers
  half8 wf[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) wf[t][s] = *(const half8*)(a.w + (long)(t * 16 + l15) * 128 + 32 * s + 8 * g);
  float bias[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool paired = (t ^ 1) < NT;
      const int ch = paired ? 32 * (t >> 1) + 8 * g + 4 * (t & 1) + i : 16 * t + 4 * g + i;
      bias[t][i] = a.bias[ch];
    }
  // tap-pair offsets of this lane (fp16 elements relative to the pixel's window start): pair p = 16 s + 4 g + q holds taps
  // k = 2 p, 2 p + 1 = (kh, j = 2 p - 18 kh); pairs past tap 107 read a valid element (their weights are zero)
  int poff[4][4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k0 = 2 * (16 * s + 4 * g + q);
      const int kh = k0 / 18;
      poff[s][q] = k0 < 108 ? kh * S6_RP + (k0 - 18 * kh) : 0;
    }
  __syncthreads();

  const int ho = ho0 + wave;
  if (ho >= Ho) return;
  const float inv255 = 1.0f / 255.0f;
  half_t* yrow = a.y + (long)b * a.y_bstride + (long)ho * Wo * a.ldy;
#pragma unroll 1
  for (int grp = 0; grp < S6_TW / 16; ++grp) {
    const int wl = 16 * grp + l15, wo = wo0 + wl;
    if (wo0 + 16 * grp >= Wo) break;                           // (wave-uniform: Wo is a multiple of 8, groups start at multiples of 16)
    const half_t* px = win + 2 * wave * S6_RP + 6 * wl + D;
    float4v acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      union { unsigned u[4]; half8 h; } bf;
#pragma unroll
      for (int q = 0; q < 4; ++q) bf.u[q] = *(const unsigned*)(px + poff[s][q]);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[t][s], bf.h, acc[t], 0, 0, 0);
    }
    if (wo >= Wo) continue;
    half_t* yp = yrow + (long)wo * a.ldy;
#pragma unroll
    for (int t = 0; t + 1 < NT; t += 2) {
      half8 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i] = m355_to_half(m355_silu(acc[t][i] * inv255 + bias[t][i]));
        o[4 + i] = m355_to_half(m355_silu(acc[t + 1][i] * inv255 + bias[t + 1][i]));
      }
      *(half8*)(yp + 32 * (t >> 1) + 8 * g) = o;
    }
    if (NT & 1) {
      constexpr int t = NT - 1;
      half4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = m355_to_half(m355_silu(acc[t][i] * inv255 + bias[t][i]));
      *(half4*)(yp + 16 * t + 4 * g) = o;
    }
  }
}

}  // namespace

bool stem6_ok(const Stem6Args& a) {
  return a.x && a.w && a.bias && a.y && a.B >= 1 && a.H >= 2 && a.W >= 16 && a.H % 2 == 0 && a.W % 16 == 0 &&
         (a.C0 == 16 || a.C0 == 32 || a.C0 == 48) && a.ldy >= a.C0 && a.ldy % 8 == 0 &&
         a.y_bstride >= (long)(a.H / 2) * (a.W / 2) * a.ldy && a.B <= 65535;
}

int launch_stem6(const Stem6Args& a, hipStream_t s) {
  if (!stem6_ok(a)) return -1;
  const dim3 grid((unsigned)((a.W / 2 + S6_TW - 1) / S6_TW), (unsigned)((a.H / 2 + S6_TH - 1) / S6_TH), (unsigned)a.B);
  switch (a.C0) {
    case 16: hipLaunchKernelGGL(stem6_s2_kernel<1>, grid, dim3(256), 0, s, a); break;
    case 32: hipLaunchKernelGGL(stem6_s2_kernel<2>, grid, dim3(256), 0, s, a); break;
    case 48: hipLaunchKernelGGL(stem6_s2_kernel<3>, grid, dim3(256), 0, s, a); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

// Host packing of (C0, 3, 6, 6) fp32 weights into the kernel's [C0 rows in MFMA order][128 k] fp16 matrix (k = (kh * 6 + kw) * 3 + c).
void pack_stem6_weights(const float* w, int C0, half_t* out) {
  const int NT = C0 / 16;
  for (int i = 0; i < C0 * 128; ++i) out[i] = (half_t)0.f;
  for (int t = 0; t < NT; ++t)
    for (int r = 0; r < 16; ++r) {
      const bool paired = (t ^ 1) < NT;
      const int co = paired ? 32 * (t >> 1) + 8 * (r >> 2) + 4 * (t & 1) + (r & 3) : 16 * t + r;
      for (int c = 0; c < 3; ++c)
        for (int kh = 0; kh < 6; ++kh)
          for (int kw = 0; kw < 6; ++kw)
            out[(t * 16 + r) * 128 + (kh * 6 + kw) * 3 + c] = (half_t)w[((co * 3 + c) * 6 + kh) * 6 + kw];
    }
}

}  // namespace m355
