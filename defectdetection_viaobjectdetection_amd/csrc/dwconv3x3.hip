// Depthwise 3x3 convolution, stride 1, pad 1 (YOLO11: the Detect class branch's DWConv and the attention's positional term)
// on fp16 NHWC channel slices (gfx950).
//   y[b, i, j, c] = act(bias[c] + sum_{dy, dx} w[dy][dx][c] * x[b, i + dy - 1, j + dx - 1, c]),  act = SiLU or none
// Rounding points: fp16 operands (weights packed to fp16 on the host), fp32 sums, + the folded BN bias in fp32, SiLU, one
// rounding to fp16.
//
// The op is memory-bound (9 MACs per 4 bytes moved), so the layout serves the bytes: a lane owns 8 consecutive channels of one
// output column and walks a band of DW_R rows down it, keeping a 3 x 3 window of 16-byte vectors in registers.  Each step loads
// the one new input row (3 vectors: columns j - 1, j, j + 1) and stores one 16-byte output vector, so an input row band with its
// halo is read from memory once: the lanes of a wave cover consecutive channel groups, then consecutive columns, and the column
// neighbours' vectors are the same cache lines as the lane's own.  Pixels outside the image read as zeros (the padding).
// Slices: x, y point at the first channel of their slice; ldx / ldy are the buffers' pixel strides (multiples of 8).
#include <stdio.h>

#include "common.h"
#include "device_prims.h"

namespace m355 {
namespace {

constexpr int DW_R = 8;          // output rows per lane (band height)
constexpr int DW_THREADS = 256;

template <bool ACT>
__global__ __launch_bounds__(DW_THREADS) void dwconv3x3_kernel(DwConvArgs a, int groups, int nbands, long total) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * DW_THREADS + threadIdx.x;
  if (t >= total) return;
  const int cg = (int)(t % groups);
  long r = t / groups;
  const int j = (int)(r % a.W);
  r /= a.W;
  const int band = (int)(r % nbands);
  const int b = (int)(r / nbands);
  const int c0 = 8 * cg;

  half8 w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = *(const half8*)(a.w + (long)k * a.C + c0);
  float bias[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bias[e] = a.bias[c0 + e];

  const half_t* xb = a.x + (long)b * a.x_bstride + c0;
  const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  auto load_row = [&](int i, half8 (&row)[3]) {
    const bool rin = i >= 0 && i < a.H;
    const half_t* p = xb + ((long)i * a.W + j) * a.ldx;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int jj = j + dx - 1;
      row[dx] = (rin && jj >= 0 && jj < a.W) ? *(const half8*)(p + (long)(dx - 1) * a.ldx) : zero8;
    }
  };
  const int i0 = band * DW_R;
  half8 win[3][3];
  load_row(i0 - 1, win[0]);
  load_row(i0, win[1]);
  half_t* yb = a.y + (long)b * a.y_bstride + c0;
#pragma unroll 1
  for (int s = 0; s < DW_R; ++s) {
    const int i = i0 + s;
    if (i >= a.H) break;
    load_row(i + 1, win[2]);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf((float)w[dy * 3 + dx][e], (float)win[dy][dx][e], acc[e]);
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = acc[e] + bias[e];
      if (ACT) v = m355_silu(v);
      o[e] = m355_to_half(v);
    }
    *(half8*)(yb + ((long)i * a.W + j) * a.ldy) = o;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      win[0][dx] = win[1][dx];
      win[1][dx] = win[2][dx];
    }
  }
}

}  // namespace

bool dwconv3x3_ok(const DwConvArgs& a) {
  if (!a.x || !a.w || !a.bias || !a.y) return false;
  if (a.B < 1 || a.H < 1 || a.W < 1 || a.C < 8 || a.C % 8) return false;
  if (a.ldx < a.C || a.ldy < a.C || a.ldx % 8 || a.ldy % 8) return false;
  if (((uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.w) & 15) return false;
  if (a.x_bstride < ((long)a.H * a.W - 1) * a.ldx + a.C || a.y_bstride < ((long)a.H * a.W - 1) * a.ldy + a.C) return false;
  const long total = (long)a.B * ((a.H + DW_R - 1) / DW_R) * a.W * (a.C / 8);
  return (total + DW_THREADS - 1) / DW_THREADS < (1L << 31);
}

int launch_dwconv3x3(const DwConvArgs& a, hipStream_t s) {
  if (!dwconv3x3_ok(a)) return -1;
  const int groups = a.C / 8, nbands = (a.H + DW_R - 1) / DW_R;
  const long total = (long)a.B * nbands * a.W * groups;
  const dim3 grid((unsigned)((total + DW_THREADS - 1) / DW_THREADS));
  if (a.act)
    hipLaunchKernelGGL(dwconv3x3_kernel<true>, grid, dim3(DW_THREADS), 0, s, a, groups, nbands, total);
  else
    hipLaunchKernelGGL(dwconv3x3_kernel<false>, grid, dim3(DW_THREADS), 0, s, a, groups, nbands, total);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// (C, 1, 3, 3) fp32 -> [9][C] fp16: tap k = dy * 3 + dx, channel-contiguous (one 16-byte load per tap and lane)
void pack_dw3x3_weights(const float* w, int C, half_t* out) {
  for (int c = 0; c < C; ++c)
    for (int k = 0; k < 9; ++k) out[(size_t)k * C + c] = (half_t)w[(size_t)c * 9 + k];
}

}  // namespace m355
