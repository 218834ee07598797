// The rest of upstream's training augmentation chain on the GPU: rotation / shear / perspective
// (a full inverse homography per layer), flipud, mixup (two layers blended) and copy-paste (a per-layer list of polygons whose
// texels read the mirrored canvas), fused with what augment.hip does -- mosaic, bilinear warp with border 114, HSV gains,
// fliplr -- into ONE gather launch over the uint8 image cache in HBM.  m355_augment (augment.hip) stays the entry of the
// default options; this one runs when one of the six new options is on.
//
// Geometry of a layer as in augment.hip: a 2H x 2W canvas of four H x W sources around (xc, yc), or the single source at the
// origin.  Output pixel (x, y) -- after flip / flipud -- samples each layer's canvas at minv * (x, y, 1) / w bilinearly.  A
// canvas texel (cx, cy) that lies inside a polygon of the layer's paste list reads texel (Wc - 1 - cx, cy) instead: the
// left-right mirrored canvas shows through the polygon, which is upstream's CopyPaste in flip mode.  Inside is even-odd with
// the half-open crossing rule stated in include/mi355yolo.h, evaluated with products only.
//
// Work per pixel and layer: 4 source texels of 3 bytes in, 3 bytes out, like its parent: HBM- and cache-bound, plain loads and
// stores, no LDS.  An image is a grid row (blockIdx.y), so the parameter record, the polygon table and the vertices are read
// at wave-uniform addresses; a polygon's vertices are walked once for the four corners, and only by pixels whose 2 x 2
// footprint touches its bounding box.
//
// No FMA contraction anywhere in this file (Makefile: -ffp-contract=off): tests/augment_ex_ref.py restates the arithmetic in
// numpy float32, operation by operation, and the bytes are equal.
#include <algorithm>

#include "../../include/mi355yolo.h"
#include "common.h"

namespace m355 {
namespace {

constexpr int AX_THREADS = 256;
constexpr int AX_MAX_BLOCKS_X = 256;   // blocks per image; each walks the image with a grid stride
constexpr int AX_MAX_DIM = 16384;

// canvas texel (cx, cy) -> source image / texel, or the 114 border (augment.hip's fetch)
__device__ __forceinline__ void fetch(const uint8_t* cache, const m355_aug_layer& L, int H, int W, int cx, int cy, float* rgb) {
  int img = -1, sx = 0, sy = 0;
  if (!L.mosaic) {
    if ((unsigned)cx < (unsigned)W && (unsigned)cy < (unsigned)H) { img = L.src[0]; sx = cx; sy = cy; }
  } else if ((unsigned)cx < (unsigned)(2 * W) && (unsigned)cy < (unsigned)(2 * H)) {
    const int xc = (int)L.xc, yc = (int)L.yc;
    const int right = cx >= xc, down = cy >= yc;
    sx = right ? cx - xc : cx - (xc - W);
    sy = down ? cy - yc : cy - (yc - H);
    if ((unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H) img = L.src[down * 2 + right];
  }
  if (img < 0) {
    rgb[0] = rgb[1] = rgb[2] = 114.f;
    return;
  }
  const uint8_t* t = cache + (((long)img * H + sy) * W + sx) * 3;
  rgb[0] = (float)t[0]; rgb[1] = (float)t[1]; rgb[2] = (float)t[2];
}

// Bit k of the result: corner k of the footprint (x0 + (k & 1), y0 + (k >> 1)) is inside polygon q (bounding box, then even-odd).
__device__ __forceinline__ unsigned corners_inside(const m355_aug_poly& q, const float* verts, int x0, int y0) {
#pragma clang fp contract(off)
  unsigned box = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
    if (cx >= q.x0 && cx <= q.x1 && cy >= q.y0 && cy <= q.y1) box |= 1u << k;
  }
  if (!box) return 0;
  const float* v = verts + 2 * (long)q.vert_first;
  float ax = v[2 * (q.vert_count - 1)], ay = v[2 * (q.vert_count - 1) + 1];
  unsigned par = 0;
  for (int j = 0; j < q.vert_count; ++j) {
    const float bx = v[2 * j], by = v[2 * j + 1];
    const float d = by - ay, e = bx - ax;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float px = (float)(x0 + (k & 1)), py = (float)(y0 + (k >> 1));
      if ((ay > py) != (by > py)) {
        const float lhs = (px - ax) * d, rhs = (py - ay) * e;
        if (d > 0.f ? lhs < rhs : lhs > rhs) par ^= 1u << k;
      }
    }
    ax = bx; ay = by;
  }
  return par & box;
}

__device__ __forceinline__ void sample_layer(const uint8_t* cache, const m355_aug_layer& L, const m355_aug_poly* polys,
                                             const float* verts, int H, int W, float xs, float ys, float* rgb) {
#pragma clang fp contract(off)
  const int Wc = L.mosaic ? 2 * W : W, Hc = L.mosaic ? 2 * H : H;
  const float un = L.minv[0] * xs + L.minv[1] * ys + L.minv[2];
  const float vn = L.minv[3] * xs + L.minv[4] * ys + L.minv[5];
  const float wn = L.minv[6] * xs + L.minv[7] * ys + L.minv[8];
  // everything from -1 down and from Wc up is border: the clamp changes no byte and keeps the integer coordinates small
  // (fmaxf / fminf drop a NaN, so a vanishing w lands on the border too)
  const float u = fminf(fmaxf(un / wn, -2.f), (float)(Wc + 1));
  const float v = fminf(fmaxf(vn / wn, -2.f), (float)(Hc + 1));
  const float fu = floorf(u), fv = floorf(v);
  const int x0 = (int)fu, y0 = (int)fv;
  const float ax = u - fu, ay = v - fv;
  unsigned paste = 0;
  for (int k = 0; k < L.poly_count; ++k) {
    const m355_aug_poly q = polys[L.poly_first + k];
    if (x0 + 1 < q.x0 || x0 > q.x1 || y0 + 1 < q.y0 || y0 > q.y1) continue;
    paste |= corners_inside(q, verts, x0, y0);
  }
  float c[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
    fetch(cache, L, H, W, (paste >> k) & 1u ? Wc - 1 - cx : cx, cy, c[k]);
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    rgb[ch] = (c[0][ch] * (1.f - ax) + c[1][ch] * ax) * (1.f - ay) + (c[2][ch] * (1.f - ax) + c[3][ch] * ax) * ay;
}

__global__ __launch_bounds__(AX_THREADS) void augment_ex_kernel(const uint8_t* __restrict__ cache,
                                                                const m355_aug_ex_params* __restrict__ params,
                                                                const m355_aug_poly* __restrict__ polys,
                                                                const float* __restrict__ verts, uint8_t* __restrict__ out,
                                                                int H, int W) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const m355_aug_ex_params& p = params[b];
  const int hw = H * W;
  uint8_t* const img = out + (size_t)b * hw * 3;
  for (int i = blockIdx.x * AX_THREADS + threadIdx.x; i < hw; i += gridDim.x * AX_THREADS) {
    const int x = i % W, y = i / W;
    const float xs = (float)(p.flip ? W - 1 - x : x), ys = (float)(p.flipud ? H - 1 - y : y);
    float rgb[3];
    sample_layer(cache, p.layer[0], polys, verts, H, W, xs, ys, rgb);
    if (p.n_layers == 2) {   // mixup
      float other[3];
      sample_layer(cache, p.layer[1], polys, verts, H, W, xs, ys, other);
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = p.mix * rgb[c] + (1.f - p.mix) * other[c];
    }
    if (p.hgain != 1.f || p.sgain != 1.f || p.vgain != 1.f) {   // RGB -> HSV, gains, -> RGB (V in 0..255), as augment.hip
      const float mx = fmaxf(rgb[0], fmaxf(rgb[1], rgb[2])), mn = fminf(rgb[0], fminf(rgb[1], rgb[2]));
      const float d = mx - mn;
      float h = 0.f;
      if (d > 0.f) {
        if (mx == rgb[0]) h = (rgb[1] - rgb[2]) / d;
        else if (mx == rgb[1]) h = 2.f + (rgb[2] - rgb[0]) / d;
        else h = 4.f + (rgb[0] - rgb[1]) / d;
        h *= (1.f / 6.f);
        if (h < 0.f) h += 1.f;
      }
      float s = mx > 0.f ? d / mx : 0.f;
      h = h * p.hgain;
      h -= floorf(h);
      s = fminf(s * p.sgain, 1.f);
      const float val = fminf(mx * p.vgain, 255.f);
      const float hh = h * 6.f;
      const int sector = (int)hh;
      const float f = hh - (float)sector;
      const float pq = val * (1.f - s), q = val * (1.f - s * f), t = val * (1.f - s * (1.f - f));
      switch (sector % 6) {
        case 0: rgb[0] = val; rgb[1] = t; rgb[2] = pq; break;
        case 1: rgb[0] = q; rgb[1] = val; rgb[2] = pq; break;
        case 2: rgb[0] = pq; rgb[1] = val; rgb[2] = t; break;
        case 3: rgb[0] = pq; rgb[1] = q; rgb[2] = val; break;
        case 4: rgb[0] = t; rgb[1] = pq; rgb[2] = val; break;
        default: rgb[0] = val; rgb[1] = pq; rgb[2] = q; break;
      }
    }
    uint8_t* o = img + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)fminf(fmaxf(floorf(rgb[c] + 0.5f), 0.f), 255.f);
  }
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

size_t augment_ex_workspace_bytes(int B, int n_polys, int n_verts) {
  if (B < 0 || n_polys < 0 || n_verts < 0) return 0;
  return align16((size_t)B * sizeof(m355_aug_ex_params)) + align16((size_t)n_polys * sizeof(m355_aug_poly)) +
         align16((size_t)n_verts * 2 * sizeof(float));
}

int launch_augment_ex(const uint8_t* cache, int n_images, const void* h_params, const void* h_polys, int n_polys,
                      const float* h_verts, int n_verts, void* work, long long work_bytes, uint8_t* out, int B, int H, int W,
                      hipStream_t s) {
  // every argument is checked before the first HIP call
  const m355_aug_ex_params* const par = (const m355_aug_ex_params*)h_params;
  const m355_aug_poly* const pol = (const m355_aug_poly*)h_polys;
  if (!cache || !par || !work || !out || B < 1 || H < 1 || W < 1 || B > 65535 || H > AX_MAX_DIM || W > AX_MAX_DIM) return -1;
  if (n_images < 1 || n_polys < 0 || n_verts < 0 || (n_polys > 0 && !pol) || (n_verts > 0 && !h_verts)) return -1;
  if (((uintptr_t)work & 15) || work_bytes < 0 || (size_t)work_bytes < augment_ex_workspace_bytes(B, n_polys, n_verts)) return -1;
  for (int b = 0; b < B; ++b) {
    const m355_aug_ex_params& p = par[b];
    if (p.n_layers != 1 && p.n_layers != 2) return -1;
    for (int l = 0; l < p.n_layers; ++l) {
      const m355_aug_layer& L = p.layer[l];
      for (int k = 0; k < 4; ++k)
        if (L.src[k] < 0 || L.src[k] >= n_images) return -1;
      if (L.poly_count < 0 || L.poly_count > M355_AUG_MAX_PASTE || L.poly_first < 0 || L.poly_first > n_polys - L.poly_count)
        return -1;
    }
  }
  for (int k = 0; k < n_polys; ++k) {
    const m355_aug_poly& q = pol[k];
    if (q.vert_count < 1 || q.vert_count > M355_AUG_MAX_POLY_VERTS || q.vert_first < 0 || q.vert_first > n_verts - q.vert_count)
      return -1;
  }
  char* const w = (char*)work;
  const size_t off_polys = align16((size_t)B * sizeof(m355_aug_ex_params));
  const size_t off_verts = off_polys + align16((size_t)n_polys * sizeof(m355_aug_poly));
  hipError_t e = hipMemcpyAsync(w, par, (size_t)B * sizeof(m355_aug_ex_params), hipMemcpyHostToDevice, s);
  if (e == hipSuccess && n_polys > 0)
    e = hipMemcpyAsync(w + off_polys, pol, (size_t)n_polys * sizeof(m355_aug_poly), hipMemcpyHostToDevice, s);
  if (e == hipSuccess && n_verts > 0)
    e = hipMemcpyAsync(w + off_verts, h_verts, (size_t)n_verts * 2 * sizeof(float), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return (int)e;
  const int bx = std::min((H * W + AX_THREADS - 1) / AX_THREADS, AX_MAX_BLOCKS_X);
  hipLaunchKernelGGL(augment_ex_kernel, dim3((unsigned)bx, (unsigned)B), dim3(AX_THREADS), 0, s, cache,
                     (const m355_aug_ex_params*)w, (const m355_aug_poly*)(w + off_polys), (const float*)(w + off_verts), out, H, W);
  return (int)hipGetLastError();
}

}  // namespace m355
