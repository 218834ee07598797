// Native-resolution masks: upstream utils.ops.process_mask_native (predict(retina_masks=True)) for every detection of a batch
// in one launch.  For one detection with coefficients c (32), prototypes P (mh, mw, 32) fp16 NHWC, original shape (h0, w0)
// and box (x1, y1, x2, y2) in original pixels (the fp32 boxes Results.boxes reports):
//   1. the prototype grid is cropped to the letterboxed image (native_mask_crop: the rule lives there and nowhere else);
//   2. logit(cell) = sum_k c_k P[cell, k] in fp32;
//   3. bilinear interpolation of the cropped logits to (h0, w0), F.interpolate(align_corners=False): source coordinate
//      (y + 0.5) * ch / h0 - 0.5 clamped at 0, upper neighbour clamped to the last row / column;
//   4. pixel (r, q) is kept iff x1 <= q < x2 and y1 <= r < y2, everything else is 0;
//   5. out = uint8(logit > 0).
// The source coordinate is formed exactly in integers: (2y + 1) * ch - h0 over 2 h0, so the interpolation weight is one fp32
// rounding of an exact fraction.
//
// One 256-thread block per (detection slot, band of output rows).  The block computes the logits of the prototype cells under
// its band's part of the box (plus the 1-cell interpolation halo) ONCE into LDS -- at most WIN_ROWS rows of the crop's width --
// and then walks the band's bytes as 16-byte chunks aligned in memory: a chunk with no pixel in the box is a zero store that
// waits on nothing but the box; a chunk that touches the box interpolates its 16 pixels from LDS.  Masks are written once and
// only copied to the host afterwards: non-temporal stores.
#include <algorithm>

#include "common.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int NT_THREADS = 256;
constexpr int MAX_IMGS = 32;       // images per launch: the per-image table travels in the kernel arguments
constexpr int WIN_ROWS = 16;       // prototype rows of one block's logit window (LDS = WIN_ROWS x crop width x 4 bytes)
constexpr int MAX_BAND = 64;       // output rows per block
constexpr int MAX_PROTO = 512;     // prototype grid height / width (network input <= 2048)
constexpr int MAX_ORIG = 32768;    // original height / width

struct NativeTable {
  int nimg;
  int h0[MAX_IMGS], w0[MAX_IMGS];
  int top[MAX_IMGS], left[MAX_IMGS], ch[MAX_IMGS], cw[MAX_IMGS];   // crop of the prototype grid
  int band[MAX_IMGS], nbands[MAX_IMGS];                            // output rows per block, blocks per detection slot
  int blk0[MAX_IMGS + 1];                                          // first block of each image
  long long off[MAX_IMGS];                                         // byte offset of the image's first mask in out
};

// q = n / d and r = n % d for 0 <= n < 2^31, 0 < d: a float-reciprocal estimate, off by at most one for the quotients here
// (< 2^16), corrected once either way.
__device__ __forceinline__ int divmod(int n, int d, float rcp, int& r) {
  int q = (int)((float)n * rcp);
  r = n - q * d;
  if (r < 0) { --q; r += d; }
  else if (r >= d) { ++q; r -= d; }
  return q;
}

// Source cell and weight of output index p along an axis of c cropped cells and o output pixels (align_corners=False).
__device__ __forceinline__ int src_index(int p, int c, int o, float rcp2o, float& f) {
  const int n = (2 * p + 1) * c - o;    // 2 o * source coordinate
  if (n <= 0) { f = 0.f; return 0; }    // clamped at 0
  int rem;
  const int i0 = divmod(n, 2 * o, rcp2o, rem);
  f = (float)rem * rcp2o;
  return i0;
}

__global__ __launch_bounds__(NT_THREADS) void proto_masks_native_kernel(const float* dets, const int* counts,
                                                                        const half_t* protos, int max_det, int mh, int mw,
                                                                        const float* boxes, uint8_t* out, NativeTable t) {
  extern __shared__ __attribute__((aligned(16))) float lg[];   // [WIN_ROWS][nw] logits of the block's window
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;
  int b = 0;
  while (b + 1 < t.nimg && blk >= t.blk0[b + 1]) ++b;
  const int h0 = t.h0[b], w0 = t.w0[b], ch = t.ch[b], cw = t.cw[b];
  const int local = blk - t.blk0[b];
  const int d = local / t.nbands[b];
  const int r_beg = (local - d * t.nbands[b]) * t.band[b];
  const int r_end = min(h0, r_beg + t.band[b]);
  int n = counts[b];
  n = n < 0 ? 0 : (n > max_det ? max_det : n);

  // 4. box -> integer pixel ranges: x1 <= q < x2  <=>  ceil(x1) <= q < ceil(x2).  Slots past the count are all zeros.
  int qa = 0, qb = 0, ya = 0, yb = 0;
  if (d < n) {
    const float* bx = boxes + ((long)b * max_det + d) * 4;
    qa = (int)fminf(fmaxf(ceilf(bx[0]), 0.f), (float)w0);
    ya = (int)fminf(fmaxf(ceilf(bx[1]), 0.f), (float)h0);
    qb = (int)fminf(fmaxf(ceilf(bx[2]), 0.f), (float)w0);
    yb = (int)fminf(fmaxf(ceilf(bx[3]), 0.f), (float)h0);
  }
  ya = max(ya, r_beg);
  yb = min(yb, r_end);
  const bool has = ya < yb && qa < qb;
  const float rcp_h = 1.f / (float)(2 * h0), rcp_w = 1.f / (float)(2 * w0), rcp_w0 = 1.f / (float)w0;

  // 2. logits of the window: rows [wy0, wy0 + nr) x cols [wx0, wx0 + nw) of the crop
  int wy0 = 0, wx0 = 0, nw = 1;
  if (has) {
    float f;
    wy0 = src_index(ya, ch, h0, rcp_h, f);
    const int wy1 = min(src_index(yb - 1, ch, h0, rcp_h, f) + 1, ch - 1);
    wx0 = src_index(qa, cw, w0, rcp_w, f);
    const int wx1 = min(src_index(qb - 1, cw, w0, rcp_w, f) + 1, cw - 1);
    const int nr = min(wy1 - wy0 + 1, WIN_ROWS);   // (<= WIN_ROWS by the launcher's choice of band)
    nw = wx1 - wx0 + 1;
    const float* cp = dets + ((long)b * max_det + d) * 38 + 6;
    float c[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) c[k] = cp[k];
    const half_t* pb = protos + ((long)b * mh + t.top[b] + wy0) * mw * 32 + (long)(t.left[b] + wx0) * 32;
    for (int i = tid; i < nr * nw; i += NT_THREADS) {
      const int rr = i / nw, cc = i - rr * nw;
      const half_t* pp = pb + ((long)rr * mw + cc) * 32;
      float acc = 0.f;
#pragma unroll
      for (int k8 = 0; k8 < 4; ++k8) {
        const half8 v = *(const half8*)(pp + k8 * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf(c[k8 * 8 + j], (float)v[j], acc);
      }
      lg[rr * nw + cc] = acc;
    }
  }
  __syncthreads();

  // 3-5. the band's bytes [f0, f1) of the detection's plane, in 16-byte chunks aligned in memory
  typedef unsigned uint4v __attribute__((ext_vector_type(4)));
  uint8_t* const plane = out + t.off[b] + (long)d * h0 * w0;
  const int f0 = r_beg * w0, f1 = r_end * w0;
  uint8_t* const c0p = (uint8_t*)((uintptr_t)(plane + f0) & ~(uintptr_t)15);
  const long fc0 = (long)(c0p - plane);                 // flat index of chunk 0's first byte (<= f0)
  const int nchunks = (int)((f1 - fc0 + 15) >> 4);
  for (int k = tid; k < nchunks; k += NT_THREADS) {
    const long fs = fc0 + 16L * k;
    const int jb = fs < f0 ? (int)(f0 - fs) : 0;        // bytes [jb, je) of the chunk belong to this band
    const int je = fs + 16 > f1 ? (int)(f1 - fs) : 16;
    uint8_t* const dst = plane + fs;
    int q, ql;
    const int r = divmod((int)fs + jb, w0, rcp_w0, q);
    const int rl = divmod((int)fs + je - 1, w0, rcp_w0, ql);
    const bool zero = !has || rl < ya || r >= yb || (r == rl && (ql < qa || q >= qb));
    uint4v o = {0u, 0u, 0u, 0u};
    if (!zero) {
      int rr = r, qq = q;
      bool in_row = false;
      int l0 = 0, l1 = 0;
      float fy = 0.f;
      auto row = [&]() __attribute__((always_inline)) {
        in_row = rr >= ya && rr < yb;
        if (in_row) {
          const int y0 = src_index(rr, ch, h0, rcp_h, fy);
          const int y1 = min(y0 + 1, ch - 1);
          l0 = (y0 - wy0) * nw;
          l1 = (y1 - wy0) * nw;
        }
      };
      row();
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (j >= jb && j < je) {
          if (in_row && qq >= qa && qq < qb) {
            float fx;
            const int x0 = src_index(qq, cw, w0, rcp_w, fx);
            const int x1 = min(x0 + 1, cw - 1);
            const int a0 = x0 - wx0, a1 = x1 - wx0;
            const float top = (1.f - fx) * lg[l0 + a0] + fx * lg[l0 + a1];
            const float bot = (1.f - fx) * lg[l1 + a0] + fx * lg[l1 + a1];
            const float v = (1.f - fy) * top + fy * bot;
            if (v > 0.f) o[j >> 2] |= 1u << (8 * (j & 3));
          }
          if (++qq == w0) {
            qq = 0;
            ++rr;
            row();
          }
        }
      }
    }
    if (jb == 0 && je == 16) {
      __builtin_nontemporal_store(o, (uint4v*)dst);
    } else {
      for (int j = jb; j < je; ++j) dst[j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
    }
  }
}

}  // namespace

void native_mask_crop(int mh, int mw, int h0, int w0, int* top, int* left, int* ch, int* cw) {
  // scale_masks(padding=True) of Ultralytics 8.x as recalled ([U]): the pad in prototype cells,
  // truncated; other releases round as round(pad -/+ 0.1).  tests/native_mask_ref.py restates this rule.
  const double gain = std::min((double)mh / h0, (double)mw / w0);
  const double pw = (mw - w0 * gain) / 2, ph = (mh - h0 * gain) / 2;
  *top = (int)ph;
  *left = (int)pw;
  *ch = (int)(mh - ph) - *top;
  *cw = (int)(mw - pw) - *left;
}

int launch_proto_masks_native(const float* dets, const int* counts, const half_t* protos, int B, int max_det, int mh,
                              int mw, const int* h_orig_hw, const float* boxes, const int64_t* h_offsets, uint8_t* out,
                              hipStream_t s) {
  // every argument is checked before the first launch
  if (B < 1 || max_det < 1 || max_det > 1024 || mh < 1 || mw < 1 || mh > MAX_PROTO || mw > MAX_PROTO) return -1;
  if (!dets || !counts || !protos || !boxes || !h_orig_hw || !h_offsets || ((uintptr_t)protos & 15)) return -1;
  if (h_offsets[0] < 0) return -1;
  for (int b = 0; b < B; ++b) {
    const int h0 = h_orig_hw[2 * b], w0 = h_orig_hw[2 * b + 1];
    if (h0 < 1 || w0 < 1 || h0 > MAX_ORIG || w0 > MAX_ORIG) return -1;   // (so a plane's flat index fits an int)
    int top, left, ch, cw;
    native_mask_crop(mh, mw, h0, w0, &top, &left, &ch, &cw);
    if (ch < 1 || cw < 1) return -1;
    const long long cap = h_offsets[b + 1] - h_offsets[b], plane = (long long)h0 * w0;
    if (cap < 0 || cap % plane || cap / plane > max_det) return -1;   // monotone, whole planes, at most max_det of them
  }
  if (h_offsets[B] > 0 && !out) return -1;
  const size_t lds_max = (size_t)WIN_ROWS * MAX_PROTO * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    if (const int e = prepare_kernel((const void*)proto_masks_native_kernel, (int)lds_max)) return e;
    attr_set = true;
  }
  for (int g0 = 0; g0 < B; g0 += MAX_IMGS) {
    NativeTable t{};
    t.nimg = std::min(MAX_IMGS, B - g0);
    int blocks = 0, maxw = 1;
    for (int i = 0; i < t.nimg; ++i) {
      const int b = g0 + i;
      const int h0 = h_orig_hw[2 * b], w0 = h_orig_hw[2 * b + 1];
      t.h0[i] = h0;
      t.w0[i] = w0;
      native_mask_crop(mh, mw, h0, w0, &t.top[i], &t.left[i], &t.ch[i], &t.cw[i]);
      // rows of the logit window of `band` output rows: at most ceil((band - 1) ch / h0) + 2
      int band = 1;
      while (band < MAX_BAND && ((long long)band * t.ch[i] + h0 - 1) / h0 + 2 <= WIN_ROWS) ++band;
      t.band[i] = band;
      t.nbands[i] = (h0 + band - 1) / band;
      t.off[i] = h_offsets[b];
      const int slots = (int)((h_offsets[b + 1] - h_offsets[b]) / ((long long)h0 * w0));
      t.blk0[i] = blocks;
      blocks += slots * t.nbands[i];
      if (slots) maxw = std::max(maxw, t.cw[i]);
    }
    t.blk0[t.nimg] = blocks;
    if (!blocks) continue;
    const size_t lds = (size_t)WIN_ROWS * maxw * sizeof(float);
    hipLaunchKernelGGL(proto_masks_native_kernel, dim3(blocks), dim3(NT_THREADS), lds, s,
                       dets + (long)g0 * max_det * 38, counts + g0, protos + (long)g0 * mh * mw * 32, max_det, mh, mw,
                       boxes + (long)g0 * max_det * 4, out, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // namespace m355
