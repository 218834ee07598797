// Device-side LetterBox: raw decoded BGR images of mixed sizes -> the engine's input batch, uint8 NHWC RGB,
// in one launch per 32 images (gfx950).  For image b with source (h, w, 3) and geometry (uh, uw, top, left):
//   out[b, y, x, c] = 114                                      outside [top, top + uh) x [left, left + uw)
//   out[b, y, x, c] = resize(src_b)[y - top, x - left, 2 - c]  inside
// resize is preprocess.resize_linear_u8 restated operation by operation in IEEE double with contraction off, so the bytes are
// the host function's bytes: coordinate (i + 0.5) * s - 0.5 with s = h / uh formed on the host, floor,
// weight = coordinate - floor, taps clamped to the image, p00 * (1 - wx) + p01 * wx for the two rows, the same blend down the
// column, floor(v + 0.5), clip.  Where (h, w) == (uh, uw) the host copies; so does the kernel.
//
// The op moves bytes (at most 4 source bytes read per byte written).  A lane owns a run of LB_RUN = 16 consecutive output
// pixels of a row -- 48 bytes, three aligned 16-byte stores, an output row being 3 * net_w bytes with net_w % 32 == 0 -- and
// walks a band of LB_BAND rows down it: the clamped x taps and x weights of the run are formed once and stay in registers.
// The lanes of a wave hold consecutive runs of one row, so a wave's stores cover a contiguous stretch and its source reads
// fall on the same few lines of two source rows; those go through the cache, no LDS.  The per-image table travels in the
// kernel arguments.
#include <algorithm>

#include "../../include/mi355yolo.h"
#include "common.h"

namespace m355 {
namespace {

constexpr int LB_THREADS = 256;
constexpr int LB_RUN = 16;        // output pixels per lane and row
constexpr int LB_BAND = 8;        // output rows per lane
constexpr int LB_MAX_IMGS = 32;   // images per launch
constexpr int LB_PAD = 114;
constexpr int LB_MAX_DIM = 32768;   // source and network height / width (a source row is < 2^17 bytes)

struct LbTable {
  long long off[LB_MAX_IMGS];                       // byte offset of the image in src
  double sy[LB_MAX_IMGS], sx[LB_MAX_IMGS];          // h / uh, w / uw
  int h[LB_MAX_IMGS], w[LB_MAX_IMGS], uh[LB_MAX_IMGS], uw[LB_MAX_IMGS], top[LB_MAX_IMGS], left[LB_MAX_IMGS];
};

typedef unsigned uint4v __attribute__((ext_vector_type(4)));

// Source taps and weight of output index i along an axis of n source pixels at scale s (resize_linear_u8's yy, y0, wy, y0c, y1c).
__device__ __forceinline__ void taps(int i, double s, int n, int& i0, int& i1, double& f) {
#pragma clang fp contract(off)
  const double c = ((double)i + 0.5) * s - 0.5;
  const double fl = floor(c);
  f = c - fl;
  const int k = (int)fl;
  i0 = min(max(k, 0), n - 1);
  i1 = min(max(k + 1, 0), n - 1);
}

__global__ __launch_bounds__(LB_THREADS) void letterbox_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out,
                                                               int net_h, int net_w, LbTable t) {
#pragma clang fp contract(off)
  const int runs = net_w / LB_RUN;
  const int lane = blockIdx.x * LB_THREADS + threadIdx.x;
  const int band = lane / runs;
  if (band * LB_BAND >= net_h) return;
  const int b = blockIdx.y;
  const int x_base = (lane - band * runs) * LB_RUN;
  const int h = t.h[b], w = t.w[b], uh = t.uh[b], uw = t.uw[b], top = t.top[b], left = t.left[b];
  const bool copy = h == uh && w == uw;
  const double sy = t.sy[b], sx = t.sx[b];

  // the run's x taps (byte offsets within a source row) and weights
  int xa[LB_RUN], xb[LB_RUN];
  double wx[LB_RUN];
  unsigned inside = 0;
#pragma unroll
  for (int j = 0; j < LB_RUN; ++j) {
    const int x = x_base + j - left;
    xa[j] = xb[j] = 0;
    wx[j] = 0.0;
    if (x >= 0 && x < uw) {
      inside |= 1u << j;
      if (copy) {
        xa[j] = 3 * x;
      } else {
        int x0, x1;
        taps(x, sx, w, x0, x1, wx[j]);
        xa[j] = 3 * x0;
        xb[j] = 3 * x1;
      }
    }
  }

  const uint8_t* const img = src + t.off[b];
  uint8_t* const orow = out + ((size_t)b * net_h + (size_t)band * LB_BAND) * net_w * 3 + (size_t)x_base * 3;
  const unsigned pad4 = LB_PAD * 0x01010101u;
#pragma unroll 1
  for (int r = 0; r < LB_BAND; ++r) {
    const int y = band * LB_BAND + r - top;
    unsigned o[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = pad4;
    if (inside && y >= 0 && y < uh) {
      int y0 = y, y1 = y;
      double wy = 0.0;
      if (!copy) taps(y, sy, h, y0, y1, wy);
      const uint8_t* const r0 = img + (size_t)y0 * w * 3;
      const uint8_t* const r1 = img + (size_t)y1 * w * 3;
#pragma unroll
      for (int k = 0; k < 12; ++k) o[k] = 0u;
#pragma unroll
      for (int j = 0; j < LB_RUN; ++j) {
        const bool in = (inside >> j) & 1u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          unsigned v = LB_PAD;
          if (in) {
            if (copy) {
              v = r0[xa[j] + 2 - c];
            } else {
              const double p00 = (double)r0[xa[j] + 2 - c], p01 = (double)r0[xb[j] + 2 - c];
              const double p10 = (double)r1[xa[j] + 2 - c], p11 = (double)r1[xb[j] + 2 - c];
              const double omx = 1.0 - wx[j];
              const double tp = p00 * omx + p01 * wx[j];
              const double bt = p10 * omx + p11 * wx[j];
              const double val = tp * (1.0 - wy) + bt * wy;
              const double rq = fmin(fmax(floor(val + 0.5), 0.0), 255.0);
              v = (unsigned)(int)rq;
            }
          }
          const int byte = 3 * j + c;
          o[byte >> 2] |= v << (8 * (byte & 3));
        }
      }
    }
    uint4v* const dst = (uint4v*)(orow + (size_t)r * net_w * 3);
    dst[0] = uint4v{o[0], o[1], o[2], o[3]};
    dst[1] = uint4v{o[4], o[5], o[6], o[7]};
    dst[2] = uint4v{o[8], o[9], o[10], o[11]};
  }
}

}  // namespace

int launch_letterbox_u8(const uint8_t* src, const void* table, int n, int net_h, int net_w, uint8_t* out,
                        hipStream_t s) {
  // every argument is checked before the first launch
  const m355_letterbox_image* const tab = (const m355_letterbox_image*)table;
  if (!src || !tab || !out || n < 1 || net_h < 32 || net_w < 32 || net_h % 32 || net_w % 32) return -1;
  if (net_h > LB_MAX_DIM || net_w > LB_MAX_DIM || ((uintptr_t)out & 15)) return -1;
  long long end = 0;   // first byte past the previous image
  for (int i = 0; i < n; ++i) {
    const m355_letterbox_image& e = tab[i];
    if (e.h < 1 || e.w < 1 || e.uh < 1 || e.uw < 1 || e.h > LB_MAX_DIM || e.w > LB_MAX_DIM) return -1;
    if (e.top < 0 || e.left < 0 || e.top > net_h - e.uh || e.left > net_w - e.uw) return -1;   // the window leaves the frame
    if (e.offset < end) return -1;                                                             // overlapping or misordered
    end = e.offset + 3LL * e.h * e.w;
  }
  const int lanes = (net_h / LB_BAND) * (net_w / LB_RUN);
  for (int g0 = 0; g0 < n; g0 += LB_MAX_IMGS) {
    LbTable t{};
    const int m = std::min(LB_MAX_IMGS, n - g0);
    for (int i = 0; i < m; ++i) {
      const m355_letterbox_image& e = tab[g0 + i];
      t.off[i] = e.offset;
      t.h[i] = e.h; t.w[i] = e.w; t.uh[i] = e.uh; t.uw[i] = e.uw; t.top[i] = e.top; t.left[i] = e.left;
      t.sy[i] = (double)e.h / (double)e.uh;
      t.sx[i] = (double)e.w / (double)e.uw;
    }
    hipLaunchKernelGGL(letterbox_kernel, dim3((lanes + LB_THREADS - 1) / LB_THREADS, m), dim3(LB_THREADS), 0, s, src,
                       out + (size_t)g0 * net_h * net_w * 3, net_h, net_w, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // namespace m355
