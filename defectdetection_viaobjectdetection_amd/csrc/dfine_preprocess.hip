// Image pre-processing of a D-FINE / RT-DETR model (include/mi355yolo.h: m355_dfine_preprocess): T decoded
// uint8 RGB images of mixed sizes -> fp32 (T, 3, out_h, out_w), bit for bit RTDetrImageProcessorPil's resize (Pillow BILINEAR,
// 8-bit) + rescale, in two launches (gfx950).  Pillow's filter is separable and fixed-point: per axis the host builds xmin, count and
// int32 coefficients (2^22 scale) per output index; a pass is clip((2^21 + sum coef * pixel) >> 22) into uint8, horizontal first.
//
//   pre_h_kernel  a block stages PRE_ROWS consecutive source rows of one image in LDS (they are contiguous in memory: one run of
//                 16-byte loads from the aligned address below the first byte) and writes those rows resized to out_w into the
//                 uint8 scratch `mid`.  A lane owns 4 output pixels of each row -- 12 bytes, three 4-byte stores -- and reads a
//                 coefficient once for the 3 * PRE_ROWS products it feeds.  Images without a horizontal pass leave at once.
//   pre_v_kernel  a lane owns 4 consecutive output pixels of one output row: per tap it loads their 12 interleaved bytes (mid, or
//                 the source itself where the horizontal pass was skipped) as three words, accumulates 12 int32 sums, looks the 12
//                 bytes up in the rescale table (LDS) and writes one 16-byte store into each colour plane.  The lanes of a wave
//                 hold consecutive pixels of a row, so each store instruction covers consecutive addresses of one plane row.
//                 A skipped vertical pass is a copy of the row's bytes.
// All arithmetic is integer; the fp32 values come from the caller's 256-entry table.  The entry has validated every table.
#include "../../include/mi355yolo.h"
#include "common.h"

namespace m355 {
namespace {

constexpr int PRE_THREADS = 256;
constexpr int PRE_ROWS = 4;          // source rows per block of the horizontal pass
constexpr int PRE_HALF = 1 << 21;    // Pillow's rounding term, PRECISION_BITS = 22
constexpr int PRE_SHIFT = 22;

typedef unsigned uint4v __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned clip8(int acc) { return (unsigned)min(acc >> PRE_SHIFT, 255); }   // coefficients are >= 0

__global__ __launch_bounds__(PRE_THREADS) void dfine_pre_h_kernel(const uint8_t* __restrict__ src,
                                                                  const m355_dfine_pre_image* __restrict__ images,
                                                                  const m355_dfine_pre_axis* __restrict__ axes,
                                                                  const int* __restrict__ pool, uint8_t* __restrict__ mid, int out_w) {
  extern __shared__ uint4v pre_rows[];
  const m355_dfine_pre_image im = images[blockIdx.y];
  const int y0 = blockIdx.x * PRE_ROWS;
  if (im.htab < 0 || y0 >= im.in_h) return;
  const int rows = min(PRE_ROWS, im.in_h - y0);
  const int rb = 3 * im.in_w;
  const long long first = im.offset + (long long)y0 * rb;
  const int lead = (int)(first & 15);
  const uint4v* const from = (const uint4v*)(src + (first - lead));
  const int n16 = (lead + rows * rb + 15) >> 4;   // ends inside src: src_bytes is a multiple of 16
  for (int i = threadIdx.x; i < n16; i += PRE_THREADS) pre_rows[i] = from[i];
  __syncthreads();
  const uint8_t* const row0 = (const uint8_t*)pre_rows + lead;

  const m355_dfine_pre_axis ax = axes[im.htab];
  const int* const xmin = pool + ax.offset;
  const int* const count = xmin + out_w;
  const int* const coef = count + out_w;
  uint8_t* const dst = mid + ((size_t)im.mid_row + y0) * out_w * 3;
  for (int q = threadIdx.x; q < out_w / 4; q += PRE_THREADS) {
    unsigned o[PRE_ROWS][3];
#pragma unroll
    for (int r = 0; r < PRE_ROWS; ++r) o[r][0] = o[r][1] = o[r][2] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xx = 4 * q + j;
      const int n = count[xx];
      const int* const k = coef + (size_t)xx * ax.ksize;
      const uint8_t* p = row0 + 3 * xmin[xx];
      int acc[PRE_ROWS][3];
#pragma unroll
      for (int r = 0; r < PRE_ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = PRE_HALF;
      for (int t = 0; t < n; ++t, p += 3) {
        const int c = k[t];
        // rows past the image's last (r >= rows) read bytes of the allocation nobody wrote; their sums are never stored
#pragma unroll
        for (int r = 0; r < PRE_ROWS; ++r)
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) acc[r][ch] += c * (int)p[r * rb + ch];
      }
#pragma unroll
      for (int r = 0; r < PRE_ROWS; ++r)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int byte = 3 * j + ch;
          o[r][byte >> 2] |= clip8(acc[r][ch]) << (8 * (byte & 3));
        }
    }
#pragma unroll
    for (int r = 0; r < PRE_ROWS; ++r)
      if (r < rows) {
        unsigned* const d = (unsigned*)(dst + (size_t)r * out_w * 3) + 3 * q;
        d[0] = o[r][0]; d[1] = o[r][1]; d[2] = o[r][2];
      }
  }
}

__global__ __launch_bounds__(PRE_THREADS) void dfine_pre_v_kernel(const uint8_t* __restrict__ src,
                                                                  const m355_dfine_pre_image* __restrict__ images,
                                                                  const m355_dfine_pre_axis* __restrict__ axes,
                                                                  const int* __restrict__ pool, const uint8_t* __restrict__ mid,
                                                                  const float* __restrict__ rescale, float* __restrict__ out,
                                                                  int out_h, int out_w) {
  __shared__ float value_of[256];
  value_of[threadIdx.x] = rescale[threadIdx.x];   // PRE_THREADS == 256
  __syncthreads();
  const int quads = out_w / 4;
  const int item = blockIdx.x * PRE_THREADS + threadIdx.x;
  if (item >= out_h * quads) return;
  const int y = item / quads, q = item - y * quads;
  const m355_dfine_pre_image im = images[blockIdx.y];
  const size_t rb = (size_t)out_w * 3;   // both sources have rows of out_w pixels
  const uint8_t* const base = (im.htab >= 0 ? mid + (size_t)im.mid_row * rb : src + im.offset) + 12 * q;

  unsigned v[12];
  if (im.vtab < 0) {
    const unsigned* const w = (const unsigned*)(base + (size_t)y * rb);
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = (w0 >> (8 * i)) & 255u;
      v[4 + i] = (w1 >> (8 * i)) & 255u;
      v[8 + i] = (w2 >> (8 * i)) & 255u;
    }
  } else {
    const m355_dfine_pre_axis ax = axes[im.vtab];
    const int* const tab = pool + ax.offset;
    const int y_first = tab[y], n = tab[out_h + y];
    const int* const k = tab + 2 * (size_t)out_h + (size_t)y * ax.ksize;
    int acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = PRE_HALF;
    const uint8_t* p = base + (size_t)y_first * rb;
    for (int t = 0; t < n; ++t, p += rb) {
      const int c = k[t];
      const unsigned* const w = (const unsigned*)p;
      const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[i] += c * (int)((w0 >> (8 * i)) & 255u);
        acc[4 + i] += c * (int)((w1 >> (8 * i)) & 255u);
        acc[8 + i] += c * (int)((w2 >> (8 * i)) & 255u);
      }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = clip8(acc[i]);
  }
  float* const o = out + (((size_t)blockIdx.y * 3) * out_h + y) * out_w + 4 * q;
  const size_t plane = (size_t)out_h * out_w;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    *(float4v*)(o + ch * plane) = float4v{value_of[v[ch]], value_of[v[3 + ch]], value_of[v[6 + ch]], value_of[v[9 + ch]]};
}

}  // namespace

size_t dfine_preprocess_lds_bytes(int max_in_w) { return ((size_t)PRE_ROWS * 3 * max_in_w + 15 + 15) / 16 * 16; }

int launch_dfine_preprocess(const uint8_t* src, const void* d_images, int T, const void* d_axes, const int* d_pool,
                            const float* rescale, int out_h, int out_w, uint8_t* mid, int h_max_rows, int h_max_w, float* out,
                            hipStream_t s) {
  const m355_dfine_pre_image* const images = (const m355_dfine_pre_image*)d_images;
  const m355_dfine_pre_axis* const axes = (const m355_dfine_pre_axis*)d_axes;
  if (h_max_rows > 0) {
    hipLaunchKernelGGL(dfine_pre_h_kernel, dim3((h_max_rows + PRE_ROWS - 1) / PRE_ROWS, T), dim3(PRE_THREADS),
                       dfine_preprocess_lds_bytes(h_max_w), s, src, images, axes, d_pool, mid, out_w);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  const int items = out_h * (out_w / 4);
  hipLaunchKernelGGL(dfine_pre_v_kernel, dim3((items + PRE_THREADS - 1) / PRE_THREADS, T), dim3(PRE_THREADS), 0, s, src, images, axes,
                     d_pool, mid, rescale, out, out_h, out_w);
  return (int)hipGetLastError();
}

}  // namespace m355
