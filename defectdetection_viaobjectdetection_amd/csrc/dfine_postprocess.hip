// D-FINE / RT-DETR detection post-processing on the device (transformers' RTDetrImageProcessor.post_process_object_detection,
// models/rt_detr/image_processing_rt_detr.py:482-552, focal branch), which the reference's predict and eval scripts call once per
// frame: sigmoid, top-K over the Q*C flattened scores (K = Q), label / query from the flat index, cxcywh -> xyxy, scale by the
// image size, and the count of rows above the threshold.
//
// One block per image.  Every candidate i = q*C + c gets the order key of its logit; the K = Q greatest in the total order
// (NaN first, descending logit, -0 == +0, an exact tie to the lowest flat index) come from the block-wide selection of
// topk_select.h.  Its histogram's integer atomics only count: no output bit depends on scheduling, and an image's result does not
// depend on the other images of the batch.
// This file is compiled with -ffp-contract=off: the box arithmetic is upstream's, one rounding per operation.
#include <math.h>

#include "common.h"
#include "launch_util.h"
#include "topk_select.h"

namespace m355 {
namespace {

struct PostArgs {
  const float* logits;   // (B, Q, C)
  const float* boxes;    // (B, Q, 4) cx, cy, w, h
  const float* sizes;    // (B, 2) height, width, or nullptr
  float threshold;
  int Q, C;
  float* scores;         // (B, Q)
  long long* labels;     // (B, Q)
  float* out_boxes;      // (B, Q, 4)
  int* counts;           // (B, 2) n_nan, n_keep
};

__global__ __launch_bounds__(PP_THREADS) void dfine_postprocess_kernel(const PostArgs a) {
  __shared__ TopkScratch sm;
  __shared__ int cnt[2];                           // n_nan, n_keep

  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = a.Q, C = a.C, N = a.Q * a.C;       // N < 2^24
  const float* lg = a.logits + (size_t)b * N;
  if (tid < 2) cnt[tid] = 0;
  topk_sorted_pairs([lg](int i) { return order_key(lg[i]); }, N, K, sm);

  // ---- rows -----------------------------------------------------------------------------------------------------------------
  float sw = 1.f, sh = 1.f;
  if (a.sizes) { sh = a.sizes[2 * b]; sw = a.sizes[2 * b + 1]; }
  int my_nan = 0, my_keep = 0;
  for (int r = tid; r < K; r += PP_THREADS) {
    const unsigned long long pair = sm.pairs[r];
    unsigned i = ~(unsigned)pair;
    if (i >= (unsigned)N) i = (unsigned)N - 1u;   // never taken: see the compaction's bounds
    const unsigned q = i / (unsigned)C, c = i - q * (unsigned)C;
    const float x = lg[i];
    const float score = 1.f / (1.f + expf(-x));
    my_nan += (unsigned)(pair >> 32) == PP_NAN_KEY;
    my_keep += score > a.threshold;
    const float* pb = a.boxes + ((size_t)b * a.Q + q) * 4;   // scalar loads: a caller's view need not be 16-byte aligned
    const float cx = pb[0], cy = pb[1], w = pb[2], h = pb[3];
    float x0 = cx - 0.5f * w, y0 = cy - 0.5f * h, x1 = cx + 0.5f * w, y1 = cy + 0.5f * h;
    if (a.sizes) { x0 = x0 * sw; y0 = y0 * sh; x1 = x1 * sw; y1 = y1 * sh; }
    const size_t o = (size_t)b * K + r;
    a.scores[o] = score;
    a.labels[o] = (long long)c;
    float* ob = a.out_boxes + o * 4;
    ob[0] = x0; ob[1] = y0; ob[2] = x1; ob[3] = y1;
  }
  if (my_nan) atomicAdd(&cnt[0], my_nan);     // integer counters in LDS
  if (my_keep) atomicAdd(&cnt[1], my_keep);
  __syncthreads();
  if (tid < 2) a.counts[2 * b + tid] = cnt[tid];
}

}  // namespace

int launch_dfine_postprocess(const float* logits, const float* boxes, int B, int Q, int C, const float* sizes, float threshold,
                             float* scores, long long* labels, float* out_boxes, int* counts, hipStream_t s) {
  PostArgs a{};
  a.logits = logits; a.boxes = boxes; a.sizes = sizes; a.threshold = threshold; a.Q = Q; a.C = C;
  a.scores = scores; a.labels = labels; a.out_boxes = out_boxes; a.counts = counts;
  hipLaunchKernelGGL(dfine_postprocess_kernel, dim3(B), dim3(PP_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace m355
