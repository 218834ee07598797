// D-FINE / RT-DETR detection post-processing on the device (transformers' RTDetrImageProcessor.post_process_object_detection,
// models/rt_detr/image_processing_rt_detr.py:482-552, focal branch), which the reference's predict and eval scripts call once per
// frame: sigmoid, top-K over the Q*C flattened scores (K = Q), label / query from the flat index, cxcywh -> xyxy, scale by the
// image size, and the count of rows above the threshold.
//
// One block per image.  Every candidate i = q*C + c gets a 32-bit key that orders as the output does: a NaN logit has the
// greatest key (torch.topk's order), then descending logit, -0 == +0.  With more than 2048 candidates a 4-pass radix select
// (8 bits per pass, a 256-bin integer histogram in LDS) finds the K-th greatest key; what lies above it, and the lowest-index
// candidates that equal it, are compacted into LDS in index order (wave ballots, no atomics); with 2048 candidates or fewer all
// of them go to the sort directly.  A bitonic sort of the (key, ~index) pairs, which are pairwise distinct, gives the rows.
// The histogram's integer atomics only count: no output bit depends on scheduling, and an image's result does not depend on
// the other images of the batch.
// This file is compiled with -ffp-contract=off: the box arithmetic is upstream's, one rounding per operation.
#include <math.h>

#include "common.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int PP_THREADS = 512;
constexpr int PP_WAVES = PP_THREADS / 64;
constexpr int PP_MAX_K = 2048;
// Logits crowd into a few exponents, so most lanes of a wave want the same bin, and an LDS atomic serialises over equal
// addresses: every bin has PP_COPIES counters in PP_COPIES banks, one per lane % PP_COPIES, summed when the pass is read.
constexpr int PP_COPIES = 16;
constexpr int PP_UNROLL = 8;   // loads per lane in flight in the passes over all Q * C candidates
constexpr unsigned PP_NAN_KEY = 0xffffffffu;

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

// greater key = earlier row.  No real logit has key 0 (its bit pattern would be a NaN's): 0 is the sort's padding.
__device__ __forceinline__ unsigned order_key(float x) {
  if (x != x) return PP_NAN_KEY;
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;   // -0 ties with +0, as the comparison of the logits does
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(PP_THREADS) void dfine_postprocess_kernel(const PostArgs a) {
  __shared__ unsigned long long pairs[PP_MAX_K];   // (key << 32) | ~index, sorted descending
  __shared__ unsigned hist[256 * PP_COPIES];       // [bin][copy]
  __shared__ int wave_cnt[PP_WAVES][2];            // candidates above / equal to the K-th key that each wave owns
  __shared__ int sel[2];                           // the pass's bin and how many rows are still to be found inside it
  __shared__ int cnt[2];                           // n_nan, n_keep

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.Q, C = a.C, N = a.Q * a.C;       // N < 2^24
  const float* lg = a.logits + (size_t)b * N;
  const bool select = N > PP_MAX_K;                // fewer candidates than the sort holds: all of them are sorted, no selection
  const int M = select ? K : N;                    // pairs that reach the sort
  int P = 1;
  while (P < M) P <<= 1;

  if (tid < 2) cnt[tid] = 0;
  if (!select) {
    for (int r = tid; r < P; r += PP_THREADS)
      pairs[r] = r < N ? ((unsigned long long)order_key(lg[r]) << 32) | (unsigned)~r : 0ull;
  } else {
    for (int r = tid; r < P; r += PP_THREADS) pairs[r] = 0ull;
    // ---- the K-th greatest key: `kth`, and `need` = how many of the candidates equal to it belong to the output ------------
    unsigned prefix = 0u, mask = 0u;
    int remaining = K;
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int t = tid; t < 256 * PP_COPIES; t += PP_THREADS) hist[t] = 0u;
      __syncthreads();
      for (int i0 = 0; i0 < N; i0 += PP_UNROLL * PP_THREADS) {
        unsigned keys[PP_UNROLL];
#pragma unroll
        for (int u = 0; u < PP_UNROLL; ++u) {
          const int i = i0 + u * PP_THREADS + tid;
          const unsigned key = order_key(lg[min(i, N - 1)]);   // an unconditional load: a branch around it would wait for each one
          keys[u] = i < N ? key : 0u;                          // 0: no candidate
        }
#pragma unroll
        for (int u = 0; u < PP_UNROLL; ++u) {
          const unsigned key = keys[u];
          if (key != 0u && (key & mask) == prefix) atomicAdd(&hist[((key >> shift) & 255u) * PP_COPIES + (lane & (PP_COPIES - 1))], 1u);
        }
      }
      __syncthreads();
      if (wave == 0) {   // lane l owns the bins 255 - 4l .. 252 - 4l: ascending (lane, j) is descending bin
        int c[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          c[j] = 0;
#pragma unroll
          for (int cp = 0; cp < PP_COPIES; ++cp) c[j] += (int)hist[(255 - (4 * lane + j)) * PP_COPIES + cp];
          s += c[j];
        }
        int incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int o = __shfl_up(incl, d, 64);
          if (lane >= d) incl += o;
        }
        int above = incl - s;   // candidates in greater bins
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (above < remaining && remaining <= above + c[j]) { sel[0] = 255 - (4 * lane + j); sel[1] = remaining - above; }
          above += c[j];
        }
      }
      __syncthreads();
      prefix |= (unsigned)sel[0] << shift;
      mask |= 255u << shift;
      remaining = sel[1];
    }
    const unsigned kth = prefix;
    const int need = remaining;

    // ---- compaction in index order: wave w owns a contiguous run of 64-candidate chunks -----------------------------------
    const int chunks = (N + 63) >> 6, per_wave = (chunks + PP_WAVES - 1) / PP_WAVES;
    const int c0 = wave * per_wave, c1 = min(c0 + per_wave, chunks);
    int n_gt = 0, n_eq = 0;
    for (int ch = c0; ch < c1; ch += PP_UNROLL) {
      unsigned keys[PP_UNROLL];
#pragma unroll
      for (int u = 0; u < PP_UNROLL; ++u) {
        const int i = (ch + u) * 64 + lane;   // real keys are >= 1: kth is, and 0 (no candidate) is neither above nor equal
        const unsigned key = order_key(lg[min(i, N - 1)]);
        keys[u] = (ch + u < c1 && i < N) ? key : 0u;
      }
#pragma unroll
      for (int u = 0; u < PP_UNROLL; ++u) {
        n_gt += __popcll(__ballot(keys[u] > kth));
        n_eq += __popcll(__ballot(keys[u] == kth));
      }
    }
    if (lane == 0) { wave_cnt[wave][0] = n_gt; wave_cnt[wave][1] = n_eq; }
    __syncthreads();
    int gt_base = 0, eq_base = 0, gt_total = 0;
#pragma unroll
    for (int w = 0; w < PP_WAVES; ++w) {
      const int g = wave_cnt[w][0], e = wave_cnt[w][1];
      if (w < wave) { gt_base += g; eq_base += e; }
      gt_total += g;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int ch = c0; ch < c1; ch += PP_UNROLL) {
      unsigned keys[PP_UNROLL];
#pragma unroll
      for (int u = 0; u < PP_UNROLL; ++u) {
        const int i = (ch + u) * 64 + lane;
        const unsigned key = order_key(lg[min(i, N - 1)]);
        keys[u] = (ch + u < c1 && i < N) ? key : 0u;
      }
#pragma unroll
      for (int u = 0; u < PP_UNROLL; ++u) {
        const int i = (ch + u) * 64 + lane;
        const unsigned key = keys[u];
        const bool gt = key > kth, eq = key == kth;
        const unsigned long long mg = __ballot(gt), me = __ballot(eq);
        const unsigned long long pair = ((unsigned long long)key << 32) | (unsigned)~i;
        // the bounds hold by construction (gt_total + need == K); they are kept so that a logits buffer that changes under
        // the kernel cannot send a store outside the array
        if (gt) {
          const int pos = gt_base + __popcll(mg & below);
          if (pos < K) pairs[pos] = pair;
        }
        if (eq) {
          const int rank = eq_base + __popcll(me & below);
          if (rank < need && gt_total + rank < K) pairs[gt_total + rank] = pair;
        }
        gt_base += __popcll(mg);
        eq_base += __popcll(me);
      }
    }
  }
  __syncthreads();

  // ---- bitonic sort, descending; the pairs are distinct (the padding zeros compare equal and stay where they are) ----------
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += PP_THREADS) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const unsigned long long x = pairs[i], y = pairs[l];
        const bool desc = (i & k) == 0;
        if (desc ? x < y : x > y) { pairs[i] = y; pairs[l] = x; }
      }
      __syncthreads();
    }
  }

  // ---- rows -----------------------------------------------------------------------------------------------------------------
  float sw = 1.f, sh = 1.f;
  if (a.sizes) { sh = a.sizes[2 * b]; sw = a.sizes[2 * b + 1]; }
  int my_nan = 0, my_keep = 0;
  for (int r = tid; r < K; r += PP_THREADS) {
    const unsigned long long pair = pairs[r];
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
