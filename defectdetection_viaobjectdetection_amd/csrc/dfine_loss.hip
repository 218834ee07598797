// D-FINE loss terms on the device: loss_vfl, loss_bbox, loss_giou (transformers' RTDetrLoss.loss_labels_vfl / loss_boxes,
// loss_rt_detr.py:165-254) and loss_fgl, loss_ddf (DFineLoss.loss_local, loss_d_fine.py:228-301) of ONE decoder output, with
// their gradients.  What the matcher (dfine_match.hip) leaves on the device is consumed here without a trip to the host.
//
// Forward: launch 1 gives every query (b, q) to one wave (4 queries per block).  The block finds its queries' match entries by
// scanning the entries of its image; the wave then evaluates the query's C class elements, its box pair and its 4 corner rows
// (one lane per bin, R + 1 <= 64).  Launch 2 is one block that adds the per-block partials in block order and writes the five
// values plus the two DDF group coefficients the backward needs.
// Backward: one launch of the same shape recomputes the query's quantities and writes EVERY element of the three gradient
// tensors (zeros where a term does not reach): no memset, no scatter-add.
// Sums: per lane in index order, wave shuffle (xor butterfly), waves in order, blocks in order.  No atomics; the grid is a
// function of (B, Q) alone; two runs give the same bits.  Every loop is a `for` bounded by the shapes.
// Compiled with -ffp-contract=off: one rounding per operation, upstream's expressions.
#include <math.h>

#include "common.h"
#include "device_prims.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_QPB = 4;      // queries per block: one per wave
constexpr int LOSS_SLOTS = 8;    // per-block partials: vfl, bbox, giou, fgl, ddf matched, ddf unmatched, matched count (int bits), -

// log_softmax of one row of n <= 64 values, lane i holding value i (z is ignored on lanes >= n).  The ONE routine behind both
// sides of the KL term: equal input bits give equal output bits, so a teacher equal to the prediction gives exactly 0.
__device__ __forceinline__ float row_log_softmax(float z, bool live) {
  const float m = wave_max(live ? z : -INFINITY);
  const float s = wave_sum(live ? expf(z - m) : 0.f);
  return z - (m + logf(s));
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// box_iou / generalized_box_iou of one (prediction, target) pair, both cx, cy, w, h
struct Pair {
  float px0, py0, px1, py1, tx0, ty0, tx1, ty1;
  float iw, ih, inter, uni, iou, ew, eh, area, giou;
};
__device__ __forceinline__ Pair pair_geometry(const float4 p, const float4 t) {
  Pair g;
  g.px0 = p.x - 0.5f * p.z; g.py0 = p.y - 0.5f * p.w; g.px1 = p.x + 0.5f * p.z; g.py1 = p.y + 0.5f * p.w;
  g.tx0 = t.x - 0.5f * t.z; g.ty0 = t.y - 0.5f * t.w; g.tx1 = t.x + 0.5f * t.z; g.ty1 = t.y + 0.5f * t.w;
  const float area1 = (g.px1 - g.px0) * (g.py1 - g.py0), area2 = (g.tx1 - g.tx0) * (g.ty1 - g.ty0);
  g.iw = fmaxf(fminf(g.px1, g.tx1) - fmaxf(g.px0, g.tx0), 0.f);
  g.ih = fmaxf(fminf(g.py1, g.ty1) - fmaxf(g.py0, g.ty0), 0.f);
  g.inter = g.iw * g.ih;
  g.uni = area1 + area2 - g.inter;
  g.iou = g.inter / g.uni;
  g.ew = fmaxf(fmaxf(g.px1, g.tx1) - fminf(g.px0, g.tx0), 0.f);
  g.eh = fmaxf(fmaxf(g.py1, g.ty1) - fminf(g.py0, g.ty0), 0.f);
  g.area = g.ew * g.eh;
  g.giou = g.iou - (g.area - g.uni) / g.area;
  return g;
}

// d(1 - GIoU) / d(cx, cy, w, h of the prediction), through min / max / clamp as autograd takes them
__device__ __forceinline__ float4 giou_loss_grad(const Pair& g) {
  const float g_uni = -g.inter / (g.uni * g.uni) + 1.f / g.area;   // giou = inter / uni - 1 + uni / area
  const float g_inter = 1.f / g.uni - g_uni;                        // uni = area1 + area2 - inter
  const float g_area = -g.uni / (g.area * g.area);
  const float g_iw = g.iw > 0.f ? g_inter * g.ih : 0.f, g_ih = g.ih > 0.f ? g_inter * g.iw : 0.f;
  const float g_ew = g_area * g.eh, g_eh = g_area * g.ew;
  const float pw = g.px1 - g.px0, ph = g.py1 - g.py0;
  float gx0 = -g_uni * ph, gx1 = g_uni * ph, gy0 = -g_uni * pw, gy1 = g_uni * pw;   // area1 = pw * ph
  if (g.px1 < g.tx1) gx1 += g_iw; else gx1 += g_ew;   // min(px1, tx1) feeds the intersection, max(px1, tx1) the hull
  if (g.px0 > g.tx0) gx0 -= g_iw; else gx0 -= g_ew;
  if (g.py1 < g.ty1) gy1 += g_ih; else gy1 += g_eh;
  if (g.py0 > g.ty0) gy0 -= g_ih; else gy0 -= g_eh;
  // loss = 1 - giou
  return make_float4(-(gx0 + gx1), -(gy0 + gy1), -0.5f * (gx1 - gx0), -0.5f * (gy1 - gy0));
}

// what a wave knows about its query after the block's scan of the image's match entries
struct QueryMatch {
  bool matched;
  long long label;
  float4 pbox, tbox;
  Pair g;
};

// the block's part of the image's match list -> lmap[LOSS_QPB] (entry index or -1); returns the image's first target row and count
__device__ __forceinline__ void scan_matches(const DfineLossArgs& a, int b, int q0, int* lmap, int& t0, int& nt) {
  const int tid = threadIdx.x;
  if (tid < LOSS_QPB) lmap[tid] = -1;
  __syncthreads();
  int e0 = 0, e1 = 0;
  t0 = 0; nt = 0;
  if (a.M > 0 && a.T > 0) {   // device offsets are clamped to what the host validated: never followed out of bounds
    e0 = min(max(a.offsets[b], 0), a.M);
    e1 = min(max(a.offsets[b + 1], e0), a.M);
    t0 = min(max(a.offsets[a.B + 1 + b], 0), a.T);
    nt = min(max(a.offsets[a.B + 2 + b], t0), a.T) - t0;
  }
  for (int e = e0 + tid; e < e1; e += LOSS_THREADS) {
    const long long q = a.match_q[e], t = a.match_t[e];
    if (q >= q0 && q < q0 + LOSS_QPB && q < a.Q && t >= 0 && t < nt) lmap[(int)q - q0] = e;
  }
  __syncthreads();
}

__device__ __forceinline__ QueryMatch load_match(const DfineLossArgs& a, int b, int q, int e, int t0) {
  QueryMatch m;
  m.matched = e >= 0;
  m.label = -1;
  const float* pp = a.boxes + ((size_t)b * a.Q + q) * 4;
  m.pbox = make_float4(pp[0], pp[1], pp[2], pp[3]);
  m.tbox = m.pbox;
  if (m.matched) {
    const size_t row = (size_t)t0 + (size_t)a.match_t[e];
    const float* tp = a.tboxes + row * 4;
    m.tbox = make_float4(tp[0], tp[1], tp[2], tp[3]);
    m.label = a.labels[row];
  }
  m.g = pair_geometry(m.pbox, m.tbox);
  return m;
}

// one class element of the varifocal term: the weight w and sigmoid(x) - t on request
__device__ __forceinline__ float vfl_weight(const DfineLossArgs& a, float x, bool hot, float t, float& p) {
  p = sigmoidf(x);
  const float pg = a.gamma == 2.f ? p * p : powf(p, a.gamma);
  return a.alpha * pg * (hot ? 0.f : 1.f) + t;
}

// translate_gt of one side's distance d: left bin l and the two weights.  W(lane) is `wv` on lanes < nb1.
__device__ __forceinline__ void fgl_target(float d, float wv, int lane, int nb1, int& l, float& w_left, float& w_right) {
  const int R = nb1 - 1;
  const int idx = __popcll(__ballot(lane < nb1 && wv <= d)) - 1;
  if (idx < 0) {
    l = 0; w_left = 1.f; w_right = 0.f;
  } else if (idx >= R) {
    l = R - 1; w_left = 0.f; w_right = 1.f;   // index R - 0.1, truncated
  } else {
    const float left = __shfl(wv, idx, 64), right = __shfl(wv, idx + 1, 64);
    const float ld = fabsf(d - left), rd = fabsf(right - d);
    w_right = ld / (ld + rd);
    w_left = 1.f - w_right;
    l = idx;
  }
}

// bbox2distance of side k (left, top, right, bottom)
__device__ __forceinline__ float fgl_distance(const float4 ref, const Pair& g, int k, float reg_scale) {
  const float rs = fabsf(reg_scale);
  const float num = k == 0 ? ref.x - g.tx0 : k == 1 ? ref.y - g.ty0 : k == 2 ? g.tx1 - ref.x : g.ty1 - ref.y;
  const float ext = (k & 1) ? ref.w : ref.z;
  return num / (ext / rs + 1e-16f) - 0.5f * rs;
}

__global__ __launch_bounds__(LOSS_THREADS) void dfine_loss_forward_kernel(const DfineLossArgs a) {
  __shared__ int lmap[LOSS_QPB];
  __shared__ float wpart[LOSS_QPB][LOSS_SLOTS];
  const int bpi = (a.Q + LOSS_QPB - 1) / LOSS_QPB;
  const int b = blockIdx.x / bpi, q0 = (blockIdx.x - b * bpi) * LOSS_QPB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int t0, nt;
  scan_matches(a, b, q0, lmap, t0, nt);

  const int q = q0 + wave;
  float s_vfl = 0.f, s_bbox = 0.f, s_giou = 0.f, s_fgl = 0.f, s_pos = 0.f, s_neg = 0.f;
  int n_pos = 0;
  if (q < a.Q) {
    const QueryMatch m = load_match(a, b, q, lmap[wave], t0);
    const float iou = m.matched ? m.g.iou : 0.f;
    n_pos = m.matched ? 1 : 0;
    // ---- loss_vfl: the query's C elements
    const float* lg = a.logits + ((size_t)b * a.Q + q) * a.C;
    float acc = 0.f;
    for (int c = lane; c < a.C; c += 64) {
      const float x = lg[c];
      const bool hot = m.matched && (long long)c == m.label;
      const float t = hot ? iou : 0.f;
      float p;
      const float w = vfl_weight(a, x, hot, t, p);
      const float bce = ((1.f - t) * x + fmaxf(-x, 0.f)) + log1pf(expf(-fabsf(x)));
      acc += w * bce;
    }
    s_vfl = wave_sum(acc);
    // ---- loss_bbox, loss_giou: the matched pair
    if (m.matched) {
      s_bbox = ((fabsf(m.pbox.x - m.tbox.x) + fabsf(m.pbox.y - m.tbox.y)) + fabsf(m.pbox.z - m.tbox.z)) + fabsf(m.pbox.w - m.tbox.w);
      s_giou = 1.f - m.g.giou;
    }
    // ---- loss_fgl, loss_ddf: the query's 4 corner rows
    if (a.pred_corners) {
      const int nb1 = a.nb1;
      const bool live = lane < nb1;
      const float* tl = a.teacher_logits + ((size_t)b * a.Q + q) * a.C;
      float mx = -INFINITY;
      for (int c = lane; c < a.C; c += 64) mx = fmaxf(mx, tl[c]);
      const float weight = m.matched ? iou : sigmoidf(wave_max(mx));   // max of sigmoid = sigmoid of max
      const float wv = live ? a.project[lane] : 0.f;
      const float* rp = a.ref_points + ((size_t)b * a.Q + q) * 4;
      const float4 ref = make_float4(rp[0], rp[1], rp[2], rp[3]);
      const size_t row0 = ((size_t)b * a.Q + q) * 4;
      float ddf = 0.f;
      for (int k = 0; k < 4; ++k) {
        const float x = live ? a.pred_corners[(row0 + k) * nb1 + lane] : 0.f;
        const float y = live ? a.teacher_corners[(row0 + k) * nb1 + lane] : 0.f;
        const float lp = row_log_softmax(x / a.temperature, live);
        const float lq = row_log_softmax(y / a.temperature, live);
        const float kl = wave_sum(live ? expf(lq) * (lq - lp) : 0.f);
        ddf += (weight * (a.temperature * a.temperature)) * kl;
        if (m.matched) {
          int l;
          float w_left, w_right;
          fgl_target(fgl_distance(ref, m.g, k, a.reg_scale), wv, lane, nb1, l, w_left, w_right);
          const float l1 = row_log_softmax(x, live);
          const float ce_l = -__shfl(l1, l, 64), ce_r = -__shfl(l1, l + 1, 64);
          s_fgl += (ce_l * w_left + ce_r * w_right) * iou;
        }
      }
      if (m.matched) s_pos = ddf; else s_neg = ddf;
    }
  }
  if (lane == 0) {
    wpart[wave][0] = s_vfl; wpart[wave][1] = s_bbox; wpart[wave][2] = s_giou; wpart[wave][3] = s_fgl;
    wpart[wave][4] = s_pos; wpart[wave][5] = s_neg; wpart[wave][6] = __int_as_float(n_pos); wpart[wave][7] = 0.f;
  }
  __syncthreads();
  if (tid < LOSS_SLOTS) {
    float* out = a.partials + (size_t)blockIdx.x * LOSS_SLOTS + tid;
    if (tid == 6) {
      int n = 0;
      for (int w = 0; w < LOSS_QPB; ++w) n += __float_as_int(wpart[w][6]);
      *out = __int_as_float(n);
    } else {
      float v = wpart[0][tid];
      for (int w = 1; w < LOSS_QPB; ++w) v += wpart[w][tid];
      *out = v;
    }
  }
}

// one block: the per-block partials in block order -> out[0..4] the five terms, out[5], out[6] the DDF gradient coefficient of a
// matched / an unmatched row (group weight / group size), out[7] = 0
__global__ __launch_bounds__(LOSS_THREADS) void dfine_loss_reduce_kernel(const DfineLossArgs a, int nblocks) {
  __shared__ float wsum[LOSS_THREADS / 64][LOSS_SLOTS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  for (int i = tid; i < nblocks; i += LOSS_THREADS) {
    const float* p = a.partials + (size_t)i * LOSS_SLOTS;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] += p[k];
    cnt += __float_as_int(p[6]);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = wave_sum(acc[k]);
  cnt = wave_sum_int(cnt);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) wsum[wave][k] = acc[k];
    wsum[wave][6] = __int_as_float(cnt);
  }
  __syncthreads();
  if (tid != 0) return;
  float tot[6];
  int npos = 0;
  for (int k = 0; k < 6; ++k) {
    float v = wsum[0][k];
    for (int w = 1; w < LOSS_THREADS / 64; ++w) v += wsum[w][k];
    tot[k] = v;
  }
  for (int w = 0; w < LOSS_THREADS / 64; ++w) npos += __float_as_int(wsum[w][6]);
  a.out[0] = tot[0] / a.num_boxes;
  a.out[1] = tot[1] / a.num_boxes;
  a.out[2] = tot[2] / a.num_boxes;
  float fgl = 0.f, ddf = 0.f, coef_pos = 0.f, coef_neg = 0.f;
  if (a.pred_corners) {
    fgl = tot[3] / a.num_boxes;
    const float rows_pos = 4.f * (float)npos, rows_neg = 4.f * (float)(a.B * a.Q - npos);
    const float scale = 1.f / (float)a.B;
    const float num_pos = sqrtf(rows_pos * scale), num_neg = sqrtf(rows_neg * scale);
    const float mean_pos = npos > 0 ? tot[4] / rows_pos : 0.f;              // upstream's `if mask.any()`
    const float mean_neg = rows_neg > 0.f ? tot[5] / rows_neg : 0.f;
    ddf = (mean_pos * num_pos + mean_neg * num_neg) / (num_pos + num_neg);
    coef_pos = npos > 0 ? num_pos / (num_pos + num_neg) / rows_pos : 0.f;
    coef_neg = rows_neg > 0.f ? num_neg / (num_pos + num_neg) / rows_neg : 0.f;
  }
  a.out[3] = fgl; a.out[4] = ddf; a.out[5] = coef_pos; a.out[6] = coef_neg; a.out[7] = 0.f;
}

__global__ __launch_bounds__(LOSS_THREADS) void dfine_loss_backward_kernel(const DfineLossArgs a) {
  __shared__ int lmap[LOSS_QPB];
  const int bpi = (a.Q + LOSS_QPB - 1) / LOSS_QPB;
  const int b = blockIdx.x / bpi, q0 = (blockIdx.x - b * bpi) * LOSS_QPB;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int t0, nt;
  scan_matches(a, b, q0, lmap, t0, nt);
  const int q = q0 + wave;
  if (q >= a.Q) return;

  const QueryMatch m = load_match(a, b, q, lmap[wave], t0);
  const float iou = m.matched ? m.g.iou : 0.f;
  // the five upstream gradients, scaled as the forward scales the sums
  const float g_vfl = a.grad_terms[0] / a.num_boxes, g_bbox = a.grad_terms[1] / a.num_boxes, g_giou = a.grad_terms[2] / a.num_boxes;
  if (a.grad_logits) {
    const float* lg = a.logits + ((size_t)b * a.Q + q) * a.C;
    float* gl = a.grad_logits + ((size_t)b * a.Q + q) * a.C;
    for (int c = lane; c < a.C; c += 64) {
      const bool hot = m.matched && (long long)c == m.label;
      const float t = hot ? iou : 0.f;
      float p;
      const float w = vfl_weight(a, lg[c], hot, t, p);
      gl[c] = g_vfl * (w * (p - t));
    }
  }
  if (a.grad_boxes && lane < 4) {
    float v = 0.f;
    if (m.matched) {
      const float4 gg = giou_loss_grad(m.g);
      const float d = lane == 0 ? m.pbox.x - m.tbox.x : lane == 1 ? m.pbox.y - m.tbox.y : lane == 2 ? m.pbox.z - m.tbox.z : m.pbox.w - m.tbox.w;
      const float sign = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
      const float gi = lane == 0 ? gg.x : lane == 1 ? gg.y : lane == 2 ? gg.z : gg.w;
      v += g_bbox * sign;
      v += g_giou * gi;
    }
    a.grad_boxes[((size_t)b * a.Q + q) * 4 + lane] = v;
  }
  if (a.pred_corners && a.grad_corners) {
    const float g_fgl = a.grad_terms[3] / a.num_boxes, g_ddf = a.grad_terms[4];
    const float coef = m.matched ? a.out[5] : a.out[6];
    const int nb1 = a.nb1;
    const bool live = lane < nb1;
    const float* tl = a.teacher_logits + ((size_t)b * a.Q + q) * a.C;
    float mx = -INFINITY;
    for (int c = lane; c < a.C; c += 64) mx = fmaxf(mx, tl[c]);
    const float weight = m.matched ? iou : sigmoidf(wave_max(mx));
    const float wv = live ? a.project[lane] : 0.f;
    const float* rp = a.ref_points + ((size_t)b * a.Q + q) * 4;
    const float4 ref = make_float4(rp[0], rp[1], rp[2], rp[3]);
    const size_t row0 = ((size_t)b * a.Q + q) * 4;
    for (int k = 0; k < 4; ++k) {
      const float x = live ? a.pred_corners[(row0 + k) * nb1 + lane] : 0.f;
      const float y = live ? a.teacher_corners[(row0 + k) * nb1 + lane] : 0.f;
      const float lp = row_log_softmax(x / a.temperature, live);
      const float lq = row_log_softmax(y / a.temperature, live);
      float v = 0.f;   // 0 + (-0) = +0: equal rows leave all-zero bits whatever the sign of the upstream gradient
      v += g_ddf * (((weight * a.temperature) * (expf(lp) - expf(lq))) * coef);
      if (m.matched) {
        int l;
        float w_left, w_right;
        fgl_target(fgl_distance(ref, m.g, k, a.reg_scale), wv, lane, nb1, l, w_left, w_right);
        const float sm = expf(row_log_softmax(x, live));
        v += (g_fgl * iou) * (((w_left + w_right) * sm - (lane == l ? w_left : 0.f)) - (lane == l + 1 ? w_right : 0.f));
      }
      if (live) a.grad_corners[(row0 + k) * nb1 + lane] = v;
    }
  }
}

}  // namespace

size_t dfine_loss_workspace_bytes(int B, int Q) {
  if (B < 1 || Q < 1) return 0;
  return (size_t)B * ((Q + LOSS_QPB - 1) / LOSS_QPB) * LOSS_SLOTS * sizeof(float);
}

int launch_dfine_loss_forward(const DfineLossArgs& a, hipStream_t s) {
  const int nblocks = a.B * ((a.Q + LOSS_QPB - 1) / LOSS_QPB);
  hipLaunchKernelGGL(dfine_loss_forward_kernel, dim3(nblocks), dim3(LOSS_THREADS), 0, s, a);
  hipLaunchKernelGGL(dfine_loss_reduce_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, a, nblocks);
  return (int)hipGetLastError();
}

int launch_dfine_loss_backward(const DfineLossArgs& a, hipStream_t s) {
  const int nblocks = a.B * ((a.Q + LOSS_QPB - 1) / LOSS_QPB);
  hipLaunchKernelGGL(dfine_loss_backward_kernel, dim3(nblocks), dim3(LOSS_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace m355
