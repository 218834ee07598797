// D-FINE / RT-DETR Hungarian matcher on the device (transformers' RTDetrHungarianMatcher.forward, loss_rt_detr.py:68-120,
// which the reference's D-FINE trainers reach through `self.dfine.loss_function(...)` once per frame).
//
// One block per image.  All 256 threads evaluate the image's (Q x n) cost matrix in fp32, in the order of operations of
// loss_rt_detr.py:99-114 (this file is compiled with -ffp-contract=off); then wave 0 alone solves the assignment with
// shortest augmenting paths (the algorithm of scipy.optimize.linear_sum_assignment), the shorter side as rows, dual
// variables and path lengths in fp64.  Lanes stride over the columns, min / argmin by wave shuffles, a tie goes to the lowest
// column.  Every loop is a `for` whose trip bound comes from Q and n alone; there are no atomics and no block barrier inside
// the search, so the result is bitwise reproducible and does not depend on the other images of the batch.
// The matrix lives in LDS when it fits beside the solver's arrays, otherwise in the caller's workspace.
#include <math.h>

#include "common.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int MATCH_THREADS = 256;
constexpr int MATCH_LDS_MAX = 159 * 1024;   // dynamic LDS; one workgroup may own a CU's 160 KiB, the block vote keeps a few static bytes

struct MatchArgs {
  const float* logits;       // (B, Q, C)
  const float* boxes;        // (B, Q, 4) cx, cy, w, h
  const long long* labels;   // (T)
  const float* tboxes;       // (T, 4) cx, cy, w, h
  const int* offsets;        // (B + 1) first target of each image, device
  int B, Q, C, T, nmax;      // nmax: the largest target count the host saw; sizes the LDS layout, the workspace and d_cost
  float class_cost, bbox_cost, giou_cost, alpha, one_minus_alpha, gamma;
  int focal;
  float* work;               // (B, Q * nmax) cost matrices when they do not fit in LDS, else nullptr
  float* cost_out;           // (B, Q, nmax) or nullptr
  long long* rows;           // (B, kmax) query index, ascending
  long long* cols;           // (B, kmax) target index within the image
  int kmax;
  int* flags;                // (B) 0 = solved, 1 = a non-finite cost, 2 = offsets outside what the host validated
};

// bytes of the solver's LDS arrays for a problem of at most nr rows and nc columns; each array starts 8-byte aligned
__host__ __device__ inline size_t solver_lds_bytes(int nr, int nc) {
  const size_t nr2 = (size_t)(nr + 1) & ~(size_t)1, nc2 = (size_t)(nc + 1) & ~(size_t)1;
  return nc2 * (8 + 8 + 4 + 4 + 4) + nr2 * (8 + 4);
}
inline size_t match_lds_bytes(int Q, int nmax, bool cost_in_lds) {
  const int nr = Q < nmax ? Q : nmax, nc = Q < nmax ? nmax : Q;
  return solver_lds_bytes(nr, nc) + (cost_in_lds ? (size_t)Q * nmax * 4 : 0);
}

__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// (value, index) minimum over the 64 lanes, equal values to the lower index; every lane ends with the result
__device__ __forceinline__ void wave_argmin(double& v, int& i) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double ov = __shfl_xor(v, m, 64);
    const int oi = __shfl_xor(i, m, 64);
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// one entry of loss_rt_detr.py:99-114; p (cx, cy, w, h) the query's box, t the target's, cls the class term
__device__ __forceinline__ float pair_cost(const float4 p, const float4 t, float cls, const MatchArgs& a) {
  const float l1 = ((fabsf(p.x - t.x) + fabsf(p.y - t.y)) + fabsf(p.z - t.z)) + fabsf(p.w - t.w);
  const float px0 = p.x - 0.5f * p.z, py0 = p.y - 0.5f * p.w, px1 = p.x + 0.5f * p.z, py1 = p.y + 0.5f * p.w;
  const float tx0 = t.x - 0.5f * t.z, ty0 = t.y - 0.5f * t.w, tx1 = t.x + 0.5f * t.z, ty1 = t.y + 0.5f * t.w;
  const float area1 = (px1 - px0) * (py1 - py0), area2 = (tx1 - tx0) * (ty1 - ty0);
  // torch.max / min / clamp propagate NaN; fmaxf / fminf would drop it, the L1 term above carries it instead
  const float iw = fmaxf(fminf(px1, tx1) - fmaxf(px0, tx0), 0.f), ih = fmaxf(fminf(py1, ty1) - fmaxf(py0, ty0), 0.f);
  const float inter = iw * ih;
  const float uni = area1 + area2 - inter;
  const float iou = inter / uni;
  const float ew = fmaxf(fmaxf(px1, tx1) - fminf(px0, tx0), 0.f), eh = fmaxf(fmaxf(py1, ty1) - fminf(py0, ty0), 0.f);
  const float area = ew * eh;
  const float giou = iou - (area - uni) / area;
  return a.bbox_cost * l1 + a.class_cost * cls + a.giou_cost * (-giou);
}

__device__ __forceinline__ float focal_term(float logit, const MatchArgs& a) {
  const float p = 1.f / (1.f + expf(-logit));
  const float q = 1.f - p;
  const float pg = a.gamma == 2.f ? p * p : powf(p, a.gamma), qg = a.gamma == 2.f ? q * q : powf(q, a.gamma);
  const float neg = a.one_minus_alpha * pg * (-logf(q + 1e-8f));
  const float pos = a.alpha * qg * (-logf(p + 1e-8f));
  return pos - neg;
}

__global__ __launch_bounds__(MATCH_THREADS) void dfine_match_kernel(const MatchArgs a) {
  extern __shared__ double match_lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Q = a.Q;
  const int off0 = a.offsets[b], off1 = a.offsets[b + 1];
  int n = off1 - off0;
  const bool offsets_ok = off0 >= 0 && n >= 0 && n <= a.nmax && off1 <= a.T;
  if (!offsets_ok) n = 0;
  const int nr = Q < n ? Q : n, nc = Q < n ? n : Q;
  const bool rows_are_targets = Q >= n;

  // LDS layout, sized by what the host validated (nmax), identical in every block
  const int nr_max = Q < a.nmax ? Q : a.nmax, nc_max = Q < a.nmax ? a.nmax : Q;
  const int nr2 = (nr_max + 1) & ~1, nc2 = (nc_max + 1) & ~1;
  double* v = match_lds;            // [nc] dual of the columns
  double* spc = v + nc2;            // [nc] shortest path cost to each column
  double* u = spc + nc2;            // [nr] dual of the rows
  int* path = (int*)(u + nr2);      // [nc] row before the column on its shortest path
  int* row4col = path + nc2;        // [nc]
  int* done = row4col + nc2;        // [nc] column scanned in this search
  int* col4row = done + nc2;        // [nr]
  float* cost = a.work ? a.work + (size_t)b * Q * a.nmax : (float*)(col4row + nr2);   // [nr][nc]

  // ---- cost matrix -------------------------------------------------------------------------------------------------
  const float* lg = a.logits + (size_t)b * Q * a.C;
  float2* qstat = (float2*)spc;     // [Q] (max, sum of exp) of each query's logits, softmax form only; Q <= nc_max
  if (!a.focal) {
    for (int q = tid; q < Q; q += MATCH_THREADS) {
      const float* x = lg + (size_t)q * a.C;
      float mx = x[0];
      for (int c = 1; c < a.C; ++c) mx = fmaxf(mx, x[c]);   // drops a NaN logit; the sum below keeps it
      float sum = 0.f;
      for (int c = 0; c < a.C; ++c) sum += expf(x[c] - mx);
      qstat[q] = make_float2(mx, sum);
    }
    __syncthreads();
  }
  int bad = 0;
  const int total = Q * n;
  for (int e = tid; e < total; e += MATCH_THREADS) {
    int q, t;
    if (rows_are_targets) { t = e / Q; q = e - t * Q; } else { q = e / n; t = e - q * n; }
    const float* pp = a.boxes + ((size_t)b * Q + q) * 4;      // scalar loads: a caller's view need not be 16-byte aligned
    const float* tp = a.tboxes + (size_t)(off0 + t) * 4;
    const float4 pb = make_float4(pp[0], pp[1], pp[2], pp[3]);
    const float4 tb = make_float4(tp[0], tp[1], tp[2], tp[3]);
    const long long label = a.labels[off0 + t];
    float cls = NAN;   // a label outside [0, C) has no logit: the image is flagged
    if (label >= 0 && label < a.C) {
      const float x = lg[(size_t)q * a.C + label];
      if (a.focal) {
        cls = focal_term(x, a);
      } else {
        const float2 st = qstat[q];
        cls = -(expf(x - st.x) / st.y);
      }
    }
    const float c = pair_cost(pb, tb, cls, a);
    bad |= !(fabsf(c) <= 3.402823466e38f);   // NaN or +-inf
    cost[rows_are_targets ? (size_t)t * Q + q : (size_t)q * n + t] = c;
    if (a.cost_out) a.cost_out[((size_t)b * Q + q) * a.nmax + t] = c;
  }
  bad = __syncthreads_or(bad);
  if (tid >= 64) return;   // the solve is wave 0's alone

  // ---- assignment ----------------------------------------------------------------------------------------------------
  const int lane = tid;
  long long* orow = a.rows + (size_t)b * a.kmax;
  long long* ocol = a.cols + (size_t)b * a.kmax;
  int solved = 0;
  if (!bad && nr > 0) {
    for (int j = lane; j < nc; j += 64) { v[j] = 0.0; row4col[j] = -1; }
    for (int i = lane; i < nr; i += 64) { u[i] = 0.0; col4row[i] = -1; }
    solved = 1;
    for (int cur = 0; cur < nr; ++cur) {
      for (int j = lane; j < nc; j += 64) { spc[j] = INFINITY; done[j] = 0; }
      wave_sync();
      double min_val = 0.0;
      int i = cur, sink = -1;
      for (int step = 0; step < nr; ++step) {   // row `cur` finds a free column after at most cur + 1 scans
        const double ui = u[i];
        const float* crow = cost + (size_t)i * nc;
        double lowest = INFINITY;
        int index = 0x7fffffff;
        for (int j = lane; j < nc; j += 64) {
          if (done[j]) continue;
          const double r = min_val + (double)crow[j] - ui - v[j];
          double s = spc[j];
          if (r < s) { path[j] = i; spc[j] = r; s = r; }
          if (s < lowest) { lowest = s; index = j; }
        }
        wave_argmin(lowest, index);
        if (index >= nc) break;   // no column left: cannot happen with finite costs and nr <= nc
        min_val = lowest;
        done[index] = 1;
        const int r4 = row4col[index];
        wave_sync();
        if (r4 < 0) { sink = index; break; }
        i = r4;
      }
      if (sink < 0) { solved = 0; break; }
      // dual update: the scanned columns and the rows assigned to them; the rows are distinct, one writer each
      if (lane == 0) u[cur] += min_val;
      for (int j = lane; j < nc; j += 64) {
        if (!done[j]) continue;
        const double d = min_val - spc[j];
        const int r4 = row4col[j];
        if (r4 >= 0) u[r4] += d;
        v[j] -= d;
      }
      wave_sync();
      // augment along the path back to `cur`: at most cur + 1 columns; every lane walks it with the same values
      int j = sink;
      for (int k = 0; k < nr; ++k) {
        const int pi = path[j];
        row4col[j] = pi;
        const int next = col4row[pi];
        col4row[pi] = j;
        wave_sync();
        j = next;
        if (pi == cur) break;
      }
    }
  }
  // ---- output, ascending query index; the entries behind the valid ones are -1 ---------------------------------------
  int count = 0;
  if (solved) {
    if (rows_are_targets) {   // columns are queries: compact the assigned ones in order
      for (int base = 0; base < nc; base += 64) {
        const int j = base + lane;
        const int r4 = j < nc ? row4col[j] : -1;
        const unsigned long long m = __ballot(r4 >= 0);
        if (r4 >= 0) {
          const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
          orow[pos] = j;
          ocol[pos] = r4;
        }
        count += __popcll(m);
      }
    } else {                  // rows are queries, every one assigned
      for (int i = lane; i < nr; i += 64) { orow[i] = i; ocol[i] = col4row[i]; }
      count = nr;
    }
  }
  for (int k = count + lane; k < a.kmax; k += 64) { orow[k] = -1; ocol[k] = -1; }
  if (lane == 0) a.flags[b] = !offsets_ok ? 2 : bad ? 1 : (solved || nr == 0) ? 0 : 3;
}

}  // namespace

size_t dfine_match_workspace_bytes(int B, int Q, int nmax) {
  if (B < 1 || Q < 1 || nmax < 1) return 0;
  return match_lds_bytes(Q, nmax, true) <= (size_t)MATCH_LDS_MAX ? 0 : (size_t)B * Q * nmax * sizeof(float);
}

int launch_dfine_match(const float* logits, const float* boxes, int B, int Q, int C, const long long* labels, const float* tboxes,
                       const int* d_offsets, int T, int nmax, float class_cost, float bbox_cost, float giou_cost, float alpha,
                       float gamma, int focal, void* work, float* cost_out, long long* rows, long long* cols, int kmax, int* flags,
                       hipStream_t s) {
  static bool prepared = false;
  if (!prepared) {
    if (const int e = prepare_kernel((const void*)dfine_match_kernel, MATCH_LDS_MAX)) return e;
    prepared = true;
  }
  const bool in_lds = dfine_match_workspace_bytes(B, Q, nmax) == 0;
  MatchArgs a{};
  a.logits = logits; a.boxes = boxes; a.labels = labels; a.tboxes = tboxes; a.offsets = d_offsets;
  a.B = B; a.Q = Q; a.C = C; a.T = T; a.nmax = nmax;
  a.class_cost = class_cost; a.bbox_cost = bbox_cost; a.giou_cost = giou_cost;
  a.alpha = alpha; a.one_minus_alpha = (float)(1.0 - (double)alpha); a.gamma = gamma; a.focal = focal;
  a.work = in_lds ? nullptr : (float*)work; a.cost_out = cost_out; a.rows = rows; a.cols = cols; a.kmax = kmax; a.flags = flags;
  hipLaunchKernelGGL(dfine_match_kernel, dim3(B), dim3(MATCH_THREADS), match_lds_bytes(Q, nmax, in_lds), s, a);
  return (int)hipGetLastError();
}

}  // namespace m355
