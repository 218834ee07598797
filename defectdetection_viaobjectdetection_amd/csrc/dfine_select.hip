// D-FINE encoder query selection (transformers 5.15.0 modeling_d_fine.py:1804-1828, the block of DFineModel.forward between the
// hybrid encoder's heads and the decoder): the K = num_queries tokens with the greatest class score, and the rows of the coordinate
// logits, the class logits and the encoder memory at those tokens.
//
// Forward, two launches:
//   dfine_token_scores_kernel   a grid over all CUs: the row max over C of class_logits (B, S, C) into the (B, S) workspace, NaN if
//                               the row holds one (torch.max).  L = the power of two >= the row's loads lanes share a row; 16-byte
//                               loads when the base is 16-byte aligned and C % 4 == 0, 4-byte loads otherwise.
//   dfine_select_gather_kernel  one block per image: the top K of its S scores (topk_select.h: NaN first, descending score,
//                               -0 == +0, an exact tie to the lowest token), the token indices, the gathered rows (copies, bit for
//                               bit), sigmoid of the coordinate rows and, for a backward, the inverse map (B, S): rank or -1.
// Backward, one launch: every input gradient is written completely in one streaming pass through the inverse map; a selected
// token's row is its rank's gradient row, any other row is zero.  The tokens of an image are distinct: nothing is summed, so
// there is no memset, no atomic and no scatter.  The select's integer LDS histogram counters are the file's only atomics.
// The launchers validate nothing (dfine_entries.hip does).
// This file is compiled with -ffp-contract=off: the coordinate gradient is torch's expression, one rounding per operation.
#include <math.h>

#include "common.h"
#include "launch_util.h"
#include "topk_select.h"

namespace m355 {
namespace {

constexpr int SC_THREADS = 256, SC_WAVES = SC_THREADS / 64;
constexpr int SC_ROWS = 4;       // rows per lane group in flight in the score kernel
constexpr int GATHER_ROWS = 8;   // rows per wave in flight in the gather

// max that keeps a NaN, as torch.max does; symmetric in NaN-ness, so every lane of a butterfly ends with a NaN or with the max
__device__ __forceinline__ float nanmax(float a, float b) { return a != a ? a : ((b != b || b > a) ? b : a); }
__device__ __forceinline__ float nanmax(float a, float4v v) { return nanmax(nanmax(nanmax(nanmax(a, v[0]), v[1]), v[2]), v[3]); }


// T = float4v: 16-byte loads (cls 16-byte aligned, C % 4 == 0), T = float: 4-byte loads.  units = loads per row, L = lanes per row.
template <class T>
__global__ __launch_bounds__(SC_THREADS) void dfine_token_scores_kernel(const float* __restrict__ cls, long rows, int C, int units,
                                                                         int L, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63, sub = lane & (L - 1), tok = lane / L, G = 64 / L;
  const long wave = (long)blockIdx.x * SC_WAVES + (threadIdx.x >> 6), nwaves = (long)gridDim.x * SC_WAVES;
  const long step = (long)G * SC_ROWS;
  for (long r0 = wave * step; r0 < rows; r0 += nwaves * step) {
    float m[SC_ROWS];
#pragma unroll
    for (int u = 0; u < SC_ROWS; ++u) m[u] = -INFINITY;
    for (int c = sub; c < units; c += L) {   // one trip when units <= 64
      T v[SC_ROWS];
#pragma unroll
      for (int u = 0; u < SC_ROWS; ++u) {    // unconditional loads of a clamped row: all SC_ROWS are in flight together
        const long row = min(r0 + (long)u * G + tok, rows - 1);
        v[u] = ((const T*)(cls + (size_t)row * C))[c];
      }
#pragma unroll
      for (int u = 0; u < SC_ROWS; ++u) m[u] = nanmax(m[u], v[u]);
    }
#pragma unroll
    for (int u = 0; u < SC_ROWS; ++u) {
      float x = m[u];
      for (int o = L >> 1; o > 0; o >>= 1) x = nanmax(x, __shfl_xor(x, o, 64));
      const long row = r0 + (long)u * G + tok;
      if (sub == 0 && row < rows) scores[row] = x;
    }
  }
}

struct SelectArgs {
  const float* cls;      // (B, S, C)
  const float* coord;    // (B, S, 4)
  const float* mem;      // (B, S, D) or nullptr
  const float* scores;   // (B, S): what dfine_token_scores_kernel wrote
  int S, C, D, K;
  int vec_c, vec_d;      // 16-byte copies of the class / memory rows: both bases 16-byte aligned and the width a multiple of 4
  long long* indices;    // (B, K)
  float* ref;            // (B, K, 4)
  float* boxes;          // (B, K, 4)
  float* logits;         // (B, K, C)
  float* target;         // (B, K, D) or nullptr
  int* inverse;          // (B, S) or nullptr
};

// rows tok[0 .. GATHER_ROWS) of src (n floats each) to rows r0 .. of dst, those below K; all loads before the first store
template <class T>
__device__ __forceinline__ void gather_rows(const float* __restrict__ src, float* __restrict__ dst, const int (&tok)[GATHER_ROWS], int r0,
                                            int K, int n, int lane) {
  const int units = n / (int)(sizeof(T) / sizeof(float));
  for (int u = lane; u < units; u += 64) {
    T v[GATHER_ROWS];
#pragma unroll
    for (int j = 0; j < GATHER_ROWS; ++j) v[j] = ((const T*)(src + (size_t)tok[j] * n))[u];
#pragma unroll
    for (int j = 0; j < GATHER_ROWS; ++j)
      if (r0 + j < K) ((T*)(dst + (size_t)(r0 + j) * n))[u] = v[j];
  }
}

__global__ __launch_bounds__(PP_THREADS) void dfine_select_gather_kernel(const SelectArgs a) {
  __shared__ TopkScratch sm;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S, K = a.K, C = a.C, D = a.D;
  const float* sc = a.scores + (size_t)b * S;
  int* inv = a.inverse ? a.inverse + (size_t)b * S : nullptr;
  if (inv)   // the ranks are written behind the selection's barriers: ordered after this fill for the whole block
    for (int i = tid; i < S; i += PP_THREADS) inv[i] = -1;
  topk_sorted_pairs([sc](int i) { return order_key(sc[i]); }, S, K, sm);

  for (int r = tid; r < K; r += PP_THREADS) {
    unsigned i = ~(unsigned)sm.pairs[r];
    if (i >= (unsigned)S) i = (unsigned)S - 1u;   // never taken: see the compaction's bounds
    a.indices[(size_t)b * K + r] = (long long)i;
    if (inv) inv[i] = r;
  }
  const float* cls = a.cls + (size_t)b * S * C;
  const float* coord = a.coord + (size_t)b * S * 4;
  float* logits = a.logits + (size_t)b * K * C;
  for (int r0 = wave * GATHER_ROWS; r0 < K; r0 += PP_WAVES * GATHER_ROWS) {
    int tok[GATHER_ROWS];
#pragma unroll
    for (int j = 0; j < GATHER_ROWS; ++j) {
      const unsigned i = ~(unsigned)sm.pairs[min(r0 + j, K - 1)];
      tok[j] = (int)min(i, (unsigned)S - 1u);
    }
    if (lane < 4 * GATHER_ROWS && r0 + (lane >> 2) < K) {   // lane = 4 j + side; scalar accesses: a view need not be 16-byte aligned
      const int r = r0 + (lane >> 2), side = lane & 3;
      const unsigned i = min(~(unsigned)sm.pairs[r], (unsigned)S - 1u);
      const float x = coord[(size_t)i * 4 + side];
      const size_t o = ((size_t)b * K + r) * 4 + side;
      a.ref[o] = x;
      a.boxes[o] = 1.f / (1.f + expf(-x));
    }
    if (a.vec_c) gather_rows<float4v>(cls, logits, tok, r0, K, C, lane);
    else gather_rows<float>(cls, logits, tok, r0, K, C, lane);
    if (a.mem) {
      const float* mem = a.mem + (size_t)b * S * D;
      float* target = a.target + (size_t)b * K * D;
      if (a.vec_d) gather_rows<float4v>(mem, target, tok, r0, K, D, lane);
      else gather_rows<float>(mem, target, tok, r0, K, D, lane);
    }
  }
}

struct SelectBwdArgs {
  const float *g_ref, *g_boxes;   // (B, K, 4), each may be nullptr
  const float* g_logits;          // (B, K, C) or nullptr
  const float* g_target;          // (B, K, D) or nullptr
  const float* boxes;             // (B, K, 4): the forward's sigmoid (read with g_boxes only)
  const int* inverse;             // (B, S)
  long rows;                      // B * S
  int S, K, C, D;
  int vec_c, vec_d, Lc, Ld;       // as in the forward; lanes per row of the class / memory gradient
  float *d_cls, *d_coord, *d_mem; // (B, S, C), (B, S, 4), (B, S, D), each may be nullptr
};

// the 64 rows row0 .. of dst (n floats each): row t is row srow_t of g when srow_t >= 0 (srow: lane t's value), else zero.
// L lanes share a row and 64 / L rows are written per step, so a wave's stores are one ascending run of addresses.
template <class T>
__device__ __forceinline__ void spread_rows(float* __restrict__ dst, const float* __restrict__ g, int n, int L, long row0, long rows,
                                            int srow, int lane) {
  const int units = n / (int)(sizeof(T) / sizeof(float));
  const int sub = lane & (L - 1), tok = lane / L, G = 64 / L;
  for (int t = tok; t < 64; t += G) {   // L trips for every lane: the whole wave is at each shuffle
    const int sr = __shfl(srow, t, 64);
    const long row = row0 + t;
    if (row < rows) {
      T* out = (T*)(dst + (size_t)row * n);
      if (sr >= 0) {
        const T* in = (const T*)(g + (size_t)sr * n);
        for (int u = sub; u < units; u += L) out[u] = in[u];
      } else {
        for (int u = sub; u < units; u += L) out[u] = T{};
      }
    }
  }
}

__global__ __launch_bounds__(SC_THREADS) void dfine_select_backward_kernel(const SelectBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * SC_WAVES + (threadIdx.x >> 6), nwaves = (long)gridDim.x * SC_WAVES;
  for (long row0 = wave * 64; row0 < a.rows; row0 += nwaves * 64) {
    const long row = row0 + lane;
    const int r = row < a.rows ? a.inverse[row] : -1;
    const int srow = (r >= 0 && r < a.K) ? (int)(row / a.S) * a.K + r : -1;   // B * K < 2^31 (the entry's limit on B * S)
    if (a.d_coord && row < a.rows) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = 0.f;
        if (srow >= 0) {
          if (a.g_ref) v = a.g_ref[(size_t)srow * 4 + j];
          if (a.g_boxes) {
            const float bx = a.boxes[(size_t)srow * 4 + j];
            v += a.g_boxes[(size_t)srow * 4 + j] * (1.f - bx) * bx;   // torch's sigmoid backward, its order
          }
        }
        a.d_coord[(size_t)row * 4 + j] = v;
      }
    }
    if (a.d_cls) {
      const int s = a.g_logits ? srow : -1;
      if (a.vec_c) spread_rows<float4v>(a.d_cls, a.g_logits, a.C, a.Lc, row0, a.rows, s, lane);
      else spread_rows<float>(a.d_cls, a.g_logits, a.C, a.Lc, row0, a.rows, s, lane);
    }
    if (a.d_mem) {
      const int s = a.g_target ? srow : -1;
      if (a.vec_d) spread_rows<float4v>(a.d_mem, a.g_target, a.D, a.Ld, row0, a.rows, s, lane);
      else spread_rows<float>(a.d_mem, a.g_target, a.D, a.Ld, row0, a.rows, s, lane);
    }
  }
}

int grid_for(long waves_of_work) {   // blocks of SC_WAVES waves: enough to cover the work, 16 per CU at the most
  const int cus = num_cus();
  if (cus <= 0) return -1;
  const long need = (waves_of_work + SC_WAVES - 1) / SC_WAVES, cap = (long)cus * 16;
  return (int)(need < 1 ? 1 : (need < cap ? need : cap));
}

}  // namespace

size_t dfine_select_workspace_bytes(int B, int S) { return (size_t)B * (size_t)S * sizeof(float); }

int launch_dfine_select_forward(const float* cls, const float* coord, const float* mem, int B, int S, int C, int D, int K, float* scores,
                                long long* indices, float* ref, float* boxes, float* logits, float* target, int* inverse, hipStream_t s) {
  const long rows = (long)B * S;
  const bool vec = aligned16(cls) && C % 4 == 0;
  const int units = vec ? C / 4 : C, L = lanes_per_row(units);
  const int grid = grid_for((rows + (64 / L) * SC_ROWS - 1) / ((64 / L) * SC_ROWS));
  if (grid < 0) return -2;
  if (vec) hipLaunchKernelGGL(dfine_token_scores_kernel<float4v>, dim3(grid), dim3(SC_THREADS), 0, s, cls, rows, C, units, L, scores);
  else hipLaunchKernelGGL(dfine_token_scores_kernel<float>, dim3(grid), dim3(SC_THREADS), 0, s, cls, rows, C, units, L, scores);
  SelectArgs a{};
  a.cls = cls; a.coord = coord; a.mem = mem; a.scores = scores; a.S = S; a.C = C; a.D = mem ? D : 0; a.K = K;
  a.vec_c = vec && aligned16(logits);
  a.vec_d = mem && aligned16(mem) && aligned16(target) && D % 4 == 0;
  a.indices = indices; a.ref = ref; a.boxes = boxes; a.logits = logits; a.target = mem ? target : nullptr; a.inverse = inverse;
  hipLaunchKernelGGL(dfine_select_gather_kernel, dim3(B), dim3(PP_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_select_backward(const float* g_ref, const float* g_boxes, const float* g_logits, const float* g_target, const float* boxes,
                                 const int* inverse, int B, int S, int C, int D, int K, float* d_cls, float* d_coord, float* d_mem,
                                 hipStream_t s) {
  SelectBwdArgs a{};
  a.g_ref = g_ref; a.g_boxes = g_boxes; a.g_logits = g_logits; a.g_target = g_target; a.boxes = boxes; a.inverse = inverse;
  a.rows = (long)B * S; a.S = S; a.K = K; a.C = C; a.D = D;
  a.vec_c = C % 4 == 0 && aligned16(d_cls) && aligned16(g_logits);   // nullptr counts as aligned: it is not read
  a.vec_d = D % 4 == 0 && aligned16(d_mem) && aligned16(g_target);
  a.Lc = lanes_per_row(a.vec_c ? C / 4 : C);
  a.Ld = lanes_per_row(a.vec_d ? D / 4 : D);
  a.d_cls = d_cls; a.d_coord = d_coord; a.d_mem = d_mem;
  const int grid = grid_for((a.rows + 63) / 64);
  if (grid < 0) return -2;
  hipLaunchKernelGGL(dfine_select_backward_kernel, dim3(grid), dim3(SC_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace m355
