// The quality head (DFineLQE) of a D-FINE decoder layer (transformers' DFineDecoderLayer):
//   lqe_fwd / lqe_bwd           per box side: softmax over the bins + 1 logits, the k largest probabilities, their mean
// (the layer's two LayerNorms, the gate and LayerNorm(clamp(x + y)), are sources of the row-LayerNorm kernels in dfine_rowln.hip.)
// fp32 in, fp32 out, fp32 accumulation; no float atomics: every sum has one owner and a fixed order, so results and gradients
// are bitwise reproducible.  Both kernels are row-wise: a row's result does not depend on the batch around it, no workgroup
// waits on another, no barrier.
//
// One wave per (row, side), lane i holds bin i (bins + 1 <= 64).  The k rounds of the selection are wave-wide arg-max
// butterflies over (probability, bin) pairs that prefer the lower bin on an exact tie; every lane ends with the same pair.
#include <math.h>

#include "common.h"
#include "device_prims.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int LQ_THREADS = 256;   // four waves: the four sides of one row

struct LqeArgs {
  const float* corners;       // (M, 4 nb1)
  float* stat;                // forward: (M, 4 (k + 1)): per side the k probabilities in descending order, then their mean
  unsigned char* idx;         // forward: (M, 4, k) chosen bins, or nullptr; the backward reads it
  const float* gstat;         // backward: (M, 4 (k + 1))
  float* gcorners;            // backward: (M, 4 nb1)
  long M;
  int nb1, k;
};

// softmax over the nb1 logits of (row, side), bin `lane` in lane `lane`; 0 in the lanes past nb1.  Forward and backward call
// this one function: the backward's probabilities have the forward's bits.
__device__ __forceinline__ float lqe_prob(const float* corners, long rs, int nb1, int lane) {
  const bool live = lane < nb1;
  const float x = live ? corners[rs * nb1 + lane] : -INFINITY;
  const float mx = wave_max(x);
  const float e = live ? expf(x - mx) : 0.f;
  return e / wave_sum(e);
}

__global__ __launch_bounds__(LQ_THREADS) void lqe_fwd_kernel(const LqeArgs a) {
  const int lane = threadIdx.x & 63;
  const long rs = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // (row, side); the grid is exactly M blocks
  const float p = lqe_prob(a.corners, rs, a.nb1, lane);
  float v = lane < a.nb1 ? p : -1.f;                           // -1: not a candidate (past the bins, or already taken)
  float sum = 0.f, mine = 0.f;
  int mine_i = 0;
  for (int j = 0; j < a.k; ++j) {                              // k <= nb1: a live candidate is left in every round
    float bv = v;
    int bi = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == bi) v = -1.f;
    sum += bv;
    if (lane == j) { mine = bv; mine_i = bi; }
  }
  float* st = a.stat + rs * (a.k + 1);
  if (lane < a.k) {
    st[lane] = mine;
    if (a.idx) a.idx[rs * a.k + lane] = (unsigned char)mine_i;
  }
  if (lane == a.k) st[a.k] = sum / (float)a.k;
}

// d logits = p * (dp - sum(dp * p)), dp_i = sum over the chosen slots j with bin i of (gstat_j + gstat_mean / k)
__global__ __launch_bounds__(LQ_THREADS) void lqe_bwd_kernel(const LqeArgs a) {
  const int lane = threadIdx.x & 63;
  const long rs = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const float p = lqe_prob(a.corners, rs, a.nb1, lane);
  const float* gs = a.gstat + rs * (a.k + 1);
  const float gm = gs[a.k] / (float)a.k;
  float dp = 0.f;
  for (int j = 0; j < a.k; ++j)
    if ((int)a.idx[rs * a.k + j] == lane) dp += gs[j] + gm;    // the k bins of a side are distinct: at most one term per lane
  const float dot = wave_sum(dp * p);
  if (lane < a.nb1) a.gcorners[rs * a.nb1 + lane] = p * (dp - dot);
}

}  // namespace

int launch_dfine_lqe_forward(const float* corners, long M, int nb1, int k, float* stat, unsigned char* idx, hipStream_t s) {
  LqeArgs a{};
  a.corners = corners; a.stat = stat; a.idx = idx; a.M = M; a.nb1 = nb1; a.k = k;
  hipLaunchKernelGGL(lqe_fwd_kernel, dim3((unsigned)M), dim3(LQ_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_lqe_backward(const float* gstat, const float* corners, const unsigned char* idx, long M, int nb1, int k,
                              float* gcorners, hipStream_t s) {
  LqeArgs a{};
  a.corners = corners; a.gstat = gstat; a.idx = const_cast<unsigned char*>(idx); a.gcorners = gcorners; a.M = M; a.nb1 = nb1; a.k = k;
  hipLaunchKernelGGL(lqe_bwd_kernel, dim3((unsigned)M), dim3(LQ_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace m355
