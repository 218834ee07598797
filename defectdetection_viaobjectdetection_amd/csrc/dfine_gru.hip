// The recurrence of a single-layer GRU with hidden size 256 (the "context aggregator" of the improved temporal D-FINE trainer:
// nn.GRU(256, 256, batch_first, bidirectional) on ONE sequence of T * Q = 15 000 steps), forward and backward, as two persistent
// kernels.  The input projection gi = x W_ih^T + b_ih is the caller's GEMM; these kernels own the serial chain
//   a = W_hh h_{t-1} + b_hh,  r = s(gi_r + a_r),  z = s(gi_z + a_z),  n = tanh(gi_n + r a_n),  h_t = (1 - z) n + z h_{t-1}.
//
// One direction's W_hh is 768 KiB of fp32 and fits in no single CU, so a chain (one sequence, one direction) is split over
// GRU_PARTS = 8 workgroups of 256 threads; each owns 32 hidden units and keeps its 96 KiB slice of W_hh in registers (96 per
// thread) for the whole launch: forward the 96 rows (r, z, n of its units), backward the 32 columns.  Thread (j, c) = (tid / 8,
// tid % 8) serves unit j with segment c of the reduction axis; the 8 partial sums meet in a 3-step xor shuffle, so every sum has
// one fixed order.  Per step the 8 workgroups of a chain exchange the 1 KiB h_t (backward: the 3 KiB gate-gradient vector)
// through global memory as 8-byte {epoch, value} words written and polled with relaxed agent-scope atomics: the word carries its
// own tag, so no flag, fence or ordering between words is needed.  A ring of two slots is enough: a workgroup publishes epoch
// e + 1 only after it has read all of epoch e, which every workgroup published after reading all of epoch e - 1, the previous
// tenant of the slot.  The launcher zeroes the ring on the stream before every launch; epochs start at 1 and count up to S
// (forward: S - 1), below 2^31, so no tag is ever met twice.
//
// Every wait is a bounded spin.  A thread that gives up marks the workgroup (an LDS flag per step parity, set before the
// step's barrier, read after it, and next written two barriers later); after the step's barrier the whole workgroup
// writes NaN to the rest of its outputs, ORs its bit into the caller's status word and returns.  It then publishes nothing, so
// the chain's other workgroups give up at their own bound: the kernel ends on every path.  The grid is at most 128 workgroups of
// 256 threads and 2 KiB / 6 KiB of LDS, resident on any gfx950 whatever the occupancy query says.  Workgroup placement changes
// the speed only: the block index is decoded so that the 8 parts of a chain share blockIdx % 8, the dispatcher's XCD label.
//
// fp32 throughout, no float atomics, bitwise reproducible; chains are independent, so sequence b of a batch has the bits of
// the same sequence alone and the reverse direction has the bits of the forward direction on the flipped sequence.
#include <math.h>

#include "common.h"
#include "launch_util.h"

namespace m355 {
namespace {

constexpr int GH = 256;                    // hidden size
constexpr int GRU_PARTS = 8;               // workgroups per chain
constexpr int GRU_THREADS = 256;           // 32 units x 8 segments
constexpr int GRU_SLOT = 3 * GH;           // words per ring slot (the forward uses the first GH)
constexpr int GRU_RING = 2;
constexpr unsigned GRU_SPIN_LIMIT = 1u << 21;   // polls of one word before giving up (seconds; a step takes microseconds)
constexpr int GRU_MAX_BATCH = 8;               // x 2 directions x GRU_PARTS = 128 workgroups at the most

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) int gi32;

struct GruArgs {
  const float* gi;      // (B, S, D * 3H)
  const float* w_hh;    // (D, 3H, H)
  const float* b_hh;    // (D, 3H)
  const float* h0;      // (D, B, H) or nullptr
  float* out;           // (B, S, D * H)   (backward: read)
  float* h_n;           // (D, B, H)
  float* saved;         // (B * D, S, 4, H): r, z, n, a_n by chain position, or nullptr
  const float* gout;    // backward: (B, S, D * H)
  const float* gh_n;    // backward: (D, B, H) or nullptr
  float* ggi;           // backward: (B, S, D * 3H)
  float* gan;           // backward: (B, S, D * H)
  float* gh0;           // backward: (D, B, H)
  unsigned long long* ring;   // (B * D, GRU_RING, GRU_SLOT)
  int* status;
  int B, S, D;
};

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float sum8(float v) {   // over the 8 lanes of a unit, the same order in every lane
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

__device__ __forceinline__ void publish(gu64* word, unsigned epoch, float v) {
  __hip_atomic_store(word, ((unsigned long long)epoch << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Poll N words (stride GH) until each carries `epoch`; false after GRU_SPIN_LIMIT rounds.  v: the values of the last round.
template <int N>
__device__ __forceinline__ bool await_words(gu64* word, unsigned epoch, float (&v)[N]) {
  for (unsigned spins = 0;; ++spins) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const unsigned long long x = __hip_atomic_load(word + k * GH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v[k] = __uint_as_float((unsigned)x);
      ok = ok && (unsigned)(x >> 32) == epoch;
    }
    if (ok) return true;
    if (spins >= GRU_SPIN_LIMIT) return false;
    __builtin_amdgcn_s_sleep(1);
  }
}

// chain and part of this workgroup; false: a filler block of the grid (nothing to do)
__device__ __forceinline__ bool decode_block(int chains, int& chain, int& part) {
  const int b = blockIdx.x;
  const int row = b >> 3;
  part = row & (GRU_PARTS - 1);
  chain = (b & 7) + 8 * (row >> 3);
  return chain < chains;
}

__device__ __forceinline__ void give_up(int* status, int bit) {
  if (threadIdx.x == 0) __hip_atomic_fetch_or((gi32*)status, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One kernel with and without the saved gates (a.saved == nullptr): the arithmetic is the same instructions either way, so a
// forward that keeps nothing has the bits of one that does.
__global__ __launch_bounds__(GRU_THREADS) void gru_fwd_kernel(GruArgs a) {
  __shared__ __attribute__((aligned(16))) float hvec[2][GH];
  __shared__ int failed[2];   // by step parity: a set for step s + 1 cannot reach a thread that still reads step s's
  int chain, part;
  if (!decode_block(a.B * a.D, chain, part)) return;
  const int B = a.B, S = a.S, D = a.D;
  const int dir = chain % D, bi = chain / D;
  const int tid = threadIdx.x, j = tid >> 3, c = tid & 7;
  const int u = part * 32 + j;

  float w[3][32];
  const float* W = a.w_hh + (size_t)dir * 3 * GH * GH;
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float4 v = *(const float4*)(W + (size_t)(g * GH + u) * GH + c * 32 + 4 * k);
      w[g][4 * k] = v.x; w[g][4 * k + 1] = v.y; w[g][4 * k + 2] = v.z; w[g][4 * k + 3] = v.w;
    }
  const float* bh = a.b_hh + dir * 3 * GH;
  const float br = bh[u], bz = bh[GH + u], bn = bh[2 * GH + u];
  const float* h0 = a.h0 ? a.h0 + ((size_t)dir * B + bi) * GH : nullptr;
  float hprev = h0 ? h0[u] : 0.f;
  hvec[0][tid] = h0 ? h0[tid] : 0.f;
  if (tid < 2) failed[tid] = 0;
  __syncthreads();

  gu64* ring = (gu64*)(a.ring + (size_t)chain * GRU_RING * GRU_SLOT);
  const size_t ldo = (size_t)D * GH, ldg = (size_t)D * 3 * GH;
  float* out = a.out + (size_t)bi * S * ldo + dir * GH + u;
  const float* gi = a.gi + (size_t)bi * S * ldg + dir * 3 * GH + u;
  float* sv = a.saved ? a.saved + (size_t)chain * S * 4 * GH + u : nullptr;

  for (int s = 0; s < S; ++s) {
    const int t = dir ? S - 1 - s : s;
    const float* g = gi + (size_t)t * ldg;
    const float gr = g[0], gz = g[GH], gn = g[2 * GH];   // in flight during the wait
    if (s > 0) {
      float v[1];
      if (!await_words<1>(ring + ((s - 1) & 1) * GRU_SLOT + tid, (unsigned)s, v)) failed[s & 1] = 1;
      hvec[s & 1][tid] = v[0];
      __syncthreads();
      if (failed[s & 1]) {   // uniform: NaN to the rest of this workgroup's outputs, then out
        give_up(a.status, 1);
        if (c == 0) {
          const float nan = __builtin_nanf("");
          for (int s2 = s; s2 < S; ++s2) {
            out[(size_t)(dir ? S - 1 - s2 : s2) * ldo] = nan;
            if (sv)
              for (int q = 0; q < 4; ++q) sv[((size_t)s2 * 4 + q) * GH] = nan;
          }
          a.h_n[((size_t)dir * B + bi) * GH + u] = nan;
        }
        return;
      }
    }
    const float4* hv = (const float4*)&hvec[s & 1][c * 32];
    float sr = 0.f, sz = 0.f, sn = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float4 h = hv[k];
      sr = fmaf(w[0][4 * k], h.x, sr); sr = fmaf(w[0][4 * k + 1], h.y, sr); sr = fmaf(w[0][4 * k + 2], h.z, sr); sr = fmaf(w[0][4 * k + 3], h.w, sr);
      sz = fmaf(w[1][4 * k], h.x, sz); sz = fmaf(w[1][4 * k + 1], h.y, sz); sz = fmaf(w[1][4 * k + 2], h.z, sz); sz = fmaf(w[1][4 * k + 3], h.w, sz);
      sn = fmaf(w[2][4 * k], h.x, sn); sn = fmaf(w[2][4 * k + 1], h.y, sn); sn = fmaf(w[2][4 * k + 2], h.z, sn); sn = fmaf(w[2][4 * k + 3], h.w, sn);
    }
    const float r = sigmoidf(gr + (sum8(sr) + br));
    const float z = sigmoidf(gz + (sum8(sz) + bz));
    const float an = sum8(sn) + bn;
    const float n = tanhf(gn + r * an);
    const float h = (1.f - z) * n + z * hprev;
    hprev = h;
    if (c == 0) out[(size_t)t * ldo] = h;
    else if (c == 1) { if (s + 1 < S) publish(ring + (s & 1) * GRU_SLOT + u, (unsigned)s + 1, h); }
    else if (sv && c < 6) sv[((size_t)s * 4 + (c - 2)) * GH] = c == 2 ? r : c == 3 ? z : c == 4 ? n : an;
  }
  if (c == 0) a.h_n[((size_t)dir * B + bi) * GH + u] = hprev;
}

// Reverse-time chain.  Step k handles chain position s = S - 1 - k: with dh = grad_out + z' dh' + W_hh^T ga' (primes: the step
// before, one position later),
//   d_n = dh (1 - z) (1 - n^2), d_z = dh (h_prev - n) z (1 - z), d_r = d_n a_n r (1 - r);  grad_gi = (d_r, d_z, d_n),
//   ga = (d_r, d_z, d_n r) is what W_hh sees: exchanged, and its n-part written to grad_an.
__global__ __launch_bounds__(GRU_THREADS) void gru_bwd_kernel(GruArgs a) {
  __shared__ __attribute__((aligned(16))) float gvec[2][GRU_SLOT];
  __shared__ int failed[2];   // by step parity: a set for step s + 1 cannot reach a thread that still reads step s's
  int chain, part;
  if (!decode_block(a.B * a.D, chain, part)) return;
  const int B = a.B, S = a.S, D = a.D;
  const int dir = chain % D, bi = chain / D;
  const int tid = threadIdx.x, j = tid >> 3, c = tid & 7;
  const int u = part * 32 + j;

  float w[96];   // column u of W_hh, rows 96 c .. 96 c + 95
  const float* W = a.w_hh + (size_t)dir * 3 * GH * GH + u;
#pragma unroll
  for (int i = 0; i < 96; ++i) w[i] = W[(size_t)(c * 96 + i) * GH];
  const size_t hoff = ((size_t)dir * B + bi) * GH + u;
  const float h0 = a.h0 ? a.h0[hoff] : 0.f;
  float carry = a.gh_n ? a.gh_n[hoff] : 0.f;   // dh' z' of the step before
  if (tid < 2) failed[tid] = 0;
  __syncthreads();

  gu64* ring = (gu64*)(a.ring + (size_t)chain * GRU_RING * GRU_SLOT);
  const size_t ldo = (size_t)D * GH, ldg = (size_t)D * 3 * GH;
  const float* gout = a.gout + (size_t)bi * S * ldo + dir * GH + u;
  const float* outc = a.out + (size_t)bi * S * ldo + dir * GH + u;
  const float* sv = a.saved + (size_t)chain * S * 4 * GH + u;
  float* ggi = a.ggi + (size_t)bi * S * ldg + dir * 3 * GH + u;
  float* gan = a.gan + (size_t)bi * S * ldo + dir * GH + u;

  for (int k = 0; k <= S; ++k) {   // k == S: only the last product, for grad_h0
    const int s = S - 1 - k;
    const int t = dir ? S - 1 - s : s;
    float go = 0.f, r = 0.f, z = 0.f, n = 0.f, an = 0.f, hp = 0.f;
    if (k < S) {   // in flight during the wait
      go = gout[(size_t)t * ldo];
      const float* q = sv + (size_t)s * 4 * GH;
      r = q[0]; z = q[GH]; n = q[2 * GH]; an = q[3 * GH];
      hp = s > 0 ? outc[(size_t)(dir ? t + 1 : t - 1) * ldo] : h0;
    }
    float dot = 0.f;
    if (k > 0) {
      float v[3];
      if (!await_words<3>(ring + ((k - 1) & 1) * GRU_SLOT + tid, (unsigned)k, v)) failed[k & 1] = 1;
      float* gv = gvec[k & 1];
      gv[tid] = v[0]; gv[GH + tid] = v[1]; gv[2 * GH + tid] = v[2];
      __syncthreads();
      if (failed[k & 1]) {
        give_up(a.status, 2);
        const float nan = __builtin_nanf("");
        if (c == 0) {
          for (int k2 = k; k2 < S; ++k2) {
            const int s2 = S - 1 - k2, t2 = dir ? S - 1 - s2 : s2;
            for (int g = 0; g < 3; ++g) ggi[(size_t)t2 * ldg + g * GH] = nan;
            gan[(size_t)t2 * ldo] = nan;
          }
          a.gh0[hoff] = nan;
        }
        return;
      }
      const float4* g4 = (const float4*)(gv + c * 96);
      float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;   // four chains of 24 products, then one fixed tree
#pragma unroll
      for (int i = 0; i < 24; ++i) {
        const float4 x = g4[i];
        d0 = fmaf(w[4 * i], x.x, d0); d1 = fmaf(w[4 * i + 1], x.y, d1); d2 = fmaf(w[4 * i + 2], x.z, d2); d3 = fmaf(w[4 * i + 3], x.w, d3);
      }
      dot = sum8((d0 + d1) + (d2 + d3));
    }
    const float dh = go + (carry + dot);
    if (k == S) {
      if (c == 0) a.gh0[hoff] = carry + dot;
      break;
    }
    const float dn = dh * (1.f - z) * (1.f - n * n);
    const float dz = dh * (hp - n) * z * (1.f - z);
    const float dr = dn * an * r * (1.f - r);
    const float da = dn * r;
    carry = dh * z;
    gu64* slot = ring + (k & 1) * GRU_SLOT + u;
    switch (c) {
      case 0: ggi[(size_t)t * ldg] = dr; break;
      case 1: ggi[(size_t)t * ldg + GH] = dz; break;
      case 2: ggi[(size_t)t * ldg + 2 * GH] = dn; break;
      case 3: gan[(size_t)t * ldo] = da; break;
      case 4: publish(slot, (unsigned)k + 1, dr); break;
      case 5: publish(slot + GH, (unsigned)k + 1, dz); break;
      case 6: publish(slot + 2 * GH, (unsigned)k + 1, da); break;
      default: break;
    }
  }
}

size_t ring_bytes(int B, int D) { return (size_t)B * D * GRU_RING * GRU_SLOT * sizeof(unsigned long long); }

GruArgs gru_args(void* work, int B, int S, int D, bool with_saved) {
  GruArgs a{};
  a.ring = (unsigned long long*)work;
  a.saved = with_saved ? (float*)((char*)work + ring_bytes(B, D)) : nullptr;
  a.B = B; a.S = S; a.D = D;
  return a;
}

dim3 gru_grid(int B, int D) { return dim3(64 * ((B * D + 7) / 8)); }   // 64 or 128 workgroups

}  // namespace

const char* dfine_gru_check(int B, long S, int H, int D) {
  if (H != GH) return "hidden size must be 256";
  if (D != 1 && D != 2) return "directions must be 1 or 2";
  if (B < 1 || B > GRU_MAX_BATCH) return "B must be in [1, 8]";
  if (S < 1 || S > (1L << 24)) return "S must be in [1, 2^24]";
  return nullptr;
}

size_t dfine_gru_workspace_bytes(int B, long S, int H, int D) {
  if (S < 0 || dfine_gru_check(B, S > 0 ? S : 1, H, D)) return 0;
  return ring_bytes(B, D) + (size_t)B * D * S * 4 * GH * sizeof(float);
}

int launch_dfine_gru_forward(const float* gi, const float* w_hh, const float* b_hh, const float* h0, int B, int S, int D, float* out,
                             float* h_n, void* work, bool keep, int* status, hipStream_t s) {
  GruArgs a = gru_args(work, B, S, D, keep);
  a.gi = gi; a.w_hh = w_hh; a.b_hh = b_hh; a.h0 = h0; a.out = out; a.h_n = h_n; a.status = status;
  int rc = (int)hipMemsetAsync(work, 0, ring_bytes(B, D), s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(gru_fwd_kernel, gru_grid(B, D), dim3(GRU_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

int launch_dfine_gru_backward(const float* gout, const float* gh_n, const float* w_hh, const float* h0, const float* out, int B, int S,
                              int D, float* ggi, float* gan, float* gh0, void* work, int* status, hipStream_t s) {
  GruArgs a = gru_args(work, B, S, D, true);
  a.gout = gout; a.gh_n = gh_n; a.w_hh = w_hh; a.h0 = h0; a.out = const_cast<float*>(out); a.ggi = ggi; a.gan = gan; a.gh0 = gh0;
  a.status = status;
  int rc = (int)hipMemsetAsync(work, 0, ring_bytes(B, D), s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(gru_bwd_kernel, gru_grid(B, D), dim3(GRU_THREADS), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace m355
