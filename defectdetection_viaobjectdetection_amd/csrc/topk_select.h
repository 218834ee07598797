// The K greatest of N candidates of one image by one block, in a total order: what dfine_postprocess.hip (candidates = the Q * C
// logits) and dfine_select.hip (candidates = the S token scores) share.  Include from .hip files only.
//
// Every candidate i gets a 32-bit key that orders as the output does: a NaN has the greatest key (torch.topk's order), then
// descending value, -0 == +0.  With more than PP_MAX_K candidates a 4-pass radix select (8 bits per pass, a 256-bin integer
// histogram in LDS) finds the K-th greatest key; what lies above it, and the lowest-index candidates that equal it, are compacted
// into LDS in index order (wave ballots, no atomics); with PP_MAX_K candidates or fewer all of them go to the sort directly.  A
// bitonic sort of the (key, ~index) pairs, which are pairwise distinct, gives the rows: an exact tie goes to the lowest index.
// The histogram's integer atomics only count: no output bit depends on scheduling.
//
// The functions are parameterised on `key_at`, a callable `unsigned key_at(int i)` for 0 <= i < N that returns order_key of
// candidate i; it is called several times per candidate (once per radix pass, twice in the compaction) and must read memory the
// kernel does not write.  All threads of a PP_THREADS block call each function together.
#pragma once
#include "common.h"

namespace m355 {

constexpr int PP_THREADS = 512;
constexpr int PP_WAVES = PP_THREADS / 64;
constexpr int PP_MAX_K = 2048;   // the common limit on K: what the sort holds
// Values crowd into a few exponents, so most lanes of a wave want the same bin, and an LDS atomic serialises over equal
// addresses: every bin has PP_COPIES counters in PP_COPIES banks, one per lane % PP_COPIES, summed when the pass is read.
constexpr int PP_COPIES = 16;
constexpr int PP_UNROLL = 8;   // loads per lane in flight in the passes over all candidates
constexpr unsigned PP_NAN_KEY = 0xffffffffu;

// greater key = earlier row.  No real value has key 0 (its bit pattern would be a NaN's): 0 is the sort's padding.
__device__ __forceinline__ unsigned order_key(float x) {
  if (x != x) return PP_NAN_KEY;
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;   // -0 ties with +0, as the comparison of the values does
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct TopkScratch {                      // one per block, in LDS
  unsigned long long pairs[PP_MAX_K];     // (key << 32) | ~index, sorted descending
  unsigned hist[256 * PP_COPIES];         // [bin][copy]
  int wave_cnt[PP_WAVES][2];              // candidates above / equal to the K-th key that each wave owns
  int sel[2];                             // the pass's bin and how many rows are still to be found inside it
};

// The K-th greatest key of the N candidates (N > K >= 1): returns it, and in `need` how many of the candidates equal to it belong
// to the output.
template <class KeyAt>
__device__ __forceinline__ unsigned radix_select_kth(const KeyAt& key_at, int N, int K, TopkScratch& sm, int& need) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned prefix = 0u, mask = 0u;
  int remaining = K;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int t = tid; t < 256 * PP_COPIES; t += PP_THREADS) sm.hist[t] = 0u;
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += PP_UNROLL * PP_THREADS) {
      unsigned keys[PP_UNROLL];
#pragma unroll
      for (int u = 0; u < PP_UNROLL; ++u) {
        const int i = i0 + u * PP_THREADS + tid;
        const unsigned key = key_at(min(i, N - 1));   // an unconditional load: a branch around it would wait for each one
        keys[u] = i < N ? key : 0u;                   // 0: no candidate
      }
#pragma unroll
      for (int u = 0; u < PP_UNROLL; ++u) {
        const unsigned key = keys[u];
        if (key != 0u && (key & mask) == prefix) atomicAdd(&sm.hist[((key >> shift) & 255u) * PP_COPIES + (lane & (PP_COPIES - 1))], 1u);
      }
    }
    __syncthreads();
    if (wave == 0) {   // lane l owns the bins 255 - 4l .. 252 - 4l: ascending (lane, j) is descending bin
      int c[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = 0;
#pragma unroll
        for (int cp = 0; cp < PP_COPIES; ++cp) c[j] += (int)sm.hist[(255 - (4 * lane + j)) * PP_COPIES + cp];
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
        if (above < remaining && remaining <= above + c[j]) { sm.sel[0] = 255 - (4 * lane + j); sm.sel[1] = remaining - above; }
        above += c[j];
      }
    }
    __syncthreads();
    prefix |= (unsigned)sm.sel[0] << shift;
    mask |= 255u << shift;
    remaining = sm.sel[1];
  }
  need = remaining;
  return prefix;
}

// The candidates above `kth`, then the `need` lowest-index ones equal to it, as pairs in sm.pairs[0, K), each group in index
// order: wave w owns a contiguous run of 64-candidate chunks.
template <class KeyAt>
__device__ __forceinline__ void compact_in_index_order(const KeyAt& key_at, int N, int K, unsigned kth, int need, TopkScratch& sm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunks = (N + 63) >> 6, per_wave = (chunks + PP_WAVES - 1) / PP_WAVES;
  const int c0 = wave * per_wave, c1 = min(c0 + per_wave, chunks);
  int n_gt = 0, n_eq = 0;
  for (int ch = c0; ch < c1; ch += PP_UNROLL) {
    unsigned keys[PP_UNROLL];
#pragma unroll
    for (int u = 0; u < PP_UNROLL; ++u) {
      const int i = (ch + u) * 64 + lane;   // real keys are >= 1: kth is, and 0 (no candidate) is neither above nor equal
      const unsigned key = key_at(min(i, N - 1));
      keys[u] = (ch + u < c1 && i < N) ? key : 0u;
    }
#pragma unroll
    for (int u = 0; u < PP_UNROLL; ++u) {
      n_gt += __popcll(__ballot(keys[u] > kth));
      n_eq += __popcll(__ballot(keys[u] == kth));
    }
  }
  if (lane == 0) { sm.wave_cnt[wave][0] = n_gt; sm.wave_cnt[wave][1] = n_eq; }
  __syncthreads();
  int gt_base = 0, eq_base = 0, gt_total = 0;
#pragma unroll
  for (int w = 0; w < PP_WAVES; ++w) {
    const int g = sm.wave_cnt[w][0], e = sm.wave_cnt[w][1];
    if (w < wave) { gt_base += g; eq_base += e; }
    gt_total += g;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int ch = c0; ch < c1; ch += PP_UNROLL) {
    unsigned keys[PP_UNROLL];
#pragma unroll
    for (int u = 0; u < PP_UNROLL; ++u) {
      const int i = (ch + u) * 64 + lane;
      const unsigned key = key_at(min(i, N - 1));
      keys[u] = (ch + u < c1 && i < N) ? key : 0u;
    }
#pragma unroll
    for (int u = 0; u < PP_UNROLL; ++u) {
      const int i = (ch + u) * 64 + lane;
      const unsigned key = keys[u];
      const bool gt = key > kth, eq = key == kth;
      const unsigned long long mg = __ballot(gt), me = __ballot(eq);
      const unsigned long long pair = ((unsigned long long)key << 32) | (unsigned)~i;
      // the bounds hold by construction (gt_total + need == K); they are kept so that a buffer that changes under the kernel
      // cannot send a store outside the array
      if (gt) {
        const int pos = gt_base + __popcll(mg & below);
        if (pos < K) sm.pairs[pos] = pair;
      }
      if (eq) {
        const int rank = eq_base + __popcll(me & below);
        if (rank < need && gt_total + rank < K) sm.pairs[gt_total + rank] = pair;
      }
      gt_base += __popcll(mg);
      eq_base += __popcll(me);
    }
  }
}

// Bitonic sort of sm.pairs[0, P), P a power of two, descending; the pairs are distinct (the padding zeros compare equal and stay
// where they are).  The caller has put a barrier behind the last write of the pairs.
__device__ __forceinline__ void bitonic_sort_desc(TopkScratch& sm, int P) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += PP_THREADS) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const unsigned long long x = sm.pairs[i], y = sm.pairs[l];
        const bool desc = (i & k) == 0;
        if (desc ? x < y : x > y) { sm.pairs[i] = y; sm.pairs[l] = x; }
      }
      __syncthreads();
    }
  }
}

// sm.pairs[0, K) = the K greatest of the N candidates in output order (1 <= K <= min(N, PP_MAX_K), N < 2^24); row r's candidate
// is ~(unsigned)sm.pairs[r] and its key sm.pairs[r] >> 32.  Ends behind a barrier.
template <class KeyAt>
__device__ __forceinline__ void topk_sorted_pairs(const KeyAt& key_at, int N, int K, TopkScratch& sm) {
  const int tid = threadIdx.x;
  const bool select = N > PP_MAX_K;   // fewer candidates than the sort holds: all of them are sorted, no selection
  const int M = select ? K : N;       // pairs that reach the sort
  int P = 1;
  while (P < M) P <<= 1;
  if (!select) {
    for (int r = tid; r < P; r += PP_THREADS)
      sm.pairs[r] = r < N ? ((unsigned long long)key_at(r) << 32) | (unsigned)~r : 0ull;
  } else {
    for (int r = tid; r < P; r += PP_THREADS) sm.pairs[r] = 0ull;
    int need;
    const unsigned kth = radix_select_kth(key_at, N, K, sm, need);
    compact_in_index_order(key_at, N, K, kth, need, sm);
  }
  __syncthreads();
  bitonic_sort_desc(sm, P);
}

}  // namespace m355
