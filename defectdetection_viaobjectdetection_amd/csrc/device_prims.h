// Device primitives shared by the kernel files (gfx950 only).  Include from .hip files only.
// One definition each: a kernel file whose helper differs keeps it locally under a name that says how.
#pragma once
#include "common.h"

namespace m355 {

typedef float float16v __attribute__((ext_vector_type(16)));   // the accumulator of one 32x32 MFMA

// ---- LDS-DMA: 16 (4) bytes per lane straight from memory into LDS, lane-linear at the wave-uniform LDS address
// buffer form: descriptor + per-lane byte offset voff + wave-uniform byte offset soff (out-of-range lanes read zeros)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff, char* lds) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
}
// global form (global_load_lds_dwordx4 / _dword): per-lane SOURCE address, no bound
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}
__device__ __forceinline__ void glds4(const void* gsrc, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 0);
}

// s_waitcnt immediate (gfx9 encoding): vmcnt(n) lgkmcnt(0), expcnt untouched.  The builtin (unlike inline asm) is
// visible to the compiler's own wait-count insertion, which then does not re-wait for LDS reads issued before it.
#define WAITCNT_VM_LGKM0(n) ((((n) & 0xf) | (((n) >> 4) << 14) | (7 << 4)))

__device__ __forceinline__ int lane_id() {            // volatile: lane-derived values are rebuilt where they are used, not kept
  int ln;                                             // live (= spilled) across the K loop; a scratch reload waits on vmcnt(0)
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
  return ln;
}

// q = n / d, r = n % d for 0 <= n < 2^24 via a float reciprocal estimate + exact integer correction.
__device__ __forceinline__ void fast_divmod(int n, int d, float inv_d, int& q, int& r) {
  q = (int)((float)n * inv_d);
  r = n - q * d;
  if (r < 0) { r += d; --q; }
  if (r >= d) { r -= d; ++q; }
}

// ---- weight-row order of a 32x32x16 MFMA
// MFMA row rho = 8 q + 4 h + i is accumulator register 4 q + i of lane-half h.
// Plain order: lane-half h's 16 registers are 16 consecutive channels 16 h + r (what a 16-byte NHWC store wants).
__device__ __forceinline__ int row_plain(int rho) { return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3); }
// Operand order: register r of lane-half h is channel 16 (r >> 3) + 8 h + (r & 7), so that registers 8 s .. 8 s + 7,
// converted to fp16, ARE the B fragment (K slice s, k = 16 s + 8 h + j) of the next 32x32x16 MFMA for the same pixels.
__device__ __forceinline__ int row_operand(int rho) {
  const int q = rho >> 3, h = (rho >> 2) & 1, i = rho & 3;
  return 16 * (q >> 1) + 8 * h + 4 * (q & 1) + i;
}

// ---- wave-wide xor butterflies: every lane ends with the same bits (a + b == b + a at each step)
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
  return x;
}
__device__ __forceinline__ int wave_sum_int(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// ---- torch.nan_to_num(v, nan, posinf, neginf): a finite v passes unchanged
__device__ __forceinline__ float nan_to_num(float v, float nan, float posinf, float neginf) {
  return v != v ? nan : (v == __builtin_inff() ? posinf : (v == -__builtin_inff() ? neginf : v));
}

// ---- dropout keep-mask: a pure function of (seed, site, flat element index), nothing stored (dfine_encoder.hip, dfine_rowln.hip)
// Philox4x32-10 (Salmon et al., SC'11; Random123's constants and round): counter c[0..3], key (k0, k1), result in c.
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned lo0 = c[0] * 0xD2511F53u, hi0 = __umulhi(c[0], 0xD2511F53u);
    const unsigned lo1 = c[2] * 0xCD9E8D57u, hi1 = __umulhi(c[2], 0xCD9E8D57u);
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// What a dropout site of a kernel needs: thr = floor(p * 2^32), scale = 1 / (1 - p); element e is kept when its word >= thr.
struct DropArgs {
  unsigned long long seed;
  unsigned site, thr;
  float scale;
};
inline DropArgs drop_args(float p, unsigned long long seed, int site) {
  DropArgs d{};
  d.seed = seed;
  d.site = (unsigned)site;
  d.thr = (unsigned)((double)p * 4294967296.0);   // p in [0, 1): below 2^32
  d.scale = (float)(1.0 / (1.0 - (double)p));
  return d;
}
// The ONE definition of the mask: bit e (0..3) of the result is set when element 4 * group + e of the site's tensor (flat,
// row-major index) is kept.  counter = (group lo, group hi, site, 0), key = (seed lo, seed hi): one Philox call per 4 elements.
__device__ __forceinline__ unsigned dropout_keep4(const DropArgs& d, unsigned long long group) {
  unsigned c[4] = {(unsigned)group, (unsigned)(group >> 32), d.site, 0u};
  philox4x32_10(c, (unsigned)d.seed, (unsigned)(d.seed >> 32));
  return (unsigned)(c[0] >= d.thr) | ((unsigned)(c[1] >= d.thr) << 1) | ((unsigned)(c[2] >= d.thr) << 2) |
         ((unsigned)(c[3] >= d.thr) << 3);
}

// ---- probe instances: in-kernel stamps and timing ablations
// A kernel that can stamp or ablate takes one template parameter `bool PROBE`.  Production is PROBE = false: the helpers below are
// then empty (no members, every method an empty inline) and `probe_bit<false>` is the constant false, so the instance holds no
// clock read, no stamp store and no ablation branch.  The launcher starts the PROBE = true instance exactly when a stamp buffer
// or an ablation bit (the table at ConvArgs::dbg, common.h) is set.  A call site reads the same in both instances.
template <bool PROBE>
__device__ __forceinline__ bool probe_bit(int dbg, int bits) { return PROBE && (dbg & bits); }

// Per-wave section accumulator: mark(k) adds the cycles since the last mark to section k.
template <bool PROBE, int N>
struct SectionClock {
  __device__ __forceinline__ explicit SectionClock(const unsigned long long*) {}
  __device__ __forceinline__ unsigned long long start() { return 0; }
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ unsigned long long now() const { return 0; }
  __device__ __forceinline__ unsigned long long realtime() const { return 0; }
  __device__ __forceinline__ void flush(unsigned long long*, int, int, unsigned long long = 0, unsigned long long = 0) {}
};
template <int N>
struct SectionClock<true, N> {
  static_assert(N <= 8, "a record is 8 words");
  unsigned long long acc[N] = {}, last = 0;
  bool on;                                             // false: an ablation-only launch of the probe instance, nothing is stamped
  __device__ __forceinline__ explicit SectionClock(const unsigned long long* out) : on(out != nullptr) {}
  __device__ __forceinline__ unsigned long long start() { return last = now(); }   // the clock the first section is counted from
  __device__ __forceinline__ void mark(int k) {
    if (on) {
      __builtin_amdgcn_sched_barrier(0);
      const unsigned long long tn = __builtin_amdgcn_s_memtime();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      acc[k] += tn - last;
      last = tn;
    }
  }
  __device__ __forceinline__ unsigned long long now() const { return on ? __builtin_amdgcn_s_memtime() : 0; }
  __device__ __forceinline__ unsigned long long realtime() const { return on ? __builtin_amdgcn_s_memrealtime() : 0; }   // 100 MHz
  // record (block, wave) of `waves` per block, 8 words: the N sections, then `extra` in the last word (N = 7) or the last two (N = 6)
  __device__ __forceinline__ void flush(unsigned long long* out, int waves, int wave, unsigned long long extra = 0,
                                        unsigned long long extra2 = 0) {
    if (!on || (threadIdx.x & 63)) return;
    unsigned long long* o = out + ((long)blockIdx.x * waves + wave) * 8;
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = acc[k];
    if (N == 6) { o[6] = extra; o[7] = extra2; }
    if (N == 7) o[7] = extra;
  }
};

// Point stamps: the clock at NA named points of the first tile of a block (point 0 = kernel entry, the last one = the flush) and
// at NB points of a later tile, plus the 100 MHz realtime at entry and at the flush.
template <bool PROBE, int NA = 4, int NB = 0>
struct BlockStamps {
  __device__ __forceinline__ explicit BlockStamps(unsigned long long*) {}
  __device__ __forceinline__ void at(int, bool = true) {}
  __device__ __forceinline__ void at2(int, bool = true) {}
  __device__ __forceinline__ void both(int, int) {}
  __device__ __forceinline__ void flush(long, bool = true) {}
  __device__ __forceinline__ void put(long, unsigned long long) {}
  __device__ __forceinline__ void flush2(long, int, int) {}
};
template <int NA, int NB>
struct BlockStamps<true, NA, NB> {
  unsigned long long* out;                             // nullptr: an ablation-only launch of the probe instance
  unsigned long long a[NA] = {}, b[NB ? NB : 1] = {}, rt0 = 0;
  __device__ __forceinline__ explicit BlockStamps(unsigned long long* o) : out(o) {
    if (out) {
      a[0] = __builtin_amdgcn_s_memtime();
      rt0 = __builtin_amdgcn_s_memrealtime();
    }
  }
  __device__ __forceinline__ void at(int k, bool cond = true) { if (out && cond) a[k] = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void at2(int k, bool cond = true) { if (out && cond) b[k] = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void both(int k, int j) { if (out) a[k] = b[j] = __builtin_amdgcn_s_memtime(); }
  // record `slot` (8 words, one thread calls): the NA points; then the realtime pair (NA = 4) or the realtime now (NA = 6).
  // drain: the thread's stores have left before the last point is taken.
  __device__ __forceinline__ void flush(long slot, bool drain = true) {
    if (!out) return;
    if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    a[NA - 1] = __builtin_amdgcn_s_memtime();
    unsigned long long* o = out + slot * 8;
#pragma unroll
    for (int k = 0; k < NA; ++k) o[k] = a[k];
    if (NA <= 4) o[4] = rt0;
    o[NA <= 4 ? 5 : NA] = __builtin_amdgcn_s_memrealtime();
  }
  __device__ __forceinline__ void put(long word, unsigned long long v) { if (out) out[word] = v; }
  // points [first, first + n) of the later tile to words off ..
  __device__ __forceinline__ void flush2(long off, int first, int n) {
    if (!out) return;
#pragma unroll
    for (int k = 0; k < NB; ++k)
      if (k >= first && k < first + n) out[off + k - first] = b[k];   // (constant indices: the points stay in scalar registers)
  }
};

// ---- SiLU and the conv epilogue
// v * sigmoid(v);  exp2-based, rcp approx (1 ulp) -- far inside fp16 output rounding.
// No FMA contraction in the epilogue arithmetic: the generic and the fast epilogue must give the same bits, so that an
// image's result does not depend on whether its tile was a full one (batch size / position invariance is tested).
__device__ __forceinline__ float m355_silu(float v) {
#pragma clang fp contract(off)
  const float e = __builtin_amdgcn_exp2f(v * -1.4426950408889634f);
  return v * __builtin_amdgcn_rcpf(1.0f + e);
}

// SiLU of all 16 accumulators of a lane: the five operations of m355_silu per element, staged: same bits
__device__ __forceinline__ void silu16(float16v& v) {
#pragma clang fp contract(off)
  float16v t;
#pragma unroll
  for (int j = 0; j < 16; ++j) t[j] = v[j] * -1.4426950408889634f;
#pragma unroll
  for (int j = 0; j < 16; ++j) t[j] = __builtin_amdgcn_exp2f(t[j]);
#pragma unroll
  for (int j = 0; j < 16; ++j) t[j] = 1.0f + t[j];
#pragma unroll
  for (int j = 0; j < 16; ++j) t[j] = __builtin_amdgcn_rcpf(t[j]);
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = v[j] * t[j];
}

// Round-to-fp16 of an epilogue value.  The value is made opaque first: otherwise the compiler may fuse the last
// multiply (or the residual add) with the conversion into v_fma_mix*_f16 for SOME elements of SOME template
// instantiations -- one rounding instead of two, a rare 1-ulp difference that breaks bit-exact tile / batch invariance.
__device__ __forceinline__ half_t m355_to_half(float v) {
  asm volatile("" : "+v"(v));
  return (half_t)v;
}

// ---------------------------------------------------------------------------------------------------------
// Fast conv epilogue shared by the conv kernels.
// A wave measured 13-15 k cycles in the generic epilogue of a 64 ch x 128 px tile: ~85 instructions per 16-byte
// store (per-group validity branches with EXEC save / restore, 64-bit address multiplies, an LDS / global bias read
// with its own wait) at one instruction per 4 cycles per wave.  When the whole wave tile is inside the tensor the
// addresses are affine (base + nt * ystep + group * 32 channels), the bias sits in 16 registers and the SiLU is
// packed: ~40 instructions per store, no branch.
// ---------------------------------------------------------------------------------------------------------
// acc[2s][nt] / acc[2s+1][nt] hold channels 8g..8g+3 / 8g+4..8g+7 of group s for pixel nt (see conv_igemm.hip);
// yp / rp point at (pixel nt = 0, group 0) of this lane; ystep / rstep = elements between consecutive nt.
template <int MT, int NT, bool ACT, bool RES>
__device__ __forceinline__ void conv_epilogue_fast(float4v (&acc)[MT][NT], const float4v (&bias)[MT / 2][2], half_t* yp,
                                                   long ystep, const half_t* rp, long rstep) {
#pragma clang fp contract(off)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
    for (int s = 0; s < MT / 2; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = acc[2 * s][nt][j] + bias[s][0][j];
        v[4 + j] = acc[2 * s + 1][nt][j] + bias[s][1][j];
      }
      if (ACT) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = m355_silu(v[j]);
      }
      if (RES) {
        const half8 rv = *(const half8*)(rp + nt * rstep + s * 32);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += (float)rv[j];
      }
      half8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = m355_to_half(v[j]);
      *(half8*)(yp + nt * ystep + s * 32) = o;
    }
  }
}
// Same, with one output pointer per pixel tile (ConvTranspose pixel-shuffle stores: not affine in nt), no residual.
template <int MT, int NT, bool ACT>
__device__ __forceinline__ void conv_epilogue_fast_ptrs(float4v (&acc)[MT][NT], const float4v (&bias)[MT / 2][2],
                                                        half_t* const (&yp)[NT]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
    for (int s = 0; s < MT / 2; ++s) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = acc[2 * s][nt][j] + bias[s][0][j];
        v[4 + j] = acc[2 * s + 1][nt][j] + bias[s][1][j];
      }
      if (ACT) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = m355_silu(v[j]);
      }
      half8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = m355_to_half(v[j]);
      *(half8*)(yp[nt] + s * 32) = o;
    }
  }
}

}  // namespace m355
