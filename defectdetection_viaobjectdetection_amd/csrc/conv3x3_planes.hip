// 3x3 / stride-1 / pad-1 NHWC fp16 convolutions on v_mfma_f32_32x32x16_f16 over FULL-WIDTH ROW SLABS, with an optional second
// 3x3 convolution fed from LDS: a whole C2f Bottleneck (cv1 -> cv2 (+ shortcut)) in ONE launch (gfx950).
//
// Replaces: the Conv+BN+SiLU 3x3 pairs  m.cv1 -> m.cv2  of upstream's C2f Bottleneck (e = 1.0) that
// BscanBased/yolo8_seg_predict.py:8 reaches through torch.nn.functional.conv2d, two launches and one HBM round trip of the
// hidden tensor in rounds 1-3 (conv3x3_m32 / conv3x3_halo); in single-conv mode the 3x3 layers of the 20 x 20 level
// (conv3x3_small.hip's slab kernel); in block-diagonal single mode the second 3x3 stage of a head level -- cv2.l.1, cv3.l.1 and
// cv4.l.1 over the channel slices of one tensor, three launches before -- with every channel tile on the input planes of its own conv.
//
// Why.  Round 3's stamps: a 128 -> 128 layer on a 40 x 40 map at batch 32 keeps the matrix pipe 42 % busy.  conv3x3_m32 runs
// two blocks per CU that each stream the whole 295 KB weight matrix through LDS for 128 pixels: 32 B/clk/CU of weight
// intake, which IS the L2 -> LDS intake limit (~30 B/clk/CU), plus a prologue, an epilogue and a half-empty tile round per
// launch.  Here ONE block per CU owns every output channel of a slab of R full-width image rows:
//   * a weight stage (one tap x 32 input channels x all output channels of the block) feeds 7-9 pixel blocks of 32 pixels per
//     wave instead of 2: 14-18 B/clk of weight intake;
//   * pixels are LINEAR in the slab at a pitch of W + 1: the zero column right of row y is the zero column left of row
//     y + 1, so a 40-pixel map wastes one column in 41 (the 8 x 16 tiles of m32 wasted 17 %), every MFMA pixel block is 32
//     consecutive storage indices and every tap is a constant index shift: fragment address = per-lane base(tap) + immediate;
//   * pair mode: the first convolution is evaluated on R + 2 rows (the halo rows of the second one are recomputed, 7 / 5 at
//     R = 5), goes through bias + SiLU + fp16 -- the rounding point of the two-launch form -- into LDS planes and never
//     reaches HBM; the second convolution reads it there; one launch, one prologue, one epilogue, no tail round between.
//
// Layout.  A PLANE is 32 channels of the slab: one 64-byte LDS row per storage index (pixel), 16-byte chunk c of row r at
// chunk position c ^ ((r >> 2) & 3).  A ds_read_b128 service group (16 lanes) covers 16 consecutive indices mod 16, so its
// rows hit all four (r & 3) bank quarters with four distinct chunk positions each: conflict-free for every tap shift, for the
// LDS-DMA's lane-linear writes (swizzle applied to the SOURCE address) and for the weight stages (same row format).
// GEMM orientation as in conv3x3_m32.hip: D[channel][pixel], weights = A operand, rows permuted on the DMA source side so
// that a lane-half owns 16 consecutive channels of its pixel (two 16-byte stores / LDS writes per pixel block).
//
// Block = 4 waves, one per SIMD (up to 512 VGPRs): wave = (channel block wc of WC, pixel group wp of WP = 4 / WC), NPB pixel blocks
// each (accumulators: 16 x NPB VGPRs).  K loop: PHASE = one input plane (32 channels) = 9 taps x 2 MFMA slices of K = 16 for every
// pixel block of the wave, pixel-block-major (the 18 MFMAs of a block back to back on one accumulator).
//   * WEIGHTS never touch LDS: the host packs them as MFMA A fragments in K-loop order [channel block][plane][tap][slice] (1 KiB
//     each, lane-linear: planes_frag_pack in weight_pack.hip) and a wave loads the 18 fragments of the NEXT phase straight into its A
//     registers through a per-phase buffer descriptor, each right after its last use in the current phase; they are L2 hits for all
//     blocks but the first.  No weight stage, no weight barrier, no ds_read for the A operand.
//   * B fragments (activations) come from the plane by ds_read_b128 through a register FIFO of FQ = 9 slots, FD = 8 reads in flight.
//   * Input planes: ring of two; the pieces of plane p + 1 are issued by LDS-DMA during phase p (PIT pieces per wave).  ONE barrier
//     per phase, behind a counted s_waitcnt (the weight loads issued after the pieces stay in flight across it).
//   * The VALU work of a finished pixel block (bias is the C operand of the first phase; SiLU, fp16, residual, stores / LDS writes
//     of the hidden tensor) runs as a software pipeline, one stage per MFMA slot of the following block (PostPipe), so a dependent
//     chain never stalls the wave that also feeds the matrix pipe.
#include <stdlib.h>

#include <algorithm>
#include <initializer_list>
#include <utility>

#include "common.h"
#include "device_prims.h"
#include "launch_util.h"
#include "switches.h"

namespace m355 {
namespace {

constexpr int ROWB = 64;      // bytes per LDS row: 32 channels of one pixel / 32 K values of one weight row
constexpr int LDS_MAX = 160 * 1024;

struct PlanesGeom {
  int R, nslab, PW;         // output rows per slab, slabs per image, pitch W + 1
  int irows, xrows;         // rows of an intermediate plane (32 * NB1) / of an input ring slot (16 * npieces)
  int npieces;              // 1 KiB pieces of an input plane
  int NP, NPo;              // input planes (Cin / 32); planes of the hidden tensor (pair) = WC
  int tiles_ch;             // single mode: output channel tiles
  int ntiles;
  int off_x, off_s;         // LDS byte offsets: input ring, one spare KiB behind it (reads of never-stored pixel blocks may run past a slot)
  // block-diagonal single mode (PlanesArgs::diag_n > 0): channel tile t reads the input planes [first, first + count) only and
  // finds its fragments `wo` phases (18 KiB each) into wfb.  Wave-uniform tables, packed: a nibble / a byte per channel tile.
  // A block walks UNITS of gsz consecutive tiles (1, or tiles_ch = every channel tile of a slab: the tiles differ in cost).
  int gsz, nunits;
  unsigned p0_pk, np_pk;
  unsigned long long wo_pk;
};

template <int WC_, int NPB1_, int NPB2_, bool PAIR_, int PPS_, int NW_ = 4, bool S2_ = false>
struct PCfg {
  static constexpr bool S2 = S2_;                 // stride 2 (single mode): the input plane is stored as four sub-planes (row parity x column parity)
  static constexpr int NW = NW_;                  // waves per block: 4 (one per SIMD) or 8 (two: the VALU pipe of one beside the MFMAs of the other)
  static constexpr int WC = WC_, WP = NW_ / WC_, NPB1 = NPB1_, NPB2 = NPB2_, PPS = PPS_;
  static constexpr bool PAIR = PAIR_;
  static constexpr int NB1 = WP * NPB1, NB2 = WP * NPB2;
  static constexpr int NPB = NPB1 > NPB2 ? NPB1 : NPB2;
  // B fragment FIFO (registers): FQ divides the 18 fragments of a pixel block, so every phase starts at slot 0; FD fragments in
  // flight: eight with one wave per SIMD (an LDS read returns within eight MFMAs also when all four waves stream), two with two
  // waves per SIMD (256 registers per wave; the partner's MFMAs cover the wait)
  static constexpr int FQ = NW_ == 4 ? 9 : 3, FD = NW_ == 4 ? 8 : 2;
  static constexpr int PIT = 6 * PPS;             // input pieces per wave and plane
  static constexpr int KSTEP = 2048 * WP;         // LDS bytes between consecutive pixel blocks of one wave
  static_assert(WC == 2 || WC == 4, "channel blocks per block");
};

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>) (the 126 .. 162 MFMA slots of a phase; #pragma
// unroll refuses a loop of that size with a barrier in one iteration)
template <int... Is, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, f);
}


template <class C>
struct PState {
  float16v acc[C::NPB];
  half8 A[18];                // the phase's weight fragments (MFMA A operands): (tap, slice) -> 2 * tap + slice
  half8 bq[C::FQ];
  int tb[9];                  // B fragment: LDS byte offset inside a plane for (tap, slice 0), pixel block 0 of this wave
  int pvoff[C::PIT];          // per-lane source offsets of the input pieces of the slab the loader is on
  __amdgpu_buffer_rsrc_t rs_x;
  char* smem;
  int wave, lane16;
  int pcur, pnext;            // LDS byte offset of this / the next phase's plane
  __amdgpu_buffer_rsrc_t rs_wn;   // the NEXT phase's 18 fragments (next plane, next convolution, next tile): 1 KiB each, lane-linear.
                              // A descriptor per phase (scalar registers) + lane offset + constant: 64-bit per-lane addresses of
                              // 18 fragments were 36 VGPRs -- spilled, and every scratch reload drains the memory pipeline
  // input pieces of the phase: this wave issues piece m into LDS KiB wave + 4 m of the target slot; pieces from nreal on are
  // zero fills of the spare KiB (a phase that streams nothing: nreal = 0)
  int nreal, px_soff, px_dst; // px_dst: LDS byte offset of this wave's piece 0
  int off_s;
};

// fp16 rounding of an epilogue value, opaque to mul + cvt fusion like m355_to_half, but not volatile: independent chains stay
// free to be interleaved
__device__ __forceinline__ half_t to_half_rn(float v) {
  asm("" : "+v"(v));
  return (half_t)v;
}

// The VALU work behind a finished pixel block, as a software pipeline over the MFMA slots of the phase (one wave per SIMD: a
// dependent chain  mul -> exp -> add -> rcp -> mul  issued in one piece waits for every result; issued one stage per slot, six
// independent instructions sit beside each MFMA).  Value c (0 .. 15) of block kk enters the pipe in slot 18 (kk + 1) + 1 + c --
// block kk's last MFMA was issued two slots earlier -- and advances one stage per slot:
//   +0 t = x * -log2(e)   +1 t = exp2(t)   +2 t = 1 + t   +3 t = rcp(t)   +4 y = x * t     (the five instructions of m355_silu)
//   modes 2 / 3 (output conv without / with a residual): +5 y += residual
//   then (odd c) the pair (c - 1, c) is rounded to fp16, and behind c = 7 / 15 the eight values are stored:
//   mode 1: into the hidden plane in LDS (the transition of a Bottleneck), mode 2: to the output tensor.
template <int NPBC>
struct PostPipe {
  float t[8];            // running temporaries, by c % 8
  float y[4];            // finished values, by c % 4 (a pair is packed one or two slots after its second value)
  half8 o[2];            // the two 16-byte halves of a pixel's 16 channels
  half8 rv[2][2];        // mode 3: the residual of the block in the pipe / of the next one (loaded one block ahead, an L2 hit)
};
template <int NPBC, int n, int OFF>
struct PipeAt {   // which value is at stage offset OFF in slot n
  static constexpr int m = n - 1 - OFF;
  static constexpr bool on = m >= 18 && (m % 18) < 16 && (m / 18 - 1) < NPBC;
  static constexpr int kk = on ? m / 18 - 1 : 0, c = on ? m % 18 : 0;
};

template <class C, int NPBC, int MODE, int n, class Store>
__device__ __forceinline__ void post_slot(PState<C>& st, PostPipe<NPBC>& pp, Store&& store) {
#pragma clang fp contract(off)
  using A = PipeAt<NPBC, n, 0>;
  using B = PipeAt<NPBC, n, 1>;
  using Cc = PipeAt<NPBC, n, 2>;
  using D = PipeAt<NPBC, n, 3>;
  using E = PipeAt<NPBC, n, 4>;
  using F = PipeAt<NPBC, n, 5>;
  constexpr int PKO = MODE == 3 ? 6 : 5;
  using P = PipeAt<NPBC, n, PKO>;
  using W = PipeAt<NPBC, n, PKO + 1>;
  if constexpr (A::on) pp.t[A::c % 8] = st.acc[A::kk][A::c] * -1.4426950408889634f;
  if constexpr (B::on) pp.t[B::c % 8] = __builtin_amdgcn_exp2f(pp.t[B::c % 8]);
  if constexpr (Cc::on) pp.t[Cc::c % 8] = 1.0f + pp.t[Cc::c % 8];
  if constexpr (D::on) pp.t[D::c % 8] = __builtin_amdgcn_rcpf(pp.t[D::c % 8]);
  if constexpr (E::on) pp.y[E::c % 4] = st.acc[E::kk][E::c] * pp.t[E::c % 8];
  if constexpr (MODE == 3 && F::on) pp.y[F::c % 4] = __builtin_fmaf((float)pp.rv[F::kk & 1][F::c / 8][F::c % 8], 1.0f, pp.y[F::c % 4]);   // = y + residual, one v_fma_mix
  if constexpr (P::on && (P::c & 1)) {
    pp.o[P::c / 8][(P::c % 8) - 1] = to_half_rn(pp.y[(P::c - 1) % 4]);
    pp.o[P::c / 8][P::c % 8] = to_half_rn(pp.y[P::c % 4]);
  }
  if constexpr (W::on && (W::c % 8) == 7) store.put(W::kk, W::c / 8, pp.o[W::c / 8]);
}

// One PHASE of a convolution: one input plane (32 channels) x nine taps for every pixel block of the wave, PIXEL-BLOCK MAJOR:
// the 18 weight fragments of the phase sit in registers (loaded during the previous phase), block k runs its 18 MFMAs on one
// accumulator back to back (a single accumulation chain of v_mfma_f32_32x32x16 issues at full rate), then block k + 1.  So the
// LAST phase of a convolution finishes its pixel blocks one after the other and the VALU work behind a finished block runs
// beside the MFMAs of the next one (PostPipe) instead of after the whole K loop -- it was 25 % of the kernel.
// Every slot = one MFMA + one LDS read (+ a vector-memory issue, + the pipe's six VALU instructions), pinned by a sched_barrier.
//   FIRST  first phase of the convolution: block k's first MFMA takes the bias vector as its C operand (no zero fill, no bias add)
//   MODE   0 plain phase; 1 / 2 / 3: last phase with the post pipe (transition / output / output + residual); the caller handles
//          what follows (no barrier here)
//   PRIMED the previous phase already issued this phase's first FD fragment reads (after its barrier)
template <class C, int NPBC, bool FIRST, int MODE, bool PRIMED, class Store>
__device__ __forceinline__ void planes_phase(PState<C>& st, const float16v& bv, Store&& store) {
  constexpr int N = NPBC * 18;
  constexpr int PSTEP = 3;                                       // slots between two input pieces
  constexpr int FQ = C::FQ, FD = C::FD;
  int addr[9];   // slice 0 of the nine taps; slice 1 = ^ 32 (the planes start at multiples of 64 bytes)
#pragma unroll
  for (int t = 0; t < 9; ++t) addr[t] = st.pcur + st.tb[t];
  PostPipe<NPBC> pp;
  if (!PRIMED) {
#pragma unroll
    for (int n = 0; n < FD; ++n) st.bq[n % FQ] = *(const half8*)(st.smem + (addr[(n % 18) / 2] ^ ((n & 1) << 5)) + (n / 18) * C::KSTEP);
  }
  static_for<N>([&](auto nc) __attribute__((always_inline)) {
    constexpr int n = decltype(nc)::value;
    constexpr int k = n / 18, i = n % 18;
    if constexpr (MODE == 0 && n == N - FD) {
      // every read of this plane has been issued.  Phase end: this wave's pieces of the next plane and the next phase's weight
      // fragments have landed, then every wave's; the next phase's first reads go out under this phase's last MFMAs
      // (younger than the pieces: exactly the 18 - FD weight loads of the last block's first slots, which may stay in flight)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(18 - FD) : "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (FIRST && i == 0)
      st.acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(st.A[i], st.bq[n % FQ], bv, 0, 0, 0);
    else
      st.acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(st.A[i], st.bq[n % FQ], st.acc[k], 0, 0, 0);
    if constexpr (n + FD < N) {
      constexpr int m = n + FD;
      st.bq[m % FQ] = *(const half8*)(st.smem + (addr[(m % 18) / 2] ^ ((m & 1) << 5)) + (m / 18) * C::KSTEP);
    } else if constexpr (MODE == 0) {
      constexpr int m = n + FD - N;   // the next phase's fragment m (its block 0)
      st.bq[m % FQ] = *(const half8*)(st.smem + st.pnext + (st.tb[m / 2] ^ ((m & 1) << 5)));
    }
    // the next phase's weight fragments: fragment i is reloaded right behind its last MFMA of this phase (the last pixel block), 18
    // slots + the barrier before its first MFMA of the next phase: an L2 hit (every CU streams the same fragments).  One set of
    // 18 fragments in registers, ONE code body for every middle phase of a convolution (it stays in the instruction cache).
    if constexpr (k == NPBC - 1) {
      typedef unsigned int u4 __attribute__((ext_vector_type(4)));
      const u4 wv = __builtin_amdgcn_raw_buffer_load_b128(st.rs_wn, st.lane16, i * 1024, 0);
      st.A[i] = __builtin_bit_cast(half8, wv);
    }
    // the input pieces of the phase's target plane, early in the phase
    if constexpr (n >= 1 && (n - 1) % PSTEP == 0 && (n - 1) / PSTEP < C::PIT) {
      constexpr int m = (n - 1) / PSTEP;
      const bool real = m < st.nreal;
      dma16(st.rs_x, real ? st.pvoff[m] : (int)0x80000000, st.px_soff, st.smem + (real ? st.px_dst + m * (C::NW * 1024) : st.off_s));
    }
    // block k's residual: first used in slot 18 (k + 1) + 6; the buffer's previous tenant (block k - 2) was last read in slot 18 k + 3
    if constexpr (MODE == 3 && i == 5) store.load_res(k, pp.rv[k & 1]);
    if constexpr (MODE != 0) post_slot<C, NPBC, MODE, n>(st, pp, store);
    __builtin_amdgcn_sched_barrier(0);
  });
  if constexpr (MODE != 0) {   // drain: the last block's values
    static_for<16 + 8>([&](auto nc) __attribute__((always_inline)) {
      constexpr int n = N + decltype(nc)::value;
      post_slot<C, NPBC, MODE, n>(st, pp, store);
      __builtin_amdgcn_sched_barrier(0);
    });
  }
}

struct PTile {
  int b, y0, ch;   // image, first output row, first output channel
  int p0, np, wo;  // block-diagonal mode: first input plane, input planes, fragment offset in phases
};

template <class C, bool RES, bool DIAG, bool PROBE>
__global__ __launch_bounds__(64 * C::NW, C::NW / 4) void planes_kernel(const PlanesArgs a, const PlanesGeom g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int lrow = lane >> 2, lchunk = lane & 3;
  const int wc = wave % C::WC, wp = wave / C::WC;
  const int H = a.H, W = a.W, PW = g.PW, R = g.R;   // H, W: input map
  const int Ho = C::S2 ? H / 2 : H, Wo = C::S2 ? W / 2 : W;   // output map (PW = Wo + 1)
  const int nwg = gridDim.x, ntiles = g.ntiles;
  // probe instance only, per wave.  Points: entry, first patch landed, last phase of the first conv, hidden tensor complete, last phase of
  // the second conv, end.  Second list: start of phase 0, 1, 2 and of the last phase of either conv (the block's last tile).
  BlockStamps<PROBE, 6, 8> bs(a.stamps);

  // XCD-aware persistent walk (as conv3x3_m32.hip): the virtual blocks of one XCD cover a contiguous run of tiles; channel
  // tiles fastest (they share the input slab in L2), then slabs, then images.
  // (block-diagonal mode: vb counts units of gsz tiles, `sub` is the tile inside the unit)
  auto decode = [&](int vb, int sub) __attribute__((always_inline)) {
    const int nu = DIAG ? g.nunits : ntiles;
    const int xcd = vb & 7, q = nu >> 3, r = nu & 7;
    int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (vb >> 3);
    if constexpr (DIAG) L = L * g.gsz + sub;
    PTile t;
    const int tch = L % g.tiles_ch;
    const int rest = L / g.tiles_ch;
    t.b = rest / g.nslab;
    t.y0 = (rest - t.b * g.nslab) * R;
    t.ch = tch * 32 * C::WC;
    if constexpr (DIAG) {
      t.p0 = (int)(g.p0_pk >> (4 * tch)) & 15;
      t.np = (int)(g.np_pk >> (4 * tch)) & 15;
      t.wo = (int)(g.wo_pk >> (8 * tch)) & 255;
    } else {
      t.p0 = 0; t.np = g.NP; t.wo = 0;
    }
    return t;
  };

  PState<C> st;
  st.smem = smem;
  st.wave = wave;
  st.lane16 = lane * 16;
  st.off_s = g.off_s;
  const int pbytes = 18 * 1024;                          // fragments of one phase
  const long wblock = (long)pbytes * g.NP;               // ... of one channel block of one convolution
  const int nreal_wave = (g.npieces - wave + C::NW - 1) / C::NW;     // pieces of a plane this wave issues
  const int img_stride = (int)a.x_bstride * 2;
  st.rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)((a.B - 1) * a.x_bstride + (long)H * W * a.ldx) * 2, 0x00020000);

  // input pieces of a tile: piece k = wave + 4 m covers LDS rows 16 k .. 16 k + 15 = storage indices; index j = rj * PW + cj is
  // image pixel (y0 - HALO + rj, cj - 1); outside the image (and the shared zero column cj = 0) the offset fails the range
  // check and the LDS-DMA writes zeros
  // Stride 2: a plane is FOUR sub-planes (input row parity rp x column parity cp) of (R + 1) x PW storage indices each, so that every
  // tap reads consecutive indices again: output pixel (yo, xo) at tap (kh, kw) reads sub-plane (kh != 1, kw != 1) at index
  // q + (kh != 0) * PW + (kw != 0), q = (yo - y0) * PW + xo; sub-plane index rr * PW + cc is input pixel (2 (y0 + rr - 1) + rp,
  // 2 (cc - 1) + cp).  The de-interleaving happens on the DMA's source side (per-lane addresses).
  constexpr int HALO = C::PAIR ? 2 : 1;
  const int spr = (R + 1) * PW;                          // storage indices of one sub-plane (stride 2)
  const int xrows_valid = C::S2 ? 4 * spr : (R + 2 * HALO) * PW;
  auto piece_offsets = [&](const PTile& t) __attribute__((always_inline)) {
#pragma unroll
    for (int m = 0; m < C::PIT; ++m) {
      const int j = 16 * (wave + C::NW * m) + lrow;
      int iy, ix;
      bool ok = j < xrows_valid;
      if (C::S2) {
        const int sp = j / spr, jj = j - sp * spr;
        const int rr = jj / PW, cc = jj - rr * PW;
        iy = 2 * (t.y0 + rr - 1) + (sp >> 1);
        ix = 2 * (cc - 1) + (sp & 1);
        ok = ok && (unsigned)ix < (unsigned)W && (unsigned)iy < (unsigned)H;
      } else {
        const int rj = j / PW, cj = j - rj * PW;
        iy = t.y0 - HALO + rj; ix = cj - 1;
        ok = ok && cj >= 1 && (unsigned)iy < (unsigned)H;
      }
      const int lc = lchunk ^ ((j >> 2) & 3);
      st.pvoff[m] = ok ? ((iy * W + ix) * a.ldx + lc * 8) * 2 : (int)0x80000000;
    }
  };
  // B fragment offsets of the nine taps: storage index of this lane's pixel of block 0 + the tap's shift
  const int idx0 = 32 * wp + l31;
  auto tap_offsets = [&](int dshift) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int kh = t / 3, kw = t % 3;
      const int row = C::S2 ? ((kh != 1) * 2 + (kw != 1)) * spr + idx0 + (kh != 0) * PW + (kw != 0) : idx0 + kh * PW + kw + dshift;
      st.tb[t] = row * ROWB + ((h ^ ((row >> 2) & 3)) << 4);
    }
  };
  auto load_bias = [&](const float* bias, int ch0) __attribute__((always_inline)) {
    const float* bp = bias + ch0 + wc * 32 + 16 * h;
    float16v bv;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4v v = *(const float4v*)(bp + q * 4);
      bv[q * 4 + 0] = v[0]; bv[q * 4 + 1] = v[1]; bv[q * 4 + 2] = v[2]; bv[q * 4 + 3] = v[3];
    }
    return bv;
  };
  auto load_frags = [&](const char* src, half8 (&dst)[18]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 18; ++j) dst[j] = *(const half8*)(src + st.lane16 + j * 1024);
  };

  // ---- the block's stream of tiles
  int vb = blockIdx.x, sub = 0;
  // the tile after (vb, sub) in this block's walk
  auto has_next = [&]() __attribute__((always_inline)) { return DIAG ? (sub + 1 < g.gsz || vb + nwg < g.nunits) : vb + nwg < ntiles; };
  auto next_of = [&]() __attribute__((always_inline)) {
    if constexpr (DIAG) return sub + 1 < g.gsz ? decode(vb, sub + 1) : decode(vb + nwg, 0);
    else return decode(vb + nwg, 0);
  };
  // this wave's fragments of a tile's (second / only) convolution
  auto wbase_of = [&](const PTile& t) __attribute__((always_inline)) {
    if constexpr (DIAG) return (const char*)a.wfb + (long)(t.wo + wc * t.np) * pbytes;
    else return (const char*)a.wfb + (t.ch / 32 + wc) * wblock;
  };
  PTile cur = decode(vb, 0), nxt = cur;
  bool more = has_next();
  if (more) nxt = next_of();
  const char* const wbase_a = C::PAIR ? (const char*)a.wfa + wc * wblock : nullptr;   // pair: this wave's channel block in the first conv
  const char* wbase_b = wbase_of(cur);             // second / only conv, this tile
  const char* wbase_b_next = wbase_of(nxt);        // ... the block's next tile

  // ---- prologue: input plane 0 into slot 0, the weight fragments of the first phase
  // (the fragments first: their latency -- a cold L2 for the first blocks of a launch -- covers the piece address arithmetic)
  load_frags(C::PAIR ? wbase_a : wbase_b, st.A);
  piece_offsets(cur);
#pragma unroll
  for (int m = 0; m < C::PIT; ++m) {
    const int k = wave + C::NW * m;
    if (k < g.npieces) dma16(st.rs_x, st.pvoff[m], cur.b * img_stride + (DIAG ? cur.p0 * 64 : 0), smem + g.off_x + k * 1024);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  bs.at(1);

  const int xslot = g.xrows * ROWB;   // bytes of an input ring slot
  const int iplane = g.irows * ROWB;  // bytes of an intermediate plane
  int xg = 0;                         // input planes consumed so far by this block (ring slot = xg & 1)
  int NP = DIAG ? cur.np : g.NP;      // input planes of the tile's (first) convolution

  while (true) {
    // =========================== first convolution (pair mode): R + 2 rows of the hidden tensor ===========================
    if constexpr (C::PAIR) {
      tap_offsets(-1);
      char* const plane = smem + wc * iplane;
      // the transition: a finished half pixel (8 channels, fp16) goes into plane wc of the hidden tensor.  The zero padding of the
      // second conv is written OVER it afterwards.
      struct Store1 {
        char* plane; int wp, l31, h;
        __device__ __forceinline__ void put(int k, int hh, const half8& o) const {
          const int i = 32 * (wp + C::WP * k) + l31;
          *(half8*)(plane + i * ROWB + (((2 * h + hh) ^ ((i >> 2) & 3)) << 4)) = o;
        }
        __device__ __forceinline__ void load_res(int, half8 (&)[2]) const {}
      } store1{plane, wp, l31, h};
      const float16v bv = load_bias(a.ba, 0);
      auto setup1 = [&](int p) __attribute__((always_inline)) {
        st.pcur = g.off_x + (xg & 1) * xslot;
        st.pnext = g.off_x + ((xg + 1) & 1) * xslot;
        st.nreal = p + 1 < NP ? nreal_wave : 0;   // stream plane p + 1 of this tile into the other slot
        st.px_soff = cur.b * img_stride + (p + 1) * 64;
        st.px_dst = st.pnext + wave * 1024;
        st.rs_wn = __builtin_amdgcn_make_buffer_rsrc((void*)(p + 1 < NP ? wbase_a + (p + 1) * pbytes : wbase_b), 0, pbytes, 0x00020000);
        ++xg;
      };
      setup1(0);
      bs.at2(0);
      planes_phase<C, C::NPB1, true, 0, false>(st, bv, store1);
      for (int p = 1; p + 1 < NP; ++p) {
        setup1(p);
        bs.at2(1, p == 1);
        bs.at2(2, p == 2);
        planes_phase<C, C::NPB1, false, 0, true>(st, bv, store1);
      }
      setup1(NP - 1);
      bs.both(2, 3);
      planes_phase<C, C::NPB1, false, 1, true>(st, bv, store1);
      if (more) piece_offsets(nxt);   // every piece of this tile has been issued: the loader moves on
      // zero padding (a wave's LDS operations complete in order).  Only the wp == 0 wave of a channel block writes it -- after
      // a barrier when a second pixel group wrote parts of the plane.
      if (C::WP > 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      if (wp == 0) {
        const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        // pad column: rows ri * PW, ri = 0 .. R + 2 (the last one is the pad behind the last row); 4 lanes x 16 bytes each
        for (int e = lane; e < 4 * (R + 3); e += 64) *(half8*)(plane + (e >> 2) * PW * ROWB + ((e & 3) << 4)) = z;
        // rows outside the image: only the first and the last slab of an image have any
#pragma unroll 1
        for (int ri = 0; ri < R + 2; ++ri) {
          const int iy = cur.y0 - 1 + ri;
          if ((unsigned)iy < (unsigned)H) continue;
          for (int e = lane; e < 4 * PW; e += 64) *(half8*)(plane + (ri * PW + (e >> 2)) * ROWB + ((e & 3) << 4)) = z;
        }
      }
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      bs.at(3);
    }
    // =========================== second (or only) convolution: R rows ===========================
    {
      tap_offsets(0);
      const int npl = C::PAIR ? g.NPo : NP;
      // ---- epilogue: pixel q -> (row, column) by an exact float division (q < 2^11) when a block's values are stored / its residual
      // is fetched (one block ahead of its use); out-of-image pixels get an out-of-range buffer offset: zeros / dropped stores
      struct Store2 {
        __amdgpu_buffer_rsrc_t rs_y, rs_r;
        int wp, l31, PW, W, R, H, y0, ldy, ldr, c0; bool ch_ok; float rpw;
        __device__ __forceinline__ int pixel(int k) const {
          const int q = 32 * (wp + C::WP * k) + l31;
          const int r = (int)(((float)q + 0.5f) * rpw), c = q - r * PW;
          const int yy = y0 + r;
          return (c < W && r < R && yy < H && ch_ok) ? yy * W + c : -1;
        }
        __device__ __forceinline__ void put(int k, int hh, const half8& o) const {
          typedef unsigned int u4 __attribute__((ext_vector_type(4)));
          const int pix = pixel(k);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, o), rs_y, pix >= 0 ? (pix * ldy + c0) * 2 : (int)0x80000000, 16 * hh, 0);
        }
        __device__ __forceinline__ void load_res(int k, half8 (&rv)[2]) const {
          const int pix = pixel(k);
          const int ro = pix >= 0 ? (pix * ldr + c0) * 2 : (int)0x80000000;
          rv[0] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rs_r, ro, 0, 0));
          rv[1] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rs_r, ro, 16, 0));
        }
      };
      const int c0 = cur.ch + wc * 32 + 16 * h;
      const Store2 store2{
          __builtin_amdgcn_make_buffer_rsrc((void*)(a.y + (long)cur.b * a.y_bstride), 0, (int)((long)Ho * Wo * a.ldy * 2), 0x00020000),
          __builtin_amdgcn_make_buffer_rsrc((void*)(RES ? a.res + (long)cur.b * a.r_bstride : a.x), 0, (int)((long)Ho * Wo * (RES ? a.ldr : a.ldx) * 2), 0x00020000),
          wp, l31, PW, Wo, R, Ho, cur.y0, a.ldy, a.ldr, c0, c0 + 16 <= a.Cout, 1.0f / (float)PW};
      const float16v bv2 = load_bias(a.bb, cur.ch);
      auto setup2 = [&](int p) __attribute__((always_inline)) {
        bool pieces = false;
        if (C::PAIR) {
          st.pcur = p * iplane;
          st.pnext = (p + 1) * iplane;
          if (p == 0 && more) {   // plane 0 of the next tile into the slot the next tile starts with
            pieces = true;
            st.px_soff = nxt.b * img_stride;
            st.px_dst = g.off_x + (xg & 1) * xslot + wave * 1024;
          }
        } else {
          st.pcur = g.off_x + (xg & 1) * xslot;
          st.pnext = g.off_x + ((xg + 1) & 1) * xslot;
          st.px_dst = st.pnext + wave * 1024;
          if (p + 1 < NP) {
            pieces = true;
            st.px_soff = cur.b * img_stride + ((DIAG ? cur.p0 : 0) + p + 1) * 64;
          } else if (more) {
            piece_offsets(nxt);
            pieces = true;
            st.px_soff = nxt.b * img_stride + (DIAG ? nxt.p0 * 64 : 0);
          }
          ++xg;
        }
        st.nreal = pieces ? nreal_wave : 0;
        st.rs_wn = __builtin_amdgcn_make_buffer_rsrc((void*)(p + 1 < npl ? wbase_b + (p + 1) * pbytes : (C::PAIR ? wbase_a : wbase_b_next)), 0, pbytes, 0x00020000);
      };
      setup2(0);
      bs.at2(4);
      if constexpr (DIAG) {   // a diagonal block of one input plane: its only phase is the first and the last
        if (npl == 1) {
          bs.both(4, 7);
          planes_phase<C, C::NPB2, true, RES ? 3 : 2, false>(st, bv2, store2);
        }
      }
      if (!DIAG || npl > 1) {
        planes_phase<C, C::NPB2, true, 0, false>(st, bv2, store2);
        for (int p = 1; p + 1 < npl; ++p) {
          setup2(p);
          bs.at2(5, p == 1);
          bs.at2(6, p == 2);
          planes_phase<C, C::NPB2, false, 0, true>(st, bv2, store2);
        }
        setup2(npl - 1);
        bs.both(4, 7);
        planes_phase<C, C::NPB2, false, RES ? 3 : 2, true>(st, bv2, store2);
      }
    }
    if (!more) break;
    if constexpr (DIAG) {
      if (++sub == g.gsz) { sub = 0; vb += nwg; }
      NP = nxt.np;
    } else {
      vb += nwg;
    }
    cur = nxt;
    more = has_next();
    if (more) nxt = next_of();
    wbase_b = wbase_b_next;
    wbase_b_next = wbase_of(nxt);
    // this tile's last phase ended without a barrier: the next tile's plane 0 (pieces issued in an earlier phase of this tile by
    // every wave) and its first weight fragments must have landed before anyone reads them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  if (lane == 0) {
    const long slot = (long)blockIdx.x * C::NW + wave;
    bs.flush(slot, false);
    bs.flush2(((long)gridDim.x * C::NW + slot) * 8, 0, 8);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
template <class C>
bool planes_geometry(const PlanesArgs& a, PlanesGeom* g, bool any_fill = false) {
  constexpr int HALO = C::PAIR ? 2 : 1;
  if (C::S2 && ((a.H | a.W) & 1)) return false;
  const int Ho = C::S2 ? a.H / 2 : a.H, Wo = C::S2 ? a.W / 2 : a.W;
  const int PW = Wo + 1;
  auto rows_of = [&](int R) { return C::S2 ? 4 * (R + 1) * PW : (R + 2 * HALO) * PW + 1; };   // storage indices of an input plane
  int R = 32 * C::NB2 / PW;                                      // R * PW <= 32 * NB2
  if (C::PAIR) R = std::min(R, (32 * C::NB1 - 1) / PW - 2);      // (R + 2) * PW + 1 <= 32 * NB1: the pad after the last row is computed (as zero)
  R = std::min(R, Ho);
  const int NP = a.Cin / 32;
  for (; R >= 1; --R) {
    const int npieces = (rows_of(R) + 15) / 16;
    if (npieces > C::NW * C::PIT) continue;
    const int inter = C::PAIR ? C::WC * 32 * C::NB1 * ROWB : 0;
    if (inter + 2 * npieces * 1024 + 1024 > LDS_MAX) continue;
    break;
  }
  if (R < 1) return false;
  const int nslab = (Ho + R - 1) / R;
  R = (Ho + nslab - 1) / nslab;                                 // equal slabs
  // the kernel always runs its NPB2 (and NPB1) pixel blocks: refuse geometries that leave them mostly empty
  if (!any_fill && (long)R * PW * 10 < (long)32 * C::NB2 * 6) return false;
  g->R = R; g->nslab = nslab; g->PW = PW;
  g->irows = 32 * C::NB1;
  g->npieces = (rows_of(R) + 15) / 16;
  g->xrows = 16 * g->npieces;
  g->NP = NP; g->NPo = C::WC;
  g->tiles_ch = C::PAIR ? 1 : (a.Cout + 32 * C::WC - 1) / (32 * C::WC);
  g->ntiles = a.B * nslab * g->tiles_ch;
  g->off_x = C::PAIR ? C::WC * g->irows * ROWB : 0;
  g->off_s = g->off_x + 2 * g->xrows * ROWB;
  g->gsz = 1; g->nunits = g->ntiles; g->p0_pk = g->np_pk = 0; g->wo_pk = 0;
  return g->off_s + 1024 <= LDS_MAX;
}

bool planes_common_ok(const PlanesArgs& a) {
  if (!a.x || !a.y || !a.wfb || !a.bb || a.B < 1 || a.H < 1 || a.W < 2) return false;
  if (a.Cin % 32 || a.Cin < 64 || a.ldx % 8 || a.ldy % 8 || !a.act) return false;   // (every 3x3 conv of the graphs has SiLU: the kernels apply it unconditionally)
  if (((long)(a.B - 1) * a.x_bstride + (long)a.H * a.W * a.ldx) * 2 >= (1L << 31)) return false;   // one buffer descriptor over the input
  if ((long)a.cblocks_b * (a.Cin / 32) * 18 * 1024 >= (1L << 31)) return false;                        // and one over the fragments
  return true;
}

template <class C>
int planes_launch(const PlanesArgs& a, const PlanesGeom& g, hipStream_t s) {
  auto k = a.stamps ? (a.res ? planes_kernel<C, true, false, true> : planes_kernel<C, false, false, true>)
                    : (a.res ? planes_kernel<C, true, false, false> : planes_kernel<C, false, false, false>);
  static int slots = 0;
  if (!slots) {
    for (const void* fn : {(const void*)planes_kernel<C, true, false, false>, (const void*)planes_kernel<C, false, false, false>,
                           (const void*)planes_kernel<C, true, false, true>, (const void*)planes_kernel<C, false, false, true>})
      if (const int e = prepare_kernel(fn, LDS_MAX)) return e;
    const int cus = num_cus();
    if (cus <= 0) return -2;
    slots = cus & ~7;   // one block per CU; the XCD-aware tile order needs gridDim.x % 8 == 0 whenever a block walks > 1 tile
    if (slots < 8) slots = 8;
  }
  const int grid = g.ntiles <= slots ? g.ntiles : slots;
  hipLaunchKernelGGL(k, dim3(grid), dim3(64 * C::NW), g.off_s + 1024, s, a, g);
  return (int)hipGetLastError();
}

using P128 = PCfg<4, 9, 7, true, 1>;    // 128 hidden channels: 40 x 40 maps in slabs of 5 rows (9 / 7 pixel blocks per wave)
using P64 = PCfg<2, 8, 6, true, 2>;     // 64 hidden channels: 80 x 80 maps in slabs of 4 rows (16 / 12 pixel blocks over two pixel groups).  (Measured on eight
                                        // waves, <2, 4, 3, true, 1, 8>: 256 registers per wave do not hold the pipe -- 70 spills, 91 us per pair.)
using S64 = PCfg<2, 0, 4, false, 1>;    // single conv, 64-channel tiles: 20 x 20 maps in slabs of 10 rows
using S64S2 = PCfg<2, 0, 4, false, 3, 4, true>;   // ... stride 2: 80 -> 40 in slabs of 5 output rows, 40 -> 20 in slabs of 10
using S128S2 = PCfg<4, 0, 7, false, 3, 4, true>;  // stride 2, 128-channel tiles: half the input re-reads and LDS-DMA issues per MFMA of the 64-channel form

}  // namespace

// Shape-only eligibility (graph construction): an instance exists for C hidden channels and its row slabs fit LDS.
bool bneck_pair_shape_ok(int C, int H, int W) {
  PlanesArgs a{};
  a.H = H; a.W = W; a.B = 1; a.Cin = a.Cout = C; a.stride = 1;
  PlanesGeom g;
  if (C == 128) return planes_geometry<P128>(a, &g);
  // 64 hidden channels: measured 58 us per pair on the 80 x 80 level at batch 32 against 56 for the two conv3x3_halo launches -- a
  // block finishes half of its phases with the SiLU pipe beside the MFMAs (VALU-bound), and with one wave per SIMD nothing else
  // covers it.  The instance is kept (tests, M355_PAIR64=1), the graph builder does not use it.
  if (C == 64 && live_pair64()) return planes_geometry<P64>(a, &g);   // (graph construction only: not on a launch path)
  return false;
}

// A whole Bottleneck (two 3x3 convs, hidden = in = out channels) in one launch.
bool bneck_pair_ok(const PlanesArgs& a) {
  if (!planes_common_ok(a) || !a.wfa || !a.ba) return false;
  if (a.Cin != a.Cout || a.cblocks_a * 32 < a.Cin || a.cblocks_b * 32 < a.Cin) return false;
  PlanesGeom g;
  if (a.Cin == 128) return planes_geometry<P128>(a, &g);
  if (a.Cin == 64) return planes_geometry<P64>(a, &g);
  return false;
}

int launch_bneck_pair(const PlanesArgs& a, hipStream_t s) {
  if (!bneck_pair_ok(a)) return -1;
  PlanesGeom g;
  if (a.Cin == 128) return planes_geometry<P128>(a, &g) ? planes_launch<P128>(a, g, s) : -1;
  return planes_geometry<P64>(a, &g) ? planes_launch<P64>(a, g, s) : -1;
}

// One 3x3 conv (+ SiLU, + residual) over row slabs, 64-channel output tiles.
namespace {
// Stride 2: which channel tile?  Every tile streams the whole input slab, so the 128-channel form halves the L2 -> LDS traffic and
// the LDS-DMA issues (~120 cycles each beside the MFMAs: 16 per wave and phase on an 80 x 80 input) per MFMA; it needs >= one tile
// per CU to pay.  Cost model in cycles per block: tiles x phases x (MFMA slots x 33 + pieces x 120 + 700).
template <class C>
long planes_cost(const PlanesArgs& a, PlanesGeom* g) {
  if (!planes_geometry<C>(a, g)) return -1;
  if (C::WC == 4 && a.Cout % 128) return -1;
  static const int cus = num_cus() > 0 ? num_cus() : 256;   // read once, as planes_launch does
  const long rounds = (g->ntiles + cus - 1) / cus;
  return rounds * g->NP * ((long)C::NPB2 * 18 * 33 + (long)((g->npieces + C::NW - 1) / C::NW) * 120 + 700);
}
}  // namespace

bool conv3x3_planes_ok(const PlanesArgs& a) {
  if (!planes_common_ok(a) || (a.stride != 1 && a.stride != 2)) return false;
  if ((a.Cin / 32) % 2 || a.Cout % 8 || a.cblocks_b * 32 < (a.Cout + 63) / 64 * 64) return false;   // (the input ring alternates slots across tiles: even plane count)
  if (a.stride == 2 && a.res) return false;
  PlanesGeom g;
  return a.stride == 2 ? (planes_geometry<S64S2>(a, &g) || (a.Cout % 128 == 0 && planes_geometry<S128S2>(a, &g))) : planes_geometry<S64>(a, &g);
}

// ---- block-diagonal single mode: diag_n 3x3 convs side by side (the second stage of a head level: 64 -> 64, 128 -> 128, 32 -> 32 over
// the channels of one 224-channel tensor) as ONE launch.  Channel tile t (64 channels of one conv) runs the K loop over the input
// planes of its own conv only, in the order of that conv's own conv3x3_planes<64ch,rows> launch: same bits per channel.
namespace {
constexpr int DIAG_MAX_TILES = 8;

bool diag_geometry(const PlanesArgs& a, PlanesGeom* g) {
  if (!planes_common_ok(a) || a.stride != 1 || a.res || a.diag_n < 1 || a.diag_n > 4) return false;
  int ci = 0, co = 0, tiles = 0, wo = 0;
  unsigned p0_pk = 0, np_pk = 0;
  unsigned long long wo_pk = 0;
  for (int i = 0; i < a.diag_n; ++i) {
    const int cin = a.diag_cin[i], cout = a.diag_cout[i];
    if (cin < 32 || cin % 32 || cin / 32 > 15 || cout < 16 || cout % 16) return false;
    if (i + 1 < a.diag_n && cout % 64) return false;   // only the last conv may end inside a 64-channel tile (its zero rows are never stored)
    for (int c = 0; c < cout; c += 64) {
      if (tiles >= DIAG_MAX_TILES || ci / 32 > 15 || wo > 255) return false;
      p0_pk |= (unsigned)(ci / 32) << (4 * tiles);
      np_pk |= (unsigned)(cin / 32) << (4 * tiles);
      wo_pk |= (unsigned long long)wo << (8 * tiles);
      wo += 2 * (cin / 32);   // two channel blocks of cin / 32 phases each
      ++tiles;
    }
    ci += cin; co += cout;
  }
  if (ci != a.Cin || co != a.Cout || a.ldx < a.Cin || a.ldy < a.Cout) return false;
  if ((long)wo * 18 * 1024 >= (1L << 31)) return false;
  if (!planes_geometry<S64>(a, g, true) || g->tiles_ch != tiles) return false;
  g->p0_pk = p0_pk; g->np_pk = np_pk; g->wo_pk = wo_pk;
  return true;
}

// The longest walk of a block, in cycles (the planes cost model per phase + the drain and the barrier behind a tile), when the
// blocks walk units of gsz tiles: the tiles of one slab cost 2 / 4 / 4 / 1 phases on a head level, and a block that walks single
// tiles always meets the same channel tile when the tile count per XCD is a multiple of tiles_ch.
long diag_makespan(const PlanesGeom& g, int gsz, int slots) {
  const int nunits = g.ntiles / gsz, grid = std::min(nunits, slots);
  const long phase = (long)S64::NPB2 * 18 * 33 + (long)((g.npieces + S64::NW - 1) / S64::NW) * 120 + 700, tile = 1500;
  long worst = 0;
  for (int b = 0; b < grid; ++b) {
    long c = 0;
    for (int vb = b; vb < nunits; vb += grid) {
      const int xcd = vb & 7, q = nunits >> 3, r = nunits & 7;
      const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (vb >> 3);
      for (int sub = 0; sub < gsz; ++sub) c += tile + phase * ((g.np_pk >> (4 * ((L * gsz + sub) % g.tiles_ch))) & 15);
    }
    worst = std::max(worst, c);
  }
  return worst;
}
}  // namespace

bool conv3x3_blockdiag_ok(const PlanesArgs& a) {
  PlanesGeom g;
  return diag_geometry(a, &g);
}

int launch_conv3x3_blockdiag(const PlanesArgs& a, hipStream_t s) {
  PlanesGeom g;
  if (!diag_geometry(a, &g)) return -1;
  static int slots = 0;
  if (!slots) {
    if (const int e = prepare_kernel((const void*)planes_kernel<S64, false, true, false>, LDS_MAX)) return e;
    if (const int e = prepare_kernel((const void*)planes_kernel<S64, false, true, true>, LDS_MAX)) return e;
    const int cus = num_cus();
    if (cus <= 0) return -2;
    slots = std::max(cus & ~7, 8);   // as planes_launch
  }
  // the walk: single tiles or whole slabs, whichever ends first; decided once per shape (the forward launches the same few)
  struct Walk { int B, H, W; unsigned np_pk; int gsz; };
  thread_local Walk memo[4] = {};
  thread_local int memo_n = 0;
  int gsz = a.diag_walk == 1 ? 1 : a.diag_walk == 2 ? g.tiles_ch : 0;
  for (int i = 0; !gsz && i < memo_n; ++i)
    if (memo[i].B == a.B && memo[i].H == a.H && memo[i].W == a.W && memo[i].np_pk == g.np_pk) gsz = memo[i].gsz;
  if (!gsz) {
    gsz = diag_makespan(g, g.tiles_ch, slots) < diag_makespan(g, 1, slots) ? g.tiles_ch : 1;
    memo[memo_n % 4] = Walk{a.B, a.H, a.W, g.np_pk, gsz};
    memo_n = std::min(memo_n + 1, 4);
  }
  g.gsz = gsz;
  g.nunits = g.ntiles / gsz;
  const int grid = std::min(g.nunits, slots);
  // every pixel block of a wave is read, also those behind the slab's last row (their results are never stored): the reads of the
  // last one reach 2 PW + 2 storage indices past the block -- inside the allocation for any fill of the slab
  const int reach = g.off_x + g.xrows * ROWB + (32 * S64::NB2 + 2 * g.PW + 3) * ROWB;
  const int lds = std::min(std::max(g.off_s + 1024, (reach + 1023) & ~1023), LDS_MAX);
  auto k = a.stamps ? planes_kernel<S64, false, true, true> : planes_kernel<S64, false, true, false>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(64 * S64::NW), lds, s, a, g);
  return (int)hipGetLastError();
}

int launch_conv3x3_planes(const PlanesArgs& a, hipStream_t s) {
  if (!conv3x3_planes_ok(a)) return -1;
  PlanesGeom g;
  if (a.stride == 2) {
    PlanesGeom g2;
    const long c64 = planes_cost<S64S2>(a, &g), c128 = planes_cost<S128S2>(a, &g2);
    if (c128 >= 0 && (c64 < 0 || c128 < c64)) return planes_launch<S128S2>(a, g2, s);
    return c64 >= 0 ? planes_launch<S64S2>(a, g, s) : -1;
  }
  return planes_geometry<S64>(a, &g) ? planes_launch<S64>(a, g, s) : -1;
}

}  // namespace m355
