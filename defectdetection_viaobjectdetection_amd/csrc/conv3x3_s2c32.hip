// model.1 + model.2.cv1 of YOLOv8s-seg as ONE kernel: Conv3x3 / stride 2 (32 -> 64) + BN + SiLU, then Conv1x1 (64 -> 64) + BN +
// SiLU, NHWC fp16, v_mfma_f32_32x32x16_f16 (gfx950).
//
// Replaces: the second backbone convolution and the first 1x1 of the first C2f block that upstream
// reaches through torch.nn.functional.conv2d (call site: BscanBased/yolo8_seg_predict.py:8).
//
// Why its own kernel.  At batch 32 this pair reads 210 MB (320x320x32 per image) and writes 105 MB: 63 us at the 5 TB/s
// the chip sustains.  On the im2col kernel it took 260-300 us -- 10 % of the whole forward: with Cin = 32 a pixel is a
// 64-byte row, every K step gathers two taps of 128 pixels as 16-byte pieces two pixels apart (half of every 128-byte
// line per request, nine times over through L2), and the L2 -> LDS intake is the bound.  Here a block owns an 8 x 16
// output tile: the 17 x 33-pixel input patch is staged ONCE by LDS-DMA (buffer loads; the padding row / column are
// out-of-range offsets, which write zeros), the 64 x 288 weights of the 3x3 conv and the 64 x 64 weights of the 1x1 conv
// stay in LDS for the block's whole life (persistent blocks), the 3x3 result goes to LDS as fp16 and the 1x1 conv reads
// it from there: the 64-channel intermediate never touches HBM (as in the im2col fusion it replaces: same fp16
// intermediate, so the same rounding points).
//
// Stride-2 gather without bank conflicts: the patch is stored de-interleaved, LDS row ((pr * 2 + parity) * 20 + j) = patch
// pixel (row pr, column 2 j + parity), so the sixteen x positions of a tap read sixteen CONSECUTIVE 64-byte rows of one
// plane (parity = kw & 1, j = x + (kw >> 1)); the 16-byte chunk index is XOR-ed with (j >> 2) & 3 on the DMA source side
// and on the read.  Plane offsets are multiples of 256 bytes, so every ds_read_b128 service group sees sixteen distinct
// 16-byte slots.  Weight rows and the intermediate rows are padded by 16 bytes instead (592 / 144-byte pitch: 37 and 9
// chunks are odd multiples that spread consecutive rows over all sixteen slots); they are written with ds_write.
//
// Block = 8 waves, one block per CU (150 KB of LDS): wave (q = wave & 3, m = wave >> 2) owns tile rows 2q, 2q+1 (one 32-pixel
// MFMA column block) x channels 32 m .. 32 m + 31 of both convolutions.  With four waves (one per SIMD, all 64 channels
// each) the stamps showed a latency-bound tile: 7.8 k cycles for 1.4 k cycles of MFMA (LDS round trips of the 3x3 stage
// 2.8 k, the two SiLU epilogues 2.7 k, DMA issue 1.4 k, nothing to overlap them with); two waves per SIMD interleave
// those phases.  Two barriers per tile: the intermediate is complete (both channel halves) before the 1x1 reads it, and
// the next tile's patch -- issued before this tile's arithmetic -- has landed for every wave.
#include <stdio.h>
#include <stdlib.h>

#include "common.h"
#include "device_prims.h"
#include "launch_util.h"
#include "switches.h"

namespace m355 {
namespace {

constexpr int TH = 8, TW = 16;                 // output tile
constexpr int PR = 2 * TH + 1;                 // 17 patch rows
constexpr int PJ = 20;                         // pixel pitch of a (row, parity) plane: 17 used; 20 * 64 B = 5 * 256 B
constexpr int PROWS = PR * 2 * PJ;             // 680 LDS rows of 64 bytes
constexpr int PGROUPS = (PROWS + 15) / 16;     // 43 DMA pieces of 16 rows
constexpr int PATCH_BYTES = PGROUPS * 1024;    // 44032
constexpr int NWAVES = 8;
constexpr int P_IT = (PGROUPS + NWAVES - 1) / NWAVES;   // pieces per wave
constexpr int W1_PITCH = 592, W2_PITCH = 144, Z_PITCH = 144;
constexpr int W1_OFF = 2 * PATCH_BYTES, W2_OFF = W1_OFF + 64 * W1_PITCH, Z_OFF = W2_OFF + 64 * W2_PITCH;
constexpr int BIAS_OFF = Z_OFF + 128 * Z_PITCH;    // 64 + 64 fp32 biases
constexpr int LDS_BYTES = BIAS_OFF + 512 + 16;     // 154128 (the last 16: the published next-tile index)

// MFMA row rho of a 32-row block holds logical channel 16 h + 4 q + i (rho = 8 q + 4 h + i): lane-half h's 16
// accumulator registers are 16 consecutive channels
__device__ __forceinline__ int chl_of(int R) {
  const int rho = R & 31;
  return (R & ~31) + 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3);
}

template <bool PROBE>
__global__ __launch_bounds__(512, 2) void conv_s2c32_cv1_kernel(const ConvArgs a, int tiles_x, int tiles_y, int ntiles, int dbg) {
  SectionClock<PROBE, 6> clk(a.stamps);   // probe instance only (M355_S2C32_STAMPS): cycles per section and wave
  const unsigned long long t_entry = clk.now(), rt_entry = clk.realtime();
  // dbg: the ablation bits of M355_S2C32_DBG (table: common.h), read by the probe instance only
  auto skip = [&](int bit) __attribute__((always_inline)) { return probe_bit<PROBE>(dbg, bit); };
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.Hi, W = a.Wi;
  const int nwg = gridDim.x;

  // ---- weights into LDS, once per block (plain loads + ds_write: the rows are padded)
  for (int i = tid; i < 64 * 36; i += 64 * NWAVES) {    // W1: 64 rows x 36 chunks (288 halves)
    const int R = i / 36, c = i - R * 36;
    *(float4v*)(smem + W1_OFF + R * W1_PITCH + c * 16) = *(const float4v*)(a.w + (long)chl_of(R) * a.Kpad + c * 8);
  }
  for (int i = tid; i < 64 * 8; i += 64 * NWAVES) {     // W2: 64 rows x 8 chunks (64 halves), logical [co][ci]
    const int R = i >> 3, c = i & 7;
    *(float4v*)(smem + W2_OFF + R * W2_PITCH + c * 16) = *(const float4v*)(a.w2 + (long)chl_of(R) * 64 + c * 8);
  }

  // ---- tile walk (XCD-aware: the virtual blocks of one XCD cover a contiguous run of tiles)
  // Two schedules.  Static (a.tileq == nullptr): block b walks virtual blocks b, b + grid, ...  Dynamic: the first tile is
  // static (tile b), every further one is claimed from a device counter, one tile ahead of its DMA.  A persistent block
  // that needs the whole CU's LDS cannot start while another stream's kernel (the previous batch's NMS, one long block per
  // image) sits on its CU: with the static walk those CUs' 25 tiles each start 50 - 190 us late and the launch takes 150 -
  // 270 us instead of 80 (s_memrealtime of every wave, under the pipelined bench); with the queue the late blocks simply
  // take fewer tiles.
  int* const tq = a.tileq;
  auto decode = [&](int vb, int& tb, int& y0, int& x0) __attribute__((always_inline)) {
    const int xcd = vb & 7, q = ntiles >> 3, r = ntiles & 7;
    const int L = tq ? vb : (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (vb >> 3);
    const int tx = L % tiles_x;
    const int rest = L / tiles_x;
    tb = rest / tiles_y;
    y0 = (rest - tb * tiles_y) * TH;
    x0 = tx * TW;
  };
  const int nimg = a.M / (a.Ho * a.Wo);
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.x, 0, (int)((nimg - 1) * a.x_bstride + (long)H * W * a.ldx) * 2, 0x00020000);
  const int img_stride = (int)a.x_bstride * 2;
  // patch pieces: this wave owns LDS row groups g = wave + 8 i (16 rows each); lane = (row 16 g + lane / 4, chunk slot lane % 4)
  const int prow_l = lane >> 2, pslot = lane & 3;
  // Per lane and piece, tile independent: the byte offset relative to the tile's first patch pixel (2 y0 - 1, 2 x0 - 1) and
  // whether the lane sits on the patch's first row / first column (the only ones that can leave the image: the map is a
  // multiple of the tile, so the last patch row / column is always inside).  A lane past the patch is never valid.
  int prel[P_IT], pvoff[P_IT];
  unsigned ptop = 0, pleft = 0, pdead = 0;
#pragma unroll
  for (int i = 0; i < P_IT; ++i) {
    const int R = 16 * (wave + NWAVES * i) + prow_l;
    const int plane = R / PJ, j = R - plane * PJ;
    const int pr = plane >> 1, par = plane & 1;
    const int cc = pslot ^ ((j >> 2) & 3);
    prel[i] = ((pr * W + 2 * j + par) * a.ldx + cc * 8) * 2;
    if (pr == 0) ptop |= 1u << i;
    if (j == 0 && par == 0) pleft |= 1u << i;
    if (R >= PROWS || j >= 17) pdead |= 1u << i;
  }
  auto patch_offsets = [&](int y0, int x0) __attribute__((always_inline)) {
    const int origin = (((2 * y0 - 1) * W + 2 * x0 - 1) * a.ldx) * 2;   // may be negative for border tiles: those lanes are masked
    const unsigned dead = pdead | (y0 == 0 ? ptop : 0u) | (x0 == 0 ? pleft : 0u);
#pragma unroll
    for (int i = 0; i < P_IT; ++i) pvoff[i] = ((dead >> i) & 1u) ? (int)0x80000000 : origin + prel[i];
  };
  auto issue_patch = [&](int tb, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < P_IT; ++i)
      if (wave + NWAVES * i < PGROUPS) dma16(rs_x, pvoff[i], tb * img_stride, smem + buf * PATCH_BYTES + (wave + NWAVES * i) * 1024);
  };

  // ---- fragment base offsets (tile independent)
  const int l31 = lane & 31, h = lane >> 5, x15 = lane & 15, r2 = (lane >> 4) & 1;
  const int wq = wave & 3, wm = wave >> 2;   // column block (tile rows 2 wq, 2 wq + 1), channel half
  int tb_[3][2];   // patch fragment of (kw, K slice) at kh = 0, buffer 0: this wave's column block (tile rows 2 wq + r2)
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    const int j = x15 + (kw >> 1);
    const int row = ((2 * (2 * wq + r2)) * 2 + (kw & 1)) * PJ + j;
#pragma unroll
    for (int s = 0; s < 2; ++s) tb_[kw][s] = row * 64 + (((2 * s + h) ^ ((j >> 2) & 3)) << 4);
  }
  const int ta1 = W1_OFF + (wm * 32 + l31) * W1_PITCH + h * 16;     // + tap * 64 + s * 32
  const int ta2 = W2_OFF + (wm * 32 + l31) * W2_PITCH + h * 16;     // + s * 32
  const int tz = Z_OFF + (wq * 32 + l31) * Z_PITCH;                 // this lane's intermediate row (pixel wq * 32 + l31)

  // Biases live in LDS, not in registers and not in global memory: hipcc re-loads loop-invariant global values inside the
  // tile loop, and an ordinary VGPR load beside LDS-DMA in flight makes it wait vmcnt(0) -- the patch stream of the next
  // tile would be drained at the top of every tile.  Register r of lane-half h is channel wm * 32 + 16 h + r.
  if (tid < 64) ((float*)(smem + BIAS_OFF))[tid] = a.bias[tid];
  else if (tid < 128) ((float*)(smem + BIAS_OFF))[tid] = a.bias2[tid - 64];
  const int tbias = BIAS_OFF + 16 * h * 4;
  auto bias_vec = [&](int which) __attribute__((always_inline)) {
    float16v v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4v u = *(const float4v*)(smem + tbias + which * 256 + (wm * 32 + q * 4) * 4);
      v[q * 4 + 0] = u[0]; v[q * 4 + 1] = u[1]; v[q * 4 + 2] = u[2]; v[q * 4 + 3] = u[3];
    }
    return v;
  };

  // tile queue: wave 0 claims (one lane, returning atomic, in flight under a whole tile), publishes through LDS
  int* const nslot = (int*)(smem + BIAS_OFF + 512);
  int claim = 0;
  auto claim_issue = [&]() __attribute__((always_inline)) {
    if (wave == 0 && lane == 0) claim = __hip_atomic_fetch_add(tq, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto claim_publish = [&]() __attribute__((always_inline)) {   // after a vmcnt(0) wait, before a barrier
    if (wave == 0 && lane == 0) {
      const int L = nwg + claim;
      *nslot = L < ntiles ? L : -1;
    }
  };
  int vb = blockIdx.x, tb, y0, x0;
  if (tq) claim_issue();
  decode(vb, tb, y0, x0);
  patch_offsets(y0, x0);
  issue_patch(tb, 0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if (tq) {
    claim_publish();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  int nvb = tq ? __builtin_amdgcn_readfirstlane(*nslot) : (vb + nwg < ntiles ? vb + nwg : -1);

  const unsigned long long t_loop = clk.start();
  for (int it = 0;; ++it) {
    const int buf = it & 1;
    const bool more = nvb >= 0;
    int ntb = 0, ny0 = 0, nx0 = 0;
    if (more) {                                   // the next tile's patch streams in under this tile's arithmetic
      decode(nvb, ntb, ny0, nx0);
      patch_offsets(ny0, nx0);
      if (!skip(1)) issue_patch(ntb, buf ^ 1);
      if (tq) claim_issue();                      // ... and so does the claim of the tile after it
    }
    clk.mark(0);   // decode + offsets + DMA issue
    // ---- stage B: 3x3 / s2, K = 9 taps x 32 channels = 18 slices of 16
    float16v acc = bias_vec(0);
    const char* const pb = smem + buf * PATCH_BYTES;
    if (!skip(2))
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap - 3 * kh;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const half8 bf = *(const half8*)(pb + tb_[kw][s] + kh * 2 * PJ * 64);
        const half8 af = *(const half8*)(smem + ta1 + tap * 64 + s * 32);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc, 0, 0, 0);
      }
    }
    clk.mark(1);   // stage B reads + MFMAs
    // SiLU -> fp16 -> this lane's intermediate row (16 channels: two 16-byte writes)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      half8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = acc[half * 8 + j];
        if (a.act) v = m355_silu(v);
        o[j] = m355_to_half(v);
      }
      *(half8*)(smem + tz + (wm * 32 + 16 * h + half * 8) * 2) = o;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (no vmcnt wait here: the next patch keeps streaming)
    if (!skip(8)) __builtin_amdgcn_s_barrier();         // both channel halves of every pixel row are in LDS
    clk.mark(2);   // stage B epilogue + barrier
    // ---- stage C: 1x1, K = 64 = 4 slices over the 32 pixel rows of this column block
    float16v acc2 = bias_vec(1);
    if (!skip(4))
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const half8 bf = *(const half8*)(smem + tz + s * 32 + h * 16);
      const half8 af = *(const half8*)(smem + ta2 + s * 32);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc2, 0, 0, 0);
    }
    clk.mark(3);   // stage C reads + MFMAs
    // the next patch has landed for every wave (and every wave is done reading the intermediate) BEFORE this tile's stores
    // are issued: the wait does not drain them, they fly under the next tile's arithmetic
    int nnvb = -1;
    if (more) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      if (tq) {
        claim_publish();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      if (!skip(8)) __builtin_amdgcn_s_barrier();
      nnvb = tq ? __builtin_amdgcn_readfirstlane(*nslot) : (nvb + nwg < ntiles ? nvb + nwg : -1);
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    clk.mark(4);   // wait for the next patch + barrier
    if (!skip(16)) {
      const int yy = y0 + 2 * wq + r2, xx = x0 + x15;
      half_t* const yp = (half_t*)a.y + (long)tb * a.y_bstride + ((long)yy * a.Wo + xx) * a.ldy + wm * 32 + 16 * h;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        half8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = m355_to_half(m355_silu(acc2[half * 8 + j]));
        *(half8*)(yp + half * 8) = o;
      }
    }
    clk.mark(5);   // stage C epilogue + stores issued
    if (!more) break;
    vb = nvb; nvb = nnvb;
    tb = ntb; y0 = ny0; x0 = nx0;
  }
  if (tq && tid == 0) {   // the last block out re-arms the queue for the next launch (every block's last claim has returned)
    if (__hip_atomic_fetch_add(tq + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nwg - 1) {
      __hip_atomic_store(tq, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(tq + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // words 6, 7: prologue cycles; 100 MHz exit (high half) and entry times
  clk.flush(a.stamps, NWAVES, wave, t_loop - t_entry, (clk.realtime() << 32) | (rt_entry & 0xffffffffull));
}

}  // namespace

// Eligibility: Conv3x3 / s2 / p1 with Cin = 32, Cout = 64 followed by a 64 -> 64 1x1 (both with SiLU), fp16 in and out,
// output map a multiple of the 8 x 16 tile, buffers inside 31-bit byte offsets.
bool conv_s2c32_cv1_ok(const ConvArgs& a) {
  if (a.ksize != 3 || a.stride != 2 || a.pad != 1 || a.Cin != 32 || a.Cout != 64 || a.cout2 != 64 || !a.w2 || !a.bias2) return false;
  if (a.out_f32 || a.convt_co > 0 || a.tmode || a.res || a.phase || a.csplit || a.dec_preds || !a.act) return false;
  if (a.Hi != 2 * a.Ho || a.Wi != 2 * a.Wo || a.Ho % TH || a.Wo % TW || a.ldx % 8 || a.ldy % 8 || a.Kpad < 288) return false;
  const long nimg = a.M / ((long)a.Ho * a.Wo);
  return ((nimg - 1) * a.x_bstride + (long)a.Hi * a.Wi * a.ldx) * 2 < (1L << 31);
}

int launch_conv_s2c32_cv1(const ConvArgs& a, hipStream_t s) {
  if (!conv_s2c32_cv1_ok(a) || !conv_rows_covered(a, 64)) return -1;
  const int tiles_x = a.Wo / TW, tiles_y = a.Ho / TH;
  const int B = a.M / (a.Ho * a.Wo);
  const int ntiles = B * tiles_y * tiles_x;
  static int slots = 0;
  if (!slots) {
    if (const int e = prepare_kernel((const void*)conv_s2c32_cv1_kernel<false>, LDS_BYTES)) return e;
    if (const int e = prepare_kernel((const void*)conv_s2c32_cv1_kernel<true>, LDS_BYTES)) return e;
    const int cus = num_cus();
    if (cus <= 0) return -2;
    slots = cus & ~7;   // one block per CU; the XCD-aware tile order needs gridDim.x % 8 == 0 whenever a block walks > 1 tile
    if (slots < 8) slots = 8;
  }
  const int grid = ntiles <= slots ? ntiles : slots;
  // probe instance (M355_S2C32_STAMPS, M355_S2C32_DBG): per-wave section cycles of the last launch [sync], timing ablations
  static const int dbg = proc_switches().s2c32_dbg, ring = proc_switches().s2c32_ring;
  static const char* st_path = proc_switches().s2c32_stamps;
  auto launch = [&](unsigned long long* st) {
    ConvArgs aa = a;
    aa.stamps = st;
    auto k = st || dbg ? conv_s2c32_cv1_kernel<true> : conv_s2c32_cv1_kernel<false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(64 * NWAVES), LDS_BYTES, s, aa, tiles_x, tiles_y, ntiles, dbg);
  };
  const size_t per_launch = (size_t)slots * NWAVES * 64;
  if (!st_path || ring <= 0) return launch_stamped(st_path, per_launch, (size_t)grid * NWAVES * 64, s, launch);
  // M355_S2C32_RING: the stamps of the last `ring` launches, no synchronisation, written when the process exits
  static StampSink sink;
  static size_t ring_bytes = 0;
  static long launches = 0;
  if (!sink.d) {
    ring_bytes = per_launch * ring;
    if (!sink.alloc(ring_bytes)) return -2;
    atexit([] {
      (void)hipDeviceSynchronize();
      sink.write(st_path, ring_bytes);
    });
  }
  launch(sink.d + (launches++ % ring) * (per_launch / 8));
  return (int)hipGetLastError();
}

}  // namespace m355
