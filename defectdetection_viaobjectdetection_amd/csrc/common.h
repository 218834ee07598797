// Shared declarations for libmi355yolo.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace m355 {

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int BK = 64;  // K elements per main-loop step of the implicit GEMM (one 128-byte LDS row)

// Arguments of the implicit-GEMM convolution kernel (all strides in ELEMENTS of the tensor's dtype).
struct ConvArgs {
  const half_t* x;     // input, NHWC fp16, already offset to the first input channel of the slice
  long x_bstride;      // elements between images
  int ldx;             // elements between pixels (total channels of the underlying buffer)
  int Hi, Wi, Cin;
  const half_t* w;     // packed weights [Cout_pad][Kpad], K = (kh*KS+kw)*Cin + cin
  int Kpad;
  const float* bias;   // [Cout_pad]
  void* y;             // output, fp16 (or fp32 if out_f32), offset to first output channel of the slice
  long y_bstride;
  int ldy;
  int Ho, Wo;          // output spatial size (for convT: equals Hi, Wi -- the GEMM's pixel grid)
  int Cout;            // logical output channels (for convT: 4*Co virtual channels)
  const half_t* res;   // optional residual (same pixel grid as y), offset to slice
  long r_bstride;
  int ldr;
  int ksize, stride, pad;
  int M;               // B*Ho*Wo
  int act;             // 1: SiLU
  int out_f32;         // 1: store fp32
  int convt_co;        // >0: ConvTranspose 2x2/s2 pixel-shuffle store with Co = convt_co
  const half_t* zero;  // >=16 bytes of zeros in device memory (source for padded taps)
  int tmode;           // 1: transposed-stride gather = dgrad of a 3x3 / stride-2 / pad-1 conv (x is dY, y is dX)
  int dbg;             // the bits of the table below (0 in production)
  unsigned long long* stamps;  // probe instances: the stamp buffer (nullptr in production)
  // ---- dbg / stamps.  A kernel's production instance (PROBE = false, device_prims.h) reads neither `stamps` nor an ablation bit; the
  // launcher starts the PROBE = true instance exactly when conv_probe_wanted() holds.  m355_conv2d_fwd puts force_tile >> 8 here.
  //   Ablation bits: skip work, WRONG output by design, timing experiments only (tools/ablate_*.py, tools/stamps_*.py):
  //     bit   conv_igemm          conv3x3_halo / _wide / _small (slab)          conv3x3_m32
  //       1   no activation DMA   no patch DMA of the next chunk                no patch DMA
  //       2   no weight DMA       no weight DMA (halo; wide / slab: unread)     no weight DMA in the loop
  //       4   --                  no SiLU, general epilogue                     no barrier
  //       8   no barrier          no stores, general epilogue                   --
  //      32   no SiLU, general epilogue                                   --                            --
  //     M355_S2C32_DBG (conv3x3_s2c32, its own word): 1 no patch DMA after the first tile, 2 no 3x3 stage, 4 no 1x1 stage,
  //       8 no barrier, 16 no epilogue + stores.  M355_MASK_DBG (postprocess.hip, its own word): 1 zero fill only, 2 no stores;
  //       its bit 4 (plain instead of non-temporal stores) is a path selector.
  //   Path selectors: choose between two correct paths, read at run time by every instance:
  //      64   conv_igemm: persistent grid (M355_PERSIST)
  //     256   general epilogue on every tile (M355_NO_FAST_EPI; igemm, halo, wide, slab, c32)
  //     512   conv_igemm: full wait instead of the counted wait behind a tile's stores
  //   16 and 128 have no reader.
  // Upsample read-through (1x1 convs only): input channels [0, csplit) are NOT in x but in the half-resolution tensor
  // x2 -- output pixel (h, w) reads x2 pixel (h >> 1, w >> 1), i.e. Upsample(2x, nearest) + Concat without the copy.
  const half_t* x2;
  long x2_bstride;
  int ldx2;
  int csplit;          // 0: off
  // Phase convolution (ksize 2, stride 1): the composition ConvTranspose(2x2, s2) -> Conv(3x3, s1, p1) is, for each of
  // the four output phases (py, px), a 2x2 convolution over the LOW-resolution input with window rows h-1+py .. h+py
  // (cols likewise).  Virtual channel q * convt_co + co, q = py * 2 + px, pixel-shuffle store like ConvTranspose; the
  // bias is a [9][convt_co] table indexed by the output pixel's border class (first / interior / last row x column).
  int phase;
  // Phase conv + trailing 1x1 conv (proto.cv3) in the epilogue: y2 = act(w2 . act(phase conv) + bias2), cout2 = 32 output
  // channels, K = convt_co = 128 (one 128 x 128 tile holds every channel of a pixel).  w2: fp16 [32][128] row-major in
  // LOGICAL channel order; the output goes to y (ldy / y_bstride describe the 32-channel tensor).
  const half_t* w2;
  const float* bias2;
  int cout2;
  // Head output conv + decode in one launch (fp32 1x1 conv whose single 128-channel tile holds the whole 64 + nc + nm row
  // of a pixel): the DFL expectation, dist2bbox, the class sigmoid and the coefficient copy of head_decode_kernel run in
  // the epilogue and write the prediction rows; the raw map is written too only when dec_keep_raw is set.
  float* dec_preds;        // (B, dec_A, 4 + nc + nm) fp32; nullptr: off
  int dec_A, dec_level_off, dec_nc, dec_nm, dec_keep_raw;
  float dec_stride;
  // Rows of the packed weight buffer `w` and floats of `bias` the caller allocated (0: conv_cout_pad(Cout), the
  // engine's padding).  Every launcher refuses a channel tile whose ceil(Cout / tile) * tile rows exceed it: the
  // kernels fetch whole weight-row tiles by LDS-DMA with no per-row bound.
  int w_rows;
  // Tile queue of the persistent kernels: two ints in device memory, zero before the first launch (the kernel re-arms
  // them): [0] tiles claimed beyond each block's static first one, [1] blocks that have left.  nullptr: static walk.
  // One queue per op -- never shared by launches that can run at the same time.
  int* tileq;
  // Fragment-ordered copy of `w` for the weights-in-registers kernels (conv1x1_wreg, conv3x3_s2c64, ...): fragment
  // f at halves [f * 512, f * 512 + 512), lane-linear 16 bytes = the A operand of one 32x32x16 MFMA.  nullptr: the kernels
  // gather the fragments from `w` (64 scattered 16-byte loads per fragment).
  const half_t* wf;
  const half_t* wf2;   // the same for `w2` (proto_phase_wreg.hip: the eight fragments of proto.cv3)
  int bias_lds;        // set by the implicit-GEMM launcher: this many bias floats are staged in LDS behind the stages (0: none)
};

// the ablation bits each kernel family reads (the table at ConvArgs::dbg), and when a launcher takes the probe instance
constexpr int DBG_ABLATE_IGEMM = 1 | 2 | 8 | 32, DBG_ABLATE_HALO = 1 | 2 | 4 | 8, DBG_ABLATE_M32 = 1 | 2 | 4;
inline bool conv_probe_wanted(const ConvArgs& a, int ablation_bits) { return a.stamps || (a.dbg & ablation_bits); }

// tile ids for launch_conv_igemm(force_tile)
enum { TILE_AUTO = -1, TILE_128x128 = 0, TILE_64x128 = 1, TILE_32x256 = 2, TILE_64x256 = 3, TILE_64x128W8 = 5, TILE_HALO = 16, TILE_HALO8W = 17, TILE_HALO4W = 18, TILE_HALOWIDE = 19, TILE_C32 = 20, TILE_SLAB = 25, TILE_M32 = 26, TILE_M32_128 = 27, TILE_M32_64x16 = 28, TILE_M32_64x8 = 29, TILE_W1 = 32, TILE_PLANES = 33 };

// (the M355_* environment switches and their three lifetimes: switches.h)

int launch_conv_igemm(const ConvArgs& a, int force_tile, hipStream_t s);
// tile heuristic: cout = (virtual) output channels, M = output pixels of the whole batch
int conv_pick_tile(int cout, long M);
// rows the packed weight buffer must be padded to for a given Cout (multiple of the channel tile)
int conv_cout_pad(int cout);
int conv_kpad(int cin, int ksize);
// true when a launch with channel tile `bch` stays inside the weight / bias rows the caller provided
inline bool conv_rows_covered(const ConvArgs& a, int bch) {
  const int need = (a.Cout + bch - 1) / bch * bch;
  return need <= (a.w_rows > 0 ? a.w_rows : conv_cout_pad(a.Cout));
}
// (channel, pixel) extent of a forced tile id of m355_conv2d_fwd; false for ids no launcher implements
bool conv_forced_tile_extent(int tile, int cout, int* bch, int* bpx);

// 3x3 stride-1 halo-tile kernel (conv3x3_halo.hip)
bool conv3x3_halo_ok(const ConvArgs& a);
int launch_conv3x3_halo(const ConvArgs& a, int variant, hipStream_t s);  // variant 0 auto, 1: 16x16 px / 8 waves, 2: 8x16 px / 4 waves, 3: wide
// the kernel variant 0 runs on a call conv3x3_halo_ok takes: TILE_M32, TILE_HALOWIDE or TILE_HALO (M355_NO_WIDE / M355_NO_M32 as given)
int conv3x3_halo_pick(const ConvArgs& a, bool no_wide, bool no_m32);
// 128 ch x 16x16 px, K depth 32 per step (conv3x3_wide.hip)
bool conv3x3_wide_ok(const ConvArgs& a);
int launch_conv3x3_wide(const ConvArgs& a, hipStream_t s);
// v_mfma_f32_32x32x16_f16 halo kernel (conv3x3_m32.hip); which: 0 = by shape, 1 = <128 ch, 8 rows>, 2 = <64, 16>, 3 = <64, 8>
bool conv3x3_m32_ok(const ConvArgs& a);
int launch_conv3x3_m32(const ConvArgs& a, int which, hipStream_t s);
// Conv3x3 / s2 (32 -> 64) + Conv1x1 (64 -> 64) in one persistent patch kernel (conv3x3_s2c32.hip): a.w2 / a.bias2 / a.cout2 set
bool conv_s2c32_cv1_ok(const ConvArgs& a);
int launch_conv_s2c32_cv1(const ConvArgs& a, hipStream_t s);
// narrow maps (W <= 26): slabs of full-width rows, linear pixel groups (conv3x3_small.hip)
bool conv3x3_slab_ok(const ConvArgs& a);
int launch_conv3x3_slab(const ConvArgs& a, hipStream_t s);
// D-FINE decoder ops (dfine_kernels.hip), head_dim 32.  The caller (dfine_entries.hip) has validated every argument.
struct MsdaLevels { int L; int lh[8], lw[8], lstart[8], pend[8]; };   // per level: height, width, first pixel, one past its last point
int launch_msda(const float* value, const float* loc, const float* attn, float* out, int B, int S, int H, int Q, int P,
                const MsdaLevels& lv, int discrete, hipStream_t s, const float* ref = nullptr, float offset_scale = 0.f);
int launch_dfine_decode(const float* dist, const float* project, const float* ref, float* boxes, long n, int nbins1,
                        float reg_scale, int clamp01, hipStream_t s, bool guard = false);   // guard: the trainers' nan_to_num chain
// The temporal head of the D-FINE trainers (dfine_temporal.hip): frame fusion, guarded class logits, the no-object cross-entropy of
// every frame and the frame-to-frame consistency loss, each with its backward.  The caller has validated every argument.
int dfine_tfuse_max_t();
int dfine_noobject_max_q();
int launch_dfine_tfuse_forward(const float* fused, const float* scores, const float* ctx, int T, int Q, int D, float* out, float* stats,
                               hipStream_t s);   // ctx and stats (2, Q) may be nullptr
int launch_dfine_tfuse_backward(const float* g, const float* fused, const float* scores, const float* stats, int T, int Q, int D,
                                float* d_fused, float* d_scores, hipStream_t s);   // either may be nullptr; fused is read for d_scores
int launch_dfine_guard_logits(const float* cls, const float* an, long rows, int C1, float bound, float* out, hipStream_t s);
int launch_dfine_guard_logits_backward(const float* g, const float* cls, const float* an, long rows, int C1, float bound, float* d_cls,
                                       float* d_an, hipStream_t s);
int launch_dfine_noobject_forward(const float* x, int T, int Q, int C, int cls, float* out, hipStream_t s);
int launch_dfine_noobject_backward(const float* g, const float* x, int T, int Q, int C, int cls, float* dx, hipStream_t s);
size_t dfine_consistency_workspace_bytes(int T, long N);
int launch_dfine_consistency_forward(const float* a, int T, long N, float* work, float* out, hipStream_t s);   // two launches; T >= 2
int launch_dfine_consistency_backward(const float* g, const float* a, int T, long N, float* da, hipStream_t s);
// Hungarian matcher of the D-FINE loss (dfine_match.hip): cost matrix + assignment, one block per image.  The caller has
// validated every argument; `work` holds dfine_match_workspace_bytes(B, Q, nmax) bytes (0: the matrices fit in LDS).
size_t dfine_match_workspace_bytes(int B, int Q, int nmax);
int launch_dfine_match(const float* logits, const float* boxes, int B, int Q, int C, const long long* labels, const float* tboxes,
                       const int* d_offsets, int T, int nmax, float class_cost, float bbox_cost, float giou_cost, float alpha,
                       float gamma, int focal, void* work, float* cost_out, long long* rows, long long* cols, int kmax, int* flags,
                       hipStream_t s);
// Detection post-processing of a D-FINE / RT-DETR output (dfine_postprocess.hip): top-Q rows of sigmoid(logits) with label, scaled
// xyxy box and the {n_nan, n_keep} counts, one block per image.  The caller has validated every argument; sizes may be nullptr.
int launch_dfine_postprocess(const float* logits, const float* boxes, int B, int Q, int C, const float* sizes, float threshold,
                             float* scores, long long* labels, float* out_boxes, int* counts, hipStream_t s);
// Image pre-processing of a D-FINE / RT-DETR model (dfine_preprocess.hip): Pillow's 8-bit BILINEAR resize + rescale of T packed
// uint8 RGB images into fp32 (T, 3, out_h, out_w), the horizontal pass into the uint8 scratch `mid` and the vertical pass, two
// launches (one when h_max_rows == 0: no image has a horizontal pass).  d_images / d_axes: device arrays of m355_dfine_pre_image /
// m355_dfine_pre_axis; h_max_rows, h_max_w: the largest in_h and in_w among the images with a horizontal pass.  The caller has
// validated every argument and table; dfine_preprocess_lds_bytes(h_max_w) is the horizontal launch's dynamic LDS.
size_t dfine_preprocess_lds_bytes(int max_in_w);
int launch_dfine_preprocess(const uint8_t* src, const void* d_images, int T, const void* d_axes, const int* d_pool,
                            const float* rescale, int out_h, int out_w, uint8_t* mid, int h_max_rows, int h_max_w, float* out,
                            hipStream_t s);
// Encoder query selection of DFineModel.forward (dfine_select.hip): the K tokens with the greatest row max of class_logits per image
// (the order of topk_select.h), their indices, the gathered coordinate / class / memory rows, sigmoid of the coordinate rows and the
// inverse map (rank or -1 per token); the backward writes the three input gradients in full through that map.  The caller has
// validated every argument; mem / target, inverse and every pointer of the backward but `inverse` may be nullptr.  scores: the
// forward's workspace, dfine_select_workspace_bytes(B, S).
size_t dfine_select_workspace_bytes(int B, int S);
int launch_dfine_select_forward(const float* cls, const float* coord, const float* mem, int B, int S, int C, int D, int K, float* scores,
                                long long* indices, float* ref, float* boxes, float* logits, float* target, int* inverse, hipStream_t s);   // two launches
int launch_dfine_select_backward(const float* g_ref, const float* g_boxes, const float* g_logits, const float* g_target, const float* boxes,
                                 const int* inverse, int B, int S, int C, int D, int K, float* d_cls, float* d_coord, float* d_mem,
                                 hipStream_t s);   // one launch
// Loss terms of one D-FINE decoder output (dfine_loss.hip): loss_vfl, loss_bbox, loss_giou and, with the local group
// (pred_corners != nullptr), loss_fgl and loss_ddf.  The caller has validated every argument.
struct DfineLossArgs {
  const float* logits;            // (B, Q, C)
  const float* boxes;             // (B, Q, 4) cx, cy, w, h
  const long long* match_q;       // (M) query index of each match entry, the entries of image b contiguous
  const long long* match_t;       // (M) target index within the image
  const int* offsets;             // device, 2 (B + 1): first entry of each image, then first target row of each image
  const long long* labels;        // (T)
  const float* tboxes;            // (T, 4)
  int B, Q, C, M, T;
  float num_boxes, alpha, gamma;
  const float* pred_corners;      // (B, Q, 4 * nb1) or nullptr: no local group
  const float* ref_points;        // (B, Q, 4)
  const float* teacher_corners;   // (B, Q, 4 * nb1)
  const float* teacher_logits;    // (B, Q, C)
  const float* project;           // (nb1) W(n)
  int nb1;
  float reg_scale, temperature;
  float* partials;                // dfine_loss_workspace_bytes(B, Q)
  float* out;                     // (8): the five terms, two DDF gradient coefficients, 0
  const float* grad_terms;        // backward: (5) upstream gradients, device
  float* grad_logits;             // backward: any of the three may be nullptr
  float* grad_boxes;
  float* grad_corners;
};
size_t dfine_loss_workspace_bytes(int B, int Q);
int launch_dfine_loss_forward(const DfineLossArgs& a, hipStream_t s);    // two launches
int launch_dfine_loss_backward(const DfineLossArgs& a, hipStream_t s);   // one launch
// The temporal encoder layer between its GEMMs: attention core on the packed (B, S, 3 * 32 H) projection and dropout(relu(h))
// (dfine_encoder.hip), LayerNorm(x + dropout(y)) (dfine_rowln.hip), each with its backward, and the dropout keep-mask they share
// (p = 0: no mask).  The caller has validated every argument; all tensors contiguous fp32, 16-byte aligned.
int launch_dfine_attn_forward(const float* qkv, int B, int S, int H, float p, unsigned long long seed, int site, float* out,
                              float* lse, hipStream_t s);                                  // lse may be nullptr
int launch_dfine_attn_backward(const float* gout, const float* qkv, const float* out, const float* lse, int B, int S, int H, float p,
                               unsigned long long seed, int site, float* gqkv, hipStream_t s);
int dfine_addln_max_d();
size_t dfine_addln_workspace_bytes(long M, int D);
int launch_dfine_addln_forward(const float* x, const float* y, const float* w, const float* b, long M, int D, float eps, float p,
                               unsigned long long seed, int site, float* out, float* mean, float* rstd, hipStream_t s);
int launch_dfine_addln_backward(const float* g, const float* x, const float* y, const float* w, const float* mean, const float* rstd,
                                long M, int D, float p, unsigned long long seed, int site, float* dx, float* dy, float* dweight,
                                float* dbias, float* work, hipStream_t s);                 // two launches
// LayerNorm(clamp(x + y, lo, hi)), no dropout: another source of the same kernels; zero gradient where the sum lies strictly
// outside [lo, hi]
int launch_dfine_addln_clamp_forward(const float* x, const float* y, const float* w, const float* b, long M, int D, float eps, float lo,
                                     float hi, float* out, float* mean, float* rstd, hipStream_t s);
int launch_dfine_addln_clamp_backward(const float* g, const float* x, const float* y, const float* w, const float* mean,
                                      const float* rstd, long M, int D, float lo, float hi, float* dx, float* dy, float* dweight,
                                      float* dbias, float* work, hipStream_t s);
// D-FINE decoder layers between their GEMMs.  gate_ln (dfine_rowln.hip): LayerNorm(sigmoid(g[:, :D]) x1 + sigmoid(g[:, D:]) x2),
// g (M, 2 D); the backward's dg, dx1, dx2, dweight, dbias may each be nullptr, work as for addln (dfine_addln_workspace_bytes).
int launch_dfine_gate_ln_forward(const float* g, const float* x1, const float* x2, const float* w, const float* b, long M, int D,
                                 float eps, float* out, float* mean, float* rstd, hipStream_t s);
int launch_dfine_gate_ln_backward(const float* gout, const float* g, const float* x1, const float* x2, const float* w, const float* mean,
                                  const float* rstd, long M, int D, float* dg, float* dx1, float* dx2, float* dweight, float* dbias,
                                  float* work, hipStream_t s);
// lqe (dfine_decoder.hip): per (row, side) softmax over nb1 logits, the k largest probabilities in descending order, their mean -> stat (M, 4 (k + 1));
// idx (M, 4, k) bytes (may be nullptr in the forward): the chosen bins, an exact tie to the lowest bin
int launch_dfine_lqe_forward(const float* corners, long M, int nb1, int k, float* stat, unsigned char* idx, hipStream_t s);
int launch_dfine_lqe_backward(const float* gstat, const float* corners, const unsigned char* idx, long M, int nb1, int k,
                              float* gcorners, hipStream_t s);
// The decoder's own loop around its layers (dfine_loop.hip).  query_pos: out (N, H) = relu(ref (N, 4) @ w (H, 4)^T + b), H % 4 == 0;
// the backward's dref, dweight, dbias may each be nullptr, work (dfine_query_pos_workspace_bytes) holds the slabs' partial rows of
// dweight | dbias.  refine_reference: sigmoid(delta + inverse_sigmoid(ref, eps)) on n elements; its backward reads the output.
// refine_boxes: pred = delta + prev (prev == nullptr: nothing written, pred is delta) and boxes = distance2bbox(points,
// integral(pred, project), reg_scale); the backward writes gcorners = gpred (may be nullptr) + d boxes / d pred . gboxes and gpoints
// (may be nullptr).
int launch_dfine_query_pos_forward(const float* ref, const float* w, const float* b, long N, int H, float* out, hipStream_t s);
size_t dfine_query_pos_workspace_bytes(long N, int H);
int launch_dfine_query_pos_backward(const float* gout, const float* out, const float* ref, const float* w, long N, int H, float* dref,
                                    float* dweight, float* dbias, float* work, hipStream_t s);
int launch_dfine_refine_reference_forward(const float* delta, const float* ref, long n, float eps, float* out, hipStream_t s);
int launch_dfine_refine_reference_backward(const float* gout, const float* out, long n, float* gdelta, hipStream_t s);
int launch_dfine_refine_boxes_forward(const float* delta, const float* prev, const float* project, const float* points, long N, int nb1,
                                      float reg_scale, float* pred, float* boxes, hipStream_t s);
int launch_dfine_refine_boxes_backward(const float* gpred, const float* gboxes, const float* pred, const float* project,
                                       const float* points, long N, int nb1, float reg_scale, float* gcorners, float* gpoints,
                                       hipStream_t s);
// saved == nullptr: out = dropout(relu(in)); else the backward: in = grad_out, saved = the forward's output
int launch_dfine_relu_dropout(const float* in, const float* saved, float* out, long n, float p, unsigned long long seed, int site,
                              hipStream_t s);
int launch_dfine_keep_mask(unsigned char* mask, long n, float p, unsigned long long seed, int site, hipStream_t s);
// NCHW maps <-> token rows and the exact GELU (dfine_layout.hip).  Levels: pixels and first token per level, S tokens in all.
// maps_to_tokens: maps[l] (B, D, h_l, w_l) -> tokens (B, S, D) and, with pos (S, D) or mask (S), extra = tokens + pos or mask * tokens.
// tokens_to_maps: maps[l] = tokens (+ extra (* mask)); tokens or extra may be nullptr, not both.  gelu: saved == nullptr: out =
// gelu(in); else the backward: in = grad_out, saved = the forward's input.  The caller has validated every argument, the grid
// (dfine_layout_blocks) included; maps, tokens, extra and pos 16-byte aligned.
struct DfineLayoutLevels { int L; int hw[8], start[8]; long S; };
long dfine_layout_blocks(const DfineLayoutLevels& lv, int B, int D);
int launch_dfine_maps_to_tokens(const float* const* maps, const DfineLayoutLevels& lv, int B, int D, const float* pos, const float* mask,
                                float* tokens, float* extra, hipStream_t s);
int launch_dfine_tokens_to_maps(const float* tokens, const float* extra, const float* mask, const DfineLayoutLevels& lv, int B, int D,
                                float* const* maps, hipStream_t s);
int launch_dfine_gelu(const float* in, const float* saved, float* out, long n, hipStream_t s);
// their backward (dfine_backward.hip).  Any grad_* may be nullptr (not needed); `work` holds the contribution list of
// grad_value and the per-head partials of grad_ref (msda_backward_workspace_bytes, needed for those two only).  The caller has
// validated every argument.  msda_backward_value_blocks: the grid of the grad_value pass and its ownership split (own, blk0[9]).
size_t msda_backward_workspace_bytes(int B, int Q, int H, int P);
long msda_backward_value_blocks(const MsdaLevels& lv, int B, int H, int* own, int* blk0);
int launch_msda_backward(const float* grad_out, const float* value, const float* loc, const float* attn, float* grad_value,
                         float* grad_loc, float* grad_attn, int B, int S, int H, int Q, int P, const MsdaLevels& lv, int discrete,
                         void* work, hipStream_t s, const float* ref = nullptr, float offset_scale = 0.f, float* grad_ref = nullptr);
int launch_dfine_decode_backward(const float* grad_boxes, const float* dist, const float* project, const float* ref,
                                 float* grad_dist, float* grad_ref, long n, int nbins1, float reg_scale, int clamp01,
                                 hipStream_t s, bool guard = false);
// The end of the trainers' step (dfine_optim.hip): squared gradient norm, clip and Adam / AdamW update over a device table of
// m355_dfine_optim_row (count rows, `chunks` chunks in all = the grid).  norm: two floats, the norm and the clip coefficient, written
// by launch_dfine_grad_norm from the chunks' partial sums; launch_dfine_adam applies the coefficient when norm is not nullptr.
int launch_dfine_grad_sumsq(const void* d_table, int count, int chunks, float* partials, hipStream_t s);
int launch_dfine_grad_norm(const float* partials, int chunks, float max_norm, float* norm, hipStream_t s);
int launch_dfine_clip_scale(const void* d_table, int count, int chunks, const float* norm, hipStream_t s);
int launch_dfine_adam(const void* d_table, int count, int chunks, bool adamw, const float* norm, hipStream_t s);
// The recurrence of a one-layer GRU with hidden size 256 (dfine_gru.hip): every chain (sequence x direction) on 8 persistent
// workgroups, one launch each way.  dfine_gru_check: nullptr = the shape is taken, else why not.  work: the exchange ring first
// (zeroed on the stream by the launchers), then the saved gates when `keep` / in the backward; status: one sticky int32.
const char* dfine_gru_check(int B, long S, int H, int D);
size_t dfine_gru_workspace_bytes(int B, long S, int H, int D);   // S == 0: the ring alone
int launch_dfine_gru_forward(const float* gi, const float* w_hh, const float* b_hh, const float* h0, int B, int S, int D, float* out,
                             float* h_n, void* work, bool keep, int* status, hipStream_t s);
int launch_dfine_gru_backward(const float* gout, const float* gh_n, const float* w_hh, const float* h0, const float* out, int B, int S,
                              int D, float* ggi, float* gan, float* gh0, void* work, int* status, hipStream_t s);
// 1x1, K <= 512, Cout % 128 == 0: weights in registers, persistent (conv1x1_wreg.hip)
bool conv1x1_wreg_ok(const ConvArgs& a);
int launch_conv1x1_wreg(const ConvArgs& a, hipStream_t s);
// The output convs of one head level + the decode of their rows in one launch (head_tail.hip): x = the level's 224-channel
// branch tensor (64 box | 128 class | 32 coefficient channels), dense rows; wf = 18 MFMA fragments (box 2 x 4, class 8,
// coefficients 2) of the block-diagonal weight matrix; bias = [64 | nc | nm]; preds = (B, A, 4 + nc + nm) fp32.
struct HeadTailArgs {
  const half_t* x;
  int ldx;             // 224
  long M;              // B * H * W pixels of the level
  int HW, W;           // anchors of the level per image, grid width
  float stride;
  int A, level_off, nc, nm;
  const half_t* wf;
  const float* bias;
  float* preds;
};
bool head_tail_ok(const HeadTailArgs& a);
int launch_head_tail(const HeadTailArgs& a, hipStream_t s);
// 3x3 / s2 (64 -> 128) + 1x1 (128 -> 128): model.3 + model.4.cv1 of the s scale, 3x3 weights in registers (conv3x3_s2c64.hip)
bool conv_s2c64_cv1_ok(const ConvArgs& a);
int launch_conv_s2c64_cv1(const ConvArgs& a, hipStream_t s);
// the composed Proto launch (phase conv + proto.cv3) with the weights in registers, one phase per block (proto_phase_wreg.hip)
bool proto_phase_wreg_ok(const ConvArgs& a);
int launch_proto_phase_wreg(const ConvArgs& a, hipStream_t s);
// Cin = Cout = 32, weights-stationary persistent halo kernel (conv3x3_c32.hip)
bool conv3x3_c32_ok(const ConvArgs& a);
int launch_conv3x3_c32(const ConvArgs& a, hipStream_t s);

// A whole C2f block body with 32 hidden channels in one launch (c2f_c32.hip): t = Conv3x3(y1), y2 = y1 + Conv3x3(t),
// out = Conv1x1([y0, y1, y2]); x holds [y0, y1] (what C2f.cv1 wrote) in its first 64 channels.
struct C2fC32Args {
  const half_t* x; long x_bstride; int ldx;      // NHWC fp16, channels [0, 32) = y0, [32, 64) = y1
  int H, W, B;
  const half_t *waf, *wbf;                       // fragment-ordered wa (plain rows) / wb (operand rows), 18 x 512 halves each; nullptr: gather
  const half_t *wa, *wb, *wc;                    // packed fp16 rows [32][kpad_a], [32][kpad_b] (K = tap * 32 + cin), [64][kpad_c] (K = y0, y1, y2)
  int kpad_a, kpad_b, kpad_c;
  const float *ba, *bb, *bc;                     // folded biases: 32, 32, 64 floats
  half_t* y; long y_bstride; int ldy;            // 64 output channels
  int shortcut;                                  // 1: y2 = y1 + ...
};
bool c2f_c32_ok(const C2fC32Args& a);
int launch_c2f_c32(const C2fC32Args& a, hipStream_t s);

// Row-slab 3x3 kernels (conv3x3_planes.hip): a whole Bottleneck -- y = [x +] act(conv3x3(act(conv3x3(x, wa) + ba), wb) + bb), hidden
// tensor in LDS -- or one 3x3 conv y = act(conv3x3(x, wb) + bb) [+ res].  Weights as MFMA A fragments in K-loop order
// (planes_frag_pack in weight_pack.hip): fragment ((cb * NP + p) * 9 + tap) * 2 + s = rows 32 cb .. + 31 (plain row permutation),
// K = tap * Cin + 32 p + 16 s .. + 15; 1 KiB each, lane-linear.
struct PlanesArgs {
  const half_t* x; long x_bstride; int ldx;      // NHWC fp16 input slice (Cin channels)
  int H, W, B, Cin, Cout;                        // H, W: INPUT map
  int stride;                                    // 1, or 2 (single mode only: output map H / 2 x W / 2)
  const half_t *wfa, *wfb; int cblocks_a, cblocks_b;   // fragment-ordered weights and their 32-channel blocks; wfa / ba: first conv of a pair (nullptr in single mode)
  const float *ba, *bb;
  half_t* y; long y_bstride; int ldy;
  const half_t* res; long r_bstride; int ldr;    // optional residual (the shortcut of a Bottleneck: x itself)
  int act;
  unsigned long long* stamps;                    // probe instances: 2 x 8 uint64 per wave (nullptr in production)
  // block-diagonal single mode (launch_conv3x3_blockdiag): diag_n convs side by side, conv i = the next diag_cin[i] input channels ->
  // the next diag_cout[i] output channels (Cin / Cout = their sums; every cout but the last a multiple of 64).  wfb = the convs'
  // planes_frag_pack_padded lists one after the other (each over its OWN input planes), bb = their biases at their channel offsets,
  // padded with zeros to a multiple of 64 floats.
  int diag_n;
  int diag_cin[4], diag_cout[4];
  int diag_walk;                                 // 0: the launcher chooses how a block walks the tiles; tests: 1 single tiles, 2 whole slabs
};
bool bneck_pair_shape_ok(int C, int H, int W);
bool bneck_pair_ok(const PlanesArgs& a);
int launch_bneck_pair(const PlanesArgs& a, hipStream_t s);
bool conv3x3_planes_ok(const PlanesArgs& a);
int launch_conv3x3_planes(const PlanesArgs& a, hipStream_t s);
bool conv3x3_blockdiag_ok(const PlanesArgs& a);
int launch_conv3x3_blockdiag(const PlanesArgs& a, hipStream_t s);

struct StemArgs {
  const uint8_t* x; int B, H, W;     // uint8 NHWC (B,H,W,3)
  const half_t* w16;                 // [Cout][32] fp16: k = (kh*3+kw)*3+ci, rows 27..31 zero; NOT scaled by 1/255
  const float* bias;                 // [Cout]
  half_t* y; long y_bstride; int ldy; int Cout;
};
int launch_stem(const StemArgs& a, hipStream_t s);
// YOLOv5u stem: Conv 6x6 / s2 / p2, 3 -> C0 (16, 32, 48) on the uint8 image (conv_stem6_s2.hip)
struct Stem6Args {
  const uint8_t* x; int B, H, W;     // uint8 NHWC (B,H,W,3); W a multiple of 16, H even
  const half_t* w;                   // [C0][128] fp16 in the kernel's row order (pack_stem6_weights); NOT scaled by 1/255
  const float* bias;                 // [C0], channel order
  half_t* y; long y_bstride; int ldy; int C0;
};
bool stem6_ok(const Stem6Args& a);
int launch_stem6(const Stem6Args& a, hipStream_t s);
void pack_stem6_weights(const float* w, int C0, half_t* out);   // (C0,3,6,6) fp32 -> [C0][128] fp16 (host)
// YOLO11 depthwise 3x3 / s1 / p1 conv on fp16 NHWC channel slices (dwconv3x3.hip)
struct DwConvArgs {
  const half_t* x; long x_bstride; int ldx;   // first channel of the input slice; ldx a multiple of 8
  int B, H, W, C;                             // C a multiple of 8
  const half_t* w;                            // [9][C] fp16, tap k = dy * 3 + dx (pack_dw3x3_weights)
  const float* bias;                          // [C] (BN folded)
  int act;                                    // 1: SiLU
  half_t* y; long y_bstride; int ldy;         // first channel of the output slice; ldy a multiple of 8
};
bool dwconv3x3_ok(const DwConvArgs& a);
int launch_dwconv3x3(const DwConvArgs& a, hipStream_t s);
void pack_dw3x3_weights(const float* w, int C, half_t* out);   // (C,1,3,3) fp32 -> [9][C] fp16 (host)
// YOLO11 C2PSA attention: o + pe(v) of every head in one launch (psa_attn.hip); key_dim 32, head_dim 64
struct PsaArgs {
  const half_t* qkv; long q_bstride; int ldq; // (B, H, W, ldq): head h's [q 32 | k 32 | v 64] at channel 128 h
  int B, H, W, heads, C;                      // C = 64 heads (channels of the result and of pe)
  const half_t* pe_w;                         // [9][C] fp16 (pack_dw3x3_weights of attn.pe, BN folded)
  const float* pe_b;                          // [C]
  float scale_log2e;                          // key_dim^-0.5 * log2(e)
  half_t* y; long y_bstride; int ldy;         // (B, H, W, ldy): channel 64 h + c
};
bool psa_attn_ok(const PsaArgs& a);
int launch_psa_attn(const PsaArgs& a, hipStream_t s);
// stem + model.1 + model.2.cv1 in one launch (conv_stem_s2c32.hip): a = the model.1 + cv1 launch, st = the stem launch
bool stem_s2c32_ok(const ConvArgs& a, const StemArgs& st);
int launch_stem_s2c32(const ConvArgs& a, const StemArgs& st, hipStream_t s);
// the same launch with team X building the next tile's patch image while team Y runs the two convolutions (conv_stem_c2.hip)
bool stem_s2c32_v2_ok(const ConvArgs& a, const StemArgs& st);
int launch_stem_s2c32_v2(const ConvArgs& a, const StemArgs& st, hipStream_t s);

int launch_sppf_pool(const half_t* x, long x_bstride, int ldx, half_t* y, long y_bstride, int ldy,
                     int B, int H, int W, int C, hipStream_t s);
// the instance launch_sppf_pool runs: cg | (owned << 8), or -1 where it refuses (host arithmetic only; misc_kernels.hip)
int sppf_pool_form(int B, int H, int W, int C, int ldy);
int launch_sppf_pool_bwd(const half_t* a, long a_bs, int lda, const half_t* y, long y_bs, int ldy, const half_t* gy, long gy_bs,
                         int ldgy, half_t* ga, long ga_bs, int ldga, int B, int H, int W, int C, int accumulate, hipStream_t s);
int launch_upsample2x(const half_t* x, long x_bstride, int ldx, half_t* y, long y_bstride, int ldy,
                      int B, int H, int W, int C, hipStream_t s);
// ADown's pooling (yolov9c): a = avg_pool2d(x, 2, 1, 0)[..., :C/2] (H-1 x W-1), m = max_pool2d(avg_pool2d(x, 2, 1, 0)[..., C/2:], 3, 2, 1) (H/2 x W/2)
int launch_adown_pool(const half_t* x, long x_bstride, int ldx, half_t* a, long a_bstride, int lda, half_t* m, long m_bstride,
                      int ldm, int B, int H, int W, int C, hipStream_t s);
int launch_head_decode(const float* raw, int B, int in_h, int in_w, int nc, int nm, float* preds,
                       hipStream_t s);
// agnostic != 0: no class offset.  class_mask: device bitmask of nc bits (bit c of word c / 32; nc <= 1024) -- an anchor is a
// candidate only if its argmax class is in the set; NULL = every class.
int launch_nms(const float* preds, int B, int A, int nc, int nm, float conf, float iou, int max_det,
               float* dets, int* counts, void* workspace, size_t workspace_bytes, hipStream_t s, int agnostic = 0,
               const uint32_t* class_mask = nullptr);
size_t nms_workspace_bytes(int B, int A);
int launch_proto_masks(const float* dets, const int* counts, const half_t* protos, int B, int max_det,
                       int nm, int mh, int mw, int in_h, int in_w, uint8_t* masks, hipStream_t s);
// Native-resolution masks (proto_masks_native.hip, upstream process_mask_native) for images [0, B) of one launch group:
// h_orig_hw int32 (B,2) and h_offsets int64 (B+1) are HOST arrays (image b's masks are the bytes [h_offsets[b],
// h_offsets[b+1]) of out, one h0*w0 plane per detection slot); boxes f32 (B,max_det,4) in original pixels.  Host-checked
// arguments: see m355_proto_masks_native.  Returns 0 or a negative / HIP error code.
int launch_proto_masks_native(const float* dets, const int* counts, const half_t* protos, int B, int max_det, int mh, int mw,
                              const int* h_orig_hw, const float* boxes, const int64_t* h_offsets, uint8_t* out,
                              hipStream_t s);
// The prototype-grid crop of process_mask_native for one image (rows [*top, *top + *ch), cols [*left, *left + *cw)).
void native_mask_crop(int mh, int mw, int h0, int w0, int* top, int* left, int* ch, int* cw);

// weight gradient (conv_wgrad.hip): dw fp32 [Cout][k*k*Cin] (KRSC).  Split-K partial slabs go to the caller's workspace
// (conv_wgrad_workspace_bytes) and are added in a fixed order: bitwise reproducible.  -3: workspace missing / too small.
size_t conv_wgrad_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int ksize);
// 3x3 / stride-1 layers from spatial patches (conv_wgrad3.hip); launch_conv_wgrad routes to it and adds the slabs
bool conv_wgrad3_ok(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad, int lddz, int ldx);
size_t conv_wgrad3_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int launch_conv_wgrad3(const half_t* dz, long dz_bs, int lddz, const half_t* x, long x_bs, int ldx, int B, int H, int W, int Cin,
                       int Cout, float* dw, const half_t* zero, float* ws, size_t ws_bytes, int* splitk, hipStream_t s);
int launch_conv_wgrad(const half_t* dz, long dz_bstride, int lddz, const half_t* x, long x_bstride, int ldx, int B,
                      int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int ksize, int stride, int pad, float* dw,
                      const half_t* zero, float* ws, size_t ws_bytes, hipStream_t s);
// floats of workspace the train-mode batch-norm launches need for C channels (per-block partial sums + ticket)
size_t bn_workspace_floats(int C);
// gradient glue of the training step (train_kernels.hip): fixed-order column sums, nearest-2x upsample backward, input conversion
long colsum_workspace_floats(long nb, int cols);
int launch_colsum(const void* src, int src_f16, long nb, long bstride, long rows, int ld, int cols, float* ws, float* out, hipStream_t s);
// stride-2 input gradient with 32 forward input / 64 output channels as a wave-private chunk stream (conv_dgrad_s2c32.hip; a = the phase-2 form
// of the im2col kernel: x = dY, y = dX, w = the phase-form packed matrix)
bool dgrad_s2c32_ok(const ConvArgs& a);
int launch_dgrad_s2c32(const ConvArgs& a, hipStream_t s);
// YOLOv9c training glue (train_kernels.hip): RepConvN's SiLU(a + b) and ADown's pooling front, forward and backward
int launch_addsilu_fwd(const half_t* a, const half_t* b, half_t* v, half_t* y, long npix, int ldy, int C, hipStream_t s);
int launch_addsilu_bwd(const half_t* v, const half_t* dy, int lddy, half_t* g, long npix, int C, hipStream_t s);
int launch_adown_fwd(const half_t* x, long x_bs, int ldx, half_t* p1, long p1_bs, int ld1, half_t* p2, long p2_bs, int ld2, unsigned char* arg,
                     int B, int H, int W, int c, hipStream_t s);
int launch_adown_bwd(const half_t* g1, long g1_bs, int ld1, const half_t* g2, long g2_bs, int ld2, const unsigned char* arg, half_t* gx,
                     long gx_bs, int ldg, int B, int H, int W, int c, int accumulate, hipStream_t s);
int launch_upsample2x_bwd(const half_t* g, long g_bs, int ldg, half_t* d, long d_bs, int ldd, int B, int H, int W, int C, int accumulate,
                          hipStream_t s);
int launch_u8_to_f16x8(const unsigned char* src, half_t* dst, long npx, hipStream_t s);
// mask term of the segmentation loss + its gradients in one pass (loss_kernels.hip)
int launch_mask_loss(const float* coef, const void* protos, int protos_f16, const int* masks, const int* inst, const float* boxes,
                     const float* w, int B, int K, int mh, int mw, float* slot_sum, float* d_coef, void* d_protos, int d_protos_f16,
                     const float* gscale, hipStream_t s);
int launch_box_loss(const float* logits, const float* anchors, const float* targets, const float* weights, long n, float* box_term,
                    float* dfl_term, float* d_box, float* d_dfl, hipStream_t s);
int launch_dfl_decode(const float* raw, long rows, int A, int rw, int nc, const float* anchors, const float* strides, float* boxes,
                      float* scores, hipStream_t s);
// class term of the detection loss + its gradient in one pass (loss_kernels.hip); out: cls_bce_workspace_floats() floats
int launch_cls_bce(const float* raw, int rw, const float* targets, long rows, int nc, const float* scale, float* d_raw, float* out,
                   hipStream_t s);
size_t cls_bce_workspace_floats();
int launch_tal_assign(const float* scores, const float* boxes, const float* anchors_px, const int* gt_cls, const float* gt_boxes,
                      const unsigned char* gt_valid, int B, int A, int G, int nc, void* ws, float* t_boxes, float* t_scores,
                      unsigned char* fg, long* gt_idx, hipStream_t s);
int launch_repack(const void* d_jobs /* m355_repack_job[] (include/mi355yolo.h) */, const int* d_block_job, int nblocks, hipStream_t s);

// train-mode BatchNorm + SiLU (train_kernels.hip)
int launch_bn_silu_train_fwd(const half_t* z, long npix, int ldz, int C, const float* gamma, const float* beta,
                             float eps, half_t* y, int ldy, const half_t* res, int ldr, float* sums, float* mean_out,
                             float* invstd_out, int act, float* run_mean, float* run_var, float momentum, hipStream_t s);
int launch_adamw_step(float* p, const float* g, float* m, float* v, float* ema, const unsigned char* group, long n,
                      float lr, float lr_bias, float beta1, float beta2, float eps, float wd, int step, float grad_mul,
                      float ema_d, hipStream_t s);
int launch_sgd_step(float* p, const float* g, float* buf, float* ema, const unsigned char* group, long n, float lr,
                    float lr_bias, float momentum, int nesterov, float wd, float grad_mul, float ema_d, hipStream_t s);
int launch_grad_sumsq(const float* g, long n, float* out, hipStream_t s);   // out: grad_sumsq_workspace_floats() floats
size_t grad_sumsq_workspace_floats();
// LetterBox of n raw BGR images into the uint8 NHWC RGB input batch (letterbox.hip): src = the ragged device buffer of the
// sources, table = HOST array of n m355_letterbox_image (include/mi355yolo.h), out (n, net_h, net_w, 3).  Every argument is
// checked on the host first: -1 = refused (see m355_letterbox_u8), 0 = launched, else a HIP error code.
int launch_letterbox_u8(const uint8_t* src, const void* table, int n, int net_h, int net_w, uint8_t* out, hipStream_t s);
// mosaic + affine + HSV + flip gather (augment.hip); params: device array of B m355_aug_params
int launch_augment(const uint8_t* cache, const void* params, uint8_t* out, int B, int H, int W, hipStream_t s);
// the same gather with a homography, flipud, a paste list and a second layer (augment_ex.hip): params / polys / verts are HOST
// arrays (m355_aug_ex_params, m355_aug_poly, x,y float pairs), checked, copied into `work` on the stream and read from there.
// -1 = refused before any HIP call (see m355_augment_ex), 0 = launched, else a HIP error code.
size_t augment_ex_workspace_bytes(int B, int n_polys, int n_verts);
int launch_augment_ex(const uint8_t* cache, int n_images, const void* h_params, const void* h_polys, int n_polys,
                      const float* h_verts, int n_verts, void* work, long long work_bytes, uint8_t* out, int B, int H, int W,
                      hipStream_t s);
int launch_bn_silu_train_bwd(const half_t* z, const half_t* dy, long npix, int ldz, int lddy, int C, const float* mean,
                             const float* invstd, const float* gamma, const float* beta, float* rsum, half_t* dz,
                             int lddz, int act, float* ws, hipStream_t s);

}  // namespace m355
