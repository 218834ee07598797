/*
 * mi355yolo.h -- C-ABI of libmi355yolo.so: the MI355X (gfx950) native YOLOv8-seg hot path.
 *
 * The reference (CSMaus/DefectDetection_viaObjectDetection) has no FFI of its own: its hot path is the
 * Python call `YOLO(w).predict(src, save=True)` / `.train(...)` into the un-vendored `ultralytics`
 * package (BscanBased/yolo8_seg_predict.py:5-9, BscanBased/yolo_seg_train.py:7-19).  This header is the
 * boundary a maintainer binds instead (ctypes stub in INTEGRATION.md); each entry point names the
 * upstream stage it replaces (SURVEY.md section 8a row ids A3..A12).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ / torch types; no exceptions cross the boundary.
 *   - return 0 on success, negative m355_status on error; text via m355_last_error().
 *   - every device buffer is CALLER-OWNED (e.g. a PyTorch-ROCm tensor's data_ptr()); the library owns
 *     only the weights + workspace inside the engine handle.
 *   - every call is ASYNCHRONOUS on the caller's stream (`stream` is a hipStream_t passed as void*),
 *     no hidden synchronisation -- except the entry points marked [sync], which exist for unit parity.
 *   - one engine per device; an engine is not thread-safe; distinct engines are.
 *   - there is NO CPU fallback: without a gfx950 device m355_create fails with M355_ERR_NO_DEVICE.
 */
#ifndef MI355YOLO_H_
#define MI355YOLO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct m355_engine m355_engine;

typedef enum {
  M355_OK = 0,
  M355_ERR_INVALID = -1,    /* bad argument / shape */
  M355_ERR_NO_DEVICE = -2,  /* no gfx950 device visible */
  M355_ERR_HIP = -3,        /* HIP runtime error (text in last_error) */
  M355_ERR_STATE = -4,      /* weights not loaded, batch too large, ... */
  M355_ERR_NOMEM = -5
} m355_status;

/* Model description: replaces `YOLO("yolov8{n,s,m,l,x}-seg.yaml")` graph construction
 * (yolo_seg_train.py:7).  nc = number of classes (data-seg.yaml:4-5 -> 1).
 * scale selects the graph: 'n','s','m','l','x' = yolov8{scale}-seg; 'c' = yolov9c-seg; ('5' << 8) | 'n','s','m' = YOLOv5u
 * {n,s,m}; ('1' << 8) | 'n','s','m' = YOLO11{n,s,m}; ('8' << 8) | 'n','s','m','l','x' = YOLOv8{scale} detect (the yolov8-seg backbone
 * and neck under Detect at model.22).  The last three are detection graphs: box-only head, no prototypes or mask coefficients.
 * Any other high byte, or a scale letter its family does not build, is M355_ERR_INVALID (checked before the device is). */
typedef struct {
  int scale;      /* low byte: 'n','s','m','l','x','c'; high byte: 0 (segmentation families), '5' (YOLOv5u), '1' (YOLO11) or '8' (YOLOv8 detect) */
  int nc;         /* classes */
  int in_h, in_w; /* network input size, multiples of 32 (640x640 headline) */
  int max_batch;  /* workspace is sized for this many images */
} m355_model_desc;

/* One convolution of the graph, in canonical order (the order weights are supplied in). */
typedef struct {
  char name[64];   /* ultralytics state-dict prefix, e.g. "model.2.m.0.cv1" (conv+bn) or
                      "model.22.cv2.0.2" (plain conv2d with bias) or "model.22.proto.upsample" */
  int cin, cout;   /* logical channels */
  int k, stride;   /* kernel size (1,2,3; 6 for the YOLOv5u stem model.0), stride */
  int has_bn;      /* 1: Conv2d(bias=False)+BN+SiLU (fold BN before m355_set_conv_weights) */
  int transposed;  /* 1: ConvTranspose2d(k=2,s=2,bias) -- weight layout (cin,cout,2,2) */
  int act;         /* 1: SiLU epilogue (0: none -- the YOLO11 attention's qkv / proj / pe and ffn.1) */
  int groups;      /* Conv2d groups: 1, or cin for a depthwise conv (YOLO11 DWConv and attn.pe), whose weight layout for
                      m355_set_conv_weights is (cout, cin/groups, k, k) = (C, 1, 3, 3) */
} m355_conv_info;

/* Version / build info string (static storage). */
const char* m355_version(void);

/* Last error text for this engine (or the last global error when e == NULL). */
const char* m355_last_error(const m355_engine* e);

/* Build the layer plan + allocate weights/workspace on the current HIP device.           [sync] */
int m355_create(const m355_model_desc* desc, m355_engine** out);
void m355_destroy(m355_engine* e);

/* Graph introspection (lets the host map a state dict onto the engine). */
int m355_num_convs(const m355_engine* e);
int m355_get_conv_info(const m355_engine* e, int idx, m355_conv_info* out);
int m355_num_anchors(const m355_engine* e);           /* 8400 at 640x640 */
int m355_pred_width(const m355_engine* e);            /* 4 + nc + nm: nm = 32 (segmentation) or 0 (YOLOv5u detection) */
int m355_proto_hw(const m355_engine* e, int* h, int* w); /* 160x160 at 640; 0x0 for a detection engine */
size_t m355_workspace_bytes(const m355_engine* e);
double m355_flops_per_image(const m355_engine* e);    /* 2 * conv MACs */

/* Supply BN-folded fp32 weights of conv `idx` (host pointers, copied; caller keeps ownership):
 * w is (cout,cin,k,k) [or (cin,cout,2,2) when transposed], bias is (cout).  Replaces upstream
 * `fuse()` + `.to(device)`.                                                  [sync] */
int m355_set_conv_weights(m355_engine* e, int idx, const float* w, const float* bias);

/* Inference forward: d_in is uint8 NHWC (B,in_h,in_w,3) letterboxed pixels in
 * [0,255] (the /255 normalisation is folded into the stem conv).  Outputs:
 *   d_preds  float32 (B, A, 4+nc+nm): [cx,cy,w,h (pixels), class scores (sigmoid), nm mask coefs]
 *   d_protos float16 (B, H/4, W/4, 32) NHWC; a detection engine (nm = 0) writes none and takes d_protos = NULL
 * This is upstream's (B,4+nc+32,A) / (B,32,H/4,W/4) pair in anchor-major / NHWC order. */
int m355_forward(m355_engine* e, const void* d_in_u8_nhwc, int batch, float* d_preds, void* d_protos,
                 void* stream);

/* ---- measurement hooks (bench.py's live roofline figure) ----
 * One "op" = one kernel launch of the forward plan.  With profiling enabled m355_forward brackets every
 * launch with hipEventRecord on the caller's stream; m355_collect_op_times synchronises those events
 * and returns, per op, the accumulated milliseconds and number of launches since profiling was enabled. */
typedef struct {
  char kernel[48];        /* kernel family, e.g. "conv_igemm<128x128,k3>" */
  char layer[64];         /* first state-dict prefix the launch computes */
  double flops_per_image; /* algorithmic FLOPs (2*MACs), 0 for non-conv ops */
  double bytes_per_image; /* algorithmic activation bytes: inputs read once + outputs written once */
  double weight_bytes;    /* weight bytes, read once per launch */
} m355_op_info;
int m355_num_ops(const m355_engine* e);
int m355_get_op_info(const m355_engine* e, int idx, m355_op_info* out);
int m355_set_profiling(m355_engine* e, int enable);
int m355_collect_op_times(m355_engine* e, double* ms_sum, long* counts);                  /* [sync] */

/* Train-mode style raw head maps: float32 (B, A, 64+nc+nm) = [box DFL logits(64),
 * class logits(nc), mask coefs(nm)] before decode.  Valid after m355_forward on the same stream. */
int m355_get_raw_head(m355_engine* e, const float** d_raw, int* width);
/* Asynchronous device-to-device copy of the first `batch` images of the raw head maps into d_out. */
int m355_copy_raw_head(m355_engine* e, int batch, float* d_out, void* stream);
/* keep != 0 (the default of a new engine): the raw maps are written and the decode is its own launch.  keep == 0 (the
 * predict path): each head level's output convs and the decode of its rows run as one launch (csrc/head_tail.hip; same
 * arithmetic, bit-identical predictions), the raw maps are NOT written and m355_get_raw_head / m355_copy_raw_head fail with
 * M355_ERR_STATE.  (Models whose head does not fit that kernel -- nm != 32, nc > 32 -- always write the raw maps.) */
int m355_set_keep_raw(m355_engine* e, int keep);

/* Post-processing: batched NMS + mask assembly.
 *   d_dets   float32 (B, max_det, 6+nm)  rows [x1,y1,x2,y2,conf,cls,coefs] in letterboxed pixels,
 *            sorted by confidence descending
 *   d_counts int32 (B)
 *   d_masks  uint8 (B, max_det, in_h, in_w) binary masks (may be NULL to skip mask assembly; MUST be NULL for a detection
 *            engine, else M355_ERR_INVALID) */
int m355_postprocess(m355_engine* e, const float* d_preds, const void* d_protos, int batch, float conf,
                     float iou, int max_det, float* d_dets, int* d_counts, uint8_t* d_masks, void* stream);
/* m355_postprocess with upstream's agnostic / classes options of predict().
 *   agnostic      0: class-aware NMS (class offset cls * 7680, as m355_postprocess); 1: class-agnostic (offset 0)
 *   d_class_mask  NULL: every class.  Else a DEVICE bitmask of nc bits (bit c % 32 of word c / 32, ceil(nc / 32) words):
 *                 an anchor is a candidate only if its max score is above conf AND its argmax class is in the set (an
 *                 allowed class that is not the argmax is never picked instead; an empty set gives no detections).
 * d_dets / d_counts / d_masks as m355_postprocess (d_masks may be NULL).  agnostic = 0 with d_class_mask = NULL gives rows
 * and counts bit-identical to m355_postprocess.  M355_ERR_INVALID, before any HIP call: a NULL required pointer, batch
 * outside [1, max_batch], max_det outside [1, 1024], agnostic not 0 / 1, a class mask with nc > 1024, masks of a
 * detection engine or without d_protos. */
int m355_postprocess_ex(m355_engine* e, const float* d_preds, const void* d_protos, int batch, float conf, float iou,
                        int max_det, int agnostic, const uint32_t* d_class_mask, float* d_dets, int* d_counts,
                        uint8_t* d_masks, void* stream);

/* ---- Environment switches ----------------------------------------------------------------------------------------------------
 * The library is configured by m355_model_desc and the arguments of each call.  The M355_* environment variables below are
 * read-once A/B switches for measurements and tests; none is needed in production and none changes the ABI.  Unset = the default
 * described here.  Switches that change which kernels m355_forward launches (results stay within the parity tolerances; every
 * pair is A/B-tested in tests/test_c2f_fused_gpu.py / test_engine_gpu.py):
 *   M355_NO_PAIR        Bottleneck pairs as two launches instead of one bneck_pair launch (conv3x3_planes.hip)
 *   M355_NO_HEADDIAG    cv2.l.1 / cv3.l.1 / cv4.l.1 of the 40 x 40 and 20 x 20 head levels as three launches instead of one block-diagonal
 *                       row-slab launch (M355_HEADDIAG_L0=1: experiment, also the 80 x 80 level)
 *   M355_PAIR64=1       also use the pair launch for 64-channel bottlenecks (measured no gain: off)
 *   M355_NO_PLANES      the 20 x 20 level on conv3x3_slab instead of the row-slab kernel
 *   M355_NO_C2F32       model.2 as three launches instead of c2f_c32
 *   M355_NO_W1_SPLIT    model.15.cv1 (Upsample + Concat read through) on the im2col kernel instead of conv1x1_wreg's split form
 *   M355_NO_PLANES_S2, M355_NO_PLANES_M64   the stride-2 3x3 convs / the 64 -> 64 conv of the 40 x 40 head level off the row-slab kernel
 *   M355_NO_DGRAD_PHASES  (training) stride-2 input gradients as the masked nine-tap gather instead of four phase convs
 *   M355_NO_WGRAD_STEM    (training) layer 0's weight gradient on the pixel-axis GEMM instead of wgrad_stem_kernel
 *   M355_NO_WGRAD_S2C32, M355_NO_DGRAD_S2C32   (training) model.1's weight / input gradient on the pixel-axis GEMM / the im2col kernel
 *   M355_NO_W1, M355_NO_S2C64, M355_NO_S2C32, M355_NO_PROTOR, M355_NO_PROTOFUSE(3), M355_NO_HEADTAIL, M355_NO_STEMFUSE,
 *   M355_NO_STEM2, M355_NO_CVFUSE, M355_NO_UPFUSE, M355_NO_C32, M355_NO_M32, M355_NO_WIDE, M355_NO_HALO, M355_NO_SLAB,
 *   M355_DECFUSE=1      each falls back from one fused / specialised kernel to the kernels it replaced (names = file names in csrc/)
 *   M355_NO_LANES, M355_LANE_PLAN, M355_SUBBATCH(_OPS), M355_NO_SUBBATCH   stream lanes / sub-batches inside a forward
 * Tuning knobs of single kernels (tile queues, slot counts, priorities): M355_PERSIST, M355_NO_PERSIST, M355_STATIC_TILES,
 *   M355_M32_SLOTS, M355_C32_SLOTS, M355_C32_WASTE, M355_WIDE_SLOTS, M355_WIDE_STAGGER, M355_HALO_VARIANT, M355_K1_TILE, M355_SMALLM,
 *   M355_S2C32_RING, M355_S2C64_PRIO, M355_PROTOR_PRIO, M355_C2F_NOPRIO, M355_STEM2_NXB, M355_NO_FAST_EPI, M355_NO_BIAS_LDS,
 *   M355_STEM_GATHER, M355_MASK_TILE, M355_WGRAD_BLOCKS, M355_WGRAD3_{BLOCKS,MINTILES,SHRINK,SLABMB}, M355_NO_WGRAD3,
 *   M355_NO_TRAIN_W1, M355_NO_TRAIN_C32.
 * Diagnostics (write files / print timings, never set in production): M355_STAMPS, M355_*_STAMPS, M355_*_DBG, M355_BNECK_REPS;
 * testing only: M355_HEADTAIL_MAXM (forces head levels off the head_tail launch).
 * Python side (train_engine.py, bench.py): M355_NO_WGRAD_STREAM, M355_NO_HEAD_STREAM, M355_SIDE_STREAMS, M355_NO_LOSS_KERNELS,
 * M355_DIST_BACKEND, M355_DIST_SAME_DEVICE. */

/* ---- per-op entry points for unit parity (all device pointers, asynchronous unless noted) ---- */

/* NHWC fp16 convolution + bias (+SiLU) (+residual) via the implicit-GEMM MFMA kernel.
 * h_w fp32 (cout,cin,k,k) and h_bias fp32 (cout) are HOST pointers, packed + uploaded here.  [sync] */
int m355_conv2d_fwd(const void* d_x_f16_nhwc, int B, int H, int W, int cin, const float* h_w,
                    const float* h_bias, int cout, int k, int stride, int act,
                    const void* d_res_f16_nhwc, void* d_y_f16_nhwc, int out_f32, int force_tile,
                    void* stream);
/* A whole C2f block body with 32 hidden channels in ONE launch (csrc/c2f_c32.hip; upstream nn.modules.block.C2f with
 * n = 1 after its cv1):  t = SiLU(conv3x3(y1; wa) + ba);  y2 = SiLU(conv3x3(t; wb) + bb) (+ y1 if shortcut);
 * out = SiLU(conv1x1([y0, y1, y2]; wc) + bc).  d_x fp16 NHWC (B,H,W,64) = [y0, y1]; d_y fp16 NHWC (B,H,W,64);
 * h_wa / h_wb fp32 (32,32,3,3), h_wc fp32 (64,96,1,1), biases fp32: HOST pointers (BN folded), packed + uploaded
 * here.  H % 8 == 0 and W % 16 == 0.  [sync] */
int m355_c2f_c32_fwd(const void* d_x_f16_nhwc, int B, int H, int W, const float* h_wa, const float* h_ba,
                     const float* h_wb, const float* h_bb, const float* h_wc, const float* h_bc, int shortcut,
                     void* d_y_f16_nhwc, void* stream);
/* A whole C2f Bottleneck (upstream nn.modules.block.Bottleneck with e = 1.0: cv1 3x3 -> cv2 3x3, optional shortcut)
 * in ONE launch (csrc/conv3x3_planes.hip): t = SiLU(conv3x3(x; wa) + ba) stays in LDS (rounded to fp16 exactly where the
 * two-launch form stores it), y = SiLU(conv3x3(t; wb) + bb) (+ x if shortcut).  d_x fp16 NHWC (B,H,W,ldx) of which the first C
 * channels are x; d_y fp16 NHWC (B,H,W,ldy), first C channels written; C in {64, 128}; h_wa / h_wb fp32 (C,C,3,3) and
 * biases fp32 (C): HOST pointers (BN folded), packed + uploaded here.  Shapes whose row slabs do not fit LDS are refused
 * (M355_ERR_INVALID).  [sync] */
int m355_bneck_pair_fwd(const void* d_x_f16_nhwc, int B, int H, int W, int C, int ldx, const float* h_wa, const float* h_ba,
                        const float* h_wb, const float* h_bb, int shortcut, void* d_y_f16_nhwc, int ldy, void* stream);
/* n <= 4 3x3 Conv+BN+SiLU layers (BN folded) that sit side by side in one tensor -- conv i reads the next cin[i] channels of d_x and
 * writes the next cout[i] channels of d_y: a block-diagonal convolution, upstream's cv2.l.1 / cv3.l.1 / cv4.l.1 of a Segment head
 * level -- in ONE launch of the row-slab kernel (csrc/conv3x3_planes.hip, block-diagonal single mode): every 64-channel tile runs
 * its K loop over the input planes of its own conv only, in the order of that conv's own launch.  d_x fp16 NHWC (B,H,W,ldx), d_y fp16
 * NHWC (B,H,W,ldy); cin[i] % 32 == 0, cout[i] % 16 == 0, every cout but the last a multiple of 64, at most eight 64-channel tiles;
 * h_w[i] fp32 (cout[i],cin[i],3,3) and h_b[i] fp32 (cout[i]): HOST pointers, packed + uploaded here.  walk: 0 = the launcher chooses how
 * a block walks the tiles (as inside m355_forward), 1 = single 64-channel tiles, 2 = every tile of a row slab (tests).  [sync]
 * m355_planes_diag_pack is its weight packing alone, on the host (no device needed): the fp16 MFMA fragments [conv][32-channel block,
 * padded to a multiple of two][input plane of that conv][tap][K slice], 1 KiB each -- element (lane, j) of a fragment = row
 * 32 cb + 16 ((lane >> 2) & 1) + 4 ((lane & 31) >> 3) + (lane & 3), K = tap * cin + 32 p + 16 s + 8 (lane >> 5) + j.  Returns the byte
 * size of the list (h_out_f16 = NULL: the size only), or an error code < 0. */
int m355_conv3x3_blockdiag_fwd(const void* d_x_f16_nhwc, int B, int H, int W, int ldx, int n, const int* cin, const int* cout,
                               const float* const* h_w, const float* const* h_b, void* d_y_f16_nhwc, int ldy, int walk, void* stream);
long m355_planes_diag_pack(int n, const int* cin, const int* cout, const float* const* h_w, void* h_out_f16, long out_bytes);
/* Per-op parity entries of the fused launches (round 3 kernels; host weights fp32 with BN folded, packed + uploaded here exactly as
 * m355_set_conv_weights packs them; a shape the kernel does not take is refused with M355_ERR_INVALID).  [sync]
 *   m355_s2c64_cv1_fwd       csrc/conv3x3_s2c64.hip: Conv3x3/s2 (64 -> 128) + SiLU -> fp16 -> Conv1x1 (128 -> 128) + SiLU; upstream
 *                            model.3 + model.4.cv1 of yolov8s.  d_x (B,H,W,64) -> d_y (B,H/2,W/2,128); H/2 and W/2 multiples of 8.
 *   m355_stem_s2c32_cv1_fwd  csrc/conv_stem_c2.hip (two_team = 1) / conv_stem_s2c32.hip (0): uint8 image -> Conv3x3/s2 (3 -> 32, the
 *                            1/255 input scale inside) -> Conv3x3/s2 (32 -> 64) -> Conv1x1 (64 -> 64), SiLU + fp16 after each; upstream
 *                            model.0 + model.1 + model.2.cv1.  d_in (B,H,W,3) uint8 -> d_y (B,H/4,W/4,64); H/4 % 8 == 0, W/4 % 16 == 0.
 *   m355_proto_phase_fwd     csrc/proto_phase_wreg.hip: Proto.upsample (ConvTranspose2d 2x2/s2, bias; weight (cin,cout,2,2)) -> Proto.cv2
 *                            (3x3 + SiLU) -> Proto.cv3 (1x1, 128 -> 32, + SiLU) composed into four 2x2 phase convs.  d_x (B,H,W,128) ->
 *                            d_y (B,2H,2W,32); H % 8 == 0, W % 16 == 0.
 *   m355_head_tail_fwd       csrc/head_tail.hip: the three output convs of one Detect / Segment level (cv2.l.2 64 -> 64 box bins,
 *                            cv3.l.2 128 -> nc, cv4.l.2 32 -> 32, with bias) + DFL + dist2bbox + sigmoid: d_x (B,H,W,224) = [box 64 |
 *                            class 128 | coefficient 32] branch tensor -> rows [level_off, level_off + H W) of d_preds (B,A,4+nc+32) fp32. */
int m355_s2c64_cv1_fwd(const void* d_x_f16_nhwc, int B, int H, int W, const float* h_w3, const float* h_b3, const float* h_w1,
                       const float* h_b1, void* d_y_f16_nhwc, void* stream);
int m355_stem_s2c32_cv1_fwd(const void* d_in_u8_nhwc, int B, int H, int W, const float* h_w0, const float* h_b0, const float* h_w1,
                            const float* h_b1, const float* h_w2, const float* h_b2, void* d_y_f16_nhwc, int two_team, void* stream);
int m355_proto_phase_fwd(const void* d_x_f16_nhwc, int B, int H, int W, const float* h_wt, const float* h_bt, const float* h_w3,
                         const float* h_b3, const float* h_wc, const float* h_bc, void* d_y_f16_nhwc, void* stream);
int m355_head_tail_fwd(const void* d_x_f16_nhwc, int B, int H, int W, int nc, float stride, const float* h_w2, const float* h_b2,
                       const float* h_w3, const float* h_b3, const float* h_w4, const float* h_b4, float* d_preds, int A, int level_off,
                       void* stream);
/* Data gradient of Conv2d(k in {1,3}, stride in {1,2}, pad k/2, no bias) (SURVEY A13 backward): dY fp16 NHWC
 * (B,Ho,Wo,cout) -> dX fp16 NHWC (B,H,W,cin).  Runs on the same implicit-GEMM kernel: stride 1 = convolution
 * with the spatially flipped, channel-transposed weights; stride 2 = four 2x2 phase convs over dY on even maps where
 * tmode 2 of m355_conv_launch takes the channels (cin % 64 == 0, or 128 % cin == 0 with cin >= 16; compact taps when cin and
 * cout are both multiples of 64), the masked transposed-stride gather otherwise (or with M355_NO_DGRAD_PHASES=1).  cin and
 * cout any multiples of 8.  h_w is the FORWARD weight fp32 (cout,cin,k,k) on the host.              [sync] */
int m355_conv2d_dgrad(const void* d_dy_f16_nhwc, int B, int H, int W, int cin, const float* h_w, int cout, int k,
                      int stride, void* d_dx_f16_nhwc, void* stream);
/* Weight gradient of Conv2d(k in {1,3}, stride in {1,2}, pad k/2) (SURVEY A13 backward): X fp16 NHWC (B,H,W,cin),
 * dY fp16 NHWC (B,Ho,Wo,cout) -> dW fp32 DEVICE buffer in KRSC order (cout, k, k, cin) = the packed forward
 * weight order.  Deterministic: split-K partial slabs in a workspace the call allocates, added in a fixed order. [sync] */
int m355_conv2d_wgrad(const void* d_x_f16_nhwc, const void* d_dy_f16_nhwc, int B, int H, int W, int cin, int cout,
                      int k, int stride, float* d_dw_krsc, void* stream);
/* Train-mode BatchNorm2d (batch statistics, biased variance, eps) + optional SiLU on fp16 NHWC (B,H,W,C)
 * (SURVEY A13): y = act(gamma * (z - mean) * invstd + beta).  gamma/beta/mean/invstd/ws are DEVICE fp32 arrays;
 * d_ws is a workspace of m355_bn_workspace_floats(C) floats (per-block partial rows; a second small kernel combines them in
 * block order: no float atomics, bitwise reproducible); d_mean/d_invstd receive the saved statistics.  The forward carries
 * its statistics as (count, mean, sum of squared deviations) per thread, block and batch and merges those, so the variance
 * does not cancel for channels with |mean| >> std; the backward's rows are plain sums.  The workspace need not be zeroed. */
size_t m355_bn_workspace_floats(int C);
int m355_bn_silu_train_fwd(const void* d_z, int B, int H, int W, int C, const float* d_gamma, const float* d_beta,
                           float eps, int act, void* d_y, float* d_mean, float* d_invstd, float* d_ws, void* stream);
/* Backward of the above: dz (fp16 NHWC) and d_dbeta_dgamma (device float[2*C]: [0:C] = dbeta, [C:2C] = dgamma). */
int m355_bn_silu_train_bwd(const void* d_z, const void* d_dy, int B, int H, int W, int C, const float* d_mean,
                           const float* d_invstd, const float* d_gamma, const float* d_beta, int act, void* d_dz,
                           float* d_dbeta_dgamma, float* d_ws, void* stream);
/* ConvTranspose2d(k=2,s=2)+bias; h_w fp32 (cin,cout,2,2).                                   [sync] */
int m355_convt2x2_fwd(const void* d_x_f16_nhwc, int B, int H, int W, int cin, const float* h_w,
                      const float* h_bias, int cout, void* d_y_f16_nhwc, void* stream);
/* Stem conv: uint8 NHWC (B,H,W,3) -> fp16 NHWC (B,H/2,W/2,cout), 3x3 s2 p1 + bias + SiLU;
 * h_w fp32 (cout,3,3,3) is applied to pixel/255.  cout in {16,32,48,64,80}; B >= 1; H and W even, >= 2 and at most 32768 (an odd size
 * is not the convolution's output); the image 16-byte and the output 8-byte aligned.  Every argument is checked before any HIP
 * call (-1 = M355_ERR_INVALID).                                                                               [sync] */
int m355_stem_fwd(const void* d_in_u8, int B, int H, int W, const float* h_w, const float* h_bias, int cout,
                  void* d_y_f16_nhwc, void* stream);
/* YOLOv5u stem (model.0, conv_stem6_s2.hip): uint8 NHWC (B,H,W,3) -> fp16 NHWC (B,H/2,W/2,C0),
 * Conv 6x6 / s2 / p2 + bias + SiLU; h_w fp32 (C0,3,6,6), BN folded, is applied to pixel/255.  C0 in {16,32,48}; H even and
 * positive, W a positive multiple of 16.  Every argument is checked before any HIP call (-1 = M355_ERR_INVALID).   [sync] */
int m355_stem6_fwd(const void* d_x_u8_nhwc, int B, int H, int W, const float* h_w, const float* h_bias, int C0,
                   void* d_y_f16_nhwc, void* stream);
/* YOLO11 depthwise 3x3 / s1 / p1 conv (dwconv3x3.hip) on fp16 NHWC channel slices: x (B,H,W,ldx) -> y (B,H,W,ldy), channels
 * [0, C) of each (the pointers are the slices' first channels), y = act(dwconv(x; w) + b); h_w fp32 (C,1,3,3) BN folded, h_b
 * (C), act 0 or 1 (SiLU).  C a positive multiple of 8; ldx, ldy multiples of 8 and >= C; x and y 16-byte aligned; B, H, W
 * >= 1.  Every argument is checked before any HIP call (-1 = M355_ERR_INVALID).                                  [sync] */
int m355_dwconv3x3_fwd(const void* d_x_f16_nhwc, int B, int H, int W, int C, int ldx, const float* h_w, const float* h_b,
                       int act, void* d_y_f16_nhwc, int ldy, void* stream);
/* YOLO11 C2PSA attention core (psa_attn.hip): qkv fp16 NHWC (B,H,W,heads*128), head h's channels [q 32 | k 32 | v 64] at
 * 128 h -> y fp16 NHWC (B,H,W,heads*64): y[., 64 h + c] = sum_j v[c,j] softmax_j(q_i . k_j / sqrt(32)) + pe(v), pe = the
 * depthwise 3x3 conv h_pe_w fp32 (heads*64,1,3,3) + h_pe_b (BN folded, no activation) over v as (B, heads*64, H, W).
 * key_dim must be 32 and head_dim 64 (else M355_ERR_INVALID); heads 1..64, B 1..65535, H, W >= 1, H*W <= 2^24; qkv
 * 16-byte and y 8-byte aligned.  Every argument is checked before any HIP call.                              [sync] */
int m355_psa_attn_fwd(const void* d_qkv_f16_nhwc, int B, int H, int W, int heads, int key_dim, int head_dim,
                      const float* h_pe_w, const float* h_pe_b, void* d_y_f16_nhwc, void* stream);
/* SPPF pooling: x fp16 NHWC (B,H,W,C) -> y (B,H,W,3C) = [mp5(x), mp5(mp5(x)), mp5^3(x)].  The dense form of
 * m355_sppf_pool_launch (below), with its argument checks.  Asynchronous on `stream`. */
int m355_sppf_pool(const void* d_x, int B, int H, int W, int C, void* d_y, void* stream);
/* Nearest 2x upsample, fp16 NHWC (B,H,W,C) -> (B,2H,2W,C).  The dense form of m355_upsample2x_launch (below), with its
 * argument checks.  Asynchronous on `stream`. */
int m355_upsample2x(const void* d_x, int B, int H, int W, int C, void* d_y, void* stream);
/* Head decode: raw (B,A,64+nc+nm) f32 -> preds (B,A,4+nc+nm) f32 for an in_h x in_w input, A = the anchors of
 * the three levels (strides 8, 16, 32; anchor (gx + 0.5, gy + 0.5) per cell, row-major per level): cxcywh in pixels from the
 * DFL expectation over 16 bins, sigmoid class scores, the nm coefficients copied through.  m355_head_decode is the _ex
 * entry with nm = 32.  M355_ERR_INVALID, before any HIP call: a NULL pointer, B < 1, in_h or in_w not a positive multiple
 * of 32, nc < 1, nm < 0, an nc + nm whose 64-anchor stage needs more than 160 KB of LDS, raw or preds not 16-byte aligned.
 * Asynchronous on `stream`. */
int m355_head_decode(const float* d_raw, int B, int in_h, int in_w, int nc, float* d_preds, void* stream);
int m355_head_decode_ex(const float* d_raw, int B, int in_h, int in_w, int nc, int nm, float* d_preds, void* stream);
/* Batched NMS only. preds (B,A,4+nc+nm).  An anchor is a candidate when its best class score is above conf
 * (strictly); of an image's candidates only the first 30000 by score (equal scores: the lower anchor first) enter the greedy
 * pass, as upstream's max_nms: with A <= 30000 that is all of them.  A box is suppressed by a kept one when their IoU is
 * above iou (strictly); at most max_det (1..1024) rows per image.                                                 [sync] */
int m355_nms(const float* d_preds, int B, int A, int nc, int nm, float conf, float iou, int max_det,
             float* d_dets, int* d_counts, void* stream);
/* m355_nms with the agnostic / class-set options of m355_postprocess_ex (same meaning).  M355_ERR_INVALID, before any HIP
 * call: a NULL pointer, B, A or nc < 1, nm < 0, max_det outside [1, 1024], agnostic not 0 / 1, a class mask with
 * nc > 1024.                                                                                                         [sync] */
int m355_nms_ex(const float* d_preds, int B, int A, int nc, int nm, float conf, float iou, int max_det, int agnostic,
                const uint32_t* d_class_mask, float* d_dets, int* d_counts, void* stream);
/* Native-resolution masks (upstream process_mask_native, predict(retina_masks=True)), one launch per
 * 32 images.  d_dets (B,max_det,38) and d_counts (B) as m355_nms writes them; d_protos fp16 (B,mh,mw,32), 16-byte aligned;
 * h_orig_hw HOST int32 (B,2) original (h0, w0) per image; d_boxes f32 (B,max_det,4) x1,y1,x2,y2 in original pixels (the
 * boxes the caller reports); h_offsets HOST int64 (B+1), non-decreasing from >= 0: image b's masks are the bytes
 * [h_offsets[b], h_offsets[b+1]) of d_out, one uint8 {0,1} plane (h0,w0) per detection slot, so that span must hold a whole
 * number of planes, at most max_det.  Slots at or past counts[b] are written as zeros; d_out must hold h_offsets[B] bytes
 * (it may be NULL when h_offsets[B] == 0).  The prototype grid is cropped to the letterboxed image, the fp32 logits
 * interpolated bilinearly (align_corners = false) to (h0, w0), zeroed outside the box (x1 <= col < x2, y1 <= row < y2)
 * and thresholded at > 0.  M355_ERR_INVALID, before any HIP call: a NULL required pointer, B < 1, max_det outside
 * [1, 1024], mh or mw outside [1, 512], h0 or w0 outside [1, 32768], a crop of no cells, a bad offset table. */
int m355_proto_masks_native(const float* d_dets, const int* d_counts, const void* d_protos, int B, int max_det, int mh,
                            int mw, const int32_t* h_orig_hw, const float* d_boxes, const int64_t* h_offsets,
                            uint8_t* d_out, void* stream);
/* LetterBox on the device: n raw decoded images, uint8 BGR (h,w,3), packed one after the
 * other in the device buffer d_src, become the engine's input batch d_out uint8 (n,net_h,net_w,3) RGB: image i resized to
 * (uh,uw) lies at rows [top, top+uh), columns [left, left+uw) of its frame, every other byte is 114.  The resize is the
 * bilinear one of preprocess.resize_linear_u8 (half-pixel centres, clamped taps, round half up), evaluated in the same
 * IEEE double operations, so the bytes equal the host letterbox's; (h,w) == (uh,uw) is a copy.  h_table is a HOST array.
 * Asynchronous on `stream`, one launch per 32 images.  M355_ERR_INVALID, before any HIP call: a NULL pointer, n < 1,
 * net_h or net_w not a positive multiple of 32 (or above 32768), d_out not 16-byte aligned, h, w, uh or uw < 1, h or w
 * above 32768, a window that leaves the frame, an offset below the end of the previous image (negative, overlapping or
 * misordered). */
typedef struct {
  int64_t offset;            /* byte offset of the image's first pixel in d_src; the image occupies 3*h*w bytes */
  int32_t h, w;              /* source size */
  int32_t uh, uw;            /* size after the resize */
  int32_t top, left;         /* position of the resized image in the frame */
} m355_letterbox_image;
int m355_letterbox_u8(const uint8_t* d_src, const m355_letterbox_image* h_table, int n, int net_h, int net_w,
                      uint8_t* d_out, void* stream);
/* Mask assembly only: dets (B,max_det,6+32), counts (B), protos fp16 (B,mh,mw,32)
 * -> masks uint8 (B,max_det,in_h,in_w). */
int m355_proto_masks(const float* d_dets, const int* d_counts, const void* d_protos, int B, int max_det,
                     int mh, int mw, int in_h, int in_w, uint8_t* d_masks, void* stream);

/* ---- raw strided launches (asynchronous; every pointer is a DEVICE pointer) --------------------------------
 * Used by the training orchestrator (defectdetection_viaobjectdetection_amd/train_engine.py) to run the kernels
 * on channel slices of shared NHWC buffers.  Strides are in ELEMENTS of the tensor's dtype. */
typedef struct {
  const void* x; int64_t x_bstride; int32_t ldx; int32_t hi, wi, cin;   /* input slice (fp16 NHWC) */
  const void* w_packed; int32_t kpad;   /* fp16 [ceil128(cout)][kpad], K = (kh*k+kw)*cin + ci, kpad % 64 == 0 */
  const float* bias;                    /* fp32 [ceil128(cout)] */
  void* y; int64_t y_bstride; int32_t ldy; int32_t ho, wo, cout;          /* output slice (fp16, or fp32 if out_f32) */
  const void* res; int64_t r_bstride; int32_t ldr;                        /* optional residual added after act */
  int32_t ksize, stride, pad, batch;
  int32_t act, out_f32, convt_co, tmode;
  const void* zero_page;                /* >= 16 zero bytes */
} m355_conv_args;
/* Convolution / dgrad / ConvTranspose forward on the implicit-GEMM or halo kernel (chosen by shape).
 * ConvTranspose forward (tmode 0, ksize 1, convt_co > 0): cout = 4 * convt_co virtual channels (dy, dx, co), w_packed rows in that
 *          order, y = the (2 hi) x (2 wi) output slice of convt_co channels, bias [co]; no res (M355_ERR_INVALID).
 * tmode 1: input gradient of a 3x3 / stride-2 / pad-1 conv by a transposed-stride gather (x = dY, y = dX, all nine taps masked per
 *          output parity; any size).
 * tmode 2: the same gradient as FOUR 2x2 phase convs over dY (one per parity class of the dX pixel): ksize = 2, stride = 1, pad = 0,
 *          hi x wi = ho x wo = the dY map, cout = 4 * convt_co virtual channels (phase-major), convt_co = the forward input channels,
 *          y = the (2 ho) x (2 wo) dX slice, w_packed = [4 * convt_co][(ty, tx, forward cout)] with zero rows for the taps a phase does
 *          not have (16 tap slots for 9 taps; tmode 1 multiplies 36).  Needs convt_co % 64 == 0, or 128 % convt_co == 0 with
 *          convt_co >= 16 and no res; M355_ERR_INVALID otherwise (tmode 1 takes any such shape).  With convt_co % 64 == 0 AND
 *          cin % 64 == 0 (cin = the forward cout) the K axis of a phase is COMPACT -- tap (ty, tx) of phase (a, b) at slot
 *          ty * (1 + b) + tx, zeros behind -- and the phase's K loop ends after its (1 + a)(1 + b) taps: 9 tap slots in all.
 *          Otherwise slot = ty * 2 + tx. */
int m355_conv_launch(const m355_conv_args* a, void* stream);

typedef struct {
  const void* dz; int64_t dz_bstride; int32_t lddz;   /* dY slice (fp16 NHWC), spatial ho x wo, cout channels */
  const void* x; int64_t x_bstride; int32_t ldx;      /* forward input slice, spatial hi x wi, cin channels */
  int32_t hi, wi, cin, ho, wo, cout;
  int32_t ksize, stride, pad, batch;
  float* dw;                                          /* fp32 [cout][ksize*ksize*cin] (KRSC), overwritten */
  const void* zero_page;
  float* ws; int64_t ws_bytes;                        /* >= m355_wgrad_workspace_bytes(...): split-K partial slabs */
} m355_wgrad_args;
/* Deterministic (no float atomics): every K split stores its partial tile to its slab of `ws`, a second kernel adds the
 * slabs in a fixed order.  M355_ERR_INVALID when ws is missing / too small for the shape. */
size_t m355_wgrad_workspace_bytes(int32_t batch, int32_t ho, int32_t wo, int32_t cin, int32_t cout, int32_t ksize);
int m355_wgrad_launch(const m355_wgrad_args* a, void* stream);

/* Train-mode BN(+SiLU)(+residual) on slices: y = act(bn(z)) + res.  running_mean / running_var (may be NULL) get the
 * momentum update r = (1 - momentum) * r + momentum * batch_stat (unbiased variance), like torch BatchNorm2d. */
int m355_bn_train_fwd_launch(const void* z, int64_t npix, int32_t ldz, int32_t C, const float* gamma, const float* beta,
                             float eps, int32_t act, void* y, int32_t ldy, const void* res, int32_t ldr, float* mean,
                             float* invstd, float* ws, float* running_mean, float* running_var, float momentum,
                             void* stream);
int m355_bn_train_bwd_launch(const void* z, const void* dy, int64_t npix, int32_t ldz, int32_t lddy, int32_t C,
                             const float* mean, const float* invstd, const float* gamma, const float* beta, int32_t act,
                             void* dz, int32_t lddz, float* dbeta_dgamma, float* ws, void* stream);
/* Forward glue on channel slices (csrc/misc_kernels.hip): SPPF pooling x (B,H,W,[C]) -> y (B,H,W,[3C]) = [mp5(x), mp5^2(x),
 * mp5^3(x)] (5x5 / s1 / p2 max pools, clipped windows), and (further down) m355_upsample2x_launch and m355_adown_pool_launch.
 * Every argument is checked before any HIP call (M355_ERR_INVALID, the message names the entry): B, H, W >= 1; C a
 * positive multiple of 8; for every slice a non-NULL 16-byte aligned pointer, a leading dimension >= its channel count,
 * leading dimension and batch stride multiples of 8, a batch stride >= the extent (pixels - 1) * ld + channels of one
 * image's slice.  SPPF keeps a whole plane in LDS: one of more than 160 KB (H * W > 3413) is refused.
 * m355_sppf_pool_form (host only, no HIP call) names the kernel instance m355_sppf_pool_launch runs for a shape:
 * cg | (owned << 8), cg = 8-channel groups per block (1, 2, 4), owned = 1 the per-thread-ownership kernel (planes of at
 * most 2048 elements), 0 the generic one; -1 where the launch refuses.  The choice depends on M355_SPPF_MINBLOCKS. */
int m355_sppf_pool_launch(const void* x, int64_t x_bstride, int32_t ldx, void* y, int64_t y_bstride, int32_t ldy,
                          int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
int m355_sppf_pool_form(int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldy);
/* Re-pack of fp32 master weights into fp16 GEMM layouts, every strided convert-copy of a training step in one launch.
 * A job copies a 4-d iteration space n[0..3] (n[3] fastest) from fp32 `src` to fp16 `dst` with signed ELEMENT strides on both
 * sides; block0 = index of the job's first block; block b of the launch handles elements [(b - block0) * 1024, +1024) of job
 * block_job[b].  Jobs and block_job live in DEVICE memory (built once: the pointers of a training engine never move). */
typedef struct m355_repack_job {
  const void* src;
  void* dst;
  int32_t n[4];
  int64_t ss[4];
  int64_t ds[4];
  int32_t block0;
  int32_t pad_;
} m355_repack_job;
int m355_repack_launch(const m355_repack_job* d_jobs, const int32_t* d_block_job, int32_t nblocks, void* stream);
/* Backward of the SPPF pooling chain (autograd of three F.max_pool2d(5, 1, 2) upstream): a = the pooled input slice, y = the
 * forward concat slice [y1 | y2 | y3] (3C channels), gy = its gradient, ga = d(loss)/da stored (accumulate = 0) or added to
 * what ga holds (fp16).  Gather formulation, no atomics: bitwise reproducible.  H * W * 96 bytes of LDS (<= 160 KB). */
int m355_sppf_pool_bwd_launch(const void* a, int64_t a_bstride, int32_t lda, const void* y, int64_t y_bstride, int32_t ldy,
                              const void* gy, int64_t gy_bstride, int32_t ldgy, void* ga, int64_t ga_bstride, int32_t ldga,
                              int32_t B, int32_t H, int32_t W, int32_t C, int32_t accumulate, void* stream);
/* Task-aligned assignment of the training loss (csrc/loss_kernels.hip; upstream TaskAlignedAssigner: top-10 by score^0.5 * CIoU^6 among the
 * anchors whose centre lies strictly inside the box, multiply-claimed anchors to the truth of highest CIoU, normalised alignment as
 * target score).  All pointers device: scores (B,A,nc) f32, boxes (B,A,4) xyxy px, anchors_px (A,2), gt_cls (B,G) int32, gt_boxes (B,G,4),
 * gt_valid (B,G) uint8; ws = 12 * B * G * 10 bytes of scratch; t_boxes (B,A,4), t_scores (B,A,nc), fg (B,A) uint8, gt_idx (B,A) int64 must
 * be ZERO on entry (only the positives are written).  Asynchronous on `stream`. */
int m355_tal_assign_launch(const float* scores, const float* boxes, const float* anchors_px, const int32_t* gt_cls, const float* gt_boxes,
                           const uint8_t* gt_valid, int32_t B, int32_t A, int32_t G, int32_t nc, void* ws, float* t_boxes, float* t_scores,
                           uint8_t* fg, int64_t* gt_idx, void* stream);
/* YOLOv9c training glue (csrc/train_kernels.hip; the graph /root/reference/BscanBased/yolo_seg_train.py:7 names), fp16 NHWC, asynchronous:
 *  addsilu: RepConvN's tail  y = SiLU(a + b)  of its two activation-free Conv + BN branches (upstream RepConvN.forward).  a, b, v, g are
 *    dense (npix, C) rows; v = fp16(a + b) is kept for the backward; y / dy are slices with row strides ldy / lddy.  Backward:
 *    g = dy * SiLU'(v), the gradient of BOTH branches (one buffer).
 *  adown: ADown's pooling front (upstream ADown.forward): t = avg_pool2d(x, 2, 1, 0); p1 = t[:, :c] (B,H-1,W-1,c);
 *    p2 = max_pool2d(t[:, c:], 3, 2, 1) (B,Ho,Wo,c), Ho = (H-2)/2+1; argmax (B,Ho,Wo,c) uint8 = window position 3*ky+kx of the first
 *    maximum in row-major order (torch's rule), written by the forward and read by the backward, which GATHERS: gx (B,H,W,2c) from the
 *    gradients g1 of p1 and g2 of p2 in a fixed order (no atomics); accumulate = 1 adds fp16(result) to what gx holds. */
int m355_addsilu_fwd_launch(const void* a, const void* b, void* v, void* y, int64_t npix, int32_t ldy, int32_t C, void* stream);
int m355_addsilu_bwd_launch(const void* v, const void* dy, int32_t lddy, void* g, int64_t npix, int32_t C, void* stream);
int m355_adown_fwd_launch(const void* x, int64_t x_bstride, int32_t ldx, void* p1, int64_t p1_bstride, int32_t ld1, void* p2,
                          int64_t p2_bstride, int32_t ld2, uint8_t* argmax, int32_t B, int32_t H, int32_t W, int32_t c, void* stream);
int m355_adown_bwd_launch(const void* g1, int64_t g1_bstride, int32_t ld1, const void* g2, int64_t g2_bstride, int32_t ld2,
                          const uint8_t* argmax, void* gx, int64_t gx_bstride, int32_t ldg, int32_t B, int32_t H, int32_t W, int32_t c,
                          int32_t accumulate, void* stream);
/* Nearest 2x upsample of a slice x (B,H,W,[C]) into a slice y (B,2H,2W,[C]); argument checks as m355_sppf_pool_launch
 * (H, W at most 16384). */
int m355_upsample2x_launch(const void* x, int64_t x_bstride, int32_t ldx, void* y, int64_t y_bstride, int32_t ldy,
                           int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
/* ADown's pooling front of inference (yolov9c; adown_pool_kernel): with t = avg_pool2d(x, 2, 1, 0) of the slice x (B,H,W,[C]),
 * a (B,H-1,W-1,[C/2]) = t[..., :C/2] and m (B,H/2,W/2,[C/2]) = max_pool2d(t[..., C/2:], 3, 2, 1).  An average is
 * ((p00 + p01) + (p10 + p11)) * 0.25 in fp32, rounded to fp16 once; the max runs over those fp16 values (clipped windows).
 * H and W even, >= 2 and at most 16384, C a positive multiple of 16; the other argument checks as m355_sppf_pool_launch. */
int m355_adown_pool_launch(const void* x, int64_t x_bstride, int32_t ldx, void* a, int64_t a_bstride, int32_t lda, void* m,
                           int64_t m_bstride, int32_t ldm, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
/* Gradient glue of the training step (each replaces a strided torch expression reached from yolo_seg_train.py:12's backward):
 *  colsum: out[c] = sum over b < nb, r < rows of src[b * bstride + r * ld + c] for c < cols, fp32 result, fixed summation order
 *    (bias gradients: `d_raw[:, lo:hi, :].sum((0, 1))`, `gy.float().sum((0, 1, 2))`).  src fp32 (cols <= 256) or fp16 (src_f16 = 1:
 *    cols and ld multiples of 8, cols <= 2048); strides in elements; ws: m355_colsum_workspace_floats(nb, cols) floats.
 *  upsample2x_bwd: d (B,H,W,C) = or += the 2x2 sums of g (B,2H,2W,C) (fp32 sum of the four taps, one rounding to fp16;
 *    accumulate = 1 adds that fp16 value to d).  C, ldg, ldd multiples of 8.
 *  u8_to_f16x8: (npx, 3) uint8 -> (npx, 8) fp16 rows [r/255, g/255, b/255, 0 x5] = `(u8.float() / 255).half()`, the 8-channel
 *    input buffer of the training stem. */
int64_t m355_colsum_workspace_floats(int64_t nb, int32_t cols);
int m355_colsum_launch(const void* src, int32_t src_f16, int64_t nb, int64_t bstride, int64_t rows, int32_t ld, int32_t cols, float* ws,
                       float* out, void* stream);
int m355_upsample2x_bwd_launch(const void* g, int64_t g_bstride, int32_t ldg, void* d, int64_t d_bstride, int32_t ldd, int32_t B,
                               int32_t H, int32_t W, int32_t C, int32_t accumulate, void* stream);
int m355_u8_to_f16x8_launch(const uint8_t* src, void* dst, int64_t npx, void* stream);

/* Mask term of the segmentation loss with its gradients, forward and backward in one pass (replaces
 * v8SegmentationLoss.single_mask_loss and its autograd, reached from /root/reference/BscanBased/yolo_seg_train.py:12).
 * For slot k of image b (a foreground anchor): pred[p] = coef[b,k,:] . protos[b,p,:] over 32 channels,
 * slot_sum[b,k] = sum over the pixels p with x1 <= col < x2, y1 <= row < y2 of BCEWithLogits(pred[p], masks[b,p] == inst[b,k]);
 * with L = (1 / (mh mw)) sum_{b,k} weights[b,k] slot_sum[b,k]:  d_coef = dL/dcoef (B,K,32) fp32;  d_protos = g * dL/dprotos
 * (B,mh,mw,32), fp32 or fp16 (d_protos_f16 = 1), every element written, g = *gscale (a DEVICE scalar: the gradient arriving at L
 * in the caller's backward pass) or 1 when gscale is NULL.  slot_sum + d_coef and d_protos are two independent kernels: pass
 * slot_sum = d_coef = NULL or d_protos = NULL to run only one of them (forward: value and d_coef; backward: d_protos).
 * protos (B,mh,mw,32) NHWC fp16 (protos_f16 = 1) or fp32; masks (B,mh,mw) int32 overlap-encoded; boxes (B,K,4) x1,y1,x2,y2 in
 * prototype pixels; a slot with weight 0 is skipped (its outputs are 0).  No float atomics: bitwise reproducible. */
int m355_mask_loss_launch(const float* coef, const void* protos, int32_t protos_f16, const int32_t* masks, const int32_t* inst,
                          const float* boxes, const float* weights, int32_t B, int32_t K, int32_t mh, int32_t mw, float* slot_sum,
                          float* d_coef, void* d_protos, int32_t d_protos_f16, const float* gscale, void* stream);

/* Box (CIoU) and DFL terms of the loss on n foreground slots with their gradients w.r.t. the slot's 4 x 16 distribution logits,
 * one pass (replaces BboxLoss.forward / bbox_iou(CIoU=True) / DFLoss and their autograd, yolo_seg_train.py:12).  logits (n,4,16);
 * anchors (n,2) cell centres and targets (n,4) xyxy, both in grid units; weights (n), 0 = skip the slot (outputs 0).
 * box_term[s] = w (1 - CIoU(anchor -/+ E[softmax], target)), dfl_term[s] = w mean over the 4 sides of the two-bin cross entropy
 * at clamp(target distance, 0, 14.99); d_box / d_dfl (n,64) = d box_term / d logits, d dfl_term / d logits. */
int m355_box_loss_launch(const float* logits, const float* anchors, const float* targets, const float* weights, int64_t n,
                         float* box_term, float* dfl_term, float* d_box, float* d_dfl, void* stream);
/* Boxes and class scores of all anchors for the target assignment (no gradient): raw (rows, rw) head rows [64 DFL logits | nc class
 * logits | ...], row r belongs to anchor r % A -> boxes (rows,4) xyxy pixels = (anchor -/+ E[softmax over 16 bins]) * stride,
 * scores (rows,nc) = sigmoid.  anchors (A,2) grid units, strides (A). */
int m355_dfl_decode_launch(const float* raw, int64_t rows, int32_t A, int32_t rw, int32_t nc, const float* anchors, const float* strides,
                           float* boxes, float* scores, void* stream);
/* Class term of the detection loss with its gradient, one pass (replaces BCEWithLogitsLoss(reduction="none").sum() over (B, A, nc) and
 * its autograd in v8DetectionLoss).  raw / d_raw (rows, rw) head rows: the class logits x are read in place from columns
 * [64, 64 + nc) and d_raw's same columns get (sigmoid(x) - t) * s; every other column of d_raw is left alone.  targets (rows, nc)
 * dense.  s = *scale, a DEVICE scalar (gain * batch * loss scale / target sum: no host synchronisation).  out: DEVICE buffer of
 * m355_cls_bce_workspace_floats() floats; out[0] = sum over all elements of max(x, 0) - x t + log1p(exp(-|x|)), the per-block
 * partial sums sit behind it and a one-block kernel adds them in block order.  The grid depends on rows * nc only; no float atomics:
 * bitwise reproducible.  16-byte accesses of the targets always, of the rows when rw and nc are multiples of 4. */
size_t m355_cls_bce_workspace_floats(void);
int m355_cls_bce_launch(const float* raw, int32_t rw, const float* targets, int64_t rows, int32_t nc, const float* scale, float* d_raw,
                        float* out, void* stream);

/* Optimizer step over a flat fp32 parameter buffer (replaces torch.optim.AdamW / SGD + ModelEMA.update reached from
 * /root/reference/BscanBased/yolo_seg_train.py:12).  group[i]: 0 decayed weights, 1 norm weights, 2 biases (lr_bias).
 * grad_mul = clip_coef / loss_scale.  ema may be NULL.  step counts from 1 (Adam bias correction). */
int m355_adamw_step(float* p, const float* g, float* m, float* v, float* ema, const uint8_t* group, int64_t n, float lr,
                    float lr_bias, float beta1, float beta2, float eps, float weight_decay, int32_t step, float grad_mul,
                    float ema_decay, void* stream);
int m355_sgd_step(float* p, const float* g, float* momentum_buf, float* ema, const uint8_t* group, int64_t n, float lr,
                  float lr_bias, float momentum, int32_t nesterov, float weight_decay, float grad_mul, float ema_decay,
                  void* stream);
/* out[0] = sum of squares of the finite entries of g, out[1] = number of non-finite entries.  `out` is a DEVICE buffer of
 * m355_grad_sumsq_workspace_floats() floats (the block partials sit behind the two results; a one-block kernel adds them
 * in block order): fixed reduction order, bitwise reproducible. */
size_t m355_grad_sumsq_workspace_floats(void);
int m355_grad_sumsq(const float* g, int64_t n, float* out, void* stream);

/* Training-time augmentation on the device image cache (replaces upstream's CPU Mosaic / RandomPerspective /
 * RandomHSV / RandomFlip transforms run by dataloader workers under /root/reference/BscanBased/yolo_seg_train.py:12).
 * cache: uint8 (N,H,W,3); out: uint8 (B,H,W,3); params: DEVICE array of B records.  The polygons are transformed by
 * the caller with the forward matrix (host side, dataset.py). */
typedef struct {
  int32_t src[4];          /* cache indices: top-left, top-right, bottom-left, bottom-right of the mosaic */
  float xc, yc;            /* mosaic centre on the 2W x 2H canvas */
  float minv[6];           /* canvas (u, v) = [a b c; d e f] * (x, y, 1) for output pixel (x, y) */
  float hgain, sgain, vgain;
  int32_t flip;            /* 1: mirror the output left-right */
  int32_t mosaic;          /* 0: single image src[0] at the canvas origin */
} m355_aug_params;
int m355_augment(const void* d_cache, const m355_aug_params* d_params, void* d_out, int32_t B, int32_t H, int32_t W,
                 void* stream);

/* The rest of upstream's chain -- degrees / shear / perspective (RandomPerspective), flipud (RandomFlip), mixup (MixUp) and
 * copy_paste (CopyPaste, flip mode) -- on the same image cache, still one launch per batch (csrc/augment_ex.hip, DESIGN.md
 * section 16).  An output image blends up to two LAYERS; a layer is what m355_aug_params describes, with two differences:
 *   - minv is a full inverse homography: output pixel (x, y) samples the canvas at
 *       (m0 x + m1 y + m2, m3 x + m4 y + m5) / (m6 x + m7 y + m8);   m6 = m7 = 0, m8 = 1 is m355_augment's affine;
 *   - a paste list, polygons [poly_first, poly_first + poly_count) of the table, in canvas coordinates.  Canvas texel
 *     (cx, cy) is PASTED when the point (cx, cy) is inside any listed polygon, and then reads the mirrored canvas texel
 *     (Wc - 1 - cx, cy) in place of (cx, cy); Wc = 2W with mosaic, W without.  Each of the four bilinear corners decides for
 *     itself.  Inside is even-odd over the edges (a, b) of the polygon: an edge is crossed when (a.y > cy) != (b.y > cy) and
 *     cx lies strictly left of the edge at height cy, evaluated without a division as
 *       d = b.y - a.y;   d > 0 ? (cx - a.x) * d < (cy - a.y) * (b.x - a.x) : (cx - a.x) * d > (cy - a.y) * (b.x - a.x).
 *     So a polygon owns its left and top edges and not its right and bottom ones: a point on an edge has one answer.
 *     [x0, x1] x [y0, y1] is a polygon's inclusive integer bounding box; a texel outside it is never tested, so the box must
 *     cover the vertices (floor of the minima, ceil of the maxima).
 * Per output pixel: flip / flipud applied to (x, y), each layer sampled bilinearly (border 114), rgb = mix * layer 0 +
 * (1 - mix) * layer 1 in fp32 when n_layers == 2, then the HSV gains, round half up and clip as in m355_augment.  The file
 * is built without FMA contraction: a float32 restatement in the same operation order gives the same bytes.
 * h_params (B records), h_polys (n_polys) and h_verts (n_verts x,y pairs) are HOST arrays; the entry checks them, copies them
 * into d_work (a device buffer of at least m355_augment_ex_workspace_bytes() bytes, 16-byte aligned) on `stream` and launches.
 * The three host arrays must stay valid and unchanged until `stream` has executed the copies this call enqueues (they may be
 * pageable; synchronise the stream, or record an event after the call and wait for it, before freeing or rewriting them), and
 * d_work until the kernel has run.
 * M355_ERR_INVALID, before any HIP call: a NULL pointer (h_polys / h_verts may be NULL when their count is 0); B, H or W < 1,
 * B > 65535, H or W > 16384; n_images < 1 or a src index outside [0, n_images); n_layers not 1 or 2; n_polys or n_verts < 0;
 * a layer's polygon range outside [0, n_polys) or longer than M355_AUG_MAX_PASTE; a polygon's vertex range outside
 * [0, n_verts), empty or longer than M355_AUG_MAX_POLY_VERTS; work_bytes too small or d_work misaligned.  The caller drops
 * surplus pastes; the cap bounds the work of one output pixel. */
#define M355_AUG_MAX_PASTE 32          /* polygons in one layer's paste list */
#define M355_AUG_MAX_POLY_VERTS 1024   /* vertices of one paste polygon */
typedef struct {
  int32_t src[4];          /* cache indices, as in m355_aug_params */
  float xc, yc;            /* mosaic centre on the canvas */
  float minv[9];           /* inverse homography, row-major */
  int32_t mosaic;          /* 0: single image src[0] at the canvas origin */
  int32_t poly_first, poly_count;
} m355_aug_layer;
typedef struct {
  m355_aug_layer layer[2];
  int32_t n_layers;        /* 1, or 2 for mixup */
  float mix;               /* weight r of layer 0; layer 1 gets 1 - r */
  float hgain, sgain, vgain;
  int32_t flip;            /* 1: output column x reads column W-1-x */
  int32_t flipud;          /* 1: output row y reads row H-1-y */
} m355_aug_ex_params;
typedef struct {
  int32_t vert_first, vert_count;   /* vertices [vert_first, vert_first + vert_count) of h_verts, canvas coordinates */
  int32_t x0, y0, x1, y1;           /* inclusive integer bounding box */
} m355_aug_poly;
size_t m355_augment_ex_workspace_bytes(int32_t B, int32_t n_polys, int32_t n_verts);
int m355_augment_ex(const void* d_cache, int32_t n_images, const m355_aug_ex_params* h_params, const m355_aug_poly* h_polys,
                    int32_t n_polys, const float* h_verts, int32_t n_verts, void* d_work, int64_t work_bytes, void* d_out,
                    int32_t B, int32_t H, int32_t W, void* stream);

/* ---- D-FINE decoder hot ops (/root/reference/D-Fine/temporal_dfine.py:160-181) ---------------
 * The reference reaches these through transformers' modeling_d_fine.py; each entry point names what it replaces.
 *
 * m355_msda_forward = multi_scale_deformable_attention_v2 (modeling_d_fine.py:150-221), called by every decoder
 * layer's cross-attention under `self.dfine.model(pixel_values=...)` (temporal_dfine.py:162).
 *   value  (B, S, heads, head_dim) fp32, S = sum of h*w over the levels, head_dim must be 32
 *   shapes_hw: HOST array [num_levels][2] = (height, width); points_per_level: HOST array, sums to P (<= 32)
 *   loc    (B, Q, heads, P, 2) fp32 (x, y); attn (B, Q, heads, P) fp32 (already soft-maxed by the caller)
 *   discrete 0: method "default" (bilinear grid_sample on 2*loc-1, zeros padding, align_corners=False)
 *            1: method "discrete" (nearest pixel of loc * (w, h) + 0.5, clamped)
 *   out    (B, Q, heads * head_dim) fp32 */
int m355_msda_forward(const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim, const int32_t* shapes_hw,
                      int32_t num_levels, const float* d_loc, const float* d_attn, const int32_t* points_per_level,
                      int32_t Q, int32_t P, int32_t discrete, float* d_out, void* stream);
/* m355_msda_module_forward = the part of DFineMultiscaleDeformableAttention.forward (modeling_d_fine.py:268-311) behind its
 * two linear layers, for 4-d reference points and method "default": softmax of the attention logits over the P points,
 * sampling location = ref.xy + offset * (1 / points of the level) * ref.wh * offset_scale, then the core above.
 *   ref (B, Q, 4) cx, cy, w, h; offsets (B, Q, heads, P, 2) and logits (B, Q, heads, P): raw outputs of
 *   `sampling_offsets` / `attention_weights`; P <= 16; out (B, Q, heads * head_dim). */
int m355_msda_module_forward(const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim, const int32_t* shapes_hw,
                             int32_t num_levels, const float* d_ref, const float* d_offsets, const float* d_logits,
                             const int32_t* points_per_level, int32_t Q, int32_t P, float offset_scale, float* d_out,
                             void* stream);
/* m355_dfine_decode = DFineIntegral.forward (modeling_d_fine.py:756-778) + distance2bbox (:1115-1137) [+ .clamp(0, 1)],
 * temporal_dfine.py:180-181.  dist (n, 4 * num_bins_plus1) fp32 logits; project (num_bins_plus1) fp32 = W(n) from
 * weighting_function (:1091-1112, host side: dfine.py); ref (n, 4) fp32 (cx, cy, w, h); boxes (n, 4) fp32 (cx, cy, w, h). */
int m355_dfine_decode(const float* d_dist, const float* d_project, const float* d_ref, float* d_boxes, int64_t n,
                      int32_t num_bins_plus1, float reg_scale, int32_t clamp01, void* stream);

/* ---- Backward of the three entries above, for fine-tuning runs that call the ops under loss.backward() --------------
 * (the reference's D-FINE trainers: D-Fine/temp_dfine_over_improved.py:152-157, 250-272; temporal_dfine.py:175-181).
 * fp32, same layouts as the forward twins.  No float atomics: every gradient is bitwise reproducible.
 *
 * m355_msda_backward = backward of m355_msda_forward.
 *   grad_out   (B, Q, heads * head_dim); value / loc / attn / shapes_hw / points_per_level / discrete as the forward
 *   grad_value (B, S, heads, head_dim), grad_loc (B, Q, heads, P, 2), grad_attn (B, Q, heads, P): each may be NULL
 *              ("not needed": its work is skipped); every element of a non-NULL output is written
 *   discrete 0: grid_sample backward (bilinear, zeros padding, align_corners=False): corners outside the map contribute
 *               nothing to any gradient;  1: grad_loc is zeros, the other two go through the one selected pixel
 *   work       device scratch of m355_msda_backward_workspace_bytes(B, Q, heads, P) bytes, 16-byte aligned; needed when
 *              grad_value is asked for (one {pixel, weight} entry per (q, point, corner), summed per pixel in that order) */
size_t m355_msda_backward_workspace_bytes(int32_t B, int32_t Q, int32_t heads, int32_t P);
int m355_msda_backward(const float* d_grad_out, const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim,
                       const int32_t* shapes_hw, int32_t num_levels, const float* d_loc, const float* d_attn,
                       const int32_t* points_per_level, int32_t Q, int32_t P, int32_t discrete, float* d_grad_value,
                       float* d_grad_loc, float* d_grad_attn, void* d_work, int64_t work_bytes, void* stream);
/* m355_msda_module_backward = backward of m355_msda_module_forward: the softmax and the sampling locations are recomputed
 * in the kernel, then the softmax backward over the P points and the chain rule of
 * location = ref.xy + offset * (1 / points of the level) * ref.wh * offset_scale.
 *   grad_value as above, grad_ref (B, Q, 4), grad_offsets (B, Q, heads, P, 2), grad_logits (B, Q, heads, P): each may be
 *   NULL; work as above, needed for grad_value and grad_ref (per-head partials, added in head order); P <= 16. */
int m355_msda_module_backward(const float* d_grad_out, const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim,
                              const int32_t* shapes_hw, int32_t num_levels, const float* d_ref, const float* d_offsets,
                              const float* d_logits, const int32_t* points_per_level, int32_t Q, int32_t P, float offset_scale,
                              float* d_grad_value, float* d_grad_ref, float* d_grad_offsets, float* d_grad_logits, void* d_work,
                              int64_t work_bytes, void* stream);
/* m355_dfine_decode_backward = backward of m355_dfine_decode: grad_boxes (n, 4) -> grad_dist (n, 4 * num_bins_plus1)
 * (softmax-expectation backward per side) and grad_ref (n, 4); either may be NULL.  With clamp01 the gradient passes where
 * 0 <= box <= 1, as torch.clamp does.  project is a constant (no gradient). */
int m355_dfine_decode_backward(const float* d_grad_boxes, const float* d_dist, const float* d_project, const float* d_ref,
                               float* d_grad_dist, float* d_grad_ref, int64_t n, int32_t num_bins_plus1, float reg_scale,
                               int32_t clamp01, void* stream);

/* ---- Hungarian matcher of the D-FINE loss ------------------------------------------------------------------------------
 * m355_dfine_match = RTDetrHungarianMatcher.forward (transformers/loss/loss_rt_detr.py:68-120), which the reference's D-FINE
 * trainers reach through `self.dfine.loss_function(...)` once per frame: the (Q x n_b) cost matrix of every image
 *   bbox_cost * L1(cxcywh) + class_cost * class_term + giou_cost * (-GIoU(xyxy))          (fp32, upstream's order)
 *   class_term: use_focal_loss != 0: alpha (1-p)^gamma (-log(p + 1e-8)) - (1-alpha) p^gamma (-log(1 - p + 1e-8)), p = sigmoid(logit)
 *               use_focal_loss == 0: -softmax(logits)[target class]
 * and its optimal assignment (shortest augmenting paths as in scipy.optimize.linear_sum_assignment, duals in fp64), ONE launch,
 * one block per image, asynchronous on `stream`, no host round trip.  All buffers are the caller's.
 *   logits (B, Q, C) fp32; pred_boxes (B, Q, 4) fp32 cx, cy, w, h
 *   target_labels (T) int64 and target_boxes (T, 4) fp32: the targets of all images, concatenated in image order
 *   d_target_offsets (B + 1) int32 DEVICE: image b owns targets [offsets[b], offsets[b + 1]);
 *   h_target_counts (B) int32 HOST: the same counts n_b, what the host validates and sizes buffers by.  A device offset that
 *     disagrees with them is never followed out of bounds: that image gets flag 2 and no match
 *   work: m355_dfine_match_workspace_bytes(B, Q, max n_b) bytes (may be NULL when that is 0: the matrices fit in LDS)
 *   d_cost: NULL, or (B, Q, max n_b) fp32; entry [b][q][t] for t < n_b is written, the rest is left alone
 *   rows, cols (B, kmax) int64, kmax >= min(Q, max n_b): the first K_b = min(Q, n_b) entries of image b are the matched query /
 *     target (index within the image) pairs by ascending query index, scipy's output order; the entries behind them are -1
 *   flags (B) int32: 0 solved; 1 some cost of the image is NaN or +-inf (a label outside [0, C) counts): the solve is skipped and
 *     all kmax entries are -1; the other images are unaffected
 * Limits, checked on the host before any HIP call (M355_ERR_INVALID): no NULL pointer, B >= 1, 1 <= Q <= 2048, C >= 1,
 * 0 <= n_b <= 512, kmax and work_bytes large enough.  No atomics: bitwise reproducible; an exact tie goes to the lowest index. */
size_t m355_dfine_match_workspace_bytes(int32_t B, int32_t Q, int32_t max_targets);
int m355_dfine_match(const float* d_logits, const float* d_pred_boxes, int32_t B, int32_t Q, int32_t C,
                     const int64_t* d_target_labels, const float* d_target_boxes, const int32_t* d_target_offsets,
                     const int32_t* h_target_counts, float class_cost, float bbox_cost, float giou_cost, float alpha, float gamma,
                     int32_t use_focal_loss, void* d_work, int64_t work_bytes, float* d_cost, int64_t* d_rows, int64_t* d_cols,
                     int32_t kmax, int32_t* d_flags, void* stream);

/* ---- Detection post-processing of a D-FINE / RT-DETR output ------------------------------------------------------------
 * m355_dfine_postprocess = RTDetrImageProcessor.post_process_object_detection (transformers
 * models/rt_detr/image_processing_rt_detr.py:482-552, the use_focal_loss=True branch), which the reference's predict and eval
 * scripts call once per frame: the K = Q best of the Q * C candidates of every image, ONE launch, one block per image,
 * asynchronous on `stream`, no host round trip.  All buffers are the caller's.
 *   logits (B, Q, C) fp32; pred_boxes (B, Q, 4) fp32 cx, cy, w, h
 *   sizes: NULL, or DEVICE (B, 2) fp32 (height, width) of each image; threshold: the score threshold
 * Order of the rows, a total order on the flat candidates i = q * C + c: NaN logits first (torch.topk treats NaN as the
 * greatest), then descending logit (sigmoid is monotone; -0 == +0), an exact tie to the lowest i.  Row r of image b:
 *   scores[b][r] = 1 / (1 + exp(-logit)) in fp32; labels[b][r] = i % C (int64); with q = i / C
 *   boxes[b][r] = (cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h) of query q, then * (W, H, W, H) when sizes is given: one fp32
 *     operation each, upstream's order, so the bits are torch's fp32 result
 *   counts[b] = {n_nan, n_keep} int32: the number of leading NaN rows, and the number of rows with score > threshold (the
 *     kernel's own fp32 score; no NaN row is among them).  The rows being sorted, upstream's three boolean masks are the
 *     slice [n_nan, n_nan + n_keep).
 * scores (B, Q), labels (B, Q), boxes (B, Q, 4) and counts (B, 2) are written in full.
 * Limits, checked on the host before any HIP call (M355_ERR_INVALID): no NULL among the required pointers, B >= 1,
 * 1 <= Q <= 2048, C >= 1, Q * C < 2^24.  Integer LDS counters only, no float atomics: bitwise reproducible, and image b of a
 * batch gives the bits of the same image alone. */
int m355_dfine_postprocess(const float* d_logits, const float* d_pred_boxes, int32_t B, int32_t Q, int32_t C, const float* d_sizes,
                           float threshold, float* d_scores, int64_t* d_labels, float* d_boxes, int32_t* d_counts, void* stream);

/* ---- Image pre-processing of a D-FINE / RT-DETR model --------------------------------------------------------------------
 * m355_dfine_preprocess = RTDetrImageProcessorPil.preprocess with its defaults (transformers
 * models/rt_detr/image_processing_pil_rt_detr.py: resize to a fixed (out_h, out_w) with Pillow's BILINEAR, rescale, no normalise,
 * no pad), which every D-FINE script of the reference runs on the host for each sequence of frames: T decoded uint8 RGB images
 * (h, w, 3) of any mix of sizes, packed in the device buffer d_src, become the model's input d_out fp32 (T, 3, out_h, out_w),
 * contiguous and planar, bit for bit what the processor returns.  At most TWO launches whatever T and however many sizes:
 * the horizontal pass of every image that needs one into the uint8 scratch d_work (rows of 3 * out_w bytes), then the vertical
 * pass and the rescale; asynchronous on `stream`, no host round trip.
 *
 * Pillow's 8-bit resize is a separable fixed-point filter; its per-axis tables are built by the caller
 * (dfine.resize_tables) and shared by all images of one (in, out) pair.  Axis table a lies in the int32 pool at
 * axes[a].offset: xmin[out_size], count[out_size], coef[out_size][ksize].  A pass computes
 * clip((2^21 + sum_{t < count} coef[t] * pixel[xmin + t]) >> 22, 0, 255) in int32 into uint8: horizontal first, the uint8 result
 * feeds the vertical pass; the final byte b becomes rescale[b] (256 fp32 values of the caller, no device arithmetic).  A pass
 * whose sizes are equal has table index -1 and is a copy.
 *
 * The three tables are passed twice: h_* on the HOST, which this call validates before any HIP call, and d_* their DEVICE
 * copies with the same bytes, which the kernels read (the caller keeps both in one staging buffer and uploads it once).
 * M355_ERR_INVALID: a NULL pointer; T outside [1, 65535]; out_h outside [1, M355_DFINE_PRE_MAX_H], out_w outside
 * [4, M355_DFINE_PRE_MAX_W] or not a multiple of 4 (16-byte stores); d_src, d_work or d_out not 16-byte aligned; src_bytes not a
 * multiple of 16 (rows are staged in 16-byte loads); an axis with in_size or out_size out of range, ksize outside
 * [1, M355_DFINE_PRE_MAX_TAPS], a table that leaves the pool, count outside [1, ksize], xmin < 0 or xmin + count > in_size, a
 * coefficient outside [0, 2^23] or a row of coefficients summing above 2^23 (the int32 sums stay below 2^31); an image whose
 * offset is negative or not a multiple of 16, whose bytes leave [0, src_bytes), whose in_h is outside [1, M355_DFINE_PRE_MAX_H]
 * or in_w outside [1, M355_DFINE_PRE_MAX_W], whose table index is neither -1 with in == out nor an axis of its (in, out), or
 * whose mid_row is not the sum of in_h over the earlier images with a horizontal pass; a scratch smaller than those rows. */
#define M355_DFINE_PRE_MAX_TAPS 64
#define M355_DFINE_PRE_MAX_W 4096
#define M355_DFINE_PRE_MAX_H 16384
typedef struct {
  int64_t offset;            /* byte offset of the image's first pixel in d_src, a multiple of 16; 3 * in_h * in_w bytes */
  int32_t in_h, in_w;        /* source size */
  int32_t htab, vtab;        /* axis table of the horizontal / vertical pass, -1: skipped (in_w == out_w / in_h == out_h) */
  int32_t mid_row;           /* first of the image's in_h rows in d_work (read only where htab >= 0) */
  int32_t reserved;
} m355_dfine_pre_image;
typedef struct {
  int32_t in_size, out_size;
  int32_t ksize;             /* coefficients stored per output index */
  int32_t offset;            /* index of the table's first int32 in the pool */
} m355_dfine_pre_axis;
int m355_dfine_preprocess(const uint8_t* d_src, int64_t src_bytes, const m355_dfine_pre_image* h_images,
                          const m355_dfine_pre_image* d_images, int32_t T, const m355_dfine_pre_axis* h_axes,
                          const m355_dfine_pre_axis* d_axes, int32_t n_axes, const int32_t* h_pool, const int32_t* d_pool,
                          int64_t pool_len, const float* d_rescale, int32_t out_h, int32_t out_w, void* d_work, int64_t work_bytes,
                          float* d_out, void* stream);

/* ---- Encoder query selection of a D-FINE model ---------------------------------------------------------------------------
 * m355_dfine_select_forward = the block of DFineModel.forward between the encoder's heads and the decoder (transformers 5.15.0
 * modeling_d_fine.py:1804-1828): per image the K tokens with the greatest score, score = the max over C of class_logits, and the
 * rows of the three tensors at those tokens.  Two launches (row max on all CUs into `work`; one block per image: top-K and
 * gathers), asynchronous on `stream`, no host round trip.  All buffers are the caller's, fp32, dense; no alignment is required
 * (16-byte aligned class_logits / memory rows are moved 16 bytes at a time).
 *   class_logits (B, S, C); coord_logits (B, S, 4); memory (B, S, D) or NULL (then target is NULL too and D is not read)
 * Order of the rows, a total order on the tokens: a NaN score first (the score is NaN when its row holds one, as torch.max
 * gives, and torch.topk treats NaN as the greatest), then descending score (-0 == +0), an exact tie to the lowest token.
 *   indices (B, K) int64: the tokens; ref (B, K, 4), logits (B, K, C), target (B, K, D): the rows of coord_logits,
 *   class_logits and memory at them, copied bit for bit; boxes (B, K, 4) = 1 / (1 + expf(-ref)), fp32
 *   inverse (B, S) int32 or NULL: the rank of a selected token, -1 elsewhere: what the backward reads
 * Every element of every output is written.
 * m355_dfine_select_backward: ONE launch.  grad_ref, grad_boxes (B, K, 4), grad_logits (B, K, C), grad_target (B, K, D): the
 * upstream gradients, each may be NULL (zero); grad_class (B, S, C), grad_coord (B, S, 4), grad_memory (B, S, D): each may be NULL
 * (not needed), the others are written in full in one streaming pass: the row of a token with rank r is grad_logits[r],
 * grad_ref[r] + grad_boxes[r] * (1 - boxes[r]) * boxes[r], grad_target[r]; any other row is zero.  boxes: the forward's (read when
 * grad_boxes and grad_coord are given).  The tokens of an image are distinct: no memset, no atomics, nothing is summed.
 * work: m355_dfine_select_workspace_bytes(B, S) = 4 B S bytes (0 for a shape outside the limits), 4-byte aligned.
 * Limits, checked on the host before any HIP call (M355_ERR_INVALID): no NULL among the required pointers, memory and target
 * together, B >= 1, C >= 1, D >= 1 where its tensor is given, 1 <= S < 2^24, B * S < 2^31, 1 <= K <= min(S, 2048), the workspace
 * size.  Integer LDS counters only, no float atomics: bitwise reproducible, and image b of a batch gives the bits of the same
 * image alone. */
size_t m355_dfine_select_workspace_bytes(int32_t B, int32_t S);
int m355_dfine_select_forward(const float* d_class_logits, const float* d_coord_logits, const float* d_memory, int32_t B, int32_t S,
                              int32_t C, int32_t D, int32_t K, void* d_work, int64_t work_bytes, int64_t* d_indices, float* d_ref,
                              float* d_boxes, float* d_logits, float* d_target, int32_t* d_inverse, void* stream);
int m355_dfine_select_backward(const float* d_grad_ref, const float* d_grad_boxes, const float* d_grad_logits, const float* d_grad_target,
                               const float* d_boxes, const int32_t* d_inverse, int32_t B, int32_t S, int32_t C, int32_t D, int32_t K,
                               float* d_grad_class, float* d_grad_coord, float* d_grad_memory, void* stream);

/* ---- Loss terms of one D-FINE decoder output ---------------------------------------------------------------------------
 * m355_dfine_loss_forward = RTDetrLoss.loss_labels_vfl + loss_boxes (transformers/loss/loss_rt_detr.py:165-254) and, with the
 * local group, DFineLoss.loss_local (loss_d_fine.py:228-301): the five UNWEIGHTED terms, fp32, upstream's expressions.
 *   logits (B, Q, C), pred_boxes (B, Q, 4) cx, cy, w, h: contiguous fp32
 *   match_q, match_t (M) int64: the match entries, those of image b contiguous and in image order: query index and target index
 *     WITHIN the image (what the matcher's rows / cols hold).  d_offsets (2 (B + 1)) int32 DEVICE: first entry of each image
 *     (B + 1 values, the last one M), then first target row of each image (B + 1 values, the last one T).
 *     An entry whose query is outside [0, Q) or whose target is outside the image's targets (the matcher's -1 entries included)
 *     is skipped in every term; an offset outside [0, M] / [0, T] is clamped: nothing is followed out of bounds.
 *     The caller promises at most one valid entry per (b, q).
 *   target_labels (T) int64, target_boxes (T, 4) fp32: the targets of all images, concatenated in image order
 *   num_boxes > 0: the host-side normaliser; alpha, gamma: the varifocal weight alpha * sigmoid(x)^gamma
 *   local group, all NULL or all present: pred_corners, teacher_corners (B, Q, 4 * num_bins_plus1), ref_points (B, Q, 4),
 *     teacher_logits (B, Q, C), project (num_bins_plus1) = W(n), with reg_scale and the temperature T of the KL term
 *   work: m355_dfine_loss_workspace_bytes(B, Q) bytes
 *   out (8) fp32: loss_vfl, loss_bbox, loss_giou, loss_fgl, loss_ddf (the last two 0 without the local group), then three
 *     values the backward reads.  Pass the same buffer to m355_dfine_loss_backward as d_saved.
 * Two launches (per-query partials; one block adds them in block order), asynchronous on `stream`, no read-back.
 * m355_dfine_loss_backward: one launch that recomputes per query and writes EVERY element of grad_logits (B, Q, C),
 * grad_pred_boxes (B, Q, 4) and grad_pred_corners (B, Q, 4 * num_bins_plus1) (zeros where no term reaches); any of the three
 * may be NULL.  d_grad_terms (5) fp32 DEVICE: the upstream gradient of each term, any combination.
 * No atomics: bitwise reproducible.  Limits, checked on the host before any HIP call (M355_ERR_INVALID): B, Q, C >= 1,
 * B * Q < 2^31, M >= 0, num_bins_plus1 in [2, 64], no NULL among the required pointers, local group all or none, workspace. */
size_t m355_dfine_loss_workspace_bytes(int32_t B, int32_t Q);
int m355_dfine_loss_forward(const float* d_logits, const float* d_pred_boxes, int32_t B, int32_t Q, int32_t C,
                            const int64_t* d_match_q, const int64_t* d_match_t, int32_t M, const int32_t* d_offsets,
                            const int64_t* d_target_labels, const float* d_target_boxes, int32_t T, float num_boxes, float alpha,
                            float gamma, const float* d_pred_corners, const float* d_ref_points, const float* d_teacher_corners,
                            const float* d_teacher_logits, const float* d_project, int32_t num_bins_plus1, float reg_scale,
                            float temperature, void* d_work, int64_t work_bytes, float* d_out, void* stream);
int m355_dfine_loss_backward(const float* d_grad_terms, const float* d_logits, const float* d_pred_boxes, int32_t B, int32_t Q,
                             int32_t C, const int64_t* d_match_q, const int64_t* d_match_t, int32_t M, const int32_t* d_offsets,
                             const int64_t* d_target_labels, const float* d_target_boxes, int32_t T, float num_boxes, float alpha,
                             float gamma, const float* d_pred_corners, const float* d_ref_points, const float* d_teacher_corners,
                             const float* d_teacher_logits, const float* d_project, int32_t num_bins_plus1, float reg_scale,
                             float temperature, const float* d_saved, float* d_grad_logits, float* d_grad_pred_boxes,
                             float* d_grad_pred_corners, void* stream);

/* ---- The temporal encoder layer of the D-FINE trainers, between its GEMMs ----------------------------------------------
 * nn.TransformerEncoderLayer(d_model = 32 * heads, post-norm, ReLU, batch_first) with the nn.Linear layers left to the caller:
 *   x1  = addln(x,  out_proj(attn(in_proj(x))), norm1)
 *   out = addln(x1, linear2(relu_dropout(linear1(x1))), norm2)
 * All tensors contiguous fp32 on the device, 16-byte aligned; fp32 accumulation; asynchronous on `stream`; no float atomics:
 * bitwise reproducible, and row / frame b of a batch gives the bits of the same row / frame alone.
 * Dropout (p, seed, site): element e of a site's tensor (flat row-major index) is kept when word e % 4 of
 * Philox4x32-10(counter = (e / 4 lo, e / 4 hi, site, 0), key = (seed lo, seed hi)) is >= floor(p * 2^32), and a kept value is
 * scaled by 1 / (1 - p).  The backward recomputes the mask from the same three numbers; no mask is stored.  p = 0 runs the
 * kernels built without the generator.  m355_dfine_dropout_mask writes that mask (n bytes, 0 / 1) with the same device function.
 *
 * m355_dfine_attn_forward: qkv (B, S, 3 D), D = 32 heads, exactly F.linear(x, in_proj_weight, in_proj_bias): head h reads q, k, v at
 *   columns 32 h, D + 32 h, 2 D + 32 h.  out (B, S, D) = softmax(q k^T / sqrt(32)) [dropout on the (B, heads, S, S) probabilities] v
 *   in the layout out_proj reads; lse (B, heads, S, 2), the log-sum-exp of each row's logits * log2(e) as the pair (maximum,
 *   log2 of the sum of exp2(logit - maximum)), or NULL when nothing is kept for a backward.  The scores never reach memory.
 * m355_dfine_attn_backward: grad_qkv (B, S, 3 D), every element written, from grad_out, qkv, out and lse (probabilities recomputed;
 *   dK / dV summed by the block that owns the key rows, dQ by the block that owns the query rows).
 * m355_dfine_addln_forward: out (M, D) = LayerNorm(x + dropout(y)) * weight + bias over the last axis (biased variance, eps inside
 *   the root); mean, rstd (M) are written for the backward.
 * m355_dfine_addln_backward: grad_x, grad_y (M, D), grad_weight, grad_bias (D); any of the four may be NULL.  The two parameter
 *   gradients are column sums in a fixed order (partial rows per block in work, then one ordered pass): two launches.
 *   work: m355_dfine_addln_workspace_bytes(M, D) bytes.
 * m355_dfine_relu_dropout_forward: out (n) = dropout(relu(h)).  _backward: grad_h = grad_out * 1 / (1 - p) where the mask keeps
 *   the element and the forward's output is positive, else 0.
 * Limits, checked on the host before any HIP call (M355_ERR_INVALID): no NULL among the required pointers, 16-byte alignment,
 * head_dim == 32, B and heads in [1, 65535], S >= 1, M >= 1, D a multiple of 4 in [4, 1024], n >= 1, p in [0, 1), site >= 0,
 * the workspace size. */
int m355_dfine_attn_forward(const float* d_qkv, int32_t B, int32_t S, int32_t H, int32_t head_dim, float p, uint64_t seed,
                            int32_t site, float* d_out, float* d_lse, void* stream);
int m355_dfine_attn_backward(const float* d_grad_out, const float* d_qkv, const float* d_out, const float* d_lse, int32_t B, int32_t S,
                             int32_t H, int32_t head_dim, float p, uint64_t seed, int32_t site, float* d_grad_qkv, void* stream);
size_t m355_dfine_addln_workspace_bytes(int64_t M, int32_t D);
int m355_dfine_addln_forward(const float* d_x, const float* d_y, const float* d_weight, const float* d_bias, int64_t M, int32_t D,
                             float eps, float p, uint64_t seed, int32_t site, float* d_out, float* d_mean, float* d_rstd, void* stream);
int m355_dfine_addln_backward(const float* d_grad_out, const float* d_x, const float* d_y, const float* d_weight, const float* d_mean,
                              const float* d_rstd, int64_t M, int32_t D, float p, uint64_t seed, int32_t site, float* d_grad_x,
                              float* d_grad_y, float* d_grad_weight, float* d_grad_bias, void* d_work, int64_t work_bytes, void* stream);
int m355_dfine_relu_dropout_forward(const float* d_h, int64_t n, float p, uint64_t seed, int32_t site, float* d_out, void* stream);
int m355_dfine_relu_dropout_backward(const float* d_grad_out, const float* d_out, int64_t n, float p, uint64_t seed, int32_t site,
                                     float* d_grad_h, void* stream);
int m355_dfine_dropout_mask(int64_t n, float p, uint64_t seed, int32_t site, uint8_t* d_mask, void* stream);

/* ---- A D-FINE decoder layer and its quality head between their GEMMs ------------------------------------------------------
 * transformers' DFineDecoderLayer / DFineLQE (models/d_fine/modeling_d_fine.py) run these between their nn.Linear products;
 * self-attention is m355_dfine_attn_*, cross-attention m355_msda_module_*, the first LayerNorm m355_dfine_addln_*.  fp32, row
 * major, no float atomics, bitwise reproducible; a row's result does not depend on the rows around it.
 * m355_dfine_addln_clamp_forward / _backward: m355_dfine_addln_* without dropout and with z = clamp(x + y, lo, hi) in front of
 *   the statistics (final_layer_norm(hidden.clamp(-65504, 65504))); grad_x and grad_y are 0 where x + y lies strictly outside
 *   [lo, hi].  Same workspace, same NULL-able gradients.
 * m355_dfine_gate_ln_forward: out (M, D) = LayerNorm(sigmoid(gate[:, :D]) * x1 + sigmoid(gate[:, D:]) * x2) * weight + bias, gate
 *   (M, 2 D) being DFineGate's nn.Linear output; mean, rstd (M) are written for the backward, nothing else is kept.
 * m355_dfine_gate_ln_backward: grad_gate (M, 2 D), grad_x1, grad_x2 (M, D), grad_weight, grad_bias (D); each may be NULL and its
 *   work is skipped.  work (m355_dfine_addln_workspace_bytes(M, D)) is needed for grad_weight / grad_bias only.
 * m355_dfine_lqe_forward: pred_corners (M, 4 * num_bins_plus1) -> stat (M, 4 * (top_k + 1)): per side the softmax over its
 *   num_bins_plus1 logits, the top_k largest probabilities in descending order, then their mean (what DFineLQE.reg_conf reads).
 *   index (M, 4, top_k) bytes, NULL when no backward follows: the chosen bins; of bins with equal probability the lowest first.
 * m355_dfine_lqe_backward: grad_pred_corners (M, 4 * num_bins_plus1) from grad_stat and the forward's index.
 * Limits (M355_ERR_INVALID before any HIP call): no NULL among the required pointers, 16-byte alignment (not for lqe), M >= 1,
 * D a multiple of 4 in [4, 1024], lo <= hi, top_k in [1, 8], top_k <= num_bins_plus1 <= 64, the workspace size. */
int m355_dfine_addln_clamp_forward(const float* d_x, const float* d_y, const float* d_weight, const float* d_bias, int64_t M, int32_t D,
                                   float eps, float lo, float hi, float* d_out, float* d_mean, float* d_rstd, void* stream);
int m355_dfine_addln_clamp_backward(const float* d_grad_out, const float* d_x, const float* d_y, const float* d_weight,
                                    const float* d_mean, const float* d_rstd, int64_t M, int32_t D, float lo, float hi,
                                    float* d_grad_x, float* d_grad_y, float* d_grad_weight, float* d_grad_bias, void* d_work,
                                    int64_t work_bytes, void* stream);
int m355_dfine_gate_ln_forward(const float* d_gate, const float* d_x1, const float* d_x2, const float* d_weight, const float* d_bias,
                               int64_t M, int32_t D, float eps, float* d_out, float* d_mean, float* d_rstd, void* stream);
int m355_dfine_gate_ln_backward(const float* d_grad_out, const float* d_gate, const float* d_x1, const float* d_x2,
                                const float* d_weight, const float* d_mean, const float* d_rstd, int64_t M, int32_t D,
                                float* d_grad_gate, float* d_grad_x1, float* d_grad_x2, float* d_grad_weight, float* d_grad_bias,
                                void* d_work, int64_t work_bytes, void* stream);
int m355_dfine_lqe_forward(const float* d_pred_corners, int64_t M, int32_t num_bins_plus1, int32_t top_k, float* d_stat, uint8_t* d_index,
                           void* stream);
int m355_dfine_lqe_backward(const float* d_grad_stat, const float* d_pred_corners, const uint8_t* d_index, int64_t M,
                            int32_t num_bins_plus1, int32_t top_k, float* d_grad_pred_corners, void* stream);

/* ---- The loop of a D-FINE decoder around its layers, between its GEMMs ------------------------------------------------------
 * What transformers' DFineDecoder.forward runs per layer besides the layers, the LQE heads and its nn.Linear products.  fp32, row
 * major, contiguous, asynchronous on `stream`; no atomics, every sum in a fixed order: bitwise reproducible; a row's result does
 * not depend on the rows around it.
 * m355_dfine_query_pos_forward: out (N, H) = relu(ref (N, 4) @ weight (H, 4)^T + bias (H)), the first Linear + ReLU of query_pos_head.
 * m355_dfine_query_pos_backward: from grad_out and the forward's out (gradient 0 where out <= 0): grad_ref (N, 4), grad_weight (H, 4),
 *   grad_bias (H); each may be NULL and its work is skipped.  grad_weight / grad_bias are per-slab partial rows in work
 *   (m355_dfine_query_pos_workspace_bytes(N, H) bytes, every word written before it is read; 0 for a shape outside the limits),
 *   added in slab order by a second launch.
 * m355_dfine_refine_reference_forward: out = sigmoid(delta + log(max(x, eps) / max(1 - x, eps))), x = clamp(ref, 0, 1), on n
 *   elements: the reference points of layer 0.  _backward: grad_delta = grad_out * (1 - out) * out.  ONE launch each.
 * m355_dfine_refine_boxes_forward: delta, prev (N, 4 * num_bins_plus1), project (num_bins_plus1), points (N, 4) -> pred = delta +
 *   prev and boxes (N, 4) = distance2bbox(points, integral(pred, project), reg_scale) in ONE launch.  prev and pred NULL together:
 *   pred is delta and is not written.
 * m355_dfine_refine_boxes_backward: grad_corners (N, 4 * num_bins_plus1) = grad_pred (or 0 when NULL) + d boxes / d pred . grad_boxes,
 *   the gradient of delta and of prev alike; grad_points (N, 4) or NULL.  pred: the forward's pred (or delta).  ONE launch.
 * Limits (M355_ERR_INVALID before any HIP call): no NULL among the required pointers, 1 <= N <= 2^31, H a multiple of 4 in
 * [4, 2048], 1 <= n <= 2^38, eps >= 0, 2 <= num_bins_plus1 <= 64, reg_scale != 0, the workspace size, 16-byte alignment of every
 * tensor but project, boxes, grad_points and those of refine_reference. */
int m355_dfine_query_pos_forward(const float* d_ref, const float* d_weight, const float* d_bias, int64_t N, int32_t H, float* d_out,
                                 void* stream);
size_t m355_dfine_query_pos_workspace_bytes(int64_t N, int32_t H);
int m355_dfine_query_pos_backward(const float* d_grad_out, const float* d_out, const float* d_ref, const float* d_weight, int64_t N,
                                  int32_t H, float* d_grad_ref, float* d_grad_weight, float* d_grad_bias, void* d_work,
                                  int64_t work_bytes, void* stream);
int m355_dfine_refine_reference_forward(const float* d_delta, const float* d_ref, int64_t n, float eps, float* d_out, void* stream);
int m355_dfine_refine_reference_backward(const float* d_grad_out, const float* d_out, int64_t n, float* d_grad_delta, void* stream);
int m355_dfine_refine_boxes_forward(const float* d_delta, const float* d_prev, const float* d_project, const float* d_points, int64_t N,
                                    int32_t num_bins_plus1, float reg_scale, float* d_pred, float* d_boxes, void* stream);
int m355_dfine_refine_boxes_backward(const float* d_grad_pred, const float* d_grad_boxes, const float* d_pred, const float* d_project,
                                     const float* d_points, int64_t N, int32_t num_bins_plus1, float reg_scale, float* d_grad_corners,
                                     float* d_grad_points, void* stream);

/* ---- NCHW feature maps <-> token rows, and the exact GELU (the AIFI layer and the decoder's memory assembly) ----------------
 * transformers' DFineAIFILayer turns its map into tokens and back around one encoder layer whose MLP uses the exact (erf) GELU, and
 * DFineModel.forward concatenates the flattened levels and multiplies them by valid_mask.  All tensors fp32, contiguous,
 * asynchronous on `stream`; no atomics, one writer per element: bitwise reproducible, an image does not depend on its batch.
 * m355_dfine_maps_to_tokens: h_maps is a HOST array of num_levels device pointers, map l (B, D, h_l, w_l) with (h_l, w_l) =
 *   shapes_hw[2 l], shapes_hw[2 l + 1] (host) -> tokens (B, S, D), S = sum h_l w_l, tokens[b, start_l + y w_l + x, c] =
 *   map_l[b, c, y, x], in ONE launch for all levels.  With pos (S, D): extra = tokens + pos; with mask (S): extra =
 *   mask[s] * tokens, a true multiply (0 * inf is NaN, 0 * -x is -0); the maps are read once for both outputs.  pos and mask
 *   exclude each other and extra is NULL exactly when both are.
 * m355_dfine_tokens_to_maps: the adjoint, map_l[b, c, y, x] = tokens[b, s, c] (+ extra[b, s, c] (* mask[s])) in ONE launch; tokens
 *   or extra may be NULL (not both), mask only with extra.
 * m355_dfine_gelu_forward: out (n) = h * 0.5 * (1 + erf(h / sqrt(2))).  _backward: grad_h = grad_out * (Phi(h) + h phi(h)) from the
 *   saved input h.
 * Limits (M355_ERR_INVALID before any HIP call): no NULL among the required pointers (the map table's entries included),
 * 1 <= num_levels <= 8, B >= 1, D a multiple of 4 in [4, 1024], h, w >= 1, S < 2^31, a grid below 2^31 blocks, 1 <= n <= 2^40,
 * 16-byte alignment of every tensor but mask (4-byte). */
int m355_dfine_maps_to_tokens(const float* const* h_maps, const int32_t* shapes_hw, int32_t num_levels, int32_t B, int32_t D,
                              const float* d_pos, const float* d_mask, float* d_tokens, float* d_extra, void* stream);
int m355_dfine_tokens_to_maps(const float* d_tokens, const float* d_extra, const float* d_mask, const int32_t* shapes_hw,
                              int32_t num_levels, int32_t B, int32_t D, float* const* h_maps, void* stream);
int m355_dfine_gelu_forward(const float* d_h, int64_t n, float* d_out, void* stream);
int m355_dfine_gelu_backward(const float* d_grad_out, const float* d_h, int64_t n, float* d_grad_h, void* stream);

/* ---- The recurrence of the D-FINE trainer's context GRU -----------------------------------------------------------------
 * torch's one-layer nn.GRU(*, 256, batch_first, uni- or bidirectional) without its input projection: the caller's GEMM gives
 * gi = x cat(W_ih, W_ih_reverse)^T + b_ih for all steps and both directions; these entries run the serial chain.  Gate order
 * r, z, n;  a = W_hh h_{t-1} + b_hh;  r = s(gi_r + a_r), z = s(gi_z + a_z), n = tanh(gi_n + r a_n), h_t = (1 - z) n + z h_{t-1};
 * direction 1 walks t = S - 1 .. 0 with its own parameters.  All tensors contiguous fp32 on the device, 16-byte aligned;
 * asynchronous on `stream`; no float atomics: bitwise reproducible, and sequence b of a batch gives the bits of the same
 * sequence alone.  H = 256, D = directions.
 *
 * m355_dfine_gru_forward: gi (B, S, D 3H), w_hh (D, 3H, H), b_hh (D, 3H), h0 (D, B, H) or NULL (zeros) -> out (B, S, D H) =
 *   cat(forward, reverse) per step, h_n (D, B, H).  ONE launch for all B D chains: each chain runs on 8 workgroups that keep a
 *   32-unit slice of w_hh in registers and pass h_t to each other through `work`.  keep != 0 also stores r, z, n and a_n of
 *   every step in work for the backward (16 H bytes per step and chain); keep == 0 writes nothing beyond the exchange area.
 * m355_dfine_gru_backward: grad_out (B, S, D H), grad_h_n (D, B, H) or NULL, w_hh, h0 or NULL and out as in the forward, work as
 *   the keep != 0 forward left it -> grad_gi (B, S, D 3H), grad_an (B, S, D H), grad_h0 (D, B, H), every element written.  The
 *   gradient of a is grad_gi with its n-part replaced by grad_an; grad_w_hh[d] = sum_t grad_a[d]^T h_{t-1} and grad_b_hh are the
 *   caller's GEMM and column sum.  ONE launch, the same split.
 * work: m355_dfine_gru_workspace_bytes(B, S, H, D) bytes (S = 0 in this query, and only here: the size a keep == 0 forward
 *   needs); 0 for a shape outside the limits.  Its head is the exchange area, zeroed on `stream` by both entries; one buffer
 *   serves one call at a time.  status: one int32 the caller zeroes once.  A workgroup whose bounded wait for its chain's other
 *   workgroups runs out writes NaN to the rest of its outputs, ORs 1 (forward) or 2 (backward) into *status and returns; nothing
 *   else writes it and the library never reads it.
 * Limits, checked on the host before any HIP call (M355_ERR_INVALID): H == 256, D in {1, 2}, B in [1, 8] (the grid is 64 or 128
 *   workgroups, resident on any gfx950), S in [1, 2^24], no NULL among the required pointers, 16-byte alignment, the
 *   workspace size. */
size_t m355_dfine_gru_workspace_bytes(int32_t B, int64_t S, int32_t H, int32_t D);
int m355_dfine_gru_forward(const float* d_gi, const float* d_w_hh, const float* d_b_hh, const float* d_h0, int32_t B, int64_t S,
                           int32_t H, int32_t D, float* d_out, float* d_h_n, void* d_work, int64_t work_bytes, int32_t keep,
                           int32_t* d_status, void* stream);
int m355_dfine_gru_backward(const float* d_grad_out, const float* d_grad_h_n, const float* d_w_hh, const float* d_h0, const float* d_out,
                            int32_t B, int64_t S, int32_t H, int32_t D, float* d_grad_gi, float* d_grad_an, float* d_grad_h0,
                            void* d_work, int64_t work_bytes, int32_t* d_status, void* stream);

/* ---- The temporal head of the D-FINE trainers ------------------------------------------------------------------------------
 * What the trainers run between the temporal encoder / context GRU and the loss or the post-processing, besides the nn.Linear
 * heads: the guarded box decode, the frame fusion of the improved trainer, the guarded class logits, the no-object cross-entropy
 * of every frame and the frame-to-frame consistency loss.  All tensors contiguous fp32 on the device; asynchronous on `stream`;
 * no float atomics, every reduction in a fixed order: bitwise reproducible.  Every entry checks on the host before any HIP call
 * (M355_ERR_INVALID): no NULL among the required pointers, then the limits stated with it.
 *
 * m355_dfine_decode_guarded / _backward: m355_dfine_decode / _backward with the trainers' guards in the same kernel:
 *   nan_to_num(dist, 0, 1, 0) -> integral -> nan_to_num(distances, 0, 1, 0) -> distance2bbox [-> clamp(0, 1)] ->
 *   nan_to_num(boxes, 0.5, 1, 0) (nan, posinf, neginf).  Gradients as torch gives them: 0 into a replaced logit, 0 through a
 *   clamped or replaced box coordinate, nothing from a replaced distance.  Where no guard fires the bits are those of the
 *   unguarded entries.  Arguments and limits as there. */
int m355_dfine_decode_guarded(const float* d_dist, const float* d_project, const float* d_ref, float* d_boxes, int64_t n,
                              int32_t num_bins_plus1, float reg_scale, int32_t clamp01, void* stream);
int m355_dfine_decode_guarded_backward(const float* d_grad_boxes, const float* d_dist, const float* d_project, const float* d_ref,
                                       float* d_grad_dist, float* d_grad_ref, int64_t n, int32_t num_bins_plus1, float reg_scale,
                                       int32_t clamp01, void* stream);
/* m355_dfine_temporal_fuse_forward: fused (T, Q, D), scores (T, Q), context (T, Q, D) or NULL -> out (T, Q, D) =
 *   fused * w (+ context), w = softmax of scores over T; stats (2, Q) or NULL: the column's max and the log of its sum of
 *   exp(score - max), all the backward keeps.  ONE launch; a query column does not depend on the other columns of the call.
 * m355_dfine_temporal_fuse_backward: ONE launch, one block per column.  grad_fused = g * w and grad_scores =
 *   w * (dw - sum_t w * dw) with dw[t] = sum_d g * fused; each may be NULL, fused may be NULL without grad_scores.  The gradient
 *   of context is grad_out itself.
 * Limits: 1 <= T <= 1024, 1 <= D <= 1024, 1 <= Q <= 2^20.  D % 4 != 0 or a base that is not 16-byte aligned is handled by
 *   4-byte accesses. */
int m355_dfine_temporal_fuse_forward(const float* d_fused, const float* d_scores, const float* d_context, int32_t T, int32_t Q,
                                     int32_t D, float* d_out, float* d_stats, void* stream);
int m355_dfine_temporal_fuse_backward(const float* d_grad_out, const float* d_fused, const float* d_scores, const float* d_stats,
                                      int32_t T, int32_t Q, int32_t D, float* d_grad_fused, float* d_grad_scores, void* stream);
/* m355_dfine_guard_logits_forward: v = cls (rows, C1), plus anomaly (rows, C1 - 1) on all but the last column when it is given;
 *   out = nan_to_num(clamp(v, -bound, bound), nan = 0, posinf = bound, neginf = -bound).  One rounding per element: torch's bits.
 * m355_dfine_guard_logits_backward: grad_cls (rows, C1) and grad_anomaly (rows, C1 - 1), each may be NULL: grad_out where
 *   -bound <= v <= bound, 0 elsewhere (NaN, +-inf, clamped), which is torch's mask.  ONE launch each.
 * Limits: rows >= 1, C1 >= 1 (>= 2 with anomaly), rows * C1 <= 2^40, bound >= 0. */
int m355_dfine_guard_logits_forward(const float* d_cls, const float* d_anomaly, int64_t rows, int32_t C1, float bound, float* d_out,
                                    void* stream);
int m355_dfine_guard_logits_backward(const float* d_grad_out, const float* d_cls, const float* d_anomaly, int64_t rows, int32_t C1,
                                     float bound, float* d_grad_cls, float* d_grad_anomaly, void* stream);
/* m355_dfine_noobject_loss_forward: logits (T, Q, C1) -> out (T): the mean over q of logsumexp(logits[t, q]) - logits[t, q,
 *   class_index], which is F.cross_entropy(logits[t], full((Q,), class_index)), one block per frame.
 * m355_dfine_noobject_loss_backward: grad_out (T) -> grad_logits (T, Q, C1) = grad_out[t] / Q * (softmax - onehot); reads the
 *   logits alone.  ONE launch each.  Limits: T >= 1, 1 <= Q <= 2048, 1 <= C1 <= 1024, 0 <= class_index < C1. */
int m355_dfine_noobject_loss_forward(const float* d_logits, int32_t T, int32_t Q, int32_t C1, int32_t class_index, float* d_out,
                                     void* stream);
int m355_dfine_noobject_loss_backward(const float* d_grad_out, const float* d_logits, int32_t T, int32_t Q, int32_t C1,
                                      int32_t class_index, float* d_grad_logits, void* stream);
/* m355_dfine_consistency_loss_forward: a (T, N) -> out (1) = (1 / (T - 1)) sum_{t >= 1} mean((a[t] - a[t - 1])^2).  TWO launches:
 *   the partial sums of every (frame, chunk of 4096 elements) into work (m355_dfine_consistency_workspace_bytes(T, N) bytes,
 *   every word written before it is read), then one wave adds them in a fixed order that depends on the shape alone.
 * m355_dfine_consistency_loss_backward: grad_out (1), read on the device -> grad_a (T, N).  ONE launch.
 * Limits: 2 <= T, 1 <= N <= 2^27, T * N < 2^31. */
size_t m355_dfine_consistency_workspace_bytes(int32_t T, int64_t N);
int m355_dfine_consistency_loss_forward(const float* d_a, int32_t T, int64_t N, void* d_work, int64_t work_bytes, float* d_out,
                                        void* stream);
int m355_dfine_consistency_loss_backward(const float* d_grad_out, const float* d_a, int32_t T, int64_t N, float* d_grad_a,
                                         void* stream);

/* ---- The end of the D-FINE trainers' step: gradient clipping and the Adam / AdamW update ---------------------------------------
 * torch.nn.utils.clip_grad_norm_(params, max_norm) (2-norm) and the step of torch.optim.Adam / AdamW with their default flags,
 * over a whole list of fp32 tensors per launch.  The kernels work from a table of m355_dfine_optim_row, one row per tensor, which
 * the caller passes twice: h_table on the host, read and checked by the entry, and d_table, the same bytes on the device, read by
 * the kernels (the caller's asynchronous copy, ordered before the entry on `stream`).  A tensor of numel elements is
 * ceil(numel / M355_DFINE_OPTIM_CHUNK) chunks, one block each; chunk0 of a row is the number of chunks of the rows before it.
 * Asynchronous on `stream`; no float atomics, every sum in an order the table alone decides: bitwise reproducible.  Pointers
 * need 4-byte alignment only: a chunk whose pointers share their offset from 16 bytes is accessed 16 bytes at a time between a
 * head and a tail of at most 3 elements, any other chunk 4 bytes at a time.
 *
 * m355_dfine_grad_sumsq_launch: d_partials[c] = the sum of g^2 over chunk c, added in double and rounded once, every one of the
 *   table's chunks written.  ONE launch.
 *   Reads g and numel of the rows; partials_len >= the number of chunks.
 * m355_dfine_clip_scale_launch: d_norm (16 bytes, 8-byte aligned): the norm = sqrt(sum of the partials), summed in double in a
 *   fixed order, as float in d_norm[0]; c = min(1, max_norm / (norm + 1e-6)) (a NaN stays NaN) as float in d_norm[1] and as the
 *   double in bytes 8..15; then g = g c in place for every row, the product taken in double and rounded once.  TWO launches:
 *   one block for the norm, one block per chunk for the scaling (c == 1 gives every bit back).  d_partials as grad_sumsq left
 *   it for the same table.
 * m355_dfine_adam_launch: one step of every row, per element and in this order (torch 2.10's _multi_tensor_adam, one rounding per
 *   pass of it):  g' = g c (with d_partials: d_norm is written as by clip_scale and c applied here; g itself is not written);
 *   weight_decay != 0: mode ADAMW p *= decay, mode ADAM g' += weight_decay p;  m += (g' - m) one_minus_beta1;
 *   v = v beta2 + one_minus_beta2 g'^2;  p -= step_size * m / (sqrt(v) / bc2_sqrt + eps).  sqrt and the divisions are correctly
 *   rounded.  The caller computes the derived scalars in double: decay = 1 - lr weight_decay, step_size = lr / (1 - beta1^t),
 *   bc2_sqrt = sqrt(1 - beta2^t), with the row's own step count t.  ONE launch, TWO with d_partials (the norm block first).
 *   d_partials and d_norm come together or not at all; max_norm is ignored without them.
 * Every entry refuses on the host, before any HIP call (M355_ERR_INVALID): a NULL table (either copy) or output; a count outside
 *   [1, M355_DFINE_OPTIM_MAX_TENSORS]; a negative numel; a pointer that is not 4-byte aligned; a NULL among the pointers the
 *   entry uses (g; adam: p, g, m, v) in a row with numel > 0; a chunk0 that is not the sum before it; more chunks than
 *   2^31 - 1, which is what a launch can index, or none at all; partials_len below the number of chunks; d_norm not 8-byte aligned; a mode
 *   that is neither constant. */
#define M355_DFINE_OPTIM_CHUNK 4096
#define M355_DFINE_OPTIM_MAX_TENSORS 65536
#define M355_DFINE_OPTIM_ADAM 0
#define M355_DFINE_OPTIM_ADAMW 1
typedef struct {
  float* p;                 /* parameter, exp_avg and exp_avg_sq: read and written by adam alone */
  float* g;                 /* gradient: read by all three, written by clip_scale */
  float* m;
  float* v;
  int64_t numel;
  int32_t chunk0;
  float lr, weight_decay, beta1, beta2, eps;             /* the group's values, as torch holds them */
  float step_size, bc2_sqrt;                             /* of this tensor's step count */
  float one_minus_beta1, one_minus_beta2, decay;         /* rounded from double, as torch passes them to its kernels */
  int32_t reserved[3];
} m355_dfine_optim_row;     /* 96 bytes */
int m355_dfine_grad_sumsq_launch(const m355_dfine_optim_row* h_table, const m355_dfine_optim_row* d_table, int32_t count,
                                 float* d_partials, int64_t partials_len, void* stream);
int m355_dfine_clip_scale_launch(const m355_dfine_optim_row* h_table, const m355_dfine_optim_row* d_table, int32_t count,
                                 const float* d_partials, int64_t partials_len, float max_norm, float* d_norm, void* stream);
int m355_dfine_adam_launch(const m355_dfine_optim_row* h_table, const m355_dfine_optim_row* d_table, int32_t count, int32_t mode,
                           const float* d_partials, int64_t partials_len, float max_norm, float* d_norm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355YOLO_H_ */
