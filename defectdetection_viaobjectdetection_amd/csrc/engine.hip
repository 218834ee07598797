// libmi355yolo.so engine: YOLOv8-seg layer plan, weight upload (layouts: weight_pack.hip), workspace and the engine's C-ABI
// (include/mi355yolo.h; the per-op entries are in op_entries.hip).  Host-side C++; all arithmetic is in the HIP kernels here.
//
// Graph (upstream yolov8-seg.yaml as exercised by
// BscanBased/yolo8_seg_predict.py:5-8): every Concat is physical-zero-copy -- producers write their
// output at a channel offset of the consumer's NHWC buffer; C2f's split/concat is one buffer.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mi355yolo.h"
#include "common.h"
#include "switches.h"
#include "weight_pack.h"

using namespace m355;

thread_local std::string m355::g_err;

namespace {

struct Tensor {
  int H = 0, W = 0, C = 0;
  half_t* p = nullptr;  // (max_batch, H, W, C) fp16 NHWC
};

struct Slice {  // channel slice of a tensor
  int t = -1, off = 0, c = 0;
};

struct ConvLayer {
  m355_conv_info info{};
  int Kpad = 0, cout_pad = 0;
  half_t* w = nullptr;  // packed [cout_pad][Kpad]
  float* bias = nullptr;
  bool loaded = false;
  // fused group: logical convs that were merged into this physical conv (head first-layer fusion)
};

enum OpKind { OP_STEM, OP_CONV, OP_CONVT, OP_PHASE, OP_POOL, OP_UP, OP_DECODE, OP_ADOWN, OP_C2F32, OP_PAIR, OP_DWCONV, OP_PSA_ATTN };

// The kernel of an OP_CONV / OP_CONVT / OP_PHASE launch, chosen once at plan time (plan_route)
enum Route {
  R_IGEMM,    // im2col implicit GEMM (conv_igemm.hip) with channel tile Op::tile
  R_HALO,     // 3x3 stride 1: halo / wide / m32 kernel as conv3x3_halo_pick chooses (conv3x3_halo.hip)
  R_C32,      // 3x3 32 -> 32 (conv3x3_c32.hip)
  R_SLAB,     // 3x3 on narrow maps (conv3x3_small.hip)
  R_W1,       // 1x1, weights in registers (conv1x1_wreg.hip)
  R_PLANES,   // 3x3 row-slab kernel in single-conv mode (conv3x3_planes.hip)
  R_S2C32,    // 3x3/s2 (32 -> 64) + 1x1 (64 -> 64) on the patch kernel (conv3x3_s2c32.hip)
  R_S2C64,    // 3x3/s2 (64 -> 128) + 1x1 (128 -> 128), weights in registers (conv3x3_s2c64.hip)
  R_PROTOR,   // OP_PHASE + proto.cv3, weights in registers (proto_phase_wreg.hip)
};

struct Op {
  OpKind kind;
  int conv = -1;       // physical conv index (phys_)
  int conv2 = -1, conv3 = -1;   // OP_C2F32: Bottleneck.cv2 and C2f.cv2 (conv = Bottleneck.cv1); `in` = the [y0, y1] slice C2f.cv1 wrote
                                // OP_PAIR: conv = Bottleneck.cv1, conv2 = Bottleneck.cv2 in one launch (conv3x3_planes.hip); out2 = the hidden tensor of the two-launch fallback
  int shortcut = 0;
  int heads = 0;       // OP_PSA_ATTN: attention heads (conv = the attn.pe depthwise conv, in = the qkv tensor)
  Slice in, out, res;  // tensor slices
  Slice in2;           // upsample read-through: channels [0, in2.c) of `in` come from this half-resolution slice
  Slice out2;          // OP_ADOWN: second output (max-pooled half); `out` is the average-pooled half
  int out_ext = 0;     // 0: internal tensor; 1: raw head buffer (fp32, anchor offset); 2: protos (caller)
  int raw_off = 0;     // channel offset in raw buffer
  int level_off = 0;   // anchor offset of the level in the raw buffer
  int Hi = 0, Wi = 0;
  // measurement metadata (per image)
  char kernel[48] = {0};  // kernel family label, e.g. "conv_igemm<128x128,k3>"
  char layer[64] = {0};   // first logical layer name
  double flops = 0;       // algorithmic FLOPs per image (2*MACs; 0 for non-conv ops)
  double bytes = 0;       // algorithmic activation bytes per image (in + out + residual)
  double wbytes = 0;      // weight bytes (read once per launch)
  Route route = R_IGEMM;
  int tile = -1;          // im2col tile id: the launch of R_IGEMM, the run-time fallback of R_S2C32 / R_S2C64 / R_PROTOR
  int decode = 0;         // head output conv that also decodes its rows into the prediction tensor (no OP_DECODE launch)
  int headtail = 0;       // head output conv of a level that can run as conv + decode in one launch (head_tail.hip) when the raw maps are not kept
  int stemfuse = -1;      // >= 0: index of the stem op this launch also computes (conv_stem_s2c32.hip); that op is then skipped
  bool fused_away = false;
  // stream lanes (plan_lanes): lane 0 is the caller's stream, lanes >= 1 are engine-owned side streams
  int lane = 0;
  std::vector<int> wait_ops;   // ops on OTHER lanes whose completion event this op's stream waits for before the launch
  bool record = false;         // an op on another lane (or the end-of-forward join) waits for this op
};

// A physical conv = what one kernel launch computes.  Usually one logical conv; the three first-layer
// head convs of a level (cv2/cv3/cv4 .0) share their input and are fused into one launch.
struct PhysConv {
  std::vector<int> logical;  // indices into convs_
  int cin = 0, cout = 0, k = 1, stride = 1, act = 1, transposed = 0;
  int groups = 1;            // > 1: depthwise 3x3 (groups = cin = cout): w = [9][cout] fp16 (pack_dw3x3_weights), bias [cout]
  int composed = 0;          // 1: ConvTranspose(2x2,s2) -> Conv(3x3) composed into four 2x2 phase convs (proto)
  int l3 = -1;               // composed + this logical 1x1 conv (proto.cv3) applied in the same kernel's epilogue
  half_t* w2 = nullptr;      // its weights, fp16 [cout2][cin] in logical order, and bias
  float* bias2 = nullptr;
  int cout2 = 0;
  std::vector<float> h_wt, h_bt, h_w3, h_b3;   // host copies of the two logical convs until both are set
  int diag = 0;              // 1: block-diagonal fusion of 1x1 convs with different inputs (cin = sum of theirs)
  double macs_px = 0;        // algorithmic MACs per output pixel (diag: sum over the blocks, not cin * cout)
  int Kpad = 0, cout_pad = 0;
  half_t* w = nullptr;
  float* bias = nullptr;
  float* stem_w = nullptr;  // stem only: [27][cout] fp32
  // fragment-ordered copies of `w` for the weights-in-registers kernels (frag_pack below): wf = plain row order (conv1x1_wreg,
  // conv3x3_s2c64, c2f_c32's first conv, the row-slab kernels), wf2 = operand row order (c2f_c32's second conv); nullptr = not built
  half_t* wf = nullptr;
  half_t* wf2 = nullptr;
  int planes = 0;            // wf = the K-loop fragment order of the row-slab 3x3 kernels (planes_frag_pack)
};

}  // namespace

struct m355_engine {
  m355_model_desc desc{};
  PlanSwitches sw{};         // the M355_* switches of graph construction and planning, as read at create
  std::string err;
  std::vector<Tensor> tensors;
  std::vector<m355_conv_info> convs;   // logical convs (canonical order)
  std::vector<bool> conv_loaded;
  std::vector<int> conv_phys;          // logical -> physical
  std::vector<int> conv_phys_off;      // output-channel offset inside the physical conv
  std::vector<int> conv_phys_koff;     // input-channel (K) offset inside the physical conv (block-diagonal fusion)
  std::vector<PhysConv> phys;
  std::vector<Op> ops;
  int nc = 1, nm = 32, A = 0, n3 = 0, n4 = 0, n5 = 0;
  int proto_h = 0, proto_w = 0;
  float* raw = nullptr;      // (max_batch, A, 64+nc+nm) fp32
  half_t* zero = nullptr;    // zero page
  int* tileq = nullptr;      // tile queues of the persistent kernels, 4 ints per op (ConvArgs.tileq)
  void* nms_ws = nullptr;
  size_t nms_ws_bytes = 0;
  size_t ws_bytes = 0;
  double macs = 0;           // conv MACs per image
  int feat_in = -1;
  // stream lanes: independent branches of the graph (Proto + the stride-8 head level vs the rest of the neck and the
  // other head levels) are launched on two streams so that the tails / partial waves of one fill the other's gaps
  int nlanes = 1;
  std::vector<hipStream_t> side;      // lanes 1 .. nlanes-1
  std::vector<hipEvent_t> op_done;    // one per op with record == true (else nullptr)
  std::vector<int> lane_last;         // last op of every lane (joined into the caller's stream at the end of a forward)
  // sub-batches: the leading large-map ops run over `sub_batch` images at a time, so that a tensor (26-52 MB instead of
  // 105-210 MB at batch 32) is still in the 256 MiB Infinity Cache when its consumer reads it
  int sub_batch = 0, sub_ops = 0;
  // head output convs decode in their epilogue (all three levels, else none); the raw maps are then written only on request
  bool decode_fused = false;
  int headtail_n = 0;        // head levels eligible for head_tail.hip (3: the decode launch is skipped when the raw maps are not kept)
  bool headtail_active = false;   // decided per forward, for ALL three levels or none: every level passes head_tail_ok for this batch
  int keep_raw = 1;
  // profiling: HIP events around every op launch, recorded on the caller's stream (single lane while profiling)
  bool profiling = false;
  std::vector<hipEvent_t> ev_pool;   // 2 events per op per recorded forward
  size_t ev_used = 0;
  std::vector<int> ev_op;    // op index of every recorded event pair (ops fused into a neighbour record none)
  std::vector<double> op_ms;         // accumulated per-op milliseconds
  std::vector<long> op_cnt;

  int fail(int code, const std::string& m) {
    err = m;
    g_err = m;
    return code;
  }
};

namespace {

#define HIP_TRY(e, call)                                                                            \
  do {                                                                                              \
    hipError_t _st = (call);                                                                        \
    if (_st != hipSuccess)                                                                          \
      return (e)->fail(M355_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_st));           \
  } while (0)

int make_divisible(double x, int d) { return (int)ceil(x / d) * d; }

struct Builder {
  m355_engine* e;
  double depth, width;
  int maxc;
  int ch(int c) const { return make_divisible(std::min(c, maxc) * width, 8); }
  int rep(int n) const { return n > 1 ? std::max((int)lround(n * depth), 1) : n; }

  int tensor(int H, int W, int C) {
    Tensor t;
    t.H = H; t.W = W; t.C = C;
    e->tensors.push_back(t);
    return (int)e->tensors.size() - 1;
  }
  int logical(const std::string& name, int cin, int cout, int k, int s, int has_bn, int transposed, int act, int groups = 1) {
    m355_conv_info ci{};
    snprintf(ci.name, sizeof(ci.name), "%s", name.c_str());
    ci.cin = cin; ci.cout = cout; ci.k = k; ci.stride = s; ci.has_bn = has_bn; ci.transposed = transposed;
    ci.act = act; ci.groups = groups;
    e->convs.push_back(ci);
    e->conv_loaded.push_back(false);
    e->conv_phys.push_back(-1);
    e->conv_phys_off.push_back(0);
    e->conv_phys_koff.push_back(0);
    return (int)e->convs.size() - 1;
  }
  int phys_from(const std::vector<int>& logicals) {
    PhysConv p;
    p.logical = logicals;
    const m355_conv_info& c0 = e->convs[logicals[0]];
    p.cin = c0.cin; p.k = c0.k; p.stride = c0.stride; p.act = c0.act; p.transposed = c0.transposed; p.groups = c0.groups;
    int off = 0;
    for (int li : logicals) {
      e->conv_phys[li] = (int)e->phys.size();
      e->conv_phys_off[li] = off;
      off += e->convs[li].cout;
    }
    p.cout = off;
    p.macs_px = (double)(p.cin / p.groups) * p.cout * p.k * p.k;
    e->phys.push_back(p);
    return (int)e->phys.size() - 1;
  }
  // 1x1 convs with DIFFERENT inputs that sit side by side in one tensor, fused into one launch with a
  // block-diagonal weight matrix: rows = all outputs, K = all inputs, zeros off the diagonal blocks.
  int phys_diag(const std::vector<int>& logicals) {
    PhysConv p;
    p.logical = logicals;
    const m355_conv_info& c0 = e->convs[logicals[0]];
    p.k = 1; p.stride = 1; p.act = c0.act; p.transposed = 0; p.diag = 1;
    int off = 0, koff = 0;
    for (int li : logicals) {
      e->conv_phys[li] = (int)e->phys.size();
      e->conv_phys_off[li] = off;
      e->conv_phys_koff[li] = koff;
      off += e->convs[li].cout;
      koff += e->convs[li].cin;
      p.macs_px += (double)e->convs[li].cin * e->convs[li].cout;
    }
    p.cout = off;
    p.cin = koff;
    e->phys.push_back(p);
    return (int)e->phys.size() - 1;
  }
  void add_macs(const Op& op, const PhysConv& p) {
    const Tensor& ti = e->tensors[op.in.t];
    if (op.kind == OP_CONVT) {
      e->macs += (double)(2 * ti.H) * (2 * ti.W) * p.cin * p.cout;
    } else {
      const int Ho = (ti.H + 2 * (p.k / 2) - p.k) / p.stride + 1, Wo = (ti.W + 2 * (p.k / 2) - p.k) / p.stride + 1;
      e->macs += (double)Ho * Wo * p.macs_px;
    }
  }
  // Conv(+BN+SiLU) from slice `in` to slice `out`
  void conv(const std::string& name, Slice in, Slice out, int k, int s, Slice res = Slice(), Slice in2 = Slice()) {
    const int li = logical(name, in.c, out.c, k, s, 1, 0, 1);
    Op op{};
    op.kind = OP_CONV;
    op.conv = phys_from({li});
    op.in = in; op.out = out; op.res = res; op.in2 = in2;
    add_macs(op, e->phys[op.conv]);
    e->ops.push_back(op);
  }
  // one launch of an existing physical conv (logicals created by the caller, e.g. C3's cv2 || cv1 pair)
  void conv_phys(int phys, Slice in, Slice out, Slice res = Slice(), Slice in2 = Slice()) {
    Op op{};
    op.kind = OP_CONV;
    op.conv = phys;
    op.in = in; op.out = out; op.res = res; op.in2 = in2;
    add_macs(op, e->phys[op.conv]);
    e->ops.push_back(op);
  }
  // C2f: in -> out
  void c2f(const std::string& name, Slice in, Slice out, int n, bool shortcut, Slice up_src = Slice()) {
    const Tensor& ti = e->tensors[in.t];
    const int H = ti.H, W = ti.W;
    const int c = out.c / 2;
    const int cat = tensor(H, W, (2 + n) * c);
    conv(name + ".cv1", in, Slice{cat, 0, 2 * c}, 1, 1, Slice(), up_src);
    // (the launch has no run-time fallback -- t and y2 have no tensors -- so the kernel's 31-bit offset bounds (c2f_c32_ok) are
    // checked here for the largest batch the engine takes: s scale at 640 x 640 from 437 images on keeps the three-launch form)
    const long c2f_px = (long)e->desc.max_batch * H * W;
    const bool c2f_addr_ok = c2f_px * (2 + n) * c * 2 < (1L << 31) && c2f_px * e->tensors[out.t].C < (1L << 31);
    if (c == 32 && n == 1 && H % 8 == 0 && W % 16 == 0 && out.c == 64 && c2f_addr_ok && !e->sw.no_c2f32) {
      // the whole block body in one launch (c2f_c32.hip): t and y2 never reach HBM, no tensor for either
      const int la = logical(name + ".m.0.cv1", c, c, 3, 1, 1, 0, 1), lb = logical(name + ".m.0.cv2", c, c, 3, 1, 1, 0, 1);
      const int lc = logical(name + ".cv2", 3 * c, out.c, 1, 1, 1, 0, 1);
      Op op{};
      op.kind = OP_C2F32;
      op.conv = phys_from({la}); op.conv2 = phys_from({lb}); op.conv3 = phys_from({lc});
      op.in = Slice{cat, 0, 2 * c}; op.out = out; op.shortcut = shortcut ? 1 : 0;
      e->macs += (double)H * W * (2.0 * 9 * c * c + 3.0 * c * out.c);
      e->ops.push_back(op);
      return;
    }
    for (int j = 0; j < n; ++j) {
      const int tmp = tensor(H, W, c);
      const Slice src{cat, (1 + j) * c, c};
      if (bneck_pair_shape_ok(c, H, W) && !e->sw.no_pair) {
        // the whole Bottleneck in one launch, hidden tensor in LDS (conv3x3_planes.hip); `tmp` only serves the two-launch
        // fallback of a call the kernel's 31-bit buffer offsets cannot address
        const std::string mn = name + ".m." + std::to_string(j);
        const int la = logical(mn + ".cv1", c, c, 3, 1, 1, 0, 1), lb = logical(mn + ".cv2", c, c, 3, 1, 1, 0, 1);
        Op op{};
        op.kind = OP_PAIR;
        op.conv = phys_from({la}); op.conv2 = phys_from({lb});
        e->phys[op.conv].planes = e->phys[op.conv2].planes = 1;
        op.in = src; op.out = Slice{cat, (2 + j) * c, c}; op.out2 = Slice{tmp, 0, c};
        op.shortcut = shortcut ? 1 : 0;
        if (shortcut) op.res = src;
        e->macs += (double)H * W * 2.0 * 9 * c * c;
        e->ops.push_back(op);
        continue;
      }
      conv(name + ".m." + std::to_string(j) + ".cv1", src, Slice{tmp, 0, c}, 3, 1);
      conv(name + ".m." + std::to_string(j) + ".cv2", Slice{tmp, 0, c}, Slice{cat, (2 + j) * c, c}, 3, 1,
           shortcut ? src : Slice());
    }
    conv(name + ".cv2", Slice{cat, 0, (2 + n) * c}, out, 1, 1);
  }
};

// model.22 = Segment(nc, 32, npr) on the three feature tensors `feats` (channels fch): Detect branches, coefficient branch,
// Proto, decode.  Shared by the yolov8-seg and yolov9c-seg graphs.
int build_segment_head(m355_engine* e, Builder& b, const int feats[3], const int fch[3], const int npr) {
  const int nc = e->nc, nm = e->nm;
  const int H3 = e->tensors[feats[0]].H, W3 = e->tensors[feats[0]].W, H4 = e->tensors[feats[1]].H, W4 = e->tensors[feats[1]].W,
            H5 = e->tensors[feats[2]].H, W5 = e->tensors[feats[2]].W, H2 = 2 * H3, W2 = 2 * W3;
  const int hc2 = std::max(std::max(16, fch[0] / 4), 64);
  const int hc3 = std::max(fch[0], std::min(nc, 100));
  const int hc4 = std::max(fch[0] / 4, nm);
  e->n3 = H3 * W3; e->n4 = H4 * W4; e->n5 = H5 * W5;
  e->A = e->n3 + e->n4 + e->n5;
  const int lvl_off[3] = {0, e->n3, e->n3 + e->n4};
  // canonical logical order follows the upstream state dict: cv2.{l}.{0,1,2}, cv3.{l}.*, proto.*, cv4.{l}.*.
  // Physical fusion: cv2.l.0 + cv3.l.0 + cv4.l.0 share their input -> one launch with cout = hc2+hc3+hc4.
  int l_cv2[3][3], l_cv3[3][3], l_cv4[3][3];
  for (int l = 0; l < 3; ++l) {
    const std::string p = "model.22.cv2." + std::to_string(l);
    l_cv2[l][0] = b.logical(p + ".0", fch[l], hc2, 3, 1, 1, 0, 1);
    l_cv2[l][1] = b.logical(p + ".1", hc2, hc2, 3, 1, 1, 0, 1);
    l_cv2[l][2] = b.logical(p + ".2", hc2, 64, 1, 1, 0, 0, 0);
  }
  for (int l = 0; l < 3; ++l) {
    const std::string p = "model.22.cv3." + std::to_string(l);
    l_cv3[l][0] = b.logical(p + ".0", fch[l], hc3, 3, 1, 1, 0, 1);
    l_cv3[l][1] = b.logical(p + ".1", hc3, hc3, 3, 1, 1, 0, 1);
    l_cv3[l][2] = b.logical(p + ".2", hc3, nc, 1, 1, 0, 0, 0);
  }
  const int l_p1 = b.logical("model.22.proto.cv1", fch[0], npr, 3, 1, 1, 0, 1);
  const int l_pu = b.logical("model.22.proto.upsample", npr, npr, 2, 2, 0, 1, 0);
  const int l_p2 = b.logical("model.22.proto.cv2", npr, npr, 3, 1, 1, 0, 1);
  const int l_p3 = b.logical("model.22.proto.cv3", npr, nm, 1, 1, 1, 0, 1);
  for (int l = 0; l < 3; ++l) {
    const std::string p = "model.22.cv4." + std::to_string(l);
    l_cv4[l][0] = b.logical(p + ".0", fch[l], hc4, 3, 1, 1, 0, 1);
    l_cv4[l][1] = b.logical(p + ".1", hc4, hc4, 3, 1, 1, 0, 1);
    l_cv4[l][2] = b.logical(p + ".2", hc4, nm, 1, 1, 0, 0, 0);
  }
  auto add_conv_op = [&](const std::vector<int>& logicals, Slice in, Slice out, int out_ext, int raw_off,
                         int level_off, OpKind kind = OP_CONV) {
    Op op{};
    op.kind = kind;
    op.conv = b.phys_from(logicals);
    op.in = in; op.out = out; op.out_ext = out_ext; op.raw_off = raw_off; op.level_off = level_off;
    b.add_macs(op, e->phys[op.conv]);
    e->ops.push_back(op);
  };
  const int HW[3][2] = {{H3, W3}, {H4, W4}, {H5, W5}};
  const int* lane_plan = e->sw.lane_plan;   // stream lane of Proto and of the three head levels (plan_lanes)
  for (int l = 0; l < 3; ++l) {
    const size_t lvl_first = e->ops.size();
    const int hcat = b.tensor(HW[l][0], HW[l][1], hc2 + hc3 + hc4);
    const Slice f{feats[l], 0, fch[l]};
    add_conv_op({l_cv2[l][0], l_cv3[l][0], l_cv4[l][0]}, f, Slice{hcat, 0, hc2 + hc3 + hc4}, 0, 0, 0);
    // the three second convs write side by side into one tensor, so that the three 1x1 output convs (64 box bins,
    // nc classes, nm mask coefficients: different inputs) run as ONE launch with a block-diagonal weight matrix and
    // write a whole row of the raw head map
    const int ucat = b.tensor(HW[l][0], HW[l][1], hc2 + hc3 + hc4);
    add_conv_op({l_cv2[l][1]}, Slice{hcat, 0, hc2}, Slice{ucat, 0, hc2}, 0, 0, 0);
    add_conv_op({l_cv3[l][1]}, Slice{hcat, hc2, hc3}, Slice{ucat, hc2, hc3}, 0, 0, 0);
    add_conv_op({l_cv4[l][1]}, Slice{hcat, hc2 + hc3, hc4}, Slice{ucat, hc2 + hc3, hc4}, 0, 0, 0);
    {
      Op op{};
      op.kind = OP_CONV;
      op.conv = b.phys_diag({l_cv2[l][2], l_cv3[l][2], l_cv4[l][2]});
      op.in = Slice{ucat, 0, hc2 + hc3 + hc4};
      op.out = Slice{-1, 0, 64 + nc + nm};
      op.out_ext = 1; op.raw_off = 0; op.level_off = lvl_off[l];
      b.add_macs(op, e->phys[op.conv]);
      e->ops.push_back(op);
    }
    for (size_t i = lvl_first; i < e->ops.size(); ++i) e->ops[i].lane = lane_plan[1 + l];
  }
  const size_t proto_first = e->ops.size();
  {
    const bool fuse2 = !e->sw.no_protofuse && npr % 64 == 0;   // a channel tile (64 or 128) must lie inside one phase
    const bool fuse3 = fuse2 && npr == 128 && nm == 32 && !e->sw.no_protofuse3;
    const int pr1 = b.tensor(H3, W3, npr);
    add_conv_op({l_p1}, Slice{feats[0], 0, fch[0]}, Slice{pr1, 0, npr}, 0, 0, 0);
    if (!fuse2) {
      const int pr2 = b.tensor(H2, W2, npr), pr3 = b.tensor(H2, W2, npr);
      add_conv_op({l_pu}, Slice{pr1, 0, npr}, Slice{pr2, 0, npr}, 0, 0, 0, OP_CONVT);
      add_conv_op({l_p2}, Slice{pr2, 0, npr}, Slice{pr3, 0, npr}, 0, 0, 0);
      add_conv_op({l_p3}, Slice{pr3, 0, npr}, Slice{-1, 0, nm}, 2, 0, 0);
    } else {
      // ConvTranspose2d(2x2, s2, bias) has no activation, so upsample -> cv2's 3x3 conv is ONE linear map of the
      // 80x80 tensor: per output phase (py, px) a 2x2 convolution with composed weights (host, fp64).  4 taps instead
      // of 1 + 9 per output pixel, and the 160x160x128 intermediate (0.42 GB of HBM traffic at batch 32) is gone.
      // With 128 prototype channels a 128 x 128 tile holds every channel of its pixels, so proto.cv3 (1x1, 128 -> 32)
      // runs in the same kernel's epilogue and the 160x160x128 tensor is never written at all.
      Op op{};
      op.kind = OP_PHASE;
      PhysConv p;
      p.logical = {l_pu, l_p2};
      p.cin = npr; p.cout = npr; p.k = 2; p.stride = 1; p.act = 1; p.composed = 1;
      p.macs_px = 4.0 * (4.0 * npr) * npr;      // per LOW-resolution pixel: 4 phases x 4 taps x npr x npr
      if (fuse3) {
        p.logical.push_back(l_p3);
        p.l3 = l_p3;
        p.cout2 = nm;
        p.macs_px += 4.0 * npr * nm;
        e->conv_phys[l_p3] = (int)e->phys.size();
      }
      e->conv_phys[l_pu] = e->conv_phys[l_p2] = (int)e->phys.size();
      e->phys.push_back(p);
      op.conv = (int)e->phys.size() - 1;
      op.in = Slice{pr1, 0, npr};
      // the model's nominal MACs (upstream counts ConvT + 3x3 (+ 1x1)) stay in the whole-net figure
      e->macs += (double)(2 * H3) * (2 * W3) * npr * npr + (double)(2 * H3) * (2 * W3) * npr * npr * 9;
      if (fuse3) {
        op.out = Slice{-1, 0, nm};
        op.out_ext = 2;
        e->macs += (double)(2 * H3) * (2 * W3) * npr * nm;
        e->ops.push_back(op);
      } else {
        const int pr3 = b.tensor(H2, W2, npr);
        op.out = Slice{pr3, 0, npr};
        e->ops.push_back(op);
        add_conv_op({l_p3}, Slice{pr3, 0, npr}, Slice{-1, 0, nm}, 2, 0, 0);
      }
    }
  }
  for (size_t i = proto_first; i < e->ops.size(); ++i) e->ops[i].lane = lane_plan[0];
  {
    Op op{};
    op.kind = OP_DECODE;
    e->ops.push_back(op);
  }
  e->proto_h = H2; e->proto_w = W2;
  return 0;
}

// yolov9c-seg (SURVEY next row N4: the architecture /root/reference/BscanBased/yolo_seg_train.py:7 names).  GELAN blocks on
// the same conv kernels: RepNCSPELAN4 = 1x1 -> two (RepCSP -> 3x3) stages -> 1x1 over the zero-copy concat of all four
// parts; RepCSP = two 1x1 branches, one RepBottleneck (RepConvN arrives from the host as ONE merged 3x3 conv), 1x1;
// ADown = one pooling kernel (2x2 average, then 3x3 / s2 max on the second channel half) + a 3x3 / s2 and a 1x1 conv
// writing the two halves of the output; SPPELAN = SPPF's serial pooling between two 1x1 convs.
// Block structure and names: oracle/yolov9c_seg_oracle.py (exact published parameter counts), spec.py conv_specs_v9c.
struct V9cBuilder {
  m355_engine* e;
  Builder& b;
  // RepCSP(c1 -> c2) from slice `in` to slice `out`
  void repcsp(const std::string& name, Slice in, Slice out) {
    const Tensor& ti = e->tensors[in.t];
    const int c_ = out.c / 2;
    const int tmp = b.tensor(ti.H, ti.W, c_), mid = b.tensor(ti.H, ti.W, c_), cat = b.tensor(ti.H, ti.W, 2 * c_);
    b.conv(name + ".cv1", in, Slice{tmp, 0, c_}, 1, 1);
    b.conv(name + ".m.0.cv1", Slice{tmp, 0, c_}, Slice{mid, 0, c_}, 3, 1);                        // RepConvN, merged
    b.conv(name + ".m.0.cv2", Slice{mid, 0, c_}, Slice{cat, 0, c_}, 3, 1, Slice{tmp, 0, c_});     // + shortcut
    b.conv(name + ".cv2", in, Slice{cat, c_, c_}, 1, 1);
    b.conv(name + ".cv3", Slice{cat, 0, 2 * c_}, out, 1, 1);
  }
  void elan(const std::string& name, Slice in, Slice out, int c3, int c4, Slice up_src = Slice()) {
    const Tensor& ti = e->tensors[in.t];
    const int cat = b.tensor(ti.H, ti.W, c3 + 2 * c4);
    b.conv(name + ".cv1", in, Slice{cat, 0, c3}, 1, 1, Slice(), up_src);
    const int r1 = b.tensor(ti.H, ti.W, c4), r2 = b.tensor(ti.H, ti.W, c4);
    repcsp(name + ".cv2.0", Slice{cat, c3 / 2, c3 / 2}, Slice{r1, 0, c4});
    b.conv(name + ".cv2.1", Slice{r1, 0, c4}, Slice{cat, c3, c4}, 3, 1);
    repcsp(name + ".cv3.0", Slice{cat, c3, c4}, Slice{r2, 0, c4});
    b.conv(name + ".cv3.1", Slice{r2, 0, c4}, Slice{cat, c3 + c4, c4}, 3, 1);
    b.conv(name + ".cv4", Slice{cat, 0, c3 + 2 * c4}, out, 1, 1);
  }
  void adown(const std::string& name, Slice in, Slice out) {
    const Tensor& ti = e->tensors[in.t];
    const int ch = in.c / 2, co = out.c / 2;
    const int ta = b.tensor(ti.H - 1, ti.W - 1, ch), tm = b.tensor(ti.H / 2, ti.W / 2, ch);
    Op op{};
    op.kind = OP_ADOWN;
    op.in = in; op.out = Slice{ta, 0, ch}; op.out2 = Slice{tm, 0, ch};
    e->ops.push_back(op);
    b.conv(name + ".cv1", Slice{ta, 0, ch}, Slice{out.t, out.off, co}, 3, 2);
    b.conv(name + ".cv2", Slice{tm, 0, ch}, Slice{out.t, out.off + co, co}, 1, 1);
  }
};

int build_graph_v9c(m355_engine* e) {
  const m355_model_desc& d = e->desc;
  Builder b{e, 1.0, 1.0, 1024};
  V9cBuilder v{e, b};
  if (d.in_h % 32 || d.in_w % 32 || d.in_h < 64 || d.in_w < 64)
    return e->fail(M355_ERR_INVALID, "in_h/in_w must be multiples of 32, at least 64");
  if (d.nc < 1 || d.max_batch < 1) return e->fail(M355_ERR_INVALID, "nc and max_batch must be >= 1");
  e->nc = d.nc; e->nm = 32;
  const int H = d.in_h, W = d.in_w;
  const int H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4, H3 = H / 8, W3 = W / 8, H4 = H / 16, W4 = W / 16, H5 = H / 32, W5 = W / 32;
  // zero-copy concat buffers: cat11 = [up(x9), x6], cat14 = [up(x12), x4], cat17 = [x16, x12], cat20 = [x19, x9]
  const int cat11 = b.tensor(H4, W4, 512 + 512), cat14 = b.tensor(H3, W3, 512 + 512);
  const int cat17 = b.tensor(H4, W4, 256 + 512), cat20 = b.tensor(H5, W5, 512 + 512);
  const Slice x4{cat14, 512, 512}, x6{cat11, 512, 512}, x9{cat20, 512, 512}, x12{cat17, 256, 512};
  const int t0 = b.tensor(H1, W1, 64);
  {
    const int li = b.logical("model.0", 3, 64, 3, 2, 1, 0, 1);
    Op op{};
    op.kind = OP_STEM;
    op.conv = b.phys_from({li});
    op.out = Slice{t0, 0, 64};
    op.Hi = H; op.Wi = W;
    e->macs += (double)H1 * W1 * 64 * 27;
    e->ops.push_back(op);
  }
  const int t1 = b.tensor(H2, W2, 128), t2 = b.tensor(H2, W2, 256), t3 = b.tensor(H3, W3, 256), t5 = b.tensor(H4, W4, 512),
            t7 = b.tensor(H5, W5, 512), t8 = b.tensor(H5, W5, 512);
  b.conv("model.1", Slice{t0, 0, 64}, Slice{t1, 0, 128}, 3, 2);
  v.elan("model.2", Slice{t1, 0, 128}, Slice{t2, 0, 256}, 128, 64);
  v.adown("model.3", Slice{t2, 0, 256}, Slice{t3, 0, 256});
  v.elan("model.4", Slice{t3, 0, 256}, x4, 256, 128);
  v.adown("model.5", x4, Slice{t5, 0, 512});
  v.elan("model.6", Slice{t5, 0, 512}, x6, 512, 256);
  v.adown("model.7", x6, Slice{t7, 0, 512});
  v.elan("model.8", Slice{t7, 0, 512}, Slice{t8, 0, 512}, 512, 256);
  {
    const int sp = b.tensor(H5, W5, 4 * 256);                  // SPPELAN: cv1 -> three serial 5x5 max pools -> cv5
    b.conv("model.9.cv1", Slice{t8, 0, 512}, Slice{sp, 0, 256}, 1, 1);
    Op op{};
    op.kind = OP_POOL;
    op.in = Slice{sp, 0, 256};
    op.out = Slice{sp, 256, 3 * 256};
    e->ops.push_back(op);
    b.conv("model.9.cv5", Slice{sp, 0, 1024}, x9, 1, 1);
  }
  const bool upfuse = !e->sw.no_upfuse;
  auto up = [&](Slice src, Slice dst) {
    if (upfuse) return;
    Op op{};
    op.kind = OP_UP;
    op.in = src; op.out = dst;
    e->ops.push_back(op);
  };
  up(x9, Slice{cat11, 0, 512});
  v.elan("model.12", Slice{cat11, 0, 1024}, x12, 512, 256, upfuse ? x9 : Slice());
  up(x12, Slice{cat14, 0, 512});
  const int t15 = b.tensor(H3, W3, 256), t18 = b.tensor(H4, W4, 512), t21 = b.tensor(H5, W5, 512);
  v.elan("model.15", Slice{cat14, 0, 1024}, Slice{t15, 0, 256}, 256, 128, upfuse ? x12 : Slice());
  v.adown("model.16", Slice{t15, 0, 256}, Slice{cat17, 0, 256});
  v.elan("model.18", Slice{cat17, 0, 768}, Slice{t18, 0, 512}, 512, 256);
  v.adown("model.19", Slice{t18, 0, 512}, Slice{cat20, 0, 512});
  v.elan("model.21", Slice{cat20, 0, 1024}, Slice{t21, 0, 512}, 512, 256);
  const int feats[3] = {t15, t18, t21};
  const int fch[3] = {256, 512, 512};
  return build_segment_head(e, b, feats, fch, 256);
}

// model.24 = Detect(nc) of YOLOv5u (box-only, nm = 0): per level the two first 3x3 convs (cv2.l.0, cv3.l.0) share their input
// and run as one launch, the two second convs write side by side, and the two 1x1 output convs run as one block-diagonal launch
// writing whole raw rows of 64 + nc.  The decode launch turns them into prediction rows of 4 + nc.
int build_detect_head(m355_engine* e, Builder& b, const int feats[3], const int fch[3], const std::string& pre) {
  const int nc = e->nc;
  const int hc2 = std::max(std::max(16, fch[0] / 4), 64);
  const int hc3 = std::max(fch[0], std::min(nc, 100));
  int HW[3][2];
  for (int l = 0; l < 3; ++l) { HW[l][0] = e->tensors[feats[l]].H; HW[l][1] = e->tensors[feats[l]].W; }
  e->n3 = HW[0][0] * HW[0][1]; e->n4 = HW[1][0] * HW[1][1]; e->n5 = HW[2][0] * HW[2][1];
  e->A = e->n3 + e->n4 + e->n5;
  const int lvl_off[3] = {0, e->n3, e->n3 + e->n4};
  int l_cv2[3][3], l_cv3[3][3];
  for (int l = 0; l < 3; ++l) {
    const std::string p = pre + ".cv2." + std::to_string(l);
    l_cv2[l][0] = b.logical(p + ".0", fch[l], hc2, 3, 1, 1, 0, 1);
    l_cv2[l][1] = b.logical(p + ".1", hc2, hc2, 3, 1, 1, 0, 1);
    l_cv2[l][2] = b.logical(p + ".2", hc2, 64, 1, 1, 0, 0, 0);
  }
  for (int l = 0; l < 3; ++l) {
    const std::string p = pre + ".cv3." + std::to_string(l);
    l_cv3[l][0] = b.logical(p + ".0", fch[l], hc3, 3, 1, 1, 0, 1);
    l_cv3[l][1] = b.logical(p + ".1", hc3, hc3, 3, 1, 1, 0, 1);
    l_cv3[l][2] = b.logical(p + ".2", hc3, nc, 1, 1, 0, 0, 0);
  }
  const int lane_plan[3] = {1, 1, 0};   // the stride-8 and stride-16 levels beside the stride-32 level on the caller's stream
  for (int l = 0; l < 3; ++l) {
    const size_t lvl_first = e->ops.size();
    const int hcat = b.tensor(HW[l][0], HW[l][1], hc2 + hc3), ucat = b.tensor(HW[l][0], HW[l][1], hc2 + hc3);
    b.conv_phys(b.phys_from({l_cv2[l][0], l_cv3[l][0]}), Slice{feats[l], 0, fch[l]}, Slice{hcat, 0, hc2 + hc3});
    b.conv_phys(b.phys_from({l_cv2[l][1]}), Slice{hcat, 0, hc2}, Slice{ucat, 0, hc2});
    b.conv_phys(b.phys_from({l_cv3[l][1]}), Slice{hcat, hc2, hc3}, Slice{ucat, hc2, hc3});
    Op op{};
    op.kind = OP_CONV;
    op.conv = b.phys_diag({l_cv2[l][2], l_cv3[l][2]});
    op.in = Slice{ucat, 0, hc2 + hc3};
    op.out = Slice{-1, 0, 64 + nc};
    op.out_ext = 1; op.raw_off = 0; op.level_off = lvl_off[l];
    b.add_macs(op, e->phys[op.conv]);
    e->ops.push_back(op);
    for (size_t i = lvl_first; i < e->ops.size(); ++i) e->ops[i].lane = lane_plan[l];
  }
  Op op{};
  op.kind = OP_DECODE;
  e->ops.push_back(op);
  e->proto_h = e->proto_w = 0;
  return 0;
}

// C3(c1 -> c2, n, shortcut) of YOLOv5u in ONE buffer X = [m out | cv2 out | cv1 out] (3 c_ channels, c_ = c2 / 2): cv2 || cv1
// are one 1x1 launch into X[c_, 3 c_); the Bottleneck chain (1x1 then 3x3, + input when shortcut) reads X[2 c_:] and leaves its
// result in X[:c_] (ping-pong tensors in between for n > 1: a residual never aliases its own output); cv3 reads X[:2 c_], which is
// upstream's cat(m(cv1 x), cv2 x) without a copy.
void build_c3(m355_engine* e, Builder& b, const std::string& name, Slice in, Slice out, int n, bool shortcut, Slice up_src = Slice()) {
  const int H = e->tensors[in.t].H, W = e->tensors[in.t].W, c_ = out.c / 2;
  const int X = b.tensor(H, W, 3 * c_);
  const int l1 = b.logical(name + ".cv1", in.c, c_, 1, 1, 1, 0, 1);
  const int l2 = b.logical(name + ".cv2", in.c, c_, 1, 1, 1, 0, 1);
  const int l3 = b.logical(name + ".cv3", 2 * c_, out.c, 1, 1, 1, 0, 1);
  b.conv_phys(b.phys_from({l2, l1}), in, Slice{X, c_, 2 * c_}, Slice(), up_src);
  const int tmp = b.tensor(H, W, c_);
  int pp[2] = {-1, -1};
  if (n > 1) { pp[0] = b.tensor(H, W, c_); pp[1] = n > 2 ? b.tensor(H, W, c_) : -1; }
  Slice src{X, 2 * c_, c_};
  for (int j = 0; j < n; ++j) {
    const std::string mn = name + ".m." + std::to_string(j);
    const int la = b.logical(mn + ".cv1", c_, c_, 1, 1, 1, 0, 1), lb = b.logical(mn + ".cv2", c_, c_, 3, 1, 1, 0, 1);
    const Slice dst = j == n - 1 ? Slice{X, 0, c_} : Slice{pp[j & 1], 0, c_};
    b.conv_phys(b.phys_from({la}), src, Slice{tmp, 0, c_});
    b.conv_phys(b.phys_from({lb}), Slice{tmp, 0, c_}, dst, shortcut ? src : Slice());
    src = dst;
  }
  b.conv_phys(b.phys_from({l3}), Slice{X, 0, 2 * c_}, out);
}

// YOLOv5u (/root/reference/BscanBased/yolo5s_retrain.py:6 loads yolov5su.pt; upstream cfg/models/v5/yolov5.yaml with
// the anchor-free Detect head).  model.0 is the 6x6 / s2 / p2 stem (conv_stem6_s2.hip); every other conv goes through the planner's
// usual kernel rules.  Names and canonical order: spec.py conv_specs_v5u; block structure: tests/yolov5u_det_ref.py.
int build_graph_v5u(m355_engine* e) {
  const m355_model_desc& d = e->desc;
  Builder b{e, 0, 0, 1024};
  switch (d.scale & 0xff) {
    case 'n': b.depth = 0.33; b.width = 0.25; break;
    case 's': b.depth = 0.33; b.width = 0.50; break;
    case 'm': b.depth = 0.67; b.width = 0.75; break;
    default: return e->fail(M355_ERR_INVALID, "YOLOv5u scale must be n, s or m (l and x are not built)");
  }
  if (d.in_h % 32 || d.in_w % 32 || d.in_h < 64 || d.in_w < 64)
    return e->fail(M355_ERR_INVALID, "in_h/in_w must be multiples of 32, at least 64");
  if (d.nc < 1 || d.max_batch < 1) return e->fail(M355_ERR_INVALID, "nc and max_batch must be >= 1");
  e->nc = d.nc; e->nm = 0;
  const int c64 = b.ch(64), c128 = b.ch(128), c256 = b.ch(256), c512 = b.ch(512), c1024 = b.ch(1024);
  const int H = d.in_h, W = d.in_w;
  const int H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4, H3 = H / 8, W3 = W / 8, H4 = H / 16, W4 = W / 16, H5 = H / 32, W5 = W / 32;
  // zero-copy concat buffers: cat12 = [up(x10), x6], cat16 = [up(x14), x4], cat19 = [x18, x14], cat22 = [x21, x10]
  const int cat12 = b.tensor(H4, W4, 2 * c512), cat16 = b.tensor(H3, W3, 2 * c256);
  const int cat19 = b.tensor(H4, W4, 2 * c256), cat22 = b.tensor(H5, W5, 2 * c512);
  const Slice x4{cat16, c256, c256}, x6{cat12, c512, c512}, x10{cat22, c512, c512}, x14{cat19, c256, c256};
  const int t0 = b.tensor(H1, W1, c64);
  {
    const int li = b.logical("model.0", 3, c64, 6, 2, 1, 0, 1);
    Op op{};
    op.kind = OP_STEM;
    op.conv = b.phys_from({li});
    op.out = Slice{t0, 0, c64};
    op.Hi = H; op.Wi = W;
    e->macs += (double)H1 * W1 * c64 * 108;
    e->ops.push_back(op);
  }
  const int t1 = b.tensor(H2, W2, c128), t2 = b.tensor(H2, W2, c128), t3 = b.tensor(H3, W3, c256), t5 = b.tensor(H4, W4, c512),
            t7 = b.tensor(H5, W5, c1024), t8 = b.tensor(H5, W5, c1024), t9 = b.tensor(H5, W5, c1024);
  b.conv("model.1", Slice{t0, 0, c64}, Slice{t1, 0, c128}, 3, 2);
  build_c3(e, b, "model.2", Slice{t1, 0, c128}, Slice{t2, 0, c128}, b.rep(3), true);
  b.conv("model.3", Slice{t2, 0, c128}, Slice{t3, 0, c256}, 3, 2);
  build_c3(e, b, "model.4", Slice{t3, 0, c256}, x4, b.rep(6), true);
  b.conv("model.5", x4, Slice{t5, 0, c512}, 3, 2);
  build_c3(e, b, "model.6", Slice{t5, 0, c512}, x6, b.rep(9), true);
  b.conv("model.7", x6, Slice{t7, 0, c1024}, 3, 2);
  build_c3(e, b, "model.8", Slice{t7, 0, c1024}, Slice{t8, 0, c1024}, b.rep(3), true);
  {
    const int c_ = c1024 / 2;
    const int sp = b.tensor(H5, W5, 4 * c_);                   // SPPF: cv1 -> three serial 5x5 max pools -> cv2
    b.conv("model.9.cv1", Slice{t8, 0, c1024}, Slice{sp, 0, c_}, 1, 1);
    Op op{};
    op.kind = OP_POOL;
    op.in = Slice{sp, 0, c_};
    op.out = Slice{sp, c_, 3 * c_};
    e->ops.push_back(op);
    b.conv("model.9.cv2", Slice{sp, 0, 4 * c_}, Slice{t9, 0, c1024}, 1, 1);
  }
  b.conv("model.10", Slice{t9, 0, c1024}, x10, 1, 1);
  // 11/12 and 15/16: Upsample + Concat read through by the next C3's cv2 || cv1 (M355_NO_UPFUSE: materialised by upsample2x)
  const bool upfuse = !e->sw.no_upfuse;
  auto up = [&](Slice src, Slice dst) {
    if (upfuse) return;
    Op op{};
    op.kind = OP_UP;
    op.in = src; op.out = dst;
    e->ops.push_back(op);
  };
  const int t13 = b.tensor(H4, W4, c512), t17 = b.tensor(H3, W3, c256), t20 = b.tensor(H4, W4, c512), t23 = b.tensor(H5, W5, c1024);
  up(x10, Slice{cat12, 0, c512});
  build_c3(e, b, "model.13", Slice{cat12, 0, 2 * c512}, Slice{t13, 0, c512}, b.rep(3), false, upfuse ? x10 : Slice());
  b.conv("model.14", Slice{t13, 0, c512}, x14, 1, 1);
  up(x14, Slice{cat16, 0, c256});
  build_c3(e, b, "model.17", Slice{cat16, 0, 2 * c256}, Slice{t17, 0, c256}, b.rep(3), false, upfuse ? x14 : Slice());
  b.conv("model.18", Slice{t17, 0, c256}, Slice{cat19, 0, c256}, 3, 2);
  build_c3(e, b, "model.20", Slice{cat19, 0, 2 * c256}, Slice{t20, 0, c512}, b.rep(3), false);
  b.conv("model.21", Slice{t20, 0, c512}, Slice{cat22, 0, c512}, 3, 2);
  build_c3(e, b, "model.23", Slice{cat22, 0, 2 * c512}, Slice{t23, 0, c1024}, b.rep(3), false);
  const int feats[3] = {t17, t20, t23};
  const int fch[3] = {c256, c512, c1024};
  return build_detect_head(e, b, feats, fch, "model.24");
}

// One depthwise 3x3 launch (dwconv3x3.hip) of the logical conv li: in -> out, both channel slices
void dwconv_op(m355_engine* e, Builder& b, int li, Slice in, Slice out) {
  Op op{};
  op.kind = OP_DWCONV;
  op.conv = b.phys_from({li});
  op.in = in; op.out = out;
  b.add_macs(op, e->phys[op.conv]);
  e->ops.push_back(op);
}

// model.23 = Detect(nc) of YOLO11 (box-only, nm = 0).  Box branch as YOLOv8's; the class branch is DWConv 3x3 -> 1x1 ->
// DWConv 3x3 -> 1x1 (cv3.l.0.0 .. cv3.l.1.1), so cv2.l.0 no longer shares its launch with the class branch's first conv.  The
// two second stages write side by side and the two output 1x1 convs run as one block-diagonal launch writing raw rows of
// 64 + nc, as in build_detect_head.
int build_detect_head_y11(m355_engine* e, Builder& b, const int feats[3], const int fch[3], const std::string& pre) {
  const int nc = e->nc;
  const int hc2 = std::max(std::max(16, fch[0] / 4), 64);
  const int hc3 = std::max(fch[0], std::min(nc, 100));
  if (hc3 % 8)
    return e->fail(M355_ERR_INVALID, "YOLO11: the class branch width max(P3 channels, min(nc, 100)) must be a multiple of 8 "
                                     "(the depthwise kernel's 16-byte channel groups): n scale with nc in 65..100 not a multiple of 8");
  int HW[3][2];
  for (int l = 0; l < 3; ++l) { HW[l][0] = e->tensors[feats[l]].H; HW[l][1] = e->tensors[feats[l]].W; }
  e->n3 = HW[0][0] * HW[0][1]; e->n4 = HW[1][0] * HW[1][1]; e->n5 = HW[2][0] * HW[2][1];
  e->A = e->n3 + e->n4 + e->n5;
  const int lvl_off[3] = {0, e->n3, e->n3 + e->n4};
  int l_cv2[3][3], l_cv3[3][5];
  for (int l = 0; l < 3; ++l) {
    const std::string p = pre + ".cv2." + std::to_string(l);
    l_cv2[l][0] = b.logical(p + ".0", fch[l], hc2, 3, 1, 1, 0, 1);
    l_cv2[l][1] = b.logical(p + ".1", hc2, hc2, 3, 1, 1, 0, 1);
    l_cv2[l][2] = b.logical(p + ".2", hc2, 64, 1, 1, 0, 0, 0);
  }
  for (int l = 0; l < 3; ++l) {
    const std::string p = pre + ".cv3." + std::to_string(l);
    l_cv3[l][0] = b.logical(p + ".0.0", fch[l], fch[l], 3, 1, 1, 0, 1, fch[l]);
    l_cv3[l][1] = b.logical(p + ".0.1", fch[l], hc3, 1, 1, 1, 0, 1);
    l_cv3[l][2] = b.logical(p + ".1.0", hc3, hc3, 3, 1, 1, 0, 1, hc3);
    l_cv3[l][3] = b.logical(p + ".1.1", hc3, hc3, 1, 1, 1, 0, 1);
    l_cv3[l][4] = b.logical(p + ".2", hc3, nc, 1, 1, 0, 0, 0);
  }
  const int lane_plan[3] = {1, 1, 0};   // as build_detect_head
  for (int l = 0; l < 3; ++l) {
    const size_t lvl_first = e->ops.size();
    const int H = HW[l][0], W = HW[l][1];
    const int hb = b.tensor(H, W, hc2), ucat = b.tensor(H, W, hc2 + hc3);
    const int d0 = b.tensor(H, W, fch[l]), e0 = b.tensor(H, W, hc3), d1 = b.tensor(H, W, hc3);
    b.conv_phys(b.phys_from({l_cv2[l][0]}), Slice{feats[l], 0, fch[l]}, Slice{hb, 0, hc2});
    b.conv_phys(b.phys_from({l_cv2[l][1]}), Slice{hb, 0, hc2}, Slice{ucat, 0, hc2});
    dwconv_op(e, b, l_cv3[l][0], Slice{feats[l], 0, fch[l]}, Slice{d0, 0, fch[l]});
    b.conv_phys(b.phys_from({l_cv3[l][1]}), Slice{d0, 0, fch[l]}, Slice{e0, 0, hc3});
    dwconv_op(e, b, l_cv3[l][2], Slice{e0, 0, hc3}, Slice{d1, 0, hc3});
    b.conv_phys(b.phys_from({l_cv3[l][3]}), Slice{d1, 0, hc3}, Slice{ucat, hc2, hc3});
    Op op{};
    op.kind = OP_CONV;
    op.conv = b.phys_diag({l_cv2[l][2], l_cv3[l][4]});
    op.in = Slice{ucat, 0, hc2 + hc3};
    op.out = Slice{-1, 0, 64 + nc};
    op.out_ext = 1; op.raw_off = 0; op.level_off = lvl_off[l];
    b.add_macs(op, e->phys[op.conv]);
    e->ops.push_back(op);
    for (size_t i = lvl_first; i < e->ops.size(); ++i) e->ops[i].lane = lane_plan[l];
  }
  Op op{};
  op.kind = OP_DECODE;
  e->ops.push_back(op);
  e->proto_h = e->proto_w = 0;
  return 0;
}

// C3k2(c1 -> c2, c3k, e) of YOLO11 (shortcut on) in ONE buffer X = [cv1 out (2c) | m.0 out (c)], c = int(c2 e): C2f's
// zero-copy layout, cv2 reads X whole.  m.0 = Bottleneck(c, c, e=0.5): 3x3 c -> c/2, 3x3 c/2 -> c + its input; or, with c3k,
// C3k(c, c, n=2) in a buffer Y = [m out | cv2 out | cv1 out] (c/2 each) as build_c3, with two 3x3 -> 3x3 Bottlenecks.
void build_c3k2(m355_engine* e, Builder& b, const std::string& name, Slice in, Slice out, bool c3k, double ew, Slice up_src = Slice()) {
  const int H = e->tensors[in.t].H, W = e->tensors[in.t].W, c = (int)(out.c * ew);
  const int X = b.tensor(H, W, 3 * c);
  const int l1 = b.logical(name + ".cv1", in.c, 2 * c, 1, 1, 1, 0, 1);
  const int l2 = b.logical(name + ".cv2", 3 * c, out.c, 1, 1, 1, 0, 1);
  b.conv_phys(b.phys_from({l1}), in, Slice{X, 0, 2 * c}, Slice(), up_src);
  const Slice src{X, c, c}, dst{X, 2 * c, c};
  const std::string mn = name + ".m.0";
  if (!c3k) {
    const int h = c / 2;
    const int la = b.logical(mn + ".cv1", c, h, 3, 1, 1, 0, 1), lb = b.logical(mn + ".cv2", h, c, 3, 1, 1, 0, 1);
    const int tmp = b.tensor(H, W, h);
    b.conv_phys(b.phys_from({la}), src, Slice{tmp, 0, h});
    b.conv_phys(b.phys_from({lb}), Slice{tmp, 0, h}, dst, src);
  } else {
    const int c_ = c / 2;
    const int k1 = b.logical(mn + ".cv1", c, c_, 1, 1, 1, 0, 1), k2 = b.logical(mn + ".cv2", c, c_, 1, 1, 1, 0, 1);
    const int k3 = b.logical(mn + ".cv3", 2 * c_, c, 1, 1, 1, 0, 1);
    int la[2], lb[2];
    for (int j = 0; j < 2; ++j) {
      la[j] = b.logical(mn + ".m." + std::to_string(j) + ".cv1", c_, c_, 3, 1, 1, 0, 1);
      lb[j] = b.logical(mn + ".m." + std::to_string(j) + ".cv2", c_, c_, 3, 1, 1, 0, 1);
    }
    const int Y = b.tensor(H, W, 3 * c_), tmp = b.tensor(H, W, c_), mid = b.tensor(H, W, c_);
    b.conv_phys(b.phys_from({k2, k1}), src, Slice{Y, c_, 2 * c_});
    b.conv_phys(b.phys_from({la[0]}), Slice{Y, 2 * c_, c_}, Slice{tmp, 0, c_});
    b.conv_phys(b.phys_from({lb[0]}), Slice{tmp, 0, c_}, Slice{mid, 0, c_}, Slice{Y, 2 * c_, c_});
    b.conv_phys(b.phys_from({la[1]}), Slice{mid, 0, c_}, Slice{tmp, 0, c_});
    b.conv_phys(b.phys_from({lb[1]}), Slice{tmp, 0, c_}, Slice{Y, 0, c_}, Slice{mid, 0, c_});
    b.conv_phys(b.phys_from({k3}), Slice{Y, 0, 2 * c_}, dst);
  }
  b.conv_phys(b.phys_from({l2}), Slice{X, 0, 3 * c}, out);
}

// C2PSA(c1) of YOLO11 with one PSABlock, c = c1 / 2, heads = c / 64.  X = [a | b] is cv1's output; the block's result b2
// overwrites b in place (b's last readers, qkv and proj's residual, run before), so cv2 reads X = cat(a, b2) without a copy.
//   qkv (1x1, BN, no act) -> QKV;  OP_PSA_ATTN: O = attention + pe(v) (psa_attn.hip);  proj (1x1, no act) + b -> B1;
//   ffn.0 (1x1 + SiLU) -> F;  ffn.1 (1x1, no act) + B1 -> X[c:];  cv2 -> out.  The two residuals are epilogue adds.
void build_c2psa(m355_engine* e, Builder& b, const std::string& name, Slice in, Slice out) {
  const int H = e->tensors[in.t].H, W = e->tensors[in.t].W, c1 = in.c, c = c1 / 2;
  const std::string pre = name + ".m.0.";
  const int l_cv1 = b.logical(name + ".cv1", c1, 2 * c, 1, 1, 1, 0, 1), l_cv2 = b.logical(name + ".cv2", 2 * c, c1, 1, 1, 1, 0, 1);
  const int l_qkv = b.logical(pre + "attn.qkv", c, 2 * c, 1, 1, 1, 0, 0);
  const int l_proj = b.logical(pre + "attn.proj", c, c, 1, 1, 1, 0, 0);
  const int l_pe = b.logical(pre + "attn.pe", c, c, 3, 1, 1, 0, 0, c);
  const int l_f0 = b.logical(pre + "ffn.0", c, 2 * c, 1, 1, 1, 0, 1);
  const int l_f1 = b.logical(pre + "ffn.1", 2 * c, c, 1, 1, 1, 0, 0);
  const int X = b.tensor(H, W, 2 * c), QKV = b.tensor(H, W, 2 * c), O = b.tensor(H, W, c), B1 = b.tensor(H, W, c), F = b.tensor(H, W, 2 * c);
  b.conv_phys(b.phys_from({l_cv1}), in, Slice{X, 0, 2 * c});
  b.conv_phys(b.phys_from({l_qkv}), Slice{X, c, c}, Slice{QKV, 0, 2 * c});
  {
    Op op{};
    op.kind = OP_PSA_ATTN;
    op.conv = b.phys_from({l_pe});
    op.heads = c / 64;
    op.in = Slice{QKV, 0, 2 * c};
    op.out = Slice{O, 0, c};
    b.add_macs(op, e->phys[op.conv]);   // the pe conv; the two attention products are in the op table's FLOPs
    e->ops.push_back(op);
  }
  b.conv_phys(b.phys_from({l_proj}), Slice{O, 0, c}, Slice{B1, 0, c}, Slice{X, c, c});
  b.conv_phys(b.phys_from({l_f0}), Slice{B1, 0, c}, Slice{F, 0, 2 * c});
  b.conv_phys(b.phys_from({l_f1}), Slice{F, 0, 2 * c}, Slice{X, c, c}, Slice{B1, 0, c});
  b.conv_phys(b.phys_from({l_cv2}), Slice{X, 0, 2 * c}, out);
}

// YOLO11 (BscanBased/yolo/yolo_bbox_retrain.py trains yolo11n; upstream cfg/models/11/yolo11.yaml, Detect at
// model.23).  Depth 0.5: every repeated block has n = 1.  Names and canonical order: spec.py conv_specs_y11; block structure:
// tests/yolo11_det_ref.py.  The stem and every plain conv go through the planner's usual rules; the depthwise convs run on
// dwconv3x3.hip and the attention core on psa_attn.hip.
int build_graph_y11(m355_engine* e) {
  const m355_model_desc& d = e->desc;
  Builder b{e, 0.5, 0, 1024};
  bool c3k_all = false;    // upstream parse_model: every C3k2 of the m (l, x) scale uses C3k
  switch (d.scale & 0xff) {
    case 'n': b.width = 0.25; break;
    case 's': b.width = 0.50; break;
    case 'm': b.width = 1.00; b.maxc = 512; c3k_all = true; break;
    default: return e->fail(M355_ERR_INVALID, "YOLO11 scale must be n, s or m (l and x are not built)");
  }
  if (d.in_h % 32 || d.in_w % 32 || d.in_h < 64 || d.in_w < 64)
    return e->fail(M355_ERR_INVALID, "in_h/in_w must be multiples of 32, at least 64");
  if (d.nc < 1 || d.max_batch < 1) return e->fail(M355_ERR_INVALID, "nc and max_batch must be >= 1");
  e->nc = d.nc; e->nm = 0;
  const int c64 = b.ch(64), c128 = b.ch(128), c256 = b.ch(256), c512 = b.ch(512), c1024 = b.ch(1024);
  const int H = d.in_h, W = d.in_w;
  const int H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4, H3 = H / 8, W3 = W / 8, H4 = H / 16, W4 = W / 16, H5 = H / 32, W5 = W / 32;
  // zero-copy concat buffers: cat12 = [up(x10), x6], cat15 = [up(x13), x4], cat18 = [x17, x13], cat21 = [x20, x10]
  const int cat12 = b.tensor(H4, W4, c1024 + c512), cat15 = b.tensor(H3, W3, c512 + c512);
  const int cat18 = b.tensor(H4, W4, c256 + c512), cat21 = b.tensor(H5, W5, c512 + c1024);
  const Slice x4{cat15, c512, c512}, x6{cat12, c1024, c512}, x10{cat21, c512, c1024}, x13{cat18, c256, c512};
  const int t0 = b.tensor(H1, W1, c64);
  {
    const int li = b.logical("model.0", 3, c64, 3, 2, 1, 0, 1);
    Op op{};
    op.kind = OP_STEM;
    op.conv = b.phys_from({li});
    op.out = Slice{t0, 0, c64};
    op.Hi = H; op.Wi = W;
    e->macs += (double)H1 * W1 * c64 * 27;
    e->ops.push_back(op);
  }
  const int t1 = b.tensor(H2, W2, c128), t2 = b.tensor(H2, W2, c256), t3 = b.tensor(H3, W3, c256), t5 = b.tensor(H4, W4, c512),
            t7 = b.tensor(H5, W5, c1024), t8 = b.tensor(H5, W5, c1024), t9 = b.tensor(H5, W5, c1024);
  b.conv("model.1", Slice{t0, 0, c64}, Slice{t1, 0, c128}, 3, 2);
  build_c3k2(e, b, "model.2", Slice{t1, 0, c128}, Slice{t2, 0, c256}, c3k_all, 0.25);
  b.conv("model.3", Slice{t2, 0, c256}, Slice{t3, 0, c256}, 3, 2);
  build_c3k2(e, b, "model.4", Slice{t3, 0, c256}, x4, c3k_all, 0.25);
  b.conv("model.5", x4, Slice{t5, 0, c512}, 3, 2);
  build_c3k2(e, b, "model.6", Slice{t5, 0, c512}, x6, true, 0.5);
  b.conv("model.7", x6, Slice{t7, 0, c1024}, 3, 2);
  build_c3k2(e, b, "model.8", Slice{t7, 0, c1024}, Slice{t8, 0, c1024}, true, 0.5);
  {
    const int c_ = c1024 / 2;
    const int sp = b.tensor(H5, W5, 4 * c_);                   // SPPF: cv1 -> three serial 5x5 max pools -> cv2
    b.conv("model.9.cv1", Slice{t8, 0, c1024}, Slice{sp, 0, c_}, 1, 1);
    Op op{};
    op.kind = OP_POOL;
    op.in = Slice{sp, 0, c_};
    op.out = Slice{sp, c_, 3 * c_};
    e->ops.push_back(op);
    b.conv("model.9.cv2", Slice{sp, 0, 4 * c_}, Slice{t9, 0, c1024}, 1, 1);
  }
  build_c2psa(e, b, "model.10", Slice{t9, 0, c1024}, x10);
  // 11/12 and 14/15: Upsample + Concat read through by the next C3k2's cv1 (M355_NO_UPFUSE: materialised by upsample2x)
  const bool upfuse = !e->sw.no_upfuse;
  auto up = [&](Slice src, Slice dst) {
    if (upfuse) return;
    Op op{};
    op.kind = OP_UP;
    op.in = src; op.out = dst;
    e->ops.push_back(op);
  };
  const int t16 = b.tensor(H3, W3, c256), t19 = b.tensor(H4, W4, c512), t22 = b.tensor(H5, W5, c1024);
  up(x10, Slice{cat12, 0, c1024});
  build_c3k2(e, b, "model.13", Slice{cat12, 0, c1024 + c512}, x13, c3k_all, 0.5, upfuse ? x10 : Slice());
  up(x13, Slice{cat15, 0, c512});
  build_c3k2(e, b, "model.16", Slice{cat15, 0, c512 + c512}, Slice{t16, 0, c256}, c3k_all, 0.5, upfuse ? x13 : Slice());
  b.conv("model.17", Slice{t16, 0, c256}, Slice{cat18, 0, c256}, 3, 2);
  build_c3k2(e, b, "model.19", Slice{cat18, 0, c256 + c512}, Slice{t19, 0, c512}, c3k_all, 0.5);
  b.conv("model.20", Slice{t19, 0, c512}, Slice{cat21, 0, c512}, 3, 2);
  build_c3k2(e, b, "model.22", Slice{cat21, 0, c512 + c1024}, Slice{t22, 0, c1024}, true, 0.5);
  const int feats[3] = {t16, t19, t22};
  const int fch[3] = {c256, c512, c1024};
  return build_detect_head_y11(e, b, feats, fch, "model.23");
}

int build_graph(m355_engine* e) {
  const m355_model_desc& d = e->desc;
  if ((d.scale >> 8) == '5') return build_graph_v5u(e);
  if ((d.scale >> 8) == '1') return build_graph_y11(e);
  if ((d.scale >> 8) != 0) return e->fail(M355_ERR_INVALID, "unknown model family in the high byte of m355_model_desc.scale");
  if (d.scale == 'c') return build_graph_v9c(e);
  Builder b{e, 0, 0, 0};
  switch (d.scale) {
    case 'n': b.depth = 0.33; b.width = 0.25; b.maxc = 1024; break;
    case 's': b.depth = 0.33; b.width = 0.50; b.maxc = 1024; break;
    case 'm': b.depth = 0.67; b.width = 0.75; b.maxc = 768; break;
    case 'l': b.depth = 1.00; b.width = 1.00; b.maxc = 512; break;
    case 'x': b.depth = 1.00; b.width = 1.25; b.maxc = 512; break;
    default: return e->fail(M355_ERR_INVALID, "scale must be one of n,s,m,l,x (yolov8-seg) or c (yolov9c-seg)");
  }
  if (d.in_h % 32 || d.in_w % 32 || d.in_h < 32 || d.in_w < 32)
    return e->fail(M355_ERR_INVALID, "in_h/in_w must be positive multiples of 32");
  if (d.nc < 1 || d.max_batch < 1) return e->fail(M355_ERR_INVALID, "nc and max_batch must be >= 1");
  const int nc = d.nc, nm = 32;
  e->nc = nc; e->nm = nm;
  const int c64 = b.ch(64), c128 = b.ch(128), c256 = b.ch(256), c512 = b.ch(512), c1024 = b.ch(1024);
  const int H = d.in_h, W = d.in_w;
  const int H1 = H / 2, W1 = W / 2, H2 = H / 4, W2 = W / 4, H3 = H / 8, W3 = W / 8, H4 = H / 16, W4 = W / 16,
            H5 = H / 32, W5 = W / 32;
  if (c64 != 16 && c64 != 32 && c64 != 48 && c64 != 64 && c64 != 80)
    return e->fail(M355_ERR_INVALID, "unsupported stem width");

  // concat buffers (zero-copy): cat11=[up(x9), x6] cat14=[up(x12), x4] cat17=[x16, x12] cat20=[x19, x9]
  const int cat11 = b.tensor(H4, W4, c1024 + c512);
  const int cat14 = b.tensor(H3, W3, c512 + c256);
  const int cat17 = b.tensor(H4, W4, c256 + c512);
  const int cat20 = b.tensor(H5, W5, c512 + c1024);
  const Slice x4{cat14, c512, c256}, x6{cat11, c1024, c512}, x9{cat20, c512, c1024}, x12{cat17, c256, c512};

  // 0: stem
  const int t0 = b.tensor(H1, W1, c64);
  {
    const int li = b.logical("model.0", 3, c64, 3, 2, 1, 0, 1);
    Op op{};
    op.kind = OP_STEM;
    op.conv = b.phys_from({li});
    op.out = Slice{t0, 0, c64};
    op.Hi = H; op.Wi = W;
    e->macs += (double)H1 * W1 * c64 * 27;
    e->ops.push_back(op);
  }
  const int t1 = b.tensor(H2, W2, c128);
  b.conv("model.1", Slice{t0, 0, c64}, Slice{t1, 0, c128}, 3, 2);
  const int t2 = b.tensor(H2, W2, c128);
  b.c2f("model.2", Slice{t1, 0, c128}, Slice{t2, 0, c128}, b.rep(3), true);
  const int t3 = b.tensor(H3, W3, c256);
  b.conv("model.3", Slice{t2, 0, c128}, Slice{t3, 0, c256}, 3, 2);
  b.c2f("model.4", Slice{t3, 0, c256}, x4, b.rep(6), true);
  const int t5 = b.tensor(H4, W4, c512);
  b.conv("model.5", x4, Slice{t5, 0, c512}, 3, 2);
  b.c2f("model.6", Slice{t5, 0, c512}, x6, b.rep(6), true);
  const int t7 = b.tensor(H5, W5, c1024);
  b.conv("model.7", x6, Slice{t7, 0, c1024}, 3, 2);
  const int t8 = b.tensor(H5, W5, c1024);
  b.c2f("model.8", Slice{t7, 0, c1024}, Slice{t8, 0, c1024}, b.rep(3), true);
  // 9: SPPF
  {
    const int c_ = c1024 / 2;
    const int sp = b.tensor(H5, W5, 4 * c_);
    b.conv("model.9.cv1", Slice{t8, 0, c1024}, Slice{sp, 0, c_}, 1, 1);
    Op op{};
    op.kind = OP_POOL;
    op.in = Slice{sp, 0, c_};
    op.out = Slice{sp, c_, 3 * c_};
    e->ops.push_back(op);
    b.conv("model.9.cv2", Slice{sp, 0, 4 * c_}, x9, 1, 1);
  }
  // 10/11: Upsample(x9) + Concat with x6.  By default nothing is copied: model.12.cv1 (1x1) reads channels
  // [0, c1024) through its gather from the half-resolution x9 (upsample read-through, conv_igemm.hip); with
  // M355_NO_UPFUSE the upsample kernel materialises them in cat11 instead.
  const bool upfuse = !e->sw.no_upfuse;
  if (!upfuse) {
    Op op{};
    op.kind = OP_UP;
    op.in = x9;
    op.out = Slice{cat11, 0, c1024};
    e->ops.push_back(op);
  }
  b.c2f("model.12", Slice{cat11, 0, c1024 + c512}, x12, b.rep(3), false, upfuse ? x9 : Slice());
  if (!upfuse) {
    Op op{};
    op.kind = OP_UP;
    op.in = x12;
    op.out = Slice{cat14, 0, c512};
    e->ops.push_back(op);
  }
  const int t15 = b.tensor(H3, W3, c256);
  b.c2f("model.15", Slice{cat14, 0, c512 + c256}, Slice{t15, 0, c256}, b.rep(3), false, upfuse ? x12 : Slice());
  b.conv("model.16", Slice{t15, 0, c256}, Slice{cat17, 0, c256}, 3, 2);
  const int t18 = b.tensor(H4, W4, c512);
  b.c2f("model.18", Slice{cat17, 0, c256 + c512}, Slice{t18, 0, c512}, b.rep(3), false);
  b.conv("model.19", Slice{t18, 0, c512}, Slice{cat20, 0, c512}, 3, 2);
  const int t21 = b.tensor(H5, W5, c1024);
  b.c2f("model.21", Slice{cat20, 0, c512 + c1024}, Slice{t21, 0, c1024}, b.rep(3), false);

  // 22: Segment head
  const int feats[3] = {t15, t18, t21};
  const int fch[3] = {c256, c512, c1024};
  return build_segment_head(e, b, feats, fch, b.ch(256));
}

// A stride-2 backbone conv whose ONLY consumer is the 1x1 cv1 of the following C2f, with as many channels as one
// im2col channel tile holds (64 or 128) on both sides: the 1x1 runs in the conv kernel's epilogue through LDS and the
// conv's own output never goes to HBM (model.1 -> model.2.cv1 and model.3 -> model.4.cv1 for the s scale).
void fuse_conv_cv1(m355_engine* e) {
  if (e->sw.no_cvfuse) return;
  for (size_t i = 0; i < e->ops.size(); ++i) {
    Op& oi = e->ops[i];
    if (oi.kind != OP_CONV || oi.out_ext != 0 || oi.res.t >= 0 || oi.in2.t >= 0) continue;
    PhysConv& pi = e->phys[oi.conv];
    if (pi.k != 3 || pi.stride != 2 || pi.logical.size() != 1 || pi.diag || pi.composed || pi.l3 >= 0 || !pi.act) continue;
    const int C = pi.cout;
    if (C != 64 && C != 128) continue;
    const Tensor& to = e->tensors[oi.out.t];
    // the kernel needs the tile that holds every channel: the same rule annotate_ops applies
    if (conv_pick_tile(C, (long)e->desc.max_batch * to.H * to.W) != (C == 128 ? TILE_128x128 : TILE_64x128)) continue;
    int j = -1, readers = 0;
    for (size_t k = 0; k < e->ops.size(); ++k) {
      const Op& ok = e->ops[k];
      if (ok.in.t == oi.out.t || ok.in2.t == oi.out.t || ok.res.t == oi.out.t) {
        ++readers;
        j = (int)k;
      }
    }
    if (readers != 1 || j <= (int)i) continue;
    const Op& oj = e->ops[j];
    if (oj.kind != OP_CONV || oj.in.t != oi.out.t || oj.in.off != oi.out.off || oj.in.c != C || oj.in2.t >= 0 || oj.res.t >= 0 ||
        oj.out_ext != 0)
      continue;
    const PhysConv& pj = e->phys[oj.conv];
    if (pj.k != 1 || pj.stride != 1 || pj.logical.size() != 1 || pj.diag || pj.cout != C || pj.cin != C || !pj.act) continue;
    const int lj = pj.logical[0];
    pi.l3 = lj;
    pi.cout2 = C;
    pi.logical.push_back(lj);
    e->conv_phys[lj] = oi.conv;
    oi.out = oj.out;
    oi.lane = oj.lane;
    e->ops.erase(e->ops.begin() + j);
  }
}

// The three head output convs (block-diagonal 1x1, fp32 rows of 64 + nc + nm) decode their own rows when a 128-channel
// tile holds a whole row and 64 raw + 64 decoded rows fit the LDS stages.  All three levels or none: OP_DECODE is then
// not launched at all.
void fuse_decode(m355_engine* e) {
  if (!e->sw.decfuse) return;   // opt-in (M355_DECFUSE)
  const int wi = 64 + e->nc + e->nm, wo = 4 + e->nc + e->nm;
  if (wi > 128 || (wi + wo) * 64 * 4 > 65536) return;
  int n = 0;
  for (Op& op : e->ops)
    if (op.kind == OP_CONV && op.out_ext == 1 && e->phys[op.conv].diag && e->phys[op.conv].cout == wi && op.raw_off == 0) ++n;
  if (n != 3) return;
  for (Op& op : e->ops)
    if (op.kind == OP_CONV && op.out_ext == 1) op.decode = 1;
  e->decode_fused = true;
}

// Producers of op i in the current op order: earlier ops that write a tensor it reads; the decode reads the raw head map.
std::vector<int> op_producers(const m355_engine* e, int i) {
  const Op& op = e->ops[i];
  std::vector<int> r;
  for (int j = 0; j < i; ++j) {
    const Op& q = e->ops[j];
    if (op.kind == OP_DECODE) {
      if (q.out_ext == 1) r.push_back(j);
      continue;
    }
    if (q.out_ext != 0 || q.out.t < 0) continue;
    auto reads = [&](int t) { return t == op.in.t || (op.in2.t >= 0 && t == op.in2.t) || (op.res.t >= 0 && t == op.res.t); };
    if (reads(q.out.t) || (q.kind == OP_ADOWN && reads(q.out2.t))) r.push_back(j);
  }
  return r;
}

// Sub-batched segment: the leading ops (stem, the stride-2 convs, the 160x160 and 80x80 C2f stages) while they are plain
// convs on the caller's lane whose output map is at least 1/8 of the input.  M355_SUBBATCH = images per pass (default 0: off),
// M355_SUBBATCH_OPS = number of leading ops.
void plan_sub_batches(m355_engine* e) {
  e->sub_batch = e->sw.subbatch;
  if (e->sub_batch <= 0 || e->sw.no_subbatch) { e->sub_batch = 0; return; }
  int n = 0;
  for (const Op& op : e->ops) {
    if ((op.kind != OP_STEM && op.kind != OP_CONV && op.kind != OP_C2F32 && op.kind != OP_PAIR) || op.lane != 0 || op.record || !op.wait_ops.empty() || op.out_ext != 0) break;
    const Tensor& to = e->tensors[op.out.t];
    if (to.H * 8 < e->desc.in_h) break;
    ++n;
  }
  e->sub_ops = std::min(n, e->sw.subbatch_ops);
}

// Stream lanes.  The builder tags the ops of Proto and of the stride-8 head level with lane 1; everything else is
// lane 0 (the caller's stream).  (1) Reorder: a lane-1 op moves to right after the last lane-0 op it depends on, so the
// host enqueues it as early as the data allows (lane order is kept, so the result is still a topological order).
// (2) Cross-lane dependencies become event waits; the last op of every side lane is joined into the caller's stream.
int plan_lanes(m355_engine* e) {
  if (e->sw.no_lanes) {
    for (Op& op : e->ops) op.lane = 0;
    return 0;
  }
  const int n = (int)e->ops.size();
  int nl = 1;
  for (const Op& op : e->ops) nl = std::max(nl, op.lane + 1);
  if (nl == 1) return 0;
  std::vector<int> ready(n, -1);          // side-lane op: index (old order) of its last lane-0 producer
  for (int i = 0; i < n; ++i) {
    if (e->ops[i].lane == 0) continue;
    for (int p : op_producers(e, i))
      if (e->ops[p].lane == 0) ready[i] = std::max(ready[i], p);
  }
  std::vector<Op> order;
  std::vector<int> pending;               // side-lane ops in their original order
  for (int i = 0; i < n; ++i)
    if (e->ops[i].lane != 0) pending.push_back(i);
  size_t pi = 0;
  int run_ready = -1;                     // a side op also waits for the side ops before it: running maximum
  for (int i = 0; i < n; ++i) {
    if (e->ops[i].lane != 0) continue;
    order.push_back(e->ops[i]);
    while (pi < pending.size()) {
      run_ready = std::max(run_ready, ready[pending[pi]]);
      if (run_ready > i) break;
      order.push_back(e->ops[pending[pi++]]);
    }
  }
  while (pi < pending.size()) order.push_back(e->ops[pending[pi++]]);
  e->ops.swap(order);
  e->lane_last.assign(nl, -1);
  for (int i = 0; i < n; ++i) {
    Op& op = e->ops[i];
    e->lane_last[op.lane] = i;
    std::vector<int> latest(nl, -1);      // stream order covers the earlier ops of a lane: wait for the latest only
    for (int p : op_producers(e, i))
      if (e->ops[p].lane != op.lane) latest[e->ops[p].lane] = std::max(latest[e->ops[p].lane], p);
    for (int l = 0; l < nl; ++l)
      if (latest[l] >= 0) {
        op.wait_ops.push_back(latest[l]);
        e->ops[latest[l]].record = true;
      }
  }
  for (int l = 1; l < nl; ++l)
    if (e->lane_last[l] >= 0) e->ops[e->lane_last[l]].record = true;
  e->op_done.assign(n, nullptr);
  for (int i = 0; i < n; ++i)
    if (e->ops[i].record) HIP_TRY(e, hipEventCreateWithFlags(&e->op_done[i], hipEventDisableTiming));
  e->side.assign(nl - 1, nullptr);
  for (int l = 1; l < nl; ++l) HIP_TRY(e, hipStreamCreateWithFlags(&e->side[l - 1], hipStreamNonBlocking));
  e->nlanes = nl;
  return 0;
}

int alloc_all(m355_engine* e) {
  const size_t B = (size_t)e->desc.max_batch;
  size_t total = 0;
  for (Tensor& t : e->tensors) {
    const size_t bytes = B * t.H * t.W * t.C * sizeof(half_t);
    HIP_TRY(e, hipMalloc((void**)&t.p, bytes));
    total += bytes;
  }
  const size_t raw_bytes = B * e->A * (64 + e->nc + e->nm) * sizeof(float);
  HIP_TRY(e, hipMalloc((void**)&e->raw, raw_bytes));
  total += raw_bytes;
  HIP_TRY(e, hipMalloc((void**)&e->zero, 4096));
  HIP_TRY(e, hipMemset(e->zero, 0, 4096));
  HIP_TRY(e, hipMalloc((void**)&e->tileq, (e->ops.size() + 1) * 16));   // one tile queue (ConvArgs.tileq) per op
  HIP_TRY(e, hipMemset(e->tileq, 0, (e->ops.size() + 1) * 16));
  e->nms_ws_bytes = nms_workspace_bytes((int)B, e->A);
  HIP_TRY(e, hipMalloc(&e->nms_ws, e->nms_ws_bytes));
  total += e->nms_ws_bytes + 4096;
  for (PhysConv& p : e->phys) {
    if (p.groups > 1) {   // depthwise 3x3: [9][C] fp16 + fp32 bias
      HIP_TRY(e, hipMalloc((void**)&p.w, (size_t)9 * p.cout * sizeof(half_t)));
      HIP_TRY(e, hipMalloc((void**)&p.bias, p.cout * sizeof(float)));
      total += (size_t)p.cout * (9 * sizeof(half_t) + sizeof(float));
      continue;
    }
    if (p.cin == 3 && p.k == 6) {   // YOLOv5u stem: [C0][128] fp16 in the kernel's row order + fp32 bias
      HIP_TRY(e, hipMalloc((void**)&p.w, (size_t)p.cout * 128 * sizeof(half_t)));
      HIP_TRY(e, hipMalloc((void**)&p.bias, p.cout * sizeof(float)));
      total += (size_t)p.cout * (128 * sizeof(half_t) + sizeof(float));
      continue;
    }
    const bool stem = (p.cin == 3);
    if (stem) {
      HIP_TRY(e, hipMalloc((void**)&p.stem_w, 27 * p.cout * sizeof(float)));
      HIP_TRY(e, hipMalloc((void**)&p.bias, p.cout * sizeof(float)));
      total += 28 * p.cout * sizeof(float);
      continue;
    }
    const int cout_v = (p.transposed || p.composed) ? 4 * p.cout : p.cout;  // virtual channels of the GEMM
    p.cout_pad = conv_cout_pad(cout_v);
    p.Kpad = p.transposed ? conv_kpad(p.cin, 1) : conv_kpad(p.cin, p.k);
    const size_t wb = (size_t)p.cout_pad * p.Kpad * sizeof(half_t);
    HIP_TRY(e, hipMalloc((void**)&p.w, wb));
    HIP_TRY(e, hipMemset(p.w, 0, wb));
    if (p.l3 >= 0) {
      HIP_TRY(e, hipMalloc((void**)&p.w2, (size_t)p.cout2 * p.cout * sizeof(half_t)));   // K of the 1x1 = p.cout
      HIP_TRY(e, hipMalloc((void**)&p.bias2, (size_t)p.cout2 * sizeof(float)));
    }
    const size_t nbias = p.composed ? (size_t)9 * p.cout : (size_t)p.cout_pad;   // composed: [9 border classes][cout]
    HIP_TRY(e, hipMalloc((void**)&p.bias, nbias * sizeof(float)));
    HIP_TRY(e, hipMemset(p.bias, 0, nbias * sizeof(float)));
    total += wb + p.cout_pad * sizeof(float);
  }
  e->ws_bytes = total;
  return 0;
}

// ---- launch arguments of an op over images [b0, b0 + B): one builder per argument struct, shared by the plan (B = max_batch,
// b0 = 0, no caller buffers yet) and the forward
ConvArgs conv_args(const m355_engine* e, const Op& op, int B, int b0, float* preds, void* protos) {
  const PhysConv& p = e->phys[op.conv];
  const Tensor& ti = e->tensors[op.in.t];
  ConvArgs a{};
  a.x_bstride = (long)ti.H * ti.W * ti.C; a.ldx = ti.C; a.x = ti.p + op.in.off + b0 * a.x_bstride;
  a.Hi = ti.H; a.Wi = ti.W; a.Cin = p.cin;
  a.w = p.w; a.Kpad = p.Kpad; a.bias = p.bias; a.wf = p.wf; a.zero = e->zero; a.act = p.act;
  if (op.kind == OP_CONV) {
    a.ksize = p.k; a.stride = p.stride; a.pad = p.k / 2;
    a.Ho = (ti.H + 2 * a.pad - p.k) / p.stride + 1;
    a.Wo = (ti.W + 2 * a.pad - p.k) / p.stride + 1;
    a.Cout = p.cout;
  } else {   // OP_CONVT: one 1x1 GEMM onto 4 cout virtual channels; OP_PHASE: four 2x2 phase convs (compose_proto_phases)
    a.ksize = op.kind == OP_PHASE ? 2 : 1; a.stride = 1; a.pad = 0; a.phase = op.kind == OP_PHASE;
    a.Ho = ti.H; a.Wo = ti.W; a.Cout = 4 * p.cout; a.convt_co = p.cout;
  }
  if (op.out_ext == 1) {   // raw head rows (external outputs are never in the sub-batched segment: b0 = 0)
    const int rw = 64 + e->nc + e->nm;
    a.y = e->raw + (long)op.level_off * rw + op.raw_off;
    a.y_bstride = (long)e->A * rw; a.ldy = rw; a.out_f32 = 1;
  } else if (op.out_ext == 2) {
    a.y = protos; a.y_bstride = (long)e->proto_h * e->proto_w * e->nm; a.ldy = e->nm;
  } else {
    const Tensor& to = e->tensors[op.out.t];
    a.y_bstride = (long)to.H * to.W * to.C; a.ldy = to.C; a.y = to.p + op.out.off + b0 * a.y_bstride;
  }
  if (op.in2.t >= 0) {   // Upsample + Concat read through
    const Tensor& t2 = e->tensors[op.in2.t];
    a.x2_bstride = (long)t2.H * t2.W * t2.C; a.ldx2 = t2.C; a.csplit = op.in2.c; a.x2 = t2.p + op.in2.off + b0 * a.x2_bstride;
  }
  if (op.res.t >= 0) {
    const Tensor& tr = e->tensors[op.res.t];
    a.r_bstride = (long)tr.H * tr.W * tr.C; a.ldr = tr.C; a.res = tr.p + op.res.off + b0 * a.r_bstride;
  }
  a.M = B * a.Ho * a.Wo;
  if (op.decode) {
    a.dec_preds = preds; a.dec_A = e->A; a.dec_level_off = op.level_off; a.dec_nc = e->nc; a.dec_nm = e->nm;
    a.dec_keep_raw = e->keep_raw; a.dec_stride = (float)(e->desc.in_h / a.Ho);
  }
  if (p.l3 >= 0) { a.w2 = p.w2; a.bias2 = p.bias2; a.cout2 = p.cout2; a.wf2 = p.wf2; }   // the 1x1 conv in this launch's epilogue
  return a;
}

// row-slab kernels (conv3x3_planes.hip): OP_PAIR, or one OP_CONV in single-conv mode (its conv in the second slot)
PlanesArgs planes_args(const m355_engine* e, const Op& op, int B, int b0) {
  const PhysConv& pa = e->phys[op.conv];
  const PhysConv& pb = e->phys[op.kind == OP_PAIR ? op.conv2 : op.conv];
  const Tensor& ti = e->tensors[op.in.t];
  const Tensor& to = e->tensors[op.out.t];
  PlanesArgs a{};
  a.x_bstride = (long)ti.H * ti.W * ti.C; a.ldx = ti.C; a.x = ti.p + op.in.off + b0 * a.x_bstride;
  a.H = ti.H; a.W = ti.W; a.B = B; a.Cin = pa.cin; a.Cout = pb.cout; a.act = pb.act; a.stride = pb.stride;
  if (op.kind == OP_PAIR) { a.wfa = pa.wf; a.cblocks_a = planes_cblocks(pa.cout); a.ba = pa.bias; }
  a.wfb = pb.wf; a.cblocks_b = planes_cblocks(pb.cout); a.bb = pb.bias;
  a.y_bstride = (long)to.H * to.W * to.C; a.ldy = to.C; a.y = to.p + op.out.off + b0 * a.y_bstride;
  if (op.res.t >= 0) {   // (a Bottleneck pair's shortcut is its input slice)
    const Tensor& tr = e->tensors[op.res.t];
    a.r_bstride = (long)tr.H * tr.W * tr.C; a.ldr = tr.C; a.res = tr.p + op.res.off + b0 * a.r_bstride;
  }
  return a;
}

StemArgs stem_args(const m355_engine* e, const Op& op, int B, int b0, const void* in) {
  const PhysConv& p = e->phys[op.conv];
  const Tensor& to = e->tensors[op.out.t];
  StemArgs a{};
  a.x = (const uint8_t*)in + (long)b0 * op.Hi * op.Wi * 3; a.B = B; a.H = op.Hi; a.W = op.Wi;
  a.w16 = (const half_t*)p.stem_w; a.bias = p.bias;
  a.y_bstride = (long)to.H * to.W * to.C; a.ldy = to.C; a.Cout = p.cout;
  a.y = to.p + op.out.off + b0 * a.y_bstride;
  return a;
}

// (a head level runs on head_tail.hip over whole batches only: b0 = 0)
HeadTailArgs head_tail_args(const m355_engine* e, const Op& op, int B, float* preds) {
  const PhysConv& p = e->phys[op.conv];
  const Tensor& ti = e->tensors[op.in.t];
  HeadTailArgs a{};
  a.x = ti.p; a.ldx = ti.C; a.M = (long)B * ti.H * ti.W; a.HW = ti.H * ti.W; a.W = ti.W;
  a.stride = (float)(e->desc.in_h / ti.H);
  a.A = e->A; a.level_off = op.level_off; a.nc = e->nc; a.nm = e->nm;
  a.wf = p.wf; a.bias = p.bias; a.preds = preds;
  return a;
}

// A head level's block-diagonal 1x1 in the layout head_tail.hip takes: box 64 <- 64, class nc <- 128, coefficient 32 <- 32
bool head_tail_layout(const m355_engine* e, const PhysConv& p) {
  return p.diag && p.logical.size() == 3 && p.cin == 224 && p.cout == 64 + e->nc + e->nm && e->nm == 32 && e->nc <= 32 &&
         e->convs[p.logical[0]].cin == 64 && e->convs[p.logical[1]].cin == 128;
}

// Which kernel an OP_CONV / OP_CONVT / OP_PHASE launch runs (op.route, op.tile), from its shapes at max_batch (`a` = its
// conv_args) and the M355_* switches; and whether a head level is eligible for head_tail.hip.
void plan_route(m355_engine* e, Op& op, const ConvArgs& a) {
  const PlanSwitches& sw = e->sw;
  PhysConv& p = e->phys[op.conv];
  const Tensor& ti = e->tensors[op.in.t];
  if (op.kind == OP_PHASE) {
    op.tile = p.cout % 128 == 0 ? TILE_128x128 : TILE_64x128;
    if (p.l3 >= 0 && p.cin == 128 && p.cout == 128 && p.cout2 == 32 && ti.H % 8 == 0 && ti.W % 16 == 0 && !sw.no_protor)
      op.route = R_PROTOR;
    return;
  }
  const bool conv = op.kind == OP_CONV;
  op.tile = conv_pick_tile(a.Cout, a.M);
  if (a.ksize == 1 && op.tile == TILE_128x128 && sw.k1_tile >= 0) op.tile = sw.k1_tile;
  if (op.decode) op.tile = TILE_128x128;   // the whole 64 + nc + nm row of a pixel in one channel tile
  if (conv && conv3x3_halo_ok(a) && !sw.no_halo) op.route = R_HALO;
  // (M355_NO_WIDE / M355_NO_M32 as launch_conv3x3_halo takes them, so that this, the label and the launch cannot disagree)
  const bool m32 = op.route == R_HALO && conv3x3_halo_pick(a, proc_switches().no_wide, proc_switches().no_m32) == TILE_M32;
  if (conv && conv3x3_c32_ok(a) && !sw.no_c32) op.route = R_C32;
  // 1x1 with K <= 512 and Cout a multiple of 128: weights in registers (conv1x1_wreg.hip)
  if (conv && op.out_ext == 0 && p.l3 < 0 && !p.diag && op.res.t < 0 && !op.decode && (op.in2.t < 0 || !sw.no_w1_split) &&
      conv1x1_wreg_ok(a) && !sw.no_w1)
    op.route = R_W1;
  if (conv && op.route != R_HALO && op.route != R_C32 && conv3x3_slab_ok(a) && !sw.no_slab) op.route = R_SLAB;
  // row-slab kernel in single-conv mode (conv3x3_planes.hip) for what the slab kernel took (the 20 x 20 level): one block per CU
  // owns a slab x 64 channels with its weights streamed to registers -- 21 us against 34 on 256 -> 256 at batch 32
  // ... and for the stride-2 3x3 convs that were on the im2col kernel (model.5 / 7 / 16 / 19 of the s scale: 177 us at batch 32)
  const bool planes_s2 = p.k == 3 && p.stride == 2 && op.res.t < 0 && op.in2.t < 0 && !sw.no_planes_s2;
  // ... and for the 64 -> 64 conv of the 40 x 40 level (model.22.cv2.1.1: 9 us against 14 on the 32x32x16 halo kernel)
  const bool planes_m64 = m32 && a.Cout <= 64 && op.res.t < 0 && op.in2.t < 0 && !sw.no_planes_m64;
  if (conv && (op.route == R_SLAB || planes_s2 || planes_m64) && op.out_ext == 0 && p.l3 < 0 && !p.diag && !sw.no_planes) {
    PlanesArgs pa = planes_args(e, op, e->desc.max_batch, 0);
    pa.wfb = (const half_t*)1;   // placeholder: the fragments are packed after planning, and only for the ops planned here
    if (conv3x3_planes_ok(pa)) {
      op.route = R_PLANES;
      p.planes = 1;
    }
  }
  if (conv && op.out_ext == 1 && !op.decode && head_tail_layout(e, p) && ti.C == 224 && op.in.off == 0 && op.raw_off == 0 &&
      a.Ho * a.Wo >= 32 && !sw.no_headtail) {
    op.headtail = 1;   // (the route stays im2col: which path runs depends on keep_raw at forward time)
    ++e->headtail_n;
  }
  if (conv && p.l3 >= 0 && p.k == 3 && p.stride == 2 && p.cin == 32 && p.cout == 64 && p.cout2 == 64 && a.Ho % 8 == 0 &&
      a.Wo % 16 == 0 && !sw.no_s2c32)
    op.route = R_S2C32;
  if (conv && p.l3 >= 0 && p.k == 3 && p.stride == 2 && p.cin == 64 && p.cout == 128 && p.cout2 == 128 && a.Ho % 8 == 0 &&
      a.Wo % 8 == 0 && !sw.no_s2c64)
    op.route = R_S2C64;
}

// The op table's kernel label of a conv launch, from its route and shapes (`a` = its conv_args at max_batch)
void conv_label(const m355_engine* e, Op& op, const ConvArgs& a) {
  static const char* tile_names[] = {"128x128", "64x128", "32x256", "64x256"};
  const PhysConv& p = e->phys[op.conv];
  char* k = op.kernel;
  const size_t n = sizeof(op.kernel);
  const char* ch = a.Cout > 64 ? "128ch" : "64ch";
  switch (op.route) {
    case R_IGEMM:
      if (op.kind == OP_PHASE) snprintf(k, n, "conv_igemm<%s,k2,phase%s>", tile_names[op.tile], p.l3 >= 0 ? "+1x1" : "");
      else snprintf(k, n, "conv_igemm<%s,k%d%s>", tile_names[op.tile], a.ksize, p.l3 >= 0 ? "+1x1" : op.decode ? "+decode" : "");
      break;
    case R_HALO: {
      const int pick = conv3x3_halo_pick(a, proc_switches().no_wide, proc_switches().no_m32);
      if (pick == TILE_HALOWIDE) snprintf(k, n, "conv3x3_wide<128ch,16x16px>");
      else if (pick == TILE_M32) snprintf(k, n, "conv3x3_m32<%s,8x16px>", ch);
      else snprintf(k, n, "conv3x3_halo<%s>", ch);
      break;
    }
    case R_C32: snprintf(k, n, "conv3x3_c32<32ch,16x16px>"); break;
    case R_SLAB: snprintf(k, n, "conv3x3_slab<64ch,rows>"); break;
    case R_W1: snprintf(k, n, "conv1x1_wreg<K%d,%dch>", p.cin, a.Cout % 256 == 0 ? 256 : 128); break;
    case R_PLANES: snprintf(k, n, p.stride == 2 ? "conv3x3_planes<64ch,rows,s2>" : "conv3x3_planes<64ch,rows>"); break;
    case R_S2C32: snprintf(k, n, "conv3x3_s2c32<8x16px>+1x1"); break;
    case R_S2C64: snprintf(k, n, "conv3x3_s2c64<8x8px>+1x1"); break;
    case R_PROTOR: snprintf(k, n, "proto_phase_wreg<8x16px>"); break;
  }
}

// Fill the measurement metadata of every op and plan its kernel (algorithmic FLOPs = 2*MACs; algorithmic
// bytes = every activation read once + written once, weights once).
void annotate_ops(m355_engine* e) {
  for (Op& op : e->ops) {
    if (op.conv >= 0) snprintf(op.layer, sizeof(op.layer), "%s", e->convs[e->phys[op.conv].logical[0]].name);
    if (op.kind == OP_CONV || op.kind == OP_CONVT || op.kind == OP_PHASE) {
      const ConvArgs a = conv_args(e, op, e->desc.max_batch, 0, nullptr, nullptr);
      plan_route(e, op, a);
      conv_label(e, op, a);
    }
    switch (op.kind) {
      case OP_STEM: {
        const PhysConv& p = e->phys[op.conv];
        const Tensor& to = e->tensors[op.out.t];
        snprintf(op.kernel, sizeof(op.kernel), "stem_conv<k3s2,u8,mfma>");
        op.flops = 2.0 * to.H * to.W * p.cout * 27;
        op.bytes = (double)op.Hi * op.Wi * 3 + (double)to.H * to.W * p.cout * 2;
        op.wbytes = 28.0 * p.cout * 4;
        if (p.k == 6) {
          snprintf(op.kernel, sizeof(op.kernel), "stem6_s2<k6s2p2,u8,mfma>");
          op.flops = 2.0 * to.H * to.W * p.cout * 108;
          op.wbytes = (double)p.cout * (128 * 2 + 4);
        }
        break;
      }
      case OP_CONV:
      case OP_CONVT: {
        const PhysConv& p = e->phys[op.conv];
        const Tensor& ti = e->tensors[op.in.t];
        int Ho, Wo, cout_v = p.cout;
        if (op.kind == OP_CONVT) {
          Ho = ti.H; Wo = ti.W; cout_v = 4 * p.cout;
          op.flops = 2.0 * Ho * Wo * p.cin * cout_v;
        } else {
          Ho = (ti.H + 2 * (p.k / 2) - p.k) / p.stride + 1;
          Wo = (ti.W + 2 * (p.k / 2) - p.k) / p.stride + 1;
          op.flops = 2.0 * Ho * Wo * p.macs_px;
        }
        if (op.kind == OP_CONV && p.l3 >= 0) {   // + the 1x1 conv in the epilogue
          snprintf(op.layer, sizeof(op.layer), "%s+%s", e->convs[p.logical[0]].name, e->convs[p.l3].name);
          op.flops += 2.0 * Ho * Wo * (double)p.cout * p.cout2;
        }
        op.bytes = (double)ti.H * ti.W * p.cin * 2 + (double)Ho * Wo * cout_v * (op.out_ext == 1 ? 4 : 2) +
                   (op.res.t >= 0 ? (double)Ho * Wo * cout_v * 2 : 0.0);
        if (op.decode)       // writes prediction rows (4 + nc + nm floats) instead of (or besides) the raw rows
          op.bytes = (double)ti.H * ti.W * p.cin * 2 + (double)Ho * Wo * (4 + e->nc + e->nm) * 4 + (e->keep_raw ? (double)Ho * Wo * cout_v * 4 : 0.0);
        if (op.in2.t >= 0)   // the read-through part is a quarter-size tensor
          op.bytes -= (double)ti.H * ti.W * op.in2.c * 2 * 0.75;
        op.wbytes = (double)p.cout_pad * p.Kpad * 2;
        break;
      }
      case OP_PHASE: {
        const PhysConv& p = e->phys[op.conv];
        const Tensor& ti = e->tensors[op.in.t];
        snprintf(op.layer, sizeof(op.layer), p.l3 >= 0 ? "model.22.proto.upsample+cv2+cv3" : "model.22.proto.upsample+cv2");
        op.flops = 2.0 * ti.H * ti.W * p.macs_px;
        op.bytes = (double)ti.H * ti.W * p.cin * 2 + (double)4 * ti.H * ti.W * (p.l3 >= 0 ? p.cout2 : p.cout) * 2;
        op.wbytes = (double)p.cout_pad * p.Kpad * 2;
        break;
      }
      case OP_C2F32: {
        const Tensor& t = e->tensors[op.in.t];
        const PhysConv &pa = e->phys[op.conv], &pb = e->phys[op.conv2], &pc = e->phys[op.conv3];
        snprintf(op.kernel, sizeof(op.kernel), "c2f_c32<8x16px>");
        snprintf(op.layer, sizeof(op.layer), "%s+cv2+%s", e->convs[pa.logical[0]].name, e->convs[pc.logical[0]].name);
        op.flops = 2.0 * t.H * t.W * (pa.macs_px + pb.macs_px + pc.macs_px);
        op.bytes = (double)t.H * t.W * (op.in.c + op.out.c) * 2;
        op.wbytes = ((double)pa.cout * pa.Kpad + (double)pb.cout * pb.Kpad + (double)pc.cout * pc.Kpad) * 2;
        break;
      }
      case OP_PAIR: {
        const Tensor& t = e->tensors[op.in.t];
        const PhysConv &pa = e->phys[op.conv], &pb = e->phys[op.conv2];
        snprintf(op.kernel, sizeof(op.kernel), "bneck_pair<%dch>", pa.cout);
        snprintf(op.layer, sizeof(op.layer), "%s+cv2", e->convs[pa.logical[0]].name);
        op.flops = 2.0 * t.H * t.W * (pa.macs_px + pb.macs_px);
        op.bytes = (double)t.H * t.W * (op.in.c + op.out.c) * 2;   // the shortcut re-reads the input slice from L2
        op.wbytes = ((double)pa.cout * pa.Kpad + (double)pb.cout * pb.Kpad) * 2;
        break;
      }
      case OP_POOL: {
        const Tensor& t = e->tensors[op.in.t];
        snprintf(op.kernel, sizeof(op.kernel), "sppf_pool");
        snprintf(op.layer, sizeof(op.layer), "model.9.m");
        op.bytes = (double)t.H * t.W * op.in.c * 2 * 4;
        break;
      }
      case OP_ADOWN: {
        const Tensor& t = e->tensors[op.in.t];
        snprintf(op.kernel, sizeof(op.kernel), "adown_pool");
        snprintf(op.layer, sizeof(op.layer), "adown.pool");
        op.bytes = (double)t.H * t.W * op.in.c * 2 + (double)(t.H - 1) * (t.W - 1) * op.out.c * 2 + (double)(t.H / 2) * (t.W / 2) * op.out2.c * 2;
        break;
      }
      case OP_UP: {
        const Tensor& t = e->tensors[op.in.t];
        snprintf(op.kernel, sizeof(op.kernel), "upsample2x");
        snprintf(op.layer, sizeof(op.layer), "upsample");
        op.bytes = (double)t.H * t.W * op.in.c * 2 * 5;
        break;
      }
      case OP_DWCONV: {
        const PhysConv& p = e->phys[op.conv];
        const Tensor& ti = e->tensors[op.in.t];
        snprintf(op.kernel, sizeof(op.kernel), "dwconv3x3<%dch%s>", p.cout, p.act ? ",silu" : "");
        op.flops = 2.0 * ti.H * ti.W * p.cout * 9;
        op.bytes = (double)ti.H * ti.W * p.cout * 2 * 2;
        op.wbytes = (double)p.cout * (9 * 2 + 4);
        break;
      }
      case OP_PSA_ATTN: {
        const PhysConv& p = e->phys[op.conv];
        const Tensor& ti = e->tensors[op.in.t];
        const double N = (double)ti.H * ti.W;
        snprintf(op.kernel, sizeof(op.kernel), "psa_attn<%d,%d>", op.heads, ti.H * ti.W);
        snprintf(op.layer, sizeof(op.layer), "%s", e->convs[p.logical[0]].name);
        char* dot = strstr(op.layer, ".pe");
        if (dot) snprintf(dot, sizeof(op.layer) - (dot - op.layer), "+pe");
        op.flops = op.heads * 2.0 * N * N * (32 + 64) + 2.0 * N * p.cout * 9;
        op.bytes = N * (op.in.c + op.out.c) * 2;
        op.wbytes = (double)p.cout * (9 * 2 + 4);
        break;
      }
      case OP_DECODE:
        snprintf(op.kernel, sizeof(op.kernel), "head_decode");
        snprintf(op.layer, sizeof(op.layer), e->nm > 0 ? "model.22.decode" : (e->desc.scale >> 8) == '1' ? "model.23.decode" : "model.24.decode");
        op.bytes = (double)e->A * ((64 + e->nc + e->nm) + (4 + e->nc + e->nm)) * 4;
        break;
    }
  }
  // stem + model.1 (+ cv1) in one launch when the patch kernel takes model.1 and the stem feeds nothing else (conv_stem_s2c32.hip)
  for (size_t i = 0; i + 1 < e->ops.size(); ++i) {
    Op& st = e->ops[i];
    Op& nx = e->ops[i + 1];
    if (st.kind != OP_STEM || e->phys[st.conv].k != 3 || nx.route != R_S2C32 || nx.in.t != st.out.t || st.lane != nx.lane || st.record || e->sw.no_stemfuse) continue;
    bool other = false;
    for (size_t j = i + 2; j < e->ops.size(); ++j)
      if (e->ops[j].in.t == st.out.t || e->ops[j].res.t == st.out.t || e->ops[j].in2.t == st.out.t) other = true;
    if (other || e->phys[st.conv].cout != 32 || (st.Wi * 3) % 16) continue;
    nx.stemfuse = (int)i;
    st.fused_away = true;
    const Tensor& to = e->tensors[nx.out.t];
    snprintf(nx.kernel, sizeof(nx.kernel), "stem+conv3x3_s2c32<8x16px>+1x1");
    snprintf(nx.layer, sizeof(nx.layer), "model.0+model.1+model.2.cv1");
    nx.flops += st.flops;
    nx.bytes = (double)st.Hi * st.Wi * 3 + (double)to.H * to.W * e->phys[nx.conv].cout2 * 2;
    nx.wbytes += st.wbytes;
    st.flops = st.bytes = st.wbytes = 0;
  }
}

// device copy of a fragment-ordered weight list (allocated on first use)
hipError_t put_frags(half_t** dst, const std::vector<half_t>& fp) {
  const size_t bytes = fp.size() * sizeof(half_t);
  const hipError_t st = *dst ? hipSuccess : hipMalloc((void**)dst, bytes);
  return st != hipSuccess ? st : hipMemcpy(*dst, fp.data(), bytes, hipMemcpyHostToDevice);
}

}  // namespace

extern "C" {

const char* m355_version(void) { return "mi355yolo 0.1 (gfx950, fp16 NHWC implicit-GEMM MFMA)"; }

const char* m355_last_error(const m355_engine* e) { return e ? e->err.c_str() : g_err.c_str(); }

int m355_create(const m355_model_desc* desc, m355_engine** out) {
  if (!desc || !out) {
    g_err = "null argument";
    return M355_ERR_INVALID;
  }
  *out = nullptr;
  {   // the family / scale code is checked before the device is: a bad descriptor is M355_ERR_INVALID on any machine
    const int fam = desc->scale >> 8, sc = desc->scale & 0xff;
    const bool ok = fam == 0 ? (sc == 'n' || sc == 's' || sc == 'm' || sc == 'l' || sc == 'x' || sc == 'c')
                             : (fam == '5' || fam == '1') && (sc == 'n' || sc == 's' || sc == 'm');
    if (!ok) {
      g_err = "m355_model_desc.scale: unknown family or scale (0 | n,s,m,l,x,c; ('5' << 8) | n,s,m; ('1' << 8) | n,s,m)";
      return M355_ERR_INVALID;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    g_err = "no HIP device visible: libmi355yolo has no CPU fallback";
    return M355_ERR_NO_DEVICE;
  }
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
    g_err = "hipGetDeviceProperties failed";
    return M355_ERR_HIP;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_err = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
    return M355_ERR_NO_DEVICE;
  }
  m355_engine* e = new m355_engine();
  e->desc = *desc;
  e->sw = read_plan_switches();
  int rc = build_graph(e);
  if (rc == 0) fuse_conv_cv1(e);
  if (rc == 0) fuse_decode(e);
  if (rc == 0) rc = plan_lanes(e);
  if (rc == 0) plan_sub_batches(e);
  if (rc == 0) rc = alloc_all(e);
  if (rc == 0) annotate_ops(e);
  if (rc != 0) {
    g_err = e->err;
    m355_destroy(e);
    return rc;
  }
  *out = e;
  return M355_OK;
}

void m355_destroy(m355_engine* e) {
  if (!e) return;
  for (Tensor& t : e->tensors)
    if (t.p) (void)hipFree(t.p);
  for (PhysConv& p : e->phys) {
    if (p.w) (void)hipFree(p.w);
    if (p.bias) (void)hipFree(p.bias);
    if (p.stem_w) (void)hipFree(p.stem_w);
    if (p.wf) (void)hipFree(p.wf);
    if (p.wf2) (void)hipFree(p.wf2);
    if (p.w2) (void)hipFree(p.w2);
    if (p.bias2) (void)hipFree(p.bias2);
  }
  if (e->raw) (void)hipFree(e->raw);
  if (e->zero) (void)hipFree(e->zero);
  if (e->tileq) (void)hipFree(e->tileq);
  if (e->nms_ws) (void)hipFree(e->nms_ws);
  for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : e->op_done)
    if (ev) (void)hipEventDestroy(ev);
  for (hipStream_t st : e->side)
    if (st) (void)hipStreamDestroy(st);
  delete e;
}

int m355_num_convs(const m355_engine* e) { return e ? (int)e->convs.size() : M355_ERR_INVALID; }

int m355_get_conv_info(const m355_engine* e, int idx, m355_conv_info* out) {
  if (!e || !out || idx < 0 || idx >= (int)e->convs.size()) return M355_ERR_INVALID;
  *out = e->convs[idx];
  return M355_OK;
}

int m355_num_anchors(const m355_engine* e) { return e ? e->A : M355_ERR_INVALID; }
int m355_pred_width(const m355_engine* e) { return e ? 4 + e->nc + e->nm : M355_ERR_INVALID; }
int m355_proto_hw(const m355_engine* e, int* h, int* w) {
  if (!e || !h || !w) return M355_ERR_INVALID;
  *h = e->proto_h; *w = e->proto_w;
  return M355_OK;
}
size_t m355_workspace_bytes(const m355_engine* e) { return e ? e->ws_bytes : 0; }
double m355_flops_per_image(const m355_engine* e) { return e ? 2.0 * e->macs : 0.0; }

int m355_set_conv_weights(m355_engine* e, int idx, const float* w, const float* bias) {
  if (!e) return M355_ERR_INVALID;
  if (!w || !bias || idx < 0 || idx >= (int)e->convs.size()) return e->fail(M355_ERR_INVALID, "bad conv index / null");
  const m355_conv_info& ci = e->convs[idx];
  PhysConv& p = e->phys[e->conv_phys[idx]];
  const int row0 = e->conv_phys_off[idx];
  if (idx == p.l3) {   // a 1x1 conv applied in its producer's epilogue (proto.cv3, C2f.cv1 after a stride-2 conv): plain fp16 [cout2][K] + bias
    const std::vector<half_t> r2 = to_half_vec(w, (size_t)p.cout2 * p.cout);
    HIP_TRY(e, hipMemcpy(p.w2, r2.data(), r2.size() * sizeof(half_t), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(p.bias2, bias, p.cout2 * sizeof(float), hipMemcpyHostToDevice));
    const bool wreg = p.composed ? (p.cout2 == 32 && p.cout == 128)   // proto_phase_wreg.hip
                                 : (p.k == 3 && p.stride == 2 && ((p.cin == 32 && p.cout == 64 && p.cout2 == 64) ||      // conv_stem_c2
                                                                  (p.cin == 64 && p.cout == 128 && p.cout2 == 128)));   // conv3x3_s2c64
    if (wreg) HIP_TRY(e, put_frags(&p.wf2, frag_pack(r2.data(), p.cout, epilogue_frags(p.cout2, p.cout), false)));
    e->conv_loaded[idx] = true;
    return M355_OK;
  }
  if (p.composed) {   // keep the two logical weight sets until both are here, then compose (fp64) and upload
    const int n = p.cout;    // = cin = npr
    if (ci.transposed) {
      p.h_wt.assign(w, w + (size_t)n * n * 4);
      p.h_bt.assign(bias, bias + n);
    } else {
      p.h_w3.assign(w, w + (size_t)n * n * 9);
      p.h_b3.assign(bias, bias + n);
    }
    e->conv_loaded[idx] = true;
    if (p.h_wt.empty() || p.h_w3.empty()) return M355_OK;
    std::vector<half_t> rows;
    std::vector<float> btab;
    compose_proto_phases(n, p.h_wt.data(), p.h_bt.data(), p.h_w3.data(), p.h_b3.data(), p.cout_pad, p.Kpad, rows, btab);
    HIP_TRY(e, hipMemcpy(p.w, rows.data(), rows.size() * sizeof(half_t), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(p.bias, btab.data(), btab.size() * sizeof(float), hipMemcpyHostToDevice));
    if (n == 128) HIP_TRY(e, put_frags(&p.wf, frag_pack(rows.data(), p.Kpad, frag_grid(4 * n, 4 * n), false)));   // proto_phase_wreg.hip
    return M355_OK;
  }
  if (p.groups > 1) {   // depthwise 3x3 (dwconv3x3.hip, psa_attn.hip's pe): (C,1,3,3) -> [9][C] fp16
    std::vector<half_t> dw((size_t)9 * ci.cout);
    pack_dw3x3_weights(w, ci.cout, dw.data());
    HIP_TRY(e, hipMemcpy(p.w, dw.data(), dw.size() * sizeof(half_t), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(p.bias, bias, ci.cout * sizeof(float), hipMemcpyHostToDevice));
  } else if (ci.cin == 3 && ci.k == 6) {   // YOLOv5u stem (conv_stem6_s2.hip): [C0][128] fp16 rows in the kernel's order
    std::vector<half_t> sw((size_t)ci.cout * 128);
    pack_stem6_weights(w, ci.cout, sw.data());
    HIP_TRY(e, hipMemcpy(p.w, sw.data(), sw.size() * sizeof(half_t), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(p.bias, bias, ci.cout * sizeof(float), hipMemcpyHostToDevice));
  } else if (ci.cin == 3) {  // 3x3 stem: [cout][32] fp16
    const std::vector<half_t> sw = pack_stem3x3(w, ci.cout);
    HIP_TRY(e, hipMemcpy(p.stem_w, sw.data(), sw.size() * sizeof(half_t), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(p.bias, bias, ci.cout * sizeof(float), hipMemcpyHostToDevice));
  } else if (ci.transposed) {  // ConvTranspose 2x2: 4 cout virtual channels, K = cin
    std::vector<half_t> rows((size_t)4 * ci.cout * p.Kpad, (half_t)0.f);
    pack_convt2x2_rows(w, ci.cin, ci.cout, p.Kpad, rows);
    HIP_TRY(e, hipMemcpy(p.w, rows.data(), rows.size() * sizeof(half_t), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(p.bias, bias, ci.cout * sizeof(float), hipMemcpyHostToDevice));
  } else {
    std::vector<half_t> rows((size_t)ci.cout * p.Kpad, (half_t)0.f);
    pack_conv_rows(w, ci.cout, ci.cin, ci.k, p.Kpad, 0, rows, p.diag ? e->conv_phys_koff[idx] : 0);
    HIP_TRY(e, hipMemcpy(p.w + (size_t)row0 * p.Kpad, rows.data(), rows.size() * sizeof(half_t),
                         hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(p.bias + row0, bias, ci.cout * sizeof(float), hipMemcpyHostToDevice));
    if (head_tail_layout(e, p)) {   // head level (head_tail.hip): the fragments, once its three convs are here
      bool all = true;
      for (int li : p.logical) all = all && (li == idx || e->conv_loaded[li]);
      const int rows_pad = conv_cout_pad(p.cout);
      if (all && 64 + e->nc + 32 <= rows_pad) {
        std::vector<half_t> full((size_t)rows_pad * p.Kpad);
        HIP_TRY(e, hipMemcpy(full.data(), p.w, full.size() * sizeof(half_t), hipMemcpyDeviceToHost));
        HIP_TRY(e, put_frags(&p.wf, frag_pack(full.data(), p.Kpad, head_level_frags(e->nc), false)));
      }
    }
    if (p.planes && ci.k == 3 && p.cin % 32 == 0 && !p.diag && p.l3 < 0) {   // K-loop fragment order of the row-slab kernels, channel blocks padded with zero rows
      bool all = true;   // (a launch shared by several logical convs -- the head's first layer -- packs once all of them are here)
      for (int li : p.logical) all = all && (li == idx || e->conv_loaded[li]);
      if (all) {
        std::vector<half_t> full((size_t)p.cout * p.Kpad);
        HIP_TRY(e, hipMemcpy(full.data(), p.w, full.size() * sizeof(half_t), hipMemcpyDeviceToHost));
        HIP_TRY(e, put_frags(&p.wf, planes_frag_pack_padded(full.data(), p.cout, p.Kpad, p.cin)));
      }
    } else if ((p.logical.size() == 1 || (p.l3 >= 0 && !p.composed && idx == p.logical[0])) && !p.diag && row0 == 0) {   // fragment-ordered copies for the weights-in-registers kernels
      const auto fl = frag_list(ci.k, ci.cin, ci.cout);
      if (!fl.empty()) {
        const bool stem_pair = ci.k == 3 && ci.cin == 32 && ci.cout == 64;   // its accumulators feed the 1x1's MFMAs directly
        HIP_TRY(e, put_frags(&p.wf, frag_pack(rows.data(), p.Kpad, fl, stem_pair)));
        if (ci.k == 3 && ci.cin == 32 && !stem_pair) HIP_TRY(e, put_frags(&p.wf2, frag_pack(rows.data(), p.Kpad, fl, true)));
      }
    }
  }
  e->conv_loaded[idx] = true;
  return M355_OK;
}

int m355_forward(m355_engine* e, const void* d_in, int B, float* d_preds, void* d_protos, void* stream) {
  if (!e) return M355_ERR_INVALID;
  if (!d_in || !d_preds || (!d_protos && e->nm > 0)) return e->fail(M355_ERR_INVALID, "null device pointer");
  if (B < 1 || B > e->desc.max_batch) return e->fail(M355_ERR_STATE, "batch exceeds max_batch");
  for (size_t i = 0; i < e->conv_loaded.size(); ++i)
    if (!e->conv_loaded[i]) return e->fail(M355_ERR_STATE, std::string("weights not set for ") + e->convs[i].name);
  hipStream_t s_main = (hipStream_t)stream;
  // head levels as conv + decode launches (head_tail.hip): all three or none.  The kernel's 31-bit byte-offset bound is reached by the
  // stride-8 level first (batch >= 749 at 640 x 640); a per-level choice would leave the decode launch to overwrite the rows
  // the other two levels had already written with whatever the raw buffer holds.
  e->headtail_active = false;
  if (!e->keep_raw && e->headtail_n == 3) {
    bool all = true;
    for (const Op& op : e->ops) {
      if (!op.headtail) continue;
      const HeadTailArgs ha = head_tail_args(e, op, B, d_preds);
      if (!ha.wf || !head_tail_ok(ha) || (e->sw.headtail_maxm > 0 && ha.M > e->sw.headtail_maxm)) all = false;
    }
    e->headtail_active = all;
  }
  const bool lanes = e->nlanes > 1 && !e->profiling;   // per-op event timing needs one stream
  // ops [lo, hi) over images [b0, b0 + Bq)
  auto run_range = [&](size_t lo, size_t hi, const int b0, const int Bq) -> int {
  for (size_t oi = lo; oi < hi; ++oi) {
    const Op& op = e->ops[oi];
    if (op.fused_away) continue;
    int rc = 0;
    hipStream_t s = (lanes && op.lane > 0) ? e->side[op.lane - 1] : s_main;
    if (lanes)
      for (int p : op.wait_ops) HIP_TRY(e, hipStreamWaitEvent(s, e->op_done[p], 0));
    if (e->profiling) {
      if (e->ev_used + 2 > e->ev_pool.size()) {
        for (int i = 0; i < 2; ++i) {
          hipEvent_t ev;
          HIP_TRY(e, hipEventCreate(&ev));
          e->ev_pool.push_back(ev);
        }
      }
      HIP_TRY(e, hipEventRecord(e->ev_pool[e->ev_used], s));
    }
    switch (op.kind) {
      case OP_STEM: {
        const PhysConv& p = e->phys[op.conv];
        if (p.k == 6) {
          const Tensor& to = e->tensors[op.out.t];
          Stem6Args a{};
          a.x = (const uint8_t*)d_in + (long)b0 * op.Hi * op.Wi * 3; a.B = Bq; a.H = op.Hi; a.W = op.Wi;
          a.w = p.w; a.bias = p.bias; a.C0 = p.cout;
          a.y_bstride = (long)to.H * to.W * to.C; a.ldy = to.C;
          a.y = to.p + op.out.off + b0 * a.y_bstride;
          rc = launch_stem6(a, s);
          break;
        }
        rc = launch_stem(stem_args(e, op, Bq, b0, d_in), s);
        break;
      }
      case OP_CONV:
      case OP_CONVT:
      case OP_PHASE: {
        if (op.headtail && e->headtail_active && !b0) {   // conv + decode of this level in one launch
          rc = launch_head_tail(head_tail_args(e, op, Bq, d_preds), s);   // (eligibility was checked for all three levels at the top of this forward)
          break;
        }
        ConvArgs a = conv_args(e, op, Bq, b0, d_preds, d_protos);
        if (op.kind != OP_PHASE) a.tileq = proc_switches().static_tiles ? nullptr : e->tileq + 4 * oi;
        if (op.stemfuse >= 0) {
          const StemArgs sa = stem_args(e, e->ops[op.stemfuse], Bq, b0, d_in);
          const bool stem2 = !live_no_stem2();  // two-team form (conv_stem_c2.hip, the default); read per launch: tests toggle it
          if (stem2 && stem_s2c32_v2_ok(a, sa)) {
            rc = launch_stem_s2c32_v2(a, sa, s);
            break;
          }
          if (stem_s2c32_ok(a, sa)) {
            rc = launch_stem_s2c32(a, sa, s);
            break;
          }
          rc = launch_stem(sa, s);            // not eligible after all (shape): the two launches
          if (rc != 0) break;
        }
        // the fused and specialised routes fall back to the kernels they replaced where THIS call's shape is not eligible
        // (e.g. a pixel count that is not a multiple of the kernel's tile although max_batch's was)
        switch (op.route) {
          case R_IGEMM: rc = launch_conv_igemm(a, op.tile, s); break;
          case R_HALO: rc = launch_conv3x3_halo(a, 0, s); break;
          case R_C32: rc = launch_conv3x3_c32(a, s); break;
          case R_SLAB: rc = launch_conv3x3_slab(a, s); break;
          case R_W1: rc = conv1x1_wreg_ok(a) ? launch_conv1x1_wreg(a, s) : launch_conv_igemm(a, TILE_AUTO, s); break;
          case R_PLANES: {
            const PlanesArgs pa = planes_args(e, op, Bq, b0);
            rc = (pa.wfb && conv3x3_planes_ok(pa)) ? launch_conv3x3_planes(pa, s)
                 : a.stride == 2 ? launch_conv_igemm(a, TILE_AUTO, s)
                 : conv3x3_slab_ok(a) ? launch_conv3x3_slab(a, s) : launch_conv3x3_halo(a, 0, s);
            break;
          }
          case R_S2C32: rc = conv_s2c32_cv1_ok(a) ? launch_conv_s2c32_cv1(a, s) : launch_conv_igemm(a, op.tile, s); break;
          case R_S2C64: rc = conv_s2c64_cv1_ok(a) ? launch_conv_s2c64_cv1(a, s) : launch_conv_igemm(a, op.tile, s); break;
          case R_PROTOR: rc = proto_phase_wreg_ok(a) ? launch_proto_phase_wreg(a, s) : launch_conv_igemm(a, op.tile, s); break;
        }
        break;
      }
      case OP_C2F32: {
        const Tensor& ti = e->tensors[op.in.t];
        const Tensor& to = e->tensors[op.out.t];
        const PhysConv &pa = e->phys[op.conv], &pb = e->phys[op.conv2], &pc = e->phys[op.conv3];
        C2fC32Args a{};
        a.x_bstride = (long)ti.H * ti.W * ti.C; a.ldx = ti.C; a.H = ti.H; a.W = ti.W; a.B = Bq;
        a.x = ti.p + op.in.off + b0 * a.x_bstride;
        a.wa = pa.w; a.wb = pb.w; a.wc = pc.w; a.waf = pa.wf; a.wbf = pb.wf2; a.kpad_a = pa.Kpad; a.kpad_b = pb.Kpad; a.kpad_c = pc.Kpad;
        a.ba = pa.bias; a.bb = pb.bias; a.bc = pc.bias;
        a.y_bstride = (long)to.H * to.W * to.C; a.ldy = to.C;
        a.y = to.p + op.out.off + b0 * a.y_bstride;
        a.shortcut = op.shortcut;
        rc = launch_c2f_c32(a, s);
        break;
      }
      case OP_PAIR: {
        const PlanesArgs a = planes_args(e, op, Bq, b0);
        if (bneck_pair_ok(a)) {
          rc = launch_bneck_pair(a, s);
          break;
        }
        // two launches through the hidden tensor (a batch whose buffers exceed the kernel's 31-bit offsets)
        for (int half = 0; half < 2 && rc == 0; ++half) {
          Op h{};
          h.kind = OP_CONV;
          h.conv = half ? op.conv2 : op.conv;
          h.in = half ? op.out2 : op.in;
          h.out = half ? op.out : op.out2;
          if (half) h.res = op.res;
          const ConvArgs c = conv_args(e, h, Bq, b0, nullptr, nullptr);
          rc = conv3x3_halo_ok(c) ? launch_conv3x3_halo(c, 0, s) : launch_conv_igemm(c, TILE_AUTO, s);
        }
        break;
      }
      case OP_POOL: {
        const Tensor& t = e->tensors[op.in.t];
        rc = launch_sppf_pool(t.p + op.in.off, (long)t.H * t.W * t.C, t.C, t.p + op.out.off, (long)t.H * t.W * t.C,
                              t.C, Bq, t.H, t.W, op.in.c, s);
        break;
      }
      case OP_ADOWN: {
        const Tensor& ti = e->tensors[op.in.t];
        const Tensor& ta = e->tensors[op.out.t];
        const Tensor& tm = e->tensors[op.out2.t];
        rc = launch_adown_pool(ti.p + op.in.off, (long)ti.H * ti.W * ti.C, ti.C, ta.p + op.out.off, (long)ta.H * ta.W * ta.C, ta.C,
                               tm.p + op.out2.off, (long)tm.H * tm.W * tm.C, tm.C, Bq, ti.H, ti.W, op.in.c, s);
        break;
      }
      case OP_UP: {
        const Tensor& ti = e->tensors[op.in.t];
        const Tensor& to = e->tensors[op.out.t];
        rc = launch_upsample2x(ti.p + op.in.off, (long)ti.H * ti.W * ti.C, ti.C, to.p + op.out.off,
                               (long)to.H * to.W * to.C, to.C, Bq, ti.H, ti.W, op.in.c, s);
        break;
      }
      case OP_DWCONV: {
        const PhysConv& p = e->phys[op.conv];
        const Tensor& ti = e->tensors[op.in.t];
        const Tensor& to = e->tensors[op.out.t];
        DwConvArgs a{};
        a.x_bstride = (long)ti.H * ti.W * ti.C; a.ldx = ti.C; a.x = ti.p + op.in.off + b0 * a.x_bstride;
        a.B = Bq; a.H = ti.H; a.W = ti.W; a.C = p.cout;
        a.w = p.w; a.bias = p.bias; a.act = p.act;
        a.y_bstride = (long)to.H * to.W * to.C; a.ldy = to.C; a.y = to.p + op.out.off + b0 * a.y_bstride;
        rc = launch_dwconv3x3(a, s);
        break;
      }
      case OP_PSA_ATTN: {
        const PhysConv& p = e->phys[op.conv];
        const Tensor& ti = e->tensors[op.in.t];
        const Tensor& to = e->tensors[op.out.t];
        PsaArgs a{};
        a.q_bstride = (long)ti.H * ti.W * ti.C; a.ldq = ti.C; a.qkv = ti.p + op.in.off + b0 * a.q_bstride;
        a.B = Bq; a.H = ti.H; a.W = ti.W; a.heads = op.heads; a.C = p.cout;
        a.pe_w = p.w; a.pe_b = p.bias; a.scale_log2e = (float)(1.4426950408889634 / sqrt(32.0));
        a.y_bstride = (long)to.H * to.W * to.C; a.ldy = to.C; a.y = to.p + op.out.off + b0 * a.y_bstride;
        rc = launch_psa_attn(a, s);
        break;
      }
      case OP_DECODE:
        if (e->decode_fused) break;   // the three head output convs wrote the prediction rows
        if (e->headtail_active) break;   // so did the three head_tail launches of this forward
        rc = launch_head_decode(e->raw, Bq, e->desc.in_h, e->desc.in_w, e->nc, e->nm, d_preds, s);
        break;
    }
    if (e->profiling) {
      HIP_TRY(e, hipEventRecord(e->ev_pool[e->ev_used + 1], s));
      e->ev_used += 2;
      e->ev_op.push_back((int)oi);
    }
    if (rc != 0) return e->fail(M355_ERR_HIP, "kernel launch failed (op kind " + std::to_string((int)op.kind) +
                                                  ", code " + std::to_string(rc) + ")");
    if (lanes && op.record) HIP_TRY(e, hipEventRecord(e->op_done[oi], s));
  }
  return M355_OK;
  };
  const size_t nops = e->ops.size();
  size_t first = 0;
  if (!e->profiling && e->sub_batch > 0 && e->sub_ops > 0 && B > e->sub_batch) {
    for (int b0 = 0; b0 < B; b0 += e->sub_batch) {
      const int rcs = run_range(0, (size_t)e->sub_ops, b0, std::min(e->sub_batch, B - b0));
      if (rcs != M355_OK) return rcs;
    }
    first = (size_t)e->sub_ops;
  }
  {
    const int rcs = run_range(first, nops, 0, B);
    if (rcs != M355_OK) return rcs;
  }
  if (lanes)   // join: everything this forward launched is ordered before whatever the caller enqueues next
    for (int l = 1; l < e->nlanes; ++l)
      if (e->lane_last[l] >= 0) HIP_TRY(e, hipStreamWaitEvent(s_main, e->op_done[e->lane_last[l]], 0));
  return M355_OK;
}

int m355_num_ops(const m355_engine* e) { return e ? (int)e->ops.size() : M355_ERR_INVALID; }

int m355_get_op_info(const m355_engine* e, int idx, m355_op_info* out) {
  if (!e || !out || idx < 0 || idx >= (int)e->ops.size()) return M355_ERR_INVALID;
  const Op& op = e->ops[idx];
  memset(out, 0, sizeof(*out));
  snprintf(out->kernel, sizeof(out->kernel), "%s", op.kernel);
  snprintf(out->layer, sizeof(out->layer), "%s", op.layer);
  out->flops_per_image = op.flops;
  out->bytes_per_image = op.bytes;
  if (e->headtail_n == 3 && !e->keep_raw) {   // the head levels run as conv + decode launches (head_tail.hip), no decode launch
    const int wo = 4 + e->nc + e->nm;
    if (op.headtail) {
      const Tensor& ti = e->tensors[op.in.t];
      snprintf(out->kernel, sizeof(out->kernel), "head_tail<128px>");
      snprintf(out->layer, sizeof(out->layer), "%s+decode", op.layer);
      out->bytes_per_image = (double)ti.H * ti.W * (ti.C * 2 + wo * 4);
    } else if (op.kind == OP_DECODE) {
      snprintf(out->kernel, sizeof(out->kernel), "(none)");
      out->bytes_per_image = 0;
    }
  }
  out->weight_bytes = op.wbytes;
  return M355_OK;
}

int m355_set_profiling(m355_engine* e, int enable) {
  if (!e) return M355_ERR_INVALID;
  e->profiling = enable != 0;  // toggles recording only; m355_collect_op_times drains and resets
  return M355_OK;
}

int m355_collect_op_times(m355_engine* e, double* ms_sum, long* counts) {
  if (!e || !ms_sum || !counts) return M355_ERR_INVALID;
  const size_t n = e->ops.size();
  if (e->op_ms.size() != n) { e->op_ms.assign(n, 0.0); e->op_cnt.assign(n, 0); }
  for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
    const size_t oi = (size_t)e->ev_op[i / 2];
    HIP_TRY(e, hipEventSynchronize(e->ev_pool[i + 1]));
    float ms = 0.f;
    HIP_TRY(e, hipEventElapsedTime(&ms, e->ev_pool[i], e->ev_pool[i + 1]));
    e->op_ms[oi] += ms;
    e->op_cnt[oi] += 1;
  }
  e->ev_used = 0;
  e->ev_op.clear();
  for (size_t i = 0; i < n; ++i) { ms_sum[i] = e->op_ms[i]; counts[i] = e->op_cnt[i]; }
  e->op_ms.assign(n, 0.0);
  e->op_cnt.assign(n, 0);
  return M355_OK;
}

int m355_get_raw_head(m355_engine* e, const float** d_raw, int* width) {
  if (!e || !d_raw || !width) return M355_ERR_INVALID;
  if ((e->decode_fused || e->headtail_n == 3) && !e->keep_raw)
    return const_cast<m355_engine*>(e)->fail(M355_ERR_STATE, "the raw head maps are not written (m355_set_keep_raw(e, 1) before the forward)");
  *d_raw = e->raw;
  *width = 64 + e->nc + e->nm;
  return M355_OK;
}

int m355_set_keep_raw(m355_engine* e, int keep) {
  if (!e) return M355_ERR_INVALID;
  e->keep_raw = keep != 0;
  return M355_OK;
}

int m355_copy_raw_head(m355_engine* e, int B, float* d_out, void* stream) {
  if (!e) return M355_ERR_INVALID;
  if ((e->decode_fused || e->headtail_n == 3) && !e->keep_raw)
    return e->fail(M355_ERR_STATE, "the raw head maps are not written (m355_set_keep_raw(e, 1) before the forward)");
  if (!d_out || B < 1 || B > e->desc.max_batch) return e->fail(M355_ERR_INVALID, "bad argument");
  const size_t n = (size_t)B * e->A * (64 + e->nc + e->nm) * sizeof(float);
  HIP_TRY(e, hipMemcpyAsync(d_out, e->raw, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return M355_OK;
}

int m355_postprocess(m355_engine* e, const float* d_preds, const void* d_protos, int B, float conf, float iou,
                     int max_det, float* d_dets, int* d_counts, uint8_t* d_masks, void* stream) {
  if (!e) return M355_ERR_INVALID;
  if (!d_preds || !d_dets || !d_counts) return e->fail(M355_ERR_INVALID, "null device pointer");
  if (B < 1 || B > e->desc.max_batch) return e->fail(M355_ERR_STATE, "batch exceeds max_batch");
  if (d_masks && e->nm == 0) return e->fail(M355_ERR_INVALID, "a detection engine has no masks: pass d_masks = NULL");
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_nms(d_preds, B, e->A, e->nc, e->nm, conf, iou, max_det, d_dets, d_counts, e->nms_ws,
                      e->nms_ws_bytes, s);
  if (rc != 0) return e->fail(M355_ERR_HIP, "nms launch failed: " + std::to_string(rc));
  if (d_masks) {
    if (!d_protos) return e->fail(M355_ERR_INVALID, "d_protos is null");
    rc = launch_proto_masks(d_dets, d_counts, (const half_t*)d_protos, B, max_det, e->nm, e->proto_h, e->proto_w,
                            e->desc.in_h, e->desc.in_w, d_masks, s);
    if (rc != 0) return e->fail(M355_ERR_HIP, "mask launch failed: " + std::to_string(rc));
  }
  return M355_OK;
}

int m355_postprocess_ex(m355_engine* e, const float* d_preds, const void* d_protos, int B, float conf, float iou,
                        int max_det, int agnostic, const uint32_t* d_class_mask, float* d_dets, int* d_counts,
                        uint8_t* d_masks, void* stream) {
  if (!e) return M355_ERR_INVALID;
  if (!d_preds || !d_dets || !d_counts) return e->fail(M355_ERR_INVALID, "null device pointer");
  if (B < 1 || B > e->desc.max_batch) return e->fail(M355_ERR_INVALID, "batch must be in [1, max_batch]");
  if (max_det < 1 || max_det > 1024) return e->fail(M355_ERR_INVALID, "max_det must be in [1, 1024]");
  if (agnostic != 0 && agnostic != 1) return e->fail(M355_ERR_INVALID, "agnostic must be 0 or 1");
  if (d_class_mask && e->nc > 1024) return e->fail(M355_ERR_INVALID, "a class set covers at most 1024 classes");
  if (d_masks && e->nm == 0) return e->fail(M355_ERR_INVALID, "a detection engine has no masks: pass d_masks = NULL");
  if (d_masks && !d_protos) return e->fail(M355_ERR_INVALID, "d_protos is null");
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_nms(d_preds, B, e->A, e->nc, e->nm, conf, iou, max_det, d_dets, d_counts, e->nms_ws,
                      e->nms_ws_bytes, s, agnostic, d_class_mask);
  if (rc != 0) return e->fail(M355_ERR_HIP, "nms launch failed: " + std::to_string(rc));
  if (d_masks) {
    rc = launch_proto_masks(d_dets, d_counts, (const half_t*)d_protos, B, max_det, e->nm, e->proto_h, e->proto_w,
                            e->desc.in_h, e->desc.in_w, d_masks, s);
    if (rc != 0) return e->fail(M355_ERR_HIP, "mask launch failed: " + std::to_string(rc));
  }
  return M355_OK;
}

}  // extern "C"
