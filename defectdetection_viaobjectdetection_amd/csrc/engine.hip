// libmi355yolo.so engine: YOLOv8-seg layer plan, weight packing, workspace and the C-ABI
// (include/mi355yolo.h).  Host-side C++; all arithmetic is in the HIP kernels of this directory.
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

using namespace m355;

namespace {

thread_local std::string g_err;

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
  long headtail_maxm = 0;    // testing only (M355_HEADTAIL_MAXM at create): a level with more pixels than this counts as ineligible
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
    if (c == 32 && n == 1 && H % 8 == 0 && W % 16 == 0 && out.c == 64 && c2f_addr_ok && !getenv("M355_NO_C2F32")) {
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
      if (bneck_pair_shape_ok(c, H, W) && !getenv("M355_NO_PAIR")) {
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
  // stream lane of Proto and of the three head levels (plan_lanes): measured best on MI355X at batch 32
  int lane_plan[4] = {1, 2, 2, 0};
  if (const char* lp = getenv("M355_LANE_PLAN"))
    for (int i = 0; i < 4 && lp[i] >= '0' && lp[i] <= '3'; ++i) lane_plan[i] = lp[i] - '0';
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
    const bool fuse2 = !getenv("M355_NO_PROTOFUSE") && npr % 64 == 0;   // a channel tile (64 or 128) must lie inside one phase
    const bool fuse3 = fuse2 && npr == 128 && nm == 32 && !getenv("M355_NO_PROTOFUSE3");
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
  const bool upfuse = !getenv("M355_NO_UPFUSE");
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
  const bool upfuse = !getenv("M355_NO_UPFUSE");
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
  const bool upfuse = !getenv("M355_NO_UPFUSE");
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
  const bool upfuse = !getenv("M355_NO_UPFUSE");
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
  if (getenv("M355_NO_CVFUSE")) return;
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
  // measured at batch 32: 179 us for the three launches against 93 + 39 us separately, -1 % end to end (two serial 64-pixel
  // passes with four barriers each behind every tile): opt-in
  if (!getenv("M355_DECFUSE")) return;
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
  const char* sb = getenv("M355_SUBBATCH");
  e->sub_batch = sb ? atoi(sb) : 0;   // measured at batch 32 with two engines in flight: 8 -> -5 %, 16 -> -2 %: off by default
  if (e->sub_batch <= 0 || getenv("M355_NO_SUBBATCH")) { e->sub_batch = 0; return; }
  int n = 0;
  for (const Op& op : e->ops) {
    if ((op.kind != OP_STEM && op.kind != OP_CONV && op.kind != OP_C2F32 && op.kind != OP_PAIR) || op.lane != 0 || op.record || !op.wait_ops.empty() || op.out_ext != 0) break;
    const Tensor& to = e->tensors[op.out.t];
    if (to.H * 8 < e->desc.in_h) break;
    ++n;
  }
  if (const char* so = getenv("M355_SUBBATCH_OPS")) n = std::min(n, atoi(so));
  e->sub_ops = n;
}

// Stream lanes.  The builder tags the ops of Proto and of the stride-8 head level with lane 1; everything else is
// lane 0 (the caller's stream).  (1) Reorder: a lane-1 op moves to right after the last lane-0 op it depends on, so the
// host enqueues it as early as the data allows (lane order is kept, so the result is still a topological order).
// (2) Cross-lane dependencies become event waits; the last op of every side lane is joined into the caller's stream.
int plan_lanes(m355_engine* e) {
  if (getenv("M355_NO_LANES")) {
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
  if (op.kind == OP_PAIR) { a.wfa = pa.wf; a.cblocks_a = (pa.cout + 63) / 64 * 2; a.ba = pa.bias; }
  a.wfb = pb.wf; a.cblocks_b = (pb.cout + 63) / 64 * 2; a.bb = pb.bias;
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
  PhysConv& p = e->phys[op.conv];
  const Tensor& ti = e->tensors[op.in.t];
  if (op.kind == OP_PHASE) {
    op.tile = p.cout % 128 == 0 ? TILE_128x128 : TILE_64x128;
    if (p.l3 >= 0 && p.cin == 128 && p.cout == 128 && p.cout2 == 32 && ti.H % 8 == 0 && ti.W % 16 == 0 && !getenv("M355_NO_PROTOR"))
      op.route = R_PROTOR;
    return;
  }
  const bool conv = op.kind == OP_CONV;
  op.tile = conv_pick_tile(a.Cout, a.M);
  if (a.ksize == 1 && op.tile == TILE_128x128 && getenv("M355_K1_TILE")) op.tile = atoi(getenv("M355_K1_TILE"));
  if (op.decode) op.tile = TILE_128x128;   // the whole 64 + nc + nm row of a pixel in one channel tile
  if (conv && conv3x3_halo_ok(a) && !getenv("M355_NO_HALO")) op.route = R_HALO;
  const bool m32 = op.route == R_HALO && conv3x3_halo_pick(a, getenv("M355_NO_WIDE"), getenv("M355_NO_M32")) == TILE_M32;
  if (conv && conv3x3_c32_ok(a) && !getenv("M355_NO_C32")) op.route = R_C32;
  // 1x1 with K <= 512 and Cout a multiple of 128: weights in registers (conv1x1_wreg.hip)
  if (conv && op.out_ext == 0 && p.l3 < 0 && !p.diag && op.res.t < 0 && !op.decode && (op.in2.t < 0 || !getenv("M355_NO_W1_SPLIT")) &&
      conv1x1_wreg_ok(a) && !getenv("M355_NO_W1"))
    op.route = R_W1;
  if (conv && op.route != R_HALO && op.route != R_C32 && conv3x3_slab_ok(a) && !getenv("M355_NO_SLAB")) op.route = R_SLAB;
  // row-slab kernel in single-conv mode (conv3x3_planes.hip) for what the slab kernel took (the 20 x 20 level): one block per CU
  // owns a slab x 64 channels with its weights streamed to registers -- 21 us against 34 on 256 -> 256 at batch 32
  // ... and for the stride-2 3x3 convs that were on the im2col kernel (model.5 / 7 / 16 / 19 of the s scale: 177 us at batch 32)
  const bool planes_s2 = p.k == 3 && p.stride == 2 && op.res.t < 0 && op.in2.t < 0 && !getenv("M355_NO_PLANES_S2");
  // ... and for the 64 -> 64 conv of the 40 x 40 level (model.22.cv2.1.1: 9 us against 14 on the 32x32x16 halo kernel)
  const bool planes_m64 = m32 && a.Cout <= 64 && op.res.t < 0 && op.in2.t < 0 && !getenv("M355_NO_PLANES_M64");
  if (conv && (op.route == R_SLAB || planes_s2 || planes_m64) && op.out_ext == 0 && p.l3 < 0 && !p.diag && !getenv("M355_NO_PLANES")) {
    PlanesArgs pa = planes_args(e, op, e->desc.max_batch, 0);
    pa.wfb = (const half_t*)1;   // placeholder: the fragments are packed after planning, and only for the ops planned here
    if (conv3x3_planes_ok(pa)) {
      op.route = R_PLANES;
      p.planes = 1;
    }
  }
  if (conv && op.out_ext == 1 && !op.decode && head_tail_layout(e, p) && ti.C == 224 && op.in.off == 0 && op.raw_off == 0 &&
      a.Ho * a.Wo >= 32 && !getenv("M355_NO_HEADTAIL")) {
    op.headtail = 1;   // (the route stays im2col: which path runs depends on keep_raw at forward time)
    ++e->headtail_n;
  }
  if (conv && p.l3 >= 0 && p.k == 3 && p.stride == 2 && p.cin == 32 && p.cout == 64 && p.cout2 == 64 && a.Ho % 8 == 0 &&
      a.Wo % 16 == 0 && !getenv("M355_NO_S2C32"))
    op.route = R_S2C32;
  if (conv && p.l3 >= 0 && p.k == 3 && p.stride == 2 && p.cin == 64 && p.cout == 128 && p.cout2 == 128 && a.Ho % 8 == 0 &&
      a.Wo % 8 == 0 && !getenv("M355_NO_S2C64"))
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
      const int pick = conv3x3_halo_pick(a, getenv("M355_NO_WIDE"), getenv("M355_NO_M32"));
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
    if (st.kind != OP_STEM || e->phys[st.conv].k != 3 || nx.route != R_S2C32 || nx.in.t != st.out.t || st.lane != nx.lane || st.record || getenv("M355_NO_STEMFUSE")) continue;
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

// Pack fp32 (cout,cin,k,k) -> fp16 rows [row0+co][ (kh*k+kw)*cin + ci ] of a [cout_pad][Kpad] matrix.
void pack_conv_rows(const float* w, int cout, int cin, int k, int Kpad, int row0, std::vector<half_t>& dst, int koff = 0) {
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int kh = 0; kh < k; ++kh)
        for (int kw = 0; kw < k; ++kw)
          dst[(size_t)(row0 + co) * Kpad + koff + (kh * k + kw) * cin + ci] =
              (half_t)w[(((size_t)co * cin + ci) * k + kh) * k + kw];
}

// Fragment-ordered copy of packed rows for the weights-in-registers kernels.  Fragment f = (first row r0 of a 32-row block,
// first K element k0 of a 16-deep slice); out[(f * 64 + lane) * 8 + j] = rows[(r0 + perm(lane & 31)) * Kpad + k0 + 8 * (lane >> 5)
// + j]: exactly the A operand of one v_mfma_f32_32x32x16_f16, so a wave fetches a fragment with ONE coalesced 1 KiB load
// (lane-linear 16 bytes) instead of 64 scattered 16-byte pieces of 32 different rows (measured in round 3: a scattered prologue cost ~10 us of a 31 us launch).  perm: plain (lane-half h's accumulators = channels 16 h + r) or operand
// (c2f_c32.hip: accumulators = the next MFMA's B fragments).
int frag_row(int rho, bool operand) {
  if (!operand) return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3);
  const int q = rho >> 3, h = (rho >> 2) & 1, i = rho & 3;
  return 16 * (q >> 1) + 8 * h + 4 * (q & 1) + i;
}
std::vector<half_t> frag_pack(const half_t* rows, int Kpad, const std::vector<std::pair<int, int>>& frags, bool operand) {
  std::vector<half_t> out(frags.size() * 512);
  for (size_t f = 0; f < frags.size(); ++f)
    for (int lane = 0; lane < 64; ++lane) {
      const half_t* src = rows + (size_t)(frags[f].first + frag_row(lane & 31, operand)) * Kpad + frags[f].second + 8 * (lane >> 5);
      for (int j = 0; j < 8; ++j) out[(f * 64 + lane) * 8 + j] = src[j];
    }
  return out;
}
// [32-row channel block][16-deep K slice] over rows x K: the fragment list of every weights-in-registers kernel but
// head_tail.hip's.  With rows = K = 4 n it is also proto_phase_wreg.hip's [phase][channel block][slice] of the composed phases.
std::vector<std::pair<int, int>> frag_grid(int rows, int K) {
  std::vector<std::pair<int, int>> f;
  for (int r = 0; r < rows; r += 32)
    for (int k = 0; k < K; k += 16) f.push_back({r, k});
  return f;
}

// the fragment lists of the kernels, by conv shape (empty = none of them takes this conv)
std::vector<std::pair<int, int>> frag_list(int k, int cin, int cout) {
  // (64 -> 64 and 128 -> 128 3x3 convs had lists for conv3x3_c64r / conv3x3_c128r: measured no gain in round 3, deleted in round 4;
  // such a conv gets fragments only when a row-slab launch uses it -- PhysConv::planes, planes_frag_pack)
  const bool taken = (k == 3 && cin == 64 && cout == 128) ||                   // conv3x3_s2c64
                     (k == 3 && cin == 32 && (cout == 64 || cout == 32)) ||    // conv_stem_c2 (model.1, operand row order), c2f_c32
                     (k == 1 && (cin == 128 || cin == 192 || cin == 256 || cin == 384 || cin == 512) && cout % 128 == 0 && cout <= 512);   // conv1x1_wreg
  return taken ? frag_grid(cout, k * k * cin) : std::vector<std::pair<int, int>>();
}

// head_tail.hip: the 18 fragments of a head level's block-diagonal matrix (head_tail_layout) -- box rows 0-63 over K 0-63, class
// rows from 64 over K 64-191 (the rows behind them are coefficient rows: zero there), coefficient rows from 64 + nc over K 192-223
std::vector<std::pair<int, int>> head_level_frags(int nc) {
  std::vector<std::pair<int, int>> f = frag_grid(64, 64);
  for (int sl = 0; sl < 8; ++sl) f.push_back({64, 64 + 16 * sl});
  for (int sl = 0; sl < 2; ++sl) f.push_back({64 + nc, 192 + 16 * sl});
  return f;
}

// device copy of a fragment-ordered weight list (allocated on first use)
hipError_t put_frags(half_t** dst, const std::vector<half_t>& fp) {
  const size_t bytes = fp.size() * sizeof(half_t);
  const hipError_t st = *dst ? hipSuccess : hipMalloc((void**)dst, bytes);
  return st != hipSuccess ? st : hipMemcpy(*dst, fp.data(), bytes, hipMemcpyHostToDevice);
}

// the 1x1 conv in the epilogue of the kernels that hold it in registers: proto.cv3 (32 x 128, proto_phase_wreg.hip), and the
// C2f cv1 after a stride-2 conv (64 x 64 on conv_stem_c2, 128 x 128 on conv3x3_s2c64)
std::vector<std::pair<int, int>> epilogue_frags(int cout2, int k) { return frag_grid(cout2, k); }

// ConvTranspose2d(2x2, s2, bias) followed by Conv3x3 (no activation between them) as four 2x2 phase convs over the low-resolution input
// (see build_segment_head): fp16 rows [4 n (padded to cout_pad)][Kpad], K = (a * 2 + b) * n + cin, and the [9 border classes][n] bias table.
void compose_proto_phases(int n, const float* wtp, const float* btp, const float* w3p, const float* b3p, int cout_pad, int Kpad,
                          std::vector<half_t>& rows, std::vector<float>& btab) {
    // Weff[q][co][(a*2+b)*n + ci] = sum over the (kh, kw) of phase q = py*2+px that fall on low-res offset (a, b):
    //   t = py + kh - 1, low-res row offset floor(t / 2) = a - 1 + py, dy = t mod 2 (same for columns)
    //   Weff += sum_c W3[co, c, kh, kw] * Wt[ci, c, dy, dx]
    rows.assign((size_t)cout_pad * Kpad, (half_t)0.f);
    std::vector<double> acc((size_t)n * n);
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px)
        for (int aa = 0; aa < 2; ++aa)
          for (int bb = 0; bb < 2; ++bb) {
            std::fill(acc.begin(), acc.end(), 0.0);
            for (int kh = 0; kh < 3; ++kh) {
              const int ty = py + kh - 1, ry = (ty < 0 ? -1 : ty / 2), dy = ty & 1;
              if (ry + 1 - py != aa) continue;
              for (int kw = 0; kw < 3; ++kw) {
                const int tx = px + kw - 1, rx = (tx < 0 ? -1 : tx / 2), dx = tx & 1;
                if (rx + 1 - px != bb) continue;
                for (int co = 0; co < n; ++co)
                  for (int c = 0; c < n; ++c) {
                    const double w3 = w3p[(((size_t)co * n + c) * 3 + kh) * 3 + kw];
                    if (w3 == 0.0) continue;
                    const float* wt = wtp;
                    double* ar = &acc[(size_t)co * n];
                    for (int cin = 0; cin < n; ++cin) ar[cin] += w3 * wt[(((size_t)cin * n + c) * 2 + dy) * 2 + dx];
                  }
              }
            }
            const int q = py * 2 + px;
            for (int co = 0; co < n; ++co)
              for (int cin = 0; cin < n; ++cin)
                rows[(size_t)(q * n + co) * Kpad + (aa * 2 + bb) * n + cin] = (half_t)(float)acc[(size_t)co * n + cin];
          }
    // bias table [ry*3+rx][co]: b3 + sum over the taps of the 3x3 window that lie inside the hi-res image of W3 . bt
    btab.assign((size_t)9 * n, 0.f);
    for (int ry = 0; ry < 3; ++ry)
      for (int rx = 0; rx < 3; ++rx)
        for (int co = 0; co < n; ++co) {
          double sacc = b3p[co];
          for (int kh = 0; kh < 3; ++kh) {
            if ((ry == 0 && kh == 0) || (ry == 2 && kh == 2)) continue;
            for (int kw = 0; kw < 3; ++kw) {
              if ((rx == 0 && kw == 0) || (rx == 2 && kw == 2)) continue;
              for (int c = 0; c < n; ++c) sacc += (double)w3p[(((size_t)co * n + c) * 3 + kh) * 3 + kw] * btp[c];
            }
          }
          btab[(size_t)(ry * 3 + rx) * n + co] = (float)sacc;
        }
}

// Fragment order of the row-slab 3x3 kernels (conv3x3_planes.hip): [channel block cb][input plane p][tap][K slice s], plain row
// permutation -- the K-loop order of one wave, so that its weight stream is one linearly advancing pointer (2 KiB per step).
std::vector<half_t> planes_frag_pack(const half_t* rows, int Kpad, int cin, int cblocks) {
  std::vector<std::pair<int, int>> fl;
  for (int cb = 0; cb < cblocks; ++cb)
    for (int p = 0; p < cin / 32; ++p)
      for (int tap = 0; tap < 9; ++tap)
        for (int s = 0; s < 2; ++s) fl.push_back({32 * cb, tap * cin + 32 * p + 16 * s});
  return frag_pack(rows, Kpad, fl, false);
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
  if (const char* mm = getenv("M355_HEADTAIL_MAXM")) e->headtail_maxm = atol(mm);   // testing: force a head level ineligible
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
    std::vector<half_t> r2((size_t)p.cout2 * p.cout);
    for (size_t i = 0; i < r2.size(); ++i) r2[i] = (half_t)w[i];
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
  } else if (ci.cin == 3) {  // stem: [cout][32] fp16, k = (kh*3+kw)*3+c; 1/255 is applied in the kernel's epilogue
    std::vector<half_t> sw((size_t)ci.cout * 32, (half_t)0.f);
    for (int co = 0; co < ci.cout; ++co)
      for (int c = 0; c < 3; ++c)
        for (int kh = 0; kh < 3; ++kh)
          for (int kw = 0; kw < 3; ++kw)
            sw[(size_t)co * 32 + (kh * 3 + kw) * 3 + c] = (half_t)w[((co * 3 + c) * 3 + kh) * 3 + kw];
    HIP_TRY(e, hipMemcpy(p.stem_w, sw.data(), sw.size() * sizeof(half_t), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(p.bias, bias, ci.cout * sizeof(float), hipMemcpyHostToDevice));
  } else if (ci.transposed) {  // (cin,cout,2,2) -> virtual channel (dy*2+dx)*cout + co, K = cin
    std::vector<half_t> rows((size_t)4 * ci.cout * p.Kpad, (half_t)0.f);
    for (int c = 0; c < ci.cin; ++c)
      for (int co = 0; co < ci.cout; ++co)
        for (int dy = 0; dy < 2; ++dy)
          for (int dx = 0; dx < 2; ++dx)
            rows[(size_t)((dy * 2 + dx) * ci.cout + co) * p.Kpad + c] =
                (half_t)w[(((size_t)c * ci.cout + co) * 2 + dy) * 2 + dx];
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
        const int cbl = (p.cout + 63) / 64 * 2;
        std::vector<half_t> padded((size_t)cbl * 32 * p.Kpad, (half_t)0.f);
        HIP_TRY(e, hipMemcpy(padded.data(), p.w, (size_t)p.cout * p.Kpad * sizeof(half_t), hipMemcpyDeviceToHost));
        HIP_TRY(e, put_frags(&p.wf, planes_frag_pack(padded.data(), p.Kpad, p.cin, cbl)));
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
      if (!ha.wf || !head_tail_ok(ha) || (e->headtail_maxm > 0 && ha.M > e->headtail_maxm)) all = false;
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
        if (op.kind != OP_PHASE) a.tileq = knobs().static_tiles ? nullptr : e->tileq + 4 * oi;
        if (op.stemfuse >= 0) {
          const StemArgs sa = stem_args(e, e->ops[op.stemfuse], Bq, b0, d_in);
          const bool stem2 = getenv("M355_NO_STEM2") == nullptr;  // two-team form (conv_stem_c2.hip, the default); read per launch: tests toggle it
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

// ------------------------------- per-op entry points (unit parity) -------------------------------

static int set_err(int code, const std::string& m) {
  g_err = m;
  return code;
}
#define HIP_TRYG(call)                                                                                \
  do {                                                                                                \
    hipError_t _st = (call);                                                                          \
    if (_st != hipSuccess) return set_err(M355_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_st)); \
  } while (0)

static int conv_op_common(const void* d_x, int B, int H, int W, int cin, const float* h_w, const float* h_bias,
                          int cout, int k, int stride, int act, const void* d_res, void* d_y, int out_f32,
                          int force_tile, int transposed, void* stream) {
  if (!d_x || !h_w || !h_bias || !d_y) return set_err(M355_ERR_INVALID, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int cout_v = transposed ? 4 * cout : cout;
  const int cout_pad = conv_cout_pad(cout_v);
  if (force_tile >= 0) {
    // A forced tile must be one a launcher implements, and its channel extent must stay inside the cout_pad weight / bias
    // rows allocated below (an experimental 256-row channel tile against 128-row padding was a GPU page fault: DESIGN.md)
    int bch = 0, bpx = 0;
    if (!conv_forced_tile_extent(force_tile & 0xff, cout_v, &bch, &bpx))
      return set_err(M355_ERR_INVALID, "unknown forced tile id " + std::to_string(force_tile & 0xff));
    if ((force_tile & 0xff) == TILE_PLANES && (transposed || k != 3 || (stride != 1 && stride != 2) || cin % 32 || out_f32))
      return set_err(M355_ERR_INVALID, "forced tile TILE_PLANES takes 3x3 convs of stride 1 or 2 with cin % 32 == 0 and fp16 output only");
    if ((cout_v + bch - 1) / bch * bch > cout_pad)
      return set_err(M355_ERR_INVALID, "forced tile reads " + std::to_string((cout_v + bch - 1) / bch * bch) +
                                           " weight rows, the packed buffer has " + std::to_string(cout_pad));
  }
  if (cin <= 0 || cout <= 0 || B <= 0 || H <= 0 || W <= 0) return set_err(M355_ERR_INVALID, "non-positive shape");
  const int Kpad = transposed ? conv_kpad(cin, 1) : conv_kpad(cin, k);
  std::vector<half_t> rows((size_t)cout_pad * Kpad, (half_t)0.f);
  std::vector<float> bias(cout_pad, 0.f);
  if (transposed) {
    for (int c = 0; c < cin; ++c)
      for (int co = 0; co < cout; ++co)
        for (int dy = 0; dy < 2; ++dy)
          for (int dx = 0; dx < 2; ++dx)
            rows[(size_t)((dy * 2 + dx) * cout + co) * Kpad + c] = (half_t)h_w[(((size_t)c * cout + co) * 2 + dy) * 2 + dx];
  } else {
    pack_conv_rows(h_w, cout, cin, k, Kpad, 0, rows);
  }
  for (int i = 0; i < cout; ++i) bias[i] = h_bias[i];
  half_t *dw = nullptr, *dz = nullptr;
  float* db = nullptr;
  HIP_TRYG(hipMalloc((void**)&dw, rows.size() * sizeof(half_t)));
  HIP_TRYG(hipMalloc((void**)&db, bias.size() * sizeof(float)));
  HIP_TRYG(hipMalloc((void**)&dz, 256));
  HIP_TRYG(hipMemset(dz, 0, 256));
  HIP_TRYG(hipMemcpy(dw, rows.data(), rows.size() * sizeof(half_t), hipMemcpyHostToDevice));
  HIP_TRYG(hipMemcpy(db, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
  half_t* dwf = nullptr;
  if (!transposed) {
    const auto fl = frag_list(k, cin, cout);
    if (!fl.empty()) {
      const auto fp = frag_pack(rows.data(), Kpad, fl, false);
      HIP_TRYG(hipMalloc((void**)&dwf, fp.size() * sizeof(half_t)));
      HIP_TRYG(hipMemcpy(dwf, fp.data(), fp.size() * sizeof(half_t), hipMemcpyHostToDevice));
    }
  }
  ConvArgs a{};
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * cin; a.ldx = cin; a.Hi = H; a.Wi = W; a.Cin = cin;
  a.w = dw; a.Kpad = Kpad; a.bias = db; a.zero = dz; a.act = act; a.out_f32 = out_f32; a.w_rows = cout_pad; a.wf = dwf;
  a.y = d_y;
  if (transposed) {
    a.ksize = 1; a.stride = 1; a.pad = 0; a.Ho = H; a.Wo = W; a.Cout = 4 * cout; a.convt_co = cout;
    a.y_bstride = (long)4 * H * W * cout; a.ldy = cout;
  } else {
    a.ksize = k; a.stride = stride; a.pad = k / 2;
    a.Ho = (H + 2 * a.pad - k) / stride + 1; a.Wo = (W + 2 * a.pad - k) / stride + 1; a.Cout = cout;
    a.y_bstride = (long)a.Ho * a.Wo * cout; a.ldy = cout;
    if (d_res) { a.res = (const half_t*)d_res; a.r_bstride = a.y_bstride; a.ldr = cout; }
  }
  a.M = B * a.Ho * a.Wo;
  a.dbg = force_tile >= 0 ? (force_tile >> 8) : 0;
  unsigned long long* d_st = nullptr;
  const char* st_path = getenv("M355_STAMPS");
  const size_t st_n = (size_t)1 << 20;
  if (st_path) {
    HIP_TRYG(hipMalloc((void**)&d_st, st_n * 8));
    HIP_TRYG(hipMemset(d_st, 0, st_n * 8));
    a.stamps = d_st;
  }
  int rc = 0;
  half_t* dpf = nullptr;
  if (force_tile >= 0 && (force_tile & 0xff) == TILE_PLANES) {   // row-slab kernel (conv3x3_planes.hip), single-conv mode
    const int cbl = (cout + 63) / 64 * 2;
    std::vector<half_t> padded((size_t)cbl * 32 * Kpad, (half_t)0.f);
    std::copy(rows.begin(), rows.begin() + (size_t)cout * Kpad, padded.begin());
    const auto fp = planes_frag_pack(padded.data(), Kpad, cin, cbl);
    HIP_TRYG(hipMalloc((void**)&dpf, fp.size() * sizeof(half_t)));
    HIP_TRYG(hipMemcpy(dpf, fp.data(), fp.size() * sizeof(half_t), hipMemcpyHostToDevice));
    PlanesArgs pa{};
    pa.x = a.x; pa.x_bstride = a.x_bstride; pa.ldx = a.ldx; pa.H = H; pa.W = W; pa.B = B; pa.Cin = cin; pa.Cout = cout; pa.stride = stride;
    pa.wfb = dpf; pa.cblocks_b = cbl; pa.bb = db; pa.y = (half_t*)d_y; pa.y_bstride = a.y_bstride; pa.ldy = a.ldy;
    pa.res = a.res; pa.r_bstride = a.r_bstride; pa.ldr = a.ldr; pa.act = act; pa.stamps = d_st;
    rc = conv3x3_planes_ok(pa) ? launch_conv3x3_planes(pa, s) : -1;
    if (const char* reps = getenv("M355_BNECK_REPS")) {
      const int n = atoi(reps);
      hipEvent_t e0, e1;
      if (rc == 0 && n > 0 && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < n && rc == 0; ++i) rc = launch_conv3x3_planes(pa, s);
        (void)hipEventRecord(e1, s);
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        fprintf(stderr, "conv3x3_planes B=%d %dx%d %d->%d: %.2f us per launch (%d launches)\n", B, H, W, cin, cout, ms * 1e3f / n, n);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
      }
    }
  } else
  for (int rep = 0; rep < (a.dbg ? 5 : 1); ++rep)
    rc = (force_tile >= 0 && (force_tile & 0xff) == TILE_W1) ? launch_conv1x1_wreg(a, s)
         : (force_tile >= 0 && (force_tile & 0xff) == TILE_C32)
             ? launch_conv3x3_c32(a, s)
             : ((force_tile >= 0 && (force_tile & 0xff) >= TILE_HALO) ? launch_conv3x3_halo(a, (force_tile & 0xff) - TILE_HALO, s)
                                                                       : launch_conv_igemm(a, force_tile, s));
  hipError_t se = hipStreamSynchronize(s);
  if (st_path && se == hipSuccess) {
    std::vector<unsigned long long> h(st_n);
    (void)hipMemcpy(h.data(), d_st, st_n * 8, hipMemcpyDeviceToHost);
    FILE* f = fopen(st_path, "wb");
    if (f) { fwrite(h.data(), 8, st_n, f); fclose(f); }
  }
  if (d_st) (void)hipFree(d_st);
  (void)hipFree(dw); (void)hipFree(db); (void)hipFree(dz);
  if (dwf) (void)hipFree(dwf);
  if (dpf) (void)hipFree(dpf);
  if (rc != 0) return set_err(M355_ERR_HIP, "conv launch failed: " + std::to_string(rc));
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string("conv kernel: ") + hipGetErrorString(se));
  return M355_OK;
}

int m355_conv2d_fwd(const void* d_x, int B, int H, int W, int cin, const float* h_w, const float* h_bias, int cout,
                    int k, int stride, int act, const void* d_res, void* d_y, int out_f32, int force_tile,
                    void* stream) {
  return conv_op_common(d_x, B, H, W, cin, h_w, h_bias, cout, k, stride, act, d_res, d_y, out_f32, force_tile, 0,
                        stream);
}

int m355_c2f_c32_fwd(const void* d_x, int B, int H, int W, const float* h_wa, const float* h_ba, const float* h_wb,
                     const float* h_bb, const float* h_wc, const float* h_bc, int shortcut, void* d_y, void* stream) {
  if (!d_x || !d_y || !h_wa || !h_ba || !h_wb || !h_bb || !h_wc || !h_bc) return set_err(M355_ERR_INVALID, "null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || H % 8 || W % 16) return set_err(M355_ERR_INVALID, "H must be a multiple of 8 and W of 16");
  hipStream_t s = (hipStream_t)stream;
  const int kp3 = conv_kpad(32, 3), kp1 = conv_kpad(96, 1);
  std::vector<half_t> ra((size_t)32 * kp3, (half_t)0.f), rb((size_t)32 * kp3, (half_t)0.f), rc_((size_t)64 * kp1, (half_t)0.f);
  pack_conv_rows(h_wa, 32, 32, 3, kp3, 0, ra);
  pack_conv_rows(h_wb, 32, 32, 3, kp3, 0, rb);
  pack_conv_rows(h_wc, 64, 96, 1, kp1, 0, rc_);
  std::vector<float> bias(128);
  for (int i = 0; i < 32; ++i) { bias[i] = h_ba[i]; bias[32 + i] = h_bb[i]; }
  for (int i = 0; i < 64; ++i) bias[64 + i] = h_bc[i];
  half_t* dw = nullptr;
  float* db = nullptr;
  const size_t na = ra.size(), nb = rb.size(), ncw = rc_.size();
  HIP_TRYG(hipMalloc((void**)&dw, (na + nb + ncw) * sizeof(half_t)));
  HIP_TRYG(hipMalloc((void**)&db, bias.size() * sizeof(float)));
  HIP_TRYG(hipMemcpy(dw, ra.data(), na * sizeof(half_t), hipMemcpyHostToDevice));
  HIP_TRYG(hipMemcpy(dw + na, rb.data(), nb * sizeof(half_t), hipMemcpyHostToDevice));
  HIP_TRYG(hipMemcpy(dw + na + nb, rc_.data(), ncw * sizeof(half_t), hipMemcpyHostToDevice));
  HIP_TRYG(hipMemcpy(db, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
  half_t* dfr = nullptr;
  {
    const auto fl = frag_list(3, 32, 32);
    auto fa = frag_pack(ra.data(), kp3, fl, false);
    const auto fb = frag_pack(rb.data(), kp3, fl, true);
    fa.insert(fa.end(), fb.begin(), fb.end());
    HIP_TRYG(hipMalloc((void**)&dfr, fa.size() * sizeof(half_t)));
    HIP_TRYG(hipMemcpy(dfr, fa.data(), fa.size() * sizeof(half_t), hipMemcpyHostToDevice));
  }
  C2fC32Args a{};
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * 64; a.ldx = 64; a.H = H; a.W = W; a.B = B;
  a.wa = dw; a.wb = dw + na; a.wc = dw + na + nb; a.kpad_a = kp3; a.kpad_b = kp3; a.kpad_c = kp1;
  a.waf = dfr; a.wbf = dfr + 18 * 512;
  a.ba = db; a.bb = db + 32; a.bc = db + 64;
  a.y = (half_t*)d_y; a.y_bstride = (long)H * W * 64; a.ldy = 64; a.shortcut = shortcut;
  const int rc = launch_c2f_c32(a, s);
  const hipError_t se = hipStreamSynchronize(s);
  (void)hipFree(dw); (void)hipFree(db); (void)hipFree(dfr);
  if (rc != 0) return set_err(M355_ERR_HIP, "c2f_c32 launch failed: " + std::to_string(rc));
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string("c2f_c32 kernel: ") + hipGetErrorString(se));
  return M355_OK;
}

int m355_bneck_pair_fwd(const void* d_x, int B, int H, int W, int C, int ldx, const float* h_wa, const float* h_ba, const float* h_wb,
                        const float* h_bb, int shortcut, void* d_y, int ldy, void* stream) {
  if (!d_x || !d_y || !h_wa || !h_ba || !h_wb || !h_bb) return set_err(M355_ERR_INVALID, "null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || ldx < C || ldy < C) return set_err(M355_ERR_INVALID, "bad shape");
  hipStream_t s = (hipStream_t)stream;
  if (C % 32) return set_err(M355_ERR_INVALID, "C must be a multiple of 32");
  const int kp = conv_kpad(C, 3), rows = conv_cout_pad(C), cbl = C / 32;
  std::vector<half_t> ra((size_t)rows * kp, (half_t)0.f), rb((size_t)rows * kp, (half_t)0.f);
  pack_conv_rows(h_wa, C, C, 3, kp, 0, ra);
  pack_conv_rows(h_wb, C, C, 3, kp, 0, rb);
  const std::vector<half_t> fa = planes_frag_pack(ra.data(), kp, C, cbl), fb = planes_frag_pack(rb.data(), kp, C, cbl);
  std::vector<float> bias(2 * rows, 0.f);
  for (int i = 0; i < C; ++i) { bias[i] = h_ba[i]; bias[rows + i] = h_bb[i]; }
  half_t* dw = nullptr;
  float* db = nullptr;
  HIP_TRYG(hipMalloc((void**)&dw, (fa.size() + fb.size()) * sizeof(half_t)));
  HIP_TRYG(hipMalloc((void**)&db, bias.size() * sizeof(float)));
  HIP_TRYG(hipMemcpy(dw, fa.data(), fa.size() * sizeof(half_t), hipMemcpyHostToDevice));
  HIP_TRYG(hipMemcpy(dw + fa.size(), fb.data(), fb.size() * sizeof(half_t), hipMemcpyHostToDevice));
  HIP_TRYG(hipMemcpy(db, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
  PlanesArgs a{};
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * ldx; a.ldx = ldx; a.H = H; a.W = W; a.B = B; a.Cin = C; a.Cout = C;
  a.wfa = dw; a.wfb = dw + fa.size(); a.cblocks_a = a.cblocks_b = cbl;
  a.ba = db; a.bb = db + rows;
  a.y = (half_t*)d_y; a.y_bstride = (long)H * W * ldy; a.ldy = ldy; a.act = 1; a.stride = 1;
  if (shortcut) { a.res = a.x; a.r_bstride = a.x_bstride; a.ldr = ldx; }
  unsigned long long* d_st = nullptr;
  const char* st_path = getenv("M355_STAMPS");
  const size_t st_n = (size_t)256 * 4 * 8 * 2;
  if (st_path) {
    HIP_TRYG(hipMalloc((void**)&d_st, st_n * 8));
    HIP_TRYG(hipMemset(d_st, 0, st_n * 8));
    a.stamps = d_st;
  }
  const bool ok = bneck_pair_ok(a);
  int rc = ok ? launch_bneck_pair(a, s) : -1;
  if (const char* reps = getenv("M355_BNECK_REPS")) {   // diagnostic: average launch time over n back-to-back launches -> stderr
    const int n = atoi(reps);
    hipEvent_t e0, e1;
    if (rc == 0 && n > 0 && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
      (void)hipEventRecord(e0, s);
      for (int i = 0; i < n && rc == 0; ++i) rc = launch_bneck_pair(a, s);
      (void)hipEventRecord(e1, s);
      (void)hipEventSynchronize(e1);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, e0, e1);
      fprintf(stderr, "bneck_pair B=%d %dx%d C=%d: %.2f us per launch (%d launches)\n", B, H, W, C, ms * 1e3f / n, n);
      (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
  }
  const hipError_t se = hipStreamSynchronize(s);
  if (st_path && se == hipSuccess && rc == 0) {
    std::vector<unsigned long long> hst(st_n);
    (void)hipMemcpy(hst.data(), d_st, st_n * 8, hipMemcpyDeviceToHost);
    FILE* f = fopen(st_path, "wb");
    if (f) { fwrite(hst.data(), 8, st_n, f); fclose(f); }
  }
  if (d_st) (void)hipFree(d_st);
  (void)hipFree(dw); (void)hipFree(db);
  if (!ok) return set_err(M355_ERR_INVALID, "bneck_pair: shape not eligible (C in {64, 128}, slab geometry must fit LDS)");
  if (rc != 0) return set_err(M355_ERR_HIP, "bneck_pair launch failed: " + std::to_string(rc));
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string("bneck_pair kernel: ") + hipGetErrorString(se));
  return M355_OK;
}

// ---- per-op parity entries of the round-3 fused launches (each: host weights packed as m355_set_conv_weights packs them, through
// the same fragment lists, one launch, stream synchronised) ---------------------------------------------------------------------
}  // extern "C" (C++ helpers follow)
namespace {
struct DevBuf {   // device allocations of one entry call, freed on scope exit
  std::vector<void*> p;
  ~DevBuf() { for (void* q : p) (void)hipFree(q); }
  template <class T>
  T* put(const std::vector<T>& h) {
    void* d = nullptr;
    if (hipMalloc(&d, h.size() * sizeof(T) + 16) != hipSuccess) return nullptr;
    p.push_back(d);
    if (hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return (T*)d;
  }
  void* raw(size_t bytes) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes + 16) != hipSuccess) return nullptr;
    p.push_back(d);
    (void)hipMemset(d, 0, bytes + 16);
    return d;
  }
};
std::vector<half_t> to_half_vec(const float* w, size_t n) {
  std::vector<half_t> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = (half_t)w[i];
  return r;
}
int finish_entry(int rc, hipStream_t s, const char* what) {
  const hipError_t se = hipStreamSynchronize(s);
  if (rc != 0) return set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, std::string(what) + ": launch refused / failed (" + std::to_string(rc) + ")");
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string(what) + " kernel: " + hipGetErrorString(se));
  return M355_OK;
}
}  // namespace
extern "C" {

int m355_s2c64_cv1_fwd(const void* d_x, int B, int H, int W, const float* h_w3, const float* h_b3, const float* h_w1, const float* h_b1,
                       void* d_y, void* stream) {
  if (!d_x || !d_y || !h_w3 || !h_b3 || !h_w1 || !h_b1 || B < 1 || H < 2 || W < 2) return set_err(M355_ERR_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int kp = conv_kpad(64, 3);
  std::vector<half_t> rows((size_t)conv_cout_pad(128) * kp, (half_t)0.f);
  pack_conv_rows(h_w3, 128, 64, 3, kp, 0, rows);
  const std::vector<half_t> r2 = to_half_vec(h_w1, (size_t)128 * 128);
  DevBuf d;
  ConvArgs a{};
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * 64; a.ldx = 64; a.Hi = H; a.Wi = W; a.Cin = 64;
  a.w = d.put(rows); a.Kpad = kp; a.wf = d.put(frag_pack(rows.data(), kp, frag_list(3, 64, 128), false));
  a.w2 = d.put(r2); a.wf2 = d.put(frag_pack(r2.data(), 128, epilogue_frags(128, 128), false));
  std::vector<float> b3(conv_cout_pad(128), 0.f), b1(128);
  for (int i = 0; i < 128; ++i) { b3[i] = h_b3[i]; b1[i] = h_b1[i]; }
  a.bias = d.put(b3); a.bias2 = d.put(b1); a.cout2 = 128; a.zero = (const half_t*)d.raw(256);
  a.ksize = 3; a.stride = 2; a.pad = 1; a.Ho = H / 2; a.Wo = W / 2; a.Cout = 128; a.act = 1; a.w_rows = conv_cout_pad(128);
  a.y = d_y; a.y_bstride = (long)a.Ho * a.Wo * 128; a.ldy = 128; a.M = B * a.Ho * a.Wo;
  if (!a.w || !a.wf || !a.w2 || !a.wf2 || !a.bias || !a.bias2 || !a.zero) return set_err(M355_ERR_HIP, "allocation failed");
  return finish_entry(conv_s2c64_cv1_ok(a) ? launch_conv_s2c64_cv1(a, s) : -1, s, "conv3x3_s2c64 + 1x1");
}

int m355_stem_s2c32_cv1_fwd(const void* d_in_u8, int B, int H, int W, const float* h_w0, const float* h_b0, const float* h_w1,
                            const float* h_b1, const float* h_w2, const float* h_b2, void* d_y, int two_team, void* stream) {
  if (!d_in_u8 || !d_y || !h_w0 || !h_b0 || !h_w1 || !h_b1 || !h_w2 || !h_b2 || B < 1 || H < 4 || W < 4) return set_err(M355_ERR_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  std::vector<half_t> sw((size_t)32 * 32, (half_t)0.f);
  for (int co = 0; co < 32; ++co)
    for (int c = 0; c < 3; ++c)
      for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) sw[(size_t)co * 32 + (kh * 3 + kw) * 3 + c] = (half_t)h_w0[((co * 3 + c) * 3 + kh) * 3 + kw];
  const int kp = conv_kpad(32, 3);
  std::vector<half_t> rows((size_t)conv_cout_pad(64) * kp, (half_t)0.f);
  pack_conv_rows(h_w1, 64, 32, 3, kp, 0, rows);
  const std::vector<half_t> r2 = to_half_vec(h_w2, (size_t)64 * 64);
  DevBuf d;
  StemArgs st{};
  st.x = (const uint8_t*)d_in_u8; st.B = B; st.H = H; st.W = W; st.w16 = d.put(sw);
  st.bias = d.put(std::vector<float>(h_b0, h_b0 + 32));
  st.y = (half_t*)d.raw((size_t)B * (H / 2) * (W / 2) * 32 * 2); st.y_bstride = (long)(H / 2) * (W / 2) * 32; st.ldy = 32; st.Cout = 32;
  ConvArgs a{};
  a.x = st.y; a.x_bstride = st.y_bstride; a.ldx = 32; a.Hi = H / 2; a.Wi = W / 2; a.Cin = 32;
  a.w = d.put(rows); a.Kpad = kp; a.wf = d.put(frag_pack(rows.data(), kp, frag_list(3, 32, 64), true));
  a.w2 = d.put(r2); a.wf2 = d.put(frag_pack(r2.data(), 64, epilogue_frags(64, 64), false));
  std::vector<float> b1(conv_cout_pad(64), 0.f);
  for (int i = 0; i < 64; ++i) b1[i] = h_b1[i];
  a.bias = d.put(b1); a.bias2 = d.put(std::vector<float>(h_b2, h_b2 + 64)); a.cout2 = 64; a.zero = (const half_t*)d.raw(256);
  a.ksize = 3; a.stride = 2; a.pad = 1; a.Ho = H / 4; a.Wo = W / 4; a.Cout = 64; a.act = 1; a.w_rows = conv_cout_pad(64);
  a.y = d_y; a.y_bstride = (long)a.Ho * a.Wo * 64; a.ldy = 64; a.M = B * a.Ho * a.Wo;
  if (!st.w16 || !st.bias || !st.y || !a.w || !a.wf || !a.w2 || !a.wf2 || !a.bias || !a.bias2 || !a.zero) return set_err(M355_ERR_HIP, "allocation failed");
  int rc = -1;
  if (two_team) rc = stem_s2c32_v2_ok(a, st) ? launch_stem_s2c32_v2(a, st, s) : -1;
  else rc = stem_s2c32_ok(a, st) ? launch_stem_s2c32(a, st, s) : -1;
  return finish_entry(rc, s, "stem + conv3x3_s2c32 + 1x1");
}

int m355_proto_phase_fwd(const void* d_x, int B, int H, int W, const float* h_wt, const float* h_bt, const float* h_w3, const float* h_b3,
                         const float* h_wc, const float* h_bc, void* d_y, void* stream) {
  if (!d_x || !d_y || !h_wt || !h_bt || !h_w3 || !h_b3 || !h_wc || !h_bc || B < 1) return set_err(M355_ERR_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int n = 128, kp = conv_kpad(4 * n, 1), cp = conv_cout_pad(4 * n);
  std::vector<half_t> rows;
  std::vector<float> btab;
  compose_proto_phases(n, h_wt, h_bt, h_w3, h_b3, cp, kp, rows, btab);
  const std::vector<half_t> r2 = to_half_vec(h_wc, (size_t)32 * 128);
  DevBuf d;
  ConvArgs a{};
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * n; a.ldx = n; a.Hi = H; a.Wi = W; a.Cin = n;
  a.w = d.put(rows); a.Kpad = kp; a.bias = d.put(btab); a.wf = d.put(frag_pack(rows.data(), kp, frag_grid(4 * n, 4 * n), false));
  a.w2 = d.put(r2); a.wf2 = d.put(frag_pack(r2.data(), 128, epilogue_frags(32, 128), false)); a.bias2 = d.put(std::vector<float>(h_bc, h_bc + 32)); a.cout2 = 32;
  a.zero = (const half_t*)d.raw(256); a.act = 1; a.ksize = 2; a.stride = 1; a.pad = 0; a.phase = 1;
  a.Ho = H; a.Wo = W; a.Cout = 4 * n; a.convt_co = n; a.w_rows = cp;
  a.y = d_y; a.y_bstride = (long)4 * H * W * 32; a.ldy = 32; a.M = B * H * W;
  if (!a.w || !a.wf || !a.w2 || !a.wf2 || !a.bias || !a.bias2 || !a.zero) return set_err(M355_ERR_HIP, "allocation failed");
  return finish_entry(proto_phase_wreg_ok(a) ? launch_proto_phase_wreg(a, s) : -1, s, "proto_phase_wreg");
}

int m355_head_tail_fwd(const void* d_x, int B, int H, int W, int nc, float stride, const float* h_w2, const float* h_b2, const float* h_w3,
                       const float* h_b3, const float* h_w4, const float* h_b4, float* d_preds, int A, int level_off, void* stream) {
  if (!d_x || !d_preds || !h_w2 || !h_b2 || !h_w3 || !h_b3 || !h_w4 || !h_b4 || B < 1 || nc < 1 || nc > 32) return set_err(M355_ERR_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int cout = 64 + nc + 32, kp = conv_kpad(224, 1), rows_pad = conv_cout_pad(cout);
  std::vector<half_t> rows((size_t)rows_pad * kp, (half_t)0.f);
  pack_conv_rows(h_w2, 64, 64, 1, kp, 0, rows, 0);           // box rows over K 0 .. 63
  pack_conv_rows(h_w3, nc, 128, 1, kp, 64, rows, 64);        // class rows over K 64 .. 191
  pack_conv_rows(h_w4, 32, 32, 1, kp, 64 + nc, rows, 192);   // coefficient rows over K 192 .. 223
  if (64 + nc + 32 > rows_pad) return set_err(M355_ERR_INVALID, "row padding");
  std::vector<float> bias(rows_pad, 0.f);
  for (int i = 0; i < 64; ++i) bias[i] = h_b2[i];
  for (int i = 0; i < nc; ++i) bias[64 + i] = h_b3[i];
  for (int i = 0; i < 32; ++i) bias[64 + nc + i] = h_b4[i];
  DevBuf d;
  HeadTailArgs ha{};
  ha.x = (const half_t*)d_x; ha.ldx = 224; ha.M = (long)B * H * W; ha.HW = H * W; ha.W = W; ha.stride = stride;
  ha.A = A; ha.level_off = level_off; ha.nc = nc; ha.nm = 32;
  ha.wf = d.put(frag_pack(rows.data(), kp, head_level_frags(nc), false)); ha.bias = d.put(bias); ha.preds = d_preds;
  if (!ha.wf || !ha.bias) return set_err(M355_ERR_HIP, "allocation failed");
  return finish_entry(head_tail_ok(ha) ? launch_head_tail(ha, s) : -1, s, "head_tail");
}

// Phase form of the stride-2 3x3 input gradient (four 2x2 phase convs over dY, conv_igemm.hip) that launch_conv_igemm can tile,
// for forward input channels cin (the phase width, convt_co) and forward output channels cout (the GEMM's K channels):
//   3 = compact taps: a channel tile inside one phase (cin % 64 == 0) and whole BK = 64 K slices per tap (cout % 64 == 0);
//   2 = window slots: a channel tile inside one phase, or whole phases inside a 64-channel tile (4 cin >= 64) without a residual
//       (phases sharing a tile take the generic epilogue, which does not accumulate);
//   0 = neither: the masked transposed-stride gather (tmode 1) is the form for that shape.
static int dgrad_phase_form(int cin, int cout, bool res) {
  if (cin <= 0 || cin % 8 || cout <= 0 || cout % 8) return 0;
  if (cin % 64 == 0) return cout % 64 == 0 ? 3 : 2;
  return (128 % cin == 0 && 4 * cin >= 64 && !res) ? 2 : 0;
}

int m355_conv2d_dgrad(const void* d_dy, int B, int H, int W, int cin, const float* h_w, int cout, int k, int stride,
                      void* d_dx, void* stream) {
  if (!d_dy || !h_w || !d_dx) return set_err(M355_ERR_INVALID, "null pointer");
  if ((k != 1 && k != 3) || (stride != 1 && stride != 2) || (k == 1 && stride != 1))
    return set_err(M355_ERR_INVALID, "dgrad supports k=3 (stride 1, 2) and k=1 (stride 1)");
  if (cin % 8 || cout % 8) return set_err(M355_ERR_INVALID, "channels must be multiples of 8");
  hipStream_t s = (hipStream_t)stream;
  const int pad = k / 2;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  // dgrad as a conv with "output channels" = cin and K = (tap, cout): row ci, column (tap', co)
  //   stride 1: tap' = flipped tap (kh' = k-1-kh);  stride 2 (transposed-stride gather): tap' = tap
  // stride 2 on even maps: four 2x2 phase convs over dY (conv_igemm.hip, phase == 2) -- rows [phase][ci], columns [(ty, tx)][co];
  // dX row 2i takes tap kh = 1 from dY row i, row 2i + 1 takes kh = 2 from row i and kh = 0 from row i + 1 (columns alike)
  // (which phase form, if any, launch_conv_igemm can tile: dgrad_phase_form; the masked gather otherwise)
  const int form = stride == 2 && k == 3 && H == 2 * Ho && W == 2 * Wo && !getenv("M355_NO_DGRAD_PHASES") ? dgrad_phase_form(cin, cout, false) : 0;
  const bool phases = form != 0;
  const int cout_pad = conv_cout_pad(phases ? 4 * cin : cin);
  const int Kpad = phases ? conv_kpad(cout, 2) : conv_kpad(cout, k);
  std::vector<half_t> rows((size_t)cout_pad * Kpad, (half_t)0.f);
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int kh = 0; kh < k; ++kh)
        for (int kw = 0; kw < k; ++kw) {
          const half_t v = (half_t)h_w[(((size_t)co * cin + ci) * k + kh) * k + kw];
          if (phases) {
            const int pa = kh == 1 ? 0 : 1, ty = kh == 0 ? 1 : 0, pb = kw == 1 ? 0 : 1, tx = kw == 0 ? 1 : 0;
            const int slot = form == 3 ? ty * (1 + pb) + tx : ty * 2 + tx;         // compact taps (phase 3) / window slots (phase 2)
            rows[(size_t)((2 * pa + pb) * cin + ci) * Kpad + (size_t)slot * cout + co] = v;
          } else {
            const int t = (stride == 1) ? ((k - 1 - kh) * k + (k - 1 - kw)) : (kh * k + kw);
            rows[(size_t)ci * Kpad + (size_t)t * cout + co] = v;
          }
        }
  std::vector<float> bias(cout_pad, 0.f);
  half_t *dw = nullptr, *dz = nullptr;
  float* db = nullptr;
  HIP_TRYG(hipMalloc((void**)&dw, rows.size() * sizeof(half_t)));
  HIP_TRYG(hipMalloc((void**)&db, bias.size() * sizeof(float)));
  HIP_TRYG(hipMalloc((void**)&dz, 256));
  HIP_TRYG(hipMemset(dz, 0, 256));
  HIP_TRYG(hipMemcpy(dw, rows.data(), rows.size() * sizeof(half_t), hipMemcpyHostToDevice));
  HIP_TRYG(hipMemcpy(db, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
  ConvArgs a{};
  a.x = (const half_t*)d_dy; a.x_bstride = (long)Ho * Wo * cout; a.ldx = cout; a.Hi = Ho; a.Wi = Wo; a.Cin = cout;
  a.w = dw; a.Kpad = Kpad; a.bias = db; a.zero = dz; a.act = 0; a.w_rows = cout_pad;
  a.y = d_dx; a.y_bstride = (long)H * W * cin; a.ldy = cin; a.Ho = H; a.Wo = W; a.Cout = cin;
  a.ksize = k; a.stride = 1; a.pad = pad; a.tmode = (stride == 2) ? 1 : 0;
  a.M = B * H * W;
  if (phases) {
    a.Ho = Ho; a.Wo = Wo; a.Cout = 4 * cin; a.convt_co = cin; a.ksize = 2; a.pad = 0; a.tmode = 0; a.phase = form;
    a.M = B * Ho * Wo;
  }
  int rc;
  if (a.phase == 2 && dgrad_s2c32_ok(a))
    rc = launch_dgrad_s2c32(a, s);
  else if (!a.tmode && !a.phase && conv3x3_halo_ok(a))
    rc = launch_conv3x3_halo(a, 0, s);
  else
    rc = launch_conv_igemm(a, TILE_AUTO, s);
  hipError_t se = hipStreamSynchronize(s);
  (void)hipFree(dw); (void)hipFree(db); (void)hipFree(dz);
  if (rc != 0) return set_err(M355_ERR_HIP, "dgrad launch failed: " + std::to_string(rc));
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string("dgrad kernel: ") + hipGetErrorString(se));
  return M355_OK;
}

int m355_conv2d_wgrad(const void* d_x, const void* d_dy, int B, int H, int W, int cin, int cout, int k, int stride,
                      float* d_dw, void* stream) {
  if (!d_x || !d_dy || !d_dw) return set_err(M355_ERR_INVALID, "null pointer");
  if ((k != 1 && k != 3) || (stride != 1 && stride != 2)) return set_err(M355_ERR_INVALID, "wgrad supports k in {1,3}, stride in {1,2}");
  static half_t* zero_page = nullptr;  // 256 zero bytes, allocated once per process
  if (!zero_page) {
    HIP_TRYG(hipMalloc((void**)&zero_page, 256));
    HIP_TRYG(hipMemset(zero_page, 0, 256));
  }
  const int pad = k / 2;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const size_t wsb = conv_wgrad_workspace_bytes(B, Ho, Wo, cin, cout, k);
  float* ws = nullptr;
  if (wsb) HIP_TRYG(hipMalloc((void**)&ws, wsb));
  const int rc = launch_conv_wgrad((const half_t*)d_dy, (long)Ho * Wo * cout, cout, (const half_t*)d_x, (long)H * W * cin,
                                   cin, B, H, W, cin, Ho, Wo, cout, k, stride, pad, d_dw, zero_page, ws, wsb, (hipStream_t)stream);
  const hipError_t se = hipStreamSynchronize((hipStream_t)stream);
  if (ws) (void)hipFree(ws);
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string("wgrad kernel: ") + hipGetErrorString(se));
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "wgrad launch failed: " + std::to_string(rc));
}

size_t m355_bn_workspace_floats(int C) { return bn_workspace_floats(C); }
size_t m355_wgrad_workspace_bytes(int32_t batch, int32_t ho, int32_t wo, int32_t cin, int32_t cout, int32_t ksize) {
  return conv_wgrad_workspace_bytes(batch, ho, wo, cin, cout, ksize);
}
size_t m355_grad_sumsq_workspace_floats(void) { return grad_sumsq_workspace_floats(); }

int m355_bn_silu_train_fwd(const void* d_z, int B, int H, int W, int C, const float* d_gamma, const float* d_beta,
                           float eps, int act, void* d_y, float* d_mean, float* d_invstd, float* d_ws, void* stream) {
  if (!d_z || !d_gamma || !d_beta || !d_y || !d_mean || !d_invstd || !d_ws) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_bn_silu_train_fwd((const half_t*)d_z, (long)B * H * W, C, C, d_gamma, d_beta, eps, (half_t*)d_y, C,
                                          nullptr, 0, d_ws, d_mean, d_invstd, act, nullptr, nullptr, 0.f, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "bn fwd launch failed: " + std::to_string(rc));
}

int m355_bn_silu_train_bwd(const void* d_z, const void* d_dy, int B, int H, int W, int C, const float* d_mean,
                           const float* d_invstd, const float* d_gamma, const float* d_beta, int act, void* d_dz,
                           float* d_dbeta_dgamma, float* d_ws, void* stream) {
  if (!d_z || !d_dy || !d_mean || !d_invstd || !d_gamma || !d_beta || !d_dz || !d_dbeta_dgamma || !d_ws)
    return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_bn_silu_train_bwd((const half_t*)d_z, (const half_t*)d_dy, (long)B * H * W, C, C, C, d_mean,
                                          d_invstd, d_gamma, d_beta, d_dbeta_dgamma, (half_t*)d_dz, C, act, d_ws,
                                          (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "bn bwd launch failed: " + std::to_string(rc));
}

int m355_convt2x2_fwd(const void* d_x, int B, int H, int W, int cin, const float* h_w, const float* h_bias, int cout,
                      void* d_y, void* stream) {
  return conv_op_common(d_x, B, H, W, cin, h_w, h_bias, cout, 2, 2, 0, nullptr, d_y, 0, TILE_AUTO, 1, stream);
}

int m355_stem_fwd(const void* d_in, int B, int H, int W, const float* h_w, const float* h_bias, int cout, void* d_y,
                  void* stream) {
  if (!d_in || !h_w || !h_bias || !d_y) return set_err(M355_ERR_INVALID, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  std::vector<half_t> sw((size_t)cout * 32, (half_t)0.f);
  for (int co = 0; co < cout; ++co)
    for (int c = 0; c < 3; ++c)
      for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw)
          sw[(size_t)co * 32 + (kh * 3 + kw) * 3 + c] = (half_t)h_w[((co * 3 + c) * 3 + kh) * 3 + kw];
  half_t* dw = nullptr;
  float* db = nullptr;
  HIP_TRYG(hipMalloc((void**)&dw, sw.size() * sizeof(half_t)));
  HIP_TRYG(hipMalloc((void**)&db, cout * sizeof(float)));
  HIP_TRYG(hipMemcpy(dw, sw.data(), sw.size() * sizeof(half_t), hipMemcpyHostToDevice));
  HIP_TRYG(hipMemcpy(db, h_bias, cout * sizeof(float), hipMemcpyHostToDevice));
  StemArgs a{};
  a.x = (const uint8_t*)d_in; a.B = B; a.H = H; a.W = W; a.w16 = dw; a.bias = db;
  a.y = (half_t*)d_y; a.y_bstride = (long)(H / 2) * (W / 2) * cout; a.ldy = cout; a.Cout = cout;
  const int rc = launch_stem(a, s);
  hipError_t se = hipStreamSynchronize(s);
  (void)hipFree(dw); (void)hipFree(db);
  if (rc != 0) return set_err(M355_ERR_HIP, "stem launch failed: " + std::to_string(rc));
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string("stem kernel: ") + hipGetErrorString(se));
  return M355_OK;
}

int m355_stem6_fwd(const void* d_x, int B, int H, int W, const float* h_w, const float* h_bias, int C0, void* d_y, void* stream) {
  // every argument before any HIP call
  if (!d_x || !h_w || !h_bias || !d_y) return set_err(M355_ERR_INVALID, "stem6: null pointer");
  if (C0 != 16 && C0 != 32 && C0 != 48) return set_err(M355_ERR_INVALID, "stem6: C0 must be 16, 32 or 48");
  if (B < 1 || B > 65535 || H < 2 || W < 16 || H % 2 || W % 16)
    return set_err(M355_ERR_INVALID, "stem6: B >= 1, H even and positive, W a positive multiple of 16");
  hipStream_t s = (hipStream_t)stream;
  std::vector<half_t> sw((size_t)C0 * 128);
  pack_stem6_weights(h_w, C0, sw.data());
  DevBuf d;
  Stem6Args a{};
  a.x = (const uint8_t*)d_x; a.B = B; a.H = H; a.W = W; a.C0 = C0;
  a.w = d.put(sw); a.bias = d.put(std::vector<float>(h_bias, h_bias + C0));
  a.y = (half_t*)d_y; a.ldy = C0; a.y_bstride = (long)(H / 2) * (W / 2) * C0;
  if (!a.w || !a.bias) return set_err(M355_ERR_HIP, "allocation failed");
  return finish_entry(launch_stem6(a, s), s, "stem6_s2");
}

int m355_dwconv3x3_fwd(const void* d_x, int B, int H, int W, int C, int ldx, const float* h_w, const float* h_b, int act, void* d_y,
                       int ldy, void* stream) {
  // every argument before any HIP call
  if (!d_x || !h_w || !h_b || !d_y) return set_err(M355_ERR_INVALID, "dwconv3x3: null pointer");
  if (C < 8 || C % 8) return set_err(M355_ERR_INVALID, "dwconv3x3: C must be a positive multiple of 8");
  if (ldx < C || ldy < C || ldx % 8 || ldy % 8) return set_err(M355_ERR_INVALID, "dwconv3x3: ldx and ldy must be multiples of 8, >= C");
  if (B < 1 || H < 1 || W < 1) return set_err(M355_ERR_INVALID, "dwconv3x3: B, H, W must be >= 1");
  if (act != 0 && act != 1) return set_err(M355_ERR_INVALID, "dwconv3x3: act must be 0 or 1");
  if (((uintptr_t)d_x | (uintptr_t)d_y) & 15) return set_err(M355_ERR_INVALID, "dwconv3x3: x and y must be 16-byte aligned");
  if ((long)B * ((H + 7) / 8) * W * (C / 8) > (1L << 38)) return set_err(M355_ERR_INVALID, "dwconv3x3: too large");
  hipStream_t s = (hipStream_t)stream;
  std::vector<half_t> dw((size_t)9 * C);
  pack_dw3x3_weights(h_w, C, dw.data());
  DevBuf d;
  DwConvArgs a{};
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * ldx; a.ldx = ldx;
  a.B = B; a.H = H; a.W = W; a.C = C; a.act = act;
  a.w = d.put(dw); a.bias = d.put(std::vector<float>(h_b, h_b + C));
  a.y = (half_t*)d_y; a.y_bstride = (long)H * W * ldy; a.ldy = ldy;
  if (!a.w || !a.bias) return set_err(M355_ERR_HIP, "allocation failed");
  return finish_entry(launch_dwconv3x3(a, s), s, "dwconv3x3");
}

int m355_psa_attn_fwd(const void* d_qkv, int B, int H, int W, int heads, int key_dim, int head_dim, const float* h_pe_w,
                      const float* h_pe_b, void* d_y, void* stream) {
  // every argument before any HIP call
  if (!d_qkv || !h_pe_w || !h_pe_b || !d_y) return set_err(M355_ERR_INVALID, "psa_attn: null pointer");
  if (key_dim != 32 || head_dim != 64) return set_err(M355_ERR_INVALID, "psa_attn: key_dim must be 32 and head_dim 64");
  if (heads < 1 || heads > 64) return set_err(M355_ERR_INVALID, "psa_attn: heads must be 1..64");
  if (B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W > (1L << 24))
    return set_err(M355_ERR_INVALID, "psa_attn: B 1..65535, H, W >= 1, H * W <= 2^24");
  if (((uintptr_t)d_qkv & 15) || ((uintptr_t)d_y & 7)) return set_err(M355_ERR_INVALID, "psa_attn: qkv 16-byte, y 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int C = 64 * heads;
  std::vector<half_t> dw((size_t)9 * C);
  pack_dw3x3_weights(h_pe_w, C, dw.data());
  DevBuf d;
  PsaArgs a{};
  a.qkv = (const half_t*)d_qkv; a.ldq = 2 * C; a.q_bstride = (long)H * W * a.ldq;
  a.B = B; a.H = H; a.W = W; a.heads = heads; a.C = C;
  a.pe_w = d.put(dw); a.pe_b = d.put(std::vector<float>(h_pe_b, h_pe_b + C));
  a.scale_log2e = (float)(1.4426950408889634 / sqrt(32.0));
  a.y = (half_t*)d_y; a.ldy = C; a.y_bstride = (long)H * W * C;
  if (!a.pe_w || !a.pe_b) return set_err(M355_ERR_HIP, "allocation failed");
  return finish_entry(launch_psa_attn(a, s), s, "psa_attn");
}

int m355_sppf_pool(const void* d_x, int B, int H, int W, int C, void* d_y, void* stream) {
  if (!d_x || !d_y) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_sppf_pool((const half_t*)d_x, (long)H * W * C, C, (half_t*)d_y, (long)H * W * 3 * C, 3 * C, B,
                                  H, W, C, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "sppf launch failed: " + std::to_string(rc));
}

int m355_upsample2x(const void* d_x, int B, int H, int W, int C, void* d_y, void* stream) {
  if (!d_x || !d_y) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_upsample2x((const half_t*)d_x, (long)H * W * C, C, (half_t*)d_y, (long)4 * H * W * C, C, B, H,
                                   W, C, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "upsample launch failed: " + std::to_string(rc));
}

int m355_head_decode(const float* d_raw, int B, int in_h, int in_w, int nc, float* d_preds, void* stream) {
  if (!d_raw || !d_preds) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_head_decode(d_raw, B, in_h, in_w, nc, 32, d_preds, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "decode launch failed: " + std::to_string(rc));
}

int m355_nms(const float* d_preds, int B, int A, int nc, int nm, float conf, float iou, int max_det, float* d_dets,
             int* d_counts, void* stream) {
  if (!d_preds || !d_dets || !d_counts) return set_err(M355_ERR_INVALID, "null pointer");
  void* ws = nullptr;
  const size_t wsb = nms_workspace_bytes(B, A);
  HIP_TRYG(hipMalloc(&ws, wsb));
  const int rc = launch_nms(d_preds, B, A, nc, nm, conf, iou, max_det, d_dets, d_counts, ws, wsb, (hipStream_t)stream);
  hipError_t se = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(ws);
  if (rc != 0) return set_err(M355_ERR_HIP, "nms launch failed: " + std::to_string(rc));
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string("nms kernel: ") + hipGetErrorString(se));
  return M355_OK;
}

int m355_nms_ex(const float* d_preds, int B, int A, int nc, int nm, float conf, float iou, int max_det, int agnostic,
                const uint32_t* d_class_mask, float* d_dets, int* d_counts, void* stream) {
  if (!d_preds || !d_dets || !d_counts) return set_err(M355_ERR_INVALID, "null pointer");
  if (B < 1 || A < 1 || nc < 1 || nm < 0) return set_err(M355_ERR_INVALID, "non-positive shape");
  if (max_det < 1 || max_det > 1024) return set_err(M355_ERR_INVALID, "max_det must be in [1, 1024]");
  if (agnostic != 0 && agnostic != 1) return set_err(M355_ERR_INVALID, "agnostic must be 0 or 1");
  if (d_class_mask && nc > 1024) return set_err(M355_ERR_INVALID, "a class set covers at most 1024 classes");
  void* ws = nullptr;
  const size_t wsb = nms_workspace_bytes(B, A);
  HIP_TRYG(hipMalloc(&ws, wsb));
  const int rc = launch_nms(d_preds, B, A, nc, nm, conf, iou, max_det, d_dets, d_counts, ws, wsb, (hipStream_t)stream,
                            agnostic, d_class_mask);
  hipError_t se = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(ws);
  if (rc != 0) return set_err(M355_ERR_HIP, "nms launch failed: " + std::to_string(rc));
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string("nms kernel: ") + hipGetErrorString(se));
  return M355_OK;
}

int m355_proto_masks_native(const float* d_dets, const int* d_counts, const void* d_protos, int B, int max_det, int mh,
                            int mw, const int32_t* h_orig_hw, const float* d_boxes, const int64_t* h_offsets,
                            uint8_t* d_out, void* stream) {
  if (!d_dets || !d_counts || !d_protos || !d_boxes || !h_orig_hw || !h_offsets)
    return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_proto_masks_native(d_dets, d_counts, (const half_t*)d_protos, B, max_det, mh, mw, h_orig_hw,
                                           d_boxes, h_offsets, d_out, (hipStream_t)stream);
  if (rc == -1)
    return set_err(M355_ERR_INVALID, "proto_masks_native: bad argument (shape, max_det, offset table, alignment or null output)");
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "native mask launch failed: " + std::to_string(rc));
}

int m355_proto_masks(const float* d_dets, const int* d_counts, const void* d_protos, int B, int max_det, int mh,
                     int mw, int in_h, int in_w, uint8_t* d_masks, void* stream) {
  if (!d_dets || !d_counts || !d_protos || !d_masks) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_proto_masks(d_dets, d_counts, (const half_t*)d_protos, B, max_det, 32, mh, mw, in_h, in_w,
                                    d_masks, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "mask launch failed: " + std::to_string(rc));
}

int m355_conv_launch(const m355_conv_args* c, void* stream) {
  if (!c || !c->x || !c->w_packed || !c->bias || !c->y || !c->zero_page) return set_err(M355_ERR_INVALID, "null pointer");
  ConvArgs a{};
  a.x = (const half_t*)c->x; a.x_bstride = c->x_bstride; a.ldx = c->ldx; a.Hi = c->hi; a.Wi = c->wi; a.Cin = c->cin;
  a.w = (const half_t*)c->w_packed; a.Kpad = c->kpad; a.bias = c->bias;
  a.y = c->y; a.y_bstride = c->y_bstride; a.ldy = c->ldy; a.Ho = c->ho; a.Wo = c->wo; a.Cout = c->cout;
  a.res = (const half_t*)c->res; a.r_bstride = c->r_bstride; a.ldr = c->ldr;
  a.ksize = c->ksize; a.stride = c->stride; a.pad = c->pad; a.M = c->batch * c->ho * c->wo;
  a.act = c->act; a.out_f32 = c->out_f32; a.convt_co = c->convt_co; a.tmode = c->tmode;
  a.zero = (const half_t*)c->zero_page;
  // ConvTranspose (convt_co, ksize 1): the residual would be read at the virtual (pre-shuffle) pixel, not at the output pixel the
  // result is stored to -- refused rather than computed wrong (the training step adds nothing to a ConvT output)
  if (c->convt_co > 0 && c->tmode == 0 && c->ksize == 1 && c->res)
    return set_err(M355_ERR_INVALID, "ConvTranspose (convt_co > 0, ksize 1) takes no residual");
  if (c->tmode == 2) {   // input gradient of a 3x3 / stride-2 / pad-1 conv as four 2x2 phase convs over dY (conv_igemm.hip, phase 2 / 3)
    a.tmode = 0;
    // compact tap layout where a channel tile lies inside one phase and the K axis is whole BK = 64 slices (the forward cout = cin here)
    a.phase = dgrad_phase_form(c->convt_co, c->cin, c->res != nullptr);
    if (!a.phase)
      return set_err(M355_ERR_INVALID, "tmode 2 needs convt_co % 64 == 0, or 128 % convt_co == 0 with convt_co >= 16 and no res "
                                       "(use the tmode 1 gather)");
  }
  int rc;
  // 1x1 convs of the training step (forward and input gradients) on conv1x1_wreg.hip where it applies (the weights are gathered
  // from the packed rows: the per-step re-pack writes no fragment-ordered copy): 27.4-27.5 -> 27.2-27.3 ms per s-seg b64 step on one box
  static const bool train_w1 = getenv("M355_NO_TRAIN_W1") == nullptr;
  static const bool train_c32 = getenv("M355_NO_TRAIN_C32") == nullptr;   // 32 -> 32 3x3 layers on conv3x3_c32.hip: a further -0.1 ms
  if (a.phase == 2 && dgrad_s2c32_ok(a))
    rc = launch_dgrad_s2c32(a, (hipStream_t)stream);
  else if (!a.tmode && conv3x3_halo_ok(a))
    rc = launch_conv3x3_halo(a, 0, (hipStream_t)stream);
  else if (train_w1 && !a.tmode && conv1x1_wreg_ok(a))
    rc = launch_conv1x1_wreg(a, (hipStream_t)stream);
  else if (train_c32 && !a.tmode && conv3x3_c32_ok(a) && conv_rows_covered(a, 32))
    rc = launch_conv3x3_c32(a, (hipStream_t)stream);
  // (3x3 / s1 on the 20 x 20 level through conv3x3_slab: measured 26.6 ms per step against 26.2 on the im2col kernel at batch 64 -- not taken)
  else
    rc = launch_conv_igemm(a, TILE_AUTO, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "conv launch failed: " + std::to_string(rc));
}

int m355_wgrad_launch(const m355_wgrad_args* w, void* stream) {
  if (!w || !w->dz || !w->x || !w->dw || !w->zero_page) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_conv_wgrad((const half_t*)w->dz, w->dz_bstride, w->lddz, (const half_t*)w->x, w->x_bstride, w->ldx,
                                   w->batch, w->hi, w->wi, w->cin, w->ho, w->wo, w->cout, w->ksize, w->stride, w->pad,
                                   w->dw, (const half_t*)w->zero_page, w->ws, (size_t)(w->ws_bytes < 0 ? 0 : w->ws_bytes),
                                   (hipStream_t)stream);
  if (rc == -3) return set_err(M355_ERR_INVALID, "wgrad workspace missing or smaller than m355_wgrad_workspace_bytes()");
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "wgrad launch failed: " + std::to_string(rc));
}

int m355_bn_train_fwd_launch(const void* z, int64_t npix, int32_t ldz, int32_t C, const float* gamma, const float* beta,
                             float eps, int32_t act, void* y, int32_t ldy, const void* res, int32_t ldr, float* mean,
                             float* invstd, float* ws, float* running_mean, float* running_var, float momentum,
                             void* stream) {
  if (!z || !gamma || !beta || !y || !mean || !invstd || !ws) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_bn_silu_train_fwd((const half_t*)z, npix, ldz, C, gamma, beta, eps, (half_t*)y, ldy,
                                          (const half_t*)res, ldr, ws, mean, invstd, act, running_mean, running_var, momentum,
                                          (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "bn fwd launch failed: " + std::to_string(rc));
}

int m355_bn_train_bwd_launch(const void* z, const void* dy, int64_t npix, int32_t ldz, int32_t lddy, int32_t C,
                             const float* mean, const float* invstd, const float* gamma, const float* beta, int32_t act,
                             void* dz, int32_t lddz, float* dbeta_dgamma, float* ws, void* stream) {
  if (!z || !dy || !mean || !invstd || !gamma || !beta || !dz || !dbeta_dgamma || !ws) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_bn_silu_train_bwd((const half_t*)z, (const half_t*)dy, npix, ldz, lddy, C, mean, invstd, gamma, beta,
                                          dbeta_dgamma, (half_t*)dz, lddz, act, ws, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "bn bwd launch failed: " + std::to_string(rc));
}

int m355_adamw_step(float* p, const float* g, float* m, float* v, float* ema, const uint8_t* group, int64_t n, float lr,
                    float lr_bias, float beta1, float beta2, float eps, float weight_decay, int32_t step, float grad_mul,
                    float ema_decay, void* stream) {
  return m355::launch_adamw_step(p, g, m, v, ema, group, n, lr, lr_bias, beta1, beta2, eps, weight_decay, step, grad_mul,
                                 ema_decay, (hipStream_t)stream);
}
int m355_sgd_step(float* p, const float* g, float* momentum_buf, float* ema, const uint8_t* group, int64_t n, float lr,
                  float lr_bias, float momentum, int32_t nesterov, float weight_decay, float grad_mul, float ema_decay,
                  void* stream) {
  return m355::launch_sgd_step(p, g, momentum_buf, ema, group, n, lr, lr_bias, momentum, nesterov, weight_decay, grad_mul,
                               ema_decay, (hipStream_t)stream);
}
int m355_grad_sumsq(const float* g, int64_t n, float* out, void* stream) {
  return m355::launch_grad_sumsq(g, n, out, (hipStream_t)stream);
}
int m355_augment(const void* d_cache, const m355_aug_params* d_params, void* d_out, int32_t B, int32_t H, int32_t W,
                 void* stream) {
  if (!d_cache || !d_params || !d_out) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = m355::launch_augment((const uint8_t*)d_cache, d_params, (uint8_t*)d_out, B, H, W, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "augment launch failed: " + std::to_string(rc));
}
int m355_msda_forward(const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim, const int32_t* shapes_hw,
                      int32_t num_levels, const float* d_loc, const float* d_attn, const int32_t* points_per_level,
                      int32_t Q, int32_t P, int32_t discrete, float* d_out, void* stream) {
  if (!d_value || !d_loc || !d_attn || !d_out || !shapes_hw || !points_per_level) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = m355::launch_msda(d_value, d_loc, d_attn, d_out, B, S, heads, head_dim, Q, P, num_levels, shapes_hw,
                                   points_per_level, discrete, (hipStream_t)stream);
  if (rc == -1)
    return set_err(M355_ERR_INVALID, "msda: head_dim must be 32, 1..8 levels tiling S, 1..32 points tiling P");
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "msda launch failed: " + std::to_string(rc));
}
int m355_msda_module_forward(const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim, const int32_t* shapes_hw,
                             int32_t num_levels, const float* d_ref, const float* d_offsets, const float* d_logits,
                             const int32_t* points_per_level, int32_t Q, int32_t P, float offset_scale, float* d_out,
                             void* stream) {
  if (!d_value || !d_ref || !d_offsets || !d_logits || !d_out || !shapes_hw || !points_per_level)
    return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = m355::launch_msda(d_value, d_offsets, d_logits, d_out, B, S, heads, head_dim, Q, P, num_levels, shapes_hw,
                                   points_per_level, 0, (hipStream_t)stream, d_ref, offset_scale);
  if (rc == -1)
    return set_err(M355_ERR_INVALID, "msda module: head_dim must be 32, 1..8 levels tiling S, 1..16 points tiling P");
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "msda launch failed: " + std::to_string(rc));
}
int m355_dfine_decode(const float* d_dist, const float* d_project, const float* d_ref, float* d_boxes, int64_t n,
                      int32_t num_bins_plus1, float reg_scale, int32_t clamp01, void* stream) {
  const int rc = m355::launch_dfine_decode(d_dist, d_project, d_ref, d_boxes, (long)n, num_bins_plus1, reg_scale, clamp01,
                                           (hipStream_t)stream);
  if (rc == -1) return set_err(M355_ERR_INVALID, "dfine_decode: null pointer, n < 0, fewer than 2 bins or reg_scale == 0");
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "dfine_decode launch failed: " + std::to_string(rc));
}
int m355_sppf_pool_launch(const void* x, int64_t x_bstride, int32_t ldx, void* y, int64_t y_bstride, int32_t ldy,
                          int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
  if (!x || !y) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_sppf_pool((const half_t*)x, x_bstride, ldx, (half_t*)y, y_bstride, ldy, B, H, W, C, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "sppf launch failed: " + std::to_string(rc));
}

int m355_repack_launch(const m355_repack_job* d_jobs, const int32_t* d_block_job, int32_t nblocks, void* stream) {
  const int rc = launch_repack(d_jobs, d_block_job, nblocks, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "repack launch failed: " + std::to_string(rc));
}

int m355_sppf_pool_bwd_launch(const void* a, int64_t a_bstride, int32_t lda, const void* y, int64_t y_bstride, int32_t ldy,
                              const void* gy, int64_t gy_bstride, int32_t ldgy, void* ga, int64_t ga_bstride, int32_t ldga,
                              int32_t B, int32_t H, int32_t W, int32_t C, int32_t accumulate, void* stream) {
  if (!a || !y || !gy || !ga) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_sppf_pool_bwd((const half_t*)a, a_bstride, lda, (const half_t*)y, y_bstride, ldy, (const half_t*)gy, gy_bstride,
                                      ldgy, (half_t*)ga, ga_bstride, ldga, B, H, W, C, accumulate, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "sppf backward launch failed: " + std::to_string(rc));
}

int64_t m355_colsum_workspace_floats(int64_t nb, int32_t cols) { return colsum_workspace_floats(nb, cols); }

int m355_colsum_launch(const void* src, int32_t src_f16, int64_t nb, int64_t bstride, int64_t rows, int32_t ld, int32_t cols, float* ws,
                       float* out, void* stream) {
  const int rc = launch_colsum(src, src_f16, nb, bstride, rows, ld, cols, ws, out, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "column-sum launch failed: " + std::to_string(rc));
}

int m355_upsample2x_bwd_launch(const void* g, int64_t g_bstride, int32_t ldg, void* d, int64_t d_bstride, int32_t ldd, int32_t B,
                               int32_t H, int32_t W, int32_t C, int32_t accumulate, void* stream) {
  const int rc = launch_upsample2x_bwd((const half_t*)g, g_bstride, ldg, (half_t*)d, d_bstride, ldd, B, H, W, C, accumulate,
                                       (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "upsample backward launch failed: " + std::to_string(rc));
}

int m355_addsilu_fwd_launch(const void* a, const void* b, void* v, void* y, int64_t npix, int32_t ldy, int32_t C, void* stream) {
  const int rc = launch_addsilu_fwd((const half_t*)a, (const half_t*)b, (half_t*)v, (half_t*)y, npix, ldy, C, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "addsilu forward launch failed: " + std::to_string(rc));
}

int m355_addsilu_bwd_launch(const void* v, const void* dy, int32_t lddy, void* g, int64_t npix, int32_t C, void* stream) {
  const int rc = launch_addsilu_bwd((const half_t*)v, (const half_t*)dy, lddy, (half_t*)g, npix, C, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "addsilu backward launch failed: " + std::to_string(rc));
}

int m355_adown_fwd_launch(const void* x, int64_t x_bstride, int32_t ldx, void* p1, int64_t p1_bstride, int32_t ld1, void* p2,
                          int64_t p2_bstride, int32_t ld2, uint8_t* argmax, int32_t B, int32_t H, int32_t W, int32_t c, void* stream) {
  const int rc = launch_adown_fwd((const half_t*)x, x_bstride, ldx, (half_t*)p1, p1_bstride, ld1, (half_t*)p2, p2_bstride, ld2, argmax, B, H, W, c,
                                  (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "adown forward launch failed: " + std::to_string(rc));
}

int m355_adown_bwd_launch(const void* g1, int64_t g1_bstride, int32_t ld1, const void* g2, int64_t g2_bstride, int32_t ld2,
                          const uint8_t* argmax, void* gx, int64_t gx_bstride, int32_t ldg, int32_t B, int32_t H, int32_t W, int32_t c,
                          int32_t accumulate, void* stream) {
  const int rc = launch_adown_bwd((const half_t*)g1, g1_bstride, ld1, (const half_t*)g2, g2_bstride, ld2, argmax, (half_t*)gx, gx_bstride, ldg, B,
                                  H, W, c, accumulate, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "adown backward launch failed: " + std::to_string(rc));
}

int m355_u8_to_f16x8_launch(const uint8_t* src, void* dst, int64_t npx, void* stream) {
  const int rc = launch_u8_to_f16x8(src, (half_t*)dst, npx, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "input conversion launch failed: " + std::to_string(rc));
}

int m355_mask_loss_launch(const float* coef, const void* protos, int32_t protos_f16, const int32_t* masks, const int32_t* inst,
                          const float* boxes, const float* weights, int32_t B, int32_t K, int32_t mh, int32_t mw, float* slot_sum,
                          float* d_coef, void* d_protos, int32_t d_protos_f16, const float* gscale, void* stream) {
  const int rc = launch_mask_loss(coef, protos, protos_f16, masks, inst, boxes, weights, B, K, mh, mw, slot_sum, d_coef, d_protos,
                                  d_protos_f16, gscale, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "mask-loss launch failed: " + std::to_string(rc));
}

int m355_box_loss_launch(const float* logits, const float* anchors, const float* targets, const float* weights, int64_t n,
                         float* box_term, float* dfl_term, float* d_box, float* d_dfl, void* stream) {
  const int rc = launch_box_loss(logits, anchors, targets, weights, n, box_term, dfl_term, d_box, d_dfl, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "box-loss launch failed: " + std::to_string(rc));
}

int m355_dfl_decode_launch(const float* raw, int64_t rows, int32_t A, int32_t rw, int32_t nc, const float* anchors, const float* strides,
                           float* boxes, float* scores, void* stream) {
  const int rc = launch_dfl_decode(raw, rows, A, rw, nc, anchors, strides, boxes, scores, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "dfl-decode launch failed: " + std::to_string(rc));
}

int m355_tal_assign_launch(const float* scores, const float* boxes, const float* anchors_px, const int32_t* gt_cls, const float* gt_boxes,
                           const uint8_t* gt_valid, int32_t B, int32_t A, int32_t G, int32_t nc, void* ws, float* t_boxes, float* t_scores,
                           uint8_t* fg, int64_t* gt_idx, void* stream) {
  const int rc = launch_tal_assign(scores, boxes, anchors_px, gt_cls, gt_boxes, gt_valid, B, A, G, nc, ws, t_boxes, t_scores, fg, (long*)gt_idx,
                                   (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "tal_assign launch failed: " + std::to_string(rc));
}

int m355_upsample2x_launch(const void* x, int64_t x_bstride, int32_t ldx, void* y, int64_t y_bstride, int32_t ldy,
                           int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
  if (!x || !y) return set_err(M355_ERR_INVALID, "null pointer");
  const int rc = launch_upsample2x((const half_t*)x, x_bstride, ldx, (half_t*)y, y_bstride, ldy, B, H, W, C, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "upsample launch failed: " + std::to_string(rc));
}

}  // extern "C"
