// libmi355yolo.so graph construction: the model families (YOLOv8-seg, YOLOv8 detect, YOLOv9c-seg, YOLOv5u, YOLO11) written as tensors,
// logical convs, physical convs and ops of an m355_engine (engine_types.h).  Host C++ only: no kernel and no HIP runtime call;
// engine.hip fuses, plans, allocates and runs what build_graph leaves.
//
// Graph (upstream yolov8-seg.yaml as exercised by
// BscanBased/yolo8_seg_predict.py:5-8): every Concat is physical-zero-copy -- producers write their
// output at a channel offset of the consumer's NHWC buffer; C2f's split/concat is one buffer.
//
// The order of tensor(), logical(), phys_from() / phys_diag() and op creation is the order of tensor ids, logical conv indices
// (the ABI of m355_get_conv_info, mirrored by spec.py), physical conv indices and launches, and e->macs is a sum of doubles in
// op order: a helper here never reorders what its callers did by hand.
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "engine_types.h"

namespace m355 {
namespace {

int make_divisible(double x, int d) { return (int)ceil(x / d) * d; }

// (depth, width, max channels) of every m355_model_desc.scale that is built; c3k_all: upstream parse_model gives every C3k2 of
// the YOLO11 m (l, x) scale a C3k
struct Scale {
  int code;
  double depth, width;
  int maxc;
  bool c3k_all;
};
const Scale kScales[] = {
    {'n', 0.33, 0.25, 1024, false},              {'s', 0.33, 0.50, 1024, false},
    {'m', 0.67, 0.75, 768, false},               {'l', 1.00, 1.00, 512, false},
    {'x', 1.00, 1.25, 512, false},               {'c', 1.00, 1.00, 1024, false},
    {('5' << 8) | 'n', 0.33, 0.25, 1024, false}, {('5' << 8) | 's', 0.33, 0.50, 1024, false},
    {('5' << 8) | 'm', 0.67, 0.75, 1024, false}, {('1' << 8) | 'n', 0.50, 0.25, 1024, false},
    {('1' << 8) | 's', 0.50, 0.50, 1024, false}, {('1' << 8) | 'm', 0.50, 1.00, 512, true},
    {('8' << 8) | 'n', 0.33, 0.25, 1024, false}, {('8' << 8) | 's', 0.33, 0.50, 1024, false},
    {('8' << 8) | 'm', 0.67, 0.75, 768, false},  {('8' << 8) | 'l', 1.00, 1.00, 512, false},
    {('8' << 8) | 'x', 1.00, 1.25, 512, false},
};

// What a family asks of the descriptor: its smallest image side and the texts of its two rejections, and its mask width
struct Family {
  int min_hw, nm;
  const char *bad_scale, *bad_size;
};
const char kBadScaleSeg[] = "scale must be one of n,s,m,l,x (yolov8-seg) or c (yolov9c-seg)";
const char kBadSize64[] = "in_h/in_w must be multiples of 32, at least 64";
const Family kV8{32, 32, kBadScaleSeg, "in_h/in_w must be positive multiples of 32"};
const Family kV9c{64, 32, kBadScaleSeg, kBadSize64};
const Family kV5u{64, 0, "YOLOv5u scale must be n, s or m (l and x are not built)", kBadSize64};
const Family kY11{64, 0, "YOLO11 scale must be n, s or m (l and x are not built)", kBadSize64};
const Family kV8Det{32, 0, "YOLOv8 detect scale must be one of n,s,m,l,x", "in_h/in_w must be positive multiples of 32"};

// One branch of a head over the three levels: {pre}.{l}.0 (3x3, fch[l] -> hc), .1 (3x3, hc -> hc), .2 (1x1 with bias, hc -> cout)
struct Branch {
  int hc, cout;
  int l[3][3];
};

// Sizes of a head: the three levels' maps and anchor offsets, the widths of the box and the class branch
struct Head {
  int HW[3][2], off[3];
  int hc2, hc3;
};

struct Builder {
  m355_engine* e;
  double depth = 0, width = 0;
  int maxc = 0;
  bool c3k_all = false;
  int H1 = 0, W1 = 0, H2 = 0, W2 = 0, H3 = 0, W3 = 0, H4 = 0, W4 = 0, H5 = 0, W5 = 0;   // the pyramid: in_h / 2 .. in_h / 32
  int c64 = 0, c128 = 0, c256 = 0, c512 = 0, c1024 = 0;                                 // ch(64) .. ch(1024)
  int ch(int c) const { return make_divisible(std::min(c, maxc) * width, 8); }
  int rep(int n) const { return n > 1 ? std::max((int)lround(n * depth), 1) : n; }

  // Checks the descriptor as family `f` does and takes the scale's row, the pyramid sizes and the channel widths from it
  int begin(const Family& f) {
    const m355_model_desc& d = e->desc;
    const Scale* sc = nullptr;
    for (const Scale& s : kScales)
      if (s.code == d.scale) sc = &s;
    if (!sc) return e->fail(M355_ERR_INVALID, f.bad_scale);
    depth = sc->depth; width = sc->width; maxc = sc->maxc; c3k_all = sc->c3k_all;
    if (d.in_h % 32 || d.in_w % 32 || d.in_h < f.min_hw || d.in_w < f.min_hw) return e->fail(M355_ERR_INVALID, f.bad_size);
    if (d.nc < 1 || d.max_batch < 1) return e->fail(M355_ERR_INVALID, "nc and max_batch must be >= 1");
    e->nc = d.nc; e->nm = f.nm;
    c64 = ch(64); c128 = ch(128); c256 = ch(256); c512 = ch(512); c1024 = ch(1024);
    H1 = d.in_h / 2; H2 = d.in_h / 4; H3 = d.in_h / 8; H4 = d.in_h / 16; H5 = d.in_h / 32;
    W1 = d.in_w / 2; W2 = d.in_w / 4; W3 = d.in_w / 8; W4 = d.in_w / 16; W5 = d.in_w / 32;
    return 0;
  }

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

  // One launch of the physical conv `phys` (OP_CONV, OP_CONVT, OP_DWCONV, OP_PSA_ATTN) from slice `in` to slice `out`, its MACs
  // added to the net's.  The caller sets what only it needs (out_ext, level_off, heads) on the op returned, before the next one.
  Op& launch(OpKind kind, int phys, Slice in, Slice out, Slice res = Slice(), Slice in2 = Slice()) {
    Op op{};
    op.kind = kind;
    op.conv = phys;
    op.in = in; op.out = out; op.res = res; op.in2 = in2;
    const PhysConv& p = e->phys[phys];
    const Tensor& ti = e->tensors[in.t];
    if (kind == OP_CONVT) {
      e->macs += (double)(2 * ti.H) * (2 * ti.W) * p.cin * p.cout;
    } else {
      const int Ho = (ti.H + 2 * (p.k / 2) - p.k) / p.stride + 1, Wo = (ti.W + 2 * (p.k / 2) - p.k) / p.stride + 1;
      e->macs += (double)Ho * Wo * p.macs_px;
    }
    e->ops.push_back(op);
    return e->ops.back();
  }
  // An op without a conv of its own (OP_POOL, OP_UP, OP_ADOWN, OP_DECODE)
  Op& aux(OpKind kind, Slice in = Slice(), Slice out = Slice()) {
    Op op{};
    op.kind = kind;
    op.in = in; op.out = out;
    e->ops.push_back(op);
    return e->ops.back();
  }
  // Conv(+BN+SiLU) from slice `in` to slice `out`
  void conv(const std::string& name, Slice in, Slice out, int k, int s, Slice res = Slice(), Slice in2 = Slice()) {
    const int li = logical(name, in.c, out.c, k, s, 1, 0, 1);
    launch(OP_CONV, phys_from({li}), in, out, res, in2);
  }
  // model.0: the k x k / s2 stem (3 k k taps per output) from the image into a new H1 x W1 tensor, which is returned
  int stem(const std::string& name, int cout, int k) {
    const int t0 = tensor(H1, W1, cout);
    const int li = logical(name, 3, cout, k, 2, 1, 0, 1);
    Op op{};
    op.kind = OP_STEM;
    op.conv = phys_from({li});
    op.out = Slice{t0, 0, cout};
    op.Hi = e->desc.in_h; op.Wi = e->desc.in_w;
    e->macs += (double)H1 * W1 * cout * (3 * k * k);
    e->ops.push_back(op);
    return t0;
  }
  // SPPF: cv1 -> three serial 5x5 max pools beside it in one buffer -> `last` (cv2; cv5 of yolov9c's SPPELAN)
  void sppf(const std::string& name, Slice in, Slice out, const char* last = "cv2") {
    const int c_ = in.c / 2;
    const int sp = tensor(e->tensors[in.t].H, e->tensors[in.t].W, 4 * c_);
    conv(name + ".cv1", in, Slice{sp, 0, c_}, 1, 1);
    aux(OP_POOL, Slice{sp, 0, c_}, Slice{sp, c_, 3 * c_});
    conv(name + "." + last, Slice{sp, 0, 4 * c_}, out, 1, 1);
  }
  // Upsample(src) + Concat into the channels `dst` in front of a block.  By default nothing is copied: the block's first 1x1
  // conv reads those channels through its gather from the half-resolution `src` (upsample read-through, conv_igemm.hip), and
  // the slice returned is that conv's in2.  With M355_NO_UPFUSE the upsample kernel materialises them and in2 is empty.
  Slice up(Slice src, Slice dst) {
    if (!e->sw.no_upfuse) return src;
    aux(OP_UP, src, dst);
    return Slice();
  }
  void decode() { aux(OP_DECODE); }

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

  // ---- what the Segment head and the two Detect heads share.  The caller decides the order of its branches' logical convs
  // (Segment puts Proto between cv3 and cv4): that order is the ABI.
  Branch branch(const std::string& pre, const int fch[3], int hc, int cout) {
    Branch br{hc, cout, {}};
    for (int l = 0; l < 3; ++l) {
      const std::string p = pre + "." + std::to_string(l);
      br.l[l][0] = logical(p + ".0", fch[l], hc, 3, 1, 1, 0, 1);
      br.l[l][1] = logical(p + ".1", hc, hc, 3, 1, 1, 0, 1);
      br.l[l][2] = logical(p + ".2", hc, cout, 1, 1, 0, 0, 0);
    }
    return br;
  }
  Head head(const int feats[3], const int fch[3]) {
    Head h{};
    for (int l = 0; l < 3; ++l) { h.HW[l][0] = e->tensors[feats[l]].H; h.HW[l][1] = e->tensors[feats[l]].W; }
    e->n3 = h.HW[0][0] * h.HW[0][1]; e->n4 = h.HW[1][0] * h.HW[1][1]; e->n5 = h.HW[2][0] * h.HW[2][1];
    e->A = e->n3 + e->n4 + e->n5;
    h.off[1] = e->n3; h.off[2] = e->n3 + e->n4;
    h.hc2 = std::max(std::max(16, fch[0] / 4), 64);
    h.hc3 = std::max(fch[0], std::min(e->nc, 100));
    return h;
  }
  // Front of head level l: the first convs of `brs` share their input `feat` and run as one launch into one tensor; their
  // second convs write side by side into a second tensor, ucat (returned), which has `extra` more channels behind them for a
  // branch the caller emits itself.
  int level_front(const Head& h, int l, Slice feat, std::initializer_list<const Branch*> brs, int extra = 0) {
    std::vector<int> first;
    int hc = 0;
    for (const Branch* br : brs) { first.push_back(br->l[l][0]); hc += br->hc; }
    const int hcat = tensor(h.HW[l][0], h.HW[l][1], hc), ucat = tensor(h.HW[l][0], h.HW[l][1], hc + extra);
    launch(OP_CONV, phys_from(first), feat, Slice{hcat, 0, hc});
    int off = 0;
    const size_t second = e->ops.size();
    for (const Branch* br : brs) {
      launch(OP_CONV, phys_from({br->l[l][1]}), Slice{hcat, off, br->hc}, Slice{ucat, off, br->hc});
      off += br->hc;
    }
    // box | class | coefficient branches: a block-diagonal 224 -> 224 3x3 conv, one launch where the engine's plan takes it.  The
    // 80 x 80 level stays on its three launches (M355_HEADDIAG_L0: measured).
    if (brs.size() == 3 && (l > 0 || e->sw.headdiag_l0)) e->ops[second].diag_n = 3;
    return ucat;
  }
  // Back of head level l: the 1x1 output convs `outs` (64 box bins, nc classes, nm mask coefficients: different inputs, side by
  // side in ucat) run as ONE launch with a block-diagonal weight matrix and write whole rows of the raw head map.  Every op of
  // the level, from `lvl_first` on, goes to stream lane `lane` (plan_lanes).
  void level_back(const Head& h, int l, int ucat, const std::vector<int>& outs, size_t lvl_first, int lane) {
    int width = 0;
    for (int li : outs) width += e->convs[li].cout;
    Op& op = launch(OP_CONV, phys_diag(outs), Slice{ucat, 0, e->tensors[ucat].C}, Slice{-1, 0, width});
    op.out_ext = 1; op.level_off = h.off[l];
    for (size_t i = lvl_first; i < e->ops.size(); ++i) e->ops[i].lane = lane;
  }
};

// model.22 = Segment(nc, 32, npr) on the three feature tensors `feats` (channels fch): Detect branches, coefficient branch,
// Proto, decode.  Shared by the yolov8-seg and yolov9c-seg graphs.
int build_segment_head(m355_engine* e, Builder& b, const int feats[3], const int fch[3], const int npr) {
  const int nc = e->nc, nm = e->nm;
  const Head h = b.head(feats, fch);
  const int H3 = h.HW[0][0], W3 = h.HW[0][1], H2 = 2 * H3, W2 = 2 * W3;
  // canonical logical order follows the upstream state dict: cv2.{l}.{0,1,2}, cv3.{l}.*, proto.*, cv4.{l}.*.
  // Physical fusion: cv2.l.0 + cv3.l.0 + cv4.l.0 share their input -> one launch with cout = hc2+hc3+hc4.
  const Branch cv2 = b.branch("model.22.cv2", fch, h.hc2, 64), cv3 = b.branch("model.22.cv3", fch, h.hc3, nc);
  const int l_p1 = b.logical("model.22.proto.cv1", fch[0], npr, 3, 1, 1, 0, 1);
  const int l_pu = b.logical("model.22.proto.upsample", npr, npr, 2, 2, 0, 1, 0);
  const int l_p2 = b.logical("model.22.proto.cv2", npr, npr, 3, 1, 1, 0, 1);
  const int l_p3 = b.logical("model.22.proto.cv3", npr, nm, 1, 1, 1, 0, 1);
  const Branch cv4 = b.branch("model.22.cv4", fch, std::max(fch[0] / 4, nm), nm);
  const int* lane_plan = e->sw.lane_plan;   // stream lane of Proto and of the three head levels (plan_lanes)
  for (int l = 0; l < 3; ++l) {
    const size_t lvl_first = e->ops.size();
    const int ucat = b.level_front(h, l, Slice{feats[l], 0, fch[l]}, {&cv2, &cv3, &cv4});
    b.level_back(h, l, ucat, {cv2.l[l][2], cv3.l[l][2], cv4.l[l][2]}, lvl_first, lane_plan[1 + l]);
  }
  const size_t proto_first = e->ops.size();
  {
    const bool fuse2 = !e->sw.no_protofuse && npr % 64 == 0;   // a channel tile (64 or 128) must lie inside one phase
    const bool fuse3 = fuse2 && npr == 128 && nm == 32 && !e->sw.no_protofuse3;
    const int pr1 = b.tensor(H3, W3, npr);
    b.launch(OP_CONV, b.phys_from({l_p1}), Slice{feats[0], 0, fch[0]}, Slice{pr1, 0, npr});
    if (!fuse2) {
      const int pr2 = b.tensor(H2, W2, npr), pr3 = b.tensor(H2, W2, npr);
      b.launch(OP_CONVT, b.phys_from({l_pu}), Slice{pr1, 0, npr}, Slice{pr2, 0, npr});
      b.launch(OP_CONV, b.phys_from({l_p2}), Slice{pr2, 0, npr}, Slice{pr3, 0, npr});
      b.launch(OP_CONV, b.phys_from({l_p3}), Slice{pr3, 0, npr}, Slice{-1, 0, nm}).out_ext = 2;
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
        b.launch(OP_CONV, b.phys_from({l_p3}), Slice{pr3, 0, npr}, Slice{-1, 0, nm}).out_ext = 2;
      }
    }
  }
  for (size_t i = proto_first; i < e->ops.size(); ++i) e->ops[i].lane = lane_plan[0];
  b.decode();
  e->proto_h = H2; e->proto_w = W2;
  return 0;
}

// yolov9c-seg (SURVEY next row N4: the architecture BscanBased/yolo_seg_train.py:7 names).  GELAN blocks on
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
    b.aux(OP_ADOWN, in, Slice{ta, 0, ch}).out2 = Slice{tm, 0, ch};
    b.conv(name + ".cv1", Slice{ta, 0, ch}, Slice{out.t, out.off, co}, 3, 2);
    b.conv(name + ".cv2", Slice{tm, 0, ch}, Slice{out.t, out.off + co, co}, 1, 1);
  }
};

int build_graph_v9c(m355_engine* e) {
  Builder b{e};
  V9cBuilder v{e, b};
  if (int rc = b.begin(kV9c)) return rc;
  const int H2 = b.H2, W2 = b.W2, H3 = b.H3, W3 = b.W3, H4 = b.H4, W4 = b.W4, H5 = b.H5, W5 = b.W5;
  // zero-copy concat buffers: cat11 = [up(x9), x6], cat14 = [up(x12), x4], cat17 = [x16, x12], cat20 = [x19, x9]
  const int cat11 = b.tensor(H4, W4, 512 + 512), cat14 = b.tensor(H3, W3, 512 + 512);
  const int cat17 = b.tensor(H4, W4, 256 + 512), cat20 = b.tensor(H5, W5, 512 + 512);
  const Slice x4{cat14, 512, 512}, x6{cat11, 512, 512}, x9{cat20, 512, 512}, x12{cat17, 256, 512};
  const int t0 = b.stem("model.0", 64, 3);
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
  b.sppf("model.9", Slice{t8, 0, 512}, x9, "cv5");             // SPPELAN
  const Slice up12 = b.up(x9, Slice{cat11, 0, 512});
  v.elan("model.12", Slice{cat11, 0, 1024}, x12, 512, 256, up12);
  const Slice up15 = b.up(x12, Slice{cat14, 0, 512});
  const int t15 = b.tensor(H3, W3, 256), t18 = b.tensor(H4, W4, 512), t21 = b.tensor(H5, W5, 512);
  v.elan("model.15", Slice{cat14, 0, 1024}, Slice{t15, 0, 256}, 256, 128, up15);
  v.adown("model.16", Slice{t15, 0, 256}, Slice{cat17, 0, 256});
  v.elan("model.18", Slice{cat17, 0, 768}, Slice{t18, 0, 512}, 512, 256);
  v.adown("model.19", Slice{t18, 0, 512}, Slice{cat20, 0, 512});
  v.elan("model.21", Slice{cat20, 0, 1024}, Slice{t21, 0, 512}, 512, 256);
  const int feats[3] = {t15, t18, t21};
  const int fch[3] = {256, 512, 512};
  return build_segment_head(e, b, feats, fch, 256);
}

// model.24 = Detect(nc) of YOLOv5u, model.22 = Detect(nc) of YOLOv8 (box-only, nm = 0): per level the two first 3x3 convs (cv2.l.0, cv3.l.0) share their input
// and run as one launch, the two second convs write side by side, and the two 1x1 output convs run as one block-diagonal launch
// writing whole raw rows of 64 + nc.  The decode launch turns them into prediction rows of 4 + nc.
int build_detect_head(m355_engine* e, Builder& b, const int feats[3], const int fch[3], const std::string& pre) {
  const Head h = b.head(feats, fch);
  const Branch cv2 = b.branch(pre + ".cv2", fch, h.hc2, 64), cv3 = b.branch(pre + ".cv3", fch, h.hc3, e->nc);
  const int lane_plan[3] = {1, 1, 0};   // the stride-8 and stride-16 levels beside the stride-32 level on the caller's stream
  for (int l = 0; l < 3; ++l) {
    const size_t lvl_first = e->ops.size();
    const int ucat = b.level_front(h, l, Slice{feats[l], 0, fch[l]}, {&cv2, &cv3});
    b.level_back(h, l, ucat, {cv2.l[l][2], cv3.l[l][2]}, lvl_first, lane_plan[l]);
  }
  b.decode();
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
  b.launch(OP_CONV, b.phys_from({l2, l1}), in, Slice{X, c_, 2 * c_}, Slice(), up_src);
  const int tmp = b.tensor(H, W, c_);
  int pp[2] = {-1, -1};
  if (n > 1) { pp[0] = b.tensor(H, W, c_); pp[1] = n > 2 ? b.tensor(H, W, c_) : -1; }
  Slice src{X, 2 * c_, c_};
  for (int j = 0; j < n; ++j) {
    const std::string mn = name + ".m." + std::to_string(j);
    const int la = b.logical(mn + ".cv1", c_, c_, 1, 1, 1, 0, 1), lb = b.logical(mn + ".cv2", c_, c_, 3, 1, 1, 0, 1);
    const Slice dst = j == n - 1 ? Slice{X, 0, c_} : Slice{pp[j & 1], 0, c_};
    b.launch(OP_CONV, b.phys_from({la}), src, Slice{tmp, 0, c_});
    b.launch(OP_CONV, b.phys_from({lb}), Slice{tmp, 0, c_}, dst, shortcut ? src : Slice());
    src = dst;
  }
  b.launch(OP_CONV, b.phys_from({l3}), Slice{X, 0, 2 * c_}, out);
}

// YOLOv5u (BscanBased/yolo5s_retrain.py:6 loads yolov5su.pt; upstream cfg/models/v5/yolov5.yaml with
// the anchor-free Detect head).  model.0 is the 6x6 / s2 / p2 stem (conv_stem6_s2.hip); every other conv goes through the planner's
// usual kernel rules.  Names and canonical order: spec.py conv_specs_v5u; block structure: tests/yolov5u_det_ref.py.
int build_graph_v5u(m355_engine* e) {
  Builder b{e};
  if (int rc = b.begin(kV5u)) return rc;
  const int c64 = b.c64, c128 = b.c128, c256 = b.c256, c512 = b.c512, c1024 = b.c1024;
  const int H2 = b.H2, W2 = b.W2, H3 = b.H3, W3 = b.W3, H4 = b.H4, W4 = b.W4, H5 = b.H5, W5 = b.W5;
  // zero-copy concat buffers: cat12 = [up(x10), x6], cat16 = [up(x14), x4], cat19 = [x18, x14], cat22 = [x21, x10]
  const int cat12 = b.tensor(H4, W4, 2 * c512), cat16 = b.tensor(H3, W3, 2 * c256);
  const int cat19 = b.tensor(H4, W4, 2 * c256), cat22 = b.tensor(H5, W5, 2 * c512);
  const Slice x4{cat16, c256, c256}, x6{cat12, c512, c512}, x10{cat22, c512, c512}, x14{cat19, c256, c256};
  const int t0 = b.stem("model.0", c64, 6);
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
  b.sppf("model.9", Slice{t8, 0, c1024}, Slice{t9, 0, c1024});
  b.conv("model.10", Slice{t9, 0, c1024}, x10, 1, 1);
  // 11/12 and 15/16: Upsample + Concat read through by the next C3's cv2 || cv1 (M355_NO_UPFUSE: materialised by upsample2x)
  const int t13 = b.tensor(H4, W4, c512), t17 = b.tensor(H3, W3, c256), t20 = b.tensor(H4, W4, c512), t23 = b.tensor(H5, W5, c1024);
  const Slice up13 = b.up(x10, Slice{cat12, 0, c512});
  build_c3(e, b, "model.13", Slice{cat12, 0, 2 * c512}, Slice{t13, 0, c512}, b.rep(3), false, up13);
  b.conv("model.14", Slice{t13, 0, c512}, x14, 1, 1);
  const Slice up17 = b.up(x14, Slice{cat16, 0, c256});
  build_c3(e, b, "model.17", Slice{cat16, 0, 2 * c256}, Slice{t17, 0, c256}, b.rep(3), false, up17);
  b.conv("model.18", Slice{t17, 0, c256}, Slice{cat19, 0, c256}, 3, 2);
  build_c3(e, b, "model.20", Slice{cat19, 0, 2 * c256}, Slice{t20, 0, c512}, b.rep(3), false);
  b.conv("model.21", Slice{t20, 0, c512}, Slice{cat22, 0, c512}, 3, 2);
  build_c3(e, b, "model.23", Slice{cat22, 0, 2 * c512}, Slice{t23, 0, c1024}, b.rep(3), false);
  const int feats[3] = {t17, t20, t23};
  const int fch[3] = {c256, c512, c1024};
  return build_detect_head(e, b, feats, fch, "model.24");
}

// model.23 = Detect(nc) of YOLO11 (box-only, nm = 0).  Box branch as YOLOv8's; the class branch is DWConv 3x3 -> 1x1 ->
// DWConv 3x3 -> 1x1 (cv3.l.0.0 .. cv3.l.1.1; the depthwise convs run on dwconv3x3.hip), so cv2.l.0 no longer shares its launch
// with the class branch's first conv.  The two second stages write side by side and the two output 1x1 convs run as one
// block-diagonal launch writing raw rows of 64 + nc, as in build_detect_head.
int build_detect_head_y11(m355_engine* e, Builder& b, const int feats[3], const int fch[3], const std::string& pre) {
  const int nc = e->nc;
  const Head h = b.head(feats, fch);
  const int hc3 = h.hc3;
  if (hc3 % 8)
    return e->fail(M355_ERR_INVALID, "YOLO11: the class branch width max(P3 channels, min(nc, 100)) must be a multiple of 8 "
                                     "(the depthwise kernel's 16-byte channel groups): n scale with nc in 65..100 not a multiple of 8");
  const Branch cv2 = b.branch(pre + ".cv2", fch, h.hc2, 64);
  int l_cv3[3][5];
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
    const int H = h.HW[l][0], W = h.HW[l][1];
    const Slice f{feats[l], 0, fch[l]};
    const int ucat = b.level_front(h, l, f, {&cv2}, hc3);
    const int d0 = b.tensor(H, W, fch[l]), e0 = b.tensor(H, W, hc3), d1 = b.tensor(H, W, hc3);
    b.launch(OP_DWCONV, b.phys_from({l_cv3[l][0]}), f, Slice{d0, 0, fch[l]});
    b.launch(OP_CONV, b.phys_from({l_cv3[l][1]}), Slice{d0, 0, fch[l]}, Slice{e0, 0, hc3});
    b.launch(OP_DWCONV, b.phys_from({l_cv3[l][2]}), Slice{e0, 0, hc3}, Slice{d1, 0, hc3});
    b.launch(OP_CONV, b.phys_from({l_cv3[l][3]}), Slice{d1, 0, hc3}, Slice{ucat, h.hc2, hc3});
    b.level_back(h, l, ucat, {cv2.l[l][2], l_cv3[l][4]}, lvl_first, lane_plan[l]);
  }
  b.decode();
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
  b.launch(OP_CONV, b.phys_from({l1}), in, Slice{X, 0, 2 * c}, Slice(), up_src);
  const Slice src{X, c, c}, dst{X, 2 * c, c};
  const std::string mn = name + ".m.0";
  if (!c3k) {
    const int h = c / 2;
    const int la = b.logical(mn + ".cv1", c, h, 3, 1, 1, 0, 1), lb = b.logical(mn + ".cv2", h, c, 3, 1, 1, 0, 1);
    const int tmp = b.tensor(H, W, h);
    b.launch(OP_CONV, b.phys_from({la}), src, Slice{tmp, 0, h});
    b.launch(OP_CONV, b.phys_from({lb}), Slice{tmp, 0, h}, dst, src);
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
    b.launch(OP_CONV, b.phys_from({k2, k1}), src, Slice{Y, c_, 2 * c_});
    b.launch(OP_CONV, b.phys_from({la[0]}), Slice{Y, 2 * c_, c_}, Slice{tmp, 0, c_});
    b.launch(OP_CONV, b.phys_from({lb[0]}), Slice{tmp, 0, c_}, Slice{mid, 0, c_}, Slice{Y, 2 * c_, c_});
    b.launch(OP_CONV, b.phys_from({la[1]}), Slice{mid, 0, c_}, Slice{tmp, 0, c_});
    b.launch(OP_CONV, b.phys_from({lb[1]}), Slice{tmp, 0, c_}, Slice{Y, 0, c_}, Slice{mid, 0, c_});
    b.launch(OP_CONV, b.phys_from({k3}), Slice{Y, 0, 2 * c_}, dst);
  }
  b.launch(OP_CONV, b.phys_from({l2}), Slice{X, 0, 3 * c}, out);
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
  b.launch(OP_CONV, b.phys_from({l_cv1}), in, Slice{X, 0, 2 * c});
  b.launch(OP_CONV, b.phys_from({l_qkv}), Slice{X, c, c}, Slice{QKV, 0, 2 * c});
  // (the MACs counted are the pe conv's; the two attention products are in the op table's FLOPs)
  b.launch(OP_PSA_ATTN, b.phys_from({l_pe}), Slice{QKV, 0, 2 * c}, Slice{O, 0, c}).heads = c / 64;
  b.launch(OP_CONV, b.phys_from({l_proj}), Slice{O, 0, c}, Slice{B1, 0, c}, Slice{X, c, c});
  b.launch(OP_CONV, b.phys_from({l_f0}), Slice{B1, 0, c}, Slice{F, 0, 2 * c});
  b.launch(OP_CONV, b.phys_from({l_f1}), Slice{F, 0, 2 * c}, Slice{X, c, c}, Slice{B1, 0, c});
  b.launch(OP_CONV, b.phys_from({l_cv2}), Slice{X, 0, 2 * c}, out);
}

// YOLO11 (BscanBased/yolo/yolo_bbox_retrain.py trains yolo11n; upstream cfg/models/11/yolo11.yaml, Detect at
// model.23).  Depth 0.5: every repeated block has n = 1.  Names and canonical order: spec.py conv_specs_y11; block structure:
// tests/yolo11_det_ref.py.  The stem and every plain conv go through the planner's usual rules; the depthwise convs run on
// dwconv3x3.hip and the attention core on psa_attn.hip.
int build_graph_y11(m355_engine* e) {
  Builder b{e};
  if (int rc = b.begin(kY11)) return rc;
  const bool c3k_all = b.c3k_all;
  const int c64 = b.c64, c128 = b.c128, c256 = b.c256, c512 = b.c512, c1024 = b.c1024;
  const int H2 = b.H2, W2 = b.W2, H3 = b.H3, W3 = b.W3, H4 = b.H4, W4 = b.W4, H5 = b.H5, W5 = b.W5;
  // zero-copy concat buffers: cat12 = [up(x10), x6], cat15 = [up(x13), x4], cat18 = [x17, x13], cat21 = [x20, x10]
  const int cat12 = b.tensor(H4, W4, c1024 + c512), cat15 = b.tensor(H3, W3, c512 + c512);
  const int cat18 = b.tensor(H4, W4, c256 + c512), cat21 = b.tensor(H5, W5, c512 + c1024);
  const Slice x4{cat15, c512, c512}, x6{cat12, c1024, c512}, x10{cat21, c512, c1024}, x13{cat18, c256, c512};
  const int t0 = b.stem("model.0", c64, 3);
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
  b.sppf("model.9", Slice{t8, 0, c1024}, Slice{t9, 0, c1024});
  build_c2psa(e, b, "model.10", Slice{t9, 0, c1024}, x10);
  // 11/12 and 14/15: Upsample + Concat read through by the next C3k2's cv1 (M355_NO_UPFUSE: materialised by upsample2x)
  const int t16 = b.tensor(H3, W3, c256), t19 = b.tensor(H4, W4, c512), t22 = b.tensor(H5, W5, c1024);
  const Slice up13 = b.up(x10, Slice{cat12, 0, c1024});
  build_c3k2(e, b, "model.13", Slice{cat12, 0, c1024 + c512}, x13, c3k_all, 0.5, up13);
  const Slice up16 = b.up(x13, Slice{cat15, 0, c512});
  build_c3k2(e, b, "model.16", Slice{cat15, 0, c512 + c512}, Slice{t16, 0, c256}, c3k_all, 0.5, up16);
  b.conv("model.17", Slice{t16, 0, c256}, Slice{cat18, 0, c256}, 3, 2);
  build_c3k2(e, b, "model.19", Slice{cat18, 0, c256 + c512}, Slice{t19, 0, c512}, c3k_all, 0.5);
  b.conv("model.20", Slice{t19, 0, c512}, Slice{cat21, 0, c512}, 3, 2);
  build_c3k2(e, b, "model.22", Slice{cat21, 0, c512 + c1024}, Slice{t22, 0, c1024}, true, 0.5);
  const int feats[3] = {t16, t19, t22};
  const int fch[3] = {c256, c512, c1024};
  return build_detect_head_y11(e, b, feats, fch, "model.23");
}

// yolov8{n,s,m,l,x}-seg, and with `detect` YOLOv8 detect (upstream yolov8.yaml: the same backbone and neck, layer for layer, under
// the box-only Detect head at model.22).  (The tensors are made one by one between the convs here, in groups in the other three
// graphs: tensor ids follow that order.)
int build_graph_v8(m355_engine* e, bool detect) {
  Builder b{e};
  if (int rc = b.begin(detect ? kV8Det : kV8)) return rc;
  const int c64 = b.c64, c128 = b.c128, c256 = b.c256, c512 = b.c512, c1024 = b.c1024;
  const int H2 = b.H2, W2 = b.W2, H3 = b.H3, W3 = b.W3, H4 = b.H4, W4 = b.W4, H5 = b.H5, W5 = b.W5;
  if (c64 != 16 && c64 != 32 && c64 != 48 && c64 != 64 && c64 != 80)
    return e->fail(M355_ERR_INVALID, "unsupported stem width");

  // concat buffers (zero-copy): cat11=[up(x9), x6] cat14=[up(x12), x4] cat17=[x16, x12] cat20=[x19, x9]
  const int cat11 = b.tensor(H4, W4, c1024 + c512);
  const int cat14 = b.tensor(H3, W3, c512 + c256);
  const int cat17 = b.tensor(H4, W4, c256 + c512);
  const int cat20 = b.tensor(H5, W5, c512 + c1024);
  const Slice x4{cat14, c512, c256}, x6{cat11, c1024, c512}, x9{cat20, c512, c1024}, x12{cat17, c256, c512};

  const int t0 = b.stem("model.0", c64, 3);
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
  b.sppf("model.9", Slice{t8, 0, c1024}, x9);
  // 10/11 and 13/14: Upsample + Concat read through by the next C2f's cv1 (M355_NO_UPFUSE: materialised by upsample2x)
  const Slice up12 = b.up(x9, Slice{cat11, 0, c1024});
  b.c2f("model.12", Slice{cat11, 0, c1024 + c512}, x12, b.rep(3), false, up12);
  const Slice up15 = b.up(x12, Slice{cat14, 0, c512});
  const int t15 = b.tensor(H3, W3, c256);
  b.c2f("model.15", Slice{cat14, 0, c512 + c256}, Slice{t15, 0, c256}, b.rep(3), false, up15);
  b.conv("model.16", Slice{t15, 0, c256}, Slice{cat17, 0, c256}, 3, 2);
  const int t18 = b.tensor(H4, W4, c512);
  b.c2f("model.18", Slice{cat17, 0, c256 + c512}, Slice{t18, 0, c512}, b.rep(3), false);
  b.conv("model.19", Slice{t18, 0, c512}, Slice{cat20, 0, c512}, 3, 2);
  const int t21 = b.tensor(H5, W5, c1024);
  b.c2f("model.21", Slice{cat20, 0, c512 + c1024}, Slice{t21, 0, c1024}, b.rep(3), false);

  // 22: Segment head, or the Detect head
  const int feats[3] = {t15, t18, t21};
  const int fch[3] = {c256, c512, c1024};
  if (detect) return build_detect_head(e, b, feats, fch, "model.22");
  return build_segment_head(e, b, feats, fch, b.ch(256));
}

}  // namespace

int build_graph(m355_engine* e) {
  const int family = e->desc.scale >> 8;
  if (family == '5') return build_graph_v5u(e);
  if (family == '1') return build_graph_y11(e);
  if (family == '8') return build_graph_v8(e, true);
  if (family != 0) return e->fail(M355_ERR_INVALID, "unknown model family in the high byte of m355_model_desc.scale");
  return e->desc.scale == 'c' ? build_graph_v9c(e) : build_graph_v8(e, false);
}

}  // namespace m355
