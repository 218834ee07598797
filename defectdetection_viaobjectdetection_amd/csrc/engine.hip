// libmi355yolo.so engine: how a built graph runs.  The passes over the graph that graph.hip builds (conv + cv1 and decode fusion,
// stream lanes, sub-batches), allocation of the workspace, the kernel choice of every op (plan_route), weight upload (layouts:
// weight_pack.hip), m355_forward and the engine's C-ABI (include/mi355yolo.h; the per-op entries are in op_entries.hip).
// Host-side C++: this file has no kernel, all arithmetic is in the HIP kernel files it launches.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mi355yolo.h"
#include "common.h"
#include "engine_types.h"
#include "switches.h"
#include "weight_pack.h"

using namespace m355;

thread_local std::string m355::g_err;

namespace {

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

// the block-diagonal launch of op `lead` and the op.diag_n - 1 ops behind it (conv3x3_planes.hip, launch_conv3x3_blockdiag)
PlanesArgs diag_args(const m355_engine* e, size_t lead, int B, int b0) {
  const Op& op = e->ops[lead];
  const PhysConv& p = e->phys[op.conv];
  const Tensor& ti = e->tensors[op.in.t];
  const Tensor& to = e->tensors[op.out.t];
  PlanesArgs a{};
  a.x_bstride = (long)ti.H * ti.W * ti.C; a.ldx = ti.C; a.x = ti.p + op.in.off + b0 * a.x_bstride;
  a.H = ti.H; a.W = ti.W; a.B = B; a.act = 1; a.stride = 1;
  a.diag_n = std::min(op.diag_n, 4);
  for (int i = 0; i < a.diag_n && lead + i < e->ops.size(); ++i) {
    const PhysConv& q = e->phys[e->ops[lead + i].conv];
    a.diag_cin[i] = q.cin; a.diag_cout[i] = q.cout;
    a.Cin += q.cin; a.Cout += q.cout; a.cblocks_b += planes_cblocks(q.cout);
  }
  a.wfb = p.wf_diag; a.bb = p.bias_diag;
  a.y_bstride = (long)to.H * to.W * to.C; a.ldy = to.C; a.y = to.p + op.out.off + b0 * a.y_bstride;
  return a;
}

// Can the ops [lead, lead + diag_n) run as one block-diagonal launch?  Plain 3x3 / s1 Conv+SiLU layers on one lane whose input and
// output slices follow each other in one tensor each, and a shape the kernel takes at max_batch.
bool head_diag_ok(const m355_engine* e, size_t lead) {
  const Op& l = e->ops[lead];
  if (l.diag_n < 2 || l.diag_n > 4 || lead + l.diag_n > e->ops.size()) return false;
  int in_off = l.in.off, out_off = l.out.off;
  for (int i = 0; i < l.diag_n; ++i) {
    const Op& op = e->ops[lead + i];
    if (op.kind != OP_CONV || op.fused_away || op.stemfuse >= 0) return false;
    const PhysConv& p = e->phys[op.conv];
    if (p.k != 3 || p.stride != 1 || !p.act || p.diag || p.l3 >= 0 || p.groups != 1 || p.logical.size() != 1) return false;
    if (op.res.t >= 0 || op.in2.t >= 0 || op.out_ext != 0 || op.decode || op.lane != l.lane) return false;
    if (op.in.t != l.in.t || op.out.t != l.out.t || op.in.off != in_off || op.out.off != out_off || op.in.c != p.cin || op.out.c != p.cout) return false;
    if (i > 0 && (op.record || !op.wait_ops.empty())) return false;
    in_off += p.cin; out_off += p.cout;
  }
  PlanesArgs a = diag_args(e, lead, e->desc.max_batch, 0);
  a.wfb = (const half_t*)1; a.bb = (const float*)1;   // placeholders: packed when the weights arrive
  return conv3x3_blockdiag_ok(a);
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
        snprintf(op.layer, sizeof(op.layer), e->nm > 0 || (e->desc.scale >> 8) == '8' ? "model.22.decode" : (e->desc.scale >> 8) == '1' ? "model.23.decode" : "model.24.decode");
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
  // the second 3x3 stage of the head levels (cv2.l.1 + cv3.l.1 + cv4.l.1) as one block-diagonal row-slab launch per level: every
  // level the graph marked, or none (the three launches)
  bool diag_all = !e->sw.no_headdiag && !e->sw.no_planes && e->nm == 32 && e->nc <= 32;   // (the head the kernel was measured on: widths 64 / 128 / 32)
  size_t diag_groups = 0;
  for (size_t i = 0; i < e->ops.size(); ++i)
    if (e->ops[i].diag_n > 0) {
      ++diag_groups;
      diag_all = diag_all && head_diag_ok(e, i) && e->ops[i].diag_n == 3 && e->ops[i].in.c == 64 && e->ops[i + 1].in.c == 128 && e->ops[i + 2].in.c == 32;
    }
  for (size_t i = 0; diag_all && diag_groups && i < e->ops.size(); ++i) {
    Op& lead = e->ops[i];
    if (lead.diag_n <= 0) continue;
    const Tensor& t = e->tensors[lead.in.t];
    lead.diag_on = 1;
    snprintf(lead.kernel, sizeof(lead.kernel), "conv3x3_planes<64ch,rows,diag>");
    int cin = 0, cout = 0;
    for (int j = 0; j < lead.diag_n; ++j) {
      Op& m = e->ops[i + j];
      PhysConv& p = e->phys[m.conv];
      p.diag_lead = (int)i;
      cin += p.cin; cout += p.cout;
      if (j == 0) continue;
      // "model.22.cv2.1.1+cv3.1.1+cv4.1.1": the members' names without the module prefix
      const char* nm = e->convs[p.logical[0]].name;
      const char* d1 = strchr(nm, '.');
      const char* d2 = d1 ? strchr(d1 + 1, '.') : nullptr;
      const size_t len = strlen(lead.layer);
      snprintf(lead.layer + len, sizeof(lead.layer) - len, "+%s", d2 ? d2 + 1 : nm);
      lead.flops += m.flops; lead.wbytes += m.wbytes;   // (a block-diagonal fusion counts its diagonal blocks only)
      m.flops = m.bytes = m.wbytes = 0;
      m.fused_away = true;
      snprintf(m.kernel, sizeof(m.kernel), "(none)");
    }
    lead.bytes = (double)t.H * t.W * (cin + cout) * 2;
  }
}

// device copy of a fragment-ordered weight list (allocated on first use)
hipError_t put_frags(half_t** dst, const std::vector<half_t>& fp) {
  const size_t bytes = fp.size() * sizeof(half_t);
  const hipError_t st = *dst ? hipSuccess : hipMalloc((void**)dst, bytes);
  return st != hipSuccess ? st : hipMemcpy(*dst, fp.data(), bytes, hipMemcpyHostToDevice);
}

// A head level's block-diagonal second stage (Op::diag_on): fragments and biases of all members, once their weights are here
int pack_head_diag(m355_engine* e, size_t lead, int idx_now) {
  const Op& l = e->ops[lead];
  std::vector<std::vector<half_t>> rows(l.diag_n);
  std::vector<float> bias;
  const half_t* rp[4];
  int cout[4], kpad[4], cin[4];
  for (int i = 0; i < l.diag_n; ++i) {
    const PhysConv& p = e->phys[e->ops[lead + i].conv];
    if (p.logical[0] != idx_now && !e->conv_loaded[p.logical[0]]) return M355_OK;
    rows[i].resize((size_t)p.cout * p.Kpad);
    HIP_TRY(e, hipMemcpy(rows[i].data(), p.w, rows[i].size() * sizeof(half_t), hipMemcpyDeviceToHost));
    bias.resize(bias.size() + p.cout);
    HIP_TRY(e, hipMemcpy(bias.data() + bias.size() - p.cout, p.bias, p.cout * sizeof(float), hipMemcpyDeviceToHost));
    rp[i] = rows[i].data(); cout[i] = p.cout; kpad[i] = p.Kpad; cin[i] = p.cin;
  }
  bias.resize((bias.size() + 63) / 64 * 64, 0.f);
  PhysConv& pl = e->phys[l.conv];
  HIP_TRY(e, put_frags(&pl.wf_diag, planes_frag_pack_diag(rp, cout, kpad, cin, l.diag_n)));
  if (!pl.bias_diag) HIP_TRY(e, hipMalloc((void**)&pl.bias_diag, bias.size() * sizeof(float)));
  HIP_TRY(e, hipMemcpy(pl.bias_diag, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
  return M355_OK;
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
                   : fam == '8' ? (sc == 'n' || sc == 's' || sc == 'm' || sc == 'l' || sc == 'x')
                                : (fam == '5' || fam == '1') && (sc == 'n' || sc == 's' || sc == 'm');
    if (!ok) {
      g_err = "m355_model_desc.scale: unknown family or scale (0 | n,s,m,l,x,c; ('5' << 8) | n,s,m; ('1' << 8) | n,s,m; ('8' << 8) | n,s,m,l,x)";
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
    if (p.wf_diag) (void)hipFree(p.wf_diag);
    if (p.bias_diag) (void)hipFree(p.bias_diag);
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
    if (p.diag_lead >= 0) {
      const int rcd = pack_head_diag(e, (size_t)p.diag_lead, idx);
      if (rcd != M355_OK) return rcd;
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
        if (op.diag_on) {   // this conv and its neighbours in one block-diagonal launch (planned at creation: no other form is kept)
          rc = launch_conv3x3_blockdiag(diag_args(e, oi, Bq, b0), s);
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
