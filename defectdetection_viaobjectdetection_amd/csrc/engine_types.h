// The engine's data model: tensors, logical and physical convs, ops and the engine itself.  graph.hip fills it with one of the
// four networks (build_graph); engine.hip fuses, plans, allocates and runs what it finds there.  Host only: no kernel file
// includes this header.
#pragma once
#include <string>
#include <vector>

#include "../../include/mi355yolo.h"
#include "common.h"
#include "switches.h"
#include "weight_pack.h"

// (nothing in this header is part of the library's surface: the C ABI sees m355_engine as an opaque pointer)
#pragma GCC visibility push(hidden)

namespace m355 {

struct Tensor {
  int H = 0, W = 0, C = 0;
  half_t* p = nullptr;  // (max_batch, H, W, C) fp16 NHWC
};

struct Slice {  // channel slice of a tensor
  int t = -1, off = 0, c = 0;
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
  int diag_n = 0;         // > 0: this 3x3 conv and the diag_n - 1 ops behind it sit side by side in one input and one output tensor (the second
                          // stage of a head level) and may run as ONE block-diagonal row-slab launch (conv3x3_planes.hip); set by the graph builder
  int diag_on = 0;        // ... and do: decided once at engine creation for all such groups together; the ops behind this one are fused away
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
  int diag_lead = -1;        // >= 0: member of a block-diagonal 3x3 launch; the index of the op that launches it (Op::diag_on)
  half_t* wf_diag = nullptr; // the launching op's conv only: the fragments of all members (planes_frag_pack_diag) and their biases,
  float* bias_diag = nullptr;   // side by side, padded to a multiple of 64 channels
};

}  // namespace m355

struct m355_engine {
  m355_model_desc desc{};
  m355::PlanSwitches sw{};   // the M355_* switches of graph construction and planning, as read at create
  std::string err;
  std::vector<m355::Tensor> tensors;
  std::vector<m355_conv_info> convs;   // logical convs (canonical order)
  std::vector<bool> conv_loaded;
  std::vector<int> conv_phys;          // logical -> physical
  std::vector<int> conv_phys_off;      // output-channel offset inside the physical conv
  std::vector<int> conv_phys_koff;     // input-channel (K) offset inside the physical conv (block-diagonal fusion)
  std::vector<m355::PhysConv> phys;
  std::vector<m355::Op> ops;
  int nc = 1, nm = 32, A = 0, n3 = 0, n4 = 0, n5 = 0;
  int proto_h = 0, proto_w = 0;
  float* raw = nullptr;      // (max_batch, A, 64+nc+nm) fp32
  m355::half_t* zero = nullptr;    // zero page
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
    m355::g_err = m;
    return code;
  }
};

#define HIP_TRY(e, call)                                                                            \
  do {                                                                                              \
    hipError_t _st = (call);                                                                        \
    if (_st != hipSuccess)                                                                          \
      return (e)->fail(M355_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_st));           \
  } while (0)

namespace m355 {

// graph.hip: the network that e->desc names, written into e as tensors, logical convs, physical convs and ops
int build_graph(m355_engine* e);

}  // namespace m355

#pragma GCC visibility pop
