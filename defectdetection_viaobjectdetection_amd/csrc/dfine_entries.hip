// libmi355yolo.so C entries of the D-FINE ops (include/mi355yolo.h: m355_msda_*, m355_dfine_*) and their workspace queries.
// Every entry validates on the host, before any HIP call and in this order: null pointers, shape and range (every grid dimension
// that an argument decides included), workspace, alignment.  Then it launches and reports the launcher's HIP status; the
// launchers (dfine_*.hip) validate nothing.  A refused call has queued nothing.
#include <initializer_list>
#include <string>

#include "../../include/mi355yolo.h"
#include "common.h"
#include "weight_pack.h"

using namespace m355;

namespace {

constexpr long kGridMax = 0x7fffffffL;   // blocks of one launch
const char* const kAlign16 = "pointers must be 16-byte aligned";

// fn: the entry's __func__; its messages carry that name without the "m355_"
int invalid(const char* fn, const std::string& why) { return set_err(M355_ERR_INVALID, std::string(fn + 5) + ": " + why); }
int launched(const char* fn, int rc) {
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, std::string(fn + 5) + " launch failed: " + std::to_string(rc));
}
bool any_null(std::initializer_list<const void*> ps) {
  for (const void* p : ps) if (!p) return true;
  return false;
}
bool any_misaligned16(std::initializer_list<const void*> ps) {   // nullptr (an optional tensor left out) counts as aligned
  for (const void* p : ps) if ((uintptr_t)p & 15u) return true;
  return false;
}
bool workspace_short(const void* work, int64_t bytes, size_t need) { return !work || bytes < 0 || (size_t)bytes < need; }

// The level table of the msda kernels, forward and backward, from the caller's (h, w) pairs and points per level.
// nullptr = accepted and lv filled, else the reason.
const char* msda_levels(const int32_t* shapes_hw, int L, const int32_t* points_per_level, int S, int Q, int P, MsdaLevels& lv) {
  if (L < 1 || L > 8) return "1..8 levels tiling S";
  lv = {}; lv.L = L;
  long start = 0, pend = 0;
  for (int l = 0; l < L; ++l) {
    const int h = shapes_hw[2 * l], w = shapes_hw[2 * l + 1], n = points_per_level[l];
    if (h < 1 || w < 1 || n < 0) return "every level needs h, w >= 1 and a point count >= 0";
    if ((long)h * w > 0x7fffffffL - start) return "1..8 levels tiling S";   // pixels are indexed with int
    if ((pend += n) > P) return "points tiling P";
    lv.lh[l] = h; lv.lw[l] = w; lv.lstart[l] = (int)start; lv.pend[l] = (int)pend;
    start += (long)h * w;
  }
  if (start != S) return "1..8 levels tiling S";
  if (pend != P) return "points tiling P";
  // entries of one (b, h) contribution list are indexed with int: 4 Q P of them, level l's segment starts at 4 Q pend[l - 1]
  if ((long)Q * P > 0x7fffffffL / 4) return "4 * Q * P must fit in int";
  return nullptr;
}

// What the four msda entries check after their null pointers.  max_points: 32, module mode (the wave kernel: bilinear) 16.
// The backward passes grad_value (asked for: its owner-computes launch has a grid too) and, when the gradients asked for need
// the workspace, `work`.  nullptr = accepted and lv filled, else the reason.
const char* msda_check(int B, int S, int H, int D, const int32_t* shapes_hw, int L, const int32_t* points_per_level, int Q, int P,
                       int max_points, MsdaLevels& lv, const void* grad_value = nullptr, bool needs_work = false,
                       const void* work = nullptr, int64_t work_bytes = 0) {
  if (D != 32) return "head_dim must be 32";
  if (B < 1 || Q < 1 || H < 1) return "B, Q and heads must be >= 1";
  if (P < 1 || P > max_points) return max_points == 16 ? "1..16 points tiling P" : "1..32 points tiling P";
  if (const char* why = msda_levels(shapes_hw, L, points_per_level, S, Q, P, lv)) return why;
  // (B Q H + 3) / 4 blocks of one wave per (b, q, h); it bounds the (B Q + 127) / 128 blocks of the grad_ref kernel too
  if ((long)B * Q > 4 * kGridMax / H) return "B * Q * heads is too large for one launch";
  int own, blk0[9];
  if (grad_value && msda_backward_value_blocks(lv, B, H, &own, blk0) > kGridMax) return "B * heads * S is too large for one launch";
  if (needs_work && workspace_short(work, work_bytes, msda_backward_workspace_bytes(B, Q, H, P)))
    return "workspace missing or smaller than m355_msda_backward_workspace_bytes";
  if (needs_work && any_misaligned16({work})) return "workspace 16-byte aligned";
  return nullptr;
}

// the argument checks m355_dfine_loss_forward and _backward share; nullptr = accepted, else the message
const char* dfine_loss_check(const DfineLossArgs& a) {
  if (a.B < 1 || a.Q < 1 || a.C < 1 || (int64_t)a.B * a.Q > INT32_MAX) return "B, Q, C >= 1 and B * Q < 2^31";
  if (a.M < 0 || a.T < 0) return "M >= 0 and T >= 0";
  if (!a.logits || !a.boxes || !a.out || !(a.num_boxes > 0.f)) return "null pointer (logits, pred_boxes, out) or num_boxes <= 0";
  if (a.M > 0 && a.T > 0 && (!a.match_q || !a.match_t || !a.offsets || !a.labels || !a.tboxes))
    return "null pointer in the match list or the targets";
  const int local = (a.pred_corners != nullptr) + (a.ref_points != nullptr) + (a.teacher_corners != nullptr) +
                    (a.teacher_logits != nullptr) + (a.project != nullptr);
  if (local != 0 && local != 5) return "the local group (pred_corners, ref_points, teacher_corners, teacher_logits, project) is all or none";
  if (local && (a.nb1 < 2 || a.nb1 > 64 || a.reg_scale == 0.f || !(a.temperature > 0.f)))
    return "2 <= bins + 1 <= 64, reg_scale != 0, temperature > 0";
  return nullptr;
}
DfineLossArgs dfine_loss_args(const float* logits, const float* boxes, int B, int Q, int C, const int64_t* mq, const int64_t* mt,
                              int M, const int32_t* offsets, const int64_t* labels, const float* tboxes, int T, float num_boxes,
                              float alpha, float gamma, const float* corners, const float* ref, const float* tcorners,
                              const float* tlogits, const float* project, int nb1, float reg_scale, float temperature) {
  DfineLossArgs a{};
  a.logits = logits; a.boxes = boxes; a.match_q = (const long long*)mq; a.match_t = (const long long*)mt; a.offsets = offsets;
  a.labels = (const long long*)labels; a.tboxes = tboxes; a.B = B; a.Q = Q; a.C = C; a.M = M; a.T = T;
  a.num_boxes = num_boxes; a.alpha = alpha; a.gamma = gamma;
  a.pred_corners = corners; a.ref_points = ref; a.teacher_corners = tcorners; a.teacher_logits = tlogits; a.project = project;
  a.nb1 = nb1; a.reg_scale = reg_scale; a.temperature = temperature;
  return a;
}

// the temporal encoder layer between its GEMMs (dfine_encoder.hip); nullptr = accepted, else the message
const char* dfine_dropout_check(float p, int32_t site) {
  if (!(p >= 0.f && p < 1.f)) return "dropout p must be in [0, 1)";
  if (site < 0) return "the dropout site id must be >= 0";
  return nullptr;
}
const char* dfine_attn_check(int32_t B, int32_t S, int32_t H, int32_t head_dim, float p, int32_t site) {
  if (head_dim != 32) return "head dim must be 32";
  if (B < 1 || B > 65535 || S < 1 || H < 1 || H > 65535) return "B and heads in [1, 65535], S >= 1";
  if ((int64_t)B * S * 96 * H > (int64_t)1 << 40 || (int64_t)S > (int64_t)1 << 24) return "S <= 2^24 and B * S * 3 D <= 2^40";
  return dfine_dropout_check(p, site);
}
const char* dfine_addln_check(int64_t M, int32_t D, float p, int32_t site) {
  if (M < 1 || M > (int64_t)1 << 31) return "1 <= rows <= 2^31";
  if (D < 4 || D % 4 != 0 || D > dfine_addln_max_d()) return "D must be a multiple of 4 in [4, 1024]";
  return dfine_dropout_check(p, site);
}
// the query selection (dfine_select.hip): one block per image, K rows from the sort of topk_select.h, tokens and rows indexed with int
const char* dfine_select_check(int32_t B, int32_t S, int32_t C, int32_t K) {
  if (B < 1 || C < 1 || S < 1 || S >= 1 << 24) return "B >= 1, C >= 1, 1 <= S < 2^24";
  if (K < 1 || K > S || K > 2048) return "1 <= K <= min(S, 2048)";
  if ((int64_t)B * S > kGridMax) return "B * S must be below 2^31";
  return nullptr;
}
// the LQE statistics (dfine_decoder.hip): one block per row
const char* dfine_lqe_check(int64_t M, int32_t nb1, int32_t k) {
  if (M < 1 || M > kGridMax) return "1 <= rows < 2^31";
  if (k < 1 || k > 8 || nb1 < k || nb1 > 64) return "top_k in [1, 8] and top_k <= bins + 1 <= 64";
  return nullptr;
}
// the box decode, plain and guarded, forward and backward: (n + 127) / 128 blocks
const char* dfine_decode_check(int64_t n, int32_t nb1, float reg_scale) {
  if (n < 0 || nb1 < 2 || reg_scale == 0.f) return "n < 0, fewer than 2 bins or reg_scale == 0";
  if (n > 128 * kGridMax) return "n is too large for one launch";
  return nullptr;
}
// the decoder's own loop (dfine_loop.hip).  query_pos: (ceil(N / 4) * H / 4 + 255) / 256 blocks forward
const char* dfine_query_pos_check(int64_t N, int32_t H) {
  if (H < 4 || H % 4 != 0 || H > 2048) return "H must be a multiple of 4 in [4, 2048]";
  if (N < 1 || N > (int64_t)1 << 31) return "1 <= rows <= 2^31";
  return nullptr;
}
// refine_boxes, forward and backward: (N + 31) / 32 blocks
const char* dfine_refine_boxes_check(int64_t N, int32_t nb1, float reg_scale) {
  if (N < 1 || N > (int64_t)1 << 31) return "1 <= rows <= 2^31";
  if (nb1 < 2 || nb1 > 64 || reg_scale == 0.f) return "2 <= bins + 1 <= 64 and reg_scale != 0";
  return nullptr;
}
// the temporal head (dfine_temporal.hip).  temporal_fuse: a block per query column, its T partial sums in LDS
const char* dfine_tfuse_check(int32_t T, int32_t Q, int32_t D) {
  if (T < 1 || T > dfine_tfuse_max_t() || D < 1 || D > 1024) return "T and D must be in [1, 1024]";
  if (Q < 1 || Q > 1 << 20) return "1 <= Q <= 2^20";
  return nullptr;
}
const char* dfine_guard_logits_check(int64_t rows, int32_t C1, bool anomaly, float bound) {
  if (rows < 1 || C1 < 1 || rows > ((int64_t)1 << 40) / C1) return "rows >= 1, C1 >= 1, rows * C1 <= 2^40";
  if (anomaly && C1 < 2) return "anomaly scores need C1 >= 2";
  if (!(bound >= 0.f)) return "bound must be >= 0";
  return nullptr;
}
const char* dfine_noobject_check(int32_t T, int32_t Q, int32_t C1, int32_t cls) {
  if (T < 1 || Q < 1 || Q > dfine_noobject_max_q() || C1 < 1 || C1 > 1024) return "T >= 1, Q in [1, 2048], C1 in [1, 1024]";
  if (cls < 0 || cls >= C1) return "0 <= class_index < C1";
  return nullptr;
}
const char* dfine_consistency_check(int32_t T, int64_t N) {
  if (T < 2 || N < 1 || N > (int64_t)1 << 27 || (int64_t)T * N > kGridMax) return "T >= 2, 1 <= N <= 2^27, T * N < 2^31";
  return nullptr;
}

// the map / token layout kernels (dfine_layout.hip): the level table from the caller's (h, w) pairs, and everything the two entries
// check after their top-level null pointers.  nullptr = accepted and lv filled, else the reason
const char* dfine_layout_check(const float* const* maps, const int32_t* shapes_hw, int L, int B, int D, DfineLayoutLevels& lv) {
  if (L < 1 || L > 8) return "1..8 levels";
  for (int l = 0; l < L; ++l) if (!maps[l]) return "null pointer";
  if (B < 1) return "B >= 1";
  if (D < 4 || D % 4 != 0 || D > 1024) return "D must be a multiple of 4 in [4, 1024]";
  lv = {}; lv.L = L;
  long start = 0;
  for (int l = 0; l < L; ++l) {
    const int h = shapes_hw[2 * l], w = shapes_hw[2 * l + 1];
    if (h < 1 || w < 1) return "every level needs h, w >= 1";
    if ((long)h * w > 0x7fffffffL - start) return "S must be below 2^31";
    lv.hw[l] = h * w; lv.start[l] = (int)start;
    start += (long)h * w;
  }
  lv.S = start;
  if (dfine_layout_blocks(lv, B, D) > kGridMax) return "B * S * D is too large for one launch";
  for (int l = 0; l < L; ++l) if ((uintptr_t)maps[l] & 15u) return kAlign16;
  return nullptr;
}

// the table of the optimizer entries (dfine_optim.hip): one block per chunk, found from the rows' chunk0 prefix.  adam: p, m, v are
// used too.  nullptr = accepted and *chunks = the grid, else the message
const char* dfine_optim_check(const m355_dfine_optim_row* h, const m355_dfine_optim_row* d, int32_t count, bool adam, int* chunks) {
  if (!h || !d) return "null table";
  if (count < 1 || count > M355_DFINE_OPTIM_MAX_TENSORS) return "the tensor count must be in [1, 65536]";
  int64_t total = 0;
  for (int i = 0; i < count; ++i) {
    const m355_dfine_optim_row& r = h[i];
    if (r.numel < 0) return "negative numel";
    if (((uintptr_t)r.p | (uintptr_t)r.g | (uintptr_t)r.m | (uintptr_t)r.v) & 3u) return "pointers must be 4-byte aligned";
    if (r.numel > 0 && (!r.g || (adam && (!r.p || !r.m || !r.v)))) return "null pointer in a row with elements";
    if (r.chunk0 != total) return "chunk0 is not the number of chunks of the rows before it";
    total += (r.numel + M355_DFINE_OPTIM_CHUNK - 1) / M355_DFINE_OPTIM_CHUNK;   // numel <= 2^63 - 1: no overflow before the test
    if (total > kGridMax) return "more chunks than one launch can index (2^31 - 1)";
  }
  if (total < 1) return "no elements";
  *chunks = (int)total;
  return nullptr;
}

}  // namespace

int m355_msda_forward(const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim, const int32_t* shapes_hw,
                      int32_t num_levels, const float* d_loc, const float* d_attn, const int32_t* points_per_level,
                      int32_t Q, int32_t P, int32_t discrete, float* d_out, void* stream) {
  if (any_null({d_value, d_loc, d_attn, d_out, shapes_hw, points_per_level})) return invalid(__func__, "null pointer");
  MsdaLevels lv;
  if (const char* why = msda_check(B, S, heads, head_dim, shapes_hw, num_levels, points_per_level, Q, P, 32, lv)) return invalid(__func__, why);
  return launched(__func__, launch_msda(d_value, d_loc, d_attn, d_out, B, S, heads, Q, P, lv, discrete, (hipStream_t)stream));
}
int m355_msda_module_forward(const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim, const int32_t* shapes_hw,
                             int32_t num_levels, const float* d_ref, const float* d_offsets, const float* d_logits,
                             const int32_t* points_per_level, int32_t Q, int32_t P, float offset_scale, float* d_out,
                             void* stream) {
  if (any_null({d_value, d_ref, d_offsets, d_logits, d_out, shapes_hw, points_per_level})) return invalid(__func__, "null pointer");
  MsdaLevels lv;
  if (const char* why = msda_check(B, S, heads, head_dim, shapes_hw, num_levels, points_per_level, Q, P, 16, lv)) return invalid(__func__, why);
  return launched(__func__, launch_msda(d_value, d_offsets, d_logits, d_out, B, S, heads, Q, P, lv, 0, (hipStream_t)stream, d_ref, offset_scale));
}
size_t m355_msda_backward_workspace_bytes(int32_t B, int32_t Q, int32_t heads, int32_t P) { return msda_backward_workspace_bytes(B, Q, heads, P); }
int m355_msda_backward(const float* d_grad_out, const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim,
                       const int32_t* shapes_hw, int32_t num_levels, const float* d_loc, const float* d_attn,
                       const int32_t* points_per_level, int32_t Q, int32_t P, int32_t discrete, float* d_grad_value,
                       float* d_grad_loc, float* d_grad_attn, void* d_work, int64_t work_bytes, void* stream) {
  if (any_null({d_grad_out, d_value, d_loc, d_attn, shapes_hw, points_per_level})) return invalid(__func__, "null pointer");
  MsdaLevels lv;   // the workspace holds the contribution list of grad_value
  if (const char* why = msda_check(B, S, heads, head_dim, shapes_hw, num_levels, points_per_level, Q, P, 32, lv, d_grad_value,
                                   d_grad_value != nullptr, d_work, work_bytes))
    return invalid(__func__, why);
  return launched(__func__, launch_msda_backward(d_grad_out, d_value, d_loc, d_attn, d_grad_value, d_grad_loc, d_grad_attn, B, S, heads,
                                                 Q, P, lv, discrete, d_work, (hipStream_t)stream));
}
int m355_msda_module_backward(const float* d_grad_out, const float* d_value, int32_t B, int32_t S, int32_t heads, int32_t head_dim,
                              const int32_t* shapes_hw, int32_t num_levels, const float* d_ref, const float* d_offsets,
                              const float* d_logits, const int32_t* points_per_level, int32_t Q, int32_t P, float offset_scale,
                              float* d_grad_value, float* d_grad_ref, float* d_grad_offsets, float* d_grad_logits, void* d_work,
                              int64_t work_bytes, void* stream) {
  // d_ref is required, so d_grad_ref never comes without it
  if (any_null({d_grad_out, d_value, d_ref, d_offsets, d_logits, shapes_hw, points_per_level})) return invalid(__func__, "null pointer");
  MsdaLevels lv;   // the workspace holds the contribution list of grad_value and the per-head partials of grad_ref
  if (const char* why = msda_check(B, S, heads, head_dim, shapes_hw, num_levels, points_per_level, Q, P, 16, lv, d_grad_value,
                                   d_grad_value || d_grad_ref, d_work, work_bytes))
    return invalid(__func__, why);
  return launched(__func__, launch_msda_backward(d_grad_out, d_value, d_offsets, d_logits, d_grad_value, d_grad_offsets, d_grad_logits,
                                                 B, S, heads, Q, P, lv, 0, d_work, (hipStream_t)stream, d_ref, offset_scale, d_grad_ref));
}
int m355_dfine_decode(const float* d_dist, const float* d_project, const float* d_ref, float* d_boxes, int64_t n,
                      int32_t num_bins_plus1, float reg_scale, int32_t clamp01, void* stream) {
  if (any_null({d_dist, d_project, d_ref, d_boxes})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_decode_check(n, num_bins_plus1, reg_scale)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_decode(d_dist, d_project, d_ref, d_boxes, (long)n, num_bins_plus1, reg_scale, clamp01, (hipStream_t)stream));
}
int m355_dfine_decode_backward(const float* d_grad_boxes, const float* d_dist, const float* d_project, const float* d_ref,
                               float* d_grad_dist, float* d_grad_ref, int64_t n, int32_t num_bins_plus1, float reg_scale,
                               int32_t clamp01, void* stream) {
  if (any_null({d_grad_boxes, d_dist, d_project, d_ref})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_decode_check(n, num_bins_plus1, reg_scale)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_decode_backward(d_grad_boxes, d_dist, d_project, d_ref, d_grad_dist, d_grad_ref, (long)n,
                                                         num_bins_plus1, reg_scale, clamp01, (hipStream_t)stream));
}
int m355_dfine_decode_guarded(const float* d_dist, const float* d_project, const float* d_ref, float* d_boxes, int64_t n,
                              int32_t num_bins_plus1, float reg_scale, int32_t clamp01, void* stream) {
  if (any_null({d_dist, d_project, d_ref, d_boxes})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_decode_check(n, num_bins_plus1, reg_scale)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_decode(d_dist, d_project, d_ref, d_boxes, (long)n, num_bins_plus1, reg_scale, clamp01,
                                                (hipStream_t)stream, true));
}
int m355_dfine_decode_guarded_backward(const float* d_grad_boxes, const float* d_dist, const float* d_project, const float* d_ref,
                                       float* d_grad_dist, float* d_grad_ref, int64_t n, int32_t num_bins_plus1, float reg_scale,
                                       int32_t clamp01, void* stream) {
  if (any_null({d_grad_boxes, d_dist, d_project, d_ref})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_decode_check(n, num_bins_plus1, reg_scale)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_decode_backward(d_grad_boxes, d_dist, d_project, d_ref, d_grad_dist, d_grad_ref, (long)n,
                                                         num_bins_plus1, reg_scale, clamp01, (hipStream_t)stream, true));
}
size_t m355_dfine_match_workspace_bytes(int32_t B, int32_t Q, int32_t max_targets) { return dfine_match_workspace_bytes(B, Q, max_targets); }
int m355_dfine_match(const float* d_logits, const float* d_pred_boxes, int32_t B, int32_t Q, int32_t C,
                     const int64_t* d_target_labels, const float* d_target_boxes, const int32_t* d_target_offsets,
                     const int32_t* h_target_counts, float class_cost, float bbox_cost, float giou_cost, float alpha, float gamma,
                     int32_t use_focal_loss, void* d_work, int64_t work_bytes, float* d_cost, int64_t* d_rows, int64_t* d_cols,
                     int32_t kmax, int32_t* d_flags, void* stream) {
  if (any_null({d_logits, d_pred_boxes, d_target_labels, d_target_boxes, d_target_offsets, h_target_counts, d_rows, d_cols, d_flags}))
    return invalid(__func__, "null pointer");
  if (B < 1 || B > 65535 || Q < 1 || Q > 2048 || C < 1) return invalid(__func__, "B >= 1, Q in [1, 2048], C >= 1");
  int nmax = 0;
  long total = 0;
  for (int b = 0; b < B; ++b) {
    const int n = h_target_counts[b];
    if (n < 0 || n > 512) return invalid(__func__, "every target count must be in [0, 512]");
    nmax = n > nmax ? n : nmax;
    total += n;
  }
  if (kmax < (Q < nmax ? Q : nmax)) return invalid(__func__, "kmax is smaller than min(Q, largest target count)");
  const size_t need = dfine_match_workspace_bytes(B, Q, nmax);
  if (need > 0 && workspace_short(d_work, work_bytes, need))
    return invalid(__func__, "workspace missing or smaller than m355_dfine_match_workspace_bytes");
  return launched(__func__, launch_dfine_match(d_logits, d_pred_boxes, B, Q, C, (const long long*)d_target_labels, d_target_boxes,
                                               d_target_offsets, (int)total, nmax, class_cost, bbox_cost, giou_cost, alpha, gamma,
                                               use_focal_loss != 0, d_work, d_cost, (long long*)d_rows, (long long*)d_cols, kmax,
                                               d_flags, (hipStream_t)stream));
}
int m355_dfine_postprocess(const float* d_logits, const float* d_pred_boxes, int32_t B, int32_t Q, int32_t C, const float* d_sizes,
                           float threshold, float* d_scores, int64_t* d_labels, float* d_boxes, int32_t* d_counts, void* stream) {
  if (any_null({d_logits, d_pred_boxes, d_scores, d_labels, d_boxes, d_counts})) return invalid(__func__, "null pointer");
  if (B < 1 || Q < 1 || Q > 2048 || C < 1 || (int64_t)Q * C >= (int64_t)1 << 24)
    return invalid(__func__, "B >= 1, Q in [1, 2048], C >= 1, Q * C < 2^24");
  return launched(__func__, launch_dfine_postprocess(d_logits, d_pred_boxes, B, Q, C, d_sizes, threshold, d_scores, (long long*)d_labels,
                                                     d_boxes, d_counts, (hipStream_t)stream));
}
int m355_dfine_preprocess(const uint8_t* d_src, int64_t src_bytes, const m355_dfine_pre_image* h_images,
                          const m355_dfine_pre_image* d_images, int32_t T, const m355_dfine_pre_axis* h_axes,
                          const m355_dfine_pre_axis* d_axes, int32_t n_axes, const int32_t* h_pool, const int32_t* d_pool,
                          int64_t pool_len, const float* d_rescale, int32_t out_h, int32_t out_w, void* d_work, int64_t work_bytes,
                          float* d_out, void* stream) {
  if (any_null({d_src, h_images, d_images, d_rescale, d_out})) return invalid(__func__, "null pointer");
  if (n_axes < 0 || pool_len < 0 || (n_axes > 0 && any_null({h_axes, d_axes, h_pool, d_pool})))
    return invalid(__func__, "axis tables missing");
  if (T < 1 || T > 65535) return invalid(__func__, "T in [1, 65535]");
  if (out_h < 1 || out_h > M355_DFINE_PRE_MAX_H || out_w < 4 || out_w > M355_DFINE_PRE_MAX_W || out_w % 4)
    return invalid(__func__, "out_h in [1, 16384], out_w a multiple of 4 in [4, 4096]");
  if (src_bytes < 0 || src_bytes % 16) return invalid(__func__, "src_bytes must be a multiple of 16");
  // every value a kernel indexes with comes from these tables: none is used unchecked
  constexpr int32_t kCoefMax = 1 << 23;
  for (int a = 0; a < n_axes; ++a) {
    const m355_dfine_pre_axis& ax = h_axes[a];
    const std::string which = "axis " + std::to_string(a) + ": ";
    if (ax.in_size < 1 || ax.in_size > M355_DFINE_PRE_MAX_H || ax.out_size < 1 || ax.out_size > M355_DFINE_PRE_MAX_H)
      return invalid(__func__, which + "sizes in [1, 16384]");
    if (ax.ksize < 1 || ax.ksize > M355_DFINE_PRE_MAX_TAPS) return invalid(__func__, which + "tap count above the kernel's maximum of 64 (or below 1)");
    if (ax.offset < 0 || (int64_t)ax.offset + (int64_t)ax.out_size * (2 + ax.ksize) > pool_len)
      return invalid(__func__, which + "the table leaves the pool");
    const int32_t* const xmin = h_pool + ax.offset;
    const int32_t* const count = xmin + ax.out_size;
    const int32_t* const coef = count + ax.out_size;
    for (int i = 0; i < ax.out_size; ++i) {
      if (count[i] < 1 || count[i] > ax.ksize) return invalid(__func__, which + "tap count outside [1, ksize]");
      if (xmin[i] < 0 || xmin[i] > ax.in_size - count[i]) return invalid(__func__, which + "xmin + count > in");
      int64_t sum = 0;
      for (int t = 0; t < count[i]; ++t) {
        const int32_t c = coef[(size_t)i * ax.ksize + t];
        if (c < 0 || c > kCoefMax) return invalid(__func__, which + "coefficient outside [0, 2^23]");
        sum += c;
      }
      if (sum > kCoefMax) return invalid(__func__, which + "coefficients of an output sum above 2^23");
    }
  }
  int64_t mid_rows = 0;
  int h_max_rows = 0, h_max_w = 0;
  for (int i = 0; i < T; ++i) {
    const m355_dfine_pre_image& im = h_images[i];
    const std::string which = "image " + std::to_string(i) + ": ";
    if (im.in_h < 1 || im.in_h > M355_DFINE_PRE_MAX_H || im.in_w < 1 || im.in_w > M355_DFINE_PRE_MAX_W)
      return invalid(__func__, which + "in_h in [1, 16384], in_w in [1, 4096]");
    if (im.offset < 0 || im.offset % 16 || im.offset > src_bytes - 3LL * im.in_h * im.in_w)
      return invalid(__func__, which + "offset negative, not a multiple of 16, or the image leaves the packed buffer");
    const struct { int32_t tab, in, out; const char* name; } pass[2] = {{im.htab, im.in_w, out_w, "horizontal"},
                                                                       {im.vtab, im.in_h, out_h, "vertical"}};
    for (const auto& p : pass) {
      if (p.tab == -1 ? p.in != p.out
                      : (p.tab < 0 || p.tab >= n_axes || h_axes[p.tab].in_size != p.in || h_axes[p.tab].out_size != p.out))
        return invalid(__func__, which + p.name + " table index is neither -1 with in == out nor an axis of its (in, out)");
    }
    if (im.htab >= 0) {
      if (im.mid_row != mid_rows) return invalid(__func__, which + "mid_row is not the sum of the earlier images' rows");
      mid_rows += im.in_h;
      if (mid_rows > INT32_MAX) return invalid(__func__, "the scratch rows must stay below 2^31");
      h_max_rows = im.in_h > h_max_rows ? im.in_h : h_max_rows;
      h_max_w = im.in_w > h_max_w ? im.in_w : h_max_w;
    }
  }
  if (mid_rows > 0 && workspace_short(d_work, work_bytes, (size_t)mid_rows * out_w * 3))
    return invalid(__func__, "scratch missing or smaller than 3 * out_w bytes per row of every image with a horizontal pass");
  if (any_misaligned16({d_src, d_work, d_out})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_preprocess(d_src, d_images, T, d_axes, d_pool, d_rescale, out_h, out_w, (uint8_t*)d_work,
                                                    h_max_rows, h_max_w, d_out, (hipStream_t)stream));
}
size_t m355_dfine_select_workspace_bytes(int32_t B, int32_t S) {
  return dfine_select_check(B, S, 1, 1) ? 0 : dfine_select_workspace_bytes(B, S);
}
int m355_dfine_select_forward(const float* d_class_logits, const float* d_coord_logits, const float* d_memory, int32_t B, int32_t S,
                              int32_t C, int32_t D, int32_t K, void* d_work, int64_t work_bytes, int64_t* d_indices, float* d_ref,
                              float* d_boxes, float* d_logits, float* d_target, int32_t* d_inverse, void* stream) {
  if (any_null({d_class_logits, d_coord_logits, d_indices, d_ref, d_boxes, d_logits})) return invalid(__func__, "null pointer");
  if ((d_memory == nullptr) != (d_target == nullptr)) return invalid(__func__, "memory and target come together or not at all");
  if (const char* why = dfine_select_check(B, S, C, K)) return invalid(__func__, why);
  if (d_memory && D < 1) return invalid(__func__, "D >= 1");
  if (workspace_short(d_work, work_bytes, dfine_select_workspace_bytes(B, S)))
    return invalid(__func__, "workspace missing or smaller than m355_dfine_select_workspace_bytes");
  if ((uintptr_t)d_work & 3u) return invalid(__func__, "workspace 4-byte aligned");
  return launched(__func__, launch_dfine_select_forward(d_class_logits, d_coord_logits, d_memory, B, S, C, D, K, (float*)d_work,
                                                        (long long*)d_indices, d_ref, d_boxes, d_logits, d_target, d_inverse,
                                                        (hipStream_t)stream));
}
int m355_dfine_select_backward(const float* d_grad_ref, const float* d_grad_boxes, const float* d_grad_logits, const float* d_grad_target,
                               const float* d_boxes, const int32_t* d_inverse, int32_t B, int32_t S, int32_t C, int32_t D, int32_t K,
                               float* d_grad_class, float* d_grad_coord, float* d_grad_memory, void* stream) {
  if (!d_inverse) return invalid(__func__, "null pointer");
  if (d_grad_boxes && d_grad_coord && !d_boxes) return invalid(__func__, "null pointer (boxes, which grad_boxes needs)");
  if (const char* why = dfine_select_check(B, S, C, K)) return invalid(__func__, why);
  if (d_grad_memory && D < 1) return invalid(__func__, "D >= 1");
  if (!d_grad_class && !d_grad_coord && !d_grad_memory) return M355_OK;   // nothing asked for
  return launched(__func__, launch_dfine_select_backward(d_grad_ref, d_grad_boxes, d_grad_logits, d_grad_target, d_boxes, d_inverse, B, S, C,
                                                         D, K, d_grad_class, d_grad_coord, d_grad_memory, (hipStream_t)stream));
}
size_t m355_dfine_loss_workspace_bytes(int32_t B, int32_t Q) { return dfine_loss_workspace_bytes(B, Q); }
int m355_dfine_loss_forward(const float* d_logits, const float* d_pred_boxes, int32_t B, int32_t Q, int32_t C,
                            const int64_t* d_match_q, const int64_t* d_match_t, int32_t M, const int32_t* d_offsets,
                            const int64_t* d_target_labels, const float* d_target_boxes, int32_t T, float num_boxes, float alpha,
                            float gamma, const float* d_pred_corners, const float* d_ref_points, const float* d_teacher_corners,
                            const float* d_teacher_logits, const float* d_project, int32_t num_bins_plus1, float reg_scale,
                            float temperature, void* d_work, int64_t work_bytes, float* d_out, void* stream) {
  DfineLossArgs a = dfine_loss_args(d_logits, d_pred_boxes, B, Q, C, d_match_q, d_match_t, M, d_offsets, d_target_labels,
                                    d_target_boxes, T, num_boxes, alpha, gamma, d_pred_corners, d_ref_points, d_teacher_corners,
                                    d_teacher_logits, d_project, num_bins_plus1, reg_scale, temperature);
  a.out = d_out;
  if (const char* why = dfine_loss_check(a)) return invalid(__func__, why);
  if (workspace_short(d_work, work_bytes, dfine_loss_workspace_bytes(B, Q)))
    return invalid(__func__, "workspace missing or smaller than m355_dfine_loss_workspace_bytes");
  a.partials = (float*)d_work;
  return launched(__func__, launch_dfine_loss_forward(a, (hipStream_t)stream));
}
int m355_dfine_loss_backward(const float* d_grad_terms, const float* d_logits, const float* d_pred_boxes, int32_t B, int32_t Q,
                             int32_t C, const int64_t* d_match_q, const int64_t* d_match_t, int32_t M, const int32_t* d_offsets,
                             const int64_t* d_target_labels, const float* d_target_boxes, int32_t T, float num_boxes, float alpha,
                             float gamma, const float* d_pred_corners, const float* d_ref_points, const float* d_teacher_corners,
                             const float* d_teacher_logits, const float* d_project, int32_t num_bins_plus1, float reg_scale,
                             float temperature, const float* d_saved, float* d_grad_logits, float* d_grad_pred_boxes,
                             float* d_grad_pred_corners, void* stream) {
  DfineLossArgs a = dfine_loss_args(d_logits, d_pred_boxes, B, Q, C, d_match_q, d_match_t, M, d_offsets, d_target_labels,
                                    d_target_boxes, T, num_boxes, alpha, gamma, d_pred_corners, d_ref_points, d_teacher_corners,
                                    d_teacher_logits, d_project, num_bins_plus1, reg_scale, temperature);
  a.out = const_cast<float*>(d_saved);   // read only here: out[5], out[6] of the forward
  if (const char* why = dfine_loss_check(a)) return invalid(__func__, why);
  if (!d_grad_terms) return invalid(__func__, "null pointer (grad_terms)");
  if (d_grad_pred_corners && !d_pred_corners) return invalid(__func__, "grad_pred_corners without the local group");
  a.grad_terms = d_grad_terms; a.grad_logits = d_grad_logits; a.grad_boxes = d_grad_pred_boxes; a.grad_corners = d_grad_pred_corners;
  if (!d_grad_logits && !d_grad_pred_boxes && !d_grad_pred_corners) return M355_OK;   // nothing asked for
  return launched(__func__, launch_dfine_loss_backward(a, (hipStream_t)stream));
}
int m355_dfine_attn_forward(const float* d_qkv, int32_t B, int32_t S, int32_t H, int32_t head_dim, float p, uint64_t seed,
                            int32_t site, float* d_out, float* d_lse, void* stream) {
  if (any_null({d_qkv, d_out})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_attn_check(B, S, H, head_dim, p, site)) return invalid(__func__, why);
  if (any_misaligned16({d_qkv, d_out})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_attn_forward(d_qkv, B, S, H, p, seed, site, d_out, d_lse, (hipStream_t)stream));
}
int m355_dfine_attn_backward(const float* d_grad_out, const float* d_qkv, const float* d_out, const float* d_lse, int32_t B, int32_t S,
                             int32_t H, int32_t head_dim, float p, uint64_t seed, int32_t site, float* d_grad_qkv, void* stream) {
  if (any_null({d_grad_out, d_qkv, d_out, d_lse, d_grad_qkv})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_attn_check(B, S, H, head_dim, p, site)) return invalid(__func__, why);
  if (any_misaligned16({d_grad_out, d_qkv, d_out, d_grad_qkv})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_attn_backward(d_grad_out, d_qkv, d_out, d_lse, B, S, H, p, seed, site, d_grad_qkv, (hipStream_t)stream));
}
size_t m355_dfine_addln_workspace_bytes(int64_t M, int32_t D) { return dfine_addln_workspace_bytes(M, D); }
int m355_dfine_addln_forward(const float* d_x, const float* d_y, const float* d_weight, const float* d_bias, int64_t M, int32_t D,
                             float eps, float p, uint64_t seed, int32_t site, float* d_out, float* d_mean, float* d_rstd, void* stream) {
  if (any_null({d_x, d_y, d_weight, d_bias, d_out, d_mean, d_rstd})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_addln_check(M, D, p, site)) return invalid(__func__, why);
  if (!(eps >= 0.f)) return invalid(__func__, "eps must be >= 0");
  if (any_misaligned16({d_x, d_y, d_weight, d_bias, d_out})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_addln_forward(d_x, d_y, d_weight, d_bias, M, D, eps, p, seed, site, d_out, d_mean, d_rstd,
                                                       (hipStream_t)stream));
}
int m355_dfine_addln_backward(const float* d_grad_out, const float* d_x, const float* d_y, const float* d_weight, const float* d_mean,
                              const float* d_rstd, int64_t M, int32_t D, float p, uint64_t seed, int32_t site, float* d_grad_x,
                              float* d_grad_y, float* d_grad_weight, float* d_grad_bias, void* d_work, int64_t work_bytes, void* stream) {
  if (any_null({d_grad_out, d_x, d_y, d_weight, d_mean, d_rstd})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_addln_check(M, D, p, site)) return invalid(__func__, why);
  if (workspace_short(d_work, work_bytes, dfine_addln_workspace_bytes(M, D)))
    return invalid(__func__, "workspace missing or smaller than m355_dfine_addln_workspace_bytes");
  if (any_misaligned16({d_grad_out, d_x, d_y, d_weight, d_grad_x, d_grad_y, d_work})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_addln_backward(d_grad_out, d_x, d_y, d_weight, d_mean, d_rstd, M, D, p, seed, site, d_grad_x,
                                                        d_grad_y, d_grad_weight, d_grad_bias, (float*)d_work, (hipStream_t)stream));
}
int m355_dfine_relu_dropout_forward(const float* d_h, int64_t n, float p, uint64_t seed, int32_t site, float* d_out, void* stream) {
  if (any_null({d_h, d_out})) return invalid(__func__, "null pointer");
  if (n < 1 || n > (int64_t)1 << 40) return invalid(__func__, "1 <= n <= 2^40");
  if (const char* why = dfine_dropout_check(p, site)) return invalid(__func__, why);
  if (any_misaligned16({d_h, d_out})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_relu_dropout(d_h, nullptr, d_out, n, p, seed, site, (hipStream_t)stream));
}
int m355_dfine_relu_dropout_backward(const float* d_grad_out, const float* d_out, int64_t n, float p, uint64_t seed, int32_t site,
                                     float* d_grad_h, void* stream) {
  if (any_null({d_grad_out, d_out, d_grad_h})) return invalid(__func__, "null pointer");
  if (n < 1 || n > (int64_t)1 << 40) return invalid(__func__, "1 <= n <= 2^40");
  if (const char* why = dfine_dropout_check(p, site)) return invalid(__func__, why);
  if (any_misaligned16({d_grad_out, d_out, d_grad_h})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_relu_dropout(d_grad_out, d_out, d_grad_h, n, p, seed, site, (hipStream_t)stream));
}
int m355_dfine_dropout_mask(int64_t n, float p, uint64_t seed, int32_t site, uint8_t* d_mask, void* stream) {
  if (!d_mask) return invalid(__func__, "null pointer");
  if (n < 1 || n > (int64_t)1 << 40) return invalid(__func__, "1 <= n <= 2^40");
  if (const char* why = dfine_dropout_check(p, site)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_keep_mask(d_mask, n, p, seed, site, (hipStream_t)stream));
}
// the decoder layer between its GEMMs (dfine_decoder.hip; the clamp form is an instance of dfine_encoder.hip's add-LayerNorm)
int m355_dfine_addln_clamp_forward(const float* d_x, const float* d_y, const float* d_weight, const float* d_bias, int64_t M, int32_t D,
                                   float eps, float lo, float hi, float* d_out, float* d_mean, float* d_rstd, void* stream) {
  if (any_null({d_x, d_y, d_weight, d_bias, d_out, d_mean, d_rstd})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_addln_check(M, D, 0.f, 0)) return invalid(__func__, why);
  if (!(eps >= 0.f)) return invalid(__func__, "eps must be >= 0");
  if (!(lo <= hi)) return invalid(__func__, "the clamp needs lo <= hi");
  if (any_misaligned16({d_x, d_y, d_weight, d_bias, d_out})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_addln_clamp_forward(d_x, d_y, d_weight, d_bias, M, D, eps, lo, hi, d_out, d_mean, d_rstd,
                                                             (hipStream_t)stream));
}
int m355_dfine_addln_clamp_backward(const float* d_grad_out, const float* d_x, const float* d_y, const float* d_weight,
                                    const float* d_mean, const float* d_rstd, int64_t M, int32_t D, float lo, float hi,
                                    float* d_grad_x, float* d_grad_y, float* d_grad_weight, float* d_grad_bias, void* d_work,
                                    int64_t work_bytes, void* stream) {
  if (any_null({d_grad_out, d_x, d_y, d_weight, d_mean, d_rstd})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_addln_check(M, D, 0.f, 0)) return invalid(__func__, why);
  if (!(lo <= hi)) return invalid(__func__, "the clamp needs lo <= hi");
  if (workspace_short(d_work, work_bytes, dfine_addln_workspace_bytes(M, D)))
    return invalid(__func__, "workspace missing or smaller than m355_dfine_addln_workspace_bytes");
  if (any_misaligned16({d_grad_out, d_x, d_y, d_weight, d_grad_x, d_grad_y, d_work})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_addln_clamp_backward(d_grad_out, d_x, d_y, d_weight, d_mean, d_rstd, M, D, lo, hi, d_grad_x,
                                                              d_grad_y, d_grad_weight, d_grad_bias, (float*)d_work, (hipStream_t)stream));
}
int m355_dfine_gate_ln_forward(const float* d_gate, const float* d_x1, const float* d_x2, const float* d_weight, const float* d_bias,
                               int64_t M, int32_t D, float eps, float* d_out, float* d_mean, float* d_rstd, void* stream) {
  if (any_null({d_gate, d_x1, d_x2, d_weight, d_bias, d_out, d_mean, d_rstd})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_addln_check(M, D, 0.f, 0)) return invalid(__func__, why);
  if (!(eps >= 0.f)) return invalid(__func__, "eps must be >= 0");
  if (any_misaligned16({d_gate, d_x1, d_x2, d_weight, d_bias, d_out})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_gate_ln_forward(d_gate, d_x1, d_x2, d_weight, d_bias, M, D, eps, d_out, d_mean, d_rstd,
                                                         (hipStream_t)stream));
}
int m355_dfine_gate_ln_backward(const float* d_grad_out, const float* d_gate, const float* d_x1, const float* d_x2,
                                const float* d_weight, const float* d_mean, const float* d_rstd, int64_t M, int32_t D,
                                float* d_grad_gate, float* d_grad_x1, float* d_grad_x2, float* d_grad_weight, float* d_grad_bias,
                                void* d_work, int64_t work_bytes, void* stream) {
  if (any_null({d_grad_out, d_gate, d_x1, d_x2, d_weight, d_mean, d_rstd})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_addln_check(M, D, 0.f, 0)) return invalid(__func__, why);
  const bool sums = d_grad_weight || d_grad_bias;   // the workspace holds their partial rows
  if (sums && workspace_short(d_work, work_bytes, dfine_addln_workspace_bytes(M, D)))
    return invalid(__func__, "workspace missing or smaller than m355_dfine_addln_workspace_bytes");
  if (any_misaligned16({d_grad_out, d_gate, d_x1, d_x2, d_weight, d_grad_gate, d_grad_x1, d_grad_x2, sums ? d_work : nullptr}))
    return invalid(__func__, kAlign16);
  if (!d_grad_gate && !d_grad_x1 && !d_grad_x2 && !sums) return M355_OK;   // nothing asked for
  return launched(__func__, launch_dfine_gate_ln_backward(d_grad_out, d_gate, d_x1, d_x2, d_weight, d_mean, d_rstd, M, D, d_grad_gate,
                                                          d_grad_x1, d_grad_x2, d_grad_weight, d_grad_bias, (float*)d_work,
                                                          (hipStream_t)stream));
}
int m355_dfine_lqe_forward(const float* d_pred_corners, int64_t M, int32_t num_bins_plus1, int32_t top_k, float* d_stat, uint8_t* d_index,
                           void* stream) {
  if (any_null({d_pred_corners, d_stat})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_lqe_check(M, num_bins_plus1, top_k)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_lqe_forward(d_pred_corners, M, num_bins_plus1, top_k, d_stat, d_index, (hipStream_t)stream));
}
int m355_dfine_lqe_backward(const float* d_grad_stat, const float* d_pred_corners, const uint8_t* d_index, int64_t M,
                            int32_t num_bins_plus1, int32_t top_k, float* d_grad_pred_corners, void* stream) {
  if (any_null({d_grad_stat, d_pred_corners, d_index, d_grad_pred_corners})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_lqe_check(M, num_bins_plus1, top_k)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_lqe_backward(d_grad_stat, d_pred_corners, d_index, M, num_bins_plus1, top_k,
                                                      d_grad_pred_corners, (hipStream_t)stream));
}
// the decoder's own loop around its layers (dfine_loop.hip)
int m355_dfine_query_pos_forward(const float* d_ref, const float* d_weight, const float* d_bias, int64_t N, int32_t H, float* d_out,
                                 void* stream) {
  if (any_null({d_ref, d_weight, d_bias, d_out})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_query_pos_check(N, H)) return invalid(__func__, why);
  if (any_misaligned16({d_ref, d_weight, d_bias, d_out})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_query_pos_forward(d_ref, d_weight, d_bias, (long)N, H, d_out, (hipStream_t)stream));
}
size_t m355_dfine_query_pos_workspace_bytes(int64_t N, int32_t H) {
  return dfine_query_pos_check(N, H) ? 0 : dfine_query_pos_workspace_bytes((long)N, H);
}
int m355_dfine_query_pos_backward(const float* d_grad_out, const float* d_out, const float* d_ref, const float* d_weight, int64_t N,
                                  int32_t H, float* d_grad_ref, float* d_grad_weight, float* d_grad_bias, void* d_work,
                                  int64_t work_bytes, void* stream) {
  if (any_null({d_grad_out, d_out, d_ref, d_weight})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_query_pos_check(N, H)) return invalid(__func__, why);
  const bool sums = d_grad_weight || d_grad_bias;   // the workspace holds their partial rows
  if (sums && workspace_short(d_work, work_bytes, dfine_query_pos_workspace_bytes((long)N, H)))
    return invalid(__func__, "workspace missing or smaller than m355_dfine_query_pos_workspace_bytes");
  if (any_misaligned16({d_grad_out, d_out, d_ref, d_weight, d_grad_ref, sums ? d_work : nullptr})) return invalid(__func__, kAlign16);
  if (!d_grad_ref && !sums) return M355_OK;   // nothing asked for
  return launched(__func__, launch_dfine_query_pos_backward(d_grad_out, d_out, d_ref, d_weight, (long)N, H, d_grad_ref, d_grad_weight,
                                                            d_grad_bias, (float*)d_work, (hipStream_t)stream));
}
int m355_dfine_refine_reference_forward(const float* d_delta, const float* d_ref, int64_t n, float eps, float* d_out, void* stream) {
  if (any_null({d_delta, d_ref, d_out})) return invalid(__func__, "null pointer");
  if (n < 1 || n > (int64_t)1 << 38) return invalid(__func__, "1 <= n <= 2^38");
  if (!(eps >= 0.f)) return invalid(__func__, "eps must be >= 0");
  return launched(__func__, launch_dfine_refine_reference_forward(d_delta, d_ref, (long)n, eps, d_out, (hipStream_t)stream));
}
int m355_dfine_refine_reference_backward(const float* d_grad_out, const float* d_out, int64_t n, float* d_grad_delta, void* stream) {
  if (any_null({d_grad_out, d_out, d_grad_delta})) return invalid(__func__, "null pointer");
  if (n < 1 || n > (int64_t)1 << 38) return invalid(__func__, "1 <= n <= 2^38");
  return launched(__func__, launch_dfine_refine_reference_backward(d_grad_out, d_out, (long)n, d_grad_delta, (hipStream_t)stream));
}
int m355_dfine_refine_boxes_forward(const float* d_delta, const float* d_prev, const float* d_project, const float* d_points, int64_t N,
                                    int32_t num_bins_plus1, float reg_scale, float* d_pred, float* d_boxes, void* stream) {
  if (any_null({d_delta, d_project, d_points, d_boxes})) return invalid(__func__, "null pointer");
  if ((d_prev == nullptr) != (d_pred == nullptr)) return invalid(__func__, "prev and pred come together or not at all");
  if (const char* why = dfine_refine_boxes_check(N, num_bins_plus1, reg_scale)) return invalid(__func__, why);
  if (any_misaligned16({d_delta, d_prev, d_points, d_pred})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_refine_boxes_forward(d_delta, d_prev, d_project, d_points, (long)N, num_bins_plus1, reg_scale,
                                                              d_pred, d_boxes, (hipStream_t)stream));
}
int m355_dfine_refine_boxes_backward(const float* d_grad_pred, const float* d_grad_boxes, const float* d_pred, const float* d_project,
                                     const float* d_points, int64_t N, int32_t num_bins_plus1, float reg_scale, float* d_grad_corners,
                                     float* d_grad_points, void* stream) {
  if (any_null({d_grad_boxes, d_pred, d_project, d_points, d_grad_corners})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_refine_boxes_check(N, num_bins_plus1, reg_scale)) return invalid(__func__, why);
  if (any_misaligned16({d_grad_pred, d_grad_boxes, d_pred, d_points, d_grad_corners})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_refine_boxes_backward(d_grad_pred, d_grad_boxes, d_pred, d_project, d_points, (long)N,
                                                               num_bins_plus1, reg_scale, d_grad_corners, d_grad_points,
                                                               (hipStream_t)stream));
}
// NCHW maps <-> token rows and the exact GELU (dfine_layout.hip)
int m355_dfine_maps_to_tokens(const float* const* h_maps, const int32_t* shapes_hw, int32_t num_levels, int32_t B, int32_t D,
                              const float* d_pos, const float* d_mask, float* d_tokens, float* d_extra, void* stream) {
  if (any_null({h_maps, shapes_hw, d_tokens})) return invalid(__func__, "null pointer");
  if (d_pos && d_mask) return invalid(__func__, "pos and mask exclude each other");
  if ((d_extra != nullptr) != (d_pos || d_mask)) return invalid(__func__, "extra comes with pos or mask and not without");
  DfineLayoutLevels lv;
  if (const char* why = dfine_layout_check(h_maps, shapes_hw, num_levels, B, D, lv)) return invalid(__func__, why);
  if (any_misaligned16({d_pos, d_tokens, d_extra}) || ((uintptr_t)d_mask & 3u)) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_maps_to_tokens(h_maps, lv, B, D, d_pos, d_mask, d_tokens, d_extra, (hipStream_t)stream));
}
int m355_dfine_tokens_to_maps(const float* d_tokens, const float* d_extra, const float* d_mask, const int32_t* shapes_hw,
                              int32_t num_levels, int32_t B, int32_t D, float* const* h_maps, void* stream) {
  if (any_null({h_maps, shapes_hw}) || (!d_tokens && !d_extra)) return invalid(__func__, "null pointer");
  if (d_mask && !d_extra) return invalid(__func__, "mask without extra");
  DfineLayoutLevels lv;
  if (const char* why = dfine_layout_check(h_maps, shapes_hw, num_levels, B, D, lv)) return invalid(__func__, why);
  if (any_misaligned16({d_tokens, d_extra}) || ((uintptr_t)d_mask & 3u)) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_tokens_to_maps(d_tokens, d_extra, d_mask, lv, B, D, h_maps, (hipStream_t)stream));
}
int m355_dfine_gelu_forward(const float* d_h, int64_t n, float* d_out, void* stream) {
  if (any_null({d_h, d_out})) return invalid(__func__, "null pointer");
  if (n < 1 || n > (int64_t)1 << 40) return invalid(__func__, "1 <= n <= 2^40");
  if (any_misaligned16({d_h, d_out})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_gelu(d_h, nullptr, d_out, (long)n, (hipStream_t)stream));
}
int m355_dfine_gelu_backward(const float* d_grad_out, const float* d_h, int64_t n, float* d_grad_h, void* stream) {
  if (any_null({d_grad_out, d_h, d_grad_h})) return invalid(__func__, "null pointer");
  if (n < 1 || n > (int64_t)1 << 40) return invalid(__func__, "1 <= n <= 2^40");
  if (any_misaligned16({d_grad_out, d_h, d_grad_h})) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_gelu(d_grad_out, d_h, d_grad_h, (long)n, (hipStream_t)stream));
}
// the GRU recurrence (dfine_gru.hip)
size_t m355_dfine_gru_workspace_bytes(int32_t B, int64_t S, int32_t H, int32_t D) { return dfine_gru_workspace_bytes(B, S, H, D); }
int m355_dfine_gru_forward(const float* d_gi, const float* d_w_hh, const float* d_b_hh, const float* d_h0, int32_t B, int64_t S,
                           int32_t H, int32_t D, float* d_out, float* d_h_n, void* d_work, int64_t work_bytes, int32_t keep,
                           int32_t* d_status, void* stream) {
  if (any_null({d_gi, d_w_hh, d_b_hh, d_out, d_h_n, d_work, d_status})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_gru_check(B, S, H, D)) return invalid(__func__, why);
  if (workspace_short(d_work, work_bytes, dfine_gru_workspace_bytes(B, keep ? S : 0, H, D)))
    return invalid(__func__, "workspace smaller than m355_dfine_gru_workspace_bytes");
  if (any_misaligned16({d_gi, d_w_hh, d_b_hh, d_h0, d_out, d_h_n, d_work}) || ((uintptr_t)d_status & 3u)) return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_gru_forward(d_gi, d_w_hh, d_b_hh, d_h0, B, (int)S, D, d_out, d_h_n, d_work, keep != 0, d_status,
                                                     (hipStream_t)stream));
}
int m355_dfine_gru_backward(const float* d_grad_out, const float* d_grad_h_n, const float* d_w_hh, const float* d_h0, const float* d_out,
                            int32_t B, int64_t S, int32_t H, int32_t D, float* d_grad_gi, float* d_grad_an, float* d_grad_h0,
                            void* d_work, int64_t work_bytes, int32_t* d_status, void* stream) {
  if (any_null({d_grad_out, d_w_hh, d_out, d_grad_gi, d_grad_an, d_grad_h0, d_work, d_status})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_gru_check(B, S, H, D)) return invalid(__func__, why);
  if (workspace_short(d_work, work_bytes, dfine_gru_workspace_bytes(B, S, H, D)))
    return invalid(__func__, "workspace smaller than m355_dfine_gru_workspace_bytes");
  if (any_misaligned16({d_grad_out, d_grad_h_n, d_w_hh, d_h0, d_out, d_grad_gi, d_grad_an, d_grad_h0, d_work}) || ((uintptr_t)d_status & 3u))
    return invalid(__func__, kAlign16);
  return launched(__func__, launch_dfine_gru_backward(d_grad_out, d_grad_h_n, d_w_hh, d_h0, d_out, B, (int)S, D, d_grad_gi, d_grad_an,
                                                      d_grad_h0, d_work, d_status, (hipStream_t)stream));
}
// the temporal head (dfine_temporal.hip)
int m355_dfine_temporal_fuse_forward(const float* d_fused, const float* d_scores, const float* d_context, int32_t T, int32_t Q,
                                     int32_t D, float* d_out, float* d_stats, void* stream) {
  if (any_null({d_fused, d_scores, d_out})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_tfuse_check(T, Q, D)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_tfuse_forward(d_fused, d_scores, d_context, T, Q, D, d_out, d_stats, (hipStream_t)stream));
}
int m355_dfine_temporal_fuse_backward(const float* d_grad_out, const float* d_fused, const float* d_scores, const float* d_stats,
                                      int32_t T, int32_t Q, int32_t D, float* d_grad_fused, float* d_grad_scores, void* stream) {
  if (any_null({d_grad_out, d_scores, d_stats})) return invalid(__func__, "null pointer");
  if (d_grad_scores && !d_fused) return invalid(__func__, "null pointer (fused, which grad_scores needs)");
  if (const char* why = dfine_tfuse_check(T, Q, D)) return invalid(__func__, why);
  if (!d_grad_fused && !d_grad_scores) return M355_OK;   // nothing asked for
  return launched(__func__, launch_dfine_tfuse_backward(d_grad_out, d_fused, d_scores, d_stats, T, Q, D, d_grad_fused, d_grad_scores,
                                                        (hipStream_t)stream));
}
int m355_dfine_guard_logits_forward(const float* d_cls, const float* d_anomaly, int64_t rows, int32_t C1, float bound, float* d_out,
                                    void* stream) {
  if (any_null({d_cls, d_out})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_guard_logits_check(rows, C1, d_anomaly != nullptr, bound)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_guard_logits(d_cls, d_anomaly, (long)rows, C1, bound, d_out, (hipStream_t)stream));
}
int m355_dfine_guard_logits_backward(const float* d_grad_out, const float* d_cls, const float* d_anomaly, int64_t rows, int32_t C1,
                                     float bound, float* d_grad_cls, float* d_grad_anomaly, void* stream) {
  if (any_null({d_grad_out, d_cls})) return invalid(__func__, "null pointer");
  if (d_grad_anomaly && !d_anomaly) return invalid(__func__, "grad_anomaly without anomaly");
  if (const char* why = dfine_guard_logits_check(rows, C1, d_anomaly != nullptr, bound)) return invalid(__func__, why);
  if (!d_grad_cls && !d_grad_anomaly) return M355_OK;   // nothing asked for
  return launched(__func__, launch_dfine_guard_logits_backward(d_grad_out, d_cls, d_anomaly, (long)rows, C1, bound, d_grad_cls,
                                                               d_grad_anomaly, (hipStream_t)stream));
}
int m355_dfine_noobject_loss_forward(const float* d_logits, int32_t T, int32_t Q, int32_t C1, int32_t class_index, float* d_out,
                                     void* stream) {
  if (any_null({d_logits, d_out})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_noobject_check(T, Q, C1, class_index)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_noobject_forward(d_logits, T, Q, C1, class_index, d_out, (hipStream_t)stream));
}
int m355_dfine_noobject_loss_backward(const float* d_grad_out, const float* d_logits, int32_t T, int32_t Q, int32_t C1,
                                      int32_t class_index, float* d_grad_logits, void* stream) {
  if (any_null({d_grad_out, d_logits, d_grad_logits})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_noobject_check(T, Q, C1, class_index)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_noobject_backward(d_grad_out, d_logits, T, Q, C1, class_index, d_grad_logits, (hipStream_t)stream));
}
size_t m355_dfine_consistency_workspace_bytes(int32_t T, int64_t N) {
  return dfine_consistency_check(T, N) ? 0 : dfine_consistency_workspace_bytes(T, (long)N);
}
int m355_dfine_consistency_loss_forward(const float* d_a, int32_t T, int64_t N, void* d_work, int64_t work_bytes, float* d_out,
                                        void* stream) {
  if (any_null({d_a, d_out})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_consistency_check(T, N)) return invalid(__func__, why);
  if (workspace_short(d_work, work_bytes, dfine_consistency_workspace_bytes(T, (long)N)))
    return invalid(__func__, "workspace missing or smaller than m355_dfine_consistency_workspace_bytes");
  if ((uintptr_t)d_work & 3u) return invalid(__func__, "workspace 4-byte aligned");
  return launched(__func__, launch_dfine_consistency_forward(d_a, T, (long)N, (float*)d_work, d_out, (hipStream_t)stream));
}
int m355_dfine_consistency_loss_backward(const float* d_grad_out, const float* d_a, int32_t T, int64_t N, float* d_grad_a,
                                         void* stream) {
  if (any_null({d_grad_out, d_a, d_grad_a})) return invalid(__func__, "null pointer");
  if (const char* why = dfine_consistency_check(T, N)) return invalid(__func__, why);
  return launched(__func__, launch_dfine_consistency_backward(d_grad_out, d_a, T, (long)N, d_grad_a, (hipStream_t)stream));
}
// the end of the trainers' step (dfine_optim.hip)
int m355_dfine_grad_sumsq_launch(const m355_dfine_optim_row* h_table, const m355_dfine_optim_row* d_table, int32_t count,
                                 float* d_partials, int64_t partials_len, void* stream) {
  int chunks = 0;
  if (const char* why = dfine_optim_check(h_table, d_table, count, false, &chunks)) return invalid(__func__, why);
  if (!d_partials || partials_len < chunks) return invalid(__func__, "partials missing or shorter than the number of chunks");
  if ((uintptr_t)d_partials & 3u) return invalid(__func__, "pointers must be 4-byte aligned");
  return launched(__func__, launch_dfine_grad_sumsq(d_table, count, chunks, d_partials, (hipStream_t)stream));
}
int m355_dfine_clip_scale_launch(const m355_dfine_optim_row* h_table, const m355_dfine_optim_row* d_table, int32_t count,
                                 const float* d_partials, int64_t partials_len, float max_norm, float* d_norm, void* stream) {
  int chunks = 0;
  if (const char* why = dfine_optim_check(h_table, d_table, count, false, &chunks)) return invalid(__func__, why);
  if (!d_partials || partials_len < chunks) return invalid(__func__, "partials missing or shorter than the number of chunks");
  if (!d_norm) return invalid(__func__, "null pointer (norm)");
  if (((uintptr_t)d_partials & 3u) || ((uintptr_t)d_norm & 7u)) return invalid(__func__, "partials must be 4-byte aligned, norm 8-byte aligned");
  if (int rc = launch_dfine_grad_norm(d_partials, chunks, max_norm, d_norm, (hipStream_t)stream)) return launched(__func__, rc);
  return launched(__func__, launch_dfine_clip_scale(d_table, count, chunks, d_norm, (hipStream_t)stream));
}
int m355_dfine_adam_launch(const m355_dfine_optim_row* h_table, const m355_dfine_optim_row* d_table, int32_t count, int32_t mode,
                           const float* d_partials, int64_t partials_len, float max_norm, float* d_norm, void* stream) {
  int chunks = 0;
  if (const char* why = dfine_optim_check(h_table, d_table, count, true, &chunks)) return invalid(__func__, why);
  if (mode != M355_DFINE_OPTIM_ADAM && mode != M355_DFINE_OPTIM_ADAMW) return invalid(__func__, "mode is neither ADAM (0) nor ADAMW (1)");
  if ((d_partials == nullptr) != (d_norm == nullptr)) return invalid(__func__, "partials and norm come together or not at all");
  if (d_partials && partials_len < chunks) return invalid(__func__, "partials shorter than the number of chunks");
  if (((uintptr_t)d_partials & 3u) || ((uintptr_t)d_norm & 7u)) return invalid(__func__, "partials must be 4-byte aligned, norm 8-byte aligned");
  if (d_partials)
    if (int rc = launch_dfine_grad_norm(d_partials, chunks, max_norm, d_norm, (hipStream_t)stream)) return launched(__func__, rc);
  return launched(__func__, launch_dfine_adam(d_table, count, chunks, mode == M355_DFINE_OPTIM_ADAMW, d_norm, (hipStream_t)stream));
}
