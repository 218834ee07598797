// libmi355yolo.so per-op C entries (include/mi355yolo.h) that need no m355_engine: the unit-parity entries of single launches
// (host weights packed by weight_pack.hip exactly as m355_set_conv_weights packs them, one launch, stream synchronised), and
// the training step's launch wrappers (conv, weight gradient, bn, optimizers, losses, augment) and workspace queries.  The
// D-FINE entries are in dfine_entries.hip.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mi355yolo.h"
#include "common.h"
#include "launch_util.h"
#include "switches.h"
#include "weight_pack.h"

using namespace m355;

namespace {

struct DevBuf {   // device allocations of one entry call, freed on scope exit; nullptr = the allocation or its copy failed
  std::vector<void*> p;
  ~DevBuf() { for (void* q : p) (void)hipFree(q); }
  void* alloc(size_t bytes) {   // uninitialised
    void* d = nullptr;
    if (hipMalloc(&d, bytes + 16) != hipSuccess) return nullptr;
    p.push_back(d);
    return d;
  }
  void* zeroed(size_t bytes) {
    void* d = alloc(bytes);
    return d && hipMemset(d, 0, bytes + 16) == hipSuccess ? d : nullptr;
  }
  template <class T>
  T* put(const std::vector<T>& h) {   // a device copy of h
    void* d = alloc(h.size() * sizeof(T));
    return d && hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? (T*)d : nullptr;
  }
};

int alloc_failed() { return set_err(M355_ERR_HIP, "allocation failed"); }

// The result of an entry's launch: rc = the launcher's return (0 = launched, any other value M355_ERR_HIP), se = the status of
// the stream synchronisation after it.
int launch_status(int rc, hipError_t se, const char* what) {
  if (rc != 0) return set_err(M355_ERR_HIP, std::string(what) + " launch failed: " + std::to_string(rc));
  if (se != hipSuccess) return set_err(M355_ERR_HIP, std::string(what) + " kernel: " + hipGetErrorString(se));
  return M355_OK;
}

// launch_status after synchronising s, for the entries whose launcher refuses a shape with -1 (M355_ERR_INVALID)
int finish_entry(int rc, hipStream_t s, const char* what) {
  const hipError_t se = hipStreamSynchronize(s);
  if (rc != 0) return set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, std::string(what) + ": launch refused / failed (" + std::to_string(rc) + ")");
  return launch_status(0, se, what);
}

// Argument checks of the forward glue entries (stem, SPPF pooling, upsample, ADown front, decode).  Each entry runs them before any HIP
// call; a failure is M355_ERR_INVALID with a message that names the entry.
int glue_invalid(const char* entry, const std::string& why) { return set_err(M355_ERR_INVALID, std::string(entry) + ": " + why); }

// One fp16 NHWC channel slice handed to a kernel of 16-byte accesses: `pixels` pixels per image, channels [0, C) of rows of ld elements,
// images bstride elements apart.  Empty = fine, else what is wrong with operand `name`.
std::string slice_fault(const char* name, const void* p, int64_t bstride, int32_t ld, long pixels, int C) {
  const std::string n(name);
  if (!p) return n + " is a null pointer";
  if ((uintptr_t)p & 15) return n + " must be 16-byte aligned";
  if (ld < C) return "the leading dimension of " + n + " is smaller than its channel count";
  if (ld % 8 || bstride % 8) return "the leading dimension and the batch stride of " + n + " must be multiples of 8";
  if (bstride < (pixels - 1) * ld + C) return "the batch stride of " + n + " is smaller than the extent of one image's slice";
  return std::string();
}

int sppf_entry(const char* entry, const void* x, int64_t x_bstride, int32_t ldx, void* y, int64_t y_bstride, int32_t ldy, int B, int H, int W,
               int C, void* stream) {
  if (B < 1 || H < 1 || W < 1) return glue_invalid(entry, "B, H, W must be >= 1");
  if (C < 8 || C % 8) return glue_invalid(entry, "C must be a positive multiple of 8");
  // three copies of the plane of one 8-channel group (launch_sppf_pool): what sppf_pool_form refuses, as a message
  if ((long)H * W * 3 * 16 > 160 * 1024) return glue_invalid(entry, "the plane needs more than 160 KB of LDS");
  std::string f = slice_fault("x", x, x_bstride, ldx, (long)H * W, C);
  if (f.empty()) f = slice_fault("y", y, y_bstride, ldy, (long)H * W, 3 * C);
  if (!f.empty()) return glue_invalid(entry, f);
  const int rc = launch_sppf_pool((const half_t*)x, x_bstride, ldx, (half_t*)y, y_bstride, ldy, B, H, W, C, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, std::string(entry) + ": launch failed: " + std::to_string(rc));
}

int upsample_entry(const char* entry, const void* x, int64_t x_bstride, int32_t ldx, void* y, int64_t y_bstride, int32_t ldy, int B, int H,
                   int W, int C, void* stream) {
  if (B < 1 || H < 1 || W < 1 || H > (1 << 14) || W > (1 << 14)) return glue_invalid(entry, "B, H, W must be >= 1 (H, W at most 16384)");
  if (C < 8 || C % 8) return glue_invalid(entry, "C must be a positive multiple of 8");
  std::string f = slice_fault("x", x, x_bstride, ldx, (long)H * W, C);
  if (f.empty()) f = slice_fault("y", y, y_bstride, ldy, (long)4 * H * W, C);
  if (!f.empty()) return glue_invalid(entry, f);
  const int rc = launch_upsample2x((const half_t*)x, x_bstride, ldx, (half_t*)y, y_bstride, ldy, B, H, W, C, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, std::string(entry) + ": launch failed: " + std::to_string(rc));
}

int decode_entry(const char* entry, const float* raw, int B, int in_h, int in_w, int nc, int nm, float* preds, void* stream) {
  if (!raw || !preds) return glue_invalid(entry, "null pointer");
  if (B < 1) return glue_invalid(entry, "B must be >= 1");
  if (in_h < 32 || in_w < 32 || in_h % 32 || in_w % 32 || in_h > 32768 || in_w > 32768)
    return glue_invalid(entry, "in_h and in_w must be positive multiples of 32 (at most 32768)");
  if (nc < 1 || nm < 0) return glue_invalid(entry, "nc must be >= 1 and nm >= 0");
  // the kernel stages 64 anchors' raw and decoded rows in LDS (launch_head_decode)
  if (((long)64 + nc + nm + 4 + nc + nm) * 64 * (long)sizeof(float) > 160 * 1024) return glue_invalid(entry, "nc + nm needs more than 160 KB of LDS");
  if (((uintptr_t)raw | (uintptr_t)preds) & 15) return glue_invalid(entry, "raw and preds must be 16-byte aligned");
  const long anchors = (long)(in_h / 8) * (in_w / 8) + (long)(in_h / 16) * (in_w / 16) + (long)(in_h / 32) * (in_w / 32);
  if (B * anchors > (1L << 36)) return glue_invalid(entry, "too many anchors");
  const int rc = launch_head_decode(raw, B, in_h, in_w, nc, nm, preds, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, std::string(entry) + ": launch failed: " + std::to_string(rc));
}

// Diagnostics of the row-slab entries (conv_op_common, m355_bneck_pair_fwd), read by tools/stamps_halo.py and tools/bneck_bench.py:
//   M355_STAMPS=<file>   the kernel's stamps go to a zeroed buffer of `words` uint64, written to <file> by dump();
//   M355_BNECK_REPS=<n>  after a launch that succeeded, n more back to back; their mean time goes to stderr.
struct SlabDiag {
  const char* path = live_stamps_path();
  size_t words = 0;
  StampSink sink;                         // over a buffer of the entry's DevBuf; sink.d stays nullptr when M355_STAMPS is unset
  bool alloc(DevBuf& d, size_t n) {       // false: the stamp buffer could not be allocated
    words = n;
    if (path) sink.d = (unsigned long long*)d.zeroed(n * 8);
    return !path || sink.d;
  }
  template <class Launch>
  int reps(int rc, hipStream_t s, const char* what, Launch launch) const {
    const int n = live_bneck_reps();
    hipEvent_t e0, e1;
    if (rc == 0 && n > 0 && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
      (void)hipEventRecord(e0, s);
      for (int i = 0; i < n && rc == 0; ++i) rc = launch();
      (void)hipEventRecord(e1, s);
      (void)hipEventSynchronize(e1);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, e0, e1);
      fprintf(stderr, "%s: %.2f us per launch (%d launches)\n", what, ms * 1e3f / n, n);
      (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    return rc;
  }
  void dump(bool ok) const {   // after the stream synchronisation
    if (ok) sink.write(path, words * 8);
  }
};

int conv_op_common(const void* d_x, int B, int H, int W, int cin, const float* h_w, const float* h_bias,
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
  if (transposed) pack_convt2x2_rows(h_w, cin, cout, Kpad, rows);
  else pack_conv_rows(h_w, cout, cin, k, Kpad, 0, rows);
  for (int i = 0; i < cout; ++i) bias[i] = h_bias[i];
  const FragList fl = transposed ? FragList() : frag_list(k, cin, cout);
  DevBuf d;
  SlabDiag diag;
  ConvArgs a{};
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * cin; a.ldx = cin; a.Hi = H; a.Wi = W; a.Cin = cin;
  a.w = d.put(rows); a.Kpad = Kpad; a.bias = d.put(bias); a.zero = (const half_t*)d.zeroed(256); a.act = act; a.out_f32 = out_f32;
  a.w_rows = cout_pad; a.wf = fl.empty() ? nullptr : d.put(frag_pack(rows.data(), Kpad, fl, false));
  if (!a.w || !a.bias || !a.zero || (!fl.empty() && !a.wf) || !diag.alloc(d, (size_t)1 << 20)) return alloc_failed();
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
  a.stamps = diag.sink.d;
  int rc = 0;
  if (force_tile >= 0 && (force_tile & 0xff) == TILE_PLANES) {   // row-slab kernel (conv3x3_planes.hip), single-conv mode
    PlanesArgs pa{};
    pa.x = a.x; pa.x_bstride = a.x_bstride; pa.ldx = a.ldx; pa.H = H; pa.W = W; pa.B = B; pa.Cin = cin; pa.Cout = cout; pa.stride = stride;
    pa.wfb = d.put(planes_frag_pack_padded(rows.data(), cout, Kpad, cin)); pa.cblocks_b = planes_cblocks(cout); pa.bb = a.bias;
    pa.y = (half_t*)d_y; pa.y_bstride = a.y_bstride; pa.ldy = a.ldy;
    pa.res = a.res; pa.r_bstride = a.r_bstride; pa.ldr = a.ldr; pa.act = act; pa.stamps = a.stamps;
    if (!pa.wfb) return alloc_failed();
    char what[80];
    snprintf(what, sizeof(what), "conv3x3_planes B=%d %dx%d %d->%d", B, H, W, cin, cout);
    rc = diag.reps(conv3x3_planes_ok(pa) ? launch_conv3x3_planes(pa, s) : -1, s, what, [&] { return launch_conv3x3_planes(pa, s); });
  } else
  for (int rep = 0; rep < (a.dbg ? 5 : 1); ++rep)
    rc = (force_tile >= 0 && (force_tile & 0xff) == TILE_W1) ? launch_conv1x1_wreg(a, s)
         : (force_tile >= 0 && (force_tile & 0xff) == TILE_C32)
             ? launch_conv3x3_c32(a, s)
             : ((force_tile >= 0 && (force_tile & 0xff) >= TILE_HALO) ? launch_conv3x3_halo(a, (force_tile & 0xff) - TILE_HALO, s)
                                                                       : launch_conv_igemm(a, force_tile, s));
  const hipError_t se = hipStreamSynchronize(s);
  diag.dump(se == hipSuccess);
  if (rc == -1) return set_err(M355_ERR_INVALID, "conv launch failed: -1");   // the launcher refused the shape, as finish_entry reports it
  return launch_status(rc, se, "conv");
}

}  // namespace

extern "C" {

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
  const FragList fl = frag_list(3, 32, 32);
  DevBuf d;
  const float* db = d.put(bias);
  C2fC32Args a{};
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * 64; a.ldx = 64; a.H = H; a.W = W; a.B = B;
  a.wa = d.put(ra); a.wb = d.put(rb); a.wc = d.put(rc_); a.kpad_a = kp3; a.kpad_b = kp3; a.kpad_c = kp1;
  a.waf = d.put(frag_pack(ra.data(), kp3, fl, false)); a.wbf = d.put(frag_pack(rb.data(), kp3, fl, true));   // wb: operand row order
  if (!db || !a.wa || !a.wb || !a.wc || !a.waf || !a.wbf) return alloc_failed();
  a.ba = db; a.bb = db + 32; a.bc = db + 64;
  a.y = (half_t*)d_y; a.y_bstride = (long)H * W * 64; a.ldy = 64; a.shortcut = shortcut;
  const int rc = launch_c2f_c32(a, s);
  return launch_status(rc, hipStreamSynchronize(s), "c2f_c32");
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
  std::vector<float> bias(2 * rows, 0.f);
  for (int i = 0; i < C; ++i) { bias[i] = h_ba[i]; bias[rows + i] = h_bb[i]; }
  DevBuf d;
  SlabDiag diag;
  const float* db = d.put(bias);
  PlanesArgs a{};
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * ldx; a.ldx = ldx; a.H = H; a.W = W; a.B = B; a.Cin = C; a.Cout = C;
  a.wfa = d.put(planes_frag_pack(ra.data(), kp, C, cbl)); a.wfb = d.put(planes_frag_pack(rb.data(), kp, C, cbl)); a.cblocks_a = a.cblocks_b = cbl;
  if (!db || !a.wfa || !a.wfb || !diag.alloc(d, (size_t)256 * 4 * 8 * 2)) return alloc_failed();
  a.ba = db; a.bb = db + rows;
  a.y = (half_t*)d_y; a.y_bstride = (long)H * W * ldy; a.ldy = ldy; a.act = 1; a.stride = 1;
  if (shortcut) { a.res = a.x; a.r_bstride = a.x_bstride; a.ldr = ldx; }
  a.stamps = diag.sink.d;
  const bool ok = bneck_pair_ok(a);
  char what[64];
  snprintf(what, sizeof(what), "bneck_pair B=%d %dx%d C=%d", B, H, W, C);
  const int rc = diag.reps(ok ? launch_bneck_pair(a, s) : -1, s, what, [&] { return launch_bneck_pair(a, s); });
  const hipError_t se = hipStreamSynchronize(s);
  diag.dump(se == hipSuccess && rc == 0);
  if (!ok) return set_err(M355_ERR_INVALID, "bneck_pair: shape not eligible (C in {64, 128}, slab geometry must fit LDS)");
  return launch_status(rc, se, "bneck_pair");
}

}  // extern "C"

// n 3x3 convs side by side as one block-diagonal launch of the row-slab kernel (the second stage of a head level)
namespace {
bool diag_shapes_ok(int n, const int* cin, const int* cout) {
  if (n < 1 || n > 4 || !cin || !cout) return false;
  for (int i = 0; i < n; ++i)
    if (cin[i] < 32 || cin[i] % 32 || cout[i] < 16 || cout[i] % 16 || (i + 1 < n && cout[i] % 64)) return false;
  return true;
}
// fp16 rows of every conv, packed as m355_set_conv_weights packs them, and their fragment list
std::vector<half_t> diag_pack(int n, const int* cin, const int* cout, const float* const* h_w) {
  std::vector<std::vector<half_t>> rows(n);
  const half_t* rp[4];
  int kp[4];
  for (int i = 0; i < n; ++i) {
    kp[i] = conv_kpad(cin[i], 3);
    rows[i].assign((size_t)cout[i] * kp[i], (half_t)0.f);
    pack_conv_rows(h_w[i], cout[i], cin[i], 3, kp[i], 0, rows[i]);
    rp[i] = rows[i].data();
  }
  return planes_frag_pack_diag(rp, cout, kp, cin, n);
}
}  // namespace

extern "C" {

long m355_planes_diag_pack(int n, const int* cin, const int* cout, const float* const* h_w, void* h_out_f16, long out_bytes) {
  if (!diag_shapes_ok(n, cin, cout) || !h_w) return set_err(M355_ERR_INVALID, "planes_diag_pack: bad shapes");
  long need = 0;
  for (int i = 0; i < n; ++i) need += (long)planes_cblocks(cout[i]) * (cin[i] / 32) * 18 * 1024;
  if (!h_out_f16) return need;
  if (out_bytes < need) return set_err(M355_ERR_INVALID, "planes_diag_pack: output buffer too small");
  for (int i = 0; i < n; ++i)
    if (!h_w[i]) return set_err(M355_ERR_INVALID, "null pointer");
  const std::vector<half_t> f = diag_pack(n, cin, cout, h_w);
  memcpy(h_out_f16, f.data(), f.size() * sizeof(half_t));
  return need;
}

int m355_conv3x3_blockdiag_fwd(const void* d_x, int B, int H, int W, int ldx, int n, const int* cin, const int* cout,
                               const float* const* h_w, const float* const* h_b, void* d_y, int ldy, int walk, void* stream) {
  if (!d_x || !d_y || !h_w || !h_b) return set_err(M355_ERR_INVALID, "null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || walk < 0 || walk > 2 || !diag_shapes_ok(n, cin, cout)) return set_err(M355_ERR_INVALID, "bad shape");
  for (int i = 0; i < n; ++i)
    if (!h_w[i] || !h_b[i]) return set_err(M355_ERR_INVALID, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  PlanesArgs a{};
  a.diag_n = n; a.diag_walk = walk;
  std::vector<float> bias;
  for (int i = 0; i < n; ++i) {
    a.diag_cin[i] = cin[i]; a.diag_cout[i] = cout[i];
    a.Cin += cin[i]; a.Cout += cout[i];
    bias.insert(bias.end(), h_b[i], h_b[i] + cout[i]);
    a.cblocks_b += planes_cblocks(cout[i]);
  }
  bias.resize((bias.size() + 63) / 64 * 64, 0.f);
  if (ldx < a.Cin || ldy < a.Cout) return set_err(M355_ERR_INVALID, "bad shape");
  DevBuf d;
  SlabDiag diag;
  a.x = (const half_t*)d_x; a.x_bstride = (long)H * W * ldx; a.ldx = ldx; a.H = H; a.W = W; a.B = B; a.stride = 1; a.act = 1;
  a.wfb = d.put(diag_pack(n, cin, cout, h_w)); a.bb = d.put(bias);
  a.y = (half_t*)d_y; a.y_bstride = (long)H * W * ldy; a.ldy = ldy;
  if (!a.wfb || !a.bb || !diag.alloc(d, (size_t)256 * 4 * 8 * 2)) return alloc_failed();
  a.stamps = diag.sink.d;
  const bool ok = conv3x3_blockdiag_ok(a);
  char what[80];
  snprintf(what, sizeof(what), "conv3x3_blockdiag B=%d %dx%d %d->%d", B, H, W, a.Cin, a.Cout);
  const int rc = diag.reps(ok ? launch_conv3x3_blockdiag(a, s) : -1, s, what, [&] { return launch_conv3x3_blockdiag(a, s); });
  const hipError_t se = hipStreamSynchronize(s);
  diag.dump(se == hipSuccess && rc == 0);
  if (!ok) return set_err(M355_ERR_INVALID, "conv3x3_blockdiag: shape not eligible (at most eight 64-channel tiles, row slabs must fit LDS)");
  return launch_status(rc, se, "conv3x3_blockdiag");
}

// ---- per-op parity entries of the round-3 fused launches (each: host weights packed as m355_set_conv_weights packs them, through
// the same fragment lists, one launch, stream synchronised) ---------------------------------------------------------------------

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
  a.bias = d.put(b3); a.bias2 = d.put(b1); a.cout2 = 128; a.zero = (const half_t*)d.zeroed(256);
  a.ksize = 3; a.stride = 2; a.pad = 1; a.Ho = H / 2; a.Wo = W / 2; a.Cout = 128; a.act = 1; a.w_rows = conv_cout_pad(128);
  a.y = d_y; a.y_bstride = (long)a.Ho * a.Wo * 128; a.ldy = 128; a.M = B * a.Ho * a.Wo;
  if (!a.w || !a.wf || !a.w2 || !a.wf2 || !a.bias || !a.bias2 || !a.zero) return alloc_failed();
  return finish_entry(conv_s2c64_cv1_ok(a) ? launch_conv_s2c64_cv1(a, s) : -1, s, "conv3x3_s2c64 + 1x1");
}

int m355_stem_s2c32_cv1_fwd(const void* d_in_u8, int B, int H, int W, const float* h_w0, const float* h_b0, const float* h_w1,
                            const float* h_b1, const float* h_w2, const float* h_b2, void* d_y, int two_team, void* stream) {
  if (!d_in_u8 || !d_y || !h_w0 || !h_b0 || !h_w1 || !h_b1 || !h_w2 || !h_b2 || B < 1 || H < 4 || W < 4) return set_err(M355_ERR_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const std::vector<half_t> sw = pack_stem3x3(h_w0, 32);
  const int kp = conv_kpad(32, 3);
  std::vector<half_t> rows((size_t)conv_cout_pad(64) * kp, (half_t)0.f);
  pack_conv_rows(h_w1, 64, 32, 3, kp, 0, rows);
  const std::vector<half_t> r2 = to_half_vec(h_w2, (size_t)64 * 64);
  DevBuf d;
  StemArgs st{};
  st.x = (const uint8_t*)d_in_u8; st.B = B; st.H = H; st.W = W; st.w16 = d.put(sw);
  st.bias = d.put(std::vector<float>(h_b0, h_b0 + 32));
  st.y = (half_t*)d.zeroed((size_t)B * (H / 2) * (W / 2) * 32 * 2); st.y_bstride = (long)(H / 2) * (W / 2) * 32; st.ldy = 32; st.Cout = 32;
  ConvArgs a{};
  a.x = st.y; a.x_bstride = st.y_bstride; a.ldx = 32; a.Hi = H / 2; a.Wi = W / 2; a.Cin = 32;
  a.w = d.put(rows); a.Kpad = kp; a.wf = d.put(frag_pack(rows.data(), kp, frag_list(3, 32, 64), true));
  a.w2 = d.put(r2); a.wf2 = d.put(frag_pack(r2.data(), 64, epilogue_frags(64, 64), false));
  std::vector<float> b1(conv_cout_pad(64), 0.f);
  for (int i = 0; i < 64; ++i) b1[i] = h_b1[i];
  a.bias = d.put(b1); a.bias2 = d.put(std::vector<float>(h_b2, h_b2 + 64)); a.cout2 = 64; a.zero = (const half_t*)d.zeroed(256);
  a.ksize = 3; a.stride = 2; a.pad = 1; a.Ho = H / 4; a.Wo = W / 4; a.Cout = 64; a.act = 1; a.w_rows = conv_cout_pad(64);
  a.y = d_y; a.y_bstride = (long)a.Ho * a.Wo * 64; a.ldy = 64; a.M = B * a.Ho * a.Wo;
  if (!st.w16 || !st.bias || !st.y || !a.w || !a.wf || !a.w2 || !a.wf2 || !a.bias || !a.bias2 || !a.zero) return alloc_failed();
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
  a.zero = (const half_t*)d.zeroed(256); a.act = 1; a.ksize = 2; a.stride = 1; a.pad = 0; a.phase = 1;
  a.Ho = H; a.Wo = W; a.Cout = 4 * n; a.convt_co = n; a.w_rows = cp;
  a.y = d_y; a.y_bstride = (long)4 * H * W * 32; a.ldy = 32; a.M = B * H * W;
  if (!a.w || !a.wf || !a.w2 || !a.wf2 || !a.bias || !a.bias2 || !a.zero) return alloc_failed();
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
  if (!ha.wf || !ha.bias) return alloc_failed();
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
  const int form = stride == 2 && k == 3 && H == 2 * Ho && W == 2 * Wo && !live_no_dgrad_phases() ? dgrad_phase_form(cin, cout, false) : 0;
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
  DevBuf d;
  ConvArgs a{};
  a.x = (const half_t*)d_dy; a.x_bstride = (long)Ho * Wo * cout; a.ldx = cout; a.Hi = Ho; a.Wi = Wo; a.Cin = cout;
  a.w = d.put(rows); a.Kpad = Kpad; a.bias = d.put(bias); a.zero = (const half_t*)d.zeroed(256); a.act = 0; a.w_rows = cout_pad;
  if (!a.w || !a.bias || !a.zero) return alloc_failed();
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
  return launch_status(rc, hipStreamSynchronize(s), "dgrad");
}

int m355_conv2d_wgrad(const void* d_x, const void* d_dy, int B, int H, int W, int cin, int cout, int k, int stride,
                      float* d_dw, void* stream) {
  if (!d_x || !d_dy || !d_dw) return set_err(M355_ERR_INVALID, "null pointer");
  if ((k != 1 && k != 3) || (stride != 1 && stride != 2)) return set_err(M355_ERR_INVALID, "wgrad supports k in {1,3}, stride in {1,2}");
  static half_t* zero_page = nullptr;  // 256 zero bytes, allocated once per process
  if (!zero_page) {
    void* z = nullptr;
    if (hipMalloc(&z, 256) != hipSuccess || hipMemset(z, 0, 256) != hipSuccess) {
      (void)hipFree(z);
      return alloc_failed();
    }
    zero_page = (half_t*)z;
  }
  const int pad = k / 2;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const size_t wsb = conv_wgrad_workspace_bytes(B, Ho, Wo, cin, cout, k);
  DevBuf d;
  float* ws = wsb ? (float*)d.alloc(wsb) : nullptr;
  if (wsb && !ws) return alloc_failed();
  const int rc = launch_conv_wgrad((const half_t*)d_dy, (long)Ho * Wo * cout, cout, (const half_t*)d_x, (long)H * W * cin,
                                   cin, B, H, W, cin, Ho, Wo, cout, k, stride, pad, d_dw, zero_page, ws, wsb, (hipStream_t)stream);
  const hipError_t se = hipStreamSynchronize((hipStream_t)stream);
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
  // every argument before any HIP call
  const char* entry = "m355_stem_fwd";
  if (!d_in || !h_w || !h_bias || !d_y) return glue_invalid(entry, "null pointer");
  if (cout != 16 && cout != 32 && cout != 48 && cout != 64 && cout != 80) return glue_invalid(entry, "cout must be 16, 32, 48, 64 or 80");
  if (B < 1) return glue_invalid(entry, "B must be >= 1");
  if (H < 2 || W < 2 || H % 2 || W % 2 || H > 32768 || W > 32768) return glue_invalid(entry, "H and W must be even and >= 2 (at most 32768)");
  if ((long)B * (H / 2) > 0x7fffffffL) return glue_invalid(entry, "too many output rows");
  if ((uintptr_t)d_in & 15) return glue_invalid(entry, "the image must be 16-byte aligned");
  if ((uintptr_t)d_y & 7) return glue_invalid(entry, "the output must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const std::vector<half_t> sw = pack_stem3x3(h_w, cout);
  DevBuf d;
  StemArgs a{};
  a.x = (const uint8_t*)d_in; a.B = B; a.H = H; a.W = W; a.w16 = d.put(sw); a.bias = d.put(std::vector<float>(h_bias, h_bias + cout));
  a.y = (half_t*)d_y; a.y_bstride = (long)(H / 2) * (W / 2) * cout; a.ldy = cout; a.Cout = cout;
  if (!a.w16 || !a.bias) return alloc_failed();
  const int rc = launch_stem(a, s);
  return launch_status(rc, hipStreamSynchronize(s), "stem");
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
  if (!a.w || !a.bias) return alloc_failed();
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
  if (!a.w || !a.bias) return alloc_failed();
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
  if (!a.pe_w || !a.pe_b) return alloc_failed();
  return finish_entry(launch_psa_attn(a, s), s, "psa_attn");
}

int m355_sppf_pool(const void* d_x, int B, int H, int W, int C, void* d_y, void* stream) {
  return sppf_entry("m355_sppf_pool", d_x, (int64_t)H * W * C, C, d_y, (int64_t)H * W * 3 * C, 3 * C, B, H, W, C, stream);
}

int m355_upsample2x(const void* d_x, int B, int H, int W, int C, void* d_y, void* stream) {
  return upsample_entry("m355_upsample2x", d_x, (int64_t)H * W * C, C, d_y, (int64_t)4 * H * W * C, C, B, H, W, C, stream);
}

int m355_head_decode(const float* d_raw, int B, int in_h, int in_w, int nc, float* d_preds, void* stream) {
  return decode_entry("m355_head_decode", d_raw, B, in_h, in_w, nc, 32, d_preds, stream);
}

int m355_head_decode_ex(const float* d_raw, int B, int in_h, int in_w, int nc, int nm, float* d_preds, void* stream) {
  return decode_entry("m355_head_decode_ex", d_raw, B, in_h, in_w, nc, nm, d_preds, stream);
}

// the body of m355_nms and m355_nms_ex, after their argument checks
static int nms_entry(const float* d_preds, int B, int A, int nc, int nm, float conf, float iou, int max_det, int agnostic,
                     const uint32_t* d_class_mask, float* d_dets, int* d_counts, void* stream) {
  const size_t wsb = nms_workspace_bytes(B, A);
  DevBuf d;
  void* ws = d.alloc(wsb);
  if (!ws) return alloc_failed();
  const int rc = launch_nms(d_preds, B, A, nc, nm, conf, iou, max_det, d_dets, d_counts, ws, wsb, (hipStream_t)stream,
                            agnostic, d_class_mask);
  return launch_status(rc, hipStreamSynchronize((hipStream_t)stream), "nms");
}

int m355_nms(const float* d_preds, int B, int A, int nc, int nm, float conf, float iou, int max_det, float* d_dets,
             int* d_counts, void* stream) {
  if (!d_preds || !d_dets || !d_counts) return set_err(M355_ERR_INVALID, "null pointer");
  return nms_entry(d_preds, B, A, nc, nm, conf, iou, max_det, 0, nullptr, d_dets, d_counts, stream);
}

int m355_nms_ex(const float* d_preds, int B, int A, int nc, int nm, float conf, float iou, int max_det, int agnostic,
                const uint32_t* d_class_mask, float* d_dets, int* d_counts, void* stream) {
  if (!d_preds || !d_dets || !d_counts) return set_err(M355_ERR_INVALID, "null pointer");
  if (B < 1 || A < 1 || nc < 1 || nm < 0) return set_err(M355_ERR_INVALID, "non-positive shape");
  if (max_det < 1 || max_det > 1024) return set_err(M355_ERR_INVALID, "max_det must be in [1, 1024]");
  if (agnostic != 0 && agnostic != 1) return set_err(M355_ERR_INVALID, "agnostic must be 0 or 1");
  if (d_class_mask && nc > 1024) return set_err(M355_ERR_INVALID, "a class set covers at most 1024 classes");
  return nms_entry(d_preds, B, A, nc, nm, conf, iou, max_det, agnostic, d_class_mask, d_dets, d_counts, stream);
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

int m355_letterbox_u8(const uint8_t* d_src, const m355_letterbox_image* h_table, int n, int net_h, int net_w,
                      uint8_t* d_out, void* stream) {
  if (!d_src || !h_table || !d_out) return set_err(M355_ERR_INVALID, "letterbox: null pointer");
  const int rc = launch_letterbox_u8(d_src, h_table, n, net_h, net_w, d_out, (hipStream_t)stream);
  if (rc == -1)
    return set_err(M355_ERR_INVALID, "letterbox: bad argument (n, net shape, output alignment, image or window size, offset table)");
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "letterbox launch failed: " + std::to_string(rc));
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
  const bool train_w1 = !proc_switches().no_train_w1;
  const bool train_c32 = !proc_switches().no_train_c32;   // 32 -> 32 3x3 layers on conv3x3_c32.hip: a further -0.1 ms
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
size_t m355_augment_ex_workspace_bytes(int32_t B, int32_t n_polys, int32_t n_verts) {
  return m355::augment_ex_workspace_bytes(B, n_polys, n_verts);
}
int m355_augment_ex(const void* d_cache, int32_t n_images, const m355_aug_ex_params* h_params, const m355_aug_poly* h_polys,
                    int32_t n_polys, const float* h_verts, int32_t n_verts, void* d_work, int64_t work_bytes, void* d_out,
                    int32_t B, int32_t H, int32_t W, void* stream) {
  if (!d_cache || !h_params || !d_work || !d_out) return set_err(M355_ERR_INVALID, "augment_ex: null pointer");
  const int rc = m355::launch_augment_ex((const uint8_t*)d_cache, n_images, h_params, h_polys, n_polys, h_verts, n_verts, d_work,
                                         work_bytes, (uint8_t*)d_out, B, H, W, (hipStream_t)stream);
  if (rc == -1)
    return set_err(M355_ERR_INVALID, "augment_ex: bad argument (shape, n_layers, src index, polygon or vertex range, paste cap, workspace)");
  return rc == 0 ? M355_OK : set_err(M355_ERR_HIP, "augment_ex launch failed: " + std::to_string(rc));
}
int m355_sppf_pool_launch(const void* x, int64_t x_bstride, int32_t ldx, void* y, int64_t y_bstride, int32_t ldy,
                          int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
  return sppf_entry("m355_sppf_pool_launch", x, x_bstride, ldx, y, y_bstride, ldy, B, H, W, C, stream);
}

int m355_sppf_pool_form(int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldy) { return sppf_pool_form(B, H, W, C, ldy); }

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

size_t m355_cls_bce_workspace_floats(void) { return cls_bce_workspace_floats(); }

int m355_cls_bce_launch(const float* raw, int32_t rw, const float* targets, int64_t rows, int32_t nc, const float* scale, float* d_raw,
                        float* out, void* stream) {
  const int rc = launch_cls_bce(raw, rw, targets, rows, nc, scale, d_raw, out, (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, "class-BCE launch failed: " + std::to_string(rc));
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
  return upsample_entry("m355_upsample2x_launch", x, x_bstride, ldx, y, y_bstride, ldy, B, H, W, C, stream);
}

int m355_adown_pool_launch(const void* x, int64_t x_bstride, int32_t ldx, void* a, int64_t a_bstride, int32_t lda, void* m,
                           int64_t m_bstride, int32_t ldm, int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
  const char* entry = "m355_adown_pool_launch";
  if (B < 1) return glue_invalid(entry, "B must be >= 1");
  if (H < 2 || W < 2 || H % 2 || W % 2 || H > (1 << 14) || W > (1 << 14)) return glue_invalid(entry, "H and W must be even and >= 2 (at most 16384)");
  if (C < 16 || C % 16) return glue_invalid(entry, "C must be a positive multiple of 16");
  std::string f = slice_fault("x", x, x_bstride, ldx, (long)H * W, C);
  if (f.empty()) f = slice_fault("a", a, a_bstride, lda, (long)(H - 1) * (W - 1), C / 2);
  if (f.empty()) f = slice_fault("m", m, m_bstride, ldm, (long)(H / 2) * (W / 2), C / 2);
  if (!f.empty()) return glue_invalid(entry, f);
  const int rc = launch_adown_pool((const half_t*)x, x_bstride, ldx, (half_t*)a, a_bstride, lda, (half_t*)m, m_bstride, ldm, B, H, W, C,
                                   (hipStream_t)stream);
  return rc == 0 ? M355_OK : set_err(rc == -1 ? M355_ERR_INVALID : M355_ERR_HIP, std::string(entry) + ": launch failed: " + std::to_string(rc));
}

}  // extern "C"
