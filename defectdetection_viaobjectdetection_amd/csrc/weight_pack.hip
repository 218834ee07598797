// Host-side weight packing (weight_pack.h): the fp16 row and MFMA-fragment layouts of the kernels, each written once, used by
// m355_set_conv_weights (engine.hip) and by the per-op entries (op_entries.hip).
#include "weight_pack.h"

#include <algorithm>

namespace m355 {

// Pack fp32 (cout,cin,k,k) -> fp16 rows [row0+co][ (kh*k+kw)*cin + ci ] of a [cout_pad][Kpad] matrix.
void pack_conv_rows(const float* w, int cout, int cin, int k, int Kpad, int row0, std::vector<half_t>& dst, int koff) {
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int kh = 0; kh < k; ++kh)
        for (int kw = 0; kw < k; ++kw)
          dst[(size_t)(row0 + co) * Kpad + koff + (kh * k + kw) * cin + ci] =
              (half_t)w[(((size_t)co * cin + ci) * k + kh) * k + kw];
}

// ConvTranspose2d(2x2, s2): fp32 (cin,cout,2,2) -> fp16 rows [virtual channel (dy*2+dx)*cout + co][ci], K = cin.
void pack_convt2x2_rows(const float* w, int cin, int cout, int Kpad, std::vector<half_t>& dst) {
  for (int c = 0; c < cin; ++c)
    for (int co = 0; co < cout; ++co)
      for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx)
          dst[(size_t)((dy * 2 + dx) * cout + co) * Kpad + c] = (half_t)w[(((size_t)c * cout + co) * 2 + dy) * 2 + dx];
}

// 3x3 stem (cin = 3): fp32 (cout,3,3,3) -> fp16 [cout][32], k = (kh*3+kw)*3+c, zero past k = 27; 1/255 is applied in the kernel's epilogue.
std::vector<half_t> pack_stem3x3(const float* w, int cout) {
  std::vector<half_t> sw((size_t)cout * 32, (half_t)0.f);
  for (int co = 0; co < cout; ++co)
    for (int c = 0; c < 3; ++c)
      for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) sw[(size_t)co * 32 + (kh * 3 + kw) * 3 + c] = (half_t)w[((co * 3 + c) * 3 + kh) * 3 + kw];
  return sw;
}

// The rows of a 1x1 conv applied in its producer's epilogue (proto.cv3, C2f.cv1 after a stride-2 conv): plain fp16, [cout2][K].
std::vector<half_t> to_half_vec(const float* w, size_t n) {
  std::vector<half_t> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = (half_t)w[i];
  return r;
}

// Fragment-ordered copy of packed rows for the weights-in-registers kernels.  Fragment f = (first row r0 of a 32-row block,
// first K element k0 of a 16-deep slice); out[(f * 64 + lane) * 8 + j] = rows[(r0 + perm(lane & 31)) * Kpad + k0 + 8 * (lane >> 5)
// + j]: exactly the A operand of one v_mfma_f32_32x32x16_f16, so a wave fetches a fragment with ONE coalesced 1 KiB load
// (lane-linear 16 bytes) instead of 64 scattered 16-byte pieces of 32 different rows (measured in round 3: a scattered prologue cost ~10 us of a 31 us launch).  perm: plain (lane-half h's accumulators = channels 16 h + r) or operand
// (c2f_c32.hip: accumulators = the next MFMA's B fragments).
static int frag_row(int rho, bool operand) {
  if (!operand) return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3);
  const int q = rho >> 3, h = (rho >> 2) & 1, i = rho & 3;
  return 16 * (q >> 1) + 8 * h + 4 * (q & 1) + i;
}
std::vector<half_t> frag_pack(const half_t* rows, int Kpad, const FragList& frags, bool operand) {
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
FragList frag_grid(int rows, int K) {
  FragList f;
  for (int r = 0; r < rows; r += 32)
    for (int k = 0; k < K; k += 16) f.push_back({r, k});
  return f;
}

// the fragment lists of the kernels, by conv shape (empty = none of them takes this conv)
FragList frag_list(int k, int cin, int cout) {
  // (64 -> 64 and 128 -> 128 3x3 convs had lists for conv3x3_c64r / conv3x3_c128r: measured no gain in round 3, deleted in round 4;
  // such a conv gets fragments only when a row-slab launch uses it -- PhysConv::planes, planes_frag_pack)
  const bool taken = (k == 3 && cin == 64 && cout == 128) ||                   // conv3x3_s2c64
                     (k == 3 && cin == 32 && (cout == 64 || cout == 32)) ||    // conv_stem_c2 (model.1, operand row order), c2f_c32
                     (k == 1 && (cin == 128 || cin == 192 || cin == 256 || cin == 384 || cin == 512) && cout % 128 == 0 && cout <= 512);   // conv1x1_wreg
  return taken ? frag_grid(cout, k * k * cin) : FragList();
}

// head_tail.hip: the 18 fragments of a head level's block-diagonal matrix (head_tail_layout) -- box rows 0-63 over K 0-63, class
// rows from 64 over K 64-191 (the rows behind them are coefficient rows: zero there), coefficient rows from 64 + nc over K 192-223
FragList head_level_frags(int nc) {
  FragList f = frag_grid(64, 64);
  for (int sl = 0; sl < 8; ++sl) f.push_back({64, 64 + 16 * sl});
  for (int sl = 0; sl < 2; ++sl) f.push_back({64 + nc, 192 + 16 * sl});
  return f;
}

// the 1x1 conv in the epilogue of the kernels that hold it in registers: proto.cv3 (32 x 128, proto_phase_wreg.hip), and the
// C2f cv1 after a stride-2 conv (64 x 64 on conv_stem_c2, 128 x 128 on conv3x3_s2c64)
FragList epilogue_frags(int cout2, int k) { return frag_grid(cout2, k); }

// ConvTranspose2d(2x2, s2, bias) followed by Conv3x3 (no activation between them) as four 2x2 phase convs over the low-resolution input
// (see build_segment_head in graph.hip): fp16 rows [4 n (padded to cout_pad)][Kpad], K = (a * 2 + b) * n + cin, and the [9 border classes][n] bias table.
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
  FragList fl;
  for (int cb = 0; cb < cblocks; ++cb)
    for (int p = 0; p < cin / 32; ++p)
      for (int tap = 0; tap < 9; ++tap)
        for (int s = 0; s < 2; ++s) fl.push_back({32 * cb, tap * cin + 32 * p + 16 * s});
  return frag_pack(rows, Kpad, fl, false);
}

// The row-slab fragments of a conv of cout channels: its rows padded with zero rows to planes_cblocks(cout) channel blocks.
std::vector<half_t> planes_frag_pack_padded(const half_t* rows, int cout, int Kpad, int cin) {
  const int cbl = planes_cblocks(cout);
  std::vector<half_t> padded((size_t)cbl * 32 * Kpad, (half_t)0.f);
  std::copy(rows, rows + (size_t)cout * Kpad, padded.begin());
  return planes_frag_pack(padded.data(), Kpad, cin, cbl);
}

// Block-diagonal single mode of the row-slab kernel (launch_conv3x3_blockdiag): n convs side by side, conv i's rows [cout[i]][kpad[i]]
// over its OWN cin[i] input channels.  The list is the convs' planes_frag_pack_padded lists one after the other -- [conv][channel
// block][plane of that conv][tap][slice] -- so a conv's fragments are exactly those of its own launch.
std::vector<half_t> planes_frag_pack_diag(const half_t* const* rows, const int* cout, const int* kpad, const int* cin, int n) {
  std::vector<half_t> out;
  for (int i = 0; i < n; ++i) {
    const std::vector<half_t> f = planes_frag_pack_padded(rows[i], cout[i], kpad[i], cin[i]);
    out.insert(out.end(), f.begin(), f.end());
  }
  return out;
}

}  // namespace m355
