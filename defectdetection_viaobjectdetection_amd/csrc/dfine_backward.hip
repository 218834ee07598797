// Backward of the D-FINE decoder ops of dfine_kernels.hip (fp32, head_dim 32, same layouts), for fine-tuning runs that
// call the bound ops under loss.backward().  No float atomics: every gradient has a fixed summation order and is bitwise
// reproducible (README "Training").
//
// msda backward, two passes:
//   pass 1  one wave per (b, q, h), the forward's lane mapping: lane k < 4 P owns the (point k >> 2, corner k & 3) pair.
//           It gathers the corner's 32-channel row, dots it with grad_out and combines the four dots of a point into
//           grad_attn / grad_loc (per-query, no conflicts).  For grad_value it writes ONE contribution entry per lane:
//           (destination pixel or -1, attention x corner weight), into a list per (b, h) that is ordered
//           (level, query, point of the level, corner).
//   pass 2  owner computes: a wave owns up to 64 consecutive pixels of one level of one (b, h), their 32-channel rows in
//           LDS, half of them per 32-lane half.  It scans that level's segment of the list 64 entries per step, finds
//           its own pixels with a ballot and adds weight x grad_out row to the LDS row in list order (the two halves of
//           the wave each walk their own hits), then writes its rows once.  Every element of
//           grad_value is written, so no memset is needed, and the sum per pixel does not depend on the ownership split.
#include "common.h"
#include "device_prims.h"

namespace m355 {
namespace {

constexpr int kOwnMax = 64;   // pixels a pass-2 wave owns at most (64 rows x 128 B = 8 KB of LDS per wave)

struct MsdaBwdArgs {
  const float* grad_out;  // (B, Q, H * 32)
  const float* value;     // (B, S, H, 32)
  const float* loc;       // (B, Q, H, P, 2); module mode: the raw sampling offsets
  const float* attn;      // (B, Q, H, P);    module mode: the raw attention logits
  const float* ref;       // (B, Q, 4) module mode, nullptr: core
  float offset_scale;
  float* grad_value;      // (B, S, H, 32) or nullptr
  float* grad_loc;        // (B, Q, H, P, 2) or nullptr (module mode: gradient of the offsets)
  float* grad_attn;       // (B, Q, H, P) or nullptr    (module mode: gradient of the logits)
  float4* ref_part;       // (B, Q, H) partial gradients of ref, module mode, or nullptr
  float* grad_ref;        // (B, Q, 4) module mode, or nullptr
  int2* list;             // (B, H, 4 * Q * P) entries {pixel of the (b, h) map or -1, weight bits}, or nullptr
  int B, S, H, Q, P, L;
  int lh[8], lw[8], lstart[8], pend[8];
  int seg[8];             // first entry of level l's segment inside a (b, h) list: 4 * Q * (points before the level)
  int blk0[9];            // pass 2: first block (within one (b, h)) of level l; blk0[L] = blocks per (b, h)
  int own;                // pass 2: pixels per wave, 8 .. kOwnMax
  int discrete;
};

__global__ __launch_bounds__(256) void msda_bwd_points_kernel(const MsdaBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const long triple = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (triple >= (long)a.B * a.Q * a.H) return;   // whole waves leave together
  const int h = (int)(triple % a.H);
  const long bq = triple / a.H;
  const int b = (int)(bq / a.Q), q = (int)(bq % a.Q);
  const bool need_dots = a.grad_loc || a.grad_attn || a.ref_part;
  // module mode (P <= 16: one chunk): softmax of the raw logits exactly as the forward forms it
  float soft = 0.f;
  if (a.ref) {
    const float z = lane < 4 * a.P ? a.attn[triple * a.P + (lane >> 2)] : -INFINITY;
    float m = z;
#pragma unroll
    for (int k = 4; k < 64; k <<= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
    const float e = lane < 4 * a.P ? __expf(z - m) : 0.f;
    float sum = e;
#pragma unroll
    for (int k = 4; k < 64; k <<= 1) sum += __shfl_xor(sum, k, 64);
    soft = e / sum;
  }
  const int slot = lane >> 3, c4 = lane & 7;
  const float4 g = ((const float4*)(a.grad_out + triple * 32))[c4];
  const float4* vb = (const float4*)(a.value + (long)b * a.S * a.H * 32 + h * 32) + c4;
  const long pix_stride4 = (long)a.H * 8;
  int2* list = a.list ? a.list + ((long)b * a.H + h) * 4 * a.Q * a.P : nullptr;

  for (int base = 0; base < 4 * a.P; base += 64) {   // P > 16: a second chunk of 64 (point, corner) pairs
    const int k = base + lane;
    const bool active = k < 4 * a.P;
    const int p = active ? k >> 2 : 0, corner = lane & 3;
    int l = 0;
    while (p >= a.pend[l]) ++l;
    const int W = a.lw[l], Hh = a.lh[l];
    const int pfirst = l ? a.pend[l - 1] : 0, npts = a.pend[l] - pfirst;
    const float* lp = a.loc + (triple * a.P + p) * 2;
    float x = lp[0], y = lp[1], aw = a.ref ? soft : a.attn[triple * a.P + p];
    const float ox = x, oy = y;
    float sx = 1.f, sy = 1.f;   // d location / d offset, module mode
    float tw = 0.f, th = 0.f;   // d location / d (ref.w, ref.h)
    if (a.ref) {
      const float* rp = a.ref + bq * 4;
      const float nscale = 1.0f / (float)npts;
      x = rp[0] + x * nscale * rp[2] * a.offset_scale;
      y = rp[1] + y * nscale * rp[3] * a.offset_scale;
      sx = nscale * rp[2] * a.offset_scale;
      sy = nscale * rp[3] * a.offset_scale;
      tw = ox * nscale * a.offset_scale;
      th = oy * nscale * a.offset_scale;
    }
    int pix = -1;               // destination pixel (level start included); -1: this corner contributes nothing
    float cw = 0.f;             // d out / d (attn * corner row)
    float dwx = 0.f, dwy = 0.f; // d cw / d x, d cw / d y (in units of the normalised location)
    if (active) {
      if (a.discrete) {
        long xi = (long)(x * (float)W + 0.5f), yi = (long)(y * (float)Hh + 0.5f);
        xi = xi < 0 ? 0 : (xi > W - 1 ? W - 1 : xi);
        yi = yi < 0 ? 0 : (yi > Hh - 1 ? Hh - 1 : yi);
        if (corner == 0) {
          pix = a.lstart[l] + (int)(yi * W + xi);
          cw = 1.f;
        }
      } else {
        const float gx = 2.f * x - 1.f, gy = 2.f * y - 1.f;
        const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)Hh - 1.f) * 0.5f;
        const float fx = floorf(ix), fy = floorf(iy);
        const float we = ix - fx, ws = iy - fy;
        const float cxf = fx + (float)(corner & 1), cyf = fy + (float)(corner >> 1);
        const bool ok = cxf >= 0.f && cxf <= (float)(W - 1) && cyf >= 0.f && cyf <= (float)(Hh - 1);
        const float wx = (corner & 1) ? we : 1.f - we, wy = (corner >> 1) ? ws : 1.f - ws;
        if (ok) {
          pix = a.lstart[l] + (int)cyf * W + (int)cxf;
          cw = wx * wy;
          dwx = ((corner & 1) ? wy : -wy) * (float)W;    // ix = x * W - 0.5
          dwy = ((corner >> 1) ? wx : -wx) * (float)Hh;
        }
      }
      if (list) {
        const long e = a.seg[l] + ((long)q * npts + (p - pfirst)) * 4 + corner;
        list[e] = make_int2(pix, __float_as_int(cw * aw));
      }
    }
    if (!need_dots) continue;
    // <corner row, grad_out> for every pair of the chunk, eight corners per load as the forward reads them
    const int gather_pix = pix < 0 ? 0 : pix;
    float dot = 0.f;
    const int left = 4 * a.P - base;
    const int iters = left >= 64 ? 8 : (left + 7) >> 3;
    for (int it = 0; it < iters; ++it) {
      const int off = __shfl(gather_pix, it * 8 + slot, 64);
      const float4 v = vb[(long)off * pix_stride4];
      float part = (v.x * g.x + v.y * g.y) + (v.z * g.z + v.w * g.w);
      part += __shfl_xor(part, 1, 64);
      part += __shfl_xor(part, 2, 64);
      part += __shfl_xor(part, 4, 64);
      const float d = __shfl(part, (lane & 7) * 8, 64);   // pair it * 8 + s was summed on the lanes of slot s
      if ((lane >> 3) == it) dot = d;
    }
    if (pix < 0) dot = 0.f;
    // the four corners of a point sit on lanes 4 p' .. 4 p' + 3
    float ga = cw * dot, glx = dwx * dot, gly = dwy * dot;
    ga += __shfl_xor(ga, 1, 64);   ga += __shfl_xor(ga, 2, 64);
    glx += __shfl_xor(glx, 1, 64); glx += __shfl_xor(glx, 2, 64);
    gly += __shfl_xor(gly, 1, 64); gly += __shfl_xor(gly, 2, 64);
    glx *= aw;                     // gradient of the sampling location
    gly *= aw;
    if (a.ref) {
      // softmax backward over the points, chain rule of the location through the offsets and the reference box
      float dotsum = active ? soft * ga : 0.f;
      float rx = active ? glx : 0.f, ry = active ? gly : 0.f;
      float rw = active ? glx * tw : 0.f, rh = active ? gly * th : 0.f;
#pragma unroll
      for (int m = 4; m < 64; m <<= 1) {
        dotsum += __shfl_xor(dotsum, m, 64);
        rx += __shfl_xor(rx, m, 64); ry += __shfl_xor(ry, m, 64);
        rw += __shfl_xor(rw, m, 64); rh += __shfl_xor(rh, m, 64);
      }
      ga = soft * (ga - dotsum);
      glx *= sx;
      gly *= sy;
      if (a.ref_part && lane == 0) a.ref_part[triple] = make_float4(rx, ry, rw, rh);
    }
    if (active && corner == 0) {
      if (a.grad_attn) a.grad_attn[triple * a.P + p] = ga;
      if (a.grad_loc) ((float2*)a.grad_loc)[triple * a.P + p] = make_float2(glx, gly);
    }
  }
}

// grad_ref (b, q, :) = sum over the heads of the pass-1 partials, in head order
__global__ void msda_bwd_ref_kernel(const MsdaBwdArgs a) {
  const long bq = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (bq >= (long)a.B * a.Q) return;
  float4 s = a.ref_part[bq * a.H];
  for (int h = 1; h < a.H; ++h) {
    const float4 v = a.ref_part[bq * a.H + h];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  ((float4*)a.grad_ref)[bq] = s;
}

__global__ __launch_bounds__(256) void msda_bwd_value_kernel(const MsdaBwdArgs a) {
  __shared__ float rows[4][kOwnMax][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = a.blk0[a.L];
  const int r = (int)(blockIdx.x % per);
  const long bh = blockIdx.x / per;
  const int b = (int)(bh / a.H), h = (int)(bh % a.H);
  int l = 0;
  while (r >= a.blk0[l + 1]) ++l;
  const int npix = a.lh[l] * a.lw[l];
  const int lo = ((r - a.blk0[l]) * 4 + wave) * a.own;   // first owned pixel, within the level
  if (lo >= npix) return;                                // no block-wide barrier below: a wave may leave alone
  const int cnt = min(a.own, npix - lo);
  const int glo = a.lstart[l] + lo;
  const int c = lane & 31, half = lane >> 5;
  float (*mine)[32] = rows[wave];
  // Each 32-lane half of the wave owns half of the rows, [first, last), and walks its own hits: the two halves add to two
  // pixels per step.  Lane (half, c) is the only lane that ever touches column c of those rows, so nothing crosses lanes
  // through LDS, and a pixel's terms are still added in list order.
  const int first = min(cnt, half * (a.own >> 1)), last = half ? cnt : min(cnt, a.own >> 1);
  for (int i = first; i < last; ++i) mine[i][c] = 0.f;
  const int npts = a.pend[l] - (l ? a.pend[l - 1] : 0);
  const long nent = 4L * a.Q * npts;
  const int2* seg = a.list + bh * 4 * a.Q * a.P + a.seg[l];
  const float* go = a.grad_out + (long)b * a.Q * a.H * 32 + h * 32 + c;
  const long go_stride = (long)a.H * 32;
  for (long e0 = 0; e0 < nent; e0 += 64) {
    const long e = e0 + lane;
    int2 ent = make_int2(-1, 0);
    if (e < nent) ent = seg[e];
    const int rel = ent.x - glo;
    const int split = min(cnt, a.own >> 1);
    const unsigned long long hits_lo = __ballot((unsigned)rel < (unsigned)split);
    const unsigned long long hits_hi = __ballot(rel >= split && rel < cnt);
    unsigned long long hits = half ? hits_hi : hits_lo;   // this half's hits
    while (__any(hits != 0)) {
      // up to four hits of each half per round: their grad_out rows are fetched together, then added in list order.
      // The shuffles run on every lane (a half without a hit left reads lane 0 and drops it).
      int row[4];
      float wt[4], gv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool has = hits != 0;
        const int j = has ? __ffsll((long long)hits) - 1 : 0;
        hits &= hits - 1;                                  // 0 stays 0
        const int rj = __shfl(rel, j, 64);
        row[u] = has ? rj : -1;
        wt[u] = __int_as_float(__shfl(ent.y, j, 64));
        gv[u] = has ? go[(e0 + j) / (4 * npts) * go_stride] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (row[u] >= 0) mine[row[u]][c] += wt[u] * gv[u];
    }
  }
  float* gvp = a.grad_value + ((long)b * a.S + glo) * a.H * 32 + h * 32 + c;
  for (int i = first; i < last; ++i) gvp[(long)i * a.H * 32] = mine[i][c];
}

// One thread per box: recompute the four softmax expectations, push grad_boxes through (clamp,) centre format and
// distance2bbox, then through the expectation: d d / d z_k = p_k (project_k - d).
// GUARD: the backward of dfine_decode_kernel<true>, as torch differentiates the chain: nan_to_num passes the gradient where its
// input is finite, so a replaced box coordinate, a replaced distance and a replaced logit each receive 0.
template <bool GUARD>
__global__ void dfine_decode_bwd_kernel(const float* gboxes, const float* dist, const float* project, const float* ref,
                                        float* gdist, float* gref, long n, int nbins1, float reg_scale, int clamp01) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  auto logit = [](float z) { return GUARD ? nan_to_num(z, 0.f, 1.f, 0.f) : z; };
  float d[4], draw[4], mx[4], sum[4];   // draw: the expectation itself, d: what distance2bbox read
  for (int s = 0; s < 4; ++s) {
    const float* z = dist + (i * 4 + s) * nbins1;
    float m = logit(z[0]);
    for (int k = 1; k < nbins1; ++k) m = fmaxf(m, logit(z[k]));
    float sm = 0.f, dot = 0.f;
    for (int k = 0; k < nbins1; ++k) {
      const float e = expf(logit(z[k]) - m);
      sm += e;
      dot += e * project[k];
    }
    draw[s] = dot / sm; mx[s] = m; sum[s] = sm;
    d[s] = GUARD ? nan_to_num(draw[s], 0.f, 1.f, 0.f) : draw[s];
  }
  const float rs = fabsf(reg_scale);
  const float cx = ref[i * 4], cy = ref[i * 4 + 1], w = ref[i * 4 + 2], hh = ref[i * 4 + 3];
  float go[4];
  for (int k = 0; k < 4; ++k) go[k] = gboxes[i * 4 + k];
  if (clamp01 || GUARD) {
    const float x0 = cx - (0.5f * rs + d[0]) * (w / rs), y0 = cy - (0.5f * rs + d[1]) * (hh / rs);
    const float x1 = cx + (0.5f * rs + d[2]) * (w / rs), y1 = cy + (0.5f * rs + d[3]) * (hh / rs);
    const float o[4] = {(x0 + x1) / 2.f, (y0 + y1) / 2.f, x1 - x0, y1 - y0};
    for (int k = 0; k < 4; ++k) {
      if (clamp01 && !(o[k] >= 0.f && o[k] <= 1.f)) go[k] = 0.f;   // torch.clamp: the gradient passes where min <= x <= max
      if (GUARD && !__builtin_isfinite(o[k])) go[k] = 0.f;         // a replaced coordinate (with clamp01: taken above already)
    }
  }
  // (x0 + x1) / 2, x1 - x0
  const float gx0 = go[0] * 0.5f - go[2], gx1 = go[0] * 0.5f + go[2];
  const float gy0 = go[1] * 0.5f - go[3], gy1 = go[1] * 0.5f + go[3];
  const float gd[4] = {-gx0 * (w / rs), -gy0 * (hh / rs), gx1 * (w / rs), gy1 * (hh / rs)};
  if (gref) {
    gref[i * 4] = gx0 + gx1;
    gref[i * 4 + 1] = gy0 + gy1;
    gref[i * 4 + 2] = (gx1 * (0.5f * rs + d[2]) - gx0 * (0.5f * rs + d[0])) / rs;
    gref[i * 4 + 3] = (gy1 * (0.5f * rs + d[3]) - gy0 * (0.5f * rs + d[1])) / rs;
  }
  if (gdist)
    for (int s = 0; s < 4; ++s) {
      const float* z = dist + (i * 4 + s) * nbins1;
      float* gz = gdist + (i * 4 + s) * nbins1;
      const bool replaced = GUARD && !__builtin_isfinite(draw[s]);   // a replaced distance passes nothing on
      for (int k = 0; k < nbins1; ++k) {
        const float v = expf(logit(z[k]) - mx[s]) / sum[s] * (project[k] - draw[s]) * gd[s];
        gz[k] = (replaced || (GUARD && !__builtin_isfinite(z[k]))) ? 0.f : v;
      }
    }
}

size_t list_bytes(int B, int Q, int H, int P) { return (size_t)B * H * 4 * Q * P * sizeof(int2); }

}  // namespace

size_t msda_backward_workspace_bytes(int B, int Q, int H, int P) {
  if (B < 1 || Q < 1 || H < 1 || P < 1) return 0;
  return list_bytes(B, Q, H, P) + (size_t)B * Q * H * sizeof(float4);   // contribution list + per-head partials of grad_ref
}

// ownership: the largest share per wave that still gives every CU a few blocks; the result does not depend on it
long msda_backward_value_blocks(const MsdaLevels& lv, int B, int H, int* own, int* blk0) {
  for (*own = kOwnMax; ; *own >>= 1) {
    int per = 0;
    for (int l = 0; l < lv.L; ++l) {
      blk0[l] = per;
      per += (int)(((long)lv.lh[l] * lv.lw[l] + 4 * *own - 1) / (4 * *own));
    }
    blk0[lv.L] = per;
    const long blocks = (long)B * H * per;
    if (blocks >= 1024 || *own == 8) return blocks;
  }
}

int launch_msda_backward(const float* grad_out, const float* value, const float* loc, const float* attn, float* grad_value,
                         float* grad_loc, float* grad_attn, int B, int S, int H, int Q, int P, const MsdaLevels& lv, int discrete,
                         void* work, hipStream_t s, const float* ref, float offset_scale, float* grad_ref) {
  MsdaBwdArgs a{};
  a.grad_out = grad_out; a.value = value; a.loc = loc; a.attn = attn; a.ref = ref; a.offset_scale = offset_scale;
  a.grad_value = grad_value; a.grad_loc = grad_loc; a.grad_attn = grad_attn; a.grad_ref = grad_ref;
  a.B = B; a.S = S; a.H = H; a.Q = Q; a.P = P; a.L = lv.L; a.discrete = discrete;
  for (int l = 0; l < lv.L; ++l) {
    a.lh[l] = lv.lh[l]; a.lw[l] = lv.lw[l]; a.lstart[l] = lv.lstart[l]; a.pend[l] = lv.pend[l];
    a.seg[l] = l ? 4 * Q * lv.pend[l - 1] : 0;
  }
  if (grad_value) a.list = (int2*)work;
  if (grad_ref) a.ref_part = (float4*)((char*)work + list_bytes(B, Q, H, P));
  const long ntriples = (long)B * Q * H;
  if (grad_value || grad_loc || grad_attn || grad_ref)
    hipLaunchKernelGGL(msda_bwd_points_kernel, dim3((unsigned)((ntriples + 3) / 4)), dim3(256), 0, s, a);
  if (grad_ref) hipLaunchKernelGGL(msda_bwd_ref_kernel, dim3((unsigned)(((long)B * Q + 127) / 128)), dim3(128), 0, s, a);
  if (grad_value) {
    const long blocks = msda_backward_value_blocks(lv, B, H, &a.own, a.blk0);
    hipLaunchKernelGGL(msda_bwd_value_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  }
  return (int)hipGetLastError();
}

int launch_dfine_decode_backward(const float* grad_boxes, const float* dist, const float* project, const float* ref,
                                 float* grad_dist, float* grad_ref, long n, int nbins1, float reg_scale, int clamp01,
                                 hipStream_t s, bool guard) {
  if (n == 0 || (!grad_dist && !grad_ref)) return 0;
  const dim3 grid((unsigned)((n + 127) / 128));
  if (guard)
    hipLaunchKernelGGL(dfine_decode_bwd_kernel<true>, grid, dim3(128), 0, s, grad_boxes, dist, project, ref, grad_dist, grad_ref, n,
                       nbins1, reg_scale, clamp01);
  else
    hipLaunchKernelGGL(dfine_decode_bwd_kernel<false>, grid, dim3(128), 0, s, grad_boxes, dist, project, ref, grad_dist, grad_ref, n,
                       nbins1, reg_scale, clamp01);
  return (int)hipGetLastError();
}

}  // namespace m355
