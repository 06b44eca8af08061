// upcat.hip -- one decoder level of URHand's DisplacementUNet as one operator, forward and backward, gfx950.
//
// The two decoder branches of DisplacementUNet.forward (ca_code/models/urhand.py:217-226, :231-239) do, per
// level, F.leaky_relu(x, 0.2) on the previous layer's output, an exact 2x bilinear resize (align_corners=True), a concat
// with the encoder's skip activation and a weight-normalised 3x3 / stride 1 / pad 1 convolution with an untied bias
// (la.Conv2dWNUB), with tanh and an affine after the last level (:227-228, :240-241).  Here, for xa[B,Ca,Hi,Wi] (the
// previous layer's output BEFORE its activation), xb[B,Cb,H,W] (the skip), H = 2 Hi, W = 2 Wi:
//     L = lrelu(xa, leak);  U = bilinear 2x of L by the integer-ratio rule of upconv.hip (gol_upconv.h)
//     acc[b,co,r,c] = sum_{ci<Ca,ky,kx} Upad[b,ci,r-1+ky,c-1+kx] w[co,ci,ky,kx] + sum_{cj<Cb,ky,kx} xbpad[b,cj,..] w[co,Ca+cj,ky,kx]
//     act 0:  y = acc + bias[co,r,c]            act 1:  y = tanh(acc + bias[co,r,c]) out_scale + out_shift
// L, U and the concatenated tensor never exist in memory.  All GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32), operand
// layout as in upconv.hip; tiles, LDS strides, the blending loader, the MFMA core and the reduction come from gol_upconv.h.
//   fwd     a workgroup owns 8 x 32 output pixels x 16 CT output channels.  The K loop walks Ca in stages of 8 channels
//           through the blending loader (the leaky applied to the loaded texels before the blend), then Cb in stages of 8
//           through a plain haloed-window loader; a stage never straddles the two (Ca and Cb are multiples of 8).
//           Co <= 4 (the 128 -> 1 heads) takes the same kernel with the missing rows as zero weights.
//   bwd     g_pre = g_y (act 0) or g_y out_scale (1 - t^2), t = (y - out_shift) / out_scale (act 1) is formed while loading.
//     bwd_xa  upconv.hip's input gradient over weight channels 0 .. Ca-1: the region of g_U that reaches a 4 x 16 tile of xa
//             is computed into LDS and gathered per texel with the bilinear weights (no atomics), times the leaky mask of xa.
//     bwd_xb  the plain transposed convolution over weight channels Ca ..: the forward's GEMM with the roles of the channels
//             exchanged and the taps mirrored while the weights are staged (no flipped copy of the weight).
//     bwd_w   per (16 co x 16 ci) a GEMM over pixels with nine accumulator tiles; the ci tiles are those of the blended half
//             (U recomputed from xa) followed by those of the plain half.  K is split over workgroups, the partial sums go
//             to scratch and up_bwd_w_reduce_kernel adds them in a fixed order (bitwise reproducible).
//     bwd_s   g_bias = sum_b g_pre.
#include "gol_upconv.h"

namespace {

// loads in flight per thread in the weight gradient's loaders.  4, not upconv.hip's 8: 66 VGPRs instead of 211, so the 42 KB
// of LDS and not the registers set the residency -- 3 workgroups per CU, exactly the one round of 768 that up_bwd_w_blocks
// plans (with 8: 2 per CU, a round and a half).  Measured at 64 + 64 -> 1 @ 512^2 / -> 64 @ 256^2: 0.646 / 0.652 ms against
// 0.785 / 0.819 ms (profiles/LOG.md).
constexpr int kBwUnroll = 4;

struct UcDims {
  int B, Ca, Cb, Co, Hi, Wi, H, W, act;
  float leak, scale, shift, inv_scale;
};

__device__ __forceinline__ float uc_gpre(const UcDims& p, float g, float yv) {
  if (p.act == 0) return g;
  const float t = (yv - p.shift) * p.inv_scale;
  return g * p.scale * (1.f - t * t);
}

// KC planes of the ROWS x COLS window with origin (r0, c0) of the plain tensor xb[C][H][W] into LDS; outside the image and
// past C: zeros.  Unconditional clamped loads in an unrolled loop, as in up_stage_u.
template <int KC, int ROWS, int COLS, int PLANE, int UNROLL>
__device__ __forceinline__ void uc_stage_plain(float* s_u, const float* __restrict__ xb, int ch0, int C, int r0, int c0, int H,
                                               int W, size_t HW, int tid) {
  constexpr int N = (KC / 4) * ROWS * COLS;
#pragma unroll UNROLL
  for (int it = 0; it < (N + 255) / 256; ++it) {
    const int idx = tid + 256 * it, idc = min(idx, N - 1);
    const int grp = idc / (ROWS * COLS), pos = idc - grp * (ROWS * COLS), rr = pos / COLS, cc = pos - rr * COLS;
    const int r = r0 + rr, c = c0 + cc;
    const bool in = r >= 0 && r < H && c >= 0 && c < W;
    const unsigned o = in ? (unsigned)r * (unsigned)W + (unsigned)c : 0u;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = xb[(size_t)min(ch0 + grp * 4 + u, C - 1) * HW + o];
    if (idx < N) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ch = grp * 4 + u;
        s_u[ch * PLANE + pos] = (in && ch0 + ch < C) ? v[u] : 0.f;
      }
    }
  }
}

// KC planes of the ROWS x COLS window with origin (r0, c0) of g_pre into LDS, formed from g_y (and y for act 1)
template <int KC, int ROWS, int COLS, int PLANE>
__device__ __forceinline__ void uc_stage_gpre(float* s_g, const UcDims& p, const float* __restrict__ gb,
                                              const float* __restrict__ yb, int co0, int r0, int c0, size_t HW, int tid) {
  constexpr int N = (KC / 4) * ROWS * COLS;
#pragma unroll
  for (int it = 0; it < (N + 255) / 256; ++it) {
    const int idx = tid + 256 * it, idc = min(idx, N - 1);
    const int grp = idc / (ROWS * COLS), pos = idc - grp * (ROWS * COLS), rr = pos / COLS, cc = pos - rr * COLS;
    const int r = r0 + rr, c = c0 + cc;
    const bool in = r >= 0 && r < p.H && c >= 0 && c < p.W;
    const unsigned o = in ? (unsigned)r * (unsigned)p.W + (unsigned)c : 0u;
    float vg[4], vy[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t oo = (size_t)min(co0 + grp * 4 + u, p.Co - 1) * HW + o;
      vg[u] = gb[oo];
      vy[u] = p.act ? yb[oo] : 0.f;
    }
    if (idx < N) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int cl = grp * 4 + u;
        s_g[cl * PLANE + pos] = (in && co0 + cl < p.Co) ? uc_gpre(p, vg[u], vy[u]) : 0.f;
      }
    }
  }
}

// wave -> rows 2 wave, 2 wave + 1 of the 8 x 32 tile, two halves of 16 columns each
__device__ __forceinline__ void uc_tile_pixels(int wave, int j, int (&poff)[4], int (&prow)[4], int (&pcol)[4]) {
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    prow[pt] = wave * 2 + (pt >> 1);
    pcol[pt] = (pt & 1) * 16 + j;
    poff[pt] = prow[pt] * kHC + pcol[pt];
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
// grid (tiles of 8 x 32 pixels, B, groups of 16 CT output channels)
template <int CT, int ACT>
__global__ __launch_bounds__(256) void uc_fwd_kernel(const UcDims p, const float* __restrict__ pxa,
                                                     const float* __restrict__ pxb, const float* __restrict__ pw,
                                                     const float* __restrict__ pbias, float* __restrict__ py) {
  __shared__ float s_u[kFwdKC * kFwdPlane];
  __shared__ float s_w[9 * kFwdKC * 16 * CT];
  __shared__ int s_ra[kHR], s_rb[kHR], s_ca[kHC], s_cb[kHC];
  __shared__ float s_rf[kHR], s_cf[kHC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, Ca = p.Ca, Cb = p.Cb, Co = p.Co, Ct = Ca + Cb;
  const int ntx = (W + kTW - 1) / kTW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int r0 = ty * kTH, c0 = tx * kTW, b = blockIdx.y, cog0 = blockIdx.z * (16 * CT);
  const size_t HWi = (size_t)p.Hi * p.Wi, HW = (size_t)H * W;
  const float* xab = pxa + (size_t)b * Ca * HWi;
  const float* xbb = pxb + (size_t)b * Cb * HW;
  up_fill_axis(s_ra, s_rb, s_rf, kHR, r0 - 1, p.Hi, H, p.Wi, tid);
  up_fill_axis(s_ca, s_cb, s_cf, kHC, c0 - 1, p.Wi, W, 1, tid);
  int poff[4], prow[4], pcol[4];
  uc_tile_pixels(wave, j, poff, prow, pcol);
  f32x4 acc[4][CT];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Ct; k0 += kFwdKC) {
    __syncthreads();  // the tables are written / the previous stage has been consumed
    if (k0 < Ca)      // (workgroup-uniform) the blended half, then the skip
      up_stage_u<kFwdKC, kHR, kHC, kFwdPlane, (CT > 1 ? 8 : 1), true>(s_u, s_ra, s_rb, s_rf, s_ca, s_cb, s_cf, xab, k0, Ca, HWi,
                                                                      tid, p.leak);
    else
      uc_stage_plain<kFwdKC, kHR, kHC, kFwdPlane, (CT > 1 ? 8 : 1)>(s_u, xbb, k0 - Ca, Cb, r0 - 1, c0 - 1, H, W, HW, tid);
    for (int idx = tid; idx < 16 * CT * kFwdKC * 9; idx += 256) {  // w[co][k0 .. k0 + 8][tap]: 72 consecutive floats per co
      const int col = idx / (kFwdKC * 9), rem = idx - col * (kFwdKC * 9), kl = rem / 9, tap = rem - kl * 9;
      const int co = cog0 + col;
      s_w[(tap * kFwdKC + kl) * (16 * CT) + col] = co < Co ? pw[((size_t)co * Ct + k0 + kl) * 9 + tap] : 0.f;
    }
    __syncthreads();
    up_conv_core<CT, 4, kFwdKC>(s_u, kFwdPlane, kHC, s_w, poff, acc, j, g);
  }
  // epilogue on the accumulators: D row = channel cog0 + 16 ct + 4 g + r4, column = pixel j of the pixel tile
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int r = r0 + prow[pt], c = c0 + pcol[pt];
    if (r >= H || c >= W) continue;
    const unsigned o = (unsigned)r * (unsigned)W + (unsigned)c;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int co = cog0 + 16 * ct + 4 * g + r4;
        if (co >= Co) continue;
        const float v = acc[pt][ct][r4] + pbias[(size_t)co * HW + o];
        py[((size_t)b * Co + co) * HW + o] = ACT == 0 ? v : tanhf(v) * p.scale + p.shift;
      }
  }
}

// ---- gradient of xa --------------------------------------------------------------------------------------------------
// grid (tiles of 4 x 16 texels of xa, B, tiles of 16 channels of xa); KC = output channels per K stage (4 for Co <= 4)
template <int KC>
__global__ __launch_bounds__(256) void uc_bwd_xa_kernel(const UcDims p, const float* __restrict__ pxa,
                                                        const float* __restrict__ pw, const float* __restrict__ py,
                                                        const float* __restrict__ pg, float* __restrict__ pgx) {
  __shared__ float s_g[KC * kBxPlane];
  __shared__ float s_gu[16 * kUR * kUC];
  __shared__ float s_w[9 * KC * 16];
  __shared__ int s_ra[kUR], s_rb[kUR], s_ca[kUC], s_cb[kUC];
  __shared__ float s_rf[kUR], s_cf[kUC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, Hi = p.Hi, Wi = p.Wi, Ca = p.Ca, Co = p.Co, Ct = p.Ca + p.Cb;
  const int ntx = (Wi + kSW - 1) / kSW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int i0 = ty * kSH, j0 = tx * kSW, b = blockIdx.y, cig0 = blockIdx.z * 16;
  const int rlo = up_first_row(i0, Hi, H), clo = up_first_row(j0, Wi, W);
  const size_t HW = (size_t)H * W;
  // source indices (mul = 1) and fractions of the region's rows and columns; -1 = outside the image
  up_fill_axis(s_ra, s_rb, s_rf, kUR, rlo, Hi, H, 1, tid);
  up_fill_axis(s_ca, s_cb, s_cf, kUC, clo, Wi, W, 1, tid);
  int poff[kBxNPT], pq[kBxNPT];
#pragma unroll
  for (int pt = 0; pt < kBxNPT; ++pt) {
    const int q = (wave * kBxNPT + pt) * 16 + j;
    pq[pt] = q < kUR * kUC ? q : -1;
    const int qq = q < kUR * kUC ? q : 0, row = qq / kUC;
    poff[pt] = row * kGC + (qq - row * kUC);
  }
  f32x4 acc[kBxNPT][1];
#pragma unroll
  for (int pt = 0; pt < kBxNPT; ++pt) acc[pt][0] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* gb = pg + (size_t)b * Co * HW;
  const float* yb = p.act ? py + (size_t)b * Co * HW : nullptr;
  for (int co0 = 0; co0 < Co; co0 += KC) {
    __syncthreads();
    uc_stage_gpre<KC, kGR, kGC, kBxPlane>(s_g, p, gb, yb, co0, rlo - 1, clo - 1, HW, tid);  // the haloed window of g_pre
    for (int idx = tid; idx < KC * 16 * 9; idx += 256) {  // A[ci][co][tap'] = w[co][ci][8 - tap'] (the mirrored taps)
      const int kl = idx / 144, rem = idx - kl * 144, cil = rem / 9, tw = rem - cil * 9;
      const int co = co0 + kl, ci = cig0 + cil;
      s_w[((8 - tw) * KC + kl) * 16 + cil] = (co < Co && ci < Ca) ? pw[((size_t)co * Ct + ci) * 9 + tw] : 0.f;
    }
    __syncthreads();
    up_conv_core<1, kBxNPT, KC>(s_g, kBxPlane, kGC, s_w, poff, acc, j, g);
  }
  // g_U of the region to LDS: D row = channel 4 g + r4, column = pixel
#pragma unroll
  for (int pt = 0; pt < kBxNPT; ++pt)
    if (pq[pt] >= 0) {
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) s_gu[(4 * g + r4) * (kUR * kUC) + pq[pt]] = acc[pt][0][r4];
    }
  __syncthreads();
  // the bilinear adjoint as a gather: thread -> texel tid & 63 of the tile, channels tid >> 6 + 4 u
  const int tl = tid & 63, ti = i0 + (tl >> 4), tj = j0 + (tl & 15);
  if (ti >= Hi || tj >= Wi) return;
  const int rs = up_first_row(ti, Hi, H) - rlo, cs = up_first_row(tj, Wi, W) - clo;  // first candidates, inside the region
  float wr[5], wc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const int rr = rs + t, cc = cs + t;
    wr[t] = wc[t] = 0.f;
    if (rr < kUR && s_ra[rr] >= 0) wr[t] = (s_ra[rr] == ti ? 1.f - s_rf[rr] : 0.f) + (s_rb[rr] == ti ? s_rf[rr] : 0.f);
    if (cc < kUC && s_ca[cc] >= 0) wc[t] = (s_ca[cc] == tj ? 1.f - s_cf[cc] : 0.f) + (s_cb[cc] == tj ? s_cf[cc] : 0.f);
  }
  const size_t tex = (size_t)b * Ca * Hi * Wi + (unsigned)ti * (unsigned)Wi + (unsigned)tj;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int cil = (tid >> 6) + 4 * u;
    if (cig0 + cil >= Ca) continue;
    const float* src = s_gu + cil * (kUR * kUC);
    float sum = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      float rowsum = 0.f;
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int rr = min(rs + a, kUR - 1), cc = min(cs + c, kUC - 1);  // (a clamped candidate has weight 0)
        rowsum += wc[c] * src[rr * kUC + cc];
      }
      sum += wr[a] * rowsum;
    }
    const size_t o = tex + (size_t)(cig0 + cil) * Hi * Wi;
    pgx[o] = pxa[o] > 0.f ? sum : sum * p.leak;  // the leaky's adjoint; at xa == 0 it takes leak, as torch
  }
}

// ---- gradient of xb --------------------------------------------------------------------------------------------------
// grid (tiles of 8 x 32 pixels, B, groups of 16 CT channels of xb); KC = output channels per K stage (4 for Co <= 4)
template <int CT, int KC>
__global__ __launch_bounds__(256) void uc_bwd_xb_kernel(const UcDims p, const float* __restrict__ pw,
                                                        const float* __restrict__ py, const float* __restrict__ pg,
                                                        float* __restrict__ pgx) {
  __shared__ float s_g[KC * kFwdPlane];
  __shared__ float s_w[9 * KC * 16 * CT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, Ca = p.Ca, Cb = p.Cb, Co = p.Co, Ct = Ca + Cb;
  const int ntx = (W + kTW - 1) / kTW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int r0 = ty * kTH, c0 = tx * kTW, b = blockIdx.y, cbg0 = blockIdx.z * (16 * CT);
  const size_t HW = (size_t)H * W;
  int poff[4], prow[4], pcol[4];
  uc_tile_pixels(wave, j, poff, prow, pcol);
  f32x4 acc[4][CT];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* gb = pg + (size_t)b * Co * HW;
  const float* yb = p.act ? py + (size_t)b * Co * HW : nullptr;
  for (int co0 = 0; co0 < Co; co0 += KC) {
    __syncthreads();
    uc_stage_gpre<KC, kHR, kHC, kFwdPlane>(s_g, p, gb, yb, co0, r0 - 1, c0 - 1, HW, tid);
    for (int idx = tid; idx < KC * 16 * CT * 9; idx += 256) {  // A[cb][co][tap'] = w[co][Ca + cb][8 - tap']
      const int kl = idx / (16 * CT * 9), rem = idx - kl * (16 * CT * 9), col = rem / 9, tw = rem - col * 9;
      const int co = co0 + kl, cb = cbg0 + col;
      s_w[((8 - tw) * KC + kl) * (16 * CT) + col] = (co < Co && cb < Cb) ? pw[((size_t)co * Ct + Ca + cb) * 9 + tw] : 0.f;
    }
    __syncthreads();
    up_conv_core<CT, 4, KC>(s_g, kFwdPlane, kHC, s_w, poff, acc, j, g);
  }
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int r = r0 + prow[pt], c = c0 + pcol[pt];
    if (r >= H || c >= W) continue;
    const unsigned o = (unsigned)r * (unsigned)W + (unsigned)c;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int cb = cbg0 + 16 * ct + 4 * g + r4;
        if (cb < Cb) pgx[((size_t)b * Cb + cb) * HW + o] = acc[pt][ct][r4];
      }
  }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------
// grid (K blocks, (co tile, ci tile) pairs); the ci tiles: gol_cdiv(Ca, 16) of the blended half, then gol_cdiv(Cb, 16) of the
// skip.  A workgroup walks a run of consecutive 8 x 32 tiles; per tile the window of the operand [16 ci][10][34] and
// g_pre [16 co][256] are staged; wave -> 64 of the 256 pixels as 16 K slices of 4 consecutive pixels.
__global__ __launch_bounds__(256) void uc_bwd_w_kernel(const UcDims p, const float* __restrict__ pxa,
                                                       const float* __restrict__ pxb, const float* __restrict__ py,
                                                       const float* __restrict__ pg, float* __restrict__ pscratch) {
  __shared__ float s_u[16 * kBwPlane];  // (also the reduction image [9][256] at the end)
  __shared__ float s_g[16 * kBwGRow];
  __shared__ int s_ra[kHR], s_rb[kHR], s_ca[kHC], s_cb[kHC];
  __shared__ float s_rf[kHR], s_cf[kHC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, Ca = p.Ca, Cb = p.Cb, Co = p.Co;
  const int nca = (Ca + 15) >> 4, nci = nca + ((Cb + 15) >> 4);
  const int cot = blockIdx.y / nci, cit = blockIdx.y - cot * nci, co0 = cot * 16;
  const bool blended = cit < nca;  // workgroup-uniform
  const int ci0 = blended ? cit * 16 : (cit - nca) * 16;
  const int ntx = (W + kTW - 1) / kTW, nty = (H + kTH - 1) / kTH, ntiles = p.B * nty * ntx;
  const size_t HWi = (size_t)p.Hi * p.Wi, HW = (size_t)H * W;
  f32x4 acc[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) acc[tap] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int per = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t0 = min((int)blockIdx.x * per, ntiles), t1 = min(t0 + per, ntiles);
  for (int tile = t0; tile < t1; ++tile) {
    const int b = tile / (nty * ntx), rem = tile - b * (nty * ntx), ty = rem / ntx, tx = rem - ty * ntx;
    const int r0 = ty * kTH, c0 = tx * kTW;
    __syncthreads();  // the previous tile's operands and tables have been consumed
    if (blended) {
      up_fill_axis(s_ra, s_rb, s_rf, kHR, r0 - 1, p.Hi, H, p.Wi, tid);
      up_fill_axis(s_ca, s_cb, s_cf, kHC, c0 - 1, p.Wi, W, 1, tid);
    }
    {  // thread -> one pixel of the tile, all 16 channels; unconditional clamped loads, all in flight together
      const int r = r0 + (tid >> 5), c = c0 + (tid & 31);
      const bool in = r < H && c < W;
      const unsigned o = in ? (unsigned)r * (unsigned)W + (unsigned)c : 0u;
      float vg[16], vy[16];
#pragma unroll
      for (int cl = 0; cl < 16; ++cl) {
        const size_t oo = ((size_t)b * Co + min(co0 + cl, Co - 1)) * HW + o;
        vg[cl] = pg[oo];
        vy[cl] = p.act ? py[oo] : 0.f;
      }
#pragma unroll
      for (int cl = 0; cl < 16; ++cl) s_g[cl * kBwGRow + tid] = (in && co0 + cl < Co) ? uc_gpre(p, vg[cl], vy[cl]) : 0.f;
    }
    __syncthreads();
    if (blended)
      up_stage_u<16, kHR, kHC, kBwPlane, kBwUnroll, true>(s_u, s_ra, s_rb, s_rf, s_ca, s_cb, s_cf, pxa + (size_t)b * Ca * HWi, ci0, Ca,
                                                  HWi, tid, p.leak);
    else
      uc_stage_plain<16, kHR, kHC, kBwPlane, kBwUnroll>(s_u, pxb + (size_t)b * Cb * HW, ci0, Cb, r0 - 1, c0 - 1, H, W, HW, tid);
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const int q0 = wave * 64 + s * 4;  // 4 consecutive pixels of one row: lane group g takes pixel q0 + g
      const float a = s_g[j * kBwGRow + q0 + g];
      const float* up = s_u + j * kBwPlane + (q0 >> 5) * kHC + (q0 & 31) + g;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, up[(tap / 3) * kHC + tap % 3], acc[tap], 0, 0, 0);
    }
  }
  // D[co = 4 g + r4][ci = j]; the four waves add up in LDS in wave order, the partial [9][16 co][16 ci] goes to scratch
  __syncthreads();
  float* s_red = s_u;
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          float* sp = &s_red[tap * 256 + (4 * g + r4) * 16 + j];
          *sp = (wv == 0 ? 0.f : *sp) + acc[tap][r4];
        }
    }
    __syncthreads();
  }
  float* dst = pscratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (9 * 256) + tid;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) dst[tap * 256] = s_red[tap * 256 + tid];
}

// ---- bias gradient ---------------------------------------------------------------------------------------------------
// out[n] = sum_b g_pre[b,n] over the Co H W plane elements
__global__ __launch_bounds__(256) void uc_bwd_s_kernel(const UcDims p, size_t N, const float* __restrict__ py,
                                                       const float* __restrict__ pg, float* __restrict__ pout) {
  const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int b = 0; b < p.B; ++b) s += uc_gpre(p, pg[(size_t)b * N + n], p.act ? py[(size_t)b * N + n] : 0.f);
  pout[n] = s;
}

int check_common(int B, int Ca, int Cb, int Co, int Hi, int Wi, int act) {
  GOL_REQUIRE(B >= 0 && Ca >= 0 && Cb >= 0 && Co > 0 && Hi > 0 && Wi > 0, "bad sizes");
  GOL_REQUIRE(act == 0 || act == 1, "act must be 0 (bias) or 1 (bias + tanh + affine)");
  if (Ca < 8 || Ca % 8 != 0 || Cb < 8 || Cb % 8 != 0 || !(Co % 8 == 0 || Co <= 4) || B > 65535) {
    gol_set_error("gol_upcat_conv: Ca and Cb must be positive multiples of 8, Co a multiple of 8 or 1..4, B <= 65535 "
                  "(got %d + %d -> %d, B = %d)", Ca, Cb, Co, B);
    return GOL_ERR_UNSUPPORTED;
  }
  // 32-bit offsets inside a plane; grid limits
  GOL_REQUIRE((long long)Hi * Wi <= (1ll << 26), "plane too large");
  GOL_REQUIRE((long long)gol_cdiv(Co, 16) * (gol_cdiv(Ca, 16) + gol_cdiv(Cb, 16)) <= 65535, "too many channel tiles");
  GOL_REQUIRE((long long)B * gol_cdiv(2 * Hi, kTH) * gol_cdiv(2 * Wi, kTW) < (1ll << 31), "too many tiles");
  GOL_REQUIRE((long long)Co * Hi * Wi * 4 / 256 < (1ll << 31), "layer too large");
  return GOL_OK;
}

int bwd_w_groups(int Ca, int Cb, int Co) { return gol_cdiv(Co, 16) * (gol_cdiv(Ca, 16) + gol_cdiv(Cb, 16)); }

int bwd_w_blocks(int B, int Ca, int Cb, int Co, int Hi, int Wi) {
  return up_bwd_w_blocks((long long)B * gol_cdiv(2 * Hi, kTH) * gol_cdiv(2 * Wi, kTW), bwd_w_groups(Ca, Cb, Co));
}

UcDims make_dims(int B, int Ca, int Cb, int Co, int Hi, int Wi, int act, float leak, float scale, float shift) {
  return UcDims{B, Ca, Cb, Co, Hi, Wi, 2 * Hi, 2 * Wi, act, leak, scale, shift, scale != 0.f ? 1.f / scale : 0.f};
}

template <int ACT>
void launch_fwd(const UcDims& p, const float* xa, const float* xb, const float* w, const float* bias, float* y,
                hipStream_t s) {
  const int tiles = gol_cdiv(p.H, kTH) * gol_cdiv(p.W, kTW);
  if (p.Co <= 16) uc_fwd_kernel<1, ACT><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, xa, xb, w, bias, y);
  else if (p.Co <= 32) uc_fwd_kernel<2, ACT><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, xa, xb, w, bias, y);
  else uc_fwd_kernel<4, ACT><<<dim3(tiles, p.B, gol_cdiv(p.Co, 64)), 256, 0, s>>>(p, xa, xb, w, bias, y);
}

template <int KC>
void launch_bwd_xb(const UcDims& p, const float* w, const float* y, const float* g, float* gx, hipStream_t s) {
  const int tiles = gol_cdiv(p.H, kTH) * gol_cdiv(p.W, kTW);
  if (p.Cb <= 16) uc_bwd_xb_kernel<1, KC><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, w, y, g, gx);
  else if (p.Cb <= 32) uc_bwd_xb_kernel<2, KC><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, w, y, g, gx);
  else uc_bwd_xb_kernel<4, KC><<<dim3(tiles, p.B, gol_cdiv(p.Cb, 64)), 256, 0, s>>>(p, w, y, g, gx);
}

}  // namespace

extern "C" int gol_upcat_conv_fwd(int B, int Ca, int Cb, int Co, int Hi, int Wi, int act, float leak, float out_scale,
                                  float out_shift, const float* xa, const float* xb, const float* w_eff, const float* bias,
                                  float* y, void* stream) {
  const int rc = check_common(B, Ca, Cb, Co, Hi, Wi, act);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(xa && xb && w_eff && bias && y, "null pointer");
  const UcDims p = make_dims(B, Ca, Cb, Co, Hi, Wi, act, leak, out_scale, out_shift);
  hipStream_t s = (hipStream_t)stream;
  if (act == 0) launch_fwd<0>(p, xa, xb, w_eff, bias, y, s);
  else launch_fwd<1>(p, xa, xb, w_eff, bias, y, s);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" long long gol_upcat_conv_bwd_scratch_floats(int B, int Ca, int Cb, int Co, int Hi, int Wi) {
  if (B <= 0 || Ca <= 0 || Cb <= 0 || Co <= 0 || Hi <= 0 || Wi <= 0) return 0;
  return (long long)bwd_w_groups(Ca, Cb, Co) * bwd_w_blocks(B, Ca, Cb, Co, Hi, Wi) * 9 * 256;
}

extern "C" int gol_upcat_conv_bwd(int B, int Ca, int Cb, int Co, int Hi, int Wi, int act, float leak, float out_scale,
                                  float out_shift, const float* xa, const float* xb, const float* w_eff, const float* y,
                                  const float* g_y, float* g_xa, float* g_xb, float* g_w, float* g_bias, float* scratch,
                                  void* stream) {
  const int rc = check_common(B, Ca, Cb, Co, Hi, Wi, act);
  if (rc != GOL_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int H = 2 * Hi, W = 2 * Wi;
  if (B == 0) {  // empty sums
    if (g_w && hipMemsetAsync(g_w, 0, sizeof(float) * 9 * (Ca + Cb) * Co, s) != hipSuccess) return GOL_ERR_LAUNCH;
    if (g_bias && hipMemsetAsync(g_bias, 0, sizeof(float) * Co * H * W, s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  if (!(g_xa || g_xb || g_w || g_bias)) return GOL_OK;
  GOL_REQUIRE(g_y, "null pointer");
  GOL_REQUIRE(act == 0 || y, "act 1 needs y (the tanh is recovered from it)");
  GOL_REQUIRE(!(g_xa || g_xb) || w_eff, "g_xa and g_xb need w_eff");
  GOL_REQUIRE(!g_xa || xa, "g_xa needs xa (the leaky mask)");
  GOL_REQUIRE(!g_w || (xa && xb && scratch), "g_w needs xa, xb and scratch");
  const UcDims p = make_dims(B, Ca, Cb, Co, Hi, Wi, act, leak, out_scale, out_shift);
  if (g_xa) {
    const int tiles = gol_cdiv(Hi, kSH) * gol_cdiv(Wi, kSW);
    if (Co <= 4) uc_bwd_xa_kernel<4><<<dim3(tiles, B, gol_cdiv(Ca, 16)), 256, 0, s>>>(p, xa, w_eff, y, g_y, g_xa);
    else uc_bwd_xa_kernel<8><<<dim3(tiles, B, gol_cdiv(Ca, 16)), 256, 0, s>>>(p, xa, w_eff, y, g_y, g_xa);
    GOL_CHECK_LAUNCH();
  }
  if (g_xb) {
    if (Co <= 4) launch_bwd_xb<4>(p, w_eff, y, g_y, g_xb, s);
    else launch_bwd_xb<8>(p, w_eff, y, g_y, g_xb, s);
    GOL_CHECK_LAUNCH();
  }
  if (g_w) {
    const int groups = bwd_w_groups(Ca, Cb, Co), nblk = bwd_w_blocks(B, Ca, Cb, Co, Hi, Wi);
    const int nca = gol_cdiv(Ca, 16), nci = nca + gol_cdiv(Cb, 16);
    uc_bwd_w_kernel<<<dim3(nblk, groups), 256, 0, s>>>(p, xa, xb, y, g_y, scratch);
    GOL_CHECK_LAUNCH();
    up_bwd_w_reduce_kernel<<<dim3(9 * 16, groups), 256, 0, s>>>(Co, Ca + Cb, Ca, nca, nci, nblk, scratch, g_w);
    GOL_CHECK_LAUNCH();
  }
  if (g_bias) {
    const size_t N = (size_t)Co * H * W;
    uc_bwd_s_kernel<<<dim3(gol_cdiv((long long)N, 256)), 256, 0, s>>>(p, N, y, g_y, g_bias);
    GOL_CHECK_LAUNCH();
  }
  return GOL_OK;
}
