// encconv.hip -- one encoder layer as one operator, forward and backward, gfx950.
//
// The reference's texture encoder stacks eight Conv2dWNUB(Ci -> Co, k4 s2 p1) + untied bias + LeakyReLU
// (/root/reference/ca_code/models/rgca.py:281-298; ca_code/nn/layers.py:276-328,472,157-244) behind `color / 255.0 - 0.5`
// (rgca.py:314):
//     xin[b,ci,r,c] = in_scale x[b,ci,r,c] + in_shift inside the image, 0 outside (the pad comes after the affine)
//     y[b,co,Y,X]   = lrelu( sum_{ci,ky,kx} xin[b,ci,2Y-1+ky,2X-1+kx] W[co,ci,ky,kx] + bias[co,Y,X] )
// run there as a MIOpen convolution, an ATen add and an ATen leaky_relu (and five kernels backward).  The convolution is the
// exact adjoint of trunk.hip's transposed one (tests/test_gpu_conv4s2_adjoint.py), so the three formulations of
// gol_conv4s2.h are taken with the roles exchanged (fine grid = x, coarse grid = y):
//   fwd     row gather, reduction over ci in K stages of 4 (Ci = 1..4: the stage's missing channels are ZERO WEIGHTS, and
//           no channel of x that does not exist is read); the affine is applied to the loaded values, bias + LeakyReLU
//           to the accumulators; nothing but y is written.
//   bwd     g_pre = g_y (y > 0 ? 1 : leak) is formed while loading (leak > 0 keeps the sign, so y carries the mask):
//     bwd_x   quad form, reduction over co in K stages of 8.  W is taken in the forward's layout [Co,Ci,4,4] (reduction
//             channel first: no permuted copy is needed);
//     bwd_w   weight gradient with x and g in each other's role: per (16 co x 16 ci) tile pair, g_pre[16 NCO][64] is the
//             coarse side and xin [16 ci] the window, up to four co tiles sharing a staged window (Ci = 1..4: B columns =
//             (ci, dx), a quarter of the MFMAs, see enc_bwd_w_kernel);
//     bwd_b   g_bias[co,Y,X] = sum_b g_pre, one streaming pass.
#include "gol_conv4s2.h"

namespace {

struct EncDims {
  int B, Ci, Co, H, W;  // x [B,Ci,H,W] -> y [B,Co,H/2,W/2]
  float leak, in_scale, in_shift;
};

constexpr int kFwdKC = 4;  // input channels per K stage of the forward (Ci is a multiple of 8, or 1..4 zero-padded to 4)
constexpr int kBxKC = 8;   // output channels per K stage of the input gradient (Co is a multiple of 16)

// ---- forward ---------------------------------------------------------------------------------------------------------
// grid (B, tiles of 64 output pixels, groups of 16 CT output channels): the B views of a spatial tile are neighbours in
// dispatch order, so the bias tile is fetched from memory once and served from L2 to the others.
// One wave = 16 output pixels (linear over the H/2 x W/2 grid) x 16 CT channels, two accumulators per channel tile
// (even / odd kx).  Lane (pixel j, row g) holds xin[ci][2Y-1+g][2X-1+kx], kx = 0..3: four consecutive floats of one row
// -- ONE 16-byte load (4-byte aligned).  At the left / right border the load starts one column late / early (it never
// leaves the row) and the values shift by one (WIDE; rows of fewer than 4 floats, W = 2, take clamped scalar loads).
// MFMA operands: A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15], D[i = 4 (lane >> 4) + r][j].
// s_w[ci][kx][ct][channel i][ky]: the A operand of (ci, kx, ct) is 64 consecutive floats (element 4 i + k).
// (written out, not a gol_conv4s2.h helper: as row_gemm + callbacks, shared with trunk_bwd_x_kernel, the VGPR counts of
// three instances moved or the loaded block spilled: profiles/LOG.md "conv4s2")
template <int CT, bool WIDE>
__global__ __launch_bounds__(256) void enc_fwd_kernel(const EncDims p, const float* __restrict__ px,
                                                      const float* __restrict__ pw, const float* __restrict__ pbias,
                                                      float* __restrict__ py) {
  __shared__ __attribute__((aligned(16))) float s_w[kFwdKC * 4 * CT * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, cog0 = blockIdx.z * (16 * CT);
  const int H = p.H, W = p.W, Ci = p.Ci, Co = p.Co;
  const int Wo = W >> 1, HWo = (H >> 1) * Wo;
  const size_t HWi = (size_t)H * W;
  const int pix = (blockIdx.y * 4 + wave) * 16 + j;
  const bool pv = pix < HWo;
  const int Y = pv ? pix / Wo : 0, X = pv ? pix - Y * Wo : 0;
  const int r = 2 * Y - 1 + g, c0 = 2 * X - 1;
  const bool rv = pv && r >= 0 && r < H;
  const unsigned rowb = rv ? (unsigned)r * (unsigned)W : 0u;
  // byte offsets inside a plane (planes hold < 2^26 floats): uniform plane pointer + 32-bit lane offset
  const int s0 = WIDE ? min(max(c0, 0), W - 4) : 0;  // first column of the 16-byte load
  const int shift = c0 - s0;                          // WIDE: -1 (X = 0), 0, +1 (X = W/2 - 1)
  unsigned coff[4];
  bool cv[4];
#pragma unroll
  for (int kx = 0; kx < 4; ++kx) {
    cv[kx] = rv && c0 + kx >= 0 && c0 + kx < W;
    coff[kx] = 4u * (rowb + (unsigned)(WIDE ? s0 : min(max(c0 + kx, 0), W - 1)));
  }
  const float* xb = px + (size_t)b * Ci * HWi;
  const float in_scale = p.in_scale, in_shift = p.in_shift;

  float4 wr[CT];
  float rx[kFwdKC * 4];
  auto issue = [&](int ci0) {
#pragma unroll
    for (int u = 0; u < CT; ++u) {  // stage = 16 CT output channels x (4 ci x 4 ky) float4, 64 consecutive floats per co
      const int f = tid + 256 * u, co = cog0 + (f >> 4), ci = ci0 + ((f >> 2) & 3);
      const bool ok = co < Co && ci < Ci;  // a channel group can overhang Co; a stage can overhang Ci = 1..4
      const float4 v = *reinterpret_cast<const float4*>(pw + ((size_t)(ok ? co : 0) * Ci + (ok ? ci : 0)) * 16 + (f & 3) * 4);
      wr[u] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int cl = 0; cl < kFwdKC; ++cl) {
      const float* xpl = gol_uniform(xb + (size_t)min(ci0 + cl, Ci - 1) * HWi);  // (never a plane past Ci)
      if constexpr (WIDE) {
        const f32x4u xv = *reinterpret_cast<const f32x4u*>(gol_at(xpl, coff[0]));
#pragma unroll
        for (int t = 0; t < 4; ++t) rx[cl * 4 + t] = xv[t];
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) rx[cl * 4 + t] = *gol_at(xpl, coff[t]);
      }
    }
  };
  f32x4 acc[CT][2];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct][0] = acc[ct][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  issue(0);
  for (int ci0 = 0; ci0 < Ci; ci0 += kFwdKC) {
    __syncthreads();  // the previous stage's weights have been consumed
    float xin[kFwdKC * 4];  // [ci][kx]
#pragma unroll
    for (int cl = 0; cl < kFwdKC; ++cl) {
      const bool chv = ci0 + cl < Ci;
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        float v = rx[cl * 4 + kx];
        if constexpr (WIDE)
          v = shift == 0 ? rx[cl * 4 + kx] : (shift > 0 ? rx[cl * 4 + min(kx + 1, 3)] : rx[cl * 4 + max(kx - 1, 0)]);
        xin[cl * 4 + kx] = (cv[kx] && chv) ? fmaf(in_scale, v, in_shift) : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < CT; ++u) {
      const int f = tid + 256 * u, co_l = f >> 4, ci_l = (f >> 2) & 3, ky = f & 3;
      const float v[4] = {wr[u].x, wr[u].y, wr[u].z, wr[u].w};
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) s_w[((ci_l * 4 + kx) * CT + (co_l >> 4)) * 64 + 4 * (co_l & 15) + ky] = v[kx];
    }
    __syncthreads();
    if (ci0 + kFwdKC < Ci) issue(ci0 + kFwdKC);
#pragma unroll
    for (int e = 0; e < kFwdKC * 4; ++e)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        acc[ct][e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[(e * CT + ct) * 64 + 4 * j + g], xin[e], acc[ct][e & 1],
                                                              0, 0, 0);
  }
  if (!pv) return;
  // epilogue on the accumulators: D row = channel cog0 + 16 ct + 4 g + r4, column = pixel j
  const float leak = p.leak;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int co = cog0 + 16 * ct + 4 * g + r4;
      if (co < Co) {
        const float v = acc[ct][0][r4] + acc[ct][1][r4] + pbias[(size_t)co * HWo + pix];
        py[((size_t)b * Co + co) * HWo + pix] = v > 0.f ? v : v * leak;
      }
    }
}

// ---- input gradient --------------------------------------------------------------------------------------------------
// gx[b,ci,r,c] = in_scale sum_{co,ky,kx} gpre[b,co,Y,X] W[co,ci,ky,kx], r = 2Y-1+ky, c = 2X-1+kx: the transposed
// convolution of g_pre.  The 2x2 quad {2m-1, 2m} x {2k-1, 2k} of x reads the 2x2 block {m-1, m} x {k-1, k} of g_pre and
// uses each of the 16 taps once, so every parity class (a,q) is a GEMM D[ci][quad] = A[ci][(co,tap)] B[(co,tap)][quad],
// K = the 4 taps of one co, and B is shared by the four classes.  grid (B, tiles of 64 quads, groups of 16 CT input
// channels); one wave = 16 quads (linear over the (H/2+1) x (W/2+1) quad grid) x 16 CT channels x 4 classes.
// (written out, not a gol_conv4s2.h helper: as quad_gemm + callbacks, shared with trunk_fwd_kernel, the epilogue's
// address arithmetic grew by 20-68 instructions per instance: profiles/LOG.md "conv4s2")
template <int CT>
__global__ __launch_bounds__(256) void enc_bwd_x_kernel(const EncDims p, const float* __restrict__ pw,
                                                        const float* __restrict__ py, const float* __restrict__ pg,
                                                        float* __restrict__ pgx) {
  // s_w[co][cls][ct][tap g][channel j]: the A operand of (co, cls, ct) is 64 consecutive floats, one per lane
  __shared__ __attribute__((aligned(16))) float s_w[kBxKC * 4 * CT * 64];
  constexpr int NW4 = kBxKC * CT / 4;  // float4 per thread and stage
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int ty = g >> 1, tx = g & 1;
  const int b = blockIdx.x, cig0 = blockIdx.z * (16 * CT);
  const int h = p.H >> 1, w = p.W >> 1, Ci = p.Ci, Co = p.Co;
  const int qw = w + 1, NQ = (h + 1) * qw;
  const size_t HWs = (size_t)h * w, HWi = 4 * HWs;
  const int t = (blockIdx.y * 4 + wave) * 16 + j;
  const bool qv = t < NQ;
  const int m = qv ? t / qw : 0, k = qv ? t - m * qw : 0;
  const int r = m - ty, c = k - tx;
  const bool vin = qv && r >= 0 && r < h && c >= 0 && c < w;
  const size_t boff = (size_t)b * Co * HWs + (vin ? (size_t)r * w + c : 0);
  const float* gb = pg + boff;
  const float* yb = py + boff;
  const float leak = p.leak;

  float4 wr[NW4];
  float Bg[kBxKC], By[kBxKC];
  auto issue = [&](int co0) {
#pragma unroll
    for (int u = 0; u < NW4; ++u) {
      const int f = tid + 256 * u, co_l = f / (CT * 64), rem = f - co_l * (CT * 64), ci = cig0 + (rem >> 2);
      const bool ok = ci < Ci;  // (a group of 16 or 32 channels can overhang Ci)
      const float4 v = *reinterpret_cast<const float4*>(pw + ((size_t)(co0 + co_l) * Ci + (ok ? ci : 0)) * 16 + (rem & 3) * 4);
      wr[u] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int cl = 0; cl < kBxKC; ++cl) {
      Bg[cl] = gb[(size_t)(co0 + cl) * HWs];
      By[cl] = yb[(size_t)(co0 + cl) * HWs];
    }
  };
  f32x4 acc[CT][4];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int cls = 0; cls < 4; ++cls) acc[ct][cls] = f32x4{0.f, 0.f, 0.f, 0.f};
  issue(0);
  for (int co0 = 0; co0 < Co; co0 += kBxKC) {
    __syncthreads();  // the previous stage's weights have been consumed
    float Bc[kBxKC];
#pragma unroll
    for (int cl = 0; cl < kBxKC; ++cl) Bc[cl] = vin ? Bg[cl] * (By[cl] > 0.f ? 1.f : leak) : 0.f;
#pragma unroll
    for (int u = 0; u < NW4; ++u) {
      const int f = tid + 256 * u, co_l = f / (CT * 64), rem = f - co_l * (CT * 64), ci_l = rem >> 2, ky = rem & 3;
      const float v[4] = {wr[u].x, wr[u].y, wr[u].z, wr[u].w};
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {  // tap (ky,kx) = (a + 2 ty, q + 2 tx)
        const int cls = 2 * (ky & 1) + (kx & 1), gg = 2 * (ky >> 1) + (kx >> 1);
        s_w[((co_l * 4 + cls) * CT + (ci_l >> 4)) * 64 + gg * 16 + (ci_l & 15)] = v[kx];
      }
    }
    __syncthreads();
    if (co0 + kBxKC < Co) issue(co0 + kBxKC);
#pragma unroll
    for (int cl = 0; cl < kBxKC; ++cl)
#pragma unroll
      for (int cls = 0; cls < 4; ++cls)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          acc[ct][cls] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[((cl * 4 + cls) * CT + ct) * 64 + lane], Bc[cl],
                                                              acc[ct][cls], 0, 0, 0);
  }
  // D row = channel cig0 + 16 ct + 4 g + r4, column = quad j
  const float in_scale = p.in_scale;
  float* gxb = pgx + (size_t)b * Ci * HWi;
#pragma unroll
  for (int cls = 0; cls < 4; ++cls) {
    const int oy = 2 * m - 1 + (cls >> 1), ox = 2 * k - 1 + (cls & 1);
    if (!(qv && oy >= 0 && oy < 2 * h && ox >= 0 && ox < 2 * w)) continue;  // half-empty border quads
    const size_t o = (size_t)oy * (2 * w) + ox;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int ci = cig0 + 16 * ct + 4 * g + r4;
        if (ci < Ci) gxb[(size_t)ci * HWi + o] = in_scale * acc[ct][cls][r4];
      }
  }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------
// gw[co,ci,ky,kx] = sum_{b,Y,X} gpre[b,co,Y,X] xin[b,ci,2Y-1+ky,2X-1+kx].  grid (K blocks, groups of NCO co tiles x ci
// tiles).  A workgroup walks tiles of one view x one output row x 64 output pixels: gpre[16 NCO][64] and the matching xin
// window [16 ci][4 rows][130 cols] are staged in LDS; the window is shared by the NCO channel tiles (wave -> channel tile
// wave % NCO, pixel part wave / NCO), each wave feeds 16-pixel chunks to 64 MFMAs (16 taps x 4 pixels per instruction);
// the waves' sums meet in LDS and leave as one partial [16 taps][16 co][16 ci] per channel tile.  Window planes past Ci
// (a ragged last tile) are zeros and are never loaded.
// SMALL (Ci = 1..4, the first layer): a 16-wide ci tile would carry 12 or more zero columns through every MFMA, so the B
// operand's 16 columns are (ci 0..3) x (dx 0..3) instead -- one MFMA per (row dy, pixel) covers the four dx, a quarter of
// the instructions -- and the window holds 4 planes, one per wave.
// (the loaders, the MFMA nest and the wave sum are written out: as gol_conv4s2.h helpers they changed the VGPR counts of the
// weight-gradient kernels, profiles/LOG.md "conv4s2")
template <int NCO, bool SMALL>
__global__ __launch_bounds__(256) void enc_bwd_w_kernel(const EncDims p, const float* __restrict__ px,
                                                        const float* __restrict__ py, const float* __restrict__ pg,
                                                        float* __restrict__ pscratch) {
  constexpr int NP = 4 / NCO;  // waves that share a channel tile split the tile's 64 pixels
  constexpr int XPL = SMALL ? 4 : 16;   // window planes
  constexpr int NSEG = XPL;             // (plane, row) segments of the window per wave
  constexpr int kMem = XPL * kWinPlane + NCO * 16 * kPixRow;
  __shared__ __attribute__((aligned(16))) float s_mem[kMem > 16 * 256 ? kMem : 16 * 256];  // (the reduction image below)
  float* s_x = s_mem;
  float* s_g = s_mem + XPL * kWinPlane;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
  const int col = wave % NCO, part = wave / NCO;
  const int H = p.H, W = p.W, h = H >> 1, w = W >> 1, Ci = p.Ci, Co = p.Co;
  const int nci = (Ci + 15) >> 4, cog = blockIdx.y / nci, cit = blockIdx.y - cog * nci;
  const int co0 = cog * (NCO * 16), ci0 = cit * 16;
  const size_t HWs = (size_t)h * w, HWi = (size_t)H * W;
  const float leak = p.leak, in_scale = p.in_scale, in_shift = p.in_shift;
  f32x4 acc[4][4];
#pragma unroll
  for (int dy = 0; dy < 4; ++dy)
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) acc[dy][dx] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tpr = (w + kWTile - 1) / kWTile, ntiles = p.B * h * tpr;
  // Staging is software-pipelined as in trunk_bwd_w_kernel: the global loads of the NEXT tile are issued (into
  // registers, all independent) before the MFMA phase of the current one.
  //   x:    wave -> NSEG of the 4 NSEG (plane, row) segments, columns [0,128) as two 64-lane loads; the 2 leftover columns
  //         of the segments go to threads 0..8 NSEG - 1;  g, y: thread -> (4 NCO channels, 1 pixel)
  float rx[2 * NSEG], rlx, rg[4 * NCO], ry[4 * NCO];
  const int lseg = (tid >> 1) & (4 * NSEG - 1), lcl = 2 * kWTile + (tid & 1);
  auto issue = [&](int tile) {
    const int b = tile / (h * tpr), rem = tile - b * (h * tpr), iy = rem / tpr, ix0 = (rem - iy * tpr) * kWTile;
    const size_t so = ((size_t)b * Co + min(co0 + wave, Co - 1)) * HWs + (size_t)iy * w + min(ix0 + lane, w - 1);
#pragma unroll
    for (int u = 0; u < 4 * NCO; ++u) {
      const size_t o = so + (co0 + wave + 4 * u < Co ? (size_t)(4 * u) * HWs : 0);
      rg[u] = pg[o];
      ry[u] = py[o];
    }
    // one scalar base + 32-bit byte offsets inside the 16-plane slab (planes hold < 2^26 floats)
    const float* xs = gol_uniform(px + ((size_t)b * Ci + ci0) * HWi);
#pragma unroll
    for (int sgm = 0; sgm < NSEG; ++sgm) {
      const int seg = wave * NSEG + sgm, pl = seg >> 2, oy = min(max(2 * iy - 1 + (seg & 3), 0), H - 1);
      const unsigned rowb = (unsigned)pl * (unsigned)HWi + (unsigned)oy * (unsigned)W;
      if (ci0 + pl < Ci) {  // wave-uniform
#pragma unroll
        for (int u = 0; u < 2; ++u)
          rx[2 * sgm + u] = *gol_at(xs, 4u * (rowb + (unsigned)min(max(2 * ix0 - 1 + lane + 64 * u, 0), W - 1)));
      } else {
        rx[2 * sgm] = rx[2 * sgm + 1] = 0.f;
      }
    }
    {
      const int pl = min(lseg >> 2, Ci - 1 - ci0);  // (the value of a plane past Ci is dropped in stage())
      const int oy = min(max(2 * iy - 1 + (lseg & 3), 0), H - 1), cc = min(max(2 * ix0 - 1 + lcl, 0), W - 1);
      rlx = *gol_at(xs, 4u * ((unsigned)pl * (unsigned)HWi + (unsigned)oy * (unsigned)W + (unsigned)cc));
    }
  };
  auto stage = [&](int tile) {  // registers -> LDS: g_pre = g (y > 0 ? 1 : leak), xin = affine(x), out of range as zeros
    const int b = tile / (h * tpr), rem = tile - b * (h * tpr), iy = rem / tpr, ix0 = (rem - iy * tpr) * kWTile;
    // (channels past Co hold a copy of a valid row: they only reach accumulator rows that the reduce kernel drops)
    const bool gv = ix0 + lane < w;
#pragma unroll
    for (int u = 0; u < 4 * NCO; ++u) s_g[(wave + 4 * u) * kPixRow + lane] = gv ? rg[u] * (ry[u] > 0.f ? 1.f : leak) : 0.f;
#pragma unroll
    for (int sgm = 0; sgm < NSEG; ++sgm) {
      const int seg = wave * NSEG + sgm, pl = seg >> 2, dy = seg & 3, oy = 2 * iy - 1 + dy;
      const bool rv = oy >= 0 && oy < H && ci0 + pl < Ci;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int cl = lane + 64 * u, cc = 2 * ix0 - 1 + cl;
        s_x[pl * kWinPlane + dy * kWinRow + cl] = (rv && cc >= 0 && cc < W) ? fmaf(in_scale, rx[2 * sgm + u], in_shift) : 0.f;
      }
    }
    if (tid < 8 * NSEG) {
      const int pl = lseg >> 2, dy = lseg & 3, oy = 2 * iy - 1 + dy, cc = 2 * ix0 - 1 + lcl;
      s_x[pl * kWinPlane + dy * kWinRow + lcl] =
          (oy >= 0 && oy < H && ci0 + pl < Ci && cc < W) ? fmaf(in_scale, rlx, in_shift) : 0.f;
    }
  };
  // A workgroup takes a run of consecutive tiles (consecutive output rows re-read two of their four window rows), and the
  // workgroups that share an L2 (blockIdx.x % 8 labels the XCD group) take neighbouring runs.
  const int nb = gridDim.x, per = (ntiles + nb - 1) / nb;
  const int vb = nb % 8 == 0 ? (int)(blockIdx.x % 8) * (nb / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int t0 = min(vb * per, ntiles), t1 = min(t0 + per, ntiles);
  if (t0 < t1) issue(t0);
  for (int tile = t0; tile < t1; ++tile) {
    __syncthreads();  // the previous tile's operands have been consumed
    stage(tile);
    __syncthreads();
    if (tile + 1 < t1) issue(tile + 1);
#pragma unroll
    for (int c = 0; c < NCO; ++c) {
      const int xl = (part * NCO + c) * 16 + 4 * kq;  // this lane's 4 output pixels (K slice) inside the tile
      const float4 ga4 = *reinterpret_cast<const float4*>(&s_g[(col * 16 + l15) * kPixRow + xl]);
      const float ga[4] = {ga4.x, ga4.y, ga4.z, ga4.w};
      if constexpr (SMALL) {  // B column l15 = (ci l15 >> 2, dx l15 & 3): acc[dy][0] is D[co][(ci, dx)]
        const float* xp = &s_x[(l15 >> 2) * kWinPlane + 2 * xl + (l15 & 3)];
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[dy][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[t], xp[dy * kWinRow + 2 * t], acc[dy][0], 0, 0, 0);
        continue;
      }
#pragma unroll
      for (int dy = 0; dy < 4; ++dy) {
        const float* xp = &s_x[l15 * kWinPlane + dy * kWinRow + 2 * xl];  // column 0 of s_x is global column 2 ix0 - 1
        float xv[10];
#pragma unroll
        for (int q = 0; q < 10; q += 2) {
          const float2 t2 = *reinterpret_cast<const float2*>(xp + q);
          xv[q] = t2.x; xv[q + 1] = t2.y;
        }
#pragma unroll
        for (int dx = 0; dx < 4; ++dx)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[dy][dx] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[t], xv[2 * t + dx], acc[dy][dx], 0, 0, 0);
      }
    }
  }
  // D[i = co][j = ci]: lane holds column l15, rows 4 kq + r.  Per channel tile, its NP waves add up in LDS in wave
  // order, then the tile's partial [16 taps][16 co][16 ci] leaves: scratch is [group][NCO][K block][16 taps][256].
  __syncthreads();
  float (*s_red)[256] = reinterpret_cast<float (*)[256]>(s_mem);
  for (int c = 0; c < NCO; ++c) {
    for (int pt = 0; pt < NP; ++pt) {
      if (col == c && part == pt) {
        if constexpr (SMALL) {  // (columns ci >= 4 of the image stay unwritten: the reduce kernel drops them)
#pragma unroll
          for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float* sp = &s_red[dy * 4 + (l15 & 3)][(kq * 4 + r) * 16 + (l15 >> 2)];
              *sp = (pt == 0 ? 0.f : *sp) + acc[dy][0][r];
            }
        } else {
#pragma unroll
          for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int dx = 0; dx < 4; ++dx)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                float* sp = &s_red[dy * 4 + dx][(kq * 4 + r) * 16 + l15];
                *sp = (pt == 0 ? 0.f : *sp) + acc[dy][dx][r];
              }
        }
      }
      __syncthreads();
    }
    float* dst = pscratch + ((((size_t)blockIdx.y * NCO + c) * gridDim.x + blockIdx.x) * 16) * 256 + tid;
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) dst[(size_t)tap * 256] = s_red[tap][tid];
    __syncthreads();
  }
}

// gw[co,ci,tap] = sum over the K blocks (written once).  grid (16 taps x 16 co rows, channel tiles)
__global__ __launch_bounds__(256) void enc_bwd_w_reduce_kernel(const EncDims p, int NCO, int nblk,
                                                               const float* __restrict__ scratch,
                                                               float* __restrict__ gw) {
  const int tap = blockIdx.x >> 4, row = blockIdx.x & 15, cl = threadIdx.x & 15;
  const int nci = (p.Ci + 15) >> 4, grp = blockIdx.y / NCO, c = blockIdx.y - grp * NCO;
  const int cog = grp / nci, cit = grp - cog * nci;
  const int co = (cog * NCO + c) * 16 + row, ci = cit * 16 + cl;
  if (co >= p.Co) return;  // block-uniform: a tile past the end of the last group
  wgrad_reduce16(scratch + (((size_t)blockIdx.y * nblk) * 16 + tap) * 256 + row * 16 + cl, nblk,
                 gw + ((size_t)co * p.Ci + ci) * 16 + tap, ci < p.Ci);  // (columns past Ci: Ci = 1..4 or a ragged last tile)
}

// ---- bias gradient: over the Co * H/2 * W/2 plane elements, four per thread --------------------------------------------
__global__ __launch_bounds__(256) void enc_bwd_b_kernel(const EncDims p, const float* __restrict__ py,
                                                        const float* __restrict__ pg, float* __restrict__ pgb) {
  lrelu_bias_grad((size_t)(p.Co >> 2) * (p.H >> 1) * (p.W >> 1), p.B, p.leak, py, pg, pgb);
}

int check_common(int B, int Ci, int Co, int H, int W, float leak) {
  GOL_REQUIRE(B >= 0 && Ci > 0 && Co > 0 && H > 0 && W > 0, "bad sizes");
  GOL_REQUIRE(leak > 0.f, "leak must be positive (the backward reads the activation mask from the sign of y)");
  if (Co % 16 != 0 || !(Ci % 8 == 0 || Ci <= 4) || H % 2 != 0 || W % 2 != 0) {
    gol_set_error("gol_enc_conv: Co must be a multiple of 16, Ci a multiple of 8 or 1..4, H and W even (got %d -> %d at %d x %d)",
                  Ci, Co, H, W);
    return GOL_ERR_UNSUPPORTED;
  }
  // 32-bit byte offsets inside a 16-plane slab; grid.y / grid.z limits
  GOL_REQUIRE((long long)H * W < (1ll << 26), "plane too large");
  GOL_REQUIRE((long long)B * (H / 2) * gol_cdiv(W / 2, kWTile) < (1ll << 31), "too many row tiles");
  GOL_REQUIRE(((long long)(H / 2 + 1) * (W / 2 + 1) + 63) / 64 <= 65535, "too many pixel tiles");
  GOL_REQUIRE((long long)(Co / 16 + 3) * gol_cdiv(Ci, 16) <= 65535, "too many channel tiles");
  GOL_REQUIRE((long long)Co * (H / 2) * (W / 2) / 1024 < (1ll << 31), "layer too large");
  return GOL_OK;
}

// channel tiles of 16 co that one workgroup of the weight gradient takes (they share the staged xin window)
int bwd_w_nco(int Co) { return Co > 32 ? 4 : (Co > 16 ? 2 : 1); }
int bwd_w_groups(int Ci, int Co) { return gol_cdiv(Co, 16 * bwd_w_nco(Co)) * gol_cdiv(Ci, 16); }

// one round of the resident workgroups: 2 per CU (registers), 4 of the small-Ci variant
int bwd_w_blocks(int B, int Ci, int Co, int H, int W) {
  return wgrad_blocks((long long)B * (H / 2) * gol_cdiv(W / 2, kWTile), bwd_w_groups(Ci, Co), Ci <= 4 ? 1024 : 512);
}

}  // namespace

extern "C" int gol_enc_conv_fwd(int B, int Ci, int Co, int H, int W, float leak, float in_scale, float in_shift,
                                const float* x, const float* w_eff, const float* bias, float* y, void* stream) {
  const int rc = check_common(B, Ci, Co, H, W, leak);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && w_eff && bias && y, "null pointer");
  GOL_REQUIRE(gol_aligned16(w_eff), "w_eff must be 16-byte aligned");
  const EncDims p{B, Ci, Co, H, W, leak, in_scale, in_shift};
  hipStream_t s = (hipStream_t)stream;
  const int tiles = gol_cdiv((long long)(H / 2) * (W / 2), 64);
#define ENC_FWD(CT)                                                                                     \
  do {                                                                                                  \
    const dim3 grid(B, tiles, gol_cdiv(Co, 16 * CT));                                                   \
    if (W >= 4) enc_fwd_kernel<CT, true><<<grid, 256, 0, s>>>(p, x, w_eff, bias, y);                    \
    else enc_fwd_kernel<CT, false><<<grid, 256, 0, s>>>(p, x, w_eff, bias, y);                          \
  } while (0)
  if (Co <= 16) ENC_FWD(1);
  else if (Co <= 32) ENC_FWD(2);
  else ENC_FWD(4);
#undef ENC_FWD
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" long long gol_enc_conv_bwd_scratch_floats(int B, int Ci, int Co, int H, int W) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0 || Co % 16 != 0 || H % 2 != 0 || W % 2 != 0) return 0;
  return (long long)bwd_w_groups(Ci, Co) * bwd_w_nco(Co) * bwd_w_blocks(B, Ci, Co, H, W) * 16 * 256;
}

extern "C" int gol_enc_conv_bwd(int B, int Ci, int Co, int H, int W, float leak, float in_scale, float in_shift,
                                const float* x, const float* w_eff, const float* y, const float* g_y, float* g_x,
                                float* g_w, float* g_bias, float* scratch, void* stream) {
  const int rc = check_common(B, Ci, Co, H, W, leak);
  if (rc != GOL_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {  // empty sums
    if (g_w && hipMemsetAsync(g_w, 0, sizeof(float) * 16 * Ci * Co, s) != hipSuccess) return GOL_ERR_LAUNCH;
    if (g_bias && hipMemsetAsync(g_bias, 0, sizeof(float) * Co * (H / 2) * (W / 2), s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  GOL_REQUIRE(y && g_y, "null pointer");
  GOL_REQUIRE(!g_x || (w_eff && gol_aligned16(w_eff)), "g_x needs w_eff (16-byte aligned)");
  GOL_REQUIRE(!g_w || (x && scratch), "g_w needs x and scratch");
  GOL_REQUIRE(!g_bias || (gol_aligned16(y) && gol_aligned16(g_y) && gol_aligned16(g_bias)), "g_bias needs 16-byte aligned y, g_y, g_bias");
  const EncDims p{B, Ci, Co, H, W, leak, in_scale, in_shift};
  if (g_x) {
    const int tiles = gol_cdiv((long long)(H / 2 + 1) * (W / 2 + 1), 64);
    if (Ci <= 16) enc_bwd_x_kernel<1><<<dim3(B, tiles, 1), 256, 0, s>>>(p, w_eff, y, g_y, g_x);
    else enc_bwd_x_kernel<2><<<dim3(B, tiles, gol_cdiv(Ci, 32)), 256, 0, s>>>(p, w_eff, y, g_y, g_x);
    GOL_CHECK_LAUNCH();
  }
  if (g_w) {
    const int nco = bwd_w_nco(Co), groups = bwd_w_groups(Ci, Co), nblk = bwd_w_blocks(B, Ci, Co, H, W);
    const dim3 grid(nblk, groups);
#define ENC_BWD_W(NCO)                                                                              \
  do {                                                                                               \
    if (Ci <= 4) enc_bwd_w_kernel<NCO, true><<<grid, 256, 0, s>>>(p, x, y, g_y, scratch);            \
    else enc_bwd_w_kernel<NCO, false><<<grid, 256, 0, s>>>(p, x, y, g_y, scratch);                   \
  } while (0)
    if (nco == 1) ENC_BWD_W(1);
    else if (nco == 2) ENC_BWD_W(2);
    else ENC_BWD_W(4);
#undef ENC_BWD_W
    GOL_CHECK_LAUNCH();
    enc_bwd_w_reduce_kernel<<<dim3(256, groups * nco), 256, 0, s>>>(p, nco, nblk, scratch, g_w);
    GOL_CHECK_LAUNCH();
  }
  if (g_bias) {
    enc_bwd_b_kernel<<<dim3(gol_cdiv((long long)(Co / 4) * (H / 2) * (W / 2), 256)), 256, 0, s>>>(p, y, g_y, g_bias);
    GOL_CHECK_LAUNCH();
  }
  return GOL_OK;
}
