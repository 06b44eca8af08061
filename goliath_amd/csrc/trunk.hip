// trunk.hip -- one hidden decoder layer as one operator, forward and backward, gfx950.
//
// The reference stacks six ConvTranspose2dWNUB(Ci -> Co, k4 s2 p1) + untied bias + LeakyReLU in front of each last
// decoder layer (/root/reference/ca_code/models/rgca.py:408-426,429-454; ca_code/nn/layers.py:331-397,157-244):
//     y[b,co,Y,X] = lrelu( sum_{ci,ky,kx} x[b,ci,iy,ix] W[ci,co,ky,kx] + bias[co,Y,X] ),   Y = 2 iy - 1 + ky
// run there as a MIOpen convolution, an ATen add and an ATen leaky_relu (and five kernels backward).  Here, in the three
// formulations of gol_conv4s2.h (coarse grid = x, fine grid = y):
//   fwd     quad form, reduction over ci in K stages of 8; bias + LeakyReLU happen on the accumulators; nothing but y is
//           written.
//   bwd     g_pre = g_y (y > 0 ? 1 : leak) is formed while loading (leak > 0 keeps the sign, so y carries the mask):
//     bwd_x   row gather, reduction over co in K stages of 4, weights pre-permuted by the caller;
//     bwd_w   weight gradient per (16 ci x 16 co) tile pair, up to four ci tiles sharing a staged g_pre window;
//     bwd_b   g_bias[co,Y,X] = sum_b g_pre, one streaming pass.
#include "gol_conv4s2.h"

namespace {

struct TrunkDims {
  int B, Ci, Co, h, w;
  float leak;
};

constexpr int kFwdKC = 8;  // input channels per K stage of the forward (Ci is a multiple of 8)
constexpr int kBxKC = 4;   // output channels per K stage of the input gradient (Co is a multiple of 16)

// ---- forward ---------------------------------------------------------------------------------------------------------
// grid (B, tiles of 64 quads, groups of 16 CT output channels): the B views of a spatial tile are neighbours in
// dispatch order, so the bias tile is fetched from memory once and served from L2 to the others.
// One wave = 16 quads (linear over the (h+1) x (w+1) quad grid, so narrow layers fill their tiles) x 16 CT channels x
// 4 classes = 4 CT independent accumulators.  MFMA operands: A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15],
// D[i = 4 (lane >> 4) + r][j].
// (written out, not a gol_conv4s2.h helper: as quad_gemm + callbacks, shared with enc_bwd_x_kernel, the epilogue's
// address arithmetic grew by 20-68 instructions per instance: profiles/LOG.md "conv4s2")
template <int CT>
__global__ __launch_bounds__(256) void trunk_fwd_kernel(const TrunkDims p, const float* __restrict__ px,
                                                        const float* __restrict__ pw, const float* __restrict__ pbias,
                                                        float* __restrict__ py) {
  // s_w[ci][cls][ct][tap g][channel j]: the A operand of (ci, cls, ct) is 64 consecutive floats, one per lane
  __shared__ __attribute__((aligned(16))) float s_w[kFwdKC * 4 * CT * 64];
  constexpr int NW4 = kFwdKC * CT / 4;  // float4 per thread and stage
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int ty = g >> 1, tx = g & 1;
  const int b = blockIdx.x, cog0 = blockIdx.z * (16 * CT);
  const int h = p.h, w = p.w, Ci = p.Ci, Co = p.Co;
  const int qw = w + 1, NQ = (h + 1) * qw;
  const size_t HWi = (size_t)h * w, HWo = 4 * HWi;
  const int t = (blockIdx.y * 4 + wave) * 16 + j;
  const bool qv = t < NQ;
  const int m = qv ? t / qw : 0, k = qv ? t - m * qw : 0;
  const int r = m - ty, c = k - tx;
  const bool vin = qv && r >= 0 && r < h && c >= 0 && c < w;
  const float* xb = px + (size_t)b * Ci * HWi + (vin ? (size_t)r * w + c : 0);

  float4 wr[NW4];
  float Bn[kFwdKC];
  auto issue = [&](int ci0) {
#pragma unroll
    for (int u = 0; u < NW4; ++u) {
      const int f = tid + 256 * u, ci_l = f / (CT * 64), rem = f - ci_l * (CT * 64), co = cog0 + (rem >> 2);
      const bool ok = co < Co;  // (a group of 32 channels can overhang Co = 16 * odd)
      const float4 v = *reinterpret_cast<const float4*>(pw + ((size_t)(ci0 + ci_l) * Co + (ok ? co : 0)) * 16 + (rem & 3) * 4);
      wr[u] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int ci = 0; ci < kFwdKC; ++ci) {
      const float v = xb[(size_t)(ci0 + ci) * HWi];
      Bn[ci] = vin ? v : 0.f;
    }
  };
  f32x4 acc[CT][4];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int cls = 0; cls < 4; ++cls) acc[ct][cls] = f32x4{0.f, 0.f, 0.f, 0.f};
  issue(0);
  for (int ci0 = 0; ci0 < Ci; ci0 += kFwdKC) {
    __syncthreads();  // the previous stage's weights have been consumed
    float Bc[kFwdKC];
#pragma unroll
    for (int ci = 0; ci < kFwdKC; ++ci) Bc[ci] = Bn[ci];
#pragma unroll
    for (int u = 0; u < NW4; ++u) {
      const int f = tid + 256 * u, ci_l = f / (CT * 64), rem = f - ci_l * (CT * 64), co_l = rem >> 2, ky = rem & 3;
      const float v[4] = {wr[u].x, wr[u].y, wr[u].z, wr[u].w};
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {  // tap (ky,kx) = (a + 2 ty, q + 2 tx)
        const int cls = 2 * (ky & 1) + (kx & 1), gg = 2 * (ky >> 1) + (kx >> 1);
        s_w[((ci_l * 4 + cls) * CT + (co_l >> 4)) * 64 + gg * 16 + (co_l & 15)] = v[kx];
      }
    }
    __syncthreads();
    if (ci0 + kFwdKC < Ci) issue(ci0 + kFwdKC);
#pragma unroll
    for (int ci = 0; ci < kFwdKC; ++ci)
#pragma unroll
      for (int cls = 0; cls < 4; ++cls)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          acc[ct][cls] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[((ci * 4 + cls) * CT + ct) * 64 + lane], Bc[ci],
                                                              acc[ct][cls], 0, 0, 0);
  }
  // epilogue on the accumulators: D row = channel cog0 + 16 ct + 4 g + r4, column = quad j
  const float leak = p.leak;
  float* yb = py + (size_t)b * Co * HWo;
#pragma unroll
  for (int cls = 0; cls < 4; ++cls) {
    const int oy = 2 * m - 1 + (cls >> 1), ox = 2 * k - 1 + (cls & 1);
    if (!(qv && oy >= 0 && oy < 2 * h && ox >= 0 && ox < 2 * w)) continue;  // half-empty border quads
    const size_t o = (size_t)oy * (2 * w) + ox;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int co = cog0 + 16 * ct + 4 * g + r4;
        if (co < Co) {
          const float v = acc[ct][cls][r4] + pbias[(size_t)co * HWo + o];
          yb[(size_t)co * HWo + o] = v > 0.f ? v : v * leak;
        }
      }
  }
}

// ---- input gradient --------------------------------------------------------------------------------------------------
// gx[b,ci,iy,ix] = sum_{co,ky,kx} gpre[b,co,2iy-1+ky,2ix-1+kx] W[ci,co,ky,kx]: gather form, no atomics.  Per (co, kx) one
// MFMA with K = the four window ROWS: lane (pixel j, row g) holds gpre[co][2iy-1+g][2ix-1+kx], so the four kx of a lane
// are four consecutive floats of one row -- ONE 16-byte load (4-byte aligned) feeds four MFMAs.  At the left / right
// border the load starts one column late / early (it never leaves the row) and the values shift by one (WIDE; rows
// of fewer than 4 floats, w = 1, take clamped scalar loads instead).
// wt = W as [Co,4 kx,Ci,4 ky], so the A operand of (co, kx, 16 input channels) is 64 consecutive floats in memory and
// in LDS (element 4 j + g).  grid (B, tiles of 64 input pixels, groups of 16 CT input channels); one wave = 16 pixels x
// 16 CT channels, two accumulators per channel tile (even / odd kx).
// (written out, not a gol_conv4s2.h helper: as row_gemm + callbacks, shared with enc_fwd_kernel, the VGPR counts of
// three instances moved or the loaded block spilled: profiles/LOG.md "conv4s2")
template <int CT, bool WIDE>
__global__ __launch_bounds__(256) void trunk_bwd_x_kernel(const TrunkDims p, const float* __restrict__ pwt,
                                                          const float* __restrict__ py, const float* __restrict__ pg,
                                                          float* __restrict__ pgx) {
  __shared__ __attribute__((aligned(16))) float s_w[kBxKC * 4 * CT * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, cig0 = blockIdx.z * (16 * CT);
  const int h = p.h, w = p.w, Ci = p.Ci, Co = p.Co;
  const int HWi = h * w;
  const size_t HWo = (size_t)4 * HWi;
  const int pix = (blockIdx.y * 4 + wave) * 16 + j;
  const bool pv = pix < HWi;
  const int iy = pv ? pix / w : 0, ix = pv ? pix - iy * w : 0;
  const int oy = 2 * iy - 1 + g, c0 = 2 * ix - 1;
  const bool rv = pv && oy >= 0 && oy < 2 * h;
  const unsigned rowb = rv ? (unsigned)oy * (unsigned)(2 * w) : 0u;
  // byte offsets inside a plane (planes hold <= 2^26 floats): uniform plane pointer + 32-bit lane offset
  const int s0 = WIDE ? min(max(c0, 0), 2 * w - 4) : 0;  // first column of the 16-byte load
  const int shift = c0 - s0;                              // WIDE: -1 (ix = 0), 0, +1 (ix = w - 1)
  unsigned coff[4];
  bool cv[4];
#pragma unroll
  for (int kx = 0; kx < 4; ++kx) {
    cv[kx] = rv && c0 + kx >= 0 && c0 + kx < 2 * w;
    coff[kx] = 4u * (rowb + (unsigned)(WIDE ? s0 : min(max(c0 + kx, 0), 2 * w - 1)));
  }
  const float* gb = pg + (size_t)b * Co * HWo;
  const float* yb = py + (size_t)b * Co * HWo;
  const float leak = p.leak;

  float4 wr[CT];
  float rg[kBxKC * 4], ry[kBxKC * 4];
  auto issue = [&](int co0) {
#pragma unroll
    for (int u = 0; u < CT; ++u) {  // stage = 16 (co,kx) rows of 16 CT float4 (one input channel each)
      const int f = tid + 256 * u, row = f / (CT * 16), ci = cig0 + (f - row * (CT * 16));
      const bool ok = ci < Ci;      // (Ci is a multiple of 8, a group holds 16, 32 or 64 channels)
      const float4 v = *reinterpret_cast<const float4*>(pwt + (((size_t)co0 * 4 + row) * Ci + (ok ? ci : 0)) * 4);
      wr[u] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int cl = 0; cl < kBxKC; ++cl) {
      const float* gpl = gol_uniform(gb + (size_t)(co0 + cl) * HWo);
      const float* ypl = gol_uniform(yb + (size_t)(co0 + cl) * HWo);
      if constexpr (WIDE) {
        const f32x4u gv = *reinterpret_cast<const f32x4u*>(gol_at(gpl, coff[0]));
        const f32x4u yv = *reinterpret_cast<const f32x4u*>(gol_at(ypl, coff[0]));
#pragma unroll
        for (int t = 0; t < 4; ++t) { rg[cl * 4 + t] = gv[t]; ry[cl * 4 + t] = yv[t]; }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) { rg[cl * 4 + t] = *gol_at(gpl, coff[t]); ry[cl * 4 + t] = *gol_at(ypl, coff[t]); }
      }
    }
  };
  f32x4 acc[CT][2];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct][0] = acc[ct][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  issue(0);
  for (int co0 = 0; co0 < Co; co0 += kBxKC) {
    __syncthreads();
    float gp[kBxKC * 4];  // [co][kx]
#pragma unroll
    for (int cl = 0; cl < kBxKC; ++cl) {
      float m[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) m[t] = rg[cl * 4 + t] * (ry[cl * 4 + t] > 0.f ? 1.f : leak);
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        float v = m[kx];
        if constexpr (WIDE) v = shift == 0 ? m[kx] : (shift > 0 ? m[min(kx + 1, 3)] : m[max(kx - 1, 0)]);
        gp[cl * 4 + kx] = cv[kx] ? v : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < CT; ++u) reinterpret_cast<float4*>(s_w)[tid + 256 * u] = wr[u];
    __syncthreads();
    if (co0 + kBxKC < Co) issue(co0 + kBxKC);
#pragma unroll
    for (int e = 0; e < kBxKC * 4; ++e)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        acc[ct][e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[(e * CT + ct) * 64 + 4 * j + g], gp[e], acc[ct][e & 1],
                                                              0, 0, 0);
  }
  if (!pv) return;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int ci = cig0 + 16 * ct + 4 * g + r4;
      if (ci < Ci) pgx[((size_t)b * Ci + ci) * HWi + pix] = acc[ct][0][r4] + acc[ct][1][r4];
    }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------
// gw[ci,co,ky,kx] = sum_{b,iy,ix} x[b,ci,iy,ix] gpre[b,co,2iy-1+ky,2ix-1+kx].  grid (K blocks, groups of NCI ci tiles x
// co tiles).  A workgroup walks tiles of one view x one input row x 64 input pixels: x[16 NCI][64] and the matching
// g_pre window [16 co][4 rows][130 cols] are staged in LDS; the window is shared by the NCI channel tiles (wave ->
// channel tile wave % NCI, pixel part wave / NCI), each wave feeds 16-pixel chunks to 64 MFMAs (16 taps x 4 pixels per
// instruction); the waves' sums meet in LDS and leave as one partial [16 taps][16 ci][16 co] per channel tile.
// (the loaders, the MFMA nest and the wave sum are written out: as gol_conv4s2.h helpers they changed the VGPR counts of the
// weight-gradient kernels, profiles/LOG.md "conv4s2")
template <int NCI>
__global__ __launch_bounds__(256) void trunk_bwd_w_kernel(const TrunkDims p, const float* __restrict__ px,
                                                          const float* __restrict__ py, const float* __restrict__ pg,
                                                          float* __restrict__ pscratch) {
  constexpr int NP = 4 / NCI;  // waves that share a channel tile split the tile's 64 pixels
  __shared__ __attribute__((aligned(16))) float s_mem[16 * kWinPlane + NCI * 16 * kPixRow];
  float* s_g = s_mem;
  float* s_x = s_mem + 16 * kWinPlane;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
  const int cil = wave % NCI, part = wave / NCI;
  const int h = p.h, w = p.w, Ci = p.Ci, Co = p.Co;
  const int nco = Co >> 4, cig = blockIdx.y / nco, cot = blockIdx.y - cig * nco;
  const int ci0 = cig * (NCI * 16), co0 = cot * 16;
  const size_t HWi = (size_t)h * w, HWo = 4 * HWi;
  const float leak = p.leak;
  f32x4 acc[4][4];
#pragma unroll
  for (int dy = 0; dy < 4; ++dy)
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) acc[dy][dx] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tpr = (w + kWTile - 1) / kWTile, ntiles = p.B * h * tpr;
  // Staging is software-pipelined as in tail_conv_bwd_w_kernel: the global loads of the NEXT tile are issued (into
  // registers, all independent) before the MFMA phase of the current one.
  //   g, y: wave -> 16 of the 64 (plane, row) segments, columns [0,128) as two 64-lane loads; the 2 leftover columns of
  //         the 64 segments go to threads 0..127;  x: thread -> (4 NCI channels, 1 pixel)
  float rg[32], ry[32], rlg, rly, rx[4 * NCI];
  const int lseg = (tid >> 1) & 63, lcl = 2 * kWTile + (tid & 1);
  auto issue = [&](int tile) {
    const int b = tile / (h * tpr), rem = tile - b * (h * tpr), iy = rem / tpr, ix0 = (rem - iy * tpr) * kWTile;
    const float* xr = px + ((size_t)b * Ci + min(ci0 + wave, Ci - 1)) * HWi + (size_t)iy * w + min(ix0 + lane, w - 1);
#pragma unroll
    for (int u = 0; u < 4 * NCI; ++u) rx[u] = xr[ci0 + wave + 4 * u < Ci ? (size_t)(4 * u) * HWi : 0];
    // one scalar base per array + 32-bit byte offsets inside the 16-plane slab (planes hold <= 2^26 floats)
    const float* gs = gol_uniform(pg + ((size_t)b * Co + co0) * HWo);
    const float* ys = gol_uniform(py + ((size_t)b * Co + co0) * HWo);
#pragma unroll
    for (int sgm = 0; sgm < 16; ++sgm) {
      const int seg = wave * 16 + sgm, oy = min(max(2 * iy - 1 + (seg & 3), 0), 2 * h - 1);
      const unsigned rowb = (unsigned)(seg >> 2) * (unsigned)HWo + (unsigned)oy * (unsigned)(2 * w);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const unsigned o = 4u * (rowb + (unsigned)min(max(2 * ix0 - 1 + lane + 64 * u, 0), 2 * w - 1));
        rg[2 * sgm + u] = *gol_at(gs, o);
        ry[2 * sgm + u] = *gol_at(ys, o);
      }
    }
    {
      const int oy = min(max(2 * iy - 1 + (lseg & 3), 0), 2 * h - 1), col = min(max(2 * ix0 - 1 + lcl, 0), 2 * w - 1);
      const unsigned o = 4u * ((unsigned)(lseg >> 2) * (unsigned)HWo + (unsigned)oy * (unsigned)(2 * w) + (unsigned)col);
      rlg = *gol_at(gs, o);
      rly = *gol_at(ys, o);
    }
  };
  auto stage = [&](int tile) {  // registers -> LDS: g_pre = g (y > 0 ? 1 : leak), out-of-range elements as zeros
    const int b = tile / (h * tpr), rem = tile - b * (h * tpr), iy = rem / tpr, ix0 = (rem - iy * tpr) * kWTile;
    // (channels past Ci hold a copy of a valid row: they only reach accumulator rows that the reduce kernel drops)
    const bool xv = ix0 + lane < w;
#pragma unroll
    for (int u = 0; u < 4 * NCI; ++u) s_x[(wave + 4 * u) * kPixRow + lane] = xv ? rx[u] : 0.f;
#pragma unroll
    for (int sgm = 0; sgm < 16; ++sgm) {
      const int seg = wave * 16 + sgm, pl = seg >> 2, dy = seg & 3, oy = 2 * iy - 1 + dy;
      const bool rv = oy >= 0 && oy < 2 * h;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int cl = lane + 64 * u, col = 2 * ix0 - 1 + cl;
        s_g[pl * kWinPlane + dy * kWinRow + cl] =
            (rv && col >= 0 && col < 2 * w) ? rg[2 * sgm + u] * (ry[2 * sgm + u] > 0.f ? 1.f : leak) : 0.f;
      }
    }
    if (tid < 128) {
      const int pl = lseg >> 2, dy = lseg & 3, oy = 2 * iy - 1 + dy, col = 2 * ix0 - 1 + lcl;
      s_g[pl * kWinPlane + dy * kWinRow + lcl] = (oy >= 0 && oy < 2 * h && col < 2 * w) ? rlg * (rly > 0.f ? 1.f : leak) : 0.f;
    }
  };
  // A workgroup takes a run of consecutive tiles (consecutive input rows re-read two of their four g_pre rows), and the
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
    for (int c = 0; c < NCI; ++c) {
      const int xl = (part * NCI + c) * 16 + 4 * kq;  // this lane's 4 input pixels (K slice) inside the tile
      const float4 xa4 = *reinterpret_cast<const float4*>(&s_x[(cil * 16 + l15) * kPixRow + xl]);
      const float xa[4] = {xa4.x, xa4.y, xa4.z, xa4.w};
#pragma unroll
      for (int dy = 0; dy < 4; ++dy) {
        const float* gp = &s_g[l15 * kWinPlane + dy * kWinRow + 2 * xl];  // column 0 of s_g is global column 2 ix0 - 1
        float gv[10];
#pragma unroll
        for (int q = 0; q < 10; q += 2) {
          const float2 t2 = *reinterpret_cast<const float2*>(gp + q);
          gv[q] = t2.x; gv[q + 1] = t2.y;
        }
#pragma unroll
        for (int dx = 0; dx < 4; ++dx)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[dy][dx] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[t], gv[2 * t + dx], acc[dy][dx], 0, 0, 0);
      }
    }
  }
  // D[i = ci][j = co]: lane holds column l15, rows 4 kq + r.  Per channel tile, its NP waves add up in LDS in wave
  // order, then the tile's partial [16 taps][16 ci][16 co] leaves: scratch is [group][NCI][K block][16 taps][256].
  __syncthreads();
  float (*s_red)[256] = reinterpret_cast<float (*)[256]>(s_mem);
  for (int c = 0; c < NCI; ++c) {
    for (int pt = 0; pt < NP; ++pt) {
      if (cil == c && part == pt) {
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
      __syncthreads();
    }
    wgrad_store_partial(pscratch + ((((size_t)blockIdx.y * NCI + c) * gridDim.x + blockIdx.x) * 16) * 256 + tid, s_red);
    __syncthreads();
  }
}

// gw[ci,co,tap] = sum over the K blocks (written once).  grid (16 taps x 16 ci rows, channel tiles)
__global__ __launch_bounds__(256) void trunk_bwd_w_reduce_kernel(const TrunkDims p, int NCI, int nblk,
                                                                 const float* __restrict__ scratch,
                                                                 float* __restrict__ gw) {
  const int tap = blockIdx.x >> 4, row = blockIdx.x & 15, col = threadIdx.x & 15;
  const int nco = p.Co >> 4, grp = blockIdx.y / NCI, c = blockIdx.y - grp * NCI;
  const int cig = grp / nco, cot = grp - cig * nco;
  const int ci = (cig * NCI + c) * 16 + row, co = cot * 16 + col;
  if (ci >= p.Ci) return;  // block-uniform: ragged last tile (Ci = 8 * odd) or a tile past the end of the last group
  wgrad_reduce16(scratch + (((size_t)blockIdx.y * nblk) * 16 + tap) * 256 + row * 16 + col, nblk,
                 gw + ((size_t)ci * p.Co + co) * 16 + tap, true);
}

// ---- bias gradient: over the Co * 2h * 2w plane elements, four per thread -----------------------------------------------
__global__ __launch_bounds__(256) void trunk_bwd_b_kernel(const TrunkDims p, const float* __restrict__ py,
                                                          const float* __restrict__ pg, float* __restrict__ pgb) {
  lrelu_bias_grad((size_t)p.Co * p.h * p.w, p.B, p.leak, py, pg, pgb);
}

int check_common(int B, int Ci, int Co, int h, int w, float leak) {
  GOL_REQUIRE(B >= 0 && Ci > 0 && Co > 0 && h > 0 && w > 0, "bad sizes");
  GOL_REQUIRE(leak > 0.f, "leak must be positive (the backward reads the activation mask from the sign of y)");
  if (Ci % 8 != 0 || Co % 16 != 0) {
    gol_set_error("gol_trunk_conv: Ci must be a multiple of 8 and Co a multiple of 16 (got %d -> %d)", Ci, Co);
    return GOL_ERR_UNSUPPORTED;
  }
  // 32-bit pixel indices inside a plane; grid.y / grid.z limits
  GOL_REQUIRE((long long)(2 * (long long)h + 2) * (2 * (long long)w + 2) < (1ll << 26), "plane too large");
  GOL_REQUIRE((long long)B * h * gol_cdiv(w, kWTile) < (1ll << 31), "too many row tiles");
  GOL_REQUIRE(gol_cdiv((long long)(h + 1) * (w + 1), 64) <= 65535, "too many pixel tiles");
  GOL_REQUIRE((long long)(gol_cdiv(Ci, 16) + 3) * (Co / 16) <= 65535, "too many channel tiles");
  GOL_REQUIRE((long long)Co * h * w / 256 < (1ll << 31), "layer too large");
  return GOL_OK;
}

// channel tiles of 16 ci that one workgroup of the weight gradient takes (they share the staged g_pre window)
int bwd_w_nci(int Ci) { return Ci > 32 ? 4 : (Ci > 16 ? 2 : 1); }
int bwd_w_groups(int Ci, int Co) { return gol_cdiv(Ci, 16 * bwd_w_nci(Ci)) * (Co / 16); }

// 2 workgroups per CU are resident (registers): one round of them
int bwd_w_blocks(int B, int Ci, int Co, int h, int w) {
  return wgrad_blocks((long long)B * h * gol_cdiv(w, kWTile), bwd_w_groups(Ci, Co), 512);
}

}  // namespace

extern "C" int gol_trunk_conv_fwd(int B, int Ci, int Co, int h, int w, float leak, const float* x, const float* w_eff,
                                  const float* bias, float* y, void* stream) {
  const int rc = check_common(B, Ci, Co, h, w, leak);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && w_eff && bias && y, "null pointer");
  GOL_REQUIRE(gol_aligned16(w_eff), "w_eff must be 16-byte aligned");
  const TrunkDims p{B, Ci, Co, h, w, leak};
  hipStream_t s = (hipStream_t)stream;
  const int tiles = gol_cdiv((long long)(h + 1) * (w + 1), 64);
  if (Co == 16) trunk_fwd_kernel<1><<<dim3(B, tiles, 1), 256, 0, s>>>(p, x, w_eff, bias, y);
  else trunk_fwd_kernel<2><<<dim3(B, tiles, gol_cdiv(Co, 32)), 256, 0, s>>>(p, x, w_eff, bias, y);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" long long gol_trunk_conv_bwd_scratch_floats(int B, int Ci, int Co, int h, int w) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || h <= 0 || w <= 0 || Co % 16 != 0) return 0;
  return (long long)bwd_w_groups(Ci, Co) * bwd_w_nci(Ci) * bwd_w_blocks(B, Ci, Co, h, w) * 16 * 256;
}

extern "C" int gol_trunk_conv_bwd(int B, int Ci, int Co, int h, int w, float leak, const float* x, const float* w_eff_t,
                                  const float* y, const float* g_y, float* g_x, float* g_w, float* g_bias, float* scratch,
                                  void* stream) {
  const int rc = check_common(B, Ci, Co, h, w, leak);
  if (rc != GOL_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {  // empty sums
    if (g_w && hipMemsetAsync(g_w, 0, sizeof(float) * 16 * Ci * Co, s) != hipSuccess) return GOL_ERR_LAUNCH;
    if (g_bias && hipMemsetAsync(g_bias, 0, sizeof(float) * 4 * Co * h * w, s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  GOL_REQUIRE(y && g_y, "null pointer");
  GOL_REQUIRE(!g_x || (w_eff_t && gol_aligned16(w_eff_t)), "g_x needs w_eff_t (16-byte aligned)");
  GOL_REQUIRE(!g_w || (x && scratch), "g_w needs x and scratch");
  GOL_REQUIRE(!g_bias || (gol_aligned16(y) && gol_aligned16(g_y) && gol_aligned16(g_bias)), "g_bias needs 16-byte aligned y, g_y, g_bias");
  const TrunkDims p{B, Ci, Co, h, w, leak};
  if (g_x) {
    const int tiles = gol_cdiv((long long)h * w, 64);
    const dim3 grid(B, tiles, gol_cdiv(Ci, Ci <= 16 ? 16 : (Ci <= 32 ? 32 : 64)));
#define TRUNK_BWD_X(CT)                                                                              \
  do {                                                                                               \
    if (w >= 2) trunk_bwd_x_kernel<CT, true><<<grid, 256, 0, s>>>(p, w_eff_t, y, g_y, g_x);          \
    else trunk_bwd_x_kernel<CT, false><<<grid, 256, 0, s>>>(p, w_eff_t, y, g_y, g_x);                \
  } while (0)
    if (Ci <= 16) TRUNK_BWD_X(1);
    else if (Ci <= 32) TRUNK_BWD_X(2);
    else TRUNK_BWD_X(4);
#undef TRUNK_BWD_X
    GOL_CHECK_LAUNCH();
  }
  if (g_w) {
    const int nci = bwd_w_nci(Ci), groups = bwd_w_groups(Ci, Co), nblk = bwd_w_blocks(B, Ci, Co, h, w);
    const dim3 grid(nblk, groups);
    if (nci == 1) trunk_bwd_w_kernel<1><<<grid, 256, 0, s>>>(p, x, y, g_y, scratch);
    else if (nci == 2) trunk_bwd_w_kernel<2><<<grid, 256, 0, s>>>(p, x, y, g_y, scratch);
    else trunk_bwd_w_kernel<4><<<grid, 256, 0, s>>>(p, x, y, g_y, scratch);
    GOL_CHECK_LAUNCH();
    trunk_bwd_w_reduce_kernel<<<dim3(256, groups * nci), 256, 0, s>>>(p, nci, nblk, scratch, g_w);
    GOL_CHECK_LAUNCH();
  }
  if (g_bias) {
    trunk_bwd_b_kernel<<<dim3(gol_cdiv((long long)Co * h * w, 256)), 256, 0, s>>>(p, y, g_y, g_bias);
    GOL_CHECK_LAUNCH();
  }
  return GOL_OK;
}
