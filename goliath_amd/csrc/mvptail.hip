// mvptail.hip -- the last layer of the MVP hand model's two decoders, written straight into the primitive template, gfx950.
//
// Both decoders of ca_code/models/hand_mvp.py end in ConvTranspose2dWNUB(16 -> TD C, k4 s2 p1) + an untied bias
// (:338-340, :384, :455), followed by relu(25 x + 100) on the colours (:472), relu on alpha (:434) and the cat / view /
// permute / reshape into the channels-last template (:172-185) of which the march keeps template[:, valid_prims]
// (ca_code/utils/render_raymarcher.py:41-47).  Here:
//   fwd     the tail.hip / trunk.hip formulation: an output 2x2 quad {2m-1, 2m} x {2k-1, 2k} reads the 2x2 input block
//           {m-1, m} x {k-1, k} and uses each of the 16 taps once, so every output parity class (a,q) is a GEMM
//           D[ch][quad] = A[ch][(ci,tap)] B[(ci,tap)][quad] on v_mfma_f32_16x16x4_f32 (exact fp32).  Up to three row tiles
//           of 16 channels (two of colour, one of alpha) stay in LDS for the life of the workgroup; one output row of the
//           wave's 32 columns goes through LDS so that every store is the 16-byte (r,g,b,a) of a depth slice and a
//           primitive's row of TW texels is one contiguous run; bias and activation are applied on that side, where the
//           bias is read in full lines.  The next tile's input and this tile's bias are in flight while the MFMAs run.
//           The slot of a texel is looked up per pixel (a quad straddles primitive boundaries); a tile whose texels are
//           all dropped or dead is not computed.  No slab is read or written.
//   bwd     staged: one pass reads g_out and out in template layout (16-byte loads: three colours and the alpha of a depth
//           slice), forms g_pre = g_out [out > 0] (colours times rgb_scale, zero for dropped and dead primitives), writes
//           it slab-shaped into scratch and sums it over the views into the bias gradients.  The input gradient is the
//           16-channel scalar gather and the weight gradient the split-K GEMM with the fixed-order reduction of
//           gol_conv4s2.h (one tile of 16 input channels, g_pre read as it is, plain run order).  No float atomics.
#include "gol_conv4s2.h"

namespace {

constexpr int kCi = 16;     // input channels of both last layers (hand_mvp.py:338)
constexpr int kMaxTD = 10;  // 3 TD <= 32: two row tiles of colour

struct MvpTailDims {
  int B, h, w, TD, TH, TW, ny, nx, Kout;
  float scale, shift;
};

// ---- forward ---------------------------------------------------------------------------------------------------------
// grid (B, K blocks): the B views of a run of tiles are neighbours in dispatch order, so a bias tile comes from memory
// once and from L2 for the other views.  A workgroup keeps the weights of all NR + 1 row tiles in LDS and walks its run of
// tiles four at a time, one per wave.  One wave tile = 16 quads of one quad row = output rows {2m-1, 2m} x 32 columns.
// MFMA operands: A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15], D[i = 4 (lane >> 4) + r][j].
// NR = row tiles of colour (0: the one-channel template).
template <int NR>
__global__ __launch_bounds__(256, 2) void mvptail_fwd_kernel(
    const MvpTailDims p, const float* __restrict__ pxr, const float* __restrict__ pwr, const float* __restrict__ pbr,
    const float* __restrict__ pxa, const float* __restrict__ pwa, const float* __restrict__ pba,
    const int* __restrict__ pslot, const int* __restrict__ plive, float* __restrict__ pout) {
  constexpr int NT = NR + 1, C = NR ? 4 : 1;
  // s_w[ci][cls][tile][tap g][channel j]: the A operand of (ci, cls, tile) is 64 consecutive floats, one per lane
  __shared__ __attribute__((aligned(16))) float s_w[kCi * 4 * NT * 64];
  // s_o[wave][z][column][C]: one output row of the wave's tile, read back as the template's texels
  __shared__ __attribute__((aligned(16))) float s_o[4][kMaxTD * 32 * C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int ty = g >> 1, tx = g & 1;
  const int b = blockIdx.x;
  const int h = p.h, w = p.w, TD = p.TD, CHr = 3 * TD, Sy = 2 * h, Sx = 2 * w;
  const size_t HWi = (size_t)h * w, HWo = 4 * HWi;

#pragma unroll 8
  for (int f = tid; f < kCi * NT * 256; f += 256) {
    const int tap = f & 15, row = (f >> 4) % (NT * 16), ci = (f >> 4) / (NT * 16);
    const int t = row >> 4, jj = row & 15;
    float v = 0.f;
    if (t < NR) {
      if (row < CHr) v = pwr[((size_t)ci * CHr + row) * 16 + tap];
    } else if (jj < TD) {
      v = pwa[((size_t)ci * TD + jj) * 16 + tap];
    }
    const int ky = tap >> 2, kx = tap & 3;  // tap (ky,kx) = (a + 2 ty, q + 2 tx)
    const int cls = 2 * (ky & 1) + (kx & 1), gg = 2 * (ky >> 1) + (kx >> 1);
    s_w[((ci * 4 + cls) * NT + t) * 64 + gg * 16 + jj] = v;
  }
  __syncthreads();

  const int tpr = (w + 1 + 15) >> 4, ntiles = (h + 1) * tpr;
  const int per = (ntiles + (int)gridDim.y - 1) / (int)gridDim.y;
  const int t0 = min((int)blockIdx.y * per, ntiles), t1 = min(t0 + per, ntiles);
  const float* xrb = NR ? pxr + (size_t)b * kCi * HWi : nullptr;
  const float* xab = pxa + (size_t)b * kCi * HWi;
  float* so = s_o[wave];
  const int scol = lane & 31, shalf = lane >> 5;  // the store phase: lane -> column of the tile, z parity

  // B[ci] of a tile: k = tap g, column = quad j.  One scalar base per view + 32-bit byte offsets (a view's 16 planes hold
  // < 2^27 floats).  The loads of the NEXT tile are issued before the MFMA phase of this one.
  float Bn[NT > 1 ? 2 : 1][kCi];
  auto issue = [&](int tile) {
    const int m = tile / tpr, kq = (tile - m * tpr) * 16 + j;
    const int r0 = m - ty, c0 = kq - tx;
    const bool vin = r0 >= 0 && r0 < h && c0 >= 0 && c0 < w;
    unsigned xoff = vin ? 4u * ((unsigned)r0 * (unsigned)w + (unsigned)c0) : 0u;
#pragma unroll
    for (int ci = 0; ci < kCi; ++ci) {
      const float va = *gol_at(xab, xoff);
      Bn[0][ci] = vin ? va : 0.f;
      if constexpr (NR > 0) {
        const float vr = *gol_at(xrb, xoff);
        Bn[1][ci] = vin ? vr : 0.f;
      }
      xoff += 4u * (unsigned)HWi;
    }
  };
  if (t0 + wave < t1) issue(t0 + wave);

#pragma unroll 1
  for (int base = t0; base < t1; base += 4) {  // the same trip count for the four waves: barriers inside
    const int tile = base + wave;
    const bool tv = tile < t1;
    const int m = tv ? tile / tpr : 0, k0 = tv ? (tile - m * tpr) * 16 : 0;
    // TD as the z loops below compare it: opaque per iteration, so that their ten loop-invariant predicates are formed
    // where they are used (hoisted out of the tile loop they are ten lane masks, 20 SGPRs, and spill)
    int TDz = TD;
    asm volatile("" : "+s"(TDz));
    float Bx[NT > 1 ? 2 : 1][kCi];
#pragma unroll
    for (int u = 0; u < (NT > 1 ? 2 : 1); ++u)
#pragma unroll
      for (int ci = 0; ci < kCi; ++ci) Bx[u][ci] = Bn[u][ci];
    // where this lane's column of the two output rows goes
    const int X = 2 * k0 - 1 + scol;
    const bool xv = tv && X >= 0 && X < Sx;
    const int pxi = xv ? X / p.TW : 0, xx = xv ? X - pxi * p.TW : 0;
    size_t obase[2];
    int ofl[2];  // 0: not stored, 1: stored as zeros (a dead primitive), 3: stored (kept as a number: a lane mask held
                 // across the MFMA phase costs two SGPRs)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int Y = 2 * m - 1 + a;
      const bool v = xv && Y >= 0 && Y < Sy;
      const int pyi = v ? Y / p.TH : 0, yy = v ? Y - pyi * p.TH : 0;
      const int k = pyi * p.nx + pxi;
      int sl = k, lv = 1;
      if (v && pslot) sl = pslot[k];
      if (v && plive) lv = plive[k];
      const bool st = v && sl >= 0 && sl < p.Kout;
      ofl[a] = st ? (lv != 0 ? 3 : 1) : 0;
      obase[a] = ((((size_t)b * p.Kout + (st ? sl : 0)) * TD * p.TH + yy) * p.TW + xx) * C;
    }
    const bool need = gol_ballot(((ofl[0] | ofl[1]) & 2) != 0) != 0ull;  // wave-uniform
#pragma unroll
    for (int a = 0; a < 2; ++a) asm volatile("" : "+v"(ofl[a]));

    // the bias where the store phase wants it: this lane's column of the two rows, the depth slices z = shalf + 2 zi it
    // stores, three colours and alpha -- full lines along X, in flight while the MFMAs run
    constexpr int NZ = kMaxTD / 2;
    float bz[2][NZ][C];
    if (need) {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        // 32-bit element indices: the 32 planes of a bias hold < 2^30 floats
        const unsigned po = ofl[a] ? (unsigned)(2 * m - 1 + a) * (unsigned)Sx + (unsigned)X : 0u;
#pragma unroll
        for (int zi = 0; zi < NZ; ++zi) {
          if (2 * zi >= TDz) break;  // wave-uniform
          const unsigned zo = (unsigned)min(shalf + 2 * zi, TDz - 1) * (unsigned)HWo + po;
          if constexpr (C == 4) {
#pragma unroll
            for (int c = 0; c < 3; ++c) bz[a][zi][c] = pbr[3u * zo - 2u * po + (unsigned)c * (unsigned)HWo];
          }
          bz[a][zi][C - 1] = pba[zo];
        }
      }
    }
    if (base + 4 + wave < t1) issue(base + 4 + wave);
    f32x4 acc[NT][4];
    if (need) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) acc[t][cls] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ci = 0; ci < kCi; ++ci)
#pragma unroll
        for (int cls = 0; cls < 4; ++cls)
#pragma unroll
          for (int t = 0; t < NT; ++t)
            acc[t][cls] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[((ci * 4 + cls) * NT + t) * 64 + lane],
                                                               Bx[t < NR ? 1 : 0][ci], acc[t][cls], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      __syncthreads();  // the previous row has left s_o
      if (need) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int col = 2 * j + q;
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int ch = (t < NR ? 16 * t : 0) + 4 * g + r;
              if (t < NR) {
                const int z = ch / 3, c = ch - 3 * z;
                if (ch < CHr) so[(z * 32 + col) * C + c] = acc[t][2 * a + q][r];
              } else if (ch < TD) {
                so[(ch * 32 + col) * C + (C - 1)] = acc[t][2 * a + q][r];
              }
            }
        }
      }
      __syncthreads();
      if (ofl[a] != 0) {
        const bool lv = (ofl[a] & 2) != 0;
        float* dst = pout + obase[a];
        const size_t zs = (size_t)p.TH * p.TW * C;
        // bias on the finished sum, then the activation; the affine as PyTorch composes it: product and sum rounded
        // separately
#pragma unroll
        for (int zi = 0; zi < NZ; ++zi) {
          if (2 * zi >= TDz) break;  // wave-uniform
          const int z = shalf + 2 * zi, zc = min(z, TDz - 1);
          if constexpr (C == 4) {
            const float4 s4 = *reinterpret_cast<const float4*>(&so[(zc * 32 + scol) * 4]);
            float4 v;
            v.x = fmaxf(__fadd_rn(__fmul_rn(p.scale, s4.x + bz[a][zi][0]), p.shift), 0.f);
            v.y = fmaxf(__fadd_rn(__fmul_rn(p.scale, s4.y + bz[a][zi][1]), p.shift), 0.f);
            v.z = fmaxf(__fadd_rn(__fmul_rn(p.scale, s4.z + bz[a][zi][2]), p.shift), 0.f);
            v.w = fmaxf(s4.w + bz[a][zi][3], 0.f);
            if (!lv) v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (z < TDz) *reinterpret_cast<float4*>(dst + (size_t)z * zs) = v;
          } else {
            const float v = lv ? fmaxf(so[zc * 32 + scol] + bz[a][zi][0], 0.f) : 0.f;
            if (z < TDz) dst[(size_t)z * zs] = v;
          }
        }
      }
    }
  }
}

// ---- backward, pass 1: template layout -> slab-shaped g_pre, and the bias gradients -----------------------------------
// One thread = one (z, Y, X) of the slabs; the views are its loop, so the bias gradient is a sum in view order.  Lanes
// run along X: the template side is 16-byte loads that are contiguous inside a primitive's row, the slab side full lines.
template <int C>
__global__ __launch_bounds__(256) void mvptail_gpre_kernel(const MvpTailDims p, const int* __restrict__ pslot,
                                                           const int* __restrict__ plive, const float* __restrict__ pg,
                                                           const float* __restrict__ po, float* __restrict__ pgr,
                                                           float* __restrict__ pga, float* __restrict__ pgbr,
                                                           float* __restrict__ pgba) {
  const int TD = p.TD, Sy = 2 * p.h, Sx = 2 * p.w;
  const size_t HWo = (size_t)Sy * Sx, N = HWo * TD;
  const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int z = (int)(n / HWo);
  const size_t pix = n - (size_t)z * HWo;
  const int Y = (int)(pix / Sx), X = (int)(pix - (size_t)Y * Sx);
  const int pyi = Y / p.TH, yy = Y - pyi * p.TH, pxi = X / p.TW, xx = X - pxi * p.TW;
  const int k = pyi * p.nx + pxi;
  const int sl = pslot ? pslot[k] : k;
  const bool on = sl >= 0 && sl < p.Kout && (!plive || plive[k] != 0);
  const size_t vstride = (size_t)p.Kout * TD * p.TH * p.TW * C;
  const size_t toff = (((((size_t)(on ? sl : 0)) * TD + z) * p.TH + yy) * p.TW + xx) * C;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < p.B; ++b) {
    float gp[4] = {0.f, 0.f, 0.f, 0.f};
    if (on) {
      if constexpr (C == 4) {
        const float4 gv = *reinterpret_cast<const float4*>(pg + (size_t)b * vstride + toff);
        const float4 ov = *reinterpret_cast<const float4*>(po + (size_t)b * vstride + toff);
        gp[0] = ov.x > 0.f ? gv.x * p.scale : 0.f;
        gp[1] = ov.y > 0.f ? gv.y * p.scale : 0.f;
        gp[2] = ov.z > 0.f ? gv.z * p.scale : 0.f;
        gp[3] = ov.w > 0.f ? gv.w : 0.f;
      } else {
        gp[3] = po[(size_t)b * vstride + toff] > 0.f ? pg[(size_t)b * vstride + toff] : 0.f;
      }
    }
    if constexpr (C == 4) {
      if (pgr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pgr[((size_t)b * 3 * TD + 3 * z + c) * HWo + pix] = gp[c];
      }
    }
    if (pga) pga[((size_t)b * TD + z) * HWo + pix] = gp[3];
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] += gp[c];
  }
  if constexpr (C == 4) {
    if (pgbr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) pgbr[(size_t)(3 * z + c) * HWo + pix] = s[c];
    }
  }
  if (pgba) pgba[(size_t)z * HWo + pix] = s[3];
}

// ---- input gradient: the scalar gather of gol_conv4s2.h; wt = W as [CH,4,4,16] --------------------------------------------
__global__ __launch_bounds__(256) void mvptail_bwd_x_kernel(int h, int w, int CH, const float* __restrict__ pwt,
                                                            const float* __restrict__ pg, float* __restrict__ pgx) {
  gather_bwd_x16(h, w, CH, pwt, pg, pgx);
}

// ---- weight gradient (trunk_bwd_w_kernel with one tile of 16 input channels, g_pre read as it is) ------------------------
// gw[ci,ch,ky,kx] = sum_{b,iy,ix} x[b,ci,iy,ix] g[b,ch,2iy-1+ky,2ix-1+kx].  grid (K blocks, tiles of 16 channels).  A
// workgroup walks tiles of one view x one input row x 64 input pixels: x[16][64] and the matching window
// [16 ch][4 rows][130 cols] are staged in LDS, each wave feeds its 16-pixel chunk to 64 MFMAs (16 taps x 4 pixels per
// instruction); the waves' sums meet in LDS in wave order and leave as one partial [16 taps][16 ci][16 ch].
// (the loaders, the MFMA nest and the wave sum are written out: as gol_conv4s2.h helpers they changed the VGPR counts of the
// weight-gradient kernels, profiles/LOG.md "conv4s2")
__global__ __launch_bounds__(256) void mvptail_bwd_w_kernel(int B, int h, int w, int CH, const float* __restrict__ px,
                                                            const float* __restrict__ pg, float* __restrict__ pscratch) {
  __shared__ __attribute__((aligned(16))) float s_mem[16 * kWinPlane + 16 * kPixRow];
  float* s_g = s_mem;
  float* s_x = s_mem + 16 * kWinPlane;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
  const int co0 = blockIdx.y * 16;
  const size_t HWi = (size_t)h * w, HWo = 4 * HWi;
  f32x4 acc[4][4];
#pragma unroll
  for (int dy = 0; dy < 4; ++dy)
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) acc[dy][dx] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tpr = (w + kWTile - 1) / kWTile, ntiles = B * h * tpr;
  // the global loads of the NEXT tile are issued (into registers, all independent) before the MFMA phase of this one.
  //   g: wave -> 16 of the 64 (plane, row) segments, columns [0,128) as two 64-lane loads; the 2 leftover columns of the
  //      64 segments go to threads 0..127;  x: thread -> (4 channels, 1 pixel)
  float rg[32], rlg, rx[4];
  const int lseg = (tid >> 1) & 63, lcl = 2 * kWTile + (tid & 1);
  auto issue = [&](int tile) {
    const int b = tile / (h * tpr), rem = tile - b * (h * tpr), iy = rem / tpr, ix0 = (rem - iy * tpr) * kWTile;
    const float* xr = px + ((size_t)b * kCi + wave) * HWi + (size_t)iy * w + min(ix0 + lane, w - 1);
#pragma unroll
    for (int u = 0; u < 4; ++u) rx[u] = xr[(size_t)(4 * u) * HWi];
    // one scalar base + 32-bit byte offsets inside the slab of <= 16 planes (planes hold < 2^26 floats)
    const float* gs = gol_uniform(pg + ((size_t)b * CH + co0) * HWo);
#pragma unroll
    for (int sgm = 0; sgm < 16; ++sgm) {
      const int seg = wave * 16 + sgm, oy = min(max(2 * iy - 1 + (seg & 3), 0), 2 * h - 1);
      const int pl = min(co0 + (seg >> 2), CH - 1) - co0;  // planes past CH re-read the last one, staged as zeros
      const unsigned rowb = (unsigned)pl * (unsigned)HWo + (unsigned)oy * (unsigned)(2 * w);
#pragma unroll
      for (int u = 0; u < 2; ++u)
        rg[2 * sgm + u] = *gol_at(gs, 4u * (rowb + (unsigned)min(max(2 * ix0 - 1 + lane + 64 * u, 0), 2 * w - 1)));
    }
    {
      const int oy = min(max(2 * iy - 1 + (lseg & 3), 0), 2 * h - 1), col = min(max(2 * ix0 - 1 + lcl, 0), 2 * w - 1);
      const int pl = min(co0 + (lseg >> 2), CH - 1) - co0;
      rlg = *gol_at(gs, 4u * ((unsigned)pl * (unsigned)HWo + (unsigned)oy * (unsigned)(2 * w) + (unsigned)col));
    }
  };
  auto stage = [&](int tile) {  // registers -> LDS, out-of-range elements as zeros
    const int b = tile / (h * tpr), rem = tile - b * (h * tpr), iy = rem / tpr, ix0 = (rem - iy * tpr) * kWTile;
    const bool xv = ix0 + lane < w;
#pragma unroll
    for (int u = 0; u < 4; ++u) s_x[(wave + 4 * u) * kPixRow + lane] = xv ? rx[u] : 0.f;
#pragma unroll
    for (int sgm = 0; sgm < 16; ++sgm) {
      const int seg = wave * 16 + sgm, pl = seg >> 2, dy = seg & 3, oy = 2 * iy - 1 + dy;
      const bool rv = co0 + pl < CH && oy >= 0 && oy < 2 * h;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int cl = lane + 64 * u, col = 2 * ix0 - 1 + cl;
        s_g[pl * kWinPlane + dy * kWinRow + cl] = (rv && col >= 0 && col < 2 * w) ? rg[2 * sgm + u] : 0.f;
      }
    }
    if (tid < 128) {
      const int pl = lseg >> 2, dy = lseg & 3, oy = 2 * iy - 1 + dy, col = 2 * ix0 - 1 + lcl;
      s_g[pl * kWinPlane + dy * kWinRow + lcl] = (co0 + pl < CH && oy >= 0 && oy < 2 * h && col < 2 * w) ? rlg : 0.f;
    }
  };
  // a workgroup takes a run of consecutive tiles (consecutive input rows re-read two of their four window rows)
  const int nb = gridDim.x, per = (ntiles + nb - 1) / nb;
  const int t0 = min((int)blockIdx.x * per, ntiles), t1 = min(t0 + per, ntiles);
  if (t0 < t1) issue(t0);
  for (int tile = t0; tile < t1; ++tile) {
    __syncthreads();  // the previous tile's operands have been consumed
    stage(tile);
    __syncthreads();
    if (tile + 1 < t1) issue(tile + 1);
    const int xl = wave * 16 + 4 * kq;  // this lane's 4 input pixels (K slice) inside the tile
    const float4 xa4 = *reinterpret_cast<const float4*>(&s_x[l15 * kPixRow + xl]);
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
  // D[i = ci][j = ch]: lane holds column l15, rows 4 kq + r.  The four waves add up in LDS in wave order; scratch is
  // [channel tile][K block][16 taps][256].
  __syncthreads();
  float (*s_red)[256] = reinterpret_cast<float (*)[256]>(s_mem);
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int dy = 0; dy < 4; ++dy)
#pragma unroll
        for (int dx = 0; dx < 4; ++dx)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* sp = &s_red[dy * 4 + dx][(kq * 4 + r) * 16 + l15];
            *sp = (wv == 0 ? 0.f : *sp) + acc[dy][dx][r];
          }
    }
    __syncthreads();
  }
  wgrad_store_partial(pscratch + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16) * 256 + tid, s_red);
}

// gw[ci,ch,tap] = sum over the K blocks, written once.  grid (16 taps x 16 ci rows, channel tiles)
__global__ __launch_bounds__(256) void mvptail_bwd_w_reduce_kernel(int CH, int nblk, const float* __restrict__ scratch,
                                                                   float* __restrict__ gw) {
  const int tap = blockIdx.x >> 4, ci = blockIdx.x & 15, col = threadIdx.x & 15;
  const int ch = blockIdx.y * 16 + col;
  wgrad_reduce16(scratch + (((size_t)blockIdx.y * nblk) * 16 + tap) * 256 + ci * 16 + col, nblk,
                 gw + ((size_t)ci * CH + ch) * 16 + tap, ch < CH);
}

int check_common(const char* who, int B, int Ci, int h, int w, int TD, int TH, int TW, int ny, int nx, int Kout) {
  if (Ci != kCi || TD < 1 || TD > kMaxTD) {
    gol_set_error("%s: 16 input channels and 1 <= TD <= 10 are supported (got Ci = %d, TD = %d)", who, Ci, TD);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(B >= 0 && h > 0 && w > 0 && TH > 0 && TW > 0 && ny > 0 && nx > 0 && Kout >= 0, "bad sizes");
  GOL_REQUIRE((long long)ny * TH == 2ll * h && (long long)nx * TW == 2ll * w, "the primitives must tile the [2h,2w] output");
  GOL_REQUIRE(B <= 65535 && h <= 65535, "grid limit: B, h <= 65535");
  GOL_REQUIRE((2ll * h + 2) * (2ll * w + 2) < (1ll << 25), "plane too large");  // 32-bit byte offsets in 16 planes
  GOL_REQUIRE((long long)B * h * gol_cdiv(w, kWTile) < (1ll << 31), "too many row tiles");
  GOL_REQUIRE((long long)ny * nx < (1ll << 31) && Kout <= (long long)ny * nx, "bad primitive count");
  return GOL_OK;
}

int bwd_w_blocks(int B, int h, int w, int ntile_ch) {  // two workgroups per CU: one round of them
  return wgrad_blocks((long long)B * h * gol_cdiv(w, kWTile), ntile_ch, 512);
}

// scratch: g_pre of the colours [B,3TD,Sy,Sx] (C == 4), g_pre of alpha [B,TD,Sy,Sx], then the weight gradient's partials
struct Scratch {
  long long gpre_rgb, gpre_alpha, part;
};
Scratch scratch_layout(int B, int h, int w, int TD, int C) {
  const long long plane = 4ll * h * w;
  Scratch s;
  s.gpre_rgb = C == 4 ? (long long)B * 3 * TD * plane : 0;
  s.gpre_alpha = (long long)B * TD * plane;
  const int nt = C == 4 ? gol_cdiv(3 * TD, 16) : 1;  // the two branches run one after the other: the larger of them
  const long long pr = (long long)nt * bwd_w_blocks(B, h, w, nt), pa = bwd_w_blocks(B, h, w, 1);
  s.part = (pr > pa ? pr : pa) * 16 * 256;
  return s;
}

}  // namespace

extern "C" int gol_mvp_tail_fwd(int B, int Ci, int h, int w, int TD, int TH, int TW, int ny, int nx, const float* x_rgb,
                                const float* w_rgb, const float* bias_rgb, const float* x_alpha, const float* w_alpha,
                                const float* bias_alpha, const int32_t* slot, const int32_t* live, int Kout,
                                float rgb_scale, float rgb_shift, float* out, void* stream) {
  const int rc = check_common(__func__, B, Ci, h, w, TD, TH, TW, ny, nx, Kout);
  if (rc != GOL_OK) return rc;
  GOL_REQUIRE(slot || Kout == ny * nx, "identity slots (slot == NULL) need Kout == ny nx");
  if (B == 0 || Kout == 0) return GOL_OK;
  GOL_REQUIRE(x_alpha && w_alpha && bias_alpha && out, "null pointer");
  GOL_REQUIRE(!x_rgb || (w_rgb && bias_rgb), "x_rgb needs w_rgb and bias_rgb");
  GOL_REQUIRE(!x_rgb || gol_aligned16(out), "the four-channel template must be 16-byte aligned");
  const MvpTailDims p{B, h, w, TD, TH, TW, ny, nx, Kout, rgb_scale, rgb_shift};
  hipStream_t s = (hipStream_t)stream;
  const int ntiles = (h + 1) * gol_cdiv(w + 1, 16);
  int nblk = gol_cdiv(1024, B);  // two resident workgroups per CU, two rounds
  const int cap = gol_cdiv(ntiles, 4);
  nblk = nblk < 1 ? 1 : (nblk > cap ? cap : nblk);
  const dim3 grid(B, nblk);
#define MVPTAIL_FWD(NR) \
  mvptail_fwd_kernel<NR><<<grid, 256, 0, s>>>(p, x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, slot, live, out)
  if (!x_rgb) MVPTAIL_FWD(0);
  else if (3 * TD <= 16) MVPTAIL_FWD(1);
  else MVPTAIL_FWD(2);
#undef MVPTAIL_FWD
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" long long gol_mvp_tail_bwd_scratch_floats(int B, int h, int w, int TD, int C) {
  if (B <= 0 || h <= 0 || w <= 0 || TD <= 0 || (C != 1 && C != 4)) return 0;
  const Scratch s = scratch_layout(B, h, w, TD, C);
  return s.gpre_rgb + s.gpre_alpha + s.part;
}

extern "C" int gol_mvp_tail_bwd(int B, int Ci, int h, int w, int TD, int TH, int TW, int ny, int nx, int C,
                                const float* x_rgb, const float* w_rgb_t, const float* x_alpha, const float* w_alpha_t,
                                const int32_t* slot, const int32_t* live, int Kout, float rgb_scale, const float* g_out,
                                const float* out, float* g_x_rgb, float* g_x_alpha, float* g_w_rgb, float* g_w_alpha,
                                float* g_bias_rgb, float* g_bias_alpha, float* scratch, void* stream) {
  const int rc = check_common(__func__, B, Ci, h, w, TD, TH, TW, ny, nx, Kout);
  if (rc != GOL_OK) return rc;
  GOL_REQUIRE(C == 1 || C == 4, "C is 4 (colour + alpha) or 1 (alpha only)");
  GOL_REQUIRE(slot || Kout == ny * nx, "identity slots (slot == NULL) need Kout == ny nx");
  GOL_REQUIRE(C == 4 || (!g_x_rgb && !g_w_rgb && !g_bias_rgb), "the one-channel template has no colour gradients");
  hipStream_t s = (hipStream_t)stream;
  const size_t HWi = (size_t)h * w, HWo = 4 * HWi;
  if (B == 0 || Kout == 0 || !g_out) {  // nothing arrives: zeros
    struct { float* q; size_t n; } outs[6] = {{g_x_rgb, (size_t)B * kCi * HWi}, {g_x_alpha, (size_t)B * kCi * HWi},
                                              {g_w_rgb, (size_t)kCi * 3 * TD * 16}, {g_w_alpha, (size_t)kCi * TD * 16},
                                              {g_bias_rgb, (size_t)3 * TD * HWo}, {g_bias_alpha, (size_t)TD * HWo}};
    for (auto& o : outs)
      if (o.q && o.n && hipMemsetAsync(o.q, 0, sizeof(float) * o.n, s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  GOL_REQUIRE(out, "null pointer");
  GOL_REQUIRE(C == 1 || (gol_aligned16(g_out) && gol_aligned16(out)), "the four-channel g_out and out must be 16-byte aligned");
  const bool slab_rgb = g_x_rgb || g_w_rgb, slab_alpha = g_x_alpha || g_w_alpha;
  GOL_REQUIRE(!(slab_rgb || slab_alpha) || scratch, "g_x and g_w need scratch");
  GOL_REQUIRE(!g_x_rgb || w_rgb_t, "g_x_rgb needs w_rgb_t");
  GOL_REQUIRE(!g_x_alpha || w_alpha_t, "g_x_alpha needs w_alpha_t");
  GOL_REQUIRE(!g_w_rgb || x_rgb, "g_w_rgb needs x_rgb");
  GOL_REQUIRE(!g_w_alpha || x_alpha, "g_w_alpha needs x_alpha");
  const MvpTailDims p{B, h, w, TD, TH, TW, ny, nx, Kout, rgb_scale, 0.f};
  const Scratch lay = scratch_layout(B, h, w, TD, C);
  float* gpre_rgb = slab_rgb ? scratch : nullptr;
  float* gpre_alpha = slab_alpha ? scratch + lay.gpre_rgb : nullptr;
  float* part = scratch ? scratch + lay.gpre_rgb + lay.gpre_alpha : nullptr;
  if (gpre_rgb || gpre_alpha || g_bias_rgb || g_bias_alpha) {
    const dim3 grid(gol_cdiv((long long)TD * HWo, 256));
    if (C == 4) mvptail_gpre_kernel<4><<<grid, 256, 0, s>>>(p, slot, live, g_out, out, gpre_rgb, gpre_alpha, g_bias_rgb, g_bias_alpha);
    else mvptail_gpre_kernel<1><<<grid, 256, 0, s>>>(p, slot, live, g_out, out, gpre_rgb, gpre_alpha, g_bias_rgb, g_bias_alpha);
    GOL_CHECK_LAUNCH();
  }
  for (int br = 0; br < 2; ++br) {  // colour, then alpha
    const int CH = br == 0 ? 3 * TD : TD;
    const float* gpre = br == 0 ? gpre_rgb : gpre_alpha;
    float* g_x = br == 0 ? g_x_rgb : g_x_alpha;
    float* g_w = br == 0 ? g_w_rgb : g_w_alpha;
    if (g_x) {
      mvptail_bwd_x_kernel<<<dim3(gol_cdiv(w, 256), h, B), 256, 0, s>>>(h, w, CH, br == 0 ? w_rgb_t : w_alpha_t, gpre, g_x);
      GOL_CHECK_LAUNCH();
    }
    if (g_w) {
      const int nt = gol_cdiv(CH, 16), nblk = bwd_w_blocks(B, h, w, nt);
      mvptail_bwd_w_kernel<<<dim3(nblk, nt), 256, 0, s>>>(B, h, w, CH, br == 0 ? x_rgb : x_alpha, gpre, part);
      GOL_CHECK_LAUNCH();
      mvptail_bwd_w_reduce_kernel<<<dim3(256, nt), 256, 0, s>>>(CH, nblk, part, g_w);
      GOL_CHECK_LAUNCH();
    }
  }
  return GOL_OK;
}
