// featenc.hip -- the front of URHand's FeatEncoderUNet as one operator, forward and backward, gfx950.
//
// FeatEncoderUNet.forward (ca_code/models/urhand.py:98-107, layers built at :91-93; ca_code/nn/layers.py:470) starts with
//     h = proj(x)          Conv2dWN(Cx -> Cm, 7, 1, 3, bias=False)        [B,Cm,H,W]
//     y = feat_mod[0](h)   Conv2dWN(Cm -> Co, 4, 2, 1, bias=False)        [B,Co,H/2,W/2]
// two MIOpen convolutions with nothing between them.  At the model's size (4 -> 64 -> 192 at 1024^2) h is 268 MB per view,
// written once, read once and kept for the weight gradient; its gradient g_h is a second tensor of that size.  Here h and
// g_h exist per tile on chip only (the recipe of mbconv.hip: recompute the wide intermediate per tile):
//     h[b,m,r,c]  = sum_{cx,ky,kx} xpad[b,cx,r-3+ky,c-3+kx] w_p[m,cx,ky,kx]           (xpad = x inside the image, 0 outside)
//     y[b,co,Y,X] = sum_{m,ky,kx}  hpad[b,m,2Y-1+ky,2X-1+kx] w_f[co,m,ky,kx]          (hpad = h inside the image, 0 outside:
//                                                                   NOT the 7x7 response of the zero-extended x out there)
// All GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32): A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15],
// D[i = 4 (lane >> 4) + r][j].
//   fwd     a workgroup = one view x 8x8 output pixels x a group of output channels.  The 24x24 window of x (all Cx
//           planes) is staged once; per K stage of 16 channels m the 18x18 region of h the tile reads is formed by GEMM 1
//           (D[m][position], K = (cx,ky,kx) in steps of 4, zero-padded on the WEIGHT side: no channel of x that does not
//           exist is read), masked to the image and left in LDS (21 KB); GEMM 2 is the row gather of gol_conv4s2.h from
//           that region: lane (pixel j, row g) holds h[m][2Y-1+g][2X-1+kx], a wave owns output-channel tiles and all four
//           16-pixel tiles of the workgroup, w_f arrives as one 16-byte load per (channel, m) row of four taps.
//           Recompute factor of GEMM 1: 21 position tiles of 16 for 256 fresh positions = 1.31.
//   bwd     the two weight gradients are independent sums and run as two kernels (either may be left out):
//     w_f     g_w_f[co,m,tap] = sum_{b,Y,X} g_y[b,co,Y,X] hpad[b,m,2Y-1+ky,2X-1+kx]: a workgroup owns (16 m x 64 co) and
//             walks a run of 8x8 tiles; per tile h[16 m][18x18] is recomputed as in the forward, g_y[64 co][64 pixels] is
//             staged, a wave owns 16 co and keeps 16 accumulator tiles (one per tap), K = the 64 pixels.
//     w_p     g_w_p[m,cx,ky,kx] = sum_{b,r,c} g_h[b,m,r,c] xpad[b,cx,r-3+ky,c-3+kx]: a workgroup owns 16 m and walks a run
//             of 16x16 blocks of h positions; per block g_h[16 m][256] = the stride-2 transposed convolution of g_y in
//             the quad form of gol_conv4s2.h (a wave = one parity class, K = (co, 2x2 taps), g_y staged in chunks of 16
//             co), masked to the image, left in LDS, then D[m][(cx,ky,kx)] += g_h[m][position] x[position + tap], K = the
//             256 positions, the 22x22 window of x staged per block.
//   The partial sums of a workgroup leave to scratch once, at the end of its run, and a second kernel adds them in a fixed
//   order: no float atomics, bitwise reproducible.
#include "gol_conv4s2.h"

namespace {

struct FeDims {
  int B, Cx, Cm, Co, H, W;  // x [B,Cx,H,W] -> y [B,Co,H/2,W/2]
};

constexpr int kMaxCx = 8;
constexpr int kMaxK = kMaxCx * 49;  // 392 = the longest reduction of GEMM 1 (a multiple of 4)
constexpr int kXW = 24;             // forward window of x: 18 + 6
constexpr int kXPlane = kXW * kXW;
constexpr int kHW = 18;             // region of h an 8x8 output tile reads
constexpr int kHPos = kHW * kHW;    // 324 positions, 21 tiles of 16
constexpr int kHTiles = (kHPos + 15) / 16;
constexpr int kHPlane = kHPos;      // even (8-byte reads) and == 4 (mod 64): in the w_f gradient the 8-byte reads of a half
                                    // wave (16 planes x 2 neighbouring pixels) cover the 64 banks once
constexpr int kGRow = 68;           // g_y[co][64 pixels], == 4 (mod 32)
constexpr int kQW = 22;             // w_p gradient: window of x of a 16x16 block of positions
constexpr int kQPlane = kQW * kQW;
constexpr int kGhRow = 260;         // g_h[m][256 positions], == 4 (mod 32)
constexpr int kGyW = 10;            // region of g_y a 16x16 block of positions reads
constexpr int kGyPlane = kGyW * kGyW + 1;

// s_koff[kk] = offset of reduction index kk = (cx, ky, kx) inside a staged window of x (0 for the zero-weight padding)
__device__ __forceinline__ void fe_fill_koff(int* s_koff, int K, int plane, int row) {
  for (int kk = threadIdx.x; kk < kMaxK; kk += 256) {
    const int cx = kk / 49, rem = kk - cx * 49, ky = rem / 7, kx = rem - ky * 7;
    s_koff[kk] = kk < K ? cx * plane + ky * row + kx : 0;
  }
}

// window [Cx][n][n] of view b with its first element at (r0, c0) of the image, zeros outside
__device__ __forceinline__ void fe_load_window(float* s_x, const FeDims& p, const float* __restrict__ px, int b, int r0,
                                               int c0, int n) {
  const size_t HWi = (size_t)p.H * p.W;
  const float* xb = px + (size_t)b * p.Cx * HWi;
  const int nn = n * n;
  for (int e = threadIdx.x; e < p.Cx * nn; e += 256) {
    const int cx = e / nn, rem = e - cx * nn, lr = rem / n, lc = rem - lr * n;
    const int r = r0 + lr, c = c0 + lc;
    const bool ok = r >= 0 && r < p.H && c >= 0 && c < p.W;
    s_x[e] = ok ? xb[(size_t)cx * HWi + (size_t)r * p.W + c] : 0.f;
  }
}

// GEMM 1: hpad[16 m from m0][18x18] of the tile whose region starts at (hr0, hc0) = (2 Y0 - 1, 2 X0 - 1) -> s_h.
// s_x = the 24x24 window at (hr0 - 3, hc0 - 3).  Wave w takes position tiles w, w + 4, ...; the A operand (w_p, 16 m x 4
// reduction indices) comes from global memory (a few KB, L1-resident) one step ahead of its use.
__device__ __forceinline__ void fe_stage_h(const FeDims& p, const float* __restrict__ pwp, int m0, int hr0, int hc0,
                                           const float* s_x, const int* s_koff, float* s_h) {
  constexpr int NT = (kHTiles + 3) / 4;  // 6
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  const int K = p.Cx * 49, ksteps = (K + 3) >> 2;
  int poff[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int pos = min((wave + 4 * u) * 16 + i, kHPos - 1), hr = pos / kHW;
    poff[u] = hr * kXW + (pos - hr * kHW);
  }
  f32x4 acc[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* wrow = pwp + (size_t)(m0 + i) * K;
  float a = kq < K ? wrow[min(kq, K - 1)] : 0.f;
  for (int s = 0; s < ksteps; ++s) {
    const int kn = 4 * (s + 1) + kq;
    const float an = kn < K ? wrow[min(kn, K - 1)] : 0.f;  // (past the end: the zero weights of the padded K stage)
    const int koff = s_koff[4 * s + kq];
#pragma unroll
    for (int u = 0; u < NT; ++u)
      if (wave + 4 * u < kHTiles)  // wave-uniform
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_x[koff + poff[u]], acc[u], 0, 0, 0);
    a = an;
  }
  // D row = channel 4 kq + r, column = position i of the tile; outside the image h is ZERO
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int pos = (wave + 4 * u) * 16 + i;
    if (wave + 4 * u < kHTiles && pos < kHPos) {
      const int hr = pos / kHW, hc = pos - hr * kHW, r = hr0 + hr, c = hc0 + hc;
      const bool in = r >= 0 && r < p.H && c >= 0 && c < p.W;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) s_h[(4 * kq + r4) * kHPlane + pos] = in ? acc[u][r4] : 0.f;
    }
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
// grid (8x8 output tiles, B, groups of 4 NCW channel tiles).  Wave w owns channel tiles (group) 4 NCW + w NCW + u and all
// four pixel tiles (pixel tile pt = output rows 2 pt, 2 pt + 1 of the workgroup's 8x8): NCW x 4 accumulators.
// GEMM 2, per channel m of the stage: K = the 16 taps in 4 steps; step s is tap column kx = s, K slot kq is tap row ky = kq.
// A: lane (channel i, kq) loads w_f[co][m][ky = kq][0..3] (16 bytes) and uses component s in step s.
// B: lane (pixel j, kq) reads h[m][2 Yl + kq][2 Xl + s] of the region (two 8-byte reads for the four s).
template <int NCW>
__global__ __launch_bounds__(256) void featenc_fwd_kernel(const FeDims p, int tilesX, const float* __restrict__ px,
                                                          const float* __restrict__ pwp, const float* __restrict__ pwf,
                                                          float* __restrict__ py) {
  __shared__ __attribute__((aligned(16))) float s_x[kMaxCx * kXPlane];
  __shared__ __attribute__((aligned(16))) float s_h[16 * kHPlane];
  __shared__ int s_koff[kMaxK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kq = lane >> 4;
  const int tY = blockIdx.x / tilesX, tX = blockIdx.x - tY * tilesX, b = blockIdx.y;
  const int Y0 = 8 * tY, X0 = 8 * tX, Ho = p.H >> 1, Wo = p.W >> 1, Cm = p.Cm, nt = p.Co >> 4;
  const int ct0 = (blockIdx.z * 4 + wave) * NCW;
  fe_fill_koff(s_koff, p.Cx * 49, kXPlane, kXW);
  fe_load_window(s_x, p, px, b, 2 * Y0 - 4, 2 * X0 - 4, kXW);

  f32x4 acc[NCW][4];
#pragma unroll
  for (int u = 0; u < NCW; ++u)
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[u][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // this lane's A rows: channel (ct0 + u) 16 + i (a tile past Co re-reads the last one and is dropped below)
  const float* wf[NCW];
#pragma unroll
  for (int u = 0; u < NCW; ++u) wf[u] = pwf + ((size_t)(min(ct0 + u, nt - 1) * 16 + i) * Cm) * 16 + 4 * kq;
  int hoff[4];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) hoff[pt] = (2 * (2 * pt + (i >> 3)) + kq) * kHW + 2 * (i & 7);

  for (int m0 = 0; m0 < Cm; m0 += 16) {
    __syncthreads();  // the window is staged / the previous stage's region has been consumed
    fe_stage_h(p, pwp, m0, 2 * Y0 - 1, 2 * X0 - 1, s_x, s_koff, s_h);
    __syncthreads();
    if (ct0 >= nt) continue;  // wave-uniform: a wave without a channel tile only helps with GEMM 1
    float4 a[NCW];
#pragma unroll
    for (int u = 0; u < NCW; ++u) a[u] = *reinterpret_cast<const float4*>(wf[u] + (size_t)m0 * 16);
#pragma unroll 2
    for (int ml = 0; ml < 16; ++ml) {
      float4 an[NCW];
      const int mn = min(m0 + ml + 1, Cm - 1);
#pragma unroll
      for (int u = 0; u < NCW; ++u) an[u] = *reinterpret_cast<const float4*>(wf[u] + (size_t)mn * 16);
      float bv[4][4];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const float* hp = &s_h[ml * kHPlane + hoff[pt]];
        const float2 t0 = *reinterpret_cast<const float2*>(hp), t1 = *reinterpret_cast<const float2*>(hp + 2);
        bv[pt][0] = t0.x; bv[pt][1] = t0.y; bv[pt][2] = t1.x; bv[pt][3] = t1.y;
      }
#pragma unroll
      for (int u = 0; u < NCW; ++u) {
        const float av[4] = {a[u].x, a[u].y, a[u].z, a[u].w};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
            acc[u][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[pt][s], acc[u][pt], 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < NCW; ++u) a[u] = an[u];
    }
  }
  // D row = channel 16 ct + 4 kq + r, column = pixel i of pixel tile pt
  const size_t HWo = (size_t)Ho * Wo;
#pragma unroll
  for (int u = 0; u < NCW; ++u) {
    if (ct0 + u >= nt) continue;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int Y = Y0 + 2 * pt + (i >> 3), X = X0 + (i & 7);
      if (Y >= Ho || X >= Wo) continue;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        py[((size_t)b * p.Co + (ct0 + u) * 16 + 4 * kq + r4) * HWo + (size_t)Y * Wo + X] = acc[u][pt][r4];
    }
  }
}

// the run of tiles of K block blockIdx.x: [t0, t1)
__device__ __forceinline__ void fe_run(long long ntiles, int& t0, int& t1) {
  const long long per = (ntiles + gridDim.x - 1) / gridDim.x;
  const long long a = min((long long)blockIdx.x * per, ntiles);
  t0 = (int)a;
  t1 = (int)min(a + per, ntiles);
}

// ---- gradient of w_f ---------------------------------------------------------------------------------------------------
// grid (K blocks, (Cm / 16) x groups of 4 channel tiles).  Wave w owns channel tile 4 group + w: acc[tap] is D[co][m].
// Per tile, K = the 64 pixels in 16 steps: A lane (co i, kq) = g_y[co][pixel 4 s + kq], B lane (m j, kq) = the 4x4 taps of
// h[m] at that pixel (four rows of two 8-byte reads).  scratch: [group][wave][K block][16 taps][16 co x 16 m].
__global__ __launch_bounds__(256) void featenc_bwd_wf_kernel(const FeDims p, int tilesX, int tilesY,
                                                             const float* __restrict__ px, const float* __restrict__ pwp,
                                                             const float* __restrict__ pg, float* __restrict__ pscratch) {
  __shared__ __attribute__((aligned(16))) float s_x[kMaxCx * kXPlane];
  __shared__ __attribute__((aligned(16))) float s_h[16 * kHPlane];
  __shared__ __attribute__((aligned(16))) float s_g[64 * kGRow];
  __shared__ int s_koff[kMaxK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kq = lane >> 4;
  const int Ho = p.H >> 1, Wo = p.W >> 1, Co = p.Co, nt = Co >> 4;
  const int ncog = (nt + 3) >> 2, mb = blockIdx.y / ncog, cog = blockIdx.y - mb * ncog;
  const bool ctv = cog * 4 + wave < nt;
  const size_t HWo = (size_t)Ho * Wo;
  fe_fill_koff(s_koff, p.Cx * 49, kXPlane, kXW);
  f32x4 acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tpv = tilesX * tilesY;
  int t0, t1;
  fe_run((long long)p.B * tpv, t0, t1);
  for (int tile = t0; tile < t1; ++tile) {
    const int b = tile / tpv, rem = tile - b * tpv, tY = rem / tilesX, Y0 = 8 * tY, X0 = 8 * (rem - tY * tilesX);
    __syncthreads();  // the previous tile's operands have been consumed
    fe_load_window(s_x, p, px, b, 2 * Y0 - 4, 2 * X0 - 4, kXW);
    for (int e = tid; e < 64 * 64; e += 256) {
      const int cl = e >> 6, pix = e & 63, co = cog * 64 + cl, Y = Y0 + (pix >> 3), X = X0 + (pix & 7);
      const bool ok = co < Co && Y < Ho && X < Wo;
      s_g[cl * kGRow + pix] = ok ? pg[((size_t)b * Co + co) * HWo + (size_t)Y * Wo + X] : 0.f;
    }
    __syncthreads();
    fe_stage_h(p, pwp, mb * 16, 2 * Y0 - 1, 2 * X0 - 1, s_x, s_koff, s_h);
    __syncthreads();
    if (!ctv) continue;  // wave-uniform
#pragma unroll 2
    for (int s = 0; s < 16; ++s) {
      const float ga = s_g[(wave * 16 + i) * kGRow + 4 * s + kq];
      const float* hp = &s_h[i * kHPlane + (2 * (s >> 1)) * kHW + 2 * (4 * (s & 1) + kq)];
#pragma unroll
      for (int ky = 0; ky < 4; ++ky) {
        const float2 u0 = *reinterpret_cast<const float2*>(hp + ky * kHW), u1 = *reinterpret_cast<const float2*>(hp + ky * kHW + 2);
        acc[ky * 4 + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, u0.x, acc[ky * 4 + 0], 0, 0, 0);
        acc[ky * 4 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, u0.y, acc[ky * 4 + 1], 0, 0, 0);
        acc[ky * 4 + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, u1.x, acc[ky * 4 + 2], 0, 0, 0);
        acc[ky * 4 + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, u1.y, acc[ky * 4 + 3], 0, 0, 0);
      }
    }
  }
  if (!ctv) return;
  // D[co 4 kq + r][m i] of every tap -> this wave's partial of this K block
  float* dst = pscratch + ((((size_t)blockIdx.y * 4 + wave) * gridDim.x + blockIdx.x) * 16) * 256;
#pragma unroll
  for (int t = 0; t < 16; ++t)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) dst[(size_t)t * 256 + (4 * kq + r4) * 16 + i] = acc[t][r4];
}

// g_w_f[co,m,tap] = sum over the K blocks (written once).  grid (16 taps x 16 co rows, (group, wave) channel-tile pairs)
__global__ __launch_bounds__(256) void featenc_bwd_wf_reduce_kernel(const FeDims p, int nblk,
                                                                    const float* __restrict__ scratch,
                                                                    float* __restrict__ gw) {
  const int tap = blockIdx.x >> 4, row = blockIdx.x & 15, cl = threadIdx.x & 15;
  const int nt = p.Co >> 4, ncog = (nt + 3) >> 2, grp = blockIdx.y >> 2, wv = blockIdx.y & 3;
  const int mb = grp / ncog, cog = grp - mb * ncog, ct = cog * 4 + wv;
  if (ct >= nt) return;  // block-uniform: a wave without a channel tile wrote nothing
  const int co = ct * 16 + row, m = mb * 16 + cl;
  wgrad_reduce16(scratch + (((size_t)blockIdx.y * nblk) * 16 + tap) * 256 + row * 16 + cl, nblk,
                 gw + ((size_t)co * p.Cm + m) * 16 + tap, true);
}

// ---- gradient of w_p ---------------------------------------------------------------------------------------------------
// grid (K blocks, Cm / 16).  A block of 16x16 positions of h starts at (2 Y0, 2 X0) (Y0, X0 multiples of 8 of the output).
// Position (2 u + e, 2 v + f) of the block is hit by the taps ky = 1 - e + 2 ty, kx = 1 - f + 2 tx of the output pixels
// (Y0 + u + e - ty, X0 + v + f - tx), ty, tx in {0, 1}: wave w is the parity class (e, f) = (w >> 1, w & 1), its 64
// positions are four tiles of 16 (tile pt = rows u = 2 pt, 2 pt + 1).
// GEMM A (g_h): K slot kq = (co parity kq & 1, ty = kq >> 1) of a PAIR of output channels, step s = tx: lane (m i, kq) loads
//   w_f[co][m][ky][0..3] (16 bytes) once per pair and uses components 1 - f and 3 - f; B lane (position j, kq) reads g_y of
//   the staged 10x10 region (origin (Y0 - 1, X0 - 1), zeros outside the output).
// GEMM B: D[m][(cx,ky,kx)] += g_h[m][position] x[position + tap], K = the 256 positions in 64 steps; column tile t of the
//   ceil(49 Cx / 16) goes to wave t % 4; columns past 49 Cx read x[0] and are dropped by the reduce kernel.
// scratch: [Cm / 16][K block][column tile][16 m x 16 columns].
template <int MAXT>
__global__ __launch_bounds__(256) void featenc_bwd_wp_kernel(const FeDims p, int tilesX, int tilesY,
                                                             const float* __restrict__ px, const float* __restrict__ pwf,
                                                             const float* __restrict__ pg, float* __restrict__ pscratch) {
  __shared__ __attribute__((aligned(16))) float s_x[kMaxCx * kQPlane];
  __shared__ __attribute__((aligned(16))) float s_gh[16 * kGhRow];
  __shared__ __attribute__((aligned(16))) float s_gy[16 * kGyPlane];
  __shared__ int s_koff[kMaxK + 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kq = lane >> 4;
  const int H = p.H, W = p.W, Ho = H >> 1, Wo = W >> 1, Co = p.Co, Cm = p.Cm, K = p.Cx * 49, ntc = (K + 15) >> 4;
  const int m0 = blockIdx.y * 16, e = wave >> 1, f = wave & 1, ty = kq >> 1;
  const size_t HWo = (size_t)Ho * Wo;
  fe_fill_koff(s_koff, K, kQPlane, kQW);
  if (tid < 16) s_koff[kMaxK + tid] = 0;
  __syncthreads();
  int koffv[MAXT];
#pragma unroll
  for (int u = 0; u < MAXT; ++u) koffv[u] = s_koff[min((wave + 4 * u) * 16 + i, kMaxK + 15)];
  f32x4 acc[MAXT];
#pragma unroll
  for (int u = 0; u < MAXT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  // A rows of GEMM A: channel co = pair + (kq & 1), row ky = 1 - e + 2 ty, channel m0 + i
  const float* wf = pwf + ((size_t)(kq & 1) * Cm + m0 + i) * 16 + 4 * (1 - e + 2 * ty);
  int goff[4][2];  // g_y of (position j of tile pt, tx)
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int s = 0; s < 2; ++s)
      goff[pt][s] = (kq & 1) * kGyPlane + (2 * pt + (i >> 3) + e - ty + 1) * kGyW + (i & 7) + f - s + 1;
  const int tpv = tilesX * tilesY;
  int t0, t1;
  fe_run((long long)p.B * tpv, t0, t1);
  for (int tile = t0; tile < t1; ++tile) {
    const int b = tile / tpv, rem = tile - b * tpv, tY = rem / tilesX, Y0 = 8 * tY, X0 = 8 * (rem - tY * tilesX);
    __syncthreads();  // the previous block's window and g_h have been consumed
    fe_load_window(s_x, p, px, b, 2 * Y0 - 3, 2 * X0 - 3, kQW);
    f32x4 gacc[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) gacc[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int cc = 0; cc < Co; cc += 16) {
      float4 a4[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) a4[q] = *reinterpret_cast<const float4*>(wf + (size_t)(cc + 2 * q) * Cm * 16);
      __syncthreads();  // the previous chunk of g_y has been consumed
      for (int el = tid; el < 16 * kGyW * kGyW; el += 256) {
        const int cl = el / (kGyW * kGyW), r2 = el - cl * (kGyW * kGyW), ly = r2 / kGyW, lx = r2 - ly * kGyW;
        const int Y = Y0 - 1 + ly, X = X0 - 1 + lx;
        const bool ok = Y >= 0 && Y < Ho && X >= 0 && X < Wo;
        s_gy[cl * kGyPlane + r2] = ok ? pg[((size_t)b * Co + cc + cl) * HWo + (size_t)Y * Wo + X] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float as[2] = {f ? a4[q].x : a4[q].y, f ? a4[q].z : a4[q].w};  // kx = 1 - f + 2 tx
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
            gacc[pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[s], s_gy[2 * q * kGyPlane + goff[pt][s]], gacc[pt], 0, 0, 0);
      }
    }
    // D row = channel 4 kq + r, column = position i of tile pt; g_h is restricted to the image
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int pr = 2 * (2 * pt + (i >> 3)) + e, pc = 2 * (i & 7) + f;
      const bool in = 2 * Y0 + pr < H && 2 * X0 + pc < W;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) s_gh[(4 * kq + r4) * kGhRow + pr * 16 + pc] = in ? gacc[pt][r4] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < 64; ++s) {
      const int pos = 4 * s + kq, xo = (pos >> 4) * kQW + (pos & 15);
      const float ga = s_gh[i * kGhRow + pos];
#pragma unroll
      for (int u = 0; u < MAXT; ++u)
        if (wave + 4 * u < ntc)  // wave-uniform
          acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, s_x[koffv[u] + xo], acc[u], 0, 0, 0);
    }
  }
#pragma unroll
  for (int u = 0; u < MAXT; ++u) {
    const int t = wave + 4 * u;
    if (t >= ntc) continue;
    float* dst = pscratch + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ntc + t) * 256;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) dst[(4 * kq + r4) * 16 + i] = acc[u][r4];
  }
}

// g_w_p[m,(cx,ky,kx)] = sum over the K blocks in block order, one thread per element
__global__ __launch_bounds__(256) void featenc_bwd_wp_reduce_kernel(const FeDims p, int nblk,
                                                                    const float* __restrict__ scratch,
                                                                    float* __restrict__ gw) {
  const int K = p.Cx * 49, ntc = (K + 15) >> 4, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= p.Cm * K) return;
  const int m = n / K, col = n - m * K;
  const float* src = scratch + (((size_t)(m >> 4) * nblk) * ntc + (col >> 4)) * 256 + (m & 15) * 16 + (col & 15);
  float acc = 0.f;
  for (int k = 0; k < nblk; ++k) acc += src[(size_t)k * ntc * 256];
  gw[n] = acc;
}

bool fe_supported(int Cx, int Cm, int Co, int H, int W) {
  return Cx >= 1 && Cx <= kMaxCx && Cm > 0 && Cm % 16 == 0 && Co > 0 && Co % 16 == 0 && H >= 2 && W >= 2 && H % 2 == 0 &&
         W % 2 == 0;
}

int fe_check(int B, int Cx, int Cm, int Co, int H, int W) {
  GOL_REQUIRE(B >= 0, "bad sizes");
  if (!fe_supported(Cx, Cm, Co, H, W) || B > 65535) {
    gol_set_error("gol_featenc_front: Cx must be 1..8, Cm and Co multiples of 16, H and W even and >= 2, B <= 65535 (got "
                  "%d x %d -> %d -> %d at %d x %d)", B, Cx, Cm, Co, H, W);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE((long long)B * gol_cdiv(H / 2, 8) * gol_cdiv(W / 2, 8) < (1ll << 31), "too many tiles");
  GOL_REQUIRE((long long)(Cm / 16) * gol_cdiv(Co / 16, 4) * 4 <= 65535, "too many channel tiles");
  return GOL_OK;
}

// K blocks: at most ONE round of the 512 workgroups that are resident (2 per CU: LDS in the w_f kernel, registers in the w_p
// kernel) over the channel groups -- rounded DOWN: 43 blocks x 12 groups = 516 workgroups would leave 4 for a second round
// that takes as long as the first -- and at most one per tile
int fe_blocks(long long ntiles, int groups) {
  const long long nblk = 512 / groups;
  return (int)(nblk < 1 ? 1 : (nblk > ntiles ? ntiles : nblk));
}
int fe_wf_groups(int Cm, int Co) { return (Cm / 16) * gol_cdiv(Co / 16, 4); }
int fe_wf_blocks(long long ntiles, int Cm, int Co) { return fe_blocks(ntiles, fe_wf_groups(Cm, Co)); }
int fe_wp_blocks(long long ntiles, int Cm) { return fe_blocks(ntiles, Cm / 16); }
long long fe_wf_floats(long long ntiles, int Cm, int Co) {
  return (long long)fe_wf_groups(Cm, Co) * 4 * fe_wf_blocks(ntiles, Cm, Co) * 16 * 256;
}

}  // namespace

extern "C" int gol_featenc_front_fwd(int B, int Cx, int Cm, int Co, int H, int W, const float* x, const float* w_p,
                                     const float* w_f, float* y, void* stream) {
  const int rc = fe_check(B, Cx, Cm, Co, H, W);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && w_p && w_f && y, "null pointer");
  GOL_REQUIRE(gol_aligned16(w_f), "w_f must be 16-byte aligned");
  const FeDims p{B, Cx, Cm, Co, H, W};
  hipStream_t s = (hipStream_t)stream;
  const int tilesX = gol_cdiv(W / 2, 8), tilesY = gol_cdiv(H / 2, 8), nt = Co / 16;
  if (nt > 4)
    featenc_fwd_kernel<3><<<dim3(tilesX * tilesY, B, gol_cdiv(nt, 12)), 256, 0, s>>>(p, tilesX, x, w_p, w_f, y);
  else
    featenc_fwd_kernel<1><<<dim3(tilesX * tilesY, B, 1), 256, 0, s>>>(p, tilesX, x, w_p, w_f, y);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" long long gol_featenc_front_bwd_scratch_floats(int B, int Cx, int Cm, int Co, int H, int W) {
  if (B <= 0 || B > 65535 || !fe_supported(Cx, Cm, Co, H, W)) return 0;
  const long long ntiles = (long long)B * gol_cdiv(H / 2, 8) * gol_cdiv(W / 2, 8);
  return fe_wf_floats(ntiles, Cm, Co) + (long long)(Cm / 16) * fe_wp_blocks(ntiles, Cm) * gol_cdiv(Cx * 49, 16) * 256;
}

extern "C" int gol_featenc_front_bwd(int B, int Cx, int Cm, int Co, int H, int W, const float* x, const float* w_p,
                                     const float* w_f, const float* g_y, float* g_w_p, float* g_w_f, float* scratch,
                                     void* stream) {
  const int rc = fe_check(B, Cx, Cm, Co, H, W);
  if (rc != GOL_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {  // empty sums
    if (g_w_p && hipMemsetAsync(g_w_p, 0, sizeof(float) * Cm * Cx * 49, s) != hipSuccess) return GOL_ERR_LAUNCH;
    if (g_w_f && hipMemsetAsync(g_w_f, 0, sizeof(float) * Co * Cm * 16, s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  if (!g_w_p && !g_w_f) return GOL_OK;
  GOL_REQUIRE(x && g_y && scratch, "null pointer");
  GOL_REQUIRE(!g_w_f || w_p, "g_w_f needs w_p");
  GOL_REQUIRE(!g_w_p || (w_f && gol_aligned16(w_f)), "g_w_p needs w_f (16-byte aligned)");
  const FeDims p{B, Cx, Cm, Co, H, W};
  const int tilesX = gol_cdiv(W / 2, 8), tilesY = gol_cdiv(H / 2, 8);
  const long long ntiles = (long long)B * tilesX * tilesY;
  if (g_w_f) {
    const int groups = fe_wf_groups(Cm, Co), nblk = fe_wf_blocks(ntiles, Cm, Co);
    featenc_bwd_wf_kernel<<<dim3(nblk, groups), 256, 0, s>>>(p, tilesX, tilesY, x, w_p, g_y, scratch);
    GOL_CHECK_LAUNCH();
    featenc_bwd_wf_reduce_kernel<<<dim3(256, groups * 4), 256, 0, s>>>(p, nblk, scratch, g_w_f);
    GOL_CHECK_LAUNCH();
  }
  if (g_w_p) {
    float* sp = scratch + fe_wf_floats(ntiles, Cm, Co);
    const int nblk = fe_wp_blocks(ntiles, Cm);
    const dim3 grid(nblk, Cm / 16);
    if (Cx <= 4) featenc_bwd_wp_kernel<4><<<grid, 256, 0, s>>>(p, tilesX, tilesY, x, w_f, g_y, sp);
    else featenc_bwd_wp_kernel<7><<<grid, 256, 0, s>>>(p, tilesX, tilesY, x, w_f, g_y, sp);
    GOL_CHECK_LAUNCH();
    featenc_bwd_wp_reduce_kernel<<<dim3(gol_cdiv((long long)Cm * Cx * 49, 256)), 256, 0, s>>>(p, nblk, sp, g_w_p);
    GOL_CHECK_LAUNCH();
  }
  return GOL_OK;
}
