// conv4x.hip -- a linear, bias-free 4x4 / stride 2 / pad 1 convolution at precision "bf16x3" with all three products:
// forward, input gradient and weight gradient.  The feature layers feat_mod[0..3] of URHand's FeatEncoderUNet
// (ca_code/models/urhand.py:93, :102; la.Conv2dWN, ca_code/nn/layers.py:470) on the EFFECTIVE weight, gfx950, wave64.
//     y[b,co,Y,X] = sum_{ci,ky,kx} xpad[b,ci,2Y-1+ky,2X-1+kx] w[co,ci,ky,kx]        x [B,Ci,H,W] -> y [B,Co,H/2,W/2]
// The arithmetic and the conventions are those of conv3x.hip (read its header): v_mfma_f32_16x16x32_bf16, every operand
// split into hi = bf16_rne(v), lo = bf16_rne(v - hi) while it is staged, three MFMAs per product (lo lo dropped), fp32
// accumulation, zero padding splits to (0,0); lane (j = lane & 15, g = lane >> 4) holds A[row j][k = 8 g .. 8 g + 7] and
// B[k = 8 g .. 8 g + 7][column j], D[row 4 g + r][column j]; every LDS image has 64-byte rows (32 bf16 = the K of one MFMA)
// and is read 16 bytes per lane through cx_slot.  Workgroups are 4 waves.  "Coarse" = the grid of y, "fine" = the grid of x.
//   pack    w -> packed[hi|lo][16 taps][Co / 8][Ci / 8][8 co][8 ci], once per call; ONE packing serves forward and input
//           gradient (which transposes a block in registers on its way to LDS).
//   fwd     implicit GEMM per tap, D[co][pixel] += w[co][ci][ky,kx] x[ci][2Y-1+ky][2X-1+kx], K stage = 32 channels.  A
//           workgroup owns 8 x 16 coarse pixels x 64 CW channels (CW = 2, or 1 where Co <= 64).  The haloed 18 x 34 fine
//           window goes to LDS pixel-major as in conv3x, but with the columns of a window row DE-INTERLEAVED BY PARITY
//           (position = row 34 + (col & 1) 17 + (col >> 1)): the 16 pixels of a B operand, two fine columns apart, are then
//           16 CONSECUTIVE positions and cx_slot is conflict-free for them as it stands -- the re-derived swizzle for the
//           stride is this permutation of the rows, not another XOR.  Window 78,336 B + the weights of one tap ROW (4 taps
//           x 64 CW rows x 32 k x hi, lo = 32 KB x CW): 110 KB (CW = 1) or 143,872 B (CW = 2), one workgroup per CU.
//           CW = 2: waves 0-1 take channels 0..63, waves 2-3 64..127, each 4 coarse rows = 4 pixel tiles x 4 channel tiles
//           (48 MFMAs per 16 ds_read_b128); CW = 1: each wave 2 rows x 4 channel tiles.  A wave whose 64 channels lie past
//           Co (Co = 192 = 128 + 64) issues no MFMA.
//   bwd_x   the quad form of gol_conv4s2.h: the fine pixel (2 i + a, 2 jj + q) of parity class (a, q) reads g_y at
//           (i + a - dy, jj + q - dx) through the tap (ky, kx) = (1 - a + 2 dy, 1 - q + 2 dx): per class a GEMM with M = Ci,
//           K = Co x 4 taps.  A workgroup owns 16 x 32 fine pixels (8 x 16 per class) x 64 channels; a wave two class rows of
//           ALL four classes (32 accumulator tiles), so a tap's A operand feeds 2 pixel tiles and g_x leaves as 8-byte
//           stores of the column pair (q = 0, 1).  The g_y window is 10 x 18 coarse positions (23 KB) + 32 KB of weights.
//   bwd_w   g_w[co][ci][tap] = sum_{b,Y,X} g_y[co][Y][X] x[ci][2Y-1+ky][2X-1+kx]: the GEMM's K is the PIXEL, so both operands
//           lie pixel-contiguous in LDS.  A chunk = 32 pixels of one coarse row; g_y goes to s_gy[hi|lo][64 co][32], x to
//           s_x[hi|lo][kx][4 fine rows][32 ci][32]: de-interleaved by column, image kx holds x[2X-1+kx] at X, so eight
//           consecutive pixels of one tap are one aligned 16-byte read.  A workgroup owns 64 co x 32 ci, a wave 32 x 16 = two
//           channel-tile pairs x 16 taps (32 accumulator tiles, 96 MFMAs per 36 reads).  K is split over workgroups
//           (contiguous runs of chunks); a partial [Co][Ci][16] leaves per workgroup and c4_reduce_kernel adds the
//           partials in block order.  Scratch = blocks x Co x Ci x 16 floats <= (512 + channel-tile pairs) x 32768 floats,
//           whatever B, H and W.
// No float atomics; every output element is a fixed-order sum: bitwise reproducible.  No host sync, no allocation.
#include "gol_splitbf16.h"

namespace {

struct C4Dims {
  int B, M, K, H, W, Ho, Wo;  // M rows of the GEMM (channels written), K channels read; fine and coarse size
};

constexpr int kKS = 32;                                 // channels per K stage = the K of one MFMA
constexpr int kTH = 8, kTW = 16;                        // coarse tile of fwd and bwd_x
constexpr int kFHR = 2 * kTH + 2, kFHC = 2 * kTW + 2;   // fwd: haloed fine window 18 x 34
constexpr int kFWin = kFHR * kFHC;                      // 612 positions
constexpr int kBHR = kTH + 2, kBHC = kTW + 2;           // bwd_x: haloed coarse window 10 x 18
constexpr int kBWin = kBHR * kBHC;                      // 180 positions
constexpr int kWPix = 32;                               // bwd_w: pixels per chunk
constexpr int kWCo = 64, kWCi = 32;                     // bwd_w: channels per workgroup
constexpr int kWTarget = 512;                           // bwd_w: workgroups aimed at (two per CU)

// 32 channels of a haloed window of an [.., HS, WS] plane stack, origin (r_org, c_org), split into s_in[hi|lo][position][32];
// outside the plane: zeros.  DEINT: the columns of a window row are stored by parity (the stride-2 B operand of fwd).  An
// item = one window position x 8 channels; the loads are unconditional (clamped to element 0, the value is dropped).
template <int HR, int HC, bool DEINT>
__device__ __forceinline__ void c4_stage(unsigned short* s_in, const float* __restrict__ in_b, int HS, int WS, int k0,
                                         int r_org, int c_org, int tid) {
  constexpr int WIN = HR * HC, N = (kKS / 8) * WIN;
  const size_t PS = (size_t)HS * WS;
  for (int idx = tid; idx < N; idx += 256) {
    const int q = idx / WIN, pos = idx - q * WIN, rr = pos / HC, cc = pos - rr * HC;
    const int r = r_org + rr, c = c_org + cc;
    const bool in = r >= 0 && r < HS && c >= 0 && c < WS;
    const unsigned o = in ? (unsigned)r * (unsigned)WS + (unsigned)c : 0u;
    float va[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) va[u] = in_b[(size_t)(k0 + q * 8 + u) * PS + o];  // every load first
    f32x8 v;
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = in ? va[u] : 0.f;
    bf16x8 hi, lo;
    cx_split(v, hi, lo);
    const int n = DEINT ? rr * HC + (cc & 1) * (HC / 2) + (cc >> 1) : pos;
    const int off = n * kKS + cx_slot(n, q) * 8;
    *reinterpret_cast<bf16x8*>(s_in + off) = hi;
    *reinterpret_cast<bf16x8*>(s_in + WIN * kKS + off) = lo;
  }
}

// the weights of tap row ky of a K stage as s_w[hi|lo][kx][MR rows][32 k], one packed 8 x 8 block per item.
// Forward: A[co][ci] = w[co][ci][tap], block (tap, co / 8, ci / 8) row by row.  TRANS: A[ci][co] = w[co][ci][tap]: block
// (tap, co / 8 = k block, ci / 8 = m block) transposed in registers.  Rows past M: zeros.
template <int MR, bool TRANS>
__device__ __forceinline__ void c4_stage_w(unsigned short* s_w, const C4Dims& p, const unsigned short* __restrict__ pw, int k0,
                                           int m0, int ky, int tid) {
  constexpr int MB = MR / 8, NBLK = 2 * 4 * MB * 4;
  const int M = p.M, K = p.K;
  for (int idx = tid; idx < NBLK; idx += 256) {
    const int kb = idx & 3, mb = (idx >> 2) % MB, rest = idx / (4 * MB), kx = rest & 3, plane = rest >> 2;
    const int tap = ky * 4 + kx, mblk = (m0 >> 3) + mb, kblk = (k0 >> 3) + kb;
    u32x4 row[8];
    if (mblk * 8 < M) {
      const size_t blk = TRANS ? (((size_t)plane * 16 + tap) * (K >> 3) + kblk) * (M >> 3) + mblk
                               : (((size_t)plane * 16 + tap) * (M >> 3) + mblk) * (K >> 3) + kblk;
      const u32x4* src = reinterpret_cast<const u32x4*>(pw + blk * 64);
#pragma unroll
      for (int r = 0; r < 8; ++r) row[r] = src[r];
      if constexpr (TRANS) {
        u32x4 t[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const unsigned e0 = (row[2 * d][c >> 1] >> (16 * (c & 1))) & 0xffffu;
            const unsigned e1 = (row[2 * d + 1][c >> 1] >> (16 * (c & 1))) & 0xffffu;
            t[c][d] = e0 | (e1 << 16);
          }
#pragma unroll
        for (int r = 0; r < 8; ++r) row[r] = t[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) row[r] = u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int m = mb * 8 + r;
      *reinterpret_cast<u32x4*>(s_w + ((plane * 4 + kx) * MR + m) * kKS + cx_slot(m, kb) * 8) = row[r];
    }
  }
}

// acc += A B in three bf16 products (hi lo + lo hi + hi hi), CT channel tiles against one pixel tile
template <int CT>
__device__ __forceinline__ void c4_mfma3(const bf16x8 (&ah)[CT], const bf16x8 (&al)[CT], const bf16x8 bh, const bf16x8 bl,
                                         f32x4 (&acc)[CT]) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ct], bl, acc[ct], 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[ct], bh, acc[ct], 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ct], bh, acc[ct], 0, 0, 0);
}

// the A operands (4 channel tiles, hi and lo) of tap column kx: rows mw + 16 ct + j of s_w[hi|lo][kx][MR][32]
template <int MR>
__device__ __forceinline__ void c4_read_a(const unsigned short* s_w, int kx, int mw, int j, int g, bf16x8 (&ah)[4],
                                          bf16x8 (&al)[4]) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int m = mw + ct * 16 + j, off = (kx * MR + m) * kKS + cx_slot(m, g) * 8;
    ah[ct] = *reinterpret_cast<const bf16x8*>(s_w + off);
    al[ct] = *reinterpret_cast<const bf16x8*>(s_w + 4 * MR * kKS + off);
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------------
// grid (coarse tiles of 8 x 16, B, groups of 64 CW output channels)
template <int CW>
__global__ __launch_bounds__(256) void c4_fwd_kernel(const C4Dims p, const float* __restrict__ px,
                                                     const unsigned short* __restrict__ pw, float* __restrict__ py) {
  constexpr int MR = 64 * CW, P = 2 * CW, PW = 4 / CW;
  __shared__ __attribute__((aligned(16))) unsigned short s_in[2 * kFWin * kKS];
  __shared__ __attribute__((aligned(16))) unsigned short s_w[2 * 4 * MR * kKS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int wp = wave % PW, mw = (wave / PW) * 64;
  const int M = p.M, K = p.K, Ho = p.Ho, Wo = p.Wo;
  const int ntx = (Wo + kTW - 1) / kTW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int Y0 = ty * kTH, X0 = tx * kTW, b = blockIdx.y, m0 = blockIdx.z * MR;
  const float* in_b = px + (size_t)b * K * ((size_t)p.H * p.W);
  const bool live = m0 + mw < M;  // wave-uniform
  f32x4 acc[P][4];
#pragma unroll
  for (int pt = 0; pt < P; ++pt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[pt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += kKS) {
    for (int ky = 0; ky < 4; ++ky) {
      __syncthreads();  // the previous tap row has been consumed
      if (ky == 0) c4_stage<kFHR, kFHC, true>(s_in, in_b, p.H, p.W, k0, 2 * Y0 - 1, 2 * X0 - 1, tid);
      c4_stage_w<MR, false>(s_w, p, pw, k0, m0, ky, tid);
      __syncthreads();
      if (live) {
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
          bf16x8 ah[4], al[4];
          c4_read_a<MR>(s_w, kx, mw, j, g, ah, al);
#pragma unroll
          for (int pt = 0; pt < P; ++pt) {  // fine (2 yl + ky, 2 j + kx): window row 2 yl + ky, parity kx & 1, half j + (kx >> 1)
            const int n = (2 * (wp * P + pt) + ky) * kFHC + (kx & 1) * (kFHC / 2) + j + (kx >> 1);
            const int off = n * kKS + cx_slot(n, g) * 8;
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(s_in + off);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(s_in + kFWin * kKS + off);
            c4_mfma3<4>(ah, al, bh, bl, acc[pt]);
          }
        }
      }
    }
  }
  if (!live) return;
  const size_t HWo = (size_t)Ho * Wo;
#pragma unroll
  for (int pt = 0; pt < P; ++pt) {
    const int Y = Y0 + wp * P + pt, X = X0 + j;
    if (Y >= Ho || X >= Wo) continue;
    const unsigned o = (unsigned)Y * (unsigned)Wo + (unsigned)X;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int m = m0 + mw + 16 * ct + 4 * g + r4;
        if (m < M) py[((size_t)b * M + m) * HWo + o] = acc[pt][ct][r4];
      }
  }
}

// ---- input gradient ------------------------------------------------------------------------------------------------------
// tap row KY of a K stage: class rows a = 1 - (KY & 1) through dy = KY >> 1; acc[a][q][row of the wave][channel tile]
template <int KY>
__device__ __forceinline__ void c4_bwd_x_step(unsigned short* s_in, unsigned short* s_w, const C4Dims& p,
                                              const float* __restrict__ in_b, const unsigned short* __restrict__ pw, int k0,
                                              int i0, int j0, int m0, int tid, f32x4 (&acc)[2][2][2][4]) {
  constexpr int a = 1 - (KY & 1), dy = KY >> 1;
  const int lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  __syncthreads();  // the previous tap row has been consumed
  if (KY == 0) c4_stage<kBHR, kBHC, false>(s_in, in_b, p.Ho, p.Wo, k0, i0 - 1, j0 - 1, tid);
  c4_stage_w<64, true>(s_w, p, pw, k0, m0, KY, tid);
  __syncthreads();
#pragma unroll
  for (int kx = 0; kx < 4; ++kx) {
    const int q = 1 - (kx & 1), dx = kx >> 1;
    bf16x8 ah[4], al[4];
    c4_read_a<64>(s_w, kx, 0, j, g, ah, al);
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {  // class pixel (il, j) reads the coarse (il + a - dy, j + q - dx): window origin (-1, -1)
      const int n = (wave * 2 + rr + 1 + a - dy) * kBHC + j + 1 + q - dx;
      const int off = n * kKS + cx_slot(n, g) * 8;
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(s_in + off);
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(s_in + kBWin * kKS + off);
      c4_mfma3<4>(ah, al, bh, bl, acc[a][q][rr]);
    }
  }
}

// grid (coarse tiles of 8 x 16 = fine tiles of 16 x 32, B, groups of 64 input channels); p.M = Ci, p.K = Co
__global__ __launch_bounds__(256) void c4_bwd_x_kernel(const C4Dims p, const float* __restrict__ pgy,
                                                       const unsigned short* __restrict__ pw, float* __restrict__ pgx) {
  __shared__ __attribute__((aligned(16))) unsigned short s_in[2 * kBWin * kKS];
  __shared__ __attribute__((aligned(16))) unsigned short s_w[2 * 4 * 64 * kKS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int M = p.M, K = p.K, H = p.H, W = p.W;
  const int ntx = (p.Wo + kTW - 1) / kTW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int i0 = ty * kTH, j0 = tx * kTW, b = blockIdx.y, m0 = blockIdx.z * 64;
  const float* in_b = pgy + (size_t)b * K * ((size_t)p.Ho * p.Wo);
  f32x4 acc[2][2][2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[a][q][rr][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += kKS) {
    c4_bwd_x_step<0>(s_in, s_w, p, in_b, pw, k0, i0, j0, m0, tid, acc);
    c4_bwd_x_step<1>(s_in, s_w, p, in_b, pw, k0, i0, j0, m0, tid, acc);
    c4_bwd_x_step<2>(s_in, s_w, p, in_b, pw, k0, i0, j0, m0, tid, acc);
    c4_bwd_x_step<3>(s_in, s_w, p, in_b, pw, k0, i0, j0, m0, tid, acc);
  }
  const size_t HW = (size_t)H * W;
  const int c = 2 * (j0 + j);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int r = 2 * (i0 + wave * 2 + rr) + a;
      if (r >= H || c >= W) continue;  // W is even: column c + 1 is inside with c
      const unsigned o = (unsigned)r * (unsigned)W + (unsigned)c;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int m = m0 + 16 * ct + 4 * g + r4;
          if (m < M)
            *reinterpret_cast<float2*>(pgx + ((size_t)b * M + m) * HW + o) =
                make_float2(acc[a][0][rr][ct][r4], acc[a][1][rr][ct][r4]);
        }
    }
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------
// grid (K blocks, Ci / 32, groups of 64 output channels); chunk = (b, coarse row Y, 32 coarse columns); block k walks chunks
// [k per, min((k + 1) per, nchunks)) and writes scratch[k][Co][Ci][16]
__global__ __launch_bounds__(256) void c4_bwd_w_kernel(const C4Dims p /* M = Co, K = Ci */, const float* __restrict__ px,
                                                       const float* __restrict__ pgy, float* __restrict__ scratch, int per,
                                                       int nchunks) {
  constexpr int kXPlane = 4 * 4 * kWCi * kWPix;  // one of hi, lo of s_x
  __shared__ __attribute__((aligned(16))) unsigned short s_x[2 * kXPlane];          // 65,536 B
  __shared__ __attribute__((aligned(16))) unsigned short s_gy[2 * kWCo * kWPix];    // 8,192 B
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int Co = p.M, Ci = p.K, H = p.H, W = p.W, Ho = p.Ho, Wo = p.Wo;
  const int ci0 = blockIdx.y * kWCi, co0 = blockIdx.z * kWCo;
  const int wco = (wave & 1) * 32, wci = (wave >> 1) * 16;
  const int nxg = (Wo + kWPix - 1) / kWPix;
  const size_t HW = (size_t)H * W, HWo = (size_t)Ho * Wo;
  f32x4 acc[2][16];
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) acc[c2][tap] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ch_begin = blockIdx.x * per, ch_end = min(nchunks, ch_begin + per);
  for (int ch = ch_begin; ch < ch_end; ++ch) {
    const int b = ch / (Ho * nxg), rem = ch - b * (Ho * nxg), Y = rem / nxg, X0 = (rem - Y * nxg) * kWPix;
    __syncthreads();  // the previous chunk has been consumed
    {  // g_y: one item = one channel x 8 pixels; channels past Co and pixels past Wo: zeros
      const int co = tid >> 2, xg = tid & 3;
      const bool cin = co0 + co < Co;
      const float* src = pgy + ((size_t)b * Co + (cin ? co0 + co : 0)) * HWo + (unsigned)Y * (unsigned)Wo;
      float va[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int X = X0 + xg * 8 + u;
        va[u] = src[X < Wo ? X : 0];
      }
      f32x8 v;
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = (cin && X0 + xg * 8 + u < Wo) ? va[u] : 0.f;
      bf16x8 hi, lo;
      cx_split(v, hi, lo);
      const int off = co * kWPix + cx_slot(co, xg) * 8;
      *reinterpret_cast<bf16x8*>(s_gy + off) = hi;
      *reinterpret_cast<bf16x8*>(s_gy + kWCo * kWPix + off) = lo;
    }
#pragma unroll
    for (int it2 = 0; it2 < 2; ++it2) {  // x: one item = one channel x one fine row x 8 pixels: 18 fine columns -> 4 images
      const int it = tid + 256 * it2, xg = it & 3, row = (it >> 2) & 3, ci = it >> 4;
      const int r = 2 * Y - 1 + row, cb = 2 * (X0 + xg * 8) - 1;
      const bool rin = r >= 0 && r < H;
      const float* src = px + ((size_t)b * Ci + ci0 + ci) * HW + (unsigned)(rin ? r : 0) * (unsigned)W;
      float va[18];
#pragma unroll
      for (int t = 0; t < 18; ++t) {
        const int c = cb + t;
        va[t] = src[(c >= 0 && c < W) ? c : 0];
      }
#pragma unroll
      for (int t = 0; t < 18; ++t) {
        const int c = cb + t;
        va[t] = (rin && c >= 0 && c < W) ? va[t] : 0.f;
      }
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) {
        f32x8 v;
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = va[kx + 2 * u];  // x[2 (X0 + 8 xg + u) - 1 + kx]
        bf16x8 hi, lo;
        cx_split(v, hi, lo);
        const int off = ((kx * 4 + row) * kWCi + ci) * kWPix + cx_slot(ci, xg) * 8;
        *reinterpret_cast<bf16x8*>(s_x + off) = hi;
        *reinterpret_cast<bf16x8*>(s_x + kXPlane + off) = lo;
      }
    }
    __syncthreads();
    bf16x8 ah[2], al[2];
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      const int m = wco + c2 * 16 + j, off = m * kWPix + cx_slot(m, g) * 8;
      ah[c2] = *reinterpret_cast<const bf16x8*>(s_gy + off);
      al[c2] = *reinterpret_cast<const bf16x8*>(s_gy + kWCo * kWPix + off);
    }
#pragma unroll
    for (int tap = 0; tap < 16; ++tap) {
      const int ky = tap >> 2, kx = tap & 3, n = wci + j;
      const int off = ((kx * 4 + ky) * kWCi + n) * kWPix + cx_slot(n, g) * 8;
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(s_x + off);
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(s_x + kXPlane + off);
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        acc[c2][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[c2], bl, acc[c2][tap], 0, 0, 0);
        acc[c2][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[c2], bh, acc[c2][tap], 0, 0, 0);
        acc[c2][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[c2], bh, acc[c2][tap], 0, 0, 0);
      }
    }
  }
  // the partial: D row = co, column = ci; the 16 taps of one (co, ci) are 64 contiguous bytes
  float* part = scratch + (size_t)blockIdx.x * Co * Ci * 16;
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int co = co0 + wco + c2 * 16 + 4 * g + r4, ci = ci0 + wci + j;
      if (co >= Co) continue;
      f32x4* dst = reinterpret_cast<f32x4*>(part + ((size_t)co * Ci + ci) * 16);
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4)
        dst[t4] = f32x4{acc[c2][4 * t4][r4], acc[c2][4 * t4 + 1][r4], acc[c2][4 * t4 + 2][r4], acc[c2][4 * t4 + 3][r4]};
    }
}

// g_w[e] = sum_k scratch[k][e] in block order, four floats per thread
__global__ __launch_bounds__(256) void c4_reduce_kernel(long long n4, int nblk, const float* __restrict__ scratch,
                                                        float* __restrict__ g_w) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  const f32x4* src = reinterpret_cast<const f32x4*>(scratch) + e;
  f32x4 s = src[0];
#pragma unroll 4
  for (int k = 1; k < nblk; ++k) s += src[(size_t)k * n4];
  reinterpret_cast<f32x4*>(g_w)[e] = s;
}

// weight[Co,Ci,4,4] -> packed[hi|lo][tap][Co / 8][Ci / 8][8 co][8 ci]; one thread per weight
__global__ __launch_bounds__(256) void c4_pack_kernel(int Co, int Ci, const float* __restrict__ w,
                                                      unsigned short* __restrict__ packed) {
  const long long n = (long long)Co * Ci * 16, idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int tap = (int)(idx & 15), ci = (int)((idx >> 4) % Ci), co = (int)(idx / (16ll * Ci));
  const float v = w[idx];
  const __bf16 hi = (__bf16)v;
  const __bf16 lo = (__bf16)(v - (float)hi);
  const size_t o = ((((size_t)tap * (Co >> 3) + (co >> 3)) * (Ci >> 3) + (ci >> 3)) * 8 + (co & 7)) * 8 + (ci & 7);
  packed[o] = __builtin_bit_cast(unsigned short, hi);
  packed[(size_t)n + o] = __builtin_bit_cast(unsigned short, lo);
}

bool c4_supported(int B, int Ci, int Co, int H, int W) {
  return Ci > 0 && Co > 0 && Ci % 32 == 0 && Co % 32 == 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && B <= 65535;
}

int c4_check(int B, int Ci, int Co, int H, int W) {
  if (!c4_supported(B, Ci, Co, H, W)) {
    gol_set_error("gol_conv4x: Ci and Co must be positive multiples of 32, H and W even and >= 2, B <= 65535 (got B %d, "
                  "%d -> %d, %d x %d)", B, Ci, Co, H, W);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(B >= 0, "bad sizes");
  GOL_REQUIRE((long long)H * W <= (1ll << 30), "plane too large (32-bit offsets inside a plane)");
  GOL_REQUIRE(gol_cdiv(Co, 64) <= 65535 && gol_cdiv(Ci, 32) <= 65535, "too many channel tiles");
  return GOL_OK;
}

// bwd_w: chunks of 32 coarse pixels, and the K blocks they are walked in (chunks per block in *per)
long long c4_wchunks(int B, int H, int W) { return (long long)B * (H / 2) * gol_cdiv(W / 2, kWPix); }

int c4_wblocks(int B, int Ci, int Co, int H, int W, int* per) {
  const long long nchunks = c4_wchunks(B, H, W), pairs = (long long)(Ci / kWCi) * gol_cdiv(Co, kWCo);
  long long nblk = (kWTarget + pairs - 1) / pairs;
  nblk = nblk > nchunks ? nchunks : nblk;
  nblk = nblk < 1 ? 1 : nblk;
  const long long pb = (nchunks + nblk - 1) / nblk;
  if (per) *per = (int)pb;
  return (int)((nchunks + pb - 1) / pb);  // no empty block
}

}  // namespace

extern "C" long long gol_conv4x_packed_elems(int Co, int Ci) {
  if (Co <= 0 || Ci <= 0 || Co % 32 != 0 || Ci % 32 != 0) return 0;
  return 2ll * 16 * Co * Ci;
}

extern "C" int gol_conv4x_pack(int Co, int Ci, const float* weight, unsigned short* packed, void* stream) {
  GOL_REQUIRE(Co > 0 && Ci > 0, "bad sizes");
  if (Co % 32 != 0 || Ci % 32 != 0) {
    gol_set_error("gol_conv4x_pack: Ci and Co must be multiples of 32 (got %d -> %d)", Ci, Co);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(weight && packed, "null pointer");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  c4_pack_kernel<<<gol_cdiv(16ll * Co * Ci, 256), 256, 0, (hipStream_t)stream>>>(Co, Ci, weight, packed);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_conv4x_fwd(int B, int Ci, int Co, int H, int W, const float* x, const unsigned short* packed, float* y,
                              void* stream) {
  const int rc = c4_check(B, Ci, Co, H, W);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && packed && y, "null pointer");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const C4Dims p{B, Co, Ci, H, W, H / 2, W / 2};
  const int tiles = gol_cdiv(p.Ho, kTH) * gol_cdiv(p.Wo, kTW);
  hipStream_t s = (hipStream_t)stream;
  if (Co <= 64) c4_fwd_kernel<1><<<dim3(tiles, B, 1), 256, 0, s>>>(p, x, packed, y);
  else c4_fwd_kernel<2><<<dim3(tiles, B, gol_cdiv(Co, 128)), 256, 0, s>>>(p, x, packed, y);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_conv4x_bwd_x(int B, int Ci, int Co, int H, int W, const unsigned short* packed, const float* g_y,
                                float* g_x, void* stream) {
  const int rc = c4_check(B, Ci, Co, H, W);
  if (rc != GOL_OK) return rc;
  if (B == 0 || !g_x) return GOL_OK;
  GOL_REQUIRE(packed && g_y, "null pointer");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  GOL_REQUIRE((reinterpret_cast<uintptr_t>(g_x) & 7) == 0, "g_x must be 8-byte aligned");
  const C4Dims p{B, Ci, Co, H, W, H / 2, W / 2};
  const int tiles = gol_cdiv(p.Ho, kTH) * gol_cdiv(p.Wo, kTW);
  c4_bwd_x_kernel<<<dim3(tiles, B, gol_cdiv(Ci, 64)), 256, 0, (hipStream_t)stream>>>(p, g_y, packed, g_x);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" long long gol_conv4x_bwd_w_scratch_floats(int B, int Ci, int Co, int H, int W) {
  if (B <= 0 || !c4_supported(B, Ci, Co, H, W)) return 0;
  return (long long)c4_wblocks(B, Ci, Co, H, W, nullptr) * Co * Ci * 16;
}

extern "C" int gol_conv4x_bwd_w(int B, int Ci, int Co, int H, int W, const float* x, const float* g_y, float* g_w,
                                float* scratch, void* stream) {
  const int rc = c4_check(B, Ci, Co, H, W);
  if (rc != GOL_OK) return rc;
  if (!g_w) return GOL_OK;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {  // an empty sum
    if (hipMemsetAsync(g_w, 0, sizeof(float) * 16 * (size_t)Co * Ci, s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  GOL_REQUIRE(x && g_y && scratch, "null pointer");
  GOL_REQUIRE(gol_aligned16(scratch) && gol_aligned16(g_w), "scratch and g_w must be 16-byte aligned");
  GOL_REQUIRE(c4_wchunks(B, H, W) <= 0x7fffffffll, "too many pixel chunks");
  const C4Dims p{B, Co, Ci, H, W, H / 2, W / 2};
  int per = 1;
  const int nblk = c4_wblocks(B, Ci, Co, H, W, &per);
  c4_bwd_w_kernel<<<dim3(nblk, Ci / kWCi, gol_cdiv(Co, kWCo)), 256, 0, s>>>(p, x, g_y, scratch, per,
                                                                          (int)c4_wchunks(B, H, W));
  GOL_CHECK_LAUNCH();
  const long long n4 = 4ll * Co * Ci;
  c4_reduce_kernel<<<gol_cdiv(n4, 256), 256, 0, s>>>(n4, nblk, scratch, g_w);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
