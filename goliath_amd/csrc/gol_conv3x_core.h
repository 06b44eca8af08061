// gol_conv3x_core.h -- the tile, the weight stager and the MFMA core that the 3x3 / stride 1 split-bf16 operators share:
// conv3x.hip (bias + ReLU, VGG19) and conv3ub.hip (two sources, untied bias + LeakyReLU, the MVP teacher's UNet).  Lifted out
// of conv3x.hip as it stood; its header explains the scheme (8 x 32 pixel tile, pixel-major window, weights per tap row).
#pragma once
#include "gol_splitbf16.h"  // the vector types, cx_split and cx_slot (shared with conv4x.hip)

namespace {

struct CxDims {
  int B, M, K, H, W, Hp, Wp;  // M rows of the GEMM (channels written), K reduction channels (channels read), pooled size
};

constexpr int kTH = 8, kTW = 32;             // pixel tile (even origin, even size)
constexpr int kHR = kTH + 2, kHC = kTW + 2;  // its haloed window
constexpr int kWin = kHR * kHC;              // 340 positions
constexpr int kKS = 32;                      // channels per K stage = the K of one MFMA

// the weights of tap row ky of a K stage as s_w[hi|lo][kx][16 CT rows][32 k], one packed 8 x 8 block per thread.
// Forward: A[co][ci][tap] = w[co][ci][tap], block (tap, co / 8, ci / 8) row by row.  TRANS: A[ci][co][tap] = w[co][ci][8 - tap]:
// block (8 - tap, co / 8 = k block, ci / 8 = m block) transposed.  Rows past M: zeros.
template <int CT, bool TRANS>
__device__ __forceinline__ void cx_stage_w(unsigned short* s_w, const CxDims& p, const unsigned short* __restrict__ pw, int k0,
                                           int m0, int ky, int tid) {
  constexpr int MB = 2 * CT, NBLK = 2 * 3 * MB * 4;
  const int M = p.M, K = p.K;
  for (int idx = tid; idx < NBLK; idx += 256) {
    const int kb = idx & 3, mb = (idx >> 2) % MB, rest = idx / (4 * MB), kx = rest % 3, plane = rest / 3;
    const int tap = ky * 3 + kx, mblk = (m0 >> 3) + mb, kblk = (k0 >> 3) + kb;
    u32x4 row[8];
    if (mblk * 8 < M) {
      const size_t blk = TRANS ? (((size_t)plane * 9 + (8 - tap)) * (K >> 3) + kblk) * (M >> 3) + mblk
                               : (((size_t)plane * 9 + tap) * (M >> 3) + mblk) * (K >> 3) + kblk;
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
      *reinterpret_cast<u32x4*>(s_w + ((plane * 3 + kx) * (16 * CT) + m) * kKS + cx_slot(m, kb) * 8) = row[r];
    }
  }
}

// D[m][pixel] += sum_{k, kx} A[m][k][ky, kx] In[k][pixel + (ky, kx)] in three bf16 products; poff = the pixel's window origin
template <int CT>
__device__ __forceinline__ void cx_core(const unsigned short* s_in, const unsigned short* s_w, const int (&poff)[4],
                                        f32x4 (&acc)[4][CT], int ky, int j, int g) {
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    bf16x8 ah[CT], al[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int m = ct * 16 + j, off = (kx * (16 * CT) + m) * kKS + cx_slot(m, g) * 8;
      ah[ct] = *reinterpret_cast<const bf16x8*>(s_w + off);
      al[ct] = *reinterpret_cast<const bf16x8*>(s_w + 3 * 16 * CT * kKS + off);
    }
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int pos = poff[pt] + ky * kHC + kx, off = pos * kKS + cx_slot(pos, g) * 8;
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(s_in + off);
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(s_in + kWin * kKS + off);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ct], bl, acc[pt][ct], 0, 0, 0);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[ct], bh, acc[pt][ct], 0, 0, 0);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[ct], bh, acc[pt][ct], 0, 0, 0);
    }
  }
}

}  // namespace
