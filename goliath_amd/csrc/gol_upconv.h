// gol_upconv.h -- what upconv.hip (bilinear 2x + conv3) and upcat.hip (leaky + bilinear 2x + concat + conv3) compile
// identically: the coordinate tables of the integer-ratio rule (gol_upcoord.h), the blending loader, the 3x3 MFMA core and the fixed-order
// reduction of the weight gradient's partial sums.  Everything lives in an unnamed namespace: a copy per translation unit.
#pragma once
#include "gol_upcoord.h"  // the coordinate rule: up_fill_axis, up_first_row, up_blend

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTH = 8, kTW = 32;              // output tile of the forward and of the weight gradient
constexpr int kHR = kTH + 2, kHC = kTW + 2;   // its haloed window of U
constexpr int kFwdKC = 8;                     // input channels per K stage of the forward
constexpr int kFwdPlane = 400;                // >= 10 * 34, == 16 (mod 64): the 4 channel groups of a B read cover the banks
constexpr int kBwPlane = 388;                 // >= 10 * 34, ==  4 (mod 64): 16 channels x 4 consecutive pixels cover the banks
constexpr int kBwGRow = 260;                  // 256 pixels of g_pre per channel, == 4 (mod 64)

constexpr int kSH = 4, kSW = 16;              // tile of x of the input gradient
constexpr int kUR = 12, kUC = 36;             // the region of g_U that reaches it (see up_first_row)
constexpr int kGR = kUR + 2, kGC = kUC + 2;   // haloed window of g_pre
constexpr int kBxPlane = 592;                 // >= 14 * 38, == 16 (mod 64)
constexpr int kBxNPT = 7;                     // pixel tiles of 16 per wave: 4 x 7 x 16 >= 12 x 36 = 27 x 16

// KC planes of the ROWS x COLS window of U into LDS, blended from x; outside the image and past Ci: zeros.
// LEAKY: the texels go through x > 0 ? x : leak x before the blend (upcat.hip: the previous layer's activation).
template <int KC, int ROWS, int COLS, int PLANE, int UNROLL, bool LEAKY = false>
__device__ __forceinline__ void up_stage_u(float* s_u, const int* s_ra, const int* s_rb, const float* s_rf, const int* s_ca,
                                           const int* s_cb, const float* s_cf, const float* __restrict__ xb, int ci0, int Ci,
                                           size_t HWi, int tid, float leak = 0.f) {
  // an item = one window position x 4 channels: the tables and the four offsets are looked up once per item.  The loads
  // are unconditional (clamped to texel 0 / the last channel, the value is dropped); with the loop unrolled (UNROLL = 8)
  // a thread's loads are all in flight together, at the price of the registers that hold them (UNROLL = 1: one item's).
  constexpr int N = (KC / 4) * ROWS * COLS;
#pragma unroll UNROLL
  for (int it = 0; it < (N + 255) / 256; ++it) {
    const int idx = tid + 256 * it, idc = min(idx, N - 1);
    const int grp = idc / (ROWS * COLS), pos = idc - grp * (ROWS * COLS), rr = pos / COLS, cc = pos - rr * COLS;
    const int ra = s_ra[rr], ca = s_ca[cc], rb = s_rb[rr], cb = s_cb[cc];
    const float fr = s_rf[rr], fc = s_cf[cc];
    const bool in = ra >= 0 && ca >= 0;
    const int o00 = in ? ra + ca : 0, o01 = in ? ra + cb : 0, o10 = in ? rb + ca : 0, o11 = in ? rb + cb : 0;
    float x00[4], x01[4], x10[4], x11[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float* pl = xb + (size_t)min(ci0 + grp * 4 + u, Ci - 1) * HWi;
      x00[u] = pl[o00]; x01[u] = pl[o01]; x10[u] = pl[o10]; x11[u] = pl[o11];
      if constexpr (LEAKY) {
        x00[u] = x00[u] > 0.f ? x00[u] : x00[u] * leak;
        x01[u] = x01[u] > 0.f ? x01[u] : x01[u] * leak;
        x10[u] = x10[u] > 0.f ? x10[u] : x10[u] * leak;
        x11[u] = x11[u] > 0.f ? x11[u] : x11[u] * leak;
      }
    }
    if (idx < N) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ch = grp * 4 + u;
        const float v = (1.f - fr) * ((1.f - fc) * x00[u] + fc * x01[u]) + fr * ((1.f - fc) * x10[u] + fc * x11[u]);
        s_u[ch * PLANE + pos] = (in && ci0 + ch < Ci) ? v : 0.f;
      }
    }
  }
}

// D[m][pixel] += sum_{k, tap} A[m][k][tap] In[k][pixel + tap]: s_w[tap][k][16 CT], s_in[k][rows][cols] with plane / row
// strides; poff = offset of the pixel's window origin
template <int CT, int NPT, int KC>
__device__ __forceinline__ void up_conv_core(const float* s_in, int plane, int rowstride, const float* s_w,
                                             const int (&poff)[NPT], f32x4 (&acc)[NPT][CT], int j, int g) {
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
    for (int kk = 0; kk < KC / 4; ++kk) {
      float a[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) a[ct] = s_w[((tap * KC + kk * 4 + g) * CT + ct) * 16 + j];
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        const float bv = s_in[(kk * 4 + g) * plane + poff[pt] + ky * rowstride + kx];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct], bv, acc[pt][ct], 0, 0, 0);
      }
    }
  }
}

// ---- the weight gradient's second kernel -----------------------------------------------------------------------------
// gw[co,ci,tap] = sum over the K blocks of the partial sums [pair][block][9][16 co][16 ci] in scratch.  grid (9 taps x 16 co
// rows, channel tile pairs): a workgroup owns 16 outputs and sums them as 16 interleaved K slices that meet in LDS in slice
// order -- a fixed order.  The nci input-channel tiles of 16 are nsplit tiles over channels [0, Csplit) followed by tiles
// over [Csplit, Ctot) (upconv.hip: one run, nsplit = nci, Csplit = Ctot; upcat.hip: the blended and the plain half).
__global__ __launch_bounds__(256) void up_bwd_w_reduce_kernel(int Co, int Ctot, int Csplit, int nsplit, int nci, int nblk,
                                                              const float* __restrict__ scratch, float* __restrict__ gw) {
  __shared__ float s_part[16][16];
  const int tap = blockIdx.x >> 4, row = blockIdx.x & 15, cl = threadIdx.x & 15, ks = threadIdx.x >> 4;
  const int cot = blockIdx.y / nci, cit = blockIdx.y - cot * nci;
  const int co = cot * 16 + row;
  const int ci = (cit < nsplit ? cit * 16 : Csplit + (cit - nsplit) * 16) + cl, cend = cit < nsplit ? Csplit : Ctot;
  if (co >= Co) return;  // block-uniform (Co <= 4)
  const float* src = scratch + ((size_t)blockIdx.y * nblk) * (9 * 256) + tap * 256 + row * 16 + cl;
  float acc = 0.f;
#pragma unroll 4
  for (int k = ks; k < nblk; k += 16) acc += src[(size_t)k * (9 * 256)];
  s_part[ks][cl] = acc;
  __syncthreads();
  if (ks == 0 && ci < cend) {
#pragma unroll
    for (int q = 1; q < 16; ++q) acc += s_part[q][cl];
    gw[((size_t)co * Ctot + ci) * 9 + tap] = acc;
  }
}

// K blocks of the weight gradient per channel tile pair: one round of the resident workgroups, 3 per CU (LDS) on 256 CUs
inline int up_bwd_w_blocks(long long ntiles, long long pairs) {
  long long nblk = (768 + pairs - 1) / pairs;
  nblk = nblk > ntiles ? ntiles : nblk;
  return (int)(nblk < 1 ? 1 : nblk);
}

}  // namespace
