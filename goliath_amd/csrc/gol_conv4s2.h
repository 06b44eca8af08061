// gol_conv4s2.h -- what the four 4x4 stride-2 pad-1 convolution operators have in common: trunk.hip (ConvT + untied bias
// + LeakyReLU), encconv.hip (its adjoint Conv), tail.hip and mvptail.hip (the 16-channel last ConvT layers).  Written from
// the transposed convolution's side: a COARSE grid [h,w] and a FINE grid [2h,2w], fine (Y,X) = (2 iy - 1 + ky, 2 ix - 1 + kx).
// All GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32): A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15],
// D[i = 4 (lane >> 4) + r][j].  Three formulations, each used from both sides of the adjoint pair:
//   quad form      (coarse -> fine: trunk fwd, encconv bwd_x) the fine 2x2 quad {2m-1, 2m} x {2k-1, 2k} reads the coarse
//                  2x2 block {m-1, m} x {k-1, k} and uses each of the 16 taps once, so every parity class (a,q) is a GEMM
//                  D[out][quad] = A[out][(red,tap)] B[(red,tap)][quad], K = the 4 taps of one reduction channel; B is
//                  shared by the four classes.  Weights [red][out][4][4] go through an LDS tile per K stage.
//   row gather     (fine -> coarse: trunk bwd_x, encconv fwd) no atomics: D[out][pixel] += A[out][ky] B[ky][pixel] per
//                  (red, kx), K = the four window ROWS: lane (pixel j, row g) holds fine[red][2iy-1+g][2ix-1+kx], so the
//                  four kx of a lane are four consecutive floats of one row -- ONE 16-byte load (4-byte aligned) feeds four
//                  MFMAs.  At the left / right border the load starts one column late / early (it never leaves the row) and
//                  the values shift by one (WIDE; rows of fewer than 4 floats take clamped scalar loads instead).
//   weight grad    per (16 x 16) channel tile pair a GEMM over pixels, 16 accumulator tiles (one per tap): a workgroup
//                  walks tiles of one view x one coarse row x 64 coarse pixels; the coarse side [16 N][64] and the matching
//                  fine WINDOW [16 planes][4 rows][130 cols] are staged in LDS, software-pipelined (the global loads of the
//                  NEXT tile are issued into registers, all independent, before the MFMA phase of the current one); the
//                  waves' sums meet in LDS in wave order and leave as one partial [16 taps][256] per channel tile; K is
//                  split over workgroups and a second kernel adds the partials in a fixed order (no float atomics).
// The formulations are DESCRIBED here once; their loop bodies (the quad and row-gather GEMMs, the window staging, the
// 4 x 4 x 4 MFMA nest, the wave-ordered LDS sum) stay written out in each kernel: moved into helpers -- as templates over
// the element transform, the dead-plane rule and the XCD run order -- the same text compiles to other register counts
// (profiles/LOG.md, "conv4s2", lists each attempt and its cost).  Here are the pieces that compile to the same machine code
// from one place: the LDS geometry, the partial store, the fixed-order K reduce, the K-block count, the 16-channel scalar
// input gradient and the streaming bias gradient.  Everything is inline and file-local (anonymous namespace).
#pragma once
#include "gol_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// ---- weight gradient -------------------------------------------------------------------------------------------------
constexpr int kWTile = 64;                  // coarse pixels per tile
constexpr int kWinRow = 2 * kWTile + 4;     // 130 used
constexpr int kWinPlane = 4 * kWinRow + 2;  // == 18 (mod 32): the 8-byte reads of a lane group's 16 planes cover the 32 banks
constexpr int kPixRow = kWTile + 4;         // == 4 (mod 32)

// the partial [16 taps][256] leaves; dst = this thread's float of tap 0 in scratch
__device__ __forceinline__ void wgrad_store_partial(float* dst, const float (*s_red)[256]) {
#pragma unroll
  for (int tap = 0; tap < 16; ++tap) dst[(size_t)tap * 256] = s_red[tap][threadIdx.x];
}

// The K reduce: a workgroup of 256 owns 16 outputs (thread & 15) and sums their nblk partials (src: this output's element
// of K block 0, blocks 16 x 256 floats apart) as 16 interleaved K slices (thread >> 4) that meet in LDS in slice order -- a
// fixed order, and 16 x the workgroups and 1/16 of the dependent loads of one thread per output (hundreds of K blocks for a
// layer with few tiles).  Slice 0 writes *dst where `valid`.
__device__ __forceinline__ void wgrad_reduce16(const float* __restrict__ src, int nblk, float* __restrict__ dst, bool valid) {
  __shared__ float s_part[16][16];
  const int col = threadIdx.x & 15, ks = threadIdx.x >> 4;
  float acc = 0.f;
#pragma unroll 4
  for (int k = ks; k < nblk; k += 16) acc += src[(size_t)k * 16 * 256];
  s_part[ks][col] = acc;
  __syncthreads();
  if (ks == 0 && valid) {
#pragma unroll
    for (int q = 1; q < 16; ++q) acc += s_part[q][col];
    *dst = acc;
  }
}

// K blocks of a weight gradient: one round of `target` resident workgroups over the `pairs` channel-tile groups, at most one
// per tile
static inline int wgrad_blocks(long long ntiles, long long pairs, long long target) {
  long long nblk = (target + pairs - 1) / pairs;
  nblk = nblk > ntiles ? ntiles : nblk;
  return (int)(nblk < 1 ? 1 : nblk);
}

// ---- 16-channel input gradient, scalar gather (the last layers: few output channels) ----------------------------------
// gx[b,ci,iy,ix] = sum_{ch,dy,dx} g[b,ch,2iy-1+dy,2ix-1+dx] W[ci,ch,dy,dx]; wt = W as [CH,4,4,16] (of this view).  One lane =
// one coarse pixel x 16 input channels; grid (w / 256, h, B).
__device__ __forceinline__ void gather_bwd_x16(int h, int w, int CH, const float* __restrict__ wt,
                                               const float* __restrict__ pg, float* __restrict__ pgx) {
  const int ix = blockIdx.x * 256 + threadIdx.x, iy = blockIdx.y, b = blockIdx.z;
  if (ix >= w) return;
  const size_t HWi = (size_t)h * w, HWo = 4 * HWi;
  const float* gb = pg + (size_t)b * CH * HWo;
  float acc[16];
#pragma unroll
  for (int ci = 0; ci < 16; ++ci) acc[ci] = 0.f;
#pragma unroll
  for (int dy = 0; dy < 4; ++dy) {
    const int oy = 2 * iy - 1 + dy;
    if (oy < 0 || oy >= 2 * h) continue;  // block-uniform
    const int ox0 = 2 * ix - 1;
    const bool ok0 = ox0 >= 0, ok3 = ox0 + 3 < 2 * w;
    for (int ch = 0; ch < CH; ++ch) {
      const float* gr = gb + (size_t)ch * HWo + (size_t)oy * (2 * w) + ox0;
      float gv[4];  // unconditional loads (edge lanes re-read a neighbour), then masked: no divergent branches
      gv[0] = gr[ok0 ? 0 : 1]; gv[1] = gr[1]; gv[2] = gr[2]; gv[3] = gr[ok3 ? 3 : 2];
      gv[0] = ok0 ? gv[0] : 0.f; gv[3] = ok3 ? gv[3] : 0.f;
#pragma unroll
      for (int dx = 0; dx < 4; ++dx) {
        const float* wq = wt + ((size_t)(ch * 4 + dy) * 4 + dx) * 16;  // wave-uniform
#pragma unroll
        for (int ci = 0; ci < 16; ++ci) acc[ci] += gv[dx] * wq[ci];
      }
    }
  }
#pragma unroll
  for (int ci = 0; ci < 16; ++ci) pgx[((size_t)b * 16 + ci) * HWi + (size_t)iy * w + ix] = acc[ci];
}

// ---- untied-bias gradient behind a LeakyReLU, one streaming pass -------------------------------------------------------
// gbias[n] = sum_b g[b,n] (y[b,n] > 0 ? 1 : leak) over the N4 float4 of one view, one per thread
__device__ __forceinline__ void lrelu_bias_grad(size_t N4, int B, float leak, const float* __restrict__ py,
                                                const float* __restrict__ pg, float* __restrict__ pgb) {
  const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N4) return;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b = 0; b < B; ++b) {
    const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pg) + (size_t)b * N4 + n);
    const f32x4 yv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(py) + (size_t)b * N4 + n);
    s.x += gv.x * (yv.x > 0.f ? 1.f : leak);
    s.y += gv.y * (yv.y > 0.f ? 1.f : leak);
    s.z += gv.z * (yv.z > 0.f ? 1.f : leak);
    s.w += gv.w * (yv.w > 0.f ? 1.f : leak);
  }
  reinterpret_cast<float4*>(pgb)[n] = s;
}

}  // namespace
