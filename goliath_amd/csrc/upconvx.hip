// upconvx.hip -- one layer of URHand's texture decoder at precision "bf16x3", gfx950, wave64: exact 2x bilinear resize
// (align_corners=True) + 3x3 / stride 1 / pad 1 convolution + epilogue, forward and backward, with the upsampled tensor
// never in memory in either direction.  The semantics are those of upconv.hip (read its header: the layers are
// ca_code/models/urhand.py:583-608, built at :302-323), for x[B,Ci,Hi,Wi], H = 2 Hi, W = 2 Wi:
//     U[b,ci,r,c]   = bilinear(x[b,ci]) by the INTEGER-RATIO rule (gol_upcoord.h), blended in fp32
//     acc[b,co,r,c] = sum_{ci,ky,kx} Upad[b,ci,r-1+ky,c-1+kx] w[co,ci,ky,kx]
//     mode 0:  y = lrelu(acc + bias[co,r,c])        mode 1:  y = (acc gate[b,co,r,c] + gb[b,co,r,c]) scale
//     g_pre = g_y (y > 0 ? 1 : leak) (mode 0) or scale gate g_y (mode 1), formed in fp32 while loading
// The only difference is the product: the arithmetic and the conventions are those of conv3x.hip (read its header) --
// v_mfma_f32_16x16x32_bf16, every operand split into hi = bf16_rne(v), lo = bf16_rne(v - hi) while it is staged (U AFTER the
// blend, g_pre AFTER it is formed), three MFMAs per product (lo lo dropped), fp32 accumulation, padding splits to (0,0);
// every LDS image has 64-byte rows read 16 bytes per lane through cx_slot.  Ci % 32 == 0, Co % 16 == 0.
//   pack    w -> packed[hi|lo][tap][Cop / 8][Ci / 8][8 co][8 ci], Cop = Co rounded up to 32, the rows past Co zeros: the layout
//           of gol_conv3ub_pack padded on the OTHER side (there Ci, here Co: the input gradient's K stage is 32 output
//           channels), so cx_stage_w serves both directions as it stands.
//   fwd     cx_kernel's scheme (gol_conv3x_core.h): 8 x 32 output pixels x 16 CT channels per workgroup (CT = 1 for Co = 16, 2
//           for 32, else 4).  Per K stage of 32 channels the haloed 10 x 34 window of U is blended from the up-to-2x2 texels of
//           x (up_fill_axis tables, up_blend), split and stored pixel-major; weights through cx_stage_w, MFMAs through cx_core.
//           Epilogues on the accumulators: mode 0, mode 1 and the gate gradient (g_gate = scale g_y acc, g_gb = scale g_y):
//           the gate gradient is the forward again.
//   bwd_x   up_bwd_x_kernel's plan on the split product.  A workgroup owns 2 x 14 texels of x x 16 CT input channels (CT = 2
//           for Ci = 32, else 4).  The rows of U that reach source rows [i0, i0 + 2) are at most 8, the columns that reach
//           [j0, j0 + 14) at most 32, both starting at up_first_row (tests/test_upconvx_cpu.py proves it for every tile of
//           every size): the region of g_U is ONE 8 x 32 tile of the forward's core with the window of g_pre (10 x 34) as the
//           B operand and the blocks transposed and the taps mirrored by cx_stage_w<.., TRANS>.  The accumulators go to LDS
//           in fp32 (over the operand images, which are done with) and every texel gathers its up-to-5x5 pixels in fp32 with
//           the forward's own row and column weights.  No g_U in memory, no atomics.
//   bwd_w   conv3ub.hip's plan: the GEMM's K is the PIXEL.  A chunk = 32 pixels of one output row; g_pre goes to
//           s_g[hi|lo][64 co][32]; the 3 x 20 texels of x behind the chunk's window of U go to LDS raw (one coalesced pass:
//           blending straight from memory costs 40 scattered loads per 10 pixels and left the kernel bound by them), and
//           the window (3 rows x 34 columns x 32 ci) is blended from there into s_x[hi|lo][kx][3 rows][32 ci][32].
//           A workgroup owns 64 co x 32 ci x 9 taps.  K is split over workgroups (contiguous runs of chunks); a partial
//           [Co][Ci][9] leaves per workgroup and ux_reduce_kernel adds the partials in block order.  Scratch = blocks x Co x
//           Ci x 9 floats <= (512 + channel-tile pairs) x 18432 floats, whatever B, H and W.
//   g_bias (mode 0) and g_gb without a gate gradient (mode 1) are gol_upconv_bwd's streaming pass (upconv.hip), exact fp32.
// No float atomics; every output element is a fixed-order sum: bitwise reproducible.  No host sync, no allocation.
#include "gol_conv3x_core.h"  // the tile, cx_stage_w, cx_core
#include "gol_upcoord.h"      // up_fill_axis, up_first_row, up_blend

namespace {

struct UxDims {
  int B, Ci, Co, Hi, Wi, H, W, mode;
  float leak, scale;
};

constexpr int kXH = 2, kXW = 14;     // bwd_x: tile of x; the region of g_U that reaches it is one kTH x kTW tile
constexpr int kGuRow = kTH * kTW + 4;  // bwd_x: floats per channel of the region in LDS, == 4 (mod 64)
constexpr int kWPix = 32;            // bwd_w: pixels per chunk
constexpr int kWCo = 64, kWCi = 32;  // bwd_w: channels per workgroup
constexpr int kWTarget = 512;        // bwd_w: workgroups aimed at (two per CU)
constexpr int kSR = 3, kSC = 20;     // bwd_w: rows and columns of x behind a chunk's 3 x 34 window of U

__device__ __forceinline__ float ux_gpre(const UxDims& p, float g, float aux) {
  return p.mode == 0 ? g * (aux > 0.f ? 1.f : p.leak) : p.scale * g * aux;
}

// 32 channels of the haloed window of U (tables: its 10 rows and 34 columns), blended from x, split into
// s_in[hi|lo][position][32]; outside the image: zeros.  xs = channel 0 of this stage.  An item = one window position x 8
// channels; the loads are unconditional (clamped to texel 0, the value is dropped).
__device__ __forceinline__ void ux_stage_u(unsigned short* s_in, const int* s_ra, const int* s_rb, const float* s_rf,
                                           const int* s_ca, const int* s_cb, const float* s_cf,
                                           const float* __restrict__ xs, size_t HWi, int tid) {
  constexpr int N = (kKS / 8) * kWin;
  for (int idx = tid; idx < N; idx += 256) {
    const int q = idx / kWin, pos = idx - q * kWin, rr = pos / kHC, cc = pos - rr * kHC;
    const int ra = s_ra[rr], ca = s_ca[cc], rb = s_rb[rr], cb = s_cb[cc];
    const float fr = s_rf[rr], fc = s_cf[cc];
    const bool in = ra >= 0 && ca >= 0;
    const int o00 = in ? ra + ca : 0, o01 = in ? ra + cb : 0, o10 = in ? rb + ca : 0, o11 = in ? rb + cb : 0;
    float x00[8], x01[8], x10[8], x11[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {  // every load first, none behind a condition
      const float* pl = xs + (size_t)(q * 8 + u) * HWi;
      x00[u] = pl[o00]; x01[u] = pl[o01]; x10[u] = pl[o10]; x11[u] = pl[o11];
    }
    f32x8 v;
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = in ? up_blend(fr, fc, x00[u], x01[u], x10[u], x11[u]) : 0.f;
    bf16x8 hi, lo;
    cx_split(v, hi, lo);
    const int off = pos * kKS + cx_slot(pos, q) * 8;
    *reinterpret_cast<bf16x8*>(s_in + off) = hi;
    *reinterpret_cast<bf16x8*>(s_in + kWin * kKS + off) = lo;
  }
}

// 32 channels of the haloed window of g_pre, origin (r0 - 1, c0 - 1), split into s_in[hi|lo][position][32]; outside the image
// and for the channels past nv (a multiple of 8): zeros.  g_s, aux_s = channel 0 of this stage (cu_stage<true> with ux_gpre).
__device__ __forceinline__ void ux_stage_g(unsigned short* s_in, const UxDims& p, const float* __restrict__ g_s,
                                           const float* __restrict__ aux_s, int nv, int r0, int c0, int tid) {
  constexpr int N = (kKS / 8) * kWin;
  const int H = p.H, W = p.W;
  const size_t PS = (size_t)H * W;
  for (int idx = tid; idx < N; idx += 256) {
    const int q = idx / kWin, pos = idx - q * kWin, rr = pos / kHC, cc = pos - rr * kHC;
    const int r = r0 - 1 + rr, c = c0 - 1 + cc;
    const bool in = r >= 0 && r < H && c >= 0 && c < W && q * 8 < nv;
    const unsigned o = in ? (unsigned)r * (unsigned)W + (unsigned)c : 0u;
    const int ch = in ? q * 8 : 0;
    float va[8], vb[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {  // every load first, none behind a condition
      const size_t oo = (size_t)(ch + u) * PS + o;
      va[u] = g_s[oo];
      vb[u] = aux_s[oo];
    }
    f32x8 v;
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = in ? ux_gpre(p, va[u], vb[u]) : 0.f;
    bf16x8 hi, lo;
    cx_split(v, hi, lo);
    const int off = pos * kKS + cx_slot(pos, q) * 8;
    *reinterpret_cast<bf16x8*>(s_in + off) = hi;
    *reinterpret_cast<bf16x8*>(s_in + kWin * kKS + off) = lo;
  }
}

__device__ __forceinline__ int ux_pad32(int c) { return (c + 31) / 32 * 32; }

// ---- forward ---------------------------------------------------------------------------------------------------------
// grid (tiles of 8 x 32 pixels, B, groups of 16 CT output channels).  EPI 0: y = lrelu(acc + bias) (pa = bias);
// EPI 1: y = (acc gate + gb) scale (pa = gate, pb = gb or NULL); EPI 2: out = scale g_y acc, out2 = scale g_y (pa = g_y).
template <int CT, int EPI>
__global__ __launch_bounds__(256) void ux_fwd_kernel(const UxDims p, const float* __restrict__ px,
                                                     const unsigned short* __restrict__ pw, const float* __restrict__ pa,
                                                     const float* __restrict__ pb, float* __restrict__ pout,
                                                     float* __restrict__ pout2) {
  __shared__ __attribute__((aligned(16))) unsigned short s_in[2 * kWin * kKS];
  __shared__ __attribute__((aligned(16))) unsigned short s_w[2 * 3 * 16 * CT * kKS];
  __shared__ int s_ra[kHR], s_rb[kHR], s_ca[kHC], s_cb[kHC];
  __shared__ float s_rf[kHR], s_cf[kHC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, Ci = p.Ci, Co = p.Co;
  const int ntx = (W + kTW - 1) / kTW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int r0 = ty * kTH, c0 = tx * kTW, b = blockIdx.y, m0 = blockIdx.z * (16 * CT);
  const size_t HWi = (size_t)p.Hi * p.Wi, HW = (size_t)H * W;
  const float* xb = px + (size_t)b * Ci * HWi;
  up_fill_axis(s_ra, s_rb, s_rf, kHR, r0 - 1, p.Hi, H, p.Wi, tid);
  up_fill_axis(s_ca, s_cb, s_cf, kHC, c0 - 1, p.Wi, W, 1, tid);
  // the packed weight as cx_stage_w sees it: M rows written (padded to 32 with zero rows), K channels read
  const CxDims pk{p.B, ux_pad32(Co), Ci, H, W, 0, 0};
  int poff[4], prow[4], pcol[4];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {  // wave -> rows 2 wave, 2 wave + 1 of the tile, two halves of 16 columns each
    prow[pt] = wave * 2 + (pt >> 1);
    pcol[pt] = (pt & 1) * 16 + j;
    poff[pt] = prow[pt] * kHC + pcol[pt];
  }
  f32x4 acc[4][CT];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Ci; k0 += kKS) {
    for (int ky = 0; ky < 3; ++ky) {
      __syncthreads();  // the tables are written / the previous tap row has been consumed
      if (ky == 0) ux_stage_u(s_in, s_ra, s_rb, s_rf, s_ca, s_cb, s_cf, xb + (size_t)k0 * HWi, HWi, tid);
      cx_stage_w<CT, false>(s_w, pk, pw, k0, m0, ky, tid);
      __syncthreads();
      cx_core<CT>(s_in, s_w, poff, acc, ky, j, g);
    }
  }
  // epilogue on the accumulators: D row = channel m0 + 16 ct + 4 g + r4, column = pixel j of the pixel tile
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int r = r0 + prow[pt], c = c0 + pcol[pt];
    if (r >= H || c >= W) continue;
    const unsigned o = (unsigned)r * (unsigned)W + (unsigned)c;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int co = m0 + 16 * ct + 4 * g + r4;
        if (co >= Co) continue;
        const size_t off = ((size_t)b * Co + co) * HW + o;
        const float a = acc[pt][ct][r4];
        if constexpr (EPI == 0) {
          const float v = a + pa[(size_t)co * HW + o];
          pout[off] = v > 0.f ? v : v * p.leak;
        } else if constexpr (EPI == 1) {
          float v = a * pa[off];
          if (pb) v += pb[off];
          pout[off] = v * p.scale;
        } else {
          const float gy = p.scale * pa[off];
          pout[off] = gy * a;
          if (pout2) pout2[off] = gy;
        }
      }
  }
}

// ---- input gradient --------------------------------------------------------------------------------------------------
// grid (tiles of 2 x 14 texels of x, B, groups of 16 CT input channels)
template <int CT>
__global__ __launch_bounds__(256) void ux_bwd_x_kernel(const UxDims p, const unsigned short* __restrict__ pw,
                                                       const float* __restrict__ paux, const float* __restrict__ pg,
                                                       float* __restrict__ pgx) {
  constexpr int kIn = 2 * kWin * kKS, kW = 2 * 3 * 16 * CT * kKS;
  static_assert((kIn + kW) * 2 >= 16 * CT * kGuRow * 4, "the region of g_U must fit over the operand images");
  __shared__ __attribute__((aligned(16))) unsigned short s_buf[kIn + kW];
  __shared__ int s_ra[kTH], s_rb[kTH], s_ca[kTW], s_cb[kTW];
  __shared__ float s_rf[kTH], s_cf[kTW];
  unsigned short* s_in = s_buf;
  unsigned short* s_w = s_buf + kIn;
  float* s_gu = reinterpret_cast<float*>(s_buf);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, Hi = p.Hi, Wi = p.Wi, Ci = p.Ci, Co = p.Co, Cop = ux_pad32(Co);
  const int ntx = (Wi + kXW - 1) / kXW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int i0 = ty * kXH, j0 = tx * kXW, b = blockIdx.y, m0 = blockIdx.z * (16 * CT);
  const int rlo = up_first_row(i0, Hi, H), clo = up_first_row(j0, Wi, W);
  const size_t HW = (size_t)H * W;
  // source indices (mul = 1) and fractions of the region's rows and columns; -1 = outside the image
  up_fill_axis(s_ra, s_rb, s_rf, kTH, rlo, Hi, H, 1, tid);
  up_fill_axis(s_ca, s_cb, s_cf, kTW, clo, Wi, W, 1, tid);
  // the packed weight as cx_stage_w<.., true> sees it: M = input channels written, K = output channels read (padded)
  const CxDims pk{p.B, Ci, Cop, H, W, 0, 0};
  int poff[4], prow[4], pcol[4];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    prow[pt] = wave * 2 + (pt >> 1);
    pcol[pt] = (pt & 1) * 16 + j;
    poff[pt] = prow[pt] * kHC + pcol[pt];
  }
  f32x4 acc[4][CT];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Cop; k0 += kKS) {
    const float* g_s = pg + ((size_t)b * Co + k0) * HW;
    const float* aux_s = paux + ((size_t)b * Co + k0) * HW;
    const int nv = min(kKS, Co - k0);
    for (int ky = 0; ky < 3; ++ky) {
      __syncthreads();  // the previous tap row has been consumed
      if (ky == 0) ux_stage_g(s_in, p, g_s, aux_s, nv, rlo, clo, tid);
      cx_stage_w<CT, true>(s_w, pk, pw, k0, m0, ky, tid);
      __syncthreads();
      cx_core<CT>(s_in, s_w, poff, acc, ky, j, g);
    }
  }
  __syncthreads();  // the operand images are done with: g_U of the region goes over them
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) s_gu[(16 * ct + 4 * g + r4) * kGuRow + prow[pt] * kTW + pcol[pt]] = acc[pt][ct][r4];
  __syncthreads();
  // the bilinear adjoint as a gather: thread -> texel tid & 31 of the tile (28 of them), channels (tid >> 5) + 8 u
  const int tl = tid & 31, ti = i0 + tl / kXW, tj = j0 + tl % kXW;
  if (tl >= kXH * kXW || ti >= Hi || tj >= Wi) return;
  const int rs = up_first_row(ti, Hi, H) - rlo, cs = up_first_row(tj, Wi, W) - clo;  // first candidates, inside the region
  float wr[5], wc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const int rr = rs + t, cc = cs + t;
    wr[t] = wc[t] = 0.f;
    if (rr < kTH && s_ra[rr] >= 0) wr[t] = (s_ra[rr] == ti ? 1.f - s_rf[rr] : 0.f) + (s_rb[rr] == ti ? s_rf[rr] : 0.f);
    if (cc < kTW && s_ca[cc] >= 0) wc[t] = (s_ca[cc] == tj ? 1.f - s_cf[cc] : 0.f) + (s_cb[cc] == tj ? s_cf[cc] : 0.f);
  }
  float* gxb = pgx + (size_t)b * Ci * Hi * Wi + (unsigned)ti * (unsigned)Wi + (unsigned)tj;
#pragma unroll
  for (int u = 0; u < 2 * CT; ++u) {
    const int ml = (tid >> 5) + 8 * u;
    if (m0 + ml >= Ci) continue;
    const float* src = s_gu + ml * kGuRow;
    float sum = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      float rowsum = 0.f;
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int rr = min(rs + a, kTH - 1), cc = min(cs + c, kTW - 1);  // (a clamped candidate has weight 0)
        rowsum += wc[c] * src[rr * kTW + cc];
      }
      sum += wr[a] * rowsum;
    }
    gxb[(size_t)(m0 + ml) * Hi * Wi] = sum;
  }
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------
// grid (K blocks, Ci / 32, groups of 64 output channels); chunk = (b, row r, 32 columns); block k walks chunks
// [k per, min((k + 1) per, nchunks)) and writes scratch[k][Co][Ci][9]
__global__ __launch_bounds__(256) void ux_bwd_w_kernel(const UxDims p, const float* __restrict__ px,
                                                       const float* __restrict__ paux, const float* __restrict__ pgy,
                                                       float* __restrict__ scratch, int per, int nchunks) {
  constexpr int kXPlane = 3 * 3 * kWCi * kWPix;  // one of hi, lo of s_x
  __shared__ __attribute__((aligned(16))) unsigned short s_x[2 * kXPlane];        // 36,864 B
  __shared__ __attribute__((aligned(16))) unsigned short s_g[2 * kWCo * kWPix];   // 8,192 B
  __shared__ float s_src[kWCi * kSR * kSC];                                       // 7,680 B
  __shared__ int s_ra[3], s_rb[3], s_ca[kWPix + 2], s_cb[kWPix + 2];
  __shared__ float s_rf[3], s_cf[kWPix + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int Ci = p.Ci, Co = p.Co, H = p.H, W = p.W;
  const int ci0 = blockIdx.y * kWCi, co0 = blockIdx.z * kWCo;
  const int wco = (wave & 1) * 32, wci = (wave >> 1) * 16;
  const int nxg = (W + kWPix - 1) / kWPix;
  const size_t HW = (size_t)H * W, HWi = (size_t)p.Hi * p.Wi;
  f32x4 acc[2][9];
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[c2][tap] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ch_begin = blockIdx.x * per, ch_end = min(nchunks, ch_begin + per);
  for (int ch = ch_begin; ch < ch_end; ++ch) {
    const int b = ch / (H * nxg), rem = ch - b * (H * nxg), r = rem / nxg, X0 = (rem - r * nxg) * kWPix;
    __syncthreads();  // the previous chunk has been consumed
    // source row / column INDICES (mul = 1) of the chunk's 3 rows and 34 columns of U, and the raw source window they
    // read: rows srow0 .. srow0 + 2, columns scol0 .. scol0 + 19 of x (the ratio is below 1/2: 3 rows of U reach at most 3
    // rows of x, 34 columns at most 19; tests/test_upconvx_cpu.py proves it), clamped to the plane
    up_fill_axis(s_ra, s_rb, s_rf, 3, r - 1, p.Hi, H, 1, tid);
    up_fill_axis(s_ca, s_cb, s_cf, kWPix + 2, X0 - 1, p.Wi, W, 1, tid);
    const int srow0 = (max(r - 1, 0) * (p.Hi - 1)) / (H - 1), scol0 = (max(X0 - 1, 0) * (p.Wi - 1)) / (W - 1);
    {
      constexpr int N = kWCi * kSR * kSC;
      const float* xb = px + ((size_t)b * Ci + ci0) * HWi;
      float v[(N + 255) / 256];
#pragma unroll
      for (int k = 0; k < (N + 255) / 256; ++k) {  // unconditional loads, clamped to the window's last element
        const int e = min(tid + 256 * k, N - 1), ci = e / (kSR * kSC), rem = e - ci * (kSR * kSC), row = rem / kSC;
        const int sr = min(srow0 + row, p.Hi - 1), sc = min(scol0 + rem - row * kSC, p.Wi - 1);
        v[k] = xb[(size_t)ci * HWi + (unsigned)sr * (unsigned)p.Wi + (unsigned)sc];
      }
#pragma unroll
      for (int k = 0; k < (N + 255) / 256; ++k)
        if (tid + 256 * k < N) s_src[tid + 256 * k] = v[k];
    }
    {  // g_pre: one item = one channel x 8 pixels; channels past Co and pixels past W: zeros
      const int co = tid >> 2, xg = tid & 3;
      const bool cin = co0 + co < Co;
      const size_t base = ((size_t)b * Co + (cin ? co0 + co : 0)) * HW + (unsigned)r * (unsigned)W;
      float va[8], vy[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int Xc = min(X0 + xg * 8 + u, W - 1);  // clamped by arithmetic: no lane mask is kept across the loads
        va[u] = pgy[base + Xc];
        vy[u] = paux[base + Xc];
      }
      f32x8 v;
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = (cin && X0 + xg * 8 + u < W) ? ux_gpre(p, va[u], vy[u]) : 0.f;
      bf16x8 hi, lo;
      cx_split(v, hi, lo);
      const int off = co * kWPix + cx_slot(co, xg) * 8;
      *reinterpret_cast<bf16x8*>(s_g + off) = hi;
      *reinterpret_cast<bf16x8*>(s_g + kWCo * kWPix + off) = lo;
    }
    __syncthreads();  // the tables and the raw window are written
#pragma unroll
    for (int it2 = 0; it2 < 2; ++it2) {  // U: one item = one channel x one row x 8 pixels: 10 columns -> 3 images
      const int it = tid + 256 * it2;
      if (it >= kWCi * 3 * 4) break;
      const int xg = it & 3, row = (it >> 2) % 3, ci = it / 12;
      const int ra = s_ra[row], rb = s_rb[row];
      const float fr = s_rf[row];
      const float* src = s_src + ci * (kSR * kSC);
      const int oa = min(max(ra - srow0, 0), kSR - 1) * kSC, ob = min(max(rb - srow0, 0), kSR - 1) * kSC;
      float va[10];
#pragma unroll
      for (int t = 0; t < 10; ++t) {  // blended from the raw window in LDS; outside the image: zero
        const int cc = xg * 8 + t, ca = s_ca[cc];
        const int qa = min(max(ca - scol0, 0), kSC - 1), qb = min(max(s_cb[cc] - scol0, 0), kSC - 1);
        const float v = up_blend(fr, s_cf[cc], src[oa + qa], src[oa + qb], src[ob + qa], src[ob + qb]);
        va[t] = (ra >= 0 && ca >= 0) ? v : 0.f;
      }
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        f32x8 v;
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = va[kx + u];  // U[X0 + 8 xg + u - 1 + kx]
        bf16x8 hi, lo;
        cx_split(v, hi, lo);
        const int off = ((kx * 3 + row) * kWCi + ci) * kWPix + cx_slot(ci, xg) * 8;
        *reinterpret_cast<bf16x8*>(s_x + off) = hi;
        *reinterpret_cast<bf16x8*>(s_x + kXPlane + off) = lo;
      }
    }
    __syncthreads();
    bf16x8 ah[2], al[2];
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      const int m = wco + c2 * 16 + j, off = m * kWPix + cx_slot(m, g) * 8;
      ah[c2] = *reinterpret_cast<const bf16x8*>(s_g + off);
      al[c2] = *reinterpret_cast<const bf16x8*>(s_g + kWCo * kWPix + off);
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky, n = wci + j;
      const int off = ((kx * 3 + ky) * kWCi + n) * kWPix + cx_slot(n, g) * 8;
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
  // the partial: D row = co, column = ci; the 9 taps of one (co, ci) are contiguous
  float* part = scratch + (size_t)blockIdx.x * Co * Ci * 9;
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int co = co0 + wco + c2 * 16 + 4 * g + r4, ci = ci0 + wci + j;
      if (co >= Co || ci >= Ci) continue;
      float* dst = part + ((size_t)co * Ci + ci) * 9;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) dst[tap] = acc[c2][tap][r4];
    }
}

// g_w[e] = sum_k scratch[k][e] in block order, four floats per thread
__global__ __launch_bounds__(256) void ux_reduce_kernel(long long n4, int nblk, const float* __restrict__ scratch,
                                                        float* __restrict__ g_w) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  const f32x4* src = reinterpret_cast<const f32x4*>(scratch) + e;
  f32x4 s = src[0];
#pragma unroll 4
  for (int k = 1; k < nblk; ++k) s += src[(size_t)k * n4];
  reinterpret_cast<f32x4*>(g_w)[e] = s;
}

// weight[Co,Ci,3,3] -> packed[hi|lo][tap][Cop / 8][Ci / 8][8 co][8 ci]; one thread per PACKED element, rows past Co: zeros
__global__ __launch_bounds__(256) void ux_pack_kernel(int Co, int Ci, int Cop, const float* __restrict__ w,
                                                      unsigned short* __restrict__ packed) {
  const long long n = (long long)Cop * Ci * 9, idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int tap = (int)(idx % 9), ci = (int)((idx / 9) % Ci), co = (int)(idx / (9ll * Ci));
  const float v = co < Co ? w[((size_t)co * Ci + ci) * 9 + tap] : 0.f;
  const __bf16 hi = (__bf16)v;
  const __bf16 lo = (__bf16)(v - (float)hi);
  const size_t o = ((((size_t)tap * (Cop >> 3) + (co >> 3)) * (Ci >> 3) + (ci >> 3)) * 8 + (co & 7)) * 8 + (ci & 7);
  packed[o] = __builtin_bit_cast(unsigned short, hi);
  packed[(size_t)n + o] = __builtin_bit_cast(unsigned short, lo);
}

bool ux_channels_ok(int Ci, int Co) { return Ci > 0 && Co > 0 && Ci % 32 == 0 && Co % 16 == 0; }

bool ux_supported(int B, int Ci, int Co, int Hi, int Wi) {
  return ux_channels_ok(Ci, Co) && Hi >= 1 && Wi >= 1 && B <= 65535;
}

// INVALID_ARG for negative sizes, a mode other than 0 / 1 and leak <= 0 in mode 0; UNSUPPORTED for shapes outside the rule
int ux_check(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak) {
  GOL_REQUIRE(B >= 0 && Ci >= 0 && Co >= 0 && Hi >= 0 && Wi >= 0, "bad sizes");
  GOL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (bias + LeakyReLU) or 1 (gate)");
  GOL_REQUIRE(mode != 0 || leak > 0.f, "leak must be positive (the backward reads the activation mask from the sign of y)");
  if (!ux_supported(B, Ci, Co, Hi, Wi)) {
    gol_set_error("gol_upconvx: Ci must be a positive multiple of 32, Co of 16, Hi and Wi >= 1, B <= 65535 (got B %d, "
                  "%d -> %d, %d x %d)", B, Ci, Co, Hi, Wi);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE((long long)Hi * Wi <= (1ll << 26), "plane too large (32-bit offsets inside a plane)");
  GOL_REQUIRE(gol_cdiv(Co, 16) <= 65535 && gol_cdiv(Ci, 32) <= 65535, "too many channel tiles");
  return GOL_OK;
}

// bwd_w: chunks of 32 pixels of an output row, and the K blocks they are walked in (chunks per block in *per)
long long ux_wchunks(int B, int Hi, int Wi) { return (long long)B * 2 * Hi * gol_cdiv(2 * Wi, kWPix); }

int ux_wblocks(int B, int Ci, int Co, int Hi, int Wi, int* per) {
  const long long nchunks = ux_wchunks(B, Hi, Wi), pairs = (long long)(Ci / kWCi) * gol_cdiv(Co, kWCo);
  long long nblk = (kWTarget + pairs - 1) / pairs;
  nblk = nblk > nchunks ? nchunks : nblk;
  nblk = nblk < 1 ? 1 : nblk;
  const long long pb = (nchunks + nblk - 1) / nblk;
  if (per) *per = (int)pb;
  return (int)((nchunks + pb - 1) / pb);  // no empty block
}

template <int EPI>
void ux_launch_fwd(const UxDims& p, const float* x, const unsigned short* pw, const float* a, const float* b, float* out,
                   float* out2, hipStream_t s) {
  const int tiles = gol_cdiv(p.H, kTH) * gol_cdiv(p.W, kTW);
  if (p.Co <= 16) ux_fwd_kernel<1, EPI><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, x, pw, a, b, out, out2);
  else if (p.Co <= 32) ux_fwd_kernel<2, EPI><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, x, pw, a, b, out, out2);
  else ux_fwd_kernel<4, EPI><<<dim3(tiles, p.B, gol_cdiv(p.Co, 64)), 256, 0, s>>>(p, x, pw, a, b, out, out2);
}

}  // namespace

extern "C" long long gol_upconvx_packed_elems(int Co, int Ci) {
  if (!ux_channels_ok(Ci, Co)) return 0;
  return 2ll * 9 * ((Co + 31) / 32 * 32) * Ci;
}

extern "C" int gol_upconvx_pack(int Co, int Ci, const float* weight, unsigned short* packed, void* stream) {
  GOL_REQUIRE(Co >= 0 && Ci >= 0, "bad sizes");
  if (!ux_channels_ok(Ci, Co)) {
    gol_set_error("gol_upconvx_pack: Ci must be a positive multiple of 32 and Co of 16 (got %d -> %d)", Ci, Co);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(weight && packed, "null pointer");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const int Cop = (Co + 31) / 32 * 32;
  ux_pack_kernel<<<gol_cdiv(9ll * Cop * Ci, 256), 256, 0, (hipStream_t)stream>>>(Co, Ci, Cop, weight, packed);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_upconvx_fwd(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale, const float* x,
                               const unsigned short* packed, const float* bias, const float* gate, const float* gb,
                               float* y, void* stream) {
  const int rc = ux_check(B, Ci, Co, Hi, Wi, mode, leak);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && packed && y, "null pointer");
  GOL_REQUIRE(mode == 0 ? bias != nullptr : gate != nullptr, "mode 0 needs bias, mode 1 needs gate");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const UxDims p{B, Ci, Co, Hi, Wi, 2 * Hi, 2 * Wi, mode, leak, scale};
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0) ux_launch_fwd<0>(p, x, packed, bias, nullptr, y, nullptr, s);
  else ux_launch_fwd<1>(p, x, packed, gate, gb, y, nullptr, s);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_upconvx_bwd_x(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale,
                                 const unsigned short* packed, const float* y, const float* gate, const float* g_y,
                                 float* g_x, void* stream) {
  const int rc = ux_check(B, Ci, Co, Hi, Wi, mode, leak);
  if (rc != GOL_OK) return rc;
  if (B == 0 || !g_x) return GOL_OK;
  const float* aux = mode == 0 ? y : gate;  // what g_pre is formed with
  GOL_REQUIRE(packed && g_y && aux, "null pointer (mode 0 needs y, mode 1 needs gate)");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const UxDims p{B, Ci, Co, Hi, Wi, 2 * Hi, 2 * Wi, mode, leak, scale};
  const int tiles = gol_cdiv(Hi, kXH) * gol_cdiv(Wi, kXW);
  hipStream_t s = (hipStream_t)stream;
  if (Ci <= 32) ux_bwd_x_kernel<2><<<dim3(tiles, B, 1), 256, 0, s>>>(p, packed, aux, g_y, g_x);
  else ux_bwd_x_kernel<4><<<dim3(tiles, B, gol_cdiv(Ci, 64)), 256, 0, s>>>(p, packed, aux, g_y, g_x);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" long long gol_upconvx_bwd_w_scratch_floats(int B, int Ci, int Co, int Hi, int Wi) {
  if (B <= 0 || !ux_supported(B, Ci, Co, Hi, Wi)) return 0;
  return (long long)ux_wblocks(B, Ci, Co, Hi, Wi, nullptr) * Co * Ci * 9;
}

extern "C" int gol_upconvx_bwd_w(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale, const float* x,
                                 const float* y, const float* gate, const float* g_y, float* g_w, float* scratch,
                                 void* stream) {
  const int rc = ux_check(B, Ci, Co, Hi, Wi, mode, leak);
  if (rc != GOL_OK) return rc;
  if (!g_w) return GOL_OK;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {  // an empty sum
    if (hipMemsetAsync(g_w, 0, sizeof(float) * 9 * (size_t)Co * Ci, s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  const float* aux = mode == 0 ? y : gate;
  GOL_REQUIRE(x && g_y && aux && scratch, "null pointer (mode 0 needs y, mode 1 needs gate)");
  GOL_REQUIRE(gol_aligned16(scratch) && gol_aligned16(g_w), "scratch and g_w must be 16-byte aligned");
  GOL_REQUIRE(ux_wchunks(B, Hi, Wi) <= 0x7fffffffll, "too many pixel chunks");
  const UxDims p{B, Ci, Co, Hi, Wi, 2 * Hi, 2 * Wi, mode, leak, scale};
  int per = 1;
  const int nblk = ux_wblocks(B, Ci, Co, Hi, Wi, &per);
  ux_bwd_w_kernel<<<dim3(nblk, Ci / kWCi, gol_cdiv(Co, kWCo)), 256, 0, s>>>(p, x, aux, g_y, scratch, per,
                                                                           (int)ux_wchunks(B, Hi, Wi));
  GOL_CHECK_LAUNCH();
  const long long n4 = 9ll * Co * Ci / 4;  // Co % 16 == 0
  ux_reduce_kernel<<<gol_cdiv(n4, 256), 256, 0, s>>>(n4, nblk, scratch, g_w);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_upconvx_bwd_gate(int B, int Ci, int Co, int Hi, int Wi, float scale, const float* x,
                                    const unsigned short* packed, const float* g_y, float* g_gate, float* g_gb,
                                    void* stream) {
  const int rc = ux_check(B, Ci, Co, Hi, Wi, 1, 0.f);
  if (rc != GOL_OK) return rc;
  if (B == 0 || !g_gate) return GOL_OK;
  GOL_REQUIRE(x && packed && g_y, "null pointer");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const UxDims p{B, Ci, Co, Hi, Wi, 2 * Hi, 2 * Wi, 1, 0.f, scale};
  ux_launch_fwd<2>(p, x, packed, g_y, nullptr, g_gate, g_gb, (hipStream_t)stream);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
