// conv3ub.hip -- a UNet level of the MVP teacher at precision "bf16x3", gfx950, wave64: 3x3 / stride 1 / pad 1 convolution of
// the channel concatenation of TWO tensors + untied bias [Co,H,W] + LeakyReLU, with all four gradients.  One level of
// OLATRGBDecoder.forward_rgb's UNet (ca_code/models/hand_teacher_mvp.py:444-467; layers built at :206-241 from
// la.Conv2dWNUB(Ci, Co, H, W, 3, 1, 1) + nn.LeakyReLU(0.2, inplace=True)) on the EFFECTIVE weight:
//     xcat = cat(xa[B,Ca,H,W], xb[B,Cb,H,W])  (never written; Cb = 0: xb absent), Ci = Ca + Cb
//     pre  = conv3x3(xcat_pad, w) + bias[co,r,c];  y = pre > 0 ? pre : leak pre
//     g_pre = y > 0 ? g_y : leak g_y    (formed while loading, THEN split: only y is kept, the activation is in place)
// The arithmetic and the conventions are those of conv3x.hip (read its header): v_mfma_f32_16x16x32_bf16, every operand
// split into hi = bf16_rne(v), lo = bf16_rne(v - hi) while it is staged, three MFMAs per product (lo lo dropped), fp32
// accumulation, zero padding splits to (0,0); every LDS image has 64-byte rows read 16 bytes per lane through cx_slot.
//   pack    w -> packed[hi|lo][tap][Co / 8][Cip / 8][8 co][8 ci], Cip = Ci rounded up to 32, the channels past Ci zeros: the
//           layout of gol_conv3x_pack at Cip channels, so cx_stage_w serves both directions as it stands.
//   fwd     cx_kernel's scheme (gol_conv3x_core.h): 8 x 32 pixels x 16 CT channels per workgroup (CT = 4, or 2 where there
//   bwd_x   are only 32 rows).  A K stage of 32 channels reads ONE source (Ca % 32 == 0 whenever Cb > 0); a last stage with
//           fewer than 32 channels (Ci = 56) stages zeros for the missing groups of 8 and reads nothing for them.  fwd adds
//           the bias plane (read as y is written: 16 consecutive floats per lane group) and applies the leak; bwd_x forms
//           g_pre in the loader, runs the transposed product (mirrored taps, blocks transposed on their way to LDS) and
//           writes rows [0,Ca) to g_xa and [Ca,Ci) to g_xb; a channel group none of whose rows has a destination exits.
//   bwd_w   c4_bwd_w_kernel's plan (conv4x.hip): the GEMM's K is the PIXEL.  A chunk = 32 pixels of one row; g_pre goes to
//           s_g[hi|lo][64 co][32], x to s_x[hi|lo][kx][3 rows][32 ci][32]: image kx holds x[X - 1 + kx] at X, so eight
//           pixels of a tap are one aligned 16-byte read.  A workgroup owns 64 co x 32 ci x 9 taps, a wave 32 x 16 (18
//           accumulator tiles, 54 MFMAs per 22 reads).  K is split over workgroups (contiguous runs of chunks); a partial
//           [Co][Ci][9] leaves per workgroup and cu_reduce_kernel adds the partials in block order.  Scratch = blocks x Co x
//           Ci x 9 floats <= (512 + channel-tile pairs) x 18432 floats, whatever B, H and W.
//   bwd_bias  g_bias[co,r,c] = sum_b g_pre[b,co,r,c], b ascending: one streaming pass, one thread per element.
// No float atomics; every output element is a fixed-order sum: bitwise reproducible.  No host sync, no allocation.
#include "gol_conv3x_core.h"

namespace {

struct CuDims {
  int B, Ca, Cb, Co, H, W;
  float leak;
};

constexpr int kWPix = 32;            // bwd_w: pixels per chunk
constexpr int kWCo = 64, kWCi = 32;  // bwd_w: channels per workgroup
constexpr int kWTarget = 512;        // bwd_w: workgroups aimed at (two per CU)

// 32 channels of the haloed window, origin (r0 - 1, c0 - 1), split into s_in[hi|lo][position][32]; outside the image and for
// the channels past nv (a multiple of 8): zeros.  in_s = channel 0 of this stage in its source; BWD: the value is g_pre,
// formed from g_y (in_s) and y (aux_s).  An item = one window position x 8 channels; the loads are unconditional (clamped to
// pixel 0 of the stage's first 8 channels, which exist; the value is dropped).
template <bool BWD>
__device__ __forceinline__ void cu_stage(unsigned short* s_in, int H, int W, const float* __restrict__ in_s,
                                         const float* __restrict__ aux_s, int nv, float leak, int r0, int c0, int tid) {
  constexpr int N = (kKS / 8) * kWin;
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
      va[u] = in_s[oo];
      vb[u] = 1.f;
      if constexpr (BWD) vb[u] = aux_s[oo];
    }
    f32x8 v;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float t = va[u];
      if constexpr (BWD) t = vb[u] > 0.f ? t : leak * t;
      v[u] = in ? t : 0.f;
    }
    bf16x8 hi, lo;
    cx_split(v, hi, lo);
    const int off = pos * kKS + cx_slot(pos, q) * 8;
    *reinterpret_cast<bf16x8*>(s_in + off) = hi;
    *reinterpret_cast<bf16x8*>(s_in + kWin * kKS + off) = lo;
  }
}

// grid (tiles of 8 x 32 pixels, B, groups of 16 CT rows).
// forward: in_a = xa, in_b = xb, out_a = y;  BWD: in_a = g_y, aux = y, out_a = g_xa, out_b = g_xb (either may be null)
template <int CT, bool BWD>
__global__ __launch_bounds__(256) void cu_kernel(const CuDims d, const float* __restrict__ in_a, const float* __restrict__ in_b,
                                                 const float* __restrict__ aux, const unsigned short* __restrict__ pw,
                                                 const float* __restrict__ pbias, float* __restrict__ out_a,
                                                 float* __restrict__ out_b) {
  __shared__ __attribute__((aligned(16))) unsigned short s_in[2 * kWin * kKS];
  __shared__ __attribute__((aligned(16))) unsigned short s_w[2 * 3 * 16 * CT * kKS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = d.H, W = d.W, Ca = d.Ca, Cb = d.Cb, Co = d.Co, Ci = Ca + Cb, Cip = (Ci + kKS - 1) / kKS * kKS;
  const int ntx = (W + kTW - 1) / kTW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int r0 = ty * kTH, c0 = tx * kTW, b = blockIdx.y, m0 = blockIdx.z * (16 * CT);
  const size_t HW = (size_t)H * W;
  if constexpr (BWD) {  // block-uniform: a group none of whose rows is wanted
    const bool want_a = out_a && m0 < Ca, want_b = out_b && m0 + 16 * CT > Ca && m0 < Ci;
    if (!want_a && !want_b) return;
  }
  // the packed weight as cx_stage_w sees it: M rows written, K channels read, the Ci side padded to Cip
  const CxDims pk{d.B, BWD ? Cip : Co, BWD ? Co : Cip, H, W, 0, 0};
  const int K = pk.K;
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
  for (int k0 = 0; k0 < K; k0 += kKS) {
    const float* in_s;
    const float* aux_s = nullptr;
    int nv = kKS;
    if constexpr (BWD) {
      in_s = in_a + ((size_t)b * Co + k0) * HW;
      aux_s = aux + ((size_t)b * Co + k0) * HW;
    } else if (k0 < Ca) {  // the source switch: a stage lies in one source
      in_s = in_a + ((size_t)b * Ca + k0) * HW;
      nv = min(kKS, Ca - k0);
    } else {
      in_s = in_b + ((size_t)b * Cb + (k0 - Ca)) * HW;
      nv = min(kKS, Ci - k0);
    }
    for (int ky = 0; ky < 3; ++ky) {
      __syncthreads();  // the previous tap row has been consumed
      if (ky == 0) cu_stage<BWD>(s_in, H, W, in_s, aux_s, nv, d.leak, r0, c0, tid);
      cx_stage_w<CT, BWD>(s_w, pk, pw, k0, m0, ky, tid);
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
        const int m = m0 + 16 * ct + 4 * g + r4;
        const float a = acc[pt][ct][r4];
        if constexpr (BWD) {
          if (m < Ca) {
            if (out_a) out_a[((size_t)b * Ca + m) * HW + o] = a;
          } else if (m < Ci) {
            if (out_b) out_b[((size_t)b * Cb + (m - Ca)) * HW + o] = a;
          }
        } else {
          if (m >= Co) continue;
          const float pre = a + pbias[(size_t)m * HW + o];
          out_a[((size_t)b * Co + m) * HW + o] = pre > 0.f ? pre : d.leak * pre;
        }
      }
  }
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------
// grid (K blocks, Cip / 32, groups of 64 output channels); chunk = (b, row r, 32 columns); block k walks chunks
// [k per, min((k + 1) per, nchunks)) and writes scratch[k][Co][Ci][9]
__global__ __launch_bounds__(256) void cu_bwd_w_kernel(const CuDims d, const float* __restrict__ pxa,
                                                       const float* __restrict__ pxb, const float* __restrict__ py,
                                                       const float* __restrict__ pgy, float* __restrict__ scratch, int per,
                                                       int nchunks) {
  constexpr int kXPlane = 3 * 3 * kWCi * kWPix;  // one of hi, lo of s_x
  __shared__ __attribute__((aligned(16))) unsigned short s_x[2 * kXPlane];        // 36,864 B
  __shared__ __attribute__((aligned(16))) unsigned short s_g[2 * kWCo * kWPix];   // 8,192 B
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int Ca = d.Ca, Cb = d.Cb, Co = d.Co, Ci = Ca + Cb, H = d.H, W = d.W;
  const int ci0 = blockIdx.y * kWCi, co0 = blockIdx.z * kWCo;
  const int wco = (wave & 1) * 32, wci = (wave >> 1) * 16;
  const int nxg = (W + kWPix - 1) / kWPix;
  const size_t HW = (size_t)H * W;
  // the 32 input channels of this workgroup lie in one source; nv of them exist (a multiple of 8, >= 8)
  const bool from_a = ci0 < Ca;
  const float* xs = from_a ? pxa : pxb;
  const int Cs = from_a ? Ca : Cb, cs0 = from_a ? ci0 : ci0 - Ca, nv = min(kWCi, Cs - cs0);
  f32x4 acc[2][9];
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[c2][tap] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ch_begin = blockIdx.x * per, ch_end = min(nchunks, ch_begin + per);
  for (int ch = ch_begin; ch < ch_end; ++ch) {
    const int b = ch / (H * nxg), rem = ch - b * (H * nxg), r = rem / nxg, X0 = (rem - r * nxg) * kWPix;
    __syncthreads();  // the previous chunk has been consumed
    {  // g_pre: one item = one channel x 8 pixels; channels past Co and pixels past W: zeros
      const int co = tid >> 2, xg = tid & 3;
      const bool cin = co0 + co < Co;
      const size_t base = ((size_t)b * Co + (cin ? co0 + co : 0)) * HW + (unsigned)r * (unsigned)W;
      float va[8], vy[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int Xc = min(X0 + xg * 8 + u, W - 1);  // clamped by arithmetic: no lane mask is kept across the loads
        va[u] = pgy[base + Xc];
        vy[u] = py[base + Xc];
      }
      f32x8 v;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float t = vy[u] > 0.f ? va[u] : d.leak * va[u];
        v[u] = (cin && X0 + xg * 8 + u < W) ? t : 0.f;
      }
      bf16x8 hi, lo;
      cx_split(v, hi, lo);
      const int off = co * kWPix + cx_slot(co, xg) * 8;
      *reinterpret_cast<bf16x8*>(s_g + off) = hi;
      *reinterpret_cast<bf16x8*>(s_g + kWCo * kWPix + off) = lo;
    }
#pragma unroll
    for (int it2 = 0; it2 < 2; ++it2) {  // x: one item = one channel x one row x 8 pixels: 10 columns -> 3 images
      const int it = tid + 256 * it2;
      if (it >= kWCi * 3 * 4) break;
      const int xg = it & 3, row = (it >> 2) % 3, ci = it / 12;
      const int rr = r - 1 + row, cb = X0 + xg * 8 - 1;
      const bool rin = rr >= 0 && rr < H && ci < nv;
      const float* src = xs + ((size_t)b * Cs + cs0 + (rin ? ci : 0)) * HW + (unsigned)(rin ? rr : 0) * (unsigned)W;
      float va[10];
#pragma unroll
      for (int t = 0; t < 10; ++t) {
        const int c = cb + t;
        va[t] = src[min(max(c, 0), W - 1)];
      }
#pragma unroll
      for (int t = 0; t < 10; ++t) {
        const int c = cb + t;
        va[t] = (rin && c >= 0 && c < W) ? va[t] : 0.f;
      }
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        f32x8 v;
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = va[kx + u];  // x[X0 + 8 xg + u - 1 + kx]
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
__global__ __launch_bounds__(256) void cu_reduce_kernel(long long n4, int nblk, const float* __restrict__ scratch,
                                                        float* __restrict__ g_w) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  const f32x4* src = reinterpret_cast<const f32x4*>(scratch) + e;
  f32x4 s = src[0];
#pragma unroll 4
  for (int k = 1; k < nblk; ++k) s += src[(size_t)k * n4];
  reinterpret_cast<f32x4*>(g_w)[e] = s;
}

// g_bias[e] = sum_b g_pre[b][e], b ascending; e over [Co, H, W]
__global__ __launch_bounds__(256) void cu_bwd_bias_kernel(long long n, int B, float leak, const float* __restrict__ py,
                                                          const float* __restrict__ pgy, float* __restrict__ g_bias) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
#pragma unroll 4
  for (int b = 0; b < B; ++b) {
    const float gv = pgy[(size_t)b * n + e];
    s += py[(size_t)b * n + e] > 0.f ? gv : leak * gv;
  }
  g_bias[e] = s;
}

// weight[Co,Ci,3,3] -> packed[hi|lo][tap][Co / 8][Cip / 8][8 co][8 ci]; one thread per PACKED element, channels past Ci: zeros
__global__ __launch_bounds__(256) void cu_pack_kernel(int Co, int Ci, int Cip, const float* __restrict__ w,
                                                      unsigned short* __restrict__ packed) {
  const long long n = (long long)Co * Cip * 9, idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int tap = (int)(idx % 9), ci = (int)((idx / 9) % Cip), co = (int)(idx / (9ll * Cip));
  const float v = ci < Ci ? w[((size_t)co * Ci + ci) * 9 + tap] : 0.f;
  const __bf16 hi = (__bf16)v;
  const __bf16 lo = (__bf16)(v - (float)hi);
  const size_t o = ((((size_t)tap * (Co >> 3) + (co >> 3)) * (Cip >> 3) + (ci >> 3)) * 8 + (co & 7)) * 8 + (ci & 7);
  packed[o] = __builtin_bit_cast(unsigned short, hi);
  packed[(size_t)n + o] = __builtin_bit_cast(unsigned short, lo);
}

int cu_pad32(int c) { return (c + 31) / 32 * 32; }

bool cu_channels_ok(int Ca, int Cb, int Co) {
  return Ca > 0 && Cb >= 0 && Co > 0 && Co % 32 == 0 && Ca % 8 == 0 && Cb % 8 == 0 && (Cb == 0 || Ca % 32 == 0);
}

bool cu_supported(int B, int Ca, int Cb, int Co, int H, int W) {
  return cu_channels_ok(Ca, Cb, Co) && H >= 1 && W >= 1 && B <= 65535;
}

int cu_check(int B, int Ca, int Cb, int Co, int H, int W) {
  if (!cu_supported(B, Ca, Cb, Co, H, W)) {
    gol_set_error("gol_conv3ub: Co must be a positive multiple of 32, Ca > 0 and Cb >= 0 multiples of 8, Ca a multiple of 32 "
                  "where Cb > 0, H and W >= 1, B <= 65535 (got B %d, %d + %d -> %d, %d x %d)", B, Ca, Cb, Co, H, W);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(B >= 0, "bad sizes");
  GOL_REQUIRE((long long)H * W <= (1ll << 30), "plane too large (32-bit offsets inside a plane)");
  GOL_REQUIRE(gol_cdiv(Co, 64) <= 65535 && gol_cdiv(Ca + Cb, 32) <= 65535, "too many channel tiles");
  return GOL_OK;
}

// bwd_w: chunks of 32 pixels of a row, and the K blocks they are walked in (chunks per block in *per)
long long cu_wchunks(int B, int H, int W) { return (long long)B * H * gol_cdiv(W, kWPix); }

int cu_wblocks(int B, int Ci, int Co, int H, int W, int* per) {
  const long long nchunks = cu_wchunks(B, H, W), pairs = (long long)(cu_pad32(Ci) / kWCi) * gol_cdiv(Co, kWCo);
  long long nblk = (kWTarget + pairs - 1) / pairs;
  nblk = nblk > nchunks ? nchunks : nblk;
  nblk = nblk < 1 ? 1 : nblk;
  const long long pb = (nchunks + nblk - 1) / nblk;
  if (per) *per = (int)pb;
  return (int)((nchunks + pb - 1) / pb);  // no empty block
}

}  // namespace

extern "C" long long gol_conv3ub_packed_elems(int Co, int Ci) {
  if (Co <= 0 || Ci <= 0 || Co % 32 != 0 || Ci % 8 != 0) return 0;
  return 2ll * 9 * Co * cu_pad32(Ci);
}

extern "C" int gol_conv3ub_pack(int Co, int Ci, const float* weight, unsigned short* packed, void* stream) {
  GOL_REQUIRE(Co > 0 && Ci > 0, "bad sizes");
  if (Co % 32 != 0 || Ci % 8 != 0) {
    gol_set_error("gol_conv3ub_pack: Co must be a multiple of 32 and Ci of 8 (got %d -> %d)", Ci, Co);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(weight && packed, "null pointer");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const int Cip = cu_pad32(Ci);
  cu_pack_kernel<<<gol_cdiv(9ll * Co * Cip, 256), 256, 0, (hipStream_t)stream>>>(Co, Ci, Cip, weight, packed);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_conv3ub_fwd(int B, int Ca, int Cb, int Co, int H, int W, float leak, const float* xa, const float* xb,
                               const unsigned short* packed, const float* bias, float* y, void* stream) {
  const int rc = cu_check(B, Ca, Cb, Co, H, W);
  if (rc != GOL_OK) return rc;
  GOL_REQUIRE(leak > 0.f, "leak must be positive");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(xa && (xb || Cb == 0) && packed && bias && y, "null pointer");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const CuDims d{B, Ca, Cb, Co, H, W, leak};
  const int tiles = gol_cdiv(H, kTH) * gol_cdiv(W, kTW);
  hipStream_t s = (hipStream_t)stream;
  if (Co <= 32) cu_kernel<2, false><<<dim3(tiles, B, 1), 256, 0, s>>>(d, xa, xb, nullptr, packed, bias, y, nullptr);
  else cu_kernel<4, false><<<dim3(tiles, B, gol_cdiv(Co, 64)), 256, 0, s>>>(d, xa, xb, nullptr, packed, bias, y, nullptr);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_conv3ub_bwd_x(int B, int Ca, int Cb, int Co, int H, int W, float leak, const unsigned short* packed,
                                 const float* y, const float* g_y, float* g_xa, float* g_xb, void* stream) {
  const int rc = cu_check(B, Ca, Cb, Co, H, W);
  if (rc != GOL_OK) return rc;
  GOL_REQUIRE(leak > 0.f, "leak must be positive");
  if (Cb == 0) g_xb = nullptr;
  if (B == 0 || (!g_xa && !g_xb)) return GOL_OK;
  GOL_REQUIRE(packed && y && g_y, "null pointer");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const CuDims d{B, Ca, Cb, Co, H, W, leak};
  const int tiles = gol_cdiv(H, kTH) * gol_cdiv(W, kTW), Ci = Ca + Cb;
  hipStream_t s = (hipStream_t)stream;
  if (Ci <= 32) cu_kernel<2, true><<<dim3(tiles, B, 1), 256, 0, s>>>(d, g_y, nullptr, y, packed, nullptr, g_xa, g_xb);
  else cu_kernel<4, true><<<dim3(tiles, B, gol_cdiv(Ci, 64)), 256, 0, s>>>(d, g_y, nullptr, y, packed, nullptr, g_xa, g_xb);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" long long gol_conv3ub_bwd_w_scratch_floats(int B, int Ca, int Cb, int Co, int H, int W) {
  if (B <= 0 || !cu_supported(B, Ca, Cb, Co, H, W)) return 0;
  return (long long)cu_wblocks(B, Ca + Cb, Co, H, W, nullptr) * Co * (Ca + Cb) * 9;
}

extern "C" int gol_conv3ub_bwd_w(int B, int Ca, int Cb, int Co, int H, int W, float leak, const float* xa, const float* xb,
                                 const float* y, const float* g_y, float* g_w, float* scratch, void* stream) {
  const int rc = cu_check(B, Ca, Cb, Co, H, W);
  if (rc != GOL_OK) return rc;
  GOL_REQUIRE(leak > 0.f, "leak must be positive");
  if (!g_w) return GOL_OK;
  const int Ci = Ca + Cb;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {  // an empty sum
    if (hipMemsetAsync(g_w, 0, sizeof(float) * 9 * (size_t)Co * Ci, s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  GOL_REQUIRE(xa && (xb || Cb == 0) && y && g_y && scratch, "null pointer");
  GOL_REQUIRE(gol_aligned16(scratch) && gol_aligned16(g_w), "scratch and g_w must be 16-byte aligned");
  GOL_REQUIRE(cu_wchunks(B, H, W) <= 0x7fffffffll, "too many pixel chunks");
  const CuDims d{B, Ca, Cb, Co, H, W, leak};
  int per = 1;
  const int nblk = cu_wblocks(B, Ci, Co, H, W, &per);
  cu_bwd_w_kernel<<<dim3(nblk, cu_pad32(Ci) / kWCi, gol_cdiv(Co, kWCo)), 256, 0, s>>>(d, xa, xb, y, g_y, scratch, per,
                                                                                     (int)cu_wchunks(B, H, W));
  GOL_CHECK_LAUNCH();
  const long long n4 = 9ll * Co * Ci / 4;  // Co % 32 == 0
  cu_reduce_kernel<<<gol_cdiv(n4, 256), 256, 0, s>>>(n4, nblk, scratch, g_w);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_conv3ub_bwd_bias(int B, int Co, int H, int W, float leak, const float* y, const float* g_y, float* g_bias,
                                    void* stream) {
  if (Co <= 0 || Co % 32 != 0 || H < 1 || W < 1 || B > 65535) {
    gol_set_error("gol_conv3ub_bwd_bias: Co must be a positive multiple of 32, H and W >= 1, B <= 65535 (got B %d, %d, "
                  "%d x %d)", B, Co, H, W);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(B >= 0, "bad sizes");
  GOL_REQUIRE(leak > 0.f, "leak must be positive");
  GOL_REQUIRE((long long)H * W <= (1ll << 30), "plane too large (32-bit offsets inside a plane)");
  if (!g_bias) return GOL_OK;
  const long long n = (long long)Co * H * W;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {  // an empty sum
    if (hipMemsetAsync(g_bias, 0, sizeof(float) * (size_t)n, s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  GOL_REQUIRE(y && g_y, "null pointer");
  cu_bwd_bias_kernel<<<gol_cdiv(n, 256), 256, 0, s>>>(n, B, leak, y, g_y, g_bias);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
