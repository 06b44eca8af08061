// mbconv.hip -- the front of an MBConv block of the frozen EfficientNet-B0 feature network, forward and input gradient, gfx950.
//
// The EfficientNet feature loss (ca_code/loss/effnet.py:16-69; `effnet`, `effnet_phys`, ca_code/loss/perceptual.py:60-69) runs
// torchvision's efficientnet_b0().features[0:4] on two full-size images.  An inverted-residual block there is
//     expand 1x1 + BN + SiLU  ->  depthwise k x k / stride s + BN + SiLU  ->  squeeze-excite  ->  project 1x1 + BN (+ input)
// and the expanded tensor e (6 x the block's input channels at the input's resolution) is pure traffic: 1.5 k MAC per
// pixel make it, the library writes it, re-reads and re-writes it for BatchNorm and SiLU and reads it for the depthwise
// convolution.  Here e NEVER exists in memory.  With BatchNorm folded into (weight, bias) on the host, for x[B,Ci,H,W],
// w_e[Ce,Ci], b_e[Ce], w_d[Ce,k,k], b_d[Ce], p = (k - 1) / 2, Ho = (H + 2p - k) / s + 1 (floor), Wo alike:
//     e[b,c,r,q]    = SiLU(sum_ci w_e[c,ci] x[b,ci,r,q] + b_e[c])                      (expand = 0: e = x, Ci == Ce)
//     z[b,c,ro,co]  = sum_{ky,kx} w_d[c,ky,kx] epad[b,c, ro s - p + ky, co s - p + kx] + b_d[c]     (the PRE-activation)
//     ssum[b,c]     = sum_{ro,co} SiLU(z[b,c,ro,co])                                                (the SE squeeze)
// epad = e inside the image and 0 outside -- NOT SiLU(b_e), which is what expanding a zero-padded x would give.
// SiLU(v) = v / (1 + expf(-v)): accurate expf, IEEE division, in that order.
//
// forward (mb_fwd_kernel): a workgroup (256 lanes) owns one tile of OUTPUT pixels of one image -- 8 x 32 (stride 1),
// 8 x 16 (stride 2) -- and walks the expanded channels in chunks of 16.  Per chunk
//   1. the chunk of e over the tile's haloed input window (k3 s1 10 x 34, k5 s1 12 x 36, k3 s2 17 x 33, k5 s2 19 x 35
//      pixels: 1.33, 1.69, 1.10, 1.30 input pixels expanded per input pixel owned) is recomputed into LDS: v_mfma_f32_16x16x4_f32 (exact fp32),
//      A[i = lane & 15][k = lane >> 4] = w_e[c0 + i][4 kk + k], B[k][j = lane & 15] = x[4 kk + k][pixel 16 pg + j] read
//      from global memory (the window of x stays in L2 across the chunks), D[i = 4 (lane >> 4) + r][j]; a wave holds the
//      accumulators of all its pixel groups and walks kk once, so A is loaded once per kk.  Bias, SiLU and the
//      zero-outside-the-image on the accumulators.  expand = 0 copies the chunk of x instead.
//   2. the depthwise convolution: a row of 16 lanes owns one channel (a wave: channels wave, wave + 4, wave + 8, wave + 12 of
//      the chunk), a lane the output columns l (and l + 16) of every output row; it walks the window's rows once, k LDS
//      reads per row and column, and scatters each row into the output rows it feeds.  Chunks are independent.
//   3. on the accumulators: z = acc + b_d written once; SiLU(z) summed per lane in double in a fixed order, the 16 lanes of
//      the row added by a DPP ladder, ONE double per (b, c, tile) written to partials[B,Ce,T].  The caller adds the T
//      partials (a `sum` over the last axis): no atomics, bitwise reproducible.
// backward (mb_bwd_kernel), the input gradient only (the net is frozen).  A workgroup owns 8 x 32 INPUT pixels (even
// origin) and up to 48 input channels, walks all chunks of 16 expanded channels and keeps the g_x accumulators:
//   a. g_zt = g_z + g_ssum[b,c] SiLU'(z), SiLU'(v) = sg (1 + v (1 - sg)), sg = 1 / (1 + expf(-v)), formed while loading the
//      window of outputs the tile feeds, 0 outside the output;
//   b. g_e = the transposed depthwise convolution of g_zt from the SAME w_d with mirrored taps (no flipped copy); with
//      stride 2 a position receives only the taps of its parity (rows: static per tile row; columns: the lane's);
//   c. e_pre recomputed from x on the MFMA (no halo), g_epre = g_e SiLU'(e_pre);
//   d. g_x[ci] += sum_c w_e[c,ci] g_epre on the MFMA, A[i = ci][k = c], B[k = c][j = pixel] through LDS.
// expand = 0: g_x = g_e, written straight from step b.  No atomics, no scratch; every element written by one lane.
#include "gol_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct MbDims {
  int B, Ci, Ce, H, W, Ho, Wo;
};

__device__ __forceinline__ float mb_silu(float v) { return __fdiv_rn(v, 1.f + expf(-v)); }
__device__ __forceinline__ float mb_dsilu(float v) {
  const float sg = __fdiv_rn(1.f, 1.f + expf(-v));
  return sg * (1.f + v * (1.f - sg));
}

// sum over the 16 lanes of a DPP row, valid in lane 15 of the row (all lanes active)
__device__ __forceinline__ double mb_row_sum(double v) {
  v = gol_dpp_add0<0x111, 0xf>(v);
  v = gol_dpp_add0<0x112, 0xf>(v);
  v = gol_dpp_add0<0x114, 0xf>(v);
  return gol_dpp_add0<0x118, 0xf>(v);
}

template <int K, int S>
struct MbFwd {
  static constexpr int P = (K - 1) / 2;
  static constexpr int TOH = 8, TOW = 32 / S, NH = TOW / 16;  // output tile, column halves
  static constexpr int IH = (TOH - 1) * S + K, IW = (TOW - 1) * S + K, NPIX = IH * IW;  // its haloed input window
  static constexpr int NPG = (NPIX + 15) / 16, PGW = (NPG + 3) / 4;                     // pixel groups of 16, per wave
  static constexpr int EP = ((NPIX + 59) / 64) * 64 + 4;  // plane stride == 4 (mod 64): D-layout stores and the four
                                                          // channels of a wave's depthwise reads cover the banks
};

// grid (output tiles, B)
template <int K, int S, bool EXPAND>
__global__ __launch_bounds__(256) void mb_fwd_kernel(const MbDims d, const float* __restrict__ px,
                                                     const float* __restrict__ pwe, const float* __restrict__ pbe,
                                                     const float* __restrict__ pwd, const float* __restrict__ pbd,
                                                     float* __restrict__ pz, double* __restrict__ ppart) {
  using T = MbFwd<K, S>;
  __shared__ float s_e[16 * T::EP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = d.H, W = d.W, Ci = d.Ci, Ce = d.Ce, Ho = d.Ho, Wo = d.Wo;
  const int ntx = (Wo + T::TOW - 1) / T::TOW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int ro0 = ty * T::TOH, co0 = tx * T::TOW, ri0 = ro0 * S - T::P, ci0 = co0 * S - T::P, b = blockIdx.y;
  const size_t HW = (size_t)H * W;
  const float* x_b = px + (size_t)b * Ci * HW;
  const int cl = wave + 4 * g;  // depthwise: the channel of this lane's row of 16; l = j

  // per pixel group of the lane: the offset of its pixel inside a plane of x (0 outside the image) and an all-ones /
  // all-zeros word that keeps or clears the value (loads stay unconditional, no lane mask lives across the K loop)
  unsigned off[T::PGW], keep[T::PGW];
  if constexpr (EXPAND) {
#pragma unroll
    for (int i = 0; i < T::PGW; ++i) {
      const int p = (wave + 4 * i) * 16 + j, rr = p / T::IW, cc = p - rr * T::IW, r = ri0 + rr, c = ci0 + cc;
      const bool in = p < T::NPIX && r >= 0 && r < H && c >= 0 && c < W;
      off[i] = in ? (unsigned)(r * W + c) : 0u;
      keep[i] = in ? 0xffffffffu : 0u;
    }
  }

  for (int c0 = 0; c0 < Ce; c0 += 16) {
    __syncthreads();  // the previous chunk of e has been consumed
    if constexpr (EXPAND) {
      f32x4 acc[T::PGW];
#pragma unroll
      for (int i = 0; i < T::PGW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* wrow = pwe + (size_t)(c0 + j) * Ci + g;
      for (int kk = 0; kk < Ci / 4; ++kk) {
        const float a = wrow[kk * 4];
        const float* xk = x_b + (size_t)(kk * 4 + g) * HW;
#pragma unroll
        for (int i = 0; i < T::PGW; ++i) {
          const float bv = __uint_as_float(__float_as_uint(xk[off[i]]) & keep[i]);
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[i], 0, 0, 0);
        }
      }
      float be[4];
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) be[r4] = pbe[c0 + 4 * g + r4];
#pragma unroll
      for (int i = 0; i < T::PGW; ++i) {
        const int p = (wave + 4 * i) * 16 + j;
        if (p < T::NPIX) {
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4)
            s_e[(4 * g + r4) * T::EP + p] = __uint_as_float(__float_as_uint(mb_silu(acc[i][r4] + be[r4])) & keep[i]);
        }
      }
    } else {
      for (int idx = tid; idx < 16 * T::NPIX; idx += 256) {
        const int ch = idx / T::NPIX, p = idx - ch * T::NPIX, rr = p / T::IW, cc = p - rr * T::IW;
        const int r = ri0 + rr, c = ci0 + cc;
        const bool in = r >= 0 && r < H && c >= 0 && c < W;
        s_e[ch * T::EP + p] = in ? x_b[(size_t)(c0 + ch) * HW + (unsigned)(r * W + c)] : 0.f;
      }
    }
    __syncthreads();

    float w[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) w[t] = pwd[(size_t)(c0 + cl) * (K * K) + t];
    float acc[T::TOH][T::NH];
#pragma unroll
    for (int ro = 0; ro < T::TOH; ++ro)
#pragma unroll
      for (int h = 0; h < T::NH; ++h) acc[ro][h] = 0.f;
    const float* e_c = s_e + cl * T::EP + j * S;
#pragma unroll
    for (int ir = 0; ir < T::IH; ++ir) {
#pragma unroll
      for (int h = 0; h < T::NH; ++h) {
        float row[K];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) row[kx] = e_c[ir * T::IW + 16 * h * S + kx];
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
          const int t = ir - ky;
          if (t >= 0 && t % S == 0 && t / S < T::TOH) {
#pragma unroll
            for (int kx = 0; kx < K; ++kx) acc[t / S][h] += w[ky * K + kx] * row[kx];
          }
        }
      }
    }
    const float bd = pbd[c0 + cl];
    float* z_c = pz + ((size_t)b * Ce + c0 + cl) * ((size_t)Ho * Wo);
    double s = 0.0;
#pragma unroll
    for (int ro = 0; ro < T::TOH; ++ro)
#pragma unroll
      for (int h = 0; h < T::NH; ++h) {
        const int R = ro0 + ro, C = co0 + j + 16 * h;
        const float zv = acc[ro][h] + bd;
        if (R < Ho && C < Wo) {
          z_c[(unsigned)(R * Wo + C)] = zv;
          s += (double)mb_silu(zv);
        }
      }
    s = mb_row_sum(s);
    if (j == 15) ppart[((size_t)b * Ce + c0 + cl) * gridDim.x + blockIdx.x] = s;
  }
}

template <int K, int S>
struct MbBwd {
  static constexpr int P = (K - 1) / 2, TH = 8, TW = 32;  // tile of input pixels (origin a multiple of the stride)
  // window of outputs the tile feeds, relative to (r0 / S, c0 / S): ro = (r + P - ky) / S over r < TH, ky < K
  static constexpr int RLO = -(P / S), RHI = (TH - 1 + P) / S, GR = RHI - RLO + 1;
  static constexpr int CLO = -(P / S), CHI = (TW - 1 + P) / S, GC = CHI - CLO + 1;
  static constexpr int NG = GR * GC, GP = ((NG + 59) / 64) * 64 + 4;
  static constexpr int NM = S == 1 ? K : (K + 1) / 2;  // column taps a position can receive
  static constexpr int GEP = TH * TW + 4;              // plane stride of g_e
};

// grid (input tiles, B, groups of 16 MT input channels)
template <int K, int S, bool EXPAND, int MT>
__global__ __launch_bounds__(256) void mb_bwd_kernel(const MbDims d, const float* __restrict__ px,
                                                     const float* __restrict__ pwe, const float* __restrict__ pbe,
                                                     const float* __restrict__ pwd, const float* __restrict__ pz,
                                                     const float* __restrict__ pgz, const float* __restrict__ pgs,
                                                     float* __restrict__ pgx) {
  using T = MbBwd<K, S>;
  __shared__ float s_g[16 * T::GP];
  __shared__ float s_ge[EXPAND ? 16 * T::GEP : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = d.H, W = d.W, Ci = d.Ci, Ce = d.Ce, Ho = d.Ho, Wo = d.Wo;
  const int ntx = (W + T::TW - 1) / T::TW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int r0 = ty * T::TH, c0p = tx * T::TW, b = blockIdx.y, cig0 = blockIdx.z * (16 * MT);
  const int go_r = r0 / S + T::RLO, go_c = c0p / S + T::CLO;  // the output window's origin
  const size_t HW = (size_t)H * W, HWo = (size_t)Ho * Wo;
  const float* x_b = px + (size_t)b * Ci * HW;
  const int cl = wave + 4 * g;  // step b: the channel of this lane's row of 16

  // step b: the lane's column taps.  stride 1: kx = m.  stride 2: kx = par + 2 m with par the parity of (column + P); a
  // tap past the filter keeps a valid address and gets weight 0.
  const int par = S == 1 ? 0 : ((j + T::P) & 1);
  int gcol[T::NM];
  bool tap_ok[T::NM];
#pragma unroll
  for (int m = 0; m < T::NM; ++m) {
    const int kx = S == 1 ? m : par + 2 * m;
    tap_ok[m] = kx < K;
    gcol[m] = (j + T::P - (tap_ok[m] ? kx : par)) / S - T::CLO;  // exact division: the numerator is >= -P and even for S = 2
  }
  // steps c, d: pixel group i of the wave = tile row (4 wave + i) / 2, columns 16 ((4 wave + i) & 1) + j
  int off[4];
  f32x4 gx[4][MT];
  if constexpr (EXPAND) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pg = 4 * wave + i, R = r0 + (pg >> 1), C = c0p + 16 * (pg & 1) + j;
      off[i] = (R < H && C < W) ? R * W + C : -1;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) gx[i][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  for (int c0 = 0; c0 < Ce; c0 += 16) {
    // a. g_zt over the output window (the barriers of the previous chunk order these writes after its reads)
    for (int idx = tid; idx < 16 * T::NG; idx += 256) {
      const int ch = idx / T::NG, t = idx - ch * T::NG, gr = t / T::GC, gc = t - gr * T::GC;
      const int ro = go_r + gr, co = go_c + gc;
      float v = 0.f;
      if (ro >= 0 && ro < Ho && co >= 0 && co < Wo) {
        const size_t o = ((size_t)b * Ce + c0 + ch) * HWo + (unsigned)(ro * Wo + co);
        v = pgz[o] + pgs[(size_t)b * Ce + c0 + ch] * mb_dsilu(pz[o]);
      }
      s_g[ch * T::GP + t] = v;
    }
    float w[K][T::NM];
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
      for (int m = 0; m < T::NM; ++m) {
        const int kx = S == 1 ? m : par + 2 * m;
        w[ky][m] = tap_ok[m] ? pwd[(size_t)(c0 + cl) * (K * K) + ky * K + kx] : 0.f;
      }
    __syncthreads();

    // b. g_e[r][column j + 16 h] of channel cl: walk the window's rows once, scatter each into the tile rows it feeds
    float ge[T::TH][2];
#pragma unroll
    for (int r = 0; r < T::TH; ++r) ge[r][0] = ge[r][1] = 0.f;
    const float* g_c = s_g + cl * T::GP;
#pragma unroll
    for (int gr = 0; gr < T::GR; ++gr) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float val[T::NM];
#pragma unroll
        for (int m = 0; m < T::NM; ++m) val[m] = g_c[gr * T::GC + gcol[m] + (16 / S) * h];
#pragma unroll
        for (int r = 0; r < T::TH; ++r)
#pragma unroll
          for (int ky = 0; ky < K; ++ky) {
            const int tr = r + T::P - ky;  // = S (ro - r0 / S)
            if (tr % S == 0 && tr / S - T::RLO == gr) {
#pragma unroll
              for (int m = 0; m < T::NM; ++m) ge[r][h] += w[ky][m] * val[m];
            }
          }
      }
    }
    if constexpr (!EXPAND) {
#pragma unroll
      for (int r = 0; r < T::TH; ++r)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int R = r0 + r, C = c0p + j + 16 * h;
          if (R < H && C < W) pgx[((size_t)b * Ci + c0 + cl) * HW + (unsigned)(R * W + C)] = ge[r][h];
        }
      __syncthreads();  // s_g consumed
    } else {
#pragma unroll
      for (int r = 0; r < T::TH; ++r)
#pragma unroll
        for (int h = 0; h < 2; ++h) s_ge[cl * T::GEP + r * T::TW + j + 16 * h] = ge[r][h];
      __syncthreads();

      // c. e_pre of the tile's pixels, g_epre = g_e SiLU'(e_pre) in place (D layout: channels 4 g + r4, pixel j)
      f32x4 ep[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ep[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* wrow = pwe + (size_t)(c0 + j) * Ci + g;
      for (int kk = 0; kk < Ci / 4; ++kk) {
        const float a = wrow[kk * 4];
        const float* xk = x_b + (size_t)(kk * 4 + g) * HW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float bv = off[i] >= 0 ? xk[off[i]] : 0.f;
          ep[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, ep[i], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const float be = pbe[c0 + 4 * g + r4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int q = (4 * g + r4) * T::GEP + (4 * wave + i) * 16 + j;
          s_ge[q] = s_ge[q] * mb_dsilu(ep[i][r4] + be);
        }
      }
      __syncthreads();

      // d. g_x[ci = cig0 + 16 mt + i][pixel] += sum over the chunk's channels
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        float a[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int ci = cig0 + 16 * mt + j;
          a[mt] = ci < Ci ? pwe[(size_t)(c0 + 4 * kk + g) * Ci + ci] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float bv = s_ge[(4 * kk + g) * T::GEP + (4 * wave + i) * 16 + j];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) gx[i][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], bv, gx[i][mt], 0, 0, 0);
        }
      }
    }
  }
  if constexpr (EXPAND) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (off[i] < 0) continue;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int ci = cig0 + 16 * mt + 4 * g + r4;
          if (ci < Ci) pgx[((size_t)b * Ci + ci) * HW + (unsigned)off[i]] = gx[i][mt][r4];
        }
    }
  }
}

int mb_out(int n, int k, int s) { return (n + 2 * ((k - 1) / 2) - k) / s + 1; }

template <int K, int S>
int mb_tiles_of(int H, int W) {
  return gol_cdiv(mb_out(H, K, S), MbFwd<K, S>::TOH) * gol_cdiv(mb_out(W, K, S), MbFwd<K, S>::TOW);
}

int mb_tiles(int H, int W, int k, int s) {
  if (k == 3) return s == 1 ? mb_tiles_of<3, 1>(H, W) : mb_tiles_of<3, 2>(H, W);
  return s == 1 ? mb_tiles_of<5, 1>(H, W) : mb_tiles_of<5, 2>(H, W);
}

int mb_check(int B, int Ci, int Ce, int H, int W, int k, int stride, int expand) {
  GOL_REQUIRE(B >= 0 && Ci > 0 && Ce > 0 && H > 0 && W > 0, "bad sizes");
  if ((k != 3 && k != 5) || (stride != 1 && stride != 2) || Ci % 8 != 0 || Ce % 16 != 0 || B > 65535 ||
      (!expand && Ci != Ce)) {
    gol_set_error("gol_mbconv_front: k must be 3 or 5, stride 1 or 2, Ci a multiple of 8, Ce a multiple of 16, B <= 65535, "
                  "Ci == Ce without expand (got B %d, %d -> %d, %d x %d, k %d, stride %d, expand %d)", B, Ci, Ce, H, W, k,
                  stride, expand);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE((long long)H * W <= (1ll << 30), "plane too large (32-bit offsets inside a plane)");
  GOL_REQUIRE(gol_cdiv(Ci, 48) <= 65535, "too many input channel groups");
  return GOL_OK;
}

template <int K, int S>
void mb_launch_fwd(const MbDims& d, int expand, const float* x, const float* we, const float* be, const float* wd,
                   const float* bd, float* z, double* part, hipStream_t s) {
  const dim3 grid(mb_tiles_of<K, S>(d.H, d.W), d.B);
  if (expand) mb_fwd_kernel<K, S, true><<<grid, 256, 0, s>>>(d, x, we, be, wd, bd, z, part);
  else mb_fwd_kernel<K, S, false><<<grid, 256, 0, s>>>(d, x, we, be, wd, bd, z, part);
}

template <int K, int S>
void mb_launch_bwd(const MbDims& d, int expand, const float* x, const float* we, const float* be, const float* wd,
                   const float* z, const float* gz, const float* gs, float* gx, hipStream_t s) {
  const int tiles = gol_cdiv(d.H, MbBwd<K, S>::TH) * gol_cdiv(d.W, MbBwd<K, S>::TW);
  if (!expand) mb_bwd_kernel<K, S, false, 1><<<dim3(tiles, d.B, 1), 256, 0, s>>>(d, x, we, be, wd, z, gz, gs, gx);
  else if (d.Ci <= 16) mb_bwd_kernel<K, S, true, 1><<<dim3(tiles, d.B, 1), 256, 0, s>>>(d, x, we, be, wd, z, gz, gs, gx);
  else if (d.Ci <= 32) mb_bwd_kernel<K, S, true, 2><<<dim3(tiles, d.B, 1), 256, 0, s>>>(d, x, we, be, wd, z, gz, gs, gx);
  else mb_bwd_kernel<K, S, true, 3><<<dim3(tiles, d.B, gol_cdiv(d.Ci, 48)), 256, 0, s>>>(d, x, we, be, wd, z, gz, gs, gx);
}

}  // namespace

extern "C" int gol_mbconv_front_tiles(int H, int W, int k, int stride) {
  if (H < 1 || W < 1 || (k != 3 && k != 5) || (stride != 1 && stride != 2)) return 0;
  return mb_tiles(H, W, k, stride);
}

extern "C" int gol_mbconv_front_fwd(int B, int Ci, int Ce, int H, int W, int k, int stride, int expand, const float* x,
                                    const float* w_e, const float* b_e, const float* w_d, const float* b_d, float* z,
                                    double* partials, void* stream) {
  const int rc = mb_check(B, Ci, Ce, H, W, k, stride, expand);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && w_d && b_d && z && partials, "null pointer");
  GOL_REQUIRE(!expand || (w_e && b_e), "expand needs w_e and b_e");
  const MbDims d{B, Ci, Ce, H, W, mb_out(H, k, stride), mb_out(W, k, stride)};
  hipStream_t s = (hipStream_t)stream;
  if (k == 3) {
    if (stride == 1) mb_launch_fwd<3, 1>(d, expand, x, w_e, b_e, w_d, b_d, z, partials, s);
    else mb_launch_fwd<3, 2>(d, expand, x, w_e, b_e, w_d, b_d, z, partials, s);
  } else {
    if (stride == 1) mb_launch_fwd<5, 1>(d, expand, x, w_e, b_e, w_d, b_d, z, partials, s);
    else mb_launch_fwd<5, 2>(d, expand, x, w_e, b_e, w_d, b_d, z, partials, s);
  }
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_mbconv_front_bwd_x(int B, int Ci, int Ce, int H, int W, int k, int stride, int expand, const float* x,
                                      const float* w_e, const float* b_e, const float* w_d, const float* z,
                                      const float* g_z, const float* g_ssum, float* g_x, void* stream) {
  const int rc = mb_check(B, Ci, Ce, H, W, k, stride, expand);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(w_d && z && g_z && g_ssum && g_x, "null pointer");
  GOL_REQUIRE(!expand || (x && w_e && b_e), "expand needs x, w_e and b_e");
  const MbDims d{B, Ci, Ce, H, W, mb_out(H, k, stride), mb_out(W, k, stride)};
  hipStream_t s = (hipStream_t)stream;
  if (k == 3) {
    if (stride == 1) mb_launch_bwd<3, 1>(d, expand, x, w_e, b_e, w_d, z, g_z, g_ssum, g_x, s);
    else mb_launch_bwd<3, 2>(d, expand, x, w_e, b_e, w_d, z, g_z, g_ssum, g_x, s);
  } else {
    if (stride == 1) mb_launch_bwd<5, 1>(d, expand, x, w_e, b_e, w_d, z, g_z, g_ssum, g_x, s);
    else mb_launch_bwd<5, 2>(d, expand, x, w_e, b_e, w_d, z, g_z, g_ssum, g_x, s);
  }
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
