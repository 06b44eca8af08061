// vggconv.hip -- a layer of the frozen VGG19 feature network as one operator, forward and input gradient, gfx950.
//
// The masked VGG19 feature loss (ca_code/loss/vgg.py:52-88) runs 13 times 3x3 / stride 1 / pad 1
// convolution + bias + ReLU, four of them followed by a 2x2 / stride 2 max-pool, on `(clamp(x / 255, 0, 1) - mean) / std`.
// The weights are frozen: the backward is the input gradient alone.  For x[B,Ci,H,W], weight[Co,Ci,3,3], bias[Co]:
//     acc[b,co,r,c] = sum_{ci,ky,kx} xpad[b,ci,r-1+ky,c-1+kx] w[co,ci,ky,kx]              (xpad = x inside the image, 0 outside)
//     y = relu(acc + bias[co])                      pool: p[b,co,i,j] = max of y over the window rows 2i, 2i+1, columns 2j, 2j+1
// All GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32), operands A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15],
// D[i = 4 (lane >> 4) + r][j], as in upconv.hip.  ONE kernel template serves both directions: a workgroup owns 8 x 32 pixels
// x 16 CT rows of the GEMM (output channels forward, input channels backward); per K stage of 8 channels the haloed
// 10 x 34 window goes to LDS through a LOADER, the stage's weights as [tap][k][row], and every tap is one MFMA per
// (4 channels, 16 pixels, 16 rows).  An EPILOGUE runs on the accumulators.
//   loaders   plain   x as it is
//             image   Ci == 3: n = (clamp(x / 255.f, 0, 1) - mean_c) / std_c formed while loading (IEEE division, that
//                     operation order, no contraction: x = 255 gives exactly 1); mean = (0.485, 0.456, 0.406), std = (0.229,
//                     0.224, 0.225) (vgg.py:62-65).  The padding is zero in NORMALISED space: a pixel outside the image
//                     contributes 0, not (0 - mean) / std.  K = (tap, channel) is 27 padded to 28: 7 MFMAs per pixel tile.
//             g_y     backward without pool: g_pre = g_y where y > 0, else 0
//             g_p     backward with pool: g_pre[r,c] = g_p[r/2,c/2] where the position byte names (r,c) and p > 0, else 0 (a
//                     window whose maximum is 0 passes nothing; a last odd row or column belongs to no window)
//   epilogues relu    y = relu(acc + bias)
//             pool    only p[B,Co,H/2,W/2] (floor) and one byte per pooled element are written: the window position 0..3,
//                     row-major, of the maximum; the first maximum in that order wins a tie.  Tiles have an even origin and
//                     an even size, so no window straddles workgroups: the two rows of a window are two accumulator tiles
//                     of one lane, the two columns neighbouring lanes (one DPP quad permute).  A last odd row or column
//                     feeds nothing.
//             g_x     the transposed 3x3 convolution of g_pre: the same GEMM with the channel roles exchanged and the taps
//                     mirrored, A[ci][co][tap'] = w[co][ci][8 - tap'] read from the SAME weight (no flipped copy)
//             g_image Ci == 3 (a 16-row tile with zero weights in rows 3..15): g_image = g_n / std_c / 255 where
//                     0 <= x / 255 <= 1, edges inclusive as in torch's clamp backward, else 0
// No atomics, no scratch: every output element is written by exactly one lane from a fixed-order sum -- bitwise reproducible.
#include "gol_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct C3Dims {
  int B, M, K, H, W, Hp, Wp;  // M rows of the GEMM (channels written), K reduction channels (channels read), pooled size
};

constexpr int kTH = 8, kTW = 32;             // pixel tile (even origin, even size)
constexpr int kHR = kTH + 2, kHC = kTW + 2;  // its haloed window
constexpr int kKC = 8;                       // channels per K stage
constexpr int kPlane = 400;                  // >= 10 * 34, == 16 (mod 64): the 4 channel groups of a B read cover the banks

enum { L_PLAIN = 0, L_IMG = 1, L_GY = 2, L_GP = 3 };
enum { E_RELU = 0, E_POOL = 1, E_GX = 2, E_GIMG = 3 };

__device__ __forceinline__ float c3_std(int c) { return c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f); }

__device__ __forceinline__ float c3_normalise(float x, int c) {
  _Pragma("clang fp contract(off)")
  const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
  const float t = fminf(fmaxf(__fdiv_rn(x, 255.f), 0.f), 1.f);
  return __fdiv_rn(t - mean, c3_std(c));
}

// KC planes of the haloed window, origin (r0 - 1, c0 - 1), into LDS; outside the image and past K: zeros.  An item = one
// window position x 4 channels; the loads are unconditional (clamped to element 0 / the last channel, the value is dropped).
template <int LOAD, int KC>
__device__ __forceinline__ void c3_stage(float* s_u, const C3Dims& p, const float* __restrict__ in_b,
                                         const float* __restrict__ aux_b, const unsigned char* __restrict__ pos_b, int k0,
                                         int r0, int c0, int tid) {
  constexpr int N = (KC / 4) * kHR * kHC;
  const int H = p.H, W = p.W, K = p.K;
  const size_t PS = LOAD == L_GP ? (size_t)p.Hp * p.Wp : (size_t)H * W;
#pragma unroll
  for (int it = 0; it < (N + 255) / 256; ++it) {
    const int idx = tid + 256 * it, idc = min(idx, N - 1);
    const int grp = idc / (kHR * kHC), pos = idc - grp * (kHR * kHC), rr = pos / kHC, cc = pos - rr * kHC;
    const int r = r0 - 1 + rr, c = c0 - 1 + cc;
    bool in = r >= 0 && r < H && c >= 0 && c < W;
    unsigned o;
    int wpos = 0;
    if constexpr (LOAD == L_GP) {
      in = in && r < 2 * p.Hp && c < 2 * p.Wp;
      o = in ? (unsigned)(r >> 1) * (unsigned)p.Wp + (unsigned)(c >> 1) : 0u;
      wpos = (r & 1) * 2 + (c & 1);
    } else {
      o = in ? (unsigned)r * (unsigned)W + (unsigned)c : 0u;
    }
    float va[4], vb[4];
    int vp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t oo = (size_t)min(k0 + grp * 4 + u, K - 1) * PS + o;
      va[u] = in_b[oo];
      vb[u] = 1.f;
      vp[u] = 0;
      if constexpr (LOAD == L_GY || LOAD == L_GP) vb[u] = aux_b[oo];
      if constexpr (LOAD == L_GP) vp[u] = pos_b[oo];
    }
    if (idx < N) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int cl = grp * 4 + u;
        float v = va[u];
        if constexpr (LOAD == L_IMG) v = c3_normalise(v, cl);
        if constexpr (LOAD == L_GY) v = vb[u] > 0.f ? v : 0.f;
        if constexpr (LOAD == L_GP) v = (vp[u] == wpos && vb[u] > 0.f) ? v : 0.f;
        s_u[cl * kPlane + pos] = (in && k0 + cl < K) ? v : 0.f;
      }
    }
  }
}

// the stage's weights as s_w[tap][k][16 CT rows].  Forward: A[co][ci][tap] = w[co][ci][tap] (72 consecutive floats per co);
// TRANS: A[ci][co][tap'] = w[co][ci][8 - tap'] (the mirrored taps; 144 CT consecutive floats per co)
template <int CT, bool TRANS>
__device__ __forceinline__ void c3_stage_w(float* s_w, const C3Dims& p, const float* __restrict__ pw, int k0, int m0,
                                           int tid) {
  const int M = p.M, K = p.K;
  if constexpr (!TRANS) {
    for (int idx = tid; idx < 16 * CT * kKC * 9; idx += 256) {
      const int col = idx / (kKC * 9), rem = idx - col * (kKC * 9), kl = rem / 9, tap = rem - kl * 9;
      const int m = m0 + col, k = k0 + kl;
      s_w[(tap * kKC + kl) * (16 * CT) + col] = (m < M && k < K) ? pw[((size_t)m * K + k) * 9 + tap] : 0.f;
    }
  } else {
    for (int idx = tid; idx < kKC * 16 * CT * 9; idx += 256) {
      const int kl = idx / (144 * CT), rem = idx - kl * (144 * CT), col = rem / 9, tw = rem - col * 9;
      const int m = m0 + col, k = k0 + kl;
      s_w[((8 - tw) * kKC + kl) * (16 * CT) + col] = (m < M && k < K) ? pw[((size_t)k * M + m) * 9 + tw] : 0.f;
    }
  }
}

// D[m][pixel] += sum_{k, tap} A[m][k][tap] In[k][pixel + tap]: s_w[tap][k][16 CT], s_in[k][10][34]; poff = offset of the
// pixel's window origin (upconv.hip's core)
template <int CT>
__device__ __forceinline__ void c3_core(const float* s_in, const float* s_w, const int (&poff)[4], f32x4 (&acc)[4][CT], int j,
                                        int g) {
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
    for (int kk = 0; kk < kKC / 4; ++kk) {
      float a[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) a[ct] = s_w[((tap * kKC + kk * 4 + g) * CT + ct) * 16 + j];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const float bv = s_in[(kk * 4 + g) * kPlane + poff[pt] + ky * kHC + kx];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct], bv, acc[pt][ct], 0, 0, 0);
      }
    }
  }
}

// the image layer: k = 3 tap + channel, 27 padded to 28 (row 27 of s_w is zero): 7 K slices of 4
template <int CT>
__device__ __forceinline__ void c3_core_image(const float* s_in, const float* s_w, const int (&poff)[4], f32x4 (&acc)[4][CT],
                                              int j, int g) {
#pragma unroll
  for (int kk = 0; kk < 7; ++kk) {
    const int k = kk * 4 + g, kc = min(k, 26), tap = kc / 3, ch = kc - 3 * tap, ky = tap / 3, kx = tap - 3 * ky;
    const int koff = ch * kPlane + ky * kHC + kx;
    float a[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) a[ct] = s_w[(k * CT + ct) * 16 + j];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const float bv = s_in[koff + poff[pt]];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct], bv, acc[pt][ct], 0, 0, 0);
    }
  }
}

// the neighbouring lane's value (lane ^ 1): DPP quad_perm [1,0,3,2]; all lanes active
__device__ __forceinline__ float c3_lane_xor1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
}

// grid (tiles of 8 x 32 pixels, B, groups of 16 CT rows).  in: x (plain, image), g_y (g_y) or g_p (g_p); aux: y (g_y) or
// p (g_p); pos: the position bytes (g_p); ximg: the image (g_image); out: y, p or g_x; outpos: the position bytes (pool)
template <int CT, int LOAD, int EPI, bool TRANS>
__global__ __launch_bounds__(256) void c3_kernel(const C3Dims p, const float* __restrict__ pin, const float* __restrict__ paux,
                                                 const unsigned char* __restrict__ ppos, const float* __restrict__ pw,
                                                 const float* __restrict__ pbias, const float* __restrict__ pximg,
                                                 float* __restrict__ pout, unsigned char* __restrict__ poutpos) {
  __shared__ float s_u[kKC * kPlane];
  __shared__ float s_w[9 * kKC * 16 * CT];  // (the image layer uses 28 rows of it)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, M = p.M, K = p.K;
  const int ntx = (W + kTW - 1) / kTW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int r0 = ty * kTH, c0 = tx * kTW, b = blockIdx.y, m0 = blockIdx.z * (16 * CT);
  const size_t HW = (size_t)H * W, PS = LOAD == L_GP ? (size_t)p.Hp * p.Wp : HW;
  const float* in_b = pin + (size_t)b * K * PS;
  const float* aux_b = nullptr;
  const unsigned char* pos_b = nullptr;
  if constexpr (LOAD == L_GY || LOAD == L_GP) aux_b = paux + (size_t)b * K * PS;
  if constexpr (LOAD == L_GP) pos_b = ppos + (size_t)b * K * PS;
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
  if constexpr (LOAD == L_IMG) {
    c3_stage<L_IMG, 4>(s_u, p, in_b, nullptr, nullptr, 0, r0, c0, tid);
    for (int idx = tid; idx < 16 * CT * 28; idx += 256) {  // w[co][27 = (ci, tap)] -> s_w[3 tap + ci][co]; row 27 = 0
      const int col = idx / 28, rem = idx - col * 28, ch = rem / 9, tap = rem - ch * 9, m = m0 + col;
      if (rem < 27) s_w[(tap * 3 + ch) * (16 * CT) + col] = m < M ? pw[(size_t)m * 27 + rem] : 0.f;
      else s_w[27 * (16 * CT) + col] = 0.f;
    }
    __syncthreads();
    c3_core_image<CT>(s_u, s_w, poff, acc, j, g);
  } else {
    for (int k0 = 0; k0 < K; k0 += kKC) {
      __syncthreads();  // the previous stage has been consumed
      c3_stage<LOAD, kKC>(s_u, p, in_b, aux_b, pos_b, k0, r0, c0, tid);
      c3_stage_w<CT, TRANS>(s_w, p, pw, k0, m0, tid);
      __syncthreads();
      c3_core<CT>(s_u, s_w, poff, acc, j, g);
    }
  }
  // epilogue on the accumulators: D row = channel m0 + 16 ct + 4 g + r4, column = pixel j of the pixel tile
  if constexpr (EPI == E_POOL) {
    const int Hp = p.Hp, Wp = p.Wp, pr = (r0 >> 1) + wave;
#pragma unroll
    for (int half = 0; half < 2; ++half) {  // pixel tiles half (upper row) and half + 2 (lower row) of the same 16 columns
      const int pc = (c0 + pcol[half]) >> 1;
      const bool live = (j & 1) == 0 && pr < Hp && pc < Wp;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int m = m0 + 16 * ct + 4 * g + r4;
          const float bs = pbias[min(m, M - 1)];
          const float v0 = fmaxf(acc[half][ct][r4] + bs, 0.f), v2 = fmaxf(acc[half + 2][ct][r4] + bs, 0.f);
          const float v1 = c3_lane_xor1(v0), v3 = c3_lane_xor1(v2);
          float best = v0;
          int w = 0;
          if (v1 > best) { best = v1; w = 1; }
          if (v2 > best) { best = v2; w = 2; }
          if (v3 > best) { best = v3; w = 3; }
          if (live && m < M) {
            const size_t off = ((size_t)b * M + m) * ((size_t)Hp * Wp) + (unsigned)pr * (unsigned)Wp + (unsigned)pc;
            pout[off] = best;
            poutpos[off] = (unsigned char)w;
          }
        }
    }
  } else {
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
          if (m >= M) continue;
          const size_t off = ((size_t)b * M + m) * HW + o;
          const float a = acc[pt][ct][r4];
          if constexpr (EPI == E_RELU) {
            pout[off] = fmaxf(a + pbias[m], 0.f);
          } else if constexpr (EPI == E_GX) {
            pout[off] = a;
          } else {
            const float t = __fdiv_rn(pximg[off], 255.f);
            pout[off] = (t >= 0.f && t <= 1.f) ? __fdiv_rn(__fdiv_rn(a, c3_std(m)), 255.f) : 0.f;
          }
        }
    }
  }
}

int c3_check(int B, int Ci, int Co, int H, int W, int image_in, int pool) {
  GOL_REQUIRE(B >= 0 && Ci > 0 && Co > 0 && H > 0 && W > 0, "bad sizes");
  const bool ci_ok = image_in ? Ci == 3 : Ci % 8 == 0;
  if (!ci_ok || Co % 16 != 0 || B > 65535 || (pool && (H < 2 || W < 2))) {
    gol_set_error("gol_conv3: Ci must be 3 with image_in or a multiple of 8 without, Co a multiple of 16, B <= 65535, H and W "
                  ">= 2 with pool (got B %d, %d -> %d, %d x %d, image_in %d, pool %d)", B, Ci, Co, H, W, image_in, pool);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE((long long)H * W <= (1ll << 30), "plane too large (32-bit offsets inside a plane)");
  GOL_REQUIRE(gol_cdiv(Co, 64) <= 65535 && gol_cdiv(Ci, 64) <= 65535, "too many channel tiles");
  return GOL_OK;
}

template <int LOAD, int EPI, bool TRANS>
void c3_launch(const C3Dims& p, const float* in, const float* aux, const unsigned char* pos, const float* w,
               const float* bias, const float* ximg, float* out, unsigned char* outpos, hipStream_t s) {
  const int tiles = gol_cdiv(p.H, kTH) * gol_cdiv(p.W, kTW);
  if (EPI == E_GIMG || p.M <= 16)
    c3_kernel<1, LOAD, EPI, TRANS><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, in, aux, pos, w, bias, ximg, out, outpos);
  else if constexpr (EPI != E_GIMG) {
    if (p.M <= 32)
      c3_kernel<2, LOAD, EPI, TRANS><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, in, aux, pos, w, bias, ximg, out, outpos);
    else
      c3_kernel<4, LOAD, EPI, TRANS><<<dim3(tiles, p.B, gol_cdiv(p.M, 64)), 256, 0, s>>>(p, in, aux, pos, w, bias, ximg,
                                                                                         out, outpos);
  }
}

}  // namespace

extern "C" int gol_conv3_fwd(int B, int Ci, int Co, int H, int W, int image_in, int pool, const float* x,
                             const float* weight, const float* bias, float* y, unsigned char* pos, void* stream) {
  const int rc = c3_check(B, Ci, Co, H, W, image_in, pool);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && weight && bias && y, "null pointer");
  GOL_REQUIRE(!pool || pos, "pool needs the position bytes");
  const C3Dims p{B, Co, Ci, H, W, H / 2, W / 2};
  hipStream_t s = (hipStream_t)stream;
  if (image_in) {
    if (pool) c3_launch<L_IMG, E_POOL, false>(p, x, nullptr, nullptr, weight, bias, nullptr, y, pos, s);
    else c3_launch<L_IMG, E_RELU, false>(p, x, nullptr, nullptr, weight, bias, nullptr, y, nullptr, s);
  } else {
    if (pool) c3_launch<L_PLAIN, E_POOL, false>(p, x, nullptr, nullptr, weight, bias, nullptr, y, pos, s);
    else c3_launch<L_PLAIN, E_RELU, false>(p, x, nullptr, nullptr, weight, bias, nullptr, y, nullptr, s);
  }
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_conv3_bwd_x(int B, int Ci, int Co, int H, int W, int image_in, int pool, const float* x,
                               const float* weight, const float* y, const unsigned char* pos, const float* g_y, float* g_x,
                               void* stream) {
  const int rc = c3_check(B, Ci, Co, H, W, image_in, pool);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(weight && y && g_y && g_x, "null pointer");
  GOL_REQUIRE(!pool || pos, "pool needs the position bytes");
  GOL_REQUIRE(!image_in || x, "image_in needs x");
  const C3Dims p{B, Ci, Co, H, W, H / 2, W / 2};
  hipStream_t s = (hipStream_t)stream;
  if (image_in) {
    if (pool) c3_launch<L_GP, E_GIMG, true>(p, g_y, y, pos, weight, nullptr, x, g_x, nullptr, s);
    else c3_launch<L_GY, E_GIMG, true>(p, g_y, y, nullptr, weight, nullptr, x, g_x, nullptr, s);
  } else {
    if (pool) c3_launch<L_GP, E_GX, true>(p, g_y, y, pos, weight, nullptr, nullptr, g_x, nullptr, s);
    else c3_launch<L_GY, E_GX, true>(p, g_y, y, nullptr, weight, nullptr, nullptr, g_x, nullptr, s);
  }
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
