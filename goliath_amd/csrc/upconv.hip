// upconv.hip -- one layer of URHand's texture decoder as one operator, forward and backward, gfx950.
//
// The two 7-layer texture branches of ConvTeacherDecoder.forward (/root/reference/ca_code/models/urhand.py:583-608, layers
// built at :302-323) do, per layer, an exact 2x bilinear resize (align_corners=True) followed by a weight-normalised 3x3 /
// stride 1 / pad 1 convolution with either an untied bias + LeakyReLU (texmod0) or a gate by the other branch's activation
// (+ gainbias, * 0.707107) (texmod1).  Here, for x[B,Ci,Hi,Wi], H = 2 Hi, W = 2 Wi:
//     U[b,ci,r,c]   = bilinear(x[b,ci]) at (r (Hi-1)/(H-1), c (Wi-1)/(W-1)), by the INTEGER-RATIO rule
//                     r0 = (r (Hi-1)) div (H-1), frac = float((r (Hi-1)) mod (H-1)) / float(H-1), r1 = min(r0+1, Hi-1)
//     acc[b,co,r,c] = sum_{ci,ky,kx} Upad[b,ci,r-1+ky,c-1+kx] w[co,ci,ky,kx]           (Upad = U inside the image, 0 outside)
//     mode 0:  y = lrelu(acc + bias[co,r,c])        mode 1:  y = (acc gate[b,co,r,c] + gb[b,co,r,c]) scale
// U never exists in memory.  All GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32), operands A[i = lane & 15][k = lane >> 4],
// B[k][j = lane & 15], D[i = 4 (lane >> 4) + r][j], as in encconv.hip / trunk.hip.
//   fwd     a workgroup owns 8 x 32 output pixels x 16 CT output channels.  Per K stage of 8 input channels the haloed
//           window of U (10 x 34) is BLENDED INTO LDS from the up-to-2x2 source texels of x (row / column tables of the
//           tile: source offsets and fractions, one integer division per row and column of the tile, none per texel; a
//           thread looks a window position up once and blends 4 channels at it),
//           the stage's weights go to LDS as [tap][ci][co], and every tap is one MFMA per (4 channels, 16 pixels, 16 co):
//           D[co][pixel] += W[co][ci] U[ci][pixel + tap].  The epilogue runs on the accumulators; a third epilogue
//           (g_gate = scale g_y acc, g_gb = scale g_y) makes the same kernel the gate gradient of mode 1 with acc recomputed.
//           Co <= 4 (the last layer, 16 -> 4) takes the same kernel with the missing rows as zero weights.
//   bwd     g_pre = g_y (y > 0 ? 1 : leak) (mode 0) or scale gate g_y (mode 1) is formed while loading.
//     bwd_x   a workgroup owns 4 x 16 texels of x x 16 input channels.  The U rows that reach source row i are those with
//             |r (Hi-1)/(H-1) - i| < 1: for the tile at most 12 x 36 pixels of g_U.  That region of g_U = the transposed
//             3x3 convolution of g_pre is the forward's GEMM with the roles of the channels exchanged and the taps
//             mirrored (B operand: a 14 x 38 window of g_pre per K stage of 8 output channels, 4 for Co <= 4); it goes to LDS and
//             every texel GATHERS its up-to-5x5 pixels with the bilinear weights of the forward's rule.  g_U never goes
//             to memory; no atomics.
//     bwd_w   per (16 co x 16 ci) a GEMM over pixels, D[co][ci] += g_pre[co][pixel] U[ci][pixel + tap], nine accumulator
//             tiles; U comes from the forward's loader.  K (the 8 x 32 tiles of all views) is split over workgroups,
//             the partial sums go to scratch and a second kernel adds them in a fixed order (bitwise reproducible).
//     bwd_s   the streaming rest: g_bias = sum_b g_pre (mode 0), g_gb = scale g_y when the gate gradient is not wanted.
#include "gol_upconv.h"  // the coordinate tables, up_stage_u, up_conv_core, the weight gradient's reduction

namespace {

struct UpDims {
  int B, Ci, Co, Hi, Wi, H, W, mode;
  float leak, scale;
};

__device__ __forceinline__ float up_gpre(const UpDims& p, float g, float aux) {
  return p.mode == 0 ? g * (aux > 0.f ? 1.f : p.leak) : p.scale * g * aux;
}

// ---- forward ---------------------------------------------------------------------------------------------------------
// grid (tiles of 8 x 32 pixels, B, groups of 16 CT output channels).  EPI 0: y = lrelu(acc + bias) (pa = bias);
// EPI 1: y = (acc gate + gb) scale (pa = gate, pb = gb or NULL); EPI 2: out = scale g_y acc, out2 = scale g_y (pa = g_y).
template <int CT, int EPI>
__global__ __launch_bounds__(256) void up_fwd_kernel(const UpDims p, const float* __restrict__ px,
                                                     const float* __restrict__ pw, const float* __restrict__ pa,
                                                     const float* __restrict__ pb, float* __restrict__ pout,
                                                     float* __restrict__ pout2) {
  __shared__ float s_u[kFwdKC * kFwdPlane];
  __shared__ float s_w[9 * kFwdKC * 16 * CT];
  __shared__ int s_ra[kHR], s_rb[kHR], s_ca[kHC], s_cb[kHC];
  __shared__ float s_rf[kHR], s_cf[kHC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, Ci = p.Ci, Co = p.Co;
  const int ntx = (W + kTW - 1) / kTW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int r0 = ty * kTH, c0 = tx * kTW, b = blockIdx.y, cog0 = blockIdx.z * (16 * CT);
  const size_t HWi = (size_t)p.Hi * p.Wi, HW = (size_t)H * W;
  const float* xb = px + (size_t)b * Ci * HWi;
  up_fill_axis(s_ra, s_rb, s_rf, kHR, r0 - 1, p.Hi, H, p.Wi, tid);
  up_fill_axis(s_ca, s_cb, s_cf, kHC, c0 - 1, p.Wi, W, 1, tid);
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
  for (int ci0 = 0; ci0 < Ci; ci0 += kFwdKC) {
    __syncthreads();  // the tables are written / the previous stage has been consumed
    up_stage_u<kFwdKC, kHR, kHC, kFwdPlane, (CT > 1 ? 8 : 1)>(s_u, s_ra, s_rb, s_rf, s_ca, s_cb, s_cf, xb, ci0, Ci, HWi, tid);
    for (int idx = tid; idx < 16 * CT * kFwdKC * 9; idx += 256) {  // w[co][ci0 .. ci0 + 8][tap]: 72 consecutive floats per co
      const int col = idx / (kFwdKC * 9), rem = idx - col * (kFwdKC * 9), kl = rem / 9, tap = rem - kl * 9;
      const int co = cog0 + col;
      s_w[(tap * kFwdKC + kl) * (16 * CT) + col] = co < Co ? pw[((size_t)co * Ci + ci0 + kl) * 9 + tap] : 0.f;
    }
    __syncthreads();
    up_conv_core<CT, 4, kFwdKC>(s_u, kFwdPlane, kHC, s_w, poff, acc, j, g);
  }
  // epilogue on the accumulators: D row = channel cog0 + 16 ct + 4 g + r4, column = pixel j of the pixel tile
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int r = r0 + prow[pt], c = c0 + pcol[pt];
    if (r >= H || c >= W) continue;
    const unsigned o = (unsigned)r * (unsigned)W + (unsigned)c;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int co = cog0 + 16 * ct + 4 * g + r4;
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
// grid (tiles of 4 x 16 texels of x, B, tiles of 16 input channels); KC = output channels per K stage (4 for Co <= 4)
template <int KC>
__global__ __launch_bounds__(256) void up_bwd_x_kernel(const UpDims p, const float* __restrict__ pw,
                                                       const float* __restrict__ paux, const float* __restrict__ pg,
                                                       float* __restrict__ pgx) {
  __shared__ float s_g[KC * kBxPlane];
  __shared__ float s_gu[16 * kUR * kUC];
  __shared__ float s_w[9 * KC * 16];
  __shared__ int s_ra[kUR], s_rb[kUR], s_ca[kUC], s_cb[kUC];
  __shared__ float s_rf[kUR], s_cf[kUC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, Hi = p.Hi, Wi = p.Wi, Ci = p.Ci, Co = p.Co;
  const int ntx = (Wi + kSW - 1) / kSW, ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int i0 = ty * kSH, j0 = tx * kSW, b = blockIdx.y, cig0 = blockIdx.z * 16;
  const int rlo = up_first_row(i0, Hi, H), clo = up_first_row(j0, Wi, W);
  const size_t HW = (size_t)H * W;
  // source indices (mul = 1) and fractions of the region's rows and columns; -1 = outside the image
  up_fill_axis(s_ra, s_rb, s_rf, kUR, rlo, Hi, H, 1, tid);
  up_fill_axis(s_ca, s_cb, s_cf, kUC, clo, Wi, W, 1, tid);
  int poff[kBxNPT], pq[kBxNPT];
#pragma unroll
  for (int pt = 0; pt < kBxNPT; ++pt) {
    const int q = (wave * kBxNPT + pt) * 16 + j;
    pq[pt] = q < kUR * kUC ? q : -1;
    const int qq = q < kUR * kUC ? q : 0, row = qq / kUC;
    poff[pt] = row * kGC + (qq - row * kUC);
  }
  f32x4 acc[kBxNPT][1];
#pragma unroll
  for (int pt = 0; pt < kBxNPT; ++pt) acc[pt][0] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* gb = pg + (size_t)b * Co * HW;
  const float* ab = paux + (size_t)b * Co * HW;
  for (int co0 = 0; co0 < Co; co0 += KC) {
    __syncthreads();
    // the haloed window of g_pre, origin (rlo - 1, clo - 1); an item = one window position x 4 channels; unconditional
    // clamped loads in an unrolled loop, as in up_stage_u
    constexpr int NG = (KC / 4) * kGR * kGC;
#pragma unroll
    for (int it = 0; it < (NG + 255) / 256; ++it) {
      const int idx = tid + 256 * it, idc = min(idx, NG - 1);
      const int grp = idc / (kGR * kGC), pos = idc - grp * (kGR * kGC), rr = pos / kGC, cc = pos - rr * kGC;
      const int r = rlo - 1 + rr, c = clo - 1 + cc;
      const bool in = r >= 0 && r < H && c >= 0 && c < W;
      const unsigned o = in ? (unsigned)r * (unsigned)W + (unsigned)c : 0u;
      float vg[4], va[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t oo = (size_t)min(co0 + grp * 4 + u, Co - 1) * HW + o;
        vg[u] = gb[oo];
        va[u] = ab[oo];
      }
      if (idx < NG) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int cl = grp * 4 + u;
          s_g[cl * kBxPlane + pos] = (in && co0 + cl < Co) ? up_gpre(p, vg[u], va[u]) : 0.f;
        }
      }
    }
    for (int idx = tid; idx < KC * 16 * 9; idx += 256) {  // A[ci][co][tap'] = w[co][ci][8 - tap'] (the mirrored taps)
      const int kl = idx / 144, rem = idx - kl * 144, cil = rem / 9, tw = rem - cil * 9;
      const int co = co0 + kl, ci = cig0 + cil;
      s_w[((8 - tw) * KC + kl) * 16 + cil] = (co < Co && ci < Ci) ? pw[((size_t)co * Ci + ci) * 9 + tw] : 0.f;
    }
    __syncthreads();
    up_conv_core<1, kBxNPT, KC>(s_g, kBxPlane, kGC, s_w, poff, acc, j, g);
  }
  // g_U of the region to LDS: D row = channel 4 g + r4, column = pixel
#pragma unroll
  for (int pt = 0; pt < kBxNPT; ++pt)
    if (pq[pt] >= 0) {
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) s_gu[(4 * g + r4) * (kUR * kUC) + pq[pt]] = acc[pt][0][r4];
    }
  __syncthreads();
  // the bilinear adjoint as a gather: thread -> texel tid & 63 of the tile, channels tid >> 6 + 4 u
  const int tl = tid & 63, ti = i0 + (tl >> 4), tj = j0 + (tl & 15);
  if (ti >= Hi || tj >= Wi) return;
  const int rs = up_first_row(ti, Hi, H) - rlo, cs = up_first_row(tj, Wi, W) - clo;  // first candidates, inside the region
  float wr[5], wc[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const int rr = rs + t, cc = cs + t;
    wr[t] = wc[t] = 0.f;
    if (rr < kUR && s_ra[rr] >= 0) wr[t] = (s_ra[rr] == ti ? 1.f - s_rf[rr] : 0.f) + (s_rb[rr] == ti ? s_rf[rr] : 0.f);
    if (cc < kUC && s_ca[cc] >= 0) wc[t] = (s_ca[cc] == tj ? 1.f - s_cf[cc] : 0.f) + (s_cb[cc] == tj ? s_cf[cc] : 0.f);
  }
  float* gxb = pgx + (size_t)b * Ci * Hi * Wi + (unsigned)ti * (unsigned)Wi + (unsigned)tj;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int cil = (tid >> 6) + 4 * u;
    if (cig0 + cil >= Ci) continue;
    const float* src = s_gu + cil * (kUR * kUC);
    float sum = 0.f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      float rowsum = 0.f;
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int rr = min(rs + a, kUR - 1), cc = min(cs + c, kUC - 1);  // (a clamped candidate has weight 0)
        rowsum += wc[c] * src[rr * kUC + cc];
      }
      sum += wr[a] * rowsum;
    }
    gxb[(size_t)(cig0 + cil) * Hi * Wi] = sum;
  }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------
// grid (K blocks, (co tile, ci tile) pairs).  A workgroup walks a run of consecutive 8 x 32 tiles; per tile the window of
// U [16 ci][10][34] and g_pre [16 co][256] are staged; wave -> 64 of the 256 pixels as 16 K slices of 4 consecutive pixels.
__global__ __launch_bounds__(256) void up_bwd_w_kernel(const UpDims p, const float* __restrict__ px,
                                                       const float* __restrict__ paux, const float* __restrict__ pg,
                                                       float* __restrict__ pscratch) {
  __shared__ float s_u[16 * kBwPlane];  // (also the reduction image [9][256] at the end)
  __shared__ float s_g[16 * kBwGRow];
  __shared__ int s_ra[kHR], s_rb[kHR], s_ca[kHC], s_cb[kHC];
  __shared__ float s_rf[kHR], s_cf[kHC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int H = p.H, W = p.W, Ci = p.Ci, Co = p.Co;
  const int nci = (Ci + 15) >> 4, cot = blockIdx.y / nci, cit = blockIdx.y - cot * nci, co0 = cot * 16, ci0 = cit * 16;
  const int ntx = (W + kTW - 1) / kTW, nty = (H + kTH - 1) / kTH, ntiles = p.B * nty * ntx;
  const size_t HWi = (size_t)p.Hi * p.Wi, HW = (size_t)H * W;
  f32x4 acc[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) acc[tap] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int per = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t0 = min((int)blockIdx.x * per, ntiles), t1 = min(t0 + per, ntiles);
  for (int tile = t0; tile < t1; ++tile) {
    const int b = tile / (nty * ntx), rem = tile - b * (nty * ntx), ty = rem / ntx, tx = rem - ty * ntx;
    const int r0 = ty * kTH, c0 = tx * kTW;
    __syncthreads();  // the previous tile's operands and tables have been consumed
    up_fill_axis(s_ra, s_rb, s_rf, kHR, r0 - 1, p.Hi, H, p.Wi, tid);
    up_fill_axis(s_ca, s_cb, s_cf, kHC, c0 - 1, p.Wi, W, 1, tid);
    const float* gb = pg + (size_t)b * Co * HW;
    const float* ab = paux + (size_t)b * Co * HW;
    {  // thread -> one pixel of the tile, all 16 channels; unconditional clamped loads, all in flight together
      const int r = r0 + (tid >> 5), c = c0 + (tid & 31);
      const bool in = r < H && c < W;
      const unsigned o = in ? (unsigned)r * (unsigned)W + (unsigned)c : 0u;
      float vg[16], va[16];
#pragma unroll
      for (int cl = 0; cl < 16; ++cl) {
        const size_t oo = (size_t)min(co0 + cl, Co - 1) * HW + o;
        vg[cl] = gb[oo];
        va[cl] = ab[oo];
      }
#pragma unroll
      for (int cl = 0; cl < 16; ++cl) s_g[cl * kBwGRow + tid] = (in && co0 + cl < Co) ? up_gpre(p, vg[cl], va[cl]) : 0.f;
    }
    __syncthreads();
    up_stage_u<16, kHR, kHC, kBwPlane, 8>(s_u, s_ra, s_rb, s_rf, s_ca, s_cb, s_cf, px + (size_t)b * Ci * HWi, ci0, Ci, HWi, tid);
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const int q0 = wave * 64 + s * 4;  // 4 consecutive pixels of one row: lane group g takes pixel q0 + g
      const float a = s_g[j * kBwGRow + q0 + g];
      const float* up = s_u + j * kBwPlane + (q0 >> 5) * kHC + (q0 & 31) + g;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, up[(tap / 3) * kHC + tap % 3], acc[tap], 0, 0, 0);
    }
  }
  // D[co = 4 g + r4][ci = j]; the four waves add up in LDS in wave order, the partial [9][16 co][16 ci] goes to scratch
  __syncthreads();
  float* s_red = s_u;
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          float* sp = &s_red[tap * 256 + (4 * g + r4) * 16 + j];
          *sp = (wv == 0 ? 0.f : *sp) + acc[tap][r4];
        }
    }
    __syncthreads();
  }
  float* dst = pscratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (9 * 256) + tid;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) dst[tap * 256] = s_red[tap * 256 + tid];
}

// ---- streaming gradients ---------------------------------------------------------------------------------------------
// mode 0: out[n] = sum_b g_pre[b,n] over the Co H W plane elements;  mode 1: out[n] = scale g[n] over all B Co H W
__global__ __launch_bounds__(256) void up_bwd_s_kernel(const UpDims p, size_t N, const float* __restrict__ paux,
                                                       const float* __restrict__ pg, float* __restrict__ pout) {
  const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  if (p.mode == 0) {
    float s = 0.f;
    for (int b = 0; b < p.B; ++b) s += pg[(size_t)b * N + n] * (paux[(size_t)b * N + n] > 0.f ? 1.f : p.leak);
    pout[n] = s;
  } else {
    pout[n] = p.scale * pg[n];
  }
}

int check_common(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak) {
  GOL_REQUIRE(B >= 0 && Ci > 0 && Co > 0 && Hi > 0 && Wi > 0, "bad sizes");
  GOL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (bias + LeakyReLU) or 1 (gate)");
  GOL_REQUIRE(mode != 0 || leak > 0.f, "leak must be positive (the backward reads the activation mask from the sign of y)");
  if (Ci % 8 != 0 || !(Co % 16 == 0 || Co <= 4)) {
    gol_set_error("gol_upconv: Ci must be a multiple of 8, Co a multiple of 16 or 1..4 (got %d -> %d)", Ci, Co);
    return GOL_ERR_UNSUPPORTED;
  }
  // 32-bit offsets inside a plane; grid limits
  GOL_REQUIRE((long long)Hi * Wi <= (1ll << 26), "plane too large");
  GOL_REQUIRE(B <= 65535 && gol_cdiv(Co, 16) * gol_cdiv(Ci, 16) <= 65535, "too many views or channel tiles");
  GOL_REQUIRE((long long)B * gol_cdiv(2 * Hi, kTH) * gol_cdiv(2 * Wi, kTW) < (1ll << 31), "too many tiles");
  GOL_REQUIRE((long long)B * Co * Hi * Wi * 4 / 256 < (1ll << 31), "layer too large");
  return GOL_OK;
}

int bwd_w_groups(int Ci, int Co) { return gol_cdiv(Co, 16) * gol_cdiv(Ci, 16); }

int bwd_w_blocks(int B, int Ci, int Co, int Hi, int Wi) {
  return up_bwd_w_blocks((long long)B * gol_cdiv(2 * Hi, kTH) * gol_cdiv(2 * Wi, kTW), bwd_w_groups(Ci, Co));
}

template <int EPI>
void launch_fwd(const UpDims& p, const float* x, const float* w, const float* a, const float* b, float* out, float* out2,
                hipStream_t s) {
  const int tiles = gol_cdiv(p.H, kTH) * gol_cdiv(p.W, kTW);
  if (p.Co <= 16) up_fwd_kernel<1, EPI><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, x, w, a, b, out, out2);
  else if (p.Co <= 32) up_fwd_kernel<2, EPI><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, x, w, a, b, out, out2);
  else up_fwd_kernel<4, EPI><<<dim3(tiles, p.B, gol_cdiv(p.Co, 64)), 256, 0, s>>>(p, x, w, a, b, out, out2);
}

}  // namespace

extern "C" int gol_upconv_fwd(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale, const float* x,
                              const float* w_eff, const float* bias, const float* gate, const float* gb, float* y,
                              void* stream) {
  const int rc = check_common(B, Ci, Co, Hi, Wi, mode, leak);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && w_eff && y, "null pointer");
  GOL_REQUIRE(mode == 0 ? bias != nullptr : gate != nullptr, "mode 0 needs bias, mode 1 needs gate");
  const UpDims p{B, Ci, Co, Hi, Wi, 2 * Hi, 2 * Wi, mode, leak, scale};
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0) launch_fwd<0>(p, x, w_eff, bias, nullptr, y, nullptr, s);
  else launch_fwd<1>(p, x, w_eff, gate, gb, y, nullptr, s);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" long long gol_upconv_bwd_scratch_floats(int B, int Ci, int Co, int Hi, int Wi) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || Hi <= 0 || Wi <= 0) return 0;
  return (long long)bwd_w_groups(Ci, Co) * bwd_w_blocks(B, Ci, Co, Hi, Wi) * 9 * 256;
}

extern "C" int gol_upconv_bwd(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale, const float* x,
                              const float* w_eff, const float* y, const float* gate, const float* g_y, float* g_x,
                              float* g_w, float* g_bias, float* g_gate, float* g_gb, float* scratch, void* stream) {
  const int rc = check_common(B, Ci, Co, Hi, Wi, mode, leak);
  if (rc != GOL_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int H = 2 * Hi, W = 2 * Wi;
  if (B == 0) {  // empty sums
    if (g_w && hipMemsetAsync(g_w, 0, sizeof(float) * 9 * Ci * Co, s) != hipSuccess) return GOL_ERR_LAUNCH;
    if (g_bias && hipMemsetAsync(g_bias, 0, sizeof(float) * Co * H * W, s) != hipSuccess) return GOL_ERR_LAUNCH;
    return GOL_OK;
  }
  GOL_REQUIRE(g_y, "null pointer");
  GOL_REQUIRE(mode == 0 ? (!g_gate && !g_gb) : !g_bias, "g_bias belongs to mode 0, g_gate and g_gb to mode 1");
  const float* aux = mode == 0 ? y : gate;  // what g_pre is formed with
  GOL_REQUIRE(!(g_x || g_w || (mode == 0 && g_bias)) || aux, "mode 0 needs y, mode 1 needs gate");
  GOL_REQUIRE(!g_x || w_eff, "g_x needs w_eff");
  GOL_REQUIRE(!g_w || (x && scratch), "g_w needs x and scratch");
  GOL_REQUIRE(!g_gate || (x && w_eff), "g_gate needs x and w_eff (acc is recomputed)");
  const UpDims p{B, Ci, Co, Hi, Wi, H, W, mode, leak, scale};
  if (g_x) {
    const int tiles = gol_cdiv(Hi, kSH) * gol_cdiv(Wi, kSW);
    if (Co <= 4) up_bwd_x_kernel<4><<<dim3(tiles, B, gol_cdiv(Ci, 16)), 256, 0, s>>>(p, w_eff, aux, g_y, g_x);
    else up_bwd_x_kernel<8><<<dim3(tiles, B, gol_cdiv(Ci, 16)), 256, 0, s>>>(p, w_eff, aux, g_y, g_x);
    GOL_CHECK_LAUNCH();
  }
  if (g_w) {
    const int groups = bwd_w_groups(Ci, Co), nblk = bwd_w_blocks(B, Ci, Co, Hi, Wi);
    up_bwd_w_kernel<<<dim3(nblk, groups), 256, 0, s>>>(p, x, aux, g_y, scratch);
    GOL_CHECK_LAUNCH();
    up_bwd_w_reduce_kernel<<<dim3(9 * 16, groups), 256, 0, s>>>(Co, Ci, Ci, gol_cdiv(Ci, 16), gol_cdiv(Ci, 16), nblk, scratch, g_w);
    GOL_CHECK_LAUNCH();
  }
  if (g_bias) {
    const size_t N = (size_t)Co * H * W;
    up_bwd_s_kernel<<<dim3(gol_cdiv((long long)N, 256)), 256, 0, s>>>(p, N, y, g_y, g_bias);
    GOL_CHECK_LAUNCH();
  }
  if (g_gate) {  // acc recomputed by the forward kernel; g_gb rides along
    launch_fwd<2>(p, x, w_eff, g_y, nullptr, g_gate, g_gb, s);
    GOL_CHECK_LAUNCH();
  } else if (g_gb) {
    const size_t N = (size_t)B * Co * H * W;
    up_bwd_s_kernel<<<dim3(gol_cdiv((long long)N, 256)), 256, 0, s>>>(p, N, nullptr, g_y, g_gb);
    GOL_CHECK_LAUNCH();
  }
  return GOL_OK;
}
