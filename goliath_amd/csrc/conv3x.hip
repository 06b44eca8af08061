// conv3x.hip -- the wide layers of the frozen VGG19 feature network on a split-bf16 MFMA operator, gfx950.
//
// The same layer as vggconv.hip (3x3 / stride 1 / pad 1 convolution + bias + ReLU, optionally the 2x2 max-pool; forward and
// input gradient), but the product runs on v_mfma_f32_16x16x32_bf16 at "bf16x3" precision: every operand v is written as
//     hi = bf16_rne(v),  lo = bf16_rne(v - float(hi))                  (the subtraction is exact in fp32)
// and   acc = sum_{k,tap} (lo_x hi_w + hi_x lo_w + hi_x hi_w)          (exact products, fp32 sum; lo lo is dropped).
// That deviates from float64 by 4.5e-6 rel-L2, under the project's 1e-5 bar, at three MFMAs of the
// 16x rate for one.  Inputs are finite and of ordinary magnitude; a subnormal lo is not handled.  Zero padding splits to (0,0).
//
// Implicit GEMM, D[m = channel written][pixel] += A[m][k = channel read] B[k][pixel] per tap.  Operands of the MFMA: lane
// (j = lane & 15, g = lane >> 4) holds A[row j][k = 8 g .. 8 g + 7] and B[k = 8 g .. 8 g + 7][column j]; D[row 4 g + r][column j]
// -- the accumulator layout of vggconv.hip, so the epilogues are the same.  A workgroup (4 waves) owns 8 x 32 pixels x 16 CT
// channels (CT = 4, or 2 where there are only 32 channels); a wave two rows of the tile = 4 pixel tiles of 16.
//   K stage = 32 channels.  The haloed 10 x 34 window is split while it goes to LDS, PIXEL-major: s_in[hi|lo][position][32
//   channels] bf16, 64 bytes per position -- the same bytes as fp32.  A B operand is then one ds_read_b128.
//   The weights are split ONCE (gol_conv3x_pack) into packed[hi|lo][tap][Co / 8][Ci / 8][8 co][8 ci]: 8 x 8 blocks of 128
//   bytes.  The forward copies a block's rows (8 ci of one co) to LDS as they are; the backward needs 8 co of one ci and
//   transposes the block in registers on its way to LDS, with the taps mirrored.  ONE packing serves both directions.
//   A stage's weights are staged per tap ROW (3 taps x 16 CT x 32 x hi, lo = 24 KB at CT = 4), so that window + weights
//   stay at 68 KB and two workgroups share a CU: one computes while the other loads.  Re-streamed weight bytes per
//   workgroup and K stage: 74 KB for 9.4 MFLOP of the layer, i.e. 2 TB/s of L2 at 250 TF -- not the bound.
//   Both LDS images are read 16 bytes per lane with rows of 64 bytes: the 16-byte slot of row n is g ^ (2 if n & 4), which
//   makes every 16-lane group of a ds_read_b128 ({0-3,12-15,20-27}, ...) hit 16 distinct slots of the 256-byte bank row.
//   loaders   plain   x
//             g_y     backward without pool: g_pre = g_y where y > 0, else 0
//             g_p     backward with pool: g_pre[r,c] = g_p[r/2,c/2] where the position byte names (r,c) and p > 0, else 0
//   epilogues relu, pool (first maximum wins, one position byte per pooled element, floor pool), g_x: as in vggconv.hip
// No atomics, no scratch: every output element is written by exactly one lane from a fixed-order sum -- bitwise reproducible.
#include "gol_conv3x_core.h"  // CxDims, the tile constants, cx_stage_w and cx_core (shared with conv3ub.hip)

namespace {

enum { L_PLAIN = 0, L_GY = 2, L_GP = 3 };
enum { E_RELU = 0, E_POOL = 1, E_GX = 2 };

// 32 channels of the haloed window, origin (r0 - 1, c0 - 1), split into s_in[hi|lo][position][32]; outside the image: zeros.
// An item = one window position x 8 channels; the loads are unconditional (clamped to element 0, the value is dropped).
template <int LOAD>
__device__ __forceinline__ void cx_stage(unsigned short* s_in, const CxDims& p, const float* __restrict__ in_b,
                                         const float* __restrict__ aux_b, const unsigned char* __restrict__ pos_b, int k0,
                                         int r0, int c0, int tid) {
  constexpr int N = (kKS / 8) * kWin;
  const int H = p.H, W = p.W;
  const size_t PS = LOAD == L_GP ? (size_t)p.Hp * p.Wp : (size_t)H * W;
  for (int idx = tid; idx < N; idx += 256) {
    const int q = idx / kWin, pos = idx - q * kWin, rr = pos / kHC, cc = pos - rr * kHC;
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
    float va[8], vb[8];
    int vp[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {  // every load first, none behind a condition
      const size_t oo = (size_t)(k0 + q * 8 + u) * PS + o;
      va[u] = in_b[oo];
      vb[u] = 1.f;
      vp[u] = 0;
      if constexpr (LOAD == L_GY || LOAD == L_GP) vb[u] = aux_b[oo];
      if constexpr (LOAD == L_GP) vp[u] = pos_b[oo];
    }
    f32x8 v;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      bool live = in;
      if constexpr (LOAD == L_GY || LOAD == L_GP) live = live & (vb[u] > 0.f);
      if constexpr (LOAD == L_GP) live = live & (vp[u] == wpos);
      v[u] = live ? va[u] : 0.f;
    }
    bf16x8 hi, lo;
    cx_split(v, hi, lo);
    const int off = pos * kKS + cx_slot(pos, q) * 8;
    *reinterpret_cast<bf16x8*>(s_in + off) = hi;
    *reinterpret_cast<bf16x8*>(s_in + kWin * kKS + off) = lo;
  }
}

// the neighbouring lane's value (lane ^ 1): DPP quad_perm [1,0,3,2]; all lanes active
__device__ __forceinline__ float cx_lane_xor1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
}

// grid (tiles of 8 x 32 pixels, B, groups of 16 CT rows).  in: x (plain), g_y (g_y) or g_p (g_p); aux: y (g_y) or p (g_p);
// pos: the position bytes (g_p); out: y, p or g_x; outpos: the position bytes (pool)
template <int CT, int LOAD, int EPI, bool TRANS>
__global__ __launch_bounds__(256) void cx_kernel(const CxDims p, const float* __restrict__ pin, const float* __restrict__ paux,
                                                 const unsigned char* __restrict__ ppos,
                                                 const unsigned short* __restrict__ pw, const float* __restrict__ pbias,
                                                 float* __restrict__ pout, unsigned char* __restrict__ poutpos) {
  __shared__ __attribute__((aligned(16))) unsigned short s_in[2 * kWin * kKS];
  __shared__ __attribute__((aligned(16))) unsigned short s_w[2 * 3 * 16 * CT * kKS];
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
  for (int k0 = 0; k0 < K; k0 += kKS) {
    for (int ky = 0; ky < 3; ++ky) {
      __syncthreads();  // the previous tap row has been consumed
      if (ky == 0) cx_stage<LOAD>(s_in, p, in_b, aux_b, pos_b, k0, r0, c0, tid);
      cx_stage_w<CT, TRANS>(s_w, p, pw, k0, m0, ky, tid);
      __syncthreads();
      cx_core<CT>(s_in, s_w, poff, acc, ky, j, g);
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
          const float v1 = cx_lane_xor1(v0), v3 = cx_lane_xor1(v2);
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
          if constexpr (EPI == E_RELU) pout[off] = fmaxf(a + pbias[m], 0.f);
          else pout[off] = a;
        }
    }
  }
}

// weight[Co,Ci,3,3] -> packed[hi|lo][tap][Co / 8][Ci / 8][8 co][8 ci]; one thread per weight
__global__ __launch_bounds__(256) void cx_pack_kernel(int Co, int Ci, const float* __restrict__ w,
                                                      unsigned short* __restrict__ packed) {
  const long long n = (long long)Co * Ci * 9, idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int tap = (int)(idx % 9), ci = (int)((idx / 9) % Ci), co = (int)(idx / (9ll * Ci));
  const float v = w[idx];
  const __bf16 hi = (__bf16)v;
  const __bf16 lo = (__bf16)(v - (float)hi);
  const size_t o = ((((size_t)tap * (Co >> 3) + (co >> 3)) * (Ci >> 3) + (ci >> 3)) * 8 + (co & 7)) * 8 + (ci & 7);
  packed[o] = __builtin_bit_cast(unsigned short, hi);
  packed[(size_t)n + o] = __builtin_bit_cast(unsigned short, lo);
}

int cx_check(int B, int Ci, int Co, int H, int W, int pool) {
  GOL_REQUIRE(B >= 0 && Ci > 0 && Co > 0 && H > 0 && W > 0, "bad sizes");
  if (Ci % 32 != 0 || Co % 32 != 0 || B > 65535 || (pool && (H < 2 || W < 2))) {
    gol_set_error("gol_conv3x: Ci and Co must be multiples of 32, B <= 65535, H and W >= 2 with pool (got B %d, %d -> %d, "
                  "%d x %d, pool %d)", B, Ci, Co, H, W, pool);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE((long long)H * W <= (1ll << 30), "plane too large (32-bit offsets inside a plane)");
  GOL_REQUIRE(gol_cdiv(Co, 64) <= 65535 && gol_cdiv(Ci, 64) <= 65535, "too many channel tiles");
  return GOL_OK;
}

template <int LOAD, int EPI, bool TRANS>
void cx_launch(const CxDims& p, const float* in, const float* aux, const unsigned char* pos, const unsigned short* w,
               const float* bias, float* out, unsigned char* outpos, hipStream_t s) {
  const int tiles = gol_cdiv(p.H, kTH) * gol_cdiv(p.W, kTW);
  if (p.M <= 32) cx_kernel<2, LOAD, EPI, TRANS><<<dim3(tiles, p.B, 1), 256, 0, s>>>(p, in, aux, pos, w, bias, out, outpos);
  else cx_kernel<4, LOAD, EPI, TRANS><<<dim3(tiles, p.B, gol_cdiv(p.M, 64)), 256, 0, s>>>(p, in, aux, pos, w, bias, out, outpos);
}

}  // namespace

extern "C" long long gol_conv3x_packed_elems(int Co, int Ci) {
  if (Co <= 0 || Ci <= 0 || Co % 32 != 0 || Ci % 32 != 0) return 0;
  return 2ll * 9 * Co * Ci;
}

extern "C" int gol_conv3x_pack(int Co, int Ci, const float* weight, unsigned short* packed, void* stream) {
  GOL_REQUIRE(Co > 0 && Ci > 0, "bad sizes");
  if (Co % 32 != 0 || Ci % 32 != 0) {
    gol_set_error("gol_conv3x_pack: Ci and Co must be multiples of 32 (got %d -> %d)", Ci, Co);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(weight && packed, "null pointer");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  cx_pack_kernel<<<gol_cdiv(9ll * Co * Ci, 256), 256, 0, (hipStream_t)stream>>>(Co, Ci, weight, packed);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_conv3x_fwd(int B, int Ci, int Co, int H, int W, int pool, const float* x, const unsigned short* packed,
                              const float* bias, float* y, unsigned char* pos, void* stream) {
  const int rc = cx_check(B, Ci, Co, H, W, pool);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && packed && bias && y, "null pointer");
  GOL_REQUIRE(!pool || pos, "pool needs the position bytes");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const CxDims p{B, Co, Ci, H, W, H / 2, W / 2};
  hipStream_t s = (hipStream_t)stream;
  if (pool) cx_launch<L_PLAIN, E_POOL, false>(p, x, nullptr, nullptr, packed, bias, y, pos, s);
  else cx_launch<L_PLAIN, E_RELU, false>(p, x, nullptr, nullptr, packed, bias, y, nullptr, s);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_conv3x_bwd_x(int B, int Ci, int Co, int H, int W, int pool, const unsigned short* packed, const float* y,
                                const unsigned char* pos, const float* g_y, float* g_x, void* stream) {
  const int rc = cx_check(B, Ci, Co, H, W, pool);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(packed && y && g_y && g_x, "null pointer");
  GOL_REQUIRE(!pool || pos, "pool needs the position bytes");
  GOL_REQUIRE(gol_aligned16(packed), "packed must be 16-byte aligned");
  const CxDims p{B, Ci, Co, H, W, H / 2, W / 2};
  hipStream_t s = (hipStream_t)stream;
  if (pool) cx_launch<L_GP, E_GX, true>(p, g_y, y, pos, packed, nullptr, g_x, nullptr, s);
  else cx_launch<L_GY, E_GX, true>(p, g_y, y, nullptr, packed, nullptr, g_x, nullptr, s);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
