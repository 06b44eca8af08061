// imgfam.hip -- the image-sized work around the L2 / focus image losses (gol_imgloss_*, gol_depth_disc_mask, gol_mask_erode,
// include/goliath_hip.h): a masked elementwise image penalty with a deterministic reduction forward and its elementwise
// gradient backward, the depth-discontinuity mask, and the binary erosion of a mask.
//
// The penalty is a streaming pass like regloss.hip: one 256-thread workgroup per chunk of kChunk = 4096 floats of one (b,c)
// plane, a lane issues all of its 16-byte loads before the first use and a full aligned chunk has no predicated access.  The
// last (partial) chunk of a plane and a plane whose base is not 16-byte aligned take a scalar path that keeps each lane's
// elements and their order, so both paths give the same bits.  Sums are double in a fixed order (lane, gol_block_sum, then
// one workgroup over the chunk sums): no atomics, the same bits every run.  The per-element arithmetic is float32 in torch's
// operation order, without contraction, with IEEE division and the accurate expf.
//
// The two mask operators stage a tile plus its halo in LDS with coalesced loads and evaluate the window there: 4 B read and
// 1 B written per pixel (depth -> mask), 4 (or 1) B read and 4 B written (erosion).
#include "gol_stream.h"

#pragma clang fp contract(off)

namespace {

using namespace gol_stream;   // f4 / gfloat / gf4 / global_in / global_out, kBlock, kChunk, kVecIters, chunk_elems

typedef __attribute__((address_space(1))) const uint8_t gbyte;
typedef __attribute__((address_space(1))) const uint32_t gword;

enum { kAbs = GOL_IMGLOSS_ABS, kSq = GOL_IMGLOSS_SQ, kExpW = GOL_IMGLOSS_EXPW };

// ---- the penalties on the residual x = (pred - target) * m: f and g_scale * df/dpred --------------------------------------
template <int KIND>
__device__ __forceinline__ float pen_f(float x) {
  if (KIND == kAbs) {
    return fabsf(x);
  } else if (KIND == kSq) {
    return x * x;
  } else {                       // abs_error * exp(abs_error / 255.)
    const float a = fabsf(x);
    return a * expf(a / 255.f);
  }
}

template <int KIND>
__device__ __forceinline__ float pen_df(float x, float m, float gs) {
  if (KIND == kAbs) {            // abs: g * sgn(x); mul: * m
    return (x > 0.f ? gs : (x < 0.f ? -gs : 0.f)) * m;
  } else if (KIND == kSq) {      // pow(2): g * (2 * x); mul: * m
    return (gs * (2.f * x)) * m;
  } else {                       // the weight is detached: mul: g * w; abs: * sgn(x); mul: * m
    const float gw = gs * expf(fabsf(x) / 255.f);
    return (x > 0.f ? gw : (x < 0.f ? -gw : 0.f)) * m;
  }
}

__device__ __forceinline__ float veto_factor(uint32_t byte) { return byte ? 0.f : 1.f; }   // 1 - veto

// grid (chunks of a plane, B * C).  mask_ may be null (factor 1), veto_ may be null (factor 1).
template <int KIND, bool BWD>
__global__ __launch_bounds__(kBlock) void imgloss_kernel(int C, int HW, int mask_c, const float* __restrict__ pred_,
                                                          const float* __restrict__ target_, const float* __restrict__ mask_,
                                                          const uint8_t* __restrict__ veto_, double* __restrict__ partial,
                                                          const float* __restrict__ g_scale, float* __restrict__ g_pred_) {
  __shared__ double sh[kBlock / GOL_WAVE];
  const int plane = blockIdx.y;   // b * C + c
  const int b = plane / C;
  const int off = (int)blockIdx.x * kChunk;
  const int cn = chunk_elems((int64_t)HW - off);
  const size_t base = (size_t)plane * HW + off;
  const gfloat* pred = global_in(pred_) + base;
  const gfloat* target = global_in(target_) + base;
  const gfloat* mask = mask_ ? global_in(mask_) + ((size_t)(mask_c == 1 ? b : plane) * HW + off) : nullptr;
  gbyte* veto = veto_ ? reinterpret_cast<gbyte*>(reinterpret_cast<uintptr_t>(veto_)) + ((size_t)b * HW + off) : nullptr;
  gfloat* g = BWD ? global_out(g_pred_) + base : nullptr;
  const float gs = BWD ? g_scale[0] : 0.f;
  const uintptr_t align = reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target) |
                          reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(g);
  double acc = 0.0;
  if (cn == kChunk && (align & 15) == 0) {
    f4 pv[kVecIters], tv[kVecIters], mv[kVecIters];
    uint32_t vw[kVecIters];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) pv[k] = reinterpret_cast<const gf4*>(pred)[threadIdx.x + k * kBlock];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) tv[k] = reinterpret_cast<const gf4*>(target)[threadIdx.x + k * kBlock];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
      if (mask) mv[k] = reinterpret_cast<const gf4*>(mask)[threadIdx.x + k * kBlock];
      else mv[k] = f4{1.f, 1.f, 1.f, 1.f};
    }
    if (veto && (reinterpret_cast<uintptr_t>(veto) & 3) == 0) {   // the bytes of a lane's four floats: one 4-byte load
#pragma unroll
      for (int k = 0; k < kVecIters; ++k) vw[k] = reinterpret_cast<gword*>(veto)[threadIdx.x + k * kBlock];
    } else if (veto) {
#pragma unroll
      for (int k = 0; k < kVecIters; ++k) {
        gbyte* q = veto + 4 * (threadIdx.x + k * kBlock);
        vw[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kVecIters; ++k) vw[k] = 0u;
    }
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m = mv[k][e] * veto_factor((vw[k] >> (8 * e)) & 0xffu);
        const float x = (pv[k][e] - tv[k][e]) * m;
        if (BWD) o[e] = pen_df<KIND>(x, m, gs);
        else acc += (double)pen_f<KIND>(x);
      }
      if (BWD) reinterpret_cast<gf4*>(g)[threadIdx.x + k * kBlock] = o;
    }
  } else {   // a lane keeps the elements and the order of the 16-byte path: the same bits from either path
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * (threadIdx.x + k * kBlock) + e;
        if (i < cn) {
          const float m = (mask ? mask[i] : 1.f) * (veto ? veto_factor(veto[i]) : 1.f);
          const float x = (pred[i] - target[i]) * m;
          if (BWD) g[i] = pen_df<KIND>(x, m, gs);
          else acc += (double)pen_f<KIND>(x);
        }
      }
    }
  }
  if (!BWD) {
    acc = gol_block_sum<double, kBlock / GOL_WAVE>(acc, sh);
    if (threadIdx.x == 0) partial[(size_t)plane * gridDim.x + blockIdx.x] = acc;
  }
}

// one workgroup: the chunk sums in a fixed order in double -> loss[0] = (float)(sum / n), sum[0] = the double sum
__global__ __launch_bounds__(kBlock) void imgloss_finalize_kernel(int64_t n_chunks, int64_t n, const double* __restrict__ partial,
                                                                   float* __restrict__ loss, double* __restrict__ sum) {
  __shared__ double sh[kBlock / GOL_WAVE];
  double acc = 0.0;
  for (int64_t c = threadIdx.x; c < n_chunks; c += kBlock) acc += partial[c];
  acc = gol_block_sum<double, kBlock / GOL_WAVE>(acc, sh);
  if (threadIdx.x == 0) {
    loss[0] = (float)(acc / (double)n);
    sum[0] = acc;
  }
}

// ---- the tiled mask operators ---------------------------------------------------------------------------------------------
constexpr int kTileW = 64, kTileH = 16;   // output pixels of a workgroup: one wave per row of 64, four rows per lane

// depth [B,H,W] -> out [B,H,W] bytes: out = any in-image centre of the POOL x POOL window has |sobel| > threshold.
// grid (cdiv(W, kTileW), cdiv(H, kTileH), B)
template <int POOL>
__global__ __launch_bounds__(kBlock) void depth_disc_kernel(int H, int W, float threshold, const float* __restrict__ depth_,
                                                             uint8_t* __restrict__ out) {
  constexpr int R = POOL / 2, HALO = 1 + R;
  constexpr int DW = kTileW + 2 * HALO, DH = kTileH + 2 * HALO;   // the depth tile: Sobel of the fire flags' halo
  constexpr int FW = kTileW + 2 * R, FH = kTileH + 2 * R;         // the fire flags: the window of the output tile
  __shared__ float sd[DH * DW];
  __shared__ uint8_t sf[FH * FW];
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const gfloat* depth = global_in(depth_) + plane;
  for (int i = threadIdx.x; i < DH * DW; i += kBlock) {           // zero padding of the convolution
    const int y = y0 - HALO + i / DW, x = x0 - HALO + i % DW;
    sd[i] = (y >= 0 && y < H && x >= 0 && x < W) ? depth[(size_t)y * W + x] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < FH * FW; i += kBlock) {
    const int r = i / FW, c = i % FW;
    const int y = y0 - R + r, x = x0 - R + c;
    uint8_t fire = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {                     // a centre outside the image is the pool's zero padding
      const float* p = sd + r * DW + c;                           // the window's top-left: centre (r + 1, c + 1)
      const float a00 = p[0], a01 = p[1], a02 = p[2], a10 = p[DW], a12 = p[DW + 2], a20 = p[2 * DW], a21 = p[2 * DW + 1],
                  a22 = p[2 * DW + 2];
      const float gx = (a02 - a00) + 2.f * (a12 - a10) + (a22 - a20);
      const float gy = (a20 - a00) + 2.f * (a21 - a01) + (a22 - a02);
      fire = __fsqrt_rn(gx * gx + gy * gy) > threshold;
    }
    sf[i] = fire;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTileH * kTileW; i += kBlock) {
    const int r = i / kTileW, c = i % kTileW;
    const int y = y0 + r, x = x0 + c;
    if (y < H && x < W) {
      uint32_t any = 0;
#pragma unroll
      for (int dy = 0; dy < POOL; ++dy) {
#pragma unroll
        for (int dx = 0; dx < POOL; ++dx) any |= sf[(r + dy) * FW + c + dx];
      }
      out[plane + (size_t)y * W + x] = (uint8_t)any;
    }
  }
}

// x [B,H,W] (float32, or bytes with U8) -> out float32: 1 iff no in-image pixel of the ks x ks window has 1 - x > 0 (U8: is 0).
// The window OR is separable: rows of the tile plus its vertical halo first, then columns.
constexpr int kMaxR = 15;   // ks <= 31
template <bool U8>
__global__ __launch_bounds__(kBlock) void erode_kernel(int H, int W, int R, const void* __restrict__ x_, float* __restrict__ out_) {
  __shared__ uint8_t sv[(kTileH + 2 * kMaxR) * (kTileW + 2 * kMaxR)];
  __shared__ uint8_t sr[(kTileH + 2 * kMaxR) * kTileW];
  const int VW = kTileW + 2 * R, VH = kTileH + 2 * R;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const gfloat* xf = global_in(static_cast<const float*>(x_)) + plane;
  gbyte* xb = reinterpret_cast<gbyte*>(reinterpret_cast<uintptr_t>(x_)) + plane;
  for (int i = threadIdx.x; i < VH * VW; i += kBlock) {           // the complement, zero padded
    const int y = y0 - R + i / VW, x = x0 - R + i % VW;
    uint8_t v = 0;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t at = (size_t)y * W + x;
      v = U8 ? (xb[at] == 0) : (1.f - xf[at] > 0.f);
    }
    sv[i] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < VH * kTileW; i += kBlock) {
    const int r = i / kTileW, c = i % kTileW;
    uint32_t any = 0;
    for (int dx = 0; dx <= 2 * R; ++dx) any |= sv[r * VW + c + dx];
    sr[i] = (uint8_t)any;
  }
  __syncthreads();
  gfloat* out = global_out(out_) + plane;
  for (int i = threadIdx.x; i < kTileH * kTileW; i += kBlock) {
    const int r = i / kTileW, c = i % kTileW;
    const int y = y0 + r, x = x0 + c;
    if (y < H && x < W) {
      uint32_t any = 0;
      for (int dy = 0; dy <= 2 * R; ++dy) any |= sr[(r + dy) * kTileW + c];
      out[(size_t)y * W + x] = any ? 0.f : 1.f;
    }
  }
}

bool known_kind(int kind) { return kind >= kAbs && kind <= kExpW; }

template <bool BWD>
int launch_imgloss(const char* who, int kind, int B, int C, int HW, int mask_c, const float* pred, const float* target,
                   const float* mask, const uint8_t* veto, double* partial, const float* g_scale, float* g_pred,
                   void* stream) {
  if (!known_kind(kind)) {
    gol_set_error("%s: unknown penalty kind %d (GOL_IMGLOSS_ABS .. GOL_IMGLOSS_EXPW)", who, kind);
    return GOL_ERR_INVALID_ARG;
  }
  if (B < 0 || C <= 0 || HW < 0) {
    gol_set_error("%s: bad sizes", who);
    return GOL_ERR_INVALID_ARG;
  }
  if (B == 0 || HW == 0) return GOL_OK;
  if (!pred || !target || (BWD ? (!g_scale || !g_pred) : !partial)) {
    gol_set_error("%s: null pointer", who);
    return GOL_ERR_INVALID_ARG;
  }
  if (mask && mask_c != 1 && mask_c != C) {
    gol_set_error("%s: mask must have 1 or C channels", who);
    return GOL_ERR_INVALID_ARG;
  }
  if ((long long)B * C > 65535) {
    gol_set_error("%s: B*C > 65535", who);
    return GOL_ERR_INVALID_ARG;
  }
  const dim3 grid((unsigned)gol_cdiv(HW, kChunk), (unsigned)(B * C)), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case kAbs:
      hipLaunchKernelGGL((imgloss_kernel<kAbs, BWD>), grid, block, 0, s, C, HW, mask_c, pred, target, mask, veto, partial,
                         g_scale, g_pred);
      break;
    case kSq:
      hipLaunchKernelGGL((imgloss_kernel<kSq, BWD>), grid, block, 0, s, C, HW, mask_c, pred, target, mask, veto, partial,
                         g_scale, g_pred);
      break;
    default:
      hipLaunchKernelGGL((imgloss_kernel<kExpW, BWD>), grid, block, 0, s, C, HW, mask_c, pred, target, mask, veto, partial,
                         g_scale, g_pred);
      break;
  }
  return GOL_OK;
}

}  // namespace

extern "C" int gol_imgloss_chunk_elems(void) { return kChunk; }

extern "C" int gol_imgloss_fwd(int kind, int B, int C, int HW, int mask_c, const float* pred, const float* target,
                               const float* mask, const uint8_t* veto, double* partial, void* stream) {
  const int rc = launch_imgloss<false>(__func__, kind, B, C, HW, mask_c, pred, target, mask, veto, partial, nullptr, nullptr,
                                       stream);
  if (rc != GOL_OK) return rc;
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_imgloss_bwd(int kind, int B, int C, int HW, int mask_c, const float* pred, const float* target,
                               const float* mask, const uint8_t* veto, const float* g_scale, float* g_pred, void* stream) {
  const int rc = launch_imgloss<true>(__func__, kind, B, C, HW, mask_c, pred, target, mask, veto, nullptr, g_scale, g_pred,
                                      stream);
  if (rc != GOL_OK) return rc;
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_imgloss_finalize(int64_t n_chunks, int64_t n, const double* partial, float* loss, double* sum,
                                    void* stream) {
  GOL_REQUIRE(n_chunks >= 0 && n >= 0, "negative count");
  if (n_chunks == 0 || n == 0) return GOL_OK;
  GOL_REQUIRE(partial && loss && sum, "null pointer");
  hipLaunchKernelGGL(imgloss_finalize_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, n_chunks, n, partial, loss, sum);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_depth_disc_mask(int B, int H, int W, int pool, float threshold, const float* depth, uint8_t* out,
                                   void* stream) {
  if (pool != 1 && pool != 3 && pool != 5) {
    gol_set_error("%s: pool size %d is not supported (1, 3 or 5)", __func__, pool);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(B >= 0 && H >= 0 && W >= 0, "bad sizes");
  if (B == 0 || H == 0 || W == 0) return GOL_OK;
  GOL_REQUIRE(depth && out, "null pointer");
  GOL_REQUIRE(B <= 65535 && gol_cdiv(H, kTileH) <= 65535, "B or H / 16 > 65535");
  const dim3 grid((unsigned)gol_cdiv(W, kTileW), (unsigned)gol_cdiv(H, kTileH), (unsigned)B), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  switch (pool) {
    case 1: hipLaunchKernelGGL(depth_disc_kernel<1>, grid, block, 0, s, H, W, threshold, depth, out); break;
    case 3: hipLaunchKernelGGL(depth_disc_kernel<3>, grid, block, 0, s, H, W, threshold, depth, out); break;
    default: hipLaunchKernelGGL(depth_disc_kernel<5>, grid, block, 0, s, H, W, threshold, depth, out); break;
  }
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_mask_erode(int B, int H, int W, int ks, int x_is_u8, const void* x, float* out, void* stream) {
  if (ks < 1 || ks > 2 * kMaxR + 1 || ks % 2 == 0) {
    gol_set_error("%s: window size %d is not supported (odd, 1 .. %d)", __func__, ks, 2 * kMaxR + 1);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(B >= 0 && H >= 0 && W >= 0, "bad sizes");
  if (B == 0 || H == 0 || W == 0) return GOL_OK;
  GOL_REQUIRE(x && out, "null pointer");
  GOL_REQUIRE(B <= 65535 && gol_cdiv(H, kTileH) <= 65535, "B or H / 16 > 65535");
  const dim3 grid((unsigned)gol_cdiv(W, kTileW), (unsigned)gol_cdiv(H, kTileH), (unsigned)B), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  if (x_is_u8) hipLaunchKernelGGL(erode_kernel<true>, grid, block, 0, s, H, W, ks / 2, x, out);
  else hipLaunchKernelGGL(erode_kernel<false>, grid, block, 0, s, H, W, ks / 2, x, out);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
