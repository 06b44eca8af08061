// regloss.hip -- the per-Gaussian regularisers of the training loss as streaming passes (gol_regloss_*, gol_backlit_*,
// include/goliath_hip.h): an elementwise penalty with a deterministic reduction forward, its elementwise gradient backward.
//
// One 256-thread workgroup per chunk of kChunk = 4096 floats = 4 float4 per lane; a lane issues all of its 16-byte loads
// before the first use and a full chunk has no predicated access.  The last (partial) chunk and a base pointer that is not
// 16-byte aligned take a scalar path that keeps each lane's elements and their order, so both paths give the same bits.
// One workgroup per chunk, no grid-stride loop and no block cap (25 M elements are 6144 workgroups).  Every sum has a fixed
// order (lane, then gol_block_sum of gol_stream.h: DPP ladder over the wave, LDS over the four waves) and is kept in double:
// no float atomics, the same bits every run.  The per-element arithmetic is float32 in torch's operation order, without
// contraction, with IEEE division and the accurate logf.
#include "gol_stream.h"

#pragma clang fp contract(off)

namespace {

using namespace gol_stream;   // f4 / gfloat / gf4 / global_in / global_out, kBlock, kChunk, kVecIters, chunk_elems

constexpr int kRows = kChunk / 4;                // backlit: rows of a chunk (C = 3: 3072 colours + 1024 weights)

enum { kBound = GOL_REGLOSS_BOUND, kNegSq = GOL_REGLOSS_NEG_SQ, kSq = GOL_REGLOSS_SQ, kAbs = GOL_REGLOSS_ABS,
       kAlphaPrior = GOL_REGLOSS_ALPHAPRIOR };

// ---- the unary penalties: f and g_scale * f', float32 in torch's operation order -----------------------------------------
template <int KIND>
__device__ __forceinline__ float pen_f(float x, float p0, float p1) {
  if (KIND == kBound) {          // where(x < min, 1 / clamp(x, 1e-7, inf), where(x > max, (x - max) ** 2, 0))
    const float d = x - p1;
    return x < p0 ? 1.f / fmaxf(x, 1e-7f) : (x > p1 ? d * d : 0.f);
  } else if (KIND == kNegSq) {   // clamp(max=0).pow(2)
    const float m = fminf(x, 0.f);
    return m * m;
  } else if (KIND == kSq) {
    return x * x;
  } else if (KIND == kAbs) {
    return fabsf(x);
  } else {                       // log(0.1 + x) + log(0.1 + 1.0 - x) - -2.20727
    return (logf(0.1f + x) + logf(1.1f - x)) + 2.20727f;
  }
}

template <int KIND>
__device__ __forceinline__ float pen_df(float x, float p0, float p1, float gs) {
  if (KIND == kBound) {          // reciprocal: -g * r * r behind clamp's mask (x >= 1e-7); pow(2): g * (2 * d)
    const float r = 1.f / fmaxf(x, 1e-7f);
    return x < p0 ? (x >= 1e-7f ? (-gs) * (r * r) : 0.f) : (x > p1 ? gs * (2.f * (x - p1)) : 0.f);
  } else if (KIND == kNegSq) {
    return gs * (2.f * fminf(x, 0.f));
  } else if (KIND == kSq) {
    return gs * (2.f * x);
  } else if (KIND == kAbs) {
    return x > 0.f ? gs : (x < 0.f ? -gs : 0.f);
  } else {                       // log: g / self, for both terms
    return gs / (0.1f + x) - gs / (1.1f - x);
  }
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void regloss_fwd_kernel(int64_t n, float p0, float p1, const float* __restrict__ x_,
                                                              double* __restrict__ partial) {
  __shared__ double sh[kBlock / GOL_WAVE];
  const int64_t off = (int64_t)blockIdx.x * kChunk;
  const int cn = chunk_elems(n - off);
  const gfloat* x = global_in(x_) + off;
  double acc = 0.0;
  if (cn == kChunk && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    f4 v[kVecIters];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) v[k] = reinterpret_cast<const gf4*>(x)[threadIdx.x + k * kBlock];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += (double)pen_f<KIND>(v[k][e], p0, p1);
    }
  } else {   // a lane keeps the elements and the order of the 16-byte path: the same bits from either path
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * (threadIdx.x + k * kBlock) + e;
        if (i < cn) acc += (double)pen_f<KIND>(x[i], p0, p1);
      }
    }
  }
  acc = gol_block_sum<double, kBlock / GOL_WAVE>(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void regloss_bwd_kernel(int64_t n, float p0, float p1, const float* __restrict__ x_,
                                                              const float* __restrict__ g_scale, float* __restrict__ g_x_) {
  const int64_t off = (int64_t)blockIdx.x * kChunk;
  const int cn = chunk_elems(n - off);
  const gfloat* x = global_in(x_) + off;
  gfloat* g = global_out(g_x_) + off;
  const float gs = g_scale[0];
  if (cn == kChunk && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g)) & 15) == 0) {
    f4 v[kVecIters];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) v[k] = reinterpret_cast<const gf4*>(x)[threadIdx.x + k * kBlock];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
      f4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pen_df<KIND>(v[k][e], p0, p1, gs);
      reinterpret_cast<gf4*>(g)[threadIdx.x + k * kBlock] = o;
    }
  } else {
    for (int i = threadIdx.x; i < cn; i += kBlock) g[i] = pen_df<KIND>(x[i], p0, p1, gs);
  }
}

// ---- backlit: w = relu(-cosw)^2 per row, sum_c w * relu(color) and sum w (each row once) ----------------------------------
__device__ __forceinline__ float backlit_w(float cw) {
  const float t = fmaxf(-cw, 0.f);
  return t * t;
}

__device__ __forceinline__ int chunk_rows(int64_t m, int64_t row0) {
  const int64_t rem = m - row0;
  return rem >= kRows ? kRows : (int)rem;
}

__global__ __launch_bounds__(kBlock) void backlit_fwd_kernel(int64_t m, int c, const float* __restrict__ color_,
                                                              const float* __restrict__ cosw_, double* __restrict__ partial) {
  __shared__ double sh[kBlock / GOL_WAVE];
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int rows = chunk_rows(m, row0);
  const gfloat* col = global_in(color_) + row0 * c;
  const gfloat* cw = global_in(cosw_) + row0;
  double num = 0.0, den = 0.0;
  if (c == 3 && rows == kRows && ((reinterpret_cast<uintptr_t>(col) | reinterpret_cast<uintptr_t>(cw)) & 15) == 0) {
    // a lane owns rows 4 t .. 4 t + 3: colour floats [12 t, 12 t + 12) and weights [4 t, 4 t + 4)
    f4 v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = reinterpret_cast<const gf4*>(col)[3 * threadIdx.x + k];
    const f4 cv = reinterpret_cast<const gf4*>(cw)[threadIdx.x];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float w = backlit_w(cv[r]);
      den += (double)w;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int e = 3 * r + j;
        num += (double)(w * fmaxf(v[e >> 2][e & 3], 0.f));
      }
    }
  } else {   // any c: a lane keeps its four rows and their order, so c == 3 gives the same bits on either path
    for (int r = 4 * threadIdx.x; r < 4 * threadIdx.x + 4 && r < rows; ++r) {
      const float w = backlit_w(cw[r]);
      den += (double)w;
      const gfloat* row = col + (int64_t)r * c;
      for (int j = 0; j < c; ++j) num += (double)(w * fmaxf(row[j], 0.f));
    }
  }
  num = gol_block_sum<double, kBlock / GOL_WAVE>(num, sh);
  den = gol_block_sum<double, kBlock / GOL_WAVE>(den, sh);
  if (threadIdx.x == 0) {
    partial[2 * (size_t)blockIdx.x] = num;
    partial[2 * (size_t)blockIdx.x + 1] = den;
  }
}

__global__ __launch_bounds__(kBlock) void backlit_bwd_kernel(int64_t m, int c, const float* __restrict__ color_,
                                                              const float* __restrict__ cosw_,
                                                              const float* __restrict__ g_scale, float* __restrict__ g_color_) {
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int rows = chunk_rows(m, row0);
  const gfloat* col = global_in(color_) + row0 * c;
  const gfloat* cw = global_in(cosw_) + row0;
  gfloat* g = global_out(g_color_) + row0 * c;
  const float gs = g_scale[0];
  const uintptr_t align = reinterpret_cast<uintptr_t>(col) | reinterpret_cast<uintptr_t>(cw) | reinterpret_cast<uintptr_t>(g);
  if (c == 3 && rows == kRows && (align & 15) == 0) {
    f4 v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = reinterpret_cast<const gf4*>(col)[3 * threadIdx.x + k];
    const f4 cv = reinterpret_cast<const gf4*>(cw)[threadIdx.x];
    f4 o[3];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gw = gs * backlit_w(cv[r]);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int e = 3 * r + j;
        o[e >> 2][e & 3] = v[e >> 2][e & 3] > 0.f ? gw : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) reinterpret_cast<gf4*>(g)[3 * threadIdx.x + k] = o[k];
  } else {
    const int64_t ne = (int64_t)rows * c;
    for (int64_t e = threadIdx.x; e < ne; e += kBlock) {
      const int r = (int)(e / c);
      g[e] = col[e] > 0.f ? gs * backlit_w(cw[r]) : 0.f;
    }
  }
}

bool known_kind(int kind) { return kind >= kBound && kind <= kAlphaPrior; }

}  // namespace

extern "C" int gol_regloss_chunk_elems(void) { return kChunk; }

extern "C" int gol_regloss_fwd(int kind, int64_t n, float p0, float p1, const float* x, double* partial, void* stream) {
  if (!known_kind(kind)) {
    gol_set_error("%s: unknown penalty kind %d (GOL_REGLOSS_BOUND .. GOL_REGLOSS_ALPHAPRIOR)", __func__, kind);
    return GOL_ERR_INVALID_ARG;
  }
  GOL_REQUIRE(n >= 0, "negative count");
  if (n == 0) return GOL_OK;
  GOL_REQUIRE(x && partial, "null pointer");
  const int64_t chunks = (n + kChunk - 1) / kChunk;
  GOL_REQUIRE(chunks <= 0x7fffffffLL, "too many elements for one launch");
  const dim3 grid((unsigned)chunks), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case kBound: hipLaunchKernelGGL(regloss_fwd_kernel<kBound>, grid, block, 0, s, n, p0, p1, x, partial); break;
    case kNegSq: hipLaunchKernelGGL(regloss_fwd_kernel<kNegSq>, grid, block, 0, s, n, p0, p1, x, partial); break;
    case kSq: hipLaunchKernelGGL(regloss_fwd_kernel<kSq>, grid, block, 0, s, n, p0, p1, x, partial); break;
    case kAbs: hipLaunchKernelGGL(regloss_fwd_kernel<kAbs>, grid, block, 0, s, n, p0, p1, x, partial); break;
    default: hipLaunchKernelGGL(regloss_fwd_kernel<kAlphaPrior>, grid, block, 0, s, n, p0, p1, x, partial); break;
  }
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_regloss_bwd(int kind, int64_t n, float p0, float p1, const float* x, const float* g_scale, float* g_x,
                               void* stream) {
  if (!known_kind(kind)) {
    gol_set_error("%s: unknown penalty kind %d (GOL_REGLOSS_BOUND .. GOL_REGLOSS_ALPHAPRIOR)", __func__, kind);
    return GOL_ERR_INVALID_ARG;
  }
  GOL_REQUIRE(n >= 0, "negative count");
  if (n == 0) return GOL_OK;
  GOL_REQUIRE(x && g_scale && g_x, "null pointer");
  const int64_t chunks = (n + kChunk - 1) / kChunk;
  GOL_REQUIRE(chunks <= 0x7fffffffLL, "too many elements for one launch");
  const dim3 grid((unsigned)chunks), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case kBound: hipLaunchKernelGGL(regloss_bwd_kernel<kBound>, grid, block, 0, s, n, p0, p1, x, g_scale, g_x); break;
    case kNegSq: hipLaunchKernelGGL(regloss_bwd_kernel<kNegSq>, grid, block, 0, s, n, p0, p1, x, g_scale, g_x); break;
    case kSq: hipLaunchKernelGGL(regloss_bwd_kernel<kSq>, grid, block, 0, s, n, p0, p1, x, g_scale, g_x); break;
    case kAbs: hipLaunchKernelGGL(regloss_bwd_kernel<kAbs>, grid, block, 0, s, n, p0, p1, x, g_scale, g_x); break;
    default: hipLaunchKernelGGL(regloss_bwd_kernel<kAlphaPrior>, grid, block, 0, s, n, p0, p1, x, g_scale, g_x); break;
  }
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_backlit_fwd(int64_t m, int c, const float* color, const float* cosw, double* partial, void* stream) {
  GOL_REQUIRE(m >= 0 && c >= 1, "negative row count or no channel");
  if (m == 0) return GOL_OK;
  GOL_REQUIRE(color && cosw && partial, "null pointer");
  const int64_t chunks = (m + kRows - 1) / kRows;
  GOL_REQUIRE(chunks <= 0x7fffffffLL, "too many rows for one launch");
  hipLaunchKernelGGL(backlit_fwd_kernel, dim3((unsigned)chunks), dim3(kBlock), 0, (hipStream_t)stream, m, c, color, cosw,
                     partial);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_backlit_bwd(int64_t m, int c, const float* color, const float* cosw, const float* g_scale, float* g_color,
                               void* stream) {
  GOL_REQUIRE(m >= 0 && c >= 1, "negative row count or no channel");
  if (m == 0) return GOL_OK;
  GOL_REQUIRE(color && cosw && g_scale && g_color, "null pointer");
  const int64_t chunks = (m + kRows - 1) / kRows;
  GOL_REQUIRE(chunks <= 0x7fffffffLL, "too many rows for one launch");
  hipLaunchKernelGGL(backlit_bwd_kernel, dim3((unsigned)chunks), dim3(kBlock), 0, (hipStream_t)stream, m, c, color, cosw,
                     g_scale, g_color);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
