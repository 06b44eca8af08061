// mvpprims.hip -- what hand_mvp.AutoEncoder does between the decoder output and the ray march, gfx950.
//
//   gol_mvp_template_fwd / _bwd    decoder slabs rgb[B,TD,3,Sy,Sx] + alpha[B,TD,1,Sy,Sx] -> channels-last primitive template
//                                  out[B,Kout,TD,TH,TW,C]: ca_code/models/hand_mvp.py:171-185 (cat, view, permute, reshape)
//                                  with the valid_prims selection of ca_code/utils/render_raymarcher.py:41-47 folded in (a
//                                  slot table: no nonzero, no host sync) -- or, with a `live` table, the teacher's
//                                  valid_prims * primalpha masking (hand_teacher_mvp.py:311).  Optionally fused on the way:
//                                  relu(25 x + 100) of hand_mvp.py:472 and the relu of :434.
//   gol_mvp_primtransf_fwd / _bwd  hand_mvp.py:410-425 with axisangle_to_matrix (:477-510): one lane per primitive.
//
// Template kernels.  A lane owns one slab position (Y, X) of a batch element (four consecutive X in the one-channel case) and
// walks the TD depth planes, so the index arithmetic (two divisions by the primitive size, the slot lookup) is paid once
// per TD elements and the loads of UNROLL planes are in flight together.  Lanes run along X: a wave reads whole plane rows
// (runs of TW floats per primitive, back to back over the primitives of the row), and the TW lanes of one primitive row
// store TW x 16 bytes back to back -- one row of the channels-last primitive, TW * C floats.  Every input element has
// one reader and every output element one writer: no atomics, no LDS, bitwise repeatable.  The backward walks the same way
// (it is the transpose): 16-byte loads of g_out / g_out_full, coalesced plane stores, zeros where a primitive was dropped
// or dead -- g_rgb / g_alpha are written completely.  Inputs may be only 4-byte aligned (scalar loads); the template side
// is the wrapper's allocation and 16-byte aligned.  All offsets are 64-bit: B K TD TH TW 4 passes 2^31 at B = 16.
#include "gol_stream.h"

#include <math.h>

namespace {

using namespace gol_stream;

constexpr int THREADS = 256;
constexpr int UNROLL = 4;   // depth planes whose loads are issued before the first store

struct TplGeom {
  int TD, TH, TW, ny, nx;   // primitive size, primitives per slab column / row
  int Kout;                 // primitives of `out` (slots are 0 .. Kout-1)
  int act;                  // 1 = relu(scale x + shift) on rgb, relu(x) on alpha
  float scale, shift;
};

__device__ __forceinline__ float relu_keep_nan(float v) { return v <= 0.f ? 0.f : v; }
// scale x + shift as a rounded product and a rounded sum -- PyTorch's two elementwise kernels, bit for bit -- NOT one FMA:
// at the reference's relu(25 x + 100) the product cancels against the shift near the kink, where the single rounding of an
// FMA differs from the composition by up to ulp(100) / 2 = 64 ulp of a result near 0.5 (and could flip the relu mask)
// (HIP's __fmul_rn / __fadd_rn are plain operators, and under the build's -ffp-contract=fast the backend fuses whatever
// product meets a sum, whatever pragma the source carries: the empty asm makes the product opaque to it)
__device__ __forceinline__ float affine(const TplGeom& g, float x) {
  float prod = g.scale * x;
  asm volatile("" : "+v"(prod));
  return prod + g.shift;
}

// where lane `q` of batch element b stands: slab position p = Y * Sx + X (PX consecutive X), primitive k, position (y, x)
// inside it, the slot of k in `out` (-1: not written; a slot outside 0 .. Kout-1 is treated as -1) and its live flag
struct TplPos {
  int64_t p, plane;
  int k, y, x, s;
  bool live;
};

template <int PX>
__device__ __forceinline__ bool tpl_pos(const TplGeom& g, const int32_t* __restrict__ slot, const int32_t* __restrict__ live,
                                        TplPos& o) {
  const unsigned Sx = (unsigned)g.nx * g.TW, Sy = (unsigned)g.ny * g.TH;
  const unsigned q = blockIdx.x * THREADS + threadIdx.x;
  const unsigned per_plane = Sy * (Sx / PX);
  if (q >= per_plane) return false;
  const unsigned Y = q / (Sx / PX), X = (q - Y * (Sx / PX)) * PX;
  const unsigned py = Y / g.TH, px = X / g.TW;
  o.y = Y - py * g.TH;
  o.x = X - px * g.TW;
  o.k = py * g.nx + px;
  o.p = (int64_t)Y * Sx + X;
  o.plane = (int64_t)Sy * Sx;
  const int s = slot ? slot[o.k] : o.k;
  o.s = (unsigned)s < (unsigned)g.Kout ? s : -1;
  o.live = live ? live[o.k] != 0 : true;
  return true;
}

// element offset (in pixels, not floats) of (b, prim, z, y, x) in a [B, Kn, TD, TH, TW, .] template
__device__ __forceinline__ int64_t tpl_off(const TplGeom& g, int b, int Kn, int prim, int z, int y, int x) {
  return ((((int64_t)b * Kn + prim) * g.TD + z) * g.TH + y) * g.TW + x;
}

// ---- four channels: one pixel per lane, one 16-byte store (load) per template --------------------------------------------
__global__ __launch_bounds__(THREADS) void template4_fwd_kernel(const TplGeom g, const float* __restrict__ rgb_,
                                                                const float* __restrict__ alpha_,
                                                                const int32_t* __restrict__ slot,
                                                                const int32_t* __restrict__ live, float* __restrict__ out_,
                                                                float* __restrict__ full_) {
  TplPos t;
  if (!tpl_pos<1>(g, slot, live, t)) return;
  const int b = blockIdx.y;
  const bool write = t.s >= 0, data = write && t.live;
  if (!write && !full_) return;                      // a dropped primitive: its input is not read
  const bool read = data || full_;
  const gfloat* rgb = global_in(rgb_) + (int64_t)b * g.TD * 3 * t.plane + t.p;
  const gfloat* alpha = global_in(alpha_) + (int64_t)b * g.TD * t.plane + t.p;
  gf4* out = reinterpret_cast<gf4*>(global_out(out_));
  gf4* full = reinterpret_cast<gf4*>(global_out(full_));
  for (int z0 = 0; z0 < g.TD; z0 += UNROLL) {
    f4 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int z = z0 + u;
      v[u] = f4{0.f, 0.f, 0.f, 0.f};
      if (z < g.TD && read) {
        const gfloat* c = rgb + (int64_t)z * 3 * t.plane;
        v[u] = f4{c[0], c[t.plane], c[2 * t.plane], alpha[(int64_t)z * t.plane]};
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int z = z0 + u;
      if (z >= g.TD) break;
      f4 w = v[u];
      if (g.act) {
        w.x = relu_keep_nan(affine(g, w.x));
        w.y = relu_keep_nan(affine(g, w.y));
        w.z = relu_keep_nan(affine(g, w.z));
        w.w = relu_keep_nan(w.w);
      }
      if (write) out[tpl_off(g, b, g.Kout, t.s, z, t.y, t.x)] = data ? w : f4{0.f, 0.f, 0.f, 0.f};
      if (full_) full[tpl_off(g, b, g.ny * g.nx, t.k, z, t.y, t.x)] = w;
    }
  }
}

__global__ __launch_bounds__(THREADS) void template4_bwd_kernel(const TplGeom g, const float* __restrict__ rgb_,
                                                                const float* __restrict__ alpha_,
                                                                const int32_t* __restrict__ slot,
                                                                const int32_t* __restrict__ live,
                                                                const float* __restrict__ g_out_,
                                                                const float* __restrict__ g_full_, float* __restrict__ g_rgb_,
                                                                float* __restrict__ g_alpha_) {
  TplPos t;
  if (!tpl_pos<1>(g, slot, live, t)) return;
  const int b = blockIdx.y;
  const bool data = g_out_ && t.s >= 0 && t.live;
  const gf4* g_out = reinterpret_cast<const gf4*>(global_in(g_out_));
  const gf4* g_full = reinterpret_cast<const gf4*>(global_in(g_full_));
  const int64_t in_rgb = (int64_t)b * g.TD * 3 * t.plane + t.p, in_a = (int64_t)b * g.TD * t.plane + t.p;
  const gfloat* rgb = global_in(rgb_) + in_rgb;
  const gfloat* alpha = global_in(alpha_) + in_a;
  gfloat* g_rgb = global_out(g_rgb_) + in_rgb;
  gfloat* g_alpha = global_out(g_alpha_) + in_a;
  const bool mask = g.act && (data || g_full_);      // the relu mask is recomputed from the input
  for (int z0 = 0; z0 < g.TD; z0 += UNROLL) {
    f4 v[UNROLL], in[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int z = z0 + u;
      v[u] = f4{0.f, 0.f, 0.f, 0.f};
      in[u] = f4{0.f, 0.f, 0.f, 0.f};
      if (z >= g.TD) continue;
      if (data) v[u] = g_out[tpl_off(g, b, g.Kout, t.s, z, t.y, t.x)];
      if (g_full_) v[u] += g_full[tpl_off(g, b, g.ny * g.nx, t.k, z, t.y, t.x)];
      if (mask) {
        const gfloat* c = rgb + (int64_t)z * 3 * t.plane;
        in[u] = f4{c[0], c[t.plane], c[2 * t.plane], alpha[(int64_t)z * t.plane]};
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int z = z0 + u;
      if (z >= g.TD) break;
      f4 w = v[u];
      if (mask) {
        w.x = affine(g, in[u].x) > 0.f ? w.x * g.scale : 0.f;
        w.y = affine(g, in[u].y) > 0.f ? w.y * g.scale : 0.f;
        w.z = affine(g, in[u].z) > 0.f ? w.z * g.scale : 0.f;
        w.w = in[u].w > 0.f ? w.w : 0.f;
      }
      gfloat* c = g_rgb + (int64_t)z * 3 * t.plane;
      c[0] = w.x;
      c[t.plane] = w.y;
      c[2 * t.plane] = w.z;
      g_alpha[(int64_t)z * t.plane] = w.w;
    }
  }
}

// ---- one channel (alpha only): PX = 4 consecutive X per lane and a 16-byte store (TW a multiple of 4), else PX = 1 -------
template <int PX>
struct PxVec {
  float v[PX];
};

template <int PX>
__device__ __forceinline__ void px_store(gfloat* p, const PxVec<PX>& w) {
  if constexpr (PX == 4) {
    *reinterpret_cast<gf4*>(p) = f4{w.v[0], w.v[1], w.v[2], w.v[3]};
  } else {
    p[0] = w.v[0];
  }
}
template <int PX>
__device__ __forceinline__ PxVec<PX> px_load(const gfloat* p) {
  PxVec<PX> w;
  if constexpr (PX == 4) {
    const f4 q = *reinterpret_cast<const gf4*>(p);
    w.v[0] = q.x, w.v[1] = q.y, w.v[2] = q.z, w.v[3] = q.w;
  } else {
    w.v[0] = p[0];
  }
  return w;
}

template <int PX>
__global__ __launch_bounds__(THREADS) void template1_fwd_kernel(const TplGeom g, const float* __restrict__ alpha_,
                                                                const int32_t* __restrict__ slot,
                                                                const int32_t* __restrict__ live, float* __restrict__ out_,
                                                                float* __restrict__ full_) {
  TplPos t;
  if (!tpl_pos<PX>(g, slot, live, t)) return;
  const int b = blockIdx.y;
  const bool write = t.s >= 0, data = write && t.live;
  if (!write && !full_) return;
  const bool read = data || full_;
  const gfloat* alpha = global_in(alpha_) + (int64_t)b * g.TD * t.plane + t.p;
  gfloat* out = global_out(out_);
  gfloat* full = global_out(full_);
  for (int z0 = 0; z0 < g.TD; z0 += UNROLL) {
    PxVec<PX> v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int z = z0 + u;
#pragma unroll
      for (int i = 0; i < PX; ++i) v[u].v[i] = (z < g.TD && read) ? alpha[(int64_t)z * t.plane + i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int z = z0 + u;
      if (z >= g.TD) break;
      PxVec<PX> w = v[u], zero;
#pragma unroll
      for (int i = 0; i < PX; ++i) {
        if (g.act) w.v[i] = relu_keep_nan(w.v[i]);
        zero.v[i] = 0.f;
      }
      if (write) px_store<PX>(out + tpl_off(g, b, g.Kout, t.s, z, t.y, t.x), data ? w : zero);
      if (full_) px_store<PX>(full + tpl_off(g, b, g.ny * g.nx, t.k, z, t.y, t.x), w);
    }
  }
}

template <int PX>
__global__ __launch_bounds__(THREADS) void template1_bwd_kernel(const TplGeom g, const float* __restrict__ alpha_,
                                                                const int32_t* __restrict__ slot,
                                                                const int32_t* __restrict__ live,
                                                                const float* __restrict__ g_out_,
                                                                const float* __restrict__ g_full_,
                                                                float* __restrict__ g_alpha_) {
  TplPos t;
  if (!tpl_pos<PX>(g, slot, live, t)) return;
  const int b = blockIdx.y;
  const bool data = g_out_ && t.s >= 0 && t.live;
  const gfloat* g_out = global_in(g_out_);
  const gfloat* g_full = global_in(g_full_);
  const int64_t in_a = (int64_t)b * g.TD * t.plane + t.p;
  const gfloat* alpha = global_in(alpha_) + in_a;
  gfloat* g_alpha = global_out(g_alpha_) + in_a;
  const bool mask = g.act && (data || g_full_);
  for (int z0 = 0; z0 < g.TD; z0 += UNROLL) {
    PxVec<PX> v[UNROLL], in[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int z = z0 + u;
#pragma unroll
      for (int i = 0; i < PX; ++i) v[u].v[i] = in[u].v[i] = 0.f;
      if (z >= g.TD) continue;
      if (data) v[u] = px_load<PX>(g_out + tpl_off(g, b, g.Kout, t.s, z, t.y, t.x));
      if (g_full_) {
        const PxVec<PX> f = px_load<PX>(g_full + tpl_off(g, b, g.ny * g.nx, t.k, z, t.y, t.x));
#pragma unroll
        for (int i = 0; i < PX; ++i) v[u].v[i] += f.v[i];
      }
      if (mask) {
#pragma unroll
        for (int i = 0; i < PX; ++i) in[u].v[i] = alpha[(int64_t)z * t.plane + i];
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int z = z0 + u;
      if (z >= g.TD) break;
#pragma unroll
      for (int i = 0; i < PX; ++i) {
        const float w = (mask && !(in[u].v[i] > 0.f)) ? 0.f : v[u].v[i];
        g_alpha[(int64_t)z * t.plane + i] = w;
      }
    }
  }
}

// ---- primitive transforms: one lane per primitive -----------------------------------------------------------------------
// A(r) of hand_mvp.py:477-510 as written: theta = sqrt(1e-5 + |r|^2), n = r / theta (NOT unit length), diagonal
// n_i^2 + (1 - n_i^2) cos theta, off-diagonal n_i n_j (1 - cos theta) -+ n_k sin theta.
struct AxisAngle {
  float theta, n[3], c, s;
};

__device__ __forceinline__ AxisAngle axis_angle(const float* r) {
  AxisAngle a;
  a.theta = sqrtf(1e-5f + (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
  for (int i = 0; i < 3; ++i) a.n[i] = r[i] / a.theta;
  a.c = cosf(a.theta);
  a.s = sinf(a.theta);
  return a;
}

__device__ __forceinline__ void axis_angle_matrix(const AxisAngle& a, float* A) {
  const float* n = a.n;
  const float k = 1.f - a.c;
  A[0] = n[0] * n[0] + (1.f - n[0] * n[0]) * a.c;
  A[1] = n[0] * n[1] * k - n[2] * a.s;
  A[2] = n[0] * n[2] * k + n[1] * a.s;
  A[3] = n[0] * n[1] * k + n[2] * a.s;
  A[4] = n[1] * n[1] + (1.f - n[1] * n[1]) * a.c;
  A[5] = n[1] * n[2] * k - n[0] * a.s;
  A[6] = n[0] * n[2] * k - n[1] * a.s;
  A[7] = n[1] * n[2] * k + n[0] * a.s;
  A[8] = n[2] * n[2] + (1.f - n[2] * n[2]) * a.c;
}

__global__ __launch_bounds__(THREADS) void primtransf_fwd_kernel(int M, const float* __restrict__ posbase,
                                                                 const float* __restrict__ rotbase,
                                                                 const float* __restrict__ delta_pos,
                                                                 const float* __restrict__ delta_rvec,
                                                                 const float* __restrict__ delta_scale, float prim_scale,
                                                                 float* __restrict__ primpos, float* __restrict__ primrot,
                                                                 float* __restrict__ primscale) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= M) return;
  float R[9], A[9], d[3], r[3];
  for (int j = 0; j < 9; ++j) R[j] = rotbase[(size_t)i * 9 + j];
  for (int j = 0; j < 3; ++j) {
    d[j] = delta_pos[(size_t)i * 3 + j];
    r[j] = delta_rvec[(size_t)i * 3 + j];
  }
  axis_angle_matrix(axis_angle(r), A);
  for (int j = 0; j < 3; ++j) {
    primpos[(size_t)i * 3 + j] = posbase[(size_t)i * 3 + j] + (R[3 * j] * d[0] + R[3 * j + 1] * d[1] + R[3 * j + 2] * d[2]);
    primscale[(size_t)i * 3 + j] = prim_scale * delta_scale[(size_t)i * 3 + j];
    for (int l = 0; l < 3; ++l)
      primrot[(size_t)i * 9 + 3 * j + l] = R[3 * j] * A[l] + R[3 * j + 1] * A[3 + l] + R[3 * j + 2] * A[6 + l];
  }
}

// g_delta_pos = R^T g_primpos; g_delta_scale = prim_scale g_primscale; G = R^T g_primrot is dL/dA, taken through
// A(n, cos, sin), n = r / theta, theta(r).  theta >= sqrt(1e-5): finite at r = 0.
__global__ __launch_bounds__(THREADS) void primtransf_bwd_kernel(int M, const float* __restrict__ rotbase,
                                                                 const float* __restrict__ delta_rvec, float prim_scale,
                                                                 const float* __restrict__ g_primpos,
                                                                 const float* __restrict__ g_primrot,
                                                                 const float* __restrict__ g_primscale,
                                                                 float* __restrict__ g_delta_pos,
                                                                 float* __restrict__ g_delta_rvec,
                                                                 float* __restrict__ g_delta_scale) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= M) return;
  float R[9], G[9], gp[3], r[3];
  for (int j = 0; j < 9; ++j) R[j] = rotbase[(size_t)i * 9 + j];
  for (int j = 0; j < 3; ++j) {
    r[j] = delta_rvec[(size_t)i * 3 + j];
    gp[j] = g_primpos ? g_primpos[(size_t)i * 3 + j] : 0.f;
    g_delta_scale[(size_t)i * 3 + j] = g_primscale ? prim_scale * g_primscale[(size_t)i * 3 + j] : 0.f;
  }
  for (int j = 0; j < 3; ++j) g_delta_pos[(size_t)i * 3 + j] = R[j] * gp[0] + R[3 + j] * gp[1] + R[6 + j] * gp[2];
  if (!g_primrot) {
    for (int j = 0; j < 3; ++j) g_delta_rvec[(size_t)i * 3 + j] = 0.f;
    return;
  }
  float H[9];
  for (int j = 0; j < 9; ++j) H[j] = g_primrot[(size_t)i * 9 + j];
  for (int j = 0; j < 3; ++j)
    for (int l = 0; l < 3; ++l) G[3 * j + l] = R[j] * H[l] + R[3 + j] * H[3 + l] + R[6 + j] * H[6 + l];
  const AxisAngle a = axis_angle(r);
  const float* n = a.n;
  const float k = 1.f - a.c;
  const float s01 = G[1] + G[3], s02 = G[2] + G[6], s12 = G[5] + G[7];
  const float g_c = G[0] * (1.f - n[0] * n[0]) + G[4] * (1.f - n[1] * n[1]) + G[8] * (1.f - n[2] * n[2])
                    - (s01 * n[0] * n[1] + s02 * n[0] * n[2] + s12 * n[1] * n[2]);
  const float g_s = n[0] * (G[7] - G[5]) + n[1] * (G[2] - G[6]) + n[2] * (G[3] - G[1]);
  float g_n[3];
  g_n[0] = k * (2.f * G[0] * n[0] + s01 * n[1] + s02 * n[2]) + a.s * (G[7] - G[5]);
  g_n[1] = k * (2.f * G[4] * n[1] + s01 * n[0] + s12 * n[2]) + a.s * (G[2] - G[6]);
  g_n[2] = k * (2.f * G[8] * n[2] + s02 * n[0] + s12 * n[1]) + a.s * (G[3] - G[1]);
  const float inv = 1.f / a.theta;
  // n = r / theta: d n_i / d theta = -n_i / theta; d theta / d r_j = r_j / theta = n_j
  const float g_theta = g_s * a.c - g_c * a.s - (g_n[0] * n[0] + g_n[1] * n[1] + g_n[2] * n[2]) * inv;
  for (int j = 0; j < 3; ++j) g_delta_rvec[(size_t)i * 3 + j] = g_n[j] * inv + g_theta * n[j];
}


}  // namespace

#define TPL_REQUIRE_SIZES()                                                                                          \
  GOL_REQUIRE(B >= 0 && TD >= 1 && TH >= 1 && TW >= 1 && ny >= 1 && nx >= 1 && Kout >= 0, "bad sizes");              \
  GOL_REQUIRE((long long)ny * TH * nx * TW < (1ll << 31) && (long long)ny * nx < (1ll << 31), "slab too large");     \
  GOL_REQUIRE(B <= 65535, "B > 65535");                                                                              \
  GOL_REQUIRE(Kout <= ny * nx, "Kout exceeds the number of primitives");                                             \
  GOL_REQUIRE(slot || Kout == ny * nx, "without a slot table Kout must be ny * nx")

extern "C" int gol_mvp_template_fwd(int B, int TD, int TH, int TW, int ny, int nx, const float* rgb, const float* alpha,
                                    const int32_t* slot, const int32_t* live, int Kout, int act, float rgb_scale,
                                    float rgb_shift, float* out, float* out_full, void* stream) {
  TPL_REQUIRE_SIZES();
  if (B == 0 || (!out_full && Kout == 0)) return GOL_OK;
  GOL_REQUIRE(alpha && (out || Kout == 0), "null pointer");
  GOL_REQUIRE(gol_aligned16(out) && gol_aligned16(out_full), "the templates must be 16-byte aligned");
  const TplGeom g{TD, TH, TW, ny, nx, out ? Kout : 0, act != 0, rgb_scale, rgb_shift};
  const long long plane = (long long)ny * TH * nx * TW;
  hipStream_t st = (hipStream_t)stream;
  if (rgb) {
    template4_fwd_kernel<<<dim3(gol_cdiv(plane, THREADS), B), THREADS, 0, st>>>(g, rgb, alpha, slot, live, out, out_full);
  } else if (TW % 4 == 0) {
    template1_fwd_kernel<4><<<dim3(gol_cdiv(plane / 4, THREADS), B), THREADS, 0, st>>>(g, alpha, slot, live, out, out_full);
  } else {
    template1_fwd_kernel<1><<<dim3(gol_cdiv(plane, THREADS), B), THREADS, 0, st>>>(g, alpha, slot, live, out, out_full);
  }
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_mvp_template_bwd(int B, int TD, int TH, int TW, int ny, int nx, const float* rgb, const float* alpha,
                                    const int32_t* slot, const int32_t* live, int Kout, int act, float rgb_scale,
                                    float rgb_shift, const float* g_out, const float* g_out_full, float* g_rgb,
                                    float* g_alpha, void* stream) {
  TPL_REQUIRE_SIZES();
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(g_alpha, "null pointer");
  GOL_REQUIRE(!act || (alpha && (rgb || !g_rgb)), "the activation's mask needs the forward's input");
  GOL_REQUIRE(gol_aligned16(g_out) && gol_aligned16(g_out_full), "the template gradients must be 16-byte aligned");
  const TplGeom g{TD, TH, TW, ny, nx, g_out ? Kout : 0, act != 0, rgb_scale, rgb_shift};
  const long long plane = (long long)ny * TH * nx * TW;
  hipStream_t st = (hipStream_t)stream;
  if (g_rgb) {
    template4_bwd_kernel<<<dim3(gol_cdiv(plane, THREADS), B), THREADS, 0, st>>>(g, rgb, alpha, slot, live, g_out, g_out_full,
                                                                                 g_rgb, g_alpha);
  } else if (TW % 4 == 0) {
    template1_bwd_kernel<4><<<dim3(gol_cdiv(plane / 4, THREADS), B), THREADS, 0, st>>>(g, alpha, slot, live, g_out,
                                                                                        g_out_full, g_alpha);
  } else {
    template1_bwd_kernel<1><<<dim3(gol_cdiv(plane, THREADS), B), THREADS, 0, st>>>(g, alpha, slot, live, g_out, g_out_full,
                                                                                    g_alpha);
  }
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_mvp_primtransf_fwd(int B, int K, const float* posbase, const float* rotbase, const float* delta_pos,
                                      const float* delta_rvec, const float* delta_scale, float prim_scale, float* primpos,
                                      float* primrot, float* primscale, void* stream) {
  GOL_REQUIRE(B >= 0 && K >= 0, "bad sizes");
  GOL_REQUIRE((long long)B * K * 9 < (1ll << 31), "B * K too large");
  if (B == 0 || K == 0) return GOL_OK;
  GOL_REQUIRE(posbase && rotbase && delta_pos && delta_rvec && delta_scale && primpos && primrot && primscale, "null pointer");
  primtransf_fwd_kernel<<<gol_cdiv((long long)B * K, THREADS), THREADS, 0, (hipStream_t)stream>>>(
      B * K, posbase, rotbase, delta_pos, delta_rvec, delta_scale, prim_scale, primpos, primrot, primscale);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_mvp_primtransf_bwd(int B, int K, const float* rotbase, const float* delta_rvec, float prim_scale,
                                      const float* g_primpos, const float* g_primrot, const float* g_primscale,
                                      float* g_delta_pos, float* g_delta_rvec, float* g_delta_scale, void* stream) {
  GOL_REQUIRE(B >= 0 && K >= 0, "bad sizes");
  GOL_REQUIRE((long long)B * K * 9 < (1ll << 31), "B * K too large");
  if (B == 0 || K == 0) return GOL_OK;
  GOL_REQUIRE(rotbase && delta_rvec && g_delta_pos && g_delta_rvec && g_delta_scale, "null pointer");
  primtransf_bwd_kernel<<<gol_cdiv((long long)B * K, THREADS), THREADS, 0, (hipStream_t)stream>>>(
      B * K, rotbase, delta_rvec, prim_scale, g_primpos, g_primrot, g_primscale, g_delta_pos, g_delta_rvec, g_delta_scale);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
