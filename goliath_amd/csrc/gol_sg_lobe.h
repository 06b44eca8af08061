// gol_sg_lobe.h -- the spherical-Gaussian specular lobe of ONE Gaussian towards ONE light as device functions on values in
// registers (evaluate_gaussian, extensions/sgutils/sg.cu:27-175): the weight of the forward and the terms of the backward,
// for the four w_type variants.  Shared by the stand-alone kernels (sg.hip) and by the shading kernels' point-light
// specular (shade.hip, w_type 0).  The written form of every expression decides the FMA chain under -ffp-contract=fast
// (see the note at the top of gol_vec3.h): change one here and every caller moves together.
#pragma once
#include "gol_common.h"

namespace gol_sg {

constexpr float kTwoPi = 6.28318530718f;         // sg.cu:18
constexpr float kInv2Pi = 0.15915494309f;        // sg.cu:19
constexpr float kSqrt2Pi23 = 3.03352966508f;     // sg.cu:20
constexpr float kInvSqrt2Pi23 = 0.32964899322f;  // sg.cu:21

__device__ __forceinline__ float sqr(float v) { return v * v; }

// per-Gaussian reciprocals and lobe normalisation, hoisted out of the light loop: the loop multiplies (one exact division
// per light in the forward, five in the backward otherwise)
struct Lobe { float sigma, s2, inv_sigma, inv_s2, inv_s3, inv_s4, norm; };

template <int W_TYPE>
__device__ __forceinline__ Lobe lobe_of(float sigma) {
  Lobe o;
  o.sigma = sigma;
  o.s2 = sigma * sigma;
  o.inv_sigma = 1.f / sigma; o.inv_s2 = 1.f / o.s2; o.inv_s3 = 1.f / (o.s2 * sigma); o.inv_s4 = 1.f / (o.s2 * o.s2);
  o.norm = W_TYPE == 0 ? 1.f / (sigma * kSqrt2Pi23) : (W_TYPE == 2 ? 1.f / (sigma * kTwoPi) : 1.f);
  return o;
}

// forward weight of a light at clamped cosine c to the lobe axis
template <int W_TYPE>
__device__ __forceinline__ float weight(const Lobe& o, float c) {
  if (W_TYPE == 0) return __expf(-0.5f * sqr(acosf(c) * o.inv_sigma)) * o.norm;
  if (W_TYPE == 1) return __expf(-0.5f * sqr(acosf(c) * o.inv_sigma));
  if (W_TYPE == 2) return __expf((c - 1.f) * o.inv_sigma) * o.norm;
  return __expf((c - 1.f) * o.inv_sigma);
}

// backward terms of a light at cosine c (cc = c clamped to [-1,1]) with upstream dw = <grad, light value>: the forward
// weight, the increment of the sigma gradient and d loss / d c
struct Terms { float weight, gs, dc; };

template <int W_TYPE>
__device__ __forceinline__ Terms terms(const Lobe& o, float c, float cc, float dw) {
  Terms t;
  if (W_TYPE == 0 || W_TYPE == 1) {
    const float angle = acosf(cc);
    const float ex = __expf(-0.5f * sqr(angle * o.inv_sigma));
    // sg.cu:129,139: d acos/dc = -1/sqrt(1-c^2) inside (-1,1), the constant -20 outside
    const float dacos = (c > -1.f && c < 1.f) ? -rsqrtf(1.f - c * c) : -20.f;
    if (W_TYPE == 0) {
      t.weight = ex * o.norm;
      t.gs = dw * ((ex * kInvSqrt2Pi23 * (sqr(angle) - o.s2)) * o.inv_s4);
      t.dc = dw * -((kInvSqrt2Pi23 * angle * ex) * o.inv_s3) * dacos;
    } else {
      t.weight = ex;
      t.gs = dw * ((ex * sqr(angle)) * o.inv_s3);
      t.dc = dw * -((angle * ex) * o.inv_s2) * dacos;
    }
  } else {
    const float ex = __expf((cc - 1.f) * o.inv_sigma);
    if (W_TYPE == 2) {
      t.weight = ex * o.norm;
      t.gs = dw * ((ex * kInv2Pi * ((1.f - cc) - o.sigma)) * o.inv_s3);
      t.dc = dw * kInv2Pi * ex * o.inv_s2;
    } else {
      t.weight = ex;
      t.gs = dw * ((ex * (1.f - cc) * o.inv_s2));
      t.dc = dw * ex * o.inv_sigma;
    }
  }
  return t;
}

// ---- the lobe angle without acos' conditioning (w_type 0 / 1) ---------------------------------------------------------
// The angle between the direction d to a light (any length) and the unit lobe axis l as atan2(|d x l|, d . l): acos of the
// clamped cosine for a unit l, but with an absolute error of a few ulps of 1 where acos(c) turns the rounding of c into
// ulp / sin(angle) -- the sharp lobes (sigma ~ 0.01) live at angles of a few hundredths.  sin = |d x l| / |d| likewise
// replaces sqrt(1 - c^2) in d acos / d c.  An axis that is not a unit vector (a zero reflection) keeps acos(0).
struct Angle { float angle, sin; };

__device__ __forceinline__ Angle angle_to(float dx, float dy, float dz, float lx, float ly, float lz, float inv_len) {
  const float cx = dy * lz - dz * ly, cy = dz * lx - dx * lz, cz = dx * ly - dy * lx;
  const float s = sqrtf(cx * cx + cy * cy + cz * cz), dot = dx * lx + dy * ly + dz * lz;
  Angle a;
  a.angle = (s == 0.f && dot == 0.f) ? 1.57079632679f : atan2f(s, dot);
  a.sin = s * inv_len;
  return a;
}

template <int W_TYPE>
__device__ __forceinline__ float weight_at(const Lobe& o, float angle) {
  static_assert(W_TYPE == 0 || W_TYPE == 1, "angle form: the acos lobes");
  const float ex = __expf(-0.5f * sqr(angle * o.inv_sigma));
  return W_TYPE == 0 ? ex * o.norm : ex;
}

// terms<W_TYPE> on that angle; the constant -20 of sg.cu:129,139 where the two directions are exactly (anti)parallel
template <int W_TYPE>
__device__ __forceinline__ Terms terms_at(const Lobe& o, const Angle& a, float dw) {
  static_assert(W_TYPE == 0 || W_TYPE == 1, "angle form: the acos lobes");
  Terms t;
  const float angle = a.angle;
  const float ex = __expf(-0.5f * sqr(angle * o.inv_sigma));
  const float dacos = a.sin > 0.f ? -1.f / a.sin : -20.f;
  if (W_TYPE == 0) {
    t.weight = ex * o.norm;
    t.gs = dw * ((ex * kInvSqrt2Pi23 * (sqr(angle) - o.s2)) * o.inv_s4);
    t.dc = dw * -((kInvSqrt2Pi23 * angle * ex) * o.inv_s3) * dacos;
  } else {
    t.weight = ex;
    t.gs = dw * ((ex * sqr(angle)) * o.inv_s3);
    t.dc = dw * -((angle * ex) * o.inv_s2) * dacos;
  }
  return t;
}

}  // namespace gol_sg
