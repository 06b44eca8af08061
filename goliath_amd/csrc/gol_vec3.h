// gol_vec3.h -- the float 3-vector of the geometry kernels (mvp.hip, uvlight.hip, uvgeom.hip, uvframes.hip).  A file opens it with
// `using namespace gol_vec3;`.  These files are built with -ffp-contract=fast, so the written form of an expression decides
// its FMA chain: dot is a.x*b.x + a.y*b.y + a.z*b.z, left to right, everywhere.  (gol_lbs_math.h's D3 is the double one.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gol_vec3 {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 ld3(const float* __restrict__ p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(float* __restrict__ p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return V3{a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return V3{a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float norm(V3 a) { return sqrtf(dot(a, a)); }
__device__ __forceinline__ float min3(V3 a) { return fminf(fminf(a.x, a.y), a.z); }
__device__ __forceinline__ float max3(V3 a) { return fmaxf(fmaxf(a.x, a.y), a.z); }
__device__ __forceinline__ V3 vmin(V3 a, V3 b) { return V3{fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z)}; }
__device__ __forceinline__ V3 vmax(V3 a, V3 b) { return V3{fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z)}; }

// the three vertex ids of row `r` of an [N,3] table (faces, texel triples), validated against [0, V): false = treat as absent
__device__ __forceinline__ bool ids3(const int32_t* __restrict__ tab, int r, int V, int& a, int& b, int& c) {
  a = tab[3 * r]; b = tab[3 * r + 1]; c = tab[3 * r + 2];
  return (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;
}

// gradient of x / max(|x|, eps) for upstream g (uvgeom.hip, uvframes.hip).  Autograd's clamp: below eps the denominator is
// a constant, at equality the gradient passes.
__device__ __forceinline__ V3 normalize_bwd(V3 x, V3 g, float eps) {
  const float n = norm(x);
  if (n >= eps) {
    const V3 u = x / n;
    return (g - u * dot(u, g)) / n;
  }
  return g / eps;
}

}  // namespace gol_vec3
