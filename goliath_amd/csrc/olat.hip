// olat.hip -- the MVP teacher's per-light work around its UNet (OLATRGBDecoder.forward_rgb, config 5), gfx950.
//
// Replaces (ca_code/models/hand_teacher_mvp.py):
//   :371-439  the UNet input: per-voxel light and view directions in the primitives' frames, the valid_prims mask, the
//             permute / reshape into UV layout and the cat with 1 - shadow                    -> gol_olat_features_fwd
//   :468-488  sigmoid / 25 t + 100 / relu / intensity product / sum over the lights and the
//             primshadow expand + sum, with their backward                                    -> gol_olat_combine_fwd / _bwd
// Streaming kernels.  A lane owns kV consecutive texels of one UV row: four (16-byte loads and stores) when the primitive's
// X is a multiple of 4 and every map pointer is 16-byte aligned, so that a run never leaves its primitive; one otherwise.
// Neighbouring lanes own neighbouring runs, so a wave writes 1 KiB of one channel row per store.  The loops over z and
// over the lights run inside the lane: every sum has one owner and a fixed order (no atomics, no scratch, bitwise
// reproducible), and what is shared by the lights of a frame -- the voxel position, the view direction, the upstream
// gradient of rgb -- is formed or loaded once.
#include <initializer_list>

#include "gol_common.h"

namespace {

constexpr int kBlock = 256;

template <int V>
struct Run {
  float v[V];
};

template <int V>
__device__ __forceinline__ Run<V> ld(const float* __restrict__ p, size_t i) {
  Run<V> r;
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
  } else {
    r.v[0] = p[i];
  }
  return r;
}
template <int V>
__device__ __forceinline__ void st(float* __restrict__ p, size_t i, const Run<V>& r) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p + i) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else p[i] = r.v[0];
}

// Where a lane's run lies: UV row / first column -> primitive k = h npx + w and the voxel row (y, x0) inside it.
struct Geom {
  int X, Y, Z, npx, npy;
};
struct Place {
  int row, col, k, y, x0;
};
template <int V>
__device__ __forceinline__ bool place_of(const Geom& g, Place& p) {
  const int Sx = g.npx * g.X, Sy = g.npy * g.Y, gw = Sx / V;
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= (unsigned)(gw * Sy)) return false;
  p.row = t / gw;
  p.col = (t - p.row * gw) * V;
  const int h = p.row / g.Y, w = p.col / g.X;
  p.y = p.row - h * g.Y;
  p.x0 = p.col - w * g.X;
  p.k = h * g.npx + w;
  return true;
}

struct FeatArgs {
  Geom g;
  int B, L;
  float volradius;
  const float *primpos, *primrot, *primscale, *valid, *light_pos, *campos, *shadow, *lx, *ly, *lz;
};

// valid * R^T normalize(src - p): F.normalize's v / max(|v|, 1e-12), then out_f = sum_e R[e][f] d_e
__device__ __forceinline__ void frame_dir(const float (&R)[9], float valid, const float (&src)[3], const float (&p)[3],
                                          float (&o)[3]) {
  const float d0 = src[0] - p[0], d1 = src[1] - p[1], d2 = src[2] - p[2];
  const float den = fmaxf(sqrtf(d0 * d0 + d1 * d1 + d2 * d2), 1e-12f);
  const float u0 = d0 / den, u1 = d1 / den, u2 = d2 / den;
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const float r = R[f] * u0 + R[3 + f] * u1 + R[6 + f] * u2;
    o[f] = valid != 0.f ? valid * r : 0.f;   // a dropped primitive gives exact zeros whatever its transform holds
  }
}

template <int V>
__global__ __launch_bounds__(kBlock) void olat_features_kernel(FeatArgs a, float* __restrict__ x) {
  Place pl;
  if (!place_of<V>(a.g, pl)) return;
  const int b = blockIdx.y, L = a.L;
  const int X = a.g.X, Y = a.g.Y, Z = a.g.Z, K = a.g.npx * a.g.npy;
  const size_t Sx = (size_t)a.g.npx * X, S2 = Sx * a.g.npy * Y;
  const size_t texel = (size_t)pl.row * Sx + pl.col;
  const size_t bk = (size_t)b * K + pl.k;
  float R[9], pos[3], sc[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = a.primrot[bk * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    pos[i] = a.primpos[bk * 3 + i];
    sc[i] = a.primscale[bk * 3 + i];
  }
  const float valid = a.valid[pl.k];
  const float cam[3] = {a.campos[b * 3], a.campos[b * 3 + 1], a.campos[b * 3 + 2]};
  const int YZ = Y * Z;
  for (int z = 0; z < Z; ++z) {
    // The reference's voxel position as written (hand_teacher_mvp.py:379-400): meshgrid([lz, ly, lx]).transpose(1, 3)
    // .reshape(3, -1) is later VIEWED as [.., Z, Y, X], so the voxel labelled (z, y, x) takes the flat index
    // i = (z Y + y) X + x and decodes it over the transposed extents [X, Y, Z]: local = (lz[i % Z], ly[(i / Z) % Y],
    // lx[i / (Y Z)]).
    float p[V][3];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int i = (z * Y + pl.y) * X + pl.x0 + j;
      const int ia = i / YZ, r = i - ia * YZ, ib = r / Z, ic = r - ib * Z;
      const float q0 = a.lz[ic] / sc[0], q1 = a.ly[ib] / sc[1], q2 = a.lx[ia] / sc[2];
#pragma unroll
      for (int e = 0; e < 3; ++e)
        p[j][e] = a.volradius * (pos[e] + (R[3 * e] * q0 + R[3 * e + 1] * q1 + R[3 * e + 2] * q2));
    }
    Run<V> o[3];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float d[3];
      frame_dir(R, valid, cam, p[j], d);
      o[0].v[j] = d[0]; o[1].v[j] = d[1]; o[2].v[j] = d[2];
    }
    for (int l = 0; l < L; ++l) {   // the view direction is the same for every light of the frame
      const size_t plane = ((size_t)(b * L + l) * 7 * Z + 3 * Z + 3 * z) * S2 + texel;
#pragma unroll
      for (int f = 0; f < 3; ++f) st<V>(x, plane + f * S2, o[f]);
    }
    for (int l = 0; l < L; ++l) {
      const int bl = b * L + l;
      const float light[3] = {a.light_pos[bl * 3], a.light_pos[bl * 3 + 1], a.light_pos[bl * 3 + 2]};
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float d[3];
        frame_dir(R, valid, light, p[j], d);
        o[0].v[j] = d[0]; o[1].v[j] = d[1]; o[2].v[j] = d[2];
      }
      const size_t img = (size_t)bl * 7 * Z * S2 + texel;
#pragma unroll
      for (int f = 0; f < 3; ++f) st<V>(x, img + (size_t)(3 * z + f) * S2, o[f]);
      Run<V> s = ld<V>(a.shadow, (((size_t)bl * K + pl.k) * Z + z) * Y * X + pl.y * X + pl.x0);
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] = 1.f - s.v[j];
      st<V>(x, img + (size_t)(6 * Z + z) * S2, s);
    }
  }
}

struct CombArgs {
  Geom g;
  int B, L, use_shadow;
  const float *tex, *inten, *shadow;
};

// torch's composition, rounded product by product: 25 t + 100 as a multiply and an add (near the relu's kink 25 t cancels
// against 100, a fused multiply-add would move the kink), relu, sigmoid as 1 / (1 + exp(-t)).
__device__ __forceinline__ float texolat_of(float t) {
  _Pragma("clang fp contract(off)")
  const float m = 25.f * t;
  return m + 100.f;
}
__device__ __forceinline__ float relu_of(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float sigmoid_of(float t) { return 1.f / (1.f + expf(-t)); }

template <int V>
__global__ __launch_bounds__(kBlock) void olat_combine_fwd_kernel(CombArgs a, float* __restrict__ rgb,
                                                                  float* __restrict__ texolat,
                                                                  float* __restrict__ primshadow) {
  Place pl;
  if (!place_of<V>(a.g, pl)) return;
  const int X = a.g.X, Y = a.g.Y, Z = a.g.Z, K = a.g.npx * a.g.npy, L = a.L;
  const int b = blockIdx.y / Z, z = blockIdx.y - b * Z;
  const size_t Sx = (size_t)a.g.npx * X, S2 = Sx * a.g.npy * Y;
  const size_t texel = (size_t)pl.row * Sx + pl.col;
  const size_t vox = (size_t)pl.y * X + pl.x0;
  float acc[3][V], ssum[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[0][j] = acc[1][j] = acc[2][j] = ssum[j] = 0.f;
  for (int l = 0; l < L; ++l) {
    _Pragma("clang fp contract(off)")
    const int bl = b * L + l;
    const float I[3] = {a.inten[bl * 3], a.inten[bl * 3 + 1], a.inten[bl * 3 + 2]};
    const size_t plane = ((size_t)bl * Z + z) * 4 * S2 + texel;
    const Run<V> sh = ld<V>(a.shadow, (((size_t)bl * K + pl.k) * Z + z) * Y * X + vox);
    Run<V> s = sh;
    if (!a.use_shadow) {
      s = ld<V>(a.tex, plane);
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] = sigmoid_of(s.v[j]);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) ssum[j] += sh.v[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Run<V> t = ld<V>(a.tex, plane + (1 + c) * S2);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        t.v[j] = texolat_of(t.v[j]);
        acc[c][j] += (s.v[j] * relu_of(t.v[j])) * I[c];
      }
      if (texolat) st<V>(texolat, ((size_t)bl * Z + z) * 3 * S2 + c * S2 + texel, t);
    }
  }
  const size_t out = ((size_t)b * Z + z) * 3 * S2 + texel;
  Run<V> ps;
#pragma unroll
  for (int j = 0; j < V; ++j) ps.v[j] = ssum[j] / (float)L;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    Run<V> r;
#pragma unroll
    for (int j = 0; j < V; ++j) r.v[j] = acc[c][j];
    st<V>(rgb, out + c * S2, r);
    st<V>(primshadow, out + c * S2, ps);
  }
}

template <int V>
__global__ __launch_bounds__(kBlock) void olat_combine_bwd_kernel(CombArgs a, const float* __restrict__ g_rgb,
                                                                  const float* __restrict__ g_texolat,
                                                                  float* __restrict__ g_tex) {
  Place pl;
  if (!place_of<V>(a.g, pl)) return;
  const int X = a.g.X, Y = a.g.Y, Z = a.g.Z, K = a.g.npx * a.g.npy, L = a.L;
  const int b = blockIdx.y / Z, z = blockIdx.y - b * Z;
  const size_t Sx = (size_t)a.g.npx * X, S2 = Sx * a.g.npy * Y;
  const size_t texel = (size_t)pl.row * Sx + pl.col;
  const size_t vox = (size_t)pl.y * X + pl.x0;
  Run<V> g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = ld<V>(g_rgb, ((size_t)b * Z + z) * 3 * S2 + c * S2 + texel);
  for (int l = 0; l < L; ++l) {
    const int bl = b * L + l;
    const float I[3] = {a.inten[bl * 3], a.inten[bl * 3 + 1], a.inten[bl * 3 + 2]};
    const size_t plane = ((size_t)bl * Z + z) * 4 * S2 + texel;
    Run<V> s;
    if (a.use_shadow) {
      s = ld<V>(a.shadow, (((size_t)bl * K + pl.k) * Z + z) * Y * X + vox);
    } else {
      s = ld<V>(a.tex, plane);
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] = sigmoid_of(s.v[j]);
    }
    Run<V> g0;
#pragma unroll
    for (int j = 0; j < V; ++j) g0.v[j] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const Run<V> t = ld<V>(a.tex, plane + (1 + c) * S2);
      Run<V> gt;
#pragma unroll
      for (int j = 0; j < V; ++j) gt.v[j] = 0.f;                 // an absent g_texolat
      if (g_texolat) gt = ld<V>(g_texolat, ((size_t)bl * Z + z) * 3 * S2 + c * S2 + texel);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float to = texolat_of(t.v[j]);
        const float gr = g[c].v[j] * I[c];                       // d rgb_c / d (s relu(texolat_c))
        g0.v[j] += gr * relu_of(to);
        const float through = to > 0.f ? s.v[j] * gr : 0.f;      // the relu passes nothing at exactly 0, as torch's
        gt.v[j] = 25.f * (gt.v[j] + through);
      }
      st<V>(g_tex, plane + (1 + c) * S2, gt);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) g0.v[j] = a.use_shadow ? 0.f : s.v[j] * (1.f - s.v[j]) * g0.v[j];
    st<V>(g_tex, plane, g0);
  }
}

bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}

int check_geom(const char* fn, const Geom& g, int B, int L, long long grid_y) {
  if (B < 0 || L < 1 || g.X < 1 || g.Y < 1 || g.Z < 1 || g.npx < 1 || g.npy < 1) {
    gol_set_error("%s: B >= 0, L >= 1 and a positive primsize and primitive grid are required", fn);
    return GOL_ERR_INVALID_ARG;
  }
  if ((long long)g.npx * g.X * g.npy * g.Y >= (1ll << 31) || (long long)g.X * g.Y * g.Z >= (1ll << 31) ||
      (long long)B * L >= (1ll << 28) || grid_y > 65535) {
    gol_set_error("%s: the map must hold fewer than 2^31 texels, a primitive fewer than 2^31 voxels, B L < 2^28 and the "
                  "launch's second grid dimension (B, or B Z for the combine) at most 65535", fn);
    return GOL_ERR_INVALID_ARG;
  }
  return GOL_OK;
}

dim3 grid_of(const Geom& g, int V, int grid_y) {
  const long long runs = (long long)(g.npx * g.X / V) * g.npy * g.Y;
  return dim3(gol_cdiv(runs, kBlock), grid_y);
}

}  // namespace

extern "C" int gol_olat_features_fwd(int B, int L, int X, int Y, int Z, int npx, int npy, const float* primpos,
                                     const float* primrot, const float* primscale, const float* valid_prims,
                                     const float* light_pos, const float* campos, const float* shadow, float volradius,
                                     const float* lin_x, const float* lin_y, const float* lin_z, float* x, void* stream) {
  const FeatArgs a{{X, Y, Z, npx, npy}, B, L, volradius, primpos, primrot, primscale, valid_prims, light_pos, campos,
                   shadow, lin_x, lin_y, lin_z};
  const int rc = check_geom("gol_olat_features_fwd", a.g, B, L, B);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(primpos && primrot && primscale && valid_prims && light_pos && campos && shadow && lin_x && lin_y && lin_z && x,
              "null pointer");
  if (X % 4 == 0 && aligned16({shadow, x}))
    olat_features_kernel<4><<<grid_of(a.g, 4, B), kBlock, 0, (hipStream_t)stream>>>(a, x);
  else
    olat_features_kernel<1><<<grid_of(a.g, 1, B), kBlock, 0, (hipStream_t)stream>>>(a, x);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_olat_combine_fwd(int B, int L, int X, int Y, int Z, int npx, int npy, int use_shadow, const float* tex,
                                    const float* light_intensity, const float* shadow, float* rgb, float* texolat,
                                    float* primshadow, void* stream) {
  const CombArgs a{{X, Y, Z, npx, npy}, B, L, use_shadow, tex, light_intensity, shadow};
  const int rc = check_geom("gol_olat_combine_fwd", a.g, B, L, (long long)B * Z);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(tex && light_intensity && shadow && rgb && primshadow, "null pointer");
  if (X % 4 == 0 && aligned16({tex, shadow, rgb, texolat, primshadow}))
    olat_combine_fwd_kernel<4><<<grid_of(a.g, 4, B * Z), kBlock, 0, (hipStream_t)stream>>>(a, rgb, texolat, primshadow);
  else
    olat_combine_fwd_kernel<1><<<grid_of(a.g, 1, B * Z), kBlock, 0, (hipStream_t)stream>>>(a, rgb, texolat, primshadow);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_olat_combine_bwd(int B, int L, int X, int Y, int Z, int npx, int npy, int use_shadow, const float* tex,
                                    const float* light_intensity, const float* shadow, const float* g_rgb,
                                    const float* g_texolat, float* g_tex, void* stream) {
  const CombArgs a{{X, Y, Z, npx, npy}, B, L, use_shadow, tex, light_intensity, shadow};
  const int rc = check_geom("gol_olat_combine_bwd", a.g, B, L, (long long)B * Z);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(tex && light_intensity && g_rgb && g_tex && (shadow || !use_shadow), "null pointer");
  if (X % 4 == 0 && aligned16({tex, shadow, g_rgb, g_texolat, g_tex}))
    olat_combine_bwd_kernel<4><<<grid_of(a.g, 4, B * Z), kBlock, 0, (hipStream_t)stream>>>(a, g_rgb, g_texolat, g_tex);
  else
    olat_combine_bwd_kernel<1><<<grid_of(a.g, 1, B * Z), kBlock, 0, (hipStream_t)stream>>>(a, g_rgb, g_texolat, g_tex);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
