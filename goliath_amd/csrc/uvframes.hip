// uvframes.hip -- URHand's per-texel tangent frames, normal map and view conditioning, forward and backward, gfx950 (wave64).
//
// Replaces the ATen chain of ConvTeacherDecoder.forward (ca_code/models/urhand.py:366-392, :467-486, :573-578): a
// boolean-mask gather of [B,M,3,3] vertex positions, a Python loop over the batch (or xyz2normals' cat / cat / slice
// stencil, ca_code/utils/geom.py:665-686), the dozen elementwise kernels of compute_tbn_uv_given_normal (geom.py:432-470),
// a zeroed [B,S,S,3,3] image with a masked scatter, and a batched [1,3] @ [3,3] matmul over all texels.
// Topology: goliath_amd/uvframes.py:UVFramesTopology = a UVTopology over index_image (texel_rec, triples, items) plus
//   tri_const[T,4]        per triple (f, vt01.y, vt02.y, 0): compute_tbn_uv_given_normal's topology constants, float32
//   tri_item_start[T+1]   a triple's run of items;  vq_start[V+1], vq_slot[3T]: vertex -> (triple, corner) slots
//   a second UVTopology over vi[face_index_image] (mode A's normal triple; the same arrays where the two images agree)
// Kernels:
//   triple fwd      one thread per (view, triple): t0 = the first, per-triangle tangent.  It does not depend on the texel.
//   texel fwd       one thread per texel in linear order, the view loop inside: normal (mode A: interpolated vertex
//                   normals, mode B: the position map's finite differences), b = n x t0, t = b x n, planar stores of
//                   the normal map and of frame . view; the [B,S,S,3,3] image only on request.  Zeros where uncovered.
//   texel bwd       the same walk: recomputes the chain, writes per-texel g_t0 and g_nraw (A) / g_U, g_V (B) planes, the
//                   view term of g_posmap and per-workgroup double partials of g_cam_pos.
//   stencil bwd     (mode B) the transpose of the finite differences as a gather over the g_U, g_V planes.
//   item / triple / vertex bwd   g_t0 summed per item (one 16-lane row each, DPP), per triple (through the tangent's
//                   normalisation to the three corners), per vertex (its (triple, corner) slots in slot order, fp64).
//   mode A's g_nraw goes through gol_values_to_uv_bwd (the normal topology) and gol_vert_normals_bwd.
// No atomics: every sum has a fixed order, results are bitwise reproducible.  Clamp semantics are autograd's.
#include "gol_common.h"
#include "gol_stream.h"
#include "gol_vec3.h"

namespace {

using namespace gol_vec3;

constexpr float kTbnEps = 1e-5f;     // compute_tbn_uv_given_normal's eps and urhand.py:383's clamp
constexpr float kXyzEps = 1e-8f;     // xyz2normals' eps (geom.py:665)
constexpr float kViewEps = 1e-12f;   // F.normalize's eps (urhand.py:573)
constexpr int kItemRow = 16;         // lanes per item (one DPP row)
constexpr int kWaves = 4;            // waves of a 256-lane workgroup

__device__ __forceinline__ V3 neg(V3 a) { return V3{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ V3 ldp(const float* __restrict__ p, size_t P) { return V3{p[0], p[P], p[2 * P]}; }
__device__ __forceinline__ void stp(float* __restrict__ p, size_t P, V3 v) { p[0] = v.x; p[P] = v.y; p[2 * P] = v.z; }

// the un-normalised tangent of a triple: f (v01 vt02.y - v02 vt01.y), geom.py:456-458
__device__ __forceinline__ V3 tangent_raw(const float* __restrict__ vb, int a, int b, int c, float4 k) {
  const V3 p0 = ld3(vb + 3 * a);
  const V3 v01 = ld3(vb + 3 * b) - p0, v02 = ld3(vb + 3 * c) - p0;
  return (v01 * k.z - v02 * k.y) * k.x;
}

__global__ __launch_bounds__(256) void t0_fwd_kernel(int B, int V, int T, const float* __restrict__ verts,
                                                     const int32_t* __restrict__ triples,
                                                     const float* __restrict__ tri_const, float* __restrict__ t0) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * T) return;
  const size_t b = i / T;
  const int tid = (int)(i - b * T);
  int ia, ib, ic;
  V3 t = {0.f, 0.f, 0.f};
  if (ids3(triples, tid, V, ia, ib, ic)) {
    t = tangent_raw(verts + b * V * 3, ia, ib, ic, reinterpret_cast<const float4*>(tri_const)[tid]);
    t = t / fmaxf(norm(t), kTbnEps);
  }
  st3(t0 + i * 3, t);
}

// what a texel needs from the topology; the same for every view
struct Texel {
  bool covered;
  int tid, row, col;
  int a, b, c;          // mode A: the normal's vertex triple
  float w0, w1, w2;
};
template <bool MODE_B>
__device__ __forceinline__ Texel load_texel(const int32_t* __restrict__ texel_rec, const int32_t* __restrict__ ntexel_rec,
                                            const int32_t* __restrict__ ntriples, size_t t, int S, int T, int Tn, int V) {
  const int4 r = reinterpret_cast<const int4*>(texel_rec)[t];
  Texel x;
  x.tid = r.x;
  x.covered = (unsigned)r.x < (unsigned)T;
  x.w0 = __int_as_float(r.y); x.w1 = __int_as_float(r.z); x.w2 = __int_as_float(r.w);
  x.row = (int)(t / S); x.col = (int)(t - (size_t)x.row * S);
  x.a = x.b = x.c = 0;
  if (!MODE_B && x.covered) {
    const int nt = ntexel_rec[4 * t];
    x.covered = (unsigned)nt < (unsigned)Tn && ids3(ntriples, nt, V, x.a, x.b, x.c);
  }
  return x;
}

// the forward chain of one (view, texel): src = the un-normalised normal (A: interpolated, B: U x V)
struct Chain {
  V3 U, Vv, src, n, braw, b, traw, t;
};
template <bool MODE_B>
__device__ __forceinline__ Chain chain(const Texel& x, int S, const float* __restrict__ vnb, const float* __restrict__ pm,
                                       V3 t0) {
  Chain k;
  if (MODE_B) {
    const size_t P = (size_t)S * S, at = (size_t)x.row * S + x.col;
    const V3 z = {0.f, 0.f, 0.f};
    const V3 dn = x.row + 1 < S ? ldp(pm + at + S, P) : z, up = x.row > 0 ? ldp(pm + at - S, P) : z;
    const V3 rt = x.col + 1 < S ? ldp(pm + at + 1, P) : z, lf = x.col > 0 ? ldp(pm + at - 1, P) : z;
    k.U = (dn - up) * -0.5f;       // (x[r+1] - x[r-1]) / -2, geom.py:679
    k.Vv = (rt - lf) * -0.5f;
    k.src = cross(k.U, k.Vv);
    k.n = k.src / fmaxf(norm(k.src), kXyzEps);
  } else {
    k.U = k.Vv = V3{0.f, 0.f, 0.f};
    k.src = ld3(vnb + 3 * x.a) * x.w0 + ld3(vnb + 3 * x.b) * x.w1 + ld3(vnb + 3 * x.c) * x.w2;
    k.n = k.src / fmaxf(norm(k.src), kTbnEps);
  }
  k.braw = cross(k.n, t0);
  k.b = k.braw / fmaxf(norm(k.braw), kTbnEps);
  k.traw = cross(k.b, k.n);
  k.t = k.traw / fmaxf(norm(k.traw), kTbnEps);
  return k;
}

template <bool MODE_B>
__global__ __launch_bounds__(256) void uvframes_fwd_kernel(int B, int V, int S, int T, int Tn, float sgn,
                                                           const int32_t* __restrict__ texel_rec,
                                                           const int32_t* __restrict__ ntexel_rec,
                                                           const int32_t* __restrict__ ntriples,
                                                           const float* __restrict__ vn, const float* __restrict__ posmap,
                                                           const float* __restrict__ cam_pos, const float* __restrict__ t0,
                                                           float* __restrict__ nml, float* __restrict__ viewout,
                                                           float* __restrict__ frames) {
  const size_t P = (size_t)S * S;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= P) return;
  const Texel x = load_texel<MODE_B>(texel_rec, ntexel_rec, ntriples, t, S, T, Tn, V);
  for (int b = 0; b < B; ++b) {
    V3 r0 = {0.f, 0.f, 0.f}, r1 = r0, r2 = r0, vo = r0;
    if (x.covered) {
      const float* pm = posmap ? posmap + (size_t)b * 3 * P : nullptr;
      const Chain k = chain<MODE_B>(x, S, vn ? vn + (size_t)b * V * 3 : nullptr, pm,
                                    ld3(t0 + ((size_t)b * T + x.tid) * 3));
      r0 = k.t; r1 = neg(k.b); r2 = k.n * sgn;
      if (viewout) {
        const V3 d = ld3(cam_pos + 3 * b) - ldp(pm + t, P);
        const V3 v = d / fmaxf(norm(d), kViewEps);
        vo = V3{dot(r0, v), dot(r1, v), dot(r2, v)};
      }
    }
    stp(nml + (size_t)b * 3 * P + t, P, r2);
    if (viewout) stp(viewout + (size_t)b * 3 * P + t, P, vo);
    if (frames) {
      float* f = frames + ((size_t)b * P + t) * 9;
      st3(f, r0); st3(f + 3, r1); st3(f + 6, r2);
    }
  }
}

// One thread per texel, every thread reaches the workgroup sums.  g_t0tex[B,3,P]; g_aux[B,3,P] (A: g_nraw) or [B,6,P]
// (B: g_U, g_V); g_posmap[B,3,P] (may be NULL) receives the view term; cam_part[B, gridDim.x, 3] (may be NULL).
template <bool MODE_B>
__global__ __launch_bounds__(256) void uvframes_bwd_texel_kernel(
    int B, int V, int S, int T, int Tn, float sgn, const int32_t* __restrict__ texel_rec,
    const int32_t* __restrict__ ntexel_rec, const int32_t* __restrict__ ntriples, const float* __restrict__ vn,
    const float* __restrict__ posmap, const float* __restrict__ cam_pos, const float* __restrict__ t0,
    const float* __restrict__ g_nml, const float* __restrict__ g_viewout, const float* __restrict__ g_frames,
    float* __restrict__ g_t0tex, float* __restrict__ g_aux, float* __restrict__ g_posmap, double* __restrict__ cam_part) {
  __shared__ double sh[kWaves];
  const size_t P = (size_t)S * S;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool inside = t < P;
  Texel x;
  x.covered = false;
  if (inside) x = load_texel<MODE_B>(texel_rec, ntexel_rec, ntriples, t, S, T, Tn, V);
  constexpr int kAux = MODE_B ? 6 : 3;
  const V3 z = {0.f, 0.f, 0.f};
  for (int b = 0; b < B; ++b) {
    V3 g_t0 = z, g_a0 = z, g_a1 = z, g_p = z;
    if (x.covered) {
      const float* pm = posmap ? posmap + (size_t)b * 3 * P : nullptr;
      const V3 t0v = ld3(t0 + ((size_t)b * T + x.tid) * 3);
      const Chain k = chain<MODE_B>(x, S, vn ? vn + (size_t)b * V * 3 : nullptr, pm, t0v);
      V3 g_r0 = z, g_r1 = z, g_r2 = z;
      if (g_frames) {
        const float* f = g_frames + ((size_t)b * P + t) * 9;
        g_r0 = ld3(f); g_r1 = ld3(f + 3); g_r2 = ld3(f + 6);
      }
      if (g_nml) g_r2 = g_r2 + ldp(g_nml + (size_t)b * 3 * P + t, P);
      if (g_viewout) {
        const V3 d = ld3(cam_pos + 3 * b) - ldp(pm + t, P);
        const V3 v = d / fmaxf(norm(d), kViewEps);
        const V3 gv = ldp(g_viewout + (size_t)b * 3 * P + t, P);
        // viewout_i = row_i . v
        const V3 g_v = k.t * gv.x + neg(k.b) * gv.y + (k.n * sgn) * gv.z;
        g_r0 = g_r0 + v * gv.x; g_r1 = g_r1 + v * gv.y; g_r2 = g_r2 + v * gv.z;
        g_p = normalize_bwd(d, g_v, kViewEps);        // the gradient of d = cam_pos - posmap
      }
      // rows (t, -b, sgn n)
      V3 g_b = neg(g_r1), g_n = g_r2 * sgn;
      const V3 g_traw = normalize_bwd(k.traw, g_r0, kTbnEps);        // traw = b x n
      g_b = g_b + cross(k.n, g_traw);
      g_n = g_n + cross(g_traw, k.b);
      const V3 g_braw = normalize_bwd(k.braw, g_b, kTbnEps);         // braw = n x t0
      g_n = g_n + cross(t0v, g_braw);
      g_t0 = cross(g_braw, k.n);
      const V3 g_src = normalize_bwd(k.src, g_n, MODE_B ? kXyzEps : kTbnEps);
      if (MODE_B) {
        g_a0 = cross(k.Vv, g_src);    // src = U x V
        g_a1 = cross(g_src, k.U);
      } else {
        g_a0 = g_src;
      }
    }
    if (inside) {
      stp(g_t0tex + (size_t)b * 3 * P + t, P, g_t0);
      stp(g_aux + (size_t)b * kAux * P + t, P, g_a0);
      if (MODE_B) stp(g_aux + ((size_t)b * kAux + 3) * P + t, P, g_a1);
      if (g_posmap) stp(g_posmap + (size_t)b * 3 * P + t, P, neg(g_p));
    }
    if (cam_part) {   // wave-uniform: a kernel argument
      const double sx = gol_block_sum<double, kWaves>((double)g_p.x, sh);
      const double sy = gol_block_sum<double, kWaves>((double)g_p.y, sh);
      const double sz = gol_block_sum<double, kWaves>((double)g_p.z, sh);
      if (threadIdx.x == 0) {
        double* o = cam_part + ((size_t)b * gridDim.x + blockIdx.x) * 3;
        o[0] = sx; o[1] = sy; o[2] = sz;
      }
    }
  }
}

// g_posmap[b, :, r, c] += 0.5 (g_U[r+1, c] - g_U[r-1, c]) + 0.5 (g_V[r, c+1] - g_V[r, c-1]), zeros beyond the map: the
// transpose of U = (x[r+1] - x[r-1]) / -2 as a gather.  The same thread wrote g_posmap[.., t] in the texel pass.
__global__ __launch_bounds__(256) void uvframes_bwd_stencil_kernel(int B, int S, const float* __restrict__ g_aux,
                                                                   float* __restrict__ g_posmap) {
  const size_t P = (size_t)S * S;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= P) return;
  const int row = (int)(t / S), col = (int)(t - (size_t)row * S);
  const V3 z = {0.f, 0.f, 0.f};
  for (int b = 0; b < B; ++b) {
    const float* gu = g_aux + (size_t)b * 6 * P + t;
    const float* gv = gu + 3 * P;
    const V3 dn = row + 1 < S ? ldp(gu + S, P) : z, up = row > 0 ? ldp(gu - S, P) : z;
    const V3 rt = col + 1 < S ? ldp(gv + 1, P) : z, lf = col > 0 ? ldp(gv - 1, P) : z;
    float* o = g_posmap + (size_t)b * 3 * P + t;
    stp(o, P, ldp(o, P) + (dn - up) * 0.5f + (rt - lf) * 0.5f);
  }
}

// One 16-lane row per (view, item): item_sums[row * 3 + c] = the sum of g_t0tex[b, c, texel] over the item's texels.
__global__ __launch_bounds__(256) void uvframes_item_kernel(int B, int P, int I, const int32_t* __restrict__ item_start,
                                                            const int32_t* __restrict__ texel_of,
                                                            const float* __restrict__ g_t0tex,
                                                            float* __restrict__ item_sums) {
  const size_t row = (size_t)blockIdx.x * (256 / kItemRow) + (threadIdx.x / kItemRow);
  const int lane = threadIdx.x % kItemRow;
  const bool valid = row < (size_t)B * I;
  int s0 = 0, s1 = 0;
  size_t b = 0;
  if (valid) {
    b = row / I;
    const int item = (int)(row - b * I);
    s0 = item_start[item]; s1 = item_start[item + 1];
  }
  const float* g = g_t0tex + b * 3 * (size_t)P;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int j = s0 + lane; j < s1; j += kItemRow) {
    const int t = texel_of[j];
    if ((unsigned)t >= (unsigned)P) continue;
    a0 += g[t]; a1 += g[(size_t)P + t]; a2 += g[2 * (size_t)P + t];
  }
  a0 = gol_row_sum_to_lane15(a0); a1 = gol_row_sum_to_lane15(a1); a2 = gol_row_sum_to_lane15(a2);
  if (valid && lane == kItemRow - 1) {
    float* o = item_sums + row * 3;
    o[0] = a0; o[1] = a1; o[2] = a2;
  }
}

// One thread per (view, triple): its items in order (fp64), through t0's normalisation, to the three corners: tri_g[i, k, c]
__global__ __launch_bounds__(256) void uvframes_triple_bwd_kernel(int B, int V, int T, int I,
                                                                  const float* __restrict__ verts,
                                                                  const int32_t* __restrict__ triples,
                                                                  const float* __restrict__ tri_const,
                                                                  const int32_t* __restrict__ tri_item_start,
                                                                  const float* __restrict__ item_sums,
                                                                  float* __restrict__ tri_g) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * T) return;
  const size_t b = i / T;
  const int tid = (int)(i - b * T);
  V3 g0 = {0.f, 0.f, 0.f}, g1 = g0, g2 = g0;
  int ia, ib, ic;
  if (ids3(triples, tid, V, ia, ib, ic)) {
    double s[3] = {0.0, 0.0, 0.0};
    const int j1 = min(tri_item_start[tid + 1], I);
    for (int j = max(tri_item_start[tid], 0); j < j1; ++j) {
      const float* o = item_sums + (b * I + j) * 3;
      s[0] += (double)o[0]; s[1] += (double)o[1]; s[2] += (double)o[2];
    }
    const float4 k = reinterpret_cast<const float4*>(tri_const)[tid];
    const V3 raw = tangent_raw(verts + b * V * 3, ia, ib, ic, k);
    const V3 g_in = normalize_bwd(raw, V3{(float)s[0], (float)s[1], (float)s[2]}, kTbnEps) * k.x;
    g1 = g_in * k.z;            // v01 = p1 - p0
    g2 = g_in * -k.y;           // v02 = p2 - p0
    g0 = neg(g1 + g2);
  }
  float* o = tri_g + i * 9;
  st3(o, g0); st3(o + 3, g1); st3(o + 6, g2);
}

// g_verts[b, v] (+)= the sum over the vertex's (triple, corner) slots, in slot order
template <bool ACCUMULATE>
__global__ __launch_bounds__(256) void uvframes_vertex_kernel(int B, int V, int T, const int32_t* __restrict__ vq_start,
                                                              const int32_t* __restrict__ vq_slot,
                                                              const float* __restrict__ tri_g,
                                                              float* __restrict__ g_verts) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * V) return;
  const size_t b = i / V;
  const int v = (int)(i - b * V);
  const float* base = tri_g + b * T * 9;
  double s[3] = {0.0, 0.0, 0.0};
  const int j1 = min(vq_start[v + 1], 3 * T);
  for (int j = max(vq_start[v], 0); j < j1; ++j) {
    const int slot = vq_slot[j];
    if ((unsigned)slot >= 3u * (unsigned)T) continue;
    const float* o = base + (size_t)slot * 3;
    s[0] += (double)o[0]; s[1] += (double)o[1]; s[2] += (double)o[2];
  }
  V3 g = {(float)s[0], (float)s[1], (float)s[2]};
  if (ACCUMULATE) g = g + ld3(g_verts + i * 3);
  st3(g_verts + i * 3, g);
}

// One workgroup per (view, axis): lane l adds partials l, l + 256, ... in order, then the fixed-order workgroup sum.
__global__ __launch_bounds__(256) void uvframes_cam_finalize_kernel(int nblk, const double* __restrict__ cam_part,
                                                                    float* __restrict__ g_cam_pos) {
  __shared__ double sh[kWaves];
  const int b = blockIdx.x / 3, c = blockIdx.x - 3 * b;
  const double* p = cam_part + (size_t)b * nblk * 3 + c;
  double s = 0.0;
  for (int j = threadIdx.x; j < nblk; j += 256) s += p[(size_t)j * 3];
  s = gol_block_sum<double, kWaves>(s, sh);
  if (threadIdx.x == 0) g_cam_pos[blockIdx.x] = (float)s;
}

inline bool fits_int(long long n) { return n > 0 && n < (1ll << 31); }
inline long long up4(long long n) { return (n + 3) & ~3ll; }

// the backward's scratch, in floats from its start (the double partials first: 8-byte aligned)
struct Scratch {
  long long cam, g_t0tex, g_aux, item_t0, tri_g, nitem, g_vn, g_s, total;
};
inline Scratch scratch_layout(int B, int V, int S, int T, int I, int In, int mode) {
  const long long P = (long long)S * S, nblk = (P + 255) / 256;
  Scratch s;
  long long at = 0;
  s.cam = at; at += up4(2 * B * nblk * 3);
  s.g_t0tex = at; at += up4(B * 3 * P);
  s.g_aux = at; at += up4(B * (mode ? 6 : 3) * P);
  s.item_t0 = at; at += up4((long long)B * (I > 0 ? I : 1) * 3);
  s.tri_g = at; at += up4((long long)B * (T > 0 ? T : 1) * 9);
  s.nitem = at; at += mode ? 0 : up4((long long)B * (In > 0 ? In : 1) * 9);
  s.g_vn = at; at += mode ? 0 : up4((long long)B * V * 3);
  s.g_s = at; at += mode ? 0 : up4((long long)B * V * 3);
  s.total = at;
  return s;
}

}  // namespace

extern "C" long long gol_uvframes_bwd_scratch_floats(int B, int V, int S, int T, int I, int In, int mode) {
  if (B <= 0 || V <= 0 || S <= 0 || T < 0 || I < 0 || In < 0) return 0;
  return scratch_layout(B, V, S, T, I, In, mode).total;
}

extern "C" int gol_uvframes_fwd(int B, int V, int F, int S, int T, int Tn, int mode, int flip_normal, const float* verts,
                                const int32_t* vi, const int32_t* vf_start, const int32_t* vf_slot,
                                const int32_t* texel_rec, const int32_t* triples, const float* tri_const,
                                const int32_t* ntexel_rec, const int32_t* ntriples, const float* posmap,
                                const float* cam_pos, float* vn, float* t0, float* nml, float* viewout, float* frames,
                                void* stream) {
  GOL_REQUIRE(B > 0 && V > 0 && F >= 0 && S > 0 && T >= 0 && Tn >= 0, "B, V, S must be positive");
  GOL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (interpolated vertex normals) or 1 (position-map normals)");
  GOL_REQUIRE(verts && texel_rec && nml && (T == 0 || (triples && tri_const && t0)), "null pointer");
  GOL_REQUIRE(mode == 1 || (vi && vf_start && vf_slot && vn && ntexel_rec && (ntriples || Tn == 0)),
              "mode 0 needs the face tables, vn and the normal topology");
  GOL_REQUIRE(mode == 0 || posmap, "mode 1 needs posmap");
  GOL_REQUIRE(!viewout || (cam_pos && posmap), "viewout needs cam_pos and posmap");
  GOL_REQUIRE(fits_int((long long)S * S) && fits_int((long long)B * V * 3) && (long long)B * T * 3 < (1ll << 31),
              "S * S, B * V * 3 and B * T * 3 must fit 31 bits");
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0) {
    const int rc = gol_vert_normals_fwd(B, V, F, verts, vi, vf_start, vf_slot, kTbnEps, vn, stream);
    if (rc != GOL_OK) return rc;
  }
  if (T > 0) {
    hipLaunchKernelGGL(t0_fwd_kernel, dim3(gol_cdiv((long long)B * T, 256)), dim3(256), 0, st, B, V, T, verts, triples,
                       tri_const, t0);
    GOL_CHECK_LAUNCH();
  }
  const dim3 grid(gol_cdiv((long long)S * S, 256));
  const float sgn = flip_normal ? -1.f : 1.f;
  if (mode == 0)
    hipLaunchKernelGGL(uvframes_fwd_kernel<false>, grid, dim3(256), 0, st, B, V, S, T, Tn, sgn, texel_rec, ntexel_rec,
                       ntriples, (const float*)vn, posmap, cam_pos, (const float*)t0, nml, viewout, frames);
  else
    hipLaunchKernelGGL(uvframes_fwd_kernel<true>, grid, dim3(256), 0, st, B, V, S, T, Tn, sgn, texel_rec, ntexel_rec,
                       ntriples, (const float*)nullptr, posmap, cam_pos, (const float*)t0, nml, viewout, frames);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_uvframes_bwd(int B, int V, int F, int S, int T, int Tn, int I, int In, int mode, int flip_normal,
                                const float* verts, const int32_t* vi, const int32_t* vf_start, const int32_t* vf_slot,
                                const int32_t* texel_rec, const int32_t* triples, const float* tri_const,
                                const int32_t* item_start, const int32_t* texel_of, const int32_t* tri_item_start,
                                const int32_t* vq_start, const int32_t* vq_slot, const int32_t* ntexel_rec,
                                const int32_t* ntriples, const int32_t* nitem_start, const int32_t* ntexel_of,
                                const int32_t* nvt_start, const int32_t* nvt_slot, const float* posmap,
                                const float* cam_pos, const float* vn, const float* t0, const float* g_nml,
                                const float* g_viewout, const float* g_frames, float* scratch, float* g_verts,
                                float* g_posmap, float* g_cam_pos, void* stream) {
  GOL_REQUIRE(B > 0 && V > 0 && F >= 0 && S > 0 && T >= 0 && Tn >= 0 && I >= 0 && In >= 0, "B, V, S must be positive");
  GOL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 or 1");
  GOL_REQUIRE(verts && texel_rec && vq_start && scratch && g_verts, "null pointer");
  GOL_REQUIRE(T == 0 || (triples && tri_const && t0 && tri_item_start && vq_slot), "null pointer");
  GOL_REQUIRE(I == 0 || (item_start && texel_of), "null pointer");
  GOL_REQUIRE(mode == 1 || (vi && vf_start && vf_slot && vn && ntexel_rec && nvt_start && (ntriples || Tn == 0) &&
                            (In == 0 || (nitem_start && ntexel_of && nvt_slot))),
              "mode 0 needs the face tables, vn and the normal topology");
  GOL_REQUIRE(mode == 0 || (posmap && g_posmap), "mode 1 needs posmap and g_posmap");
  GOL_REQUIRE(!g_viewout || (cam_pos && posmap), "g_viewout needs cam_pos and posmap");
  GOL_REQUIRE(!g_cam_pos || (cam_pos && posmap && g_posmap), "g_cam_pos needs cam_pos, posmap and g_posmap");
  GOL_REQUIRE(!g_posmap || posmap, "g_posmap needs posmap");
  GOL_REQUIRE(fits_int((long long)S * S) && fits_int((long long)B * V * 3) && (long long)B * T * 9 < (1ll << 31) &&
                  (long long)B * I * 3 < (1ll << 31) && (long long)In * 9 < (1ll << 31),
              "S * S, B * V * 3, B * T * 9, B * I * 3 and In * 9 must fit 31 bits");
  GOL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "scratch must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const Scratch L = scratch_layout(B, V, S, T, I, In, mode);
  const int P = S * S;
  const int nblk = gol_cdiv(P, 256);
  const dim3 grid(nblk);
  const float sgn = flip_normal ? -1.f : 1.f;
  double* cam_part = g_cam_pos ? reinterpret_cast<double*>(scratch + L.cam) : nullptr;
  float* g_t0tex = scratch + L.g_t0tex;
  float* g_aux = scratch + L.g_aux;
  float* item_t0 = scratch + L.item_t0;
  float* tri_g = scratch + L.tri_g;
  if (mode == 0)
    hipLaunchKernelGGL(uvframes_bwd_texel_kernel<false>, grid, dim3(256), 0, st, B, V, S, T, Tn, sgn, texel_rec,
                       ntexel_rec, ntriples, vn, posmap, cam_pos, t0, g_nml, g_viewout, g_frames, g_t0tex, g_aux, g_posmap,
                       cam_part);
  else
    hipLaunchKernelGGL(uvframes_bwd_texel_kernel<true>, grid, dim3(256), 0, st, B, V, S, T, Tn, sgn, texel_rec, ntexel_rec,
                       ntriples, (const float*)nullptr, posmap, cam_pos, t0, g_nml, g_viewout, g_frames, g_t0tex, g_aux,
                       g_posmap, cam_part);
  GOL_CHECK_LAUNCH();
  if (g_cam_pos) {
    hipLaunchKernelGGL(uvframes_cam_finalize_kernel, dim3(B * 3), dim3(256), 0, st, nblk, (const double*)cam_part,
                       g_cam_pos);
    GOL_CHECK_LAUNCH();
  }
  if (mode == 1) {
    hipLaunchKernelGGL(uvframes_bwd_stencil_kernel, grid, dim3(256), 0, st, B, S, (const float*)g_aux, g_posmap);
    GOL_CHECK_LAUNCH();
  } else {
    // g_nraw [B,3,S,S] -> g_vn over the normal topology -> g_verts through the vertex normals
    float* g_vn = scratch + L.g_vn;
    int rc = gol_values_to_uv_bwd(B, V, 3, S, Tn, In, ntexel_rec, nitem_start, ntexel_of, nvt_start, nvt_slot, g_aux,
                                  scratch + L.nitem, g_vn, stream);
    if (rc != GOL_OK) return rc;
    rc = gol_vert_normals_bwd(B, V, F, verts, vi, vf_start, vf_slot, kTbnEps, g_vn, scratch + L.g_s, g_verts, stream);
    if (rc != GOL_OK) return rc;
  }
  if (I > 0) {
    hipLaunchKernelGGL(uvframes_item_kernel, dim3(gol_cdiv((long long)B * I, 256 / kItemRow)), dim3(256), 0, st, B, P, I,
                       item_start, texel_of, (const float*)g_t0tex, item_t0);
    GOL_CHECK_LAUNCH();
  }
  if (T > 0) {
    hipLaunchKernelGGL(uvframes_triple_bwd_kernel, dim3(gol_cdiv((long long)B * T, 256)), dim3(256), 0, st, B, V, T, I, verts,
                       triples, tri_const, tri_item_start, (const float*)item_t0, tri_g);
    GOL_CHECK_LAUNCH();
  }
  const dim3 vgrid(gol_cdiv((long long)B * V, 256));
  if (mode == 0)
    hipLaunchKernelGGL(uvframes_vertex_kernel<true>, vgrid, dim3(256), 0, st, B, V, T, vq_start, vq_slot,
                       (const float*)tri_g, g_verts);
  else
    hipLaunchKernelGGL(uvframes_vertex_kernel<false>, vgrid, dim3(256), 0, st, B, V, T, vq_start, vq_slot,
                       (const float*)tri_g, g_verts);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
