// uvgeom.hip -- mesh -> UV position / normal maps with gradients, gfx950 (wave64).
//
// Replaces the reference's per-step PyTorch between the tracked mesh and the decoders (ca_code/utils/geom.py:308-346:
// values_to_uv, face_normals, vert_normals; called at ca_code/models/rgca.py:483-491 and urhand.py:375-394): boolean-mask
// gathers of [B,M,3,3] floats (one host sync each), three scatter_add_ calls, and an accumulating index_put of 3 M rows
// per view in the backward.  The topology is constant for a model's lifetime; goliath_amd/uvgeom.py:UVTopology packs it
// once:
//   texel_rec[P,4]   per texel: triple id (-1 = uncovered) and the three barycentrics' bit patterns -- one 16 B load
//   triples[T,3]     the distinct vertex triples of the covered texels
//   item_start[I+1], item_tid[I], texel_of[M]   covered texels grouped by triple; a triple's run is cut into ITEMS of at
//                    most 64 texels, so one triple of an impainted map that owns 10^5 texels is 1600 equal work items
//   vt_start[V+1], vt_slot[3 I]   vertex -> (item, corner) slots (slot = 3 item + corner)
//   vf_start[V+1], vf_slot[3 F]   vertex -> (face, corner) slots (slot = 3 face + corner), in face order
// Kernels:
//   vertex normals fwd   one thread per (view, vertex): gather over the vertex's faces in face order.  No atomics.
//   texel fwd            one thread per texel in linear order, the view loop inside: 16 B of topology per texel, not per
//                        view; planar stores, zeros where uncovered (no memset by the caller).
//   item reduce (bwd)    one 16-lane row per (view, item): lanes walk the item's texels, accumulate bary_k * g for the
//                        three corners, and sum across the row with 4 DPP adds per number.  No atomics.
//   vertex gather (bwd)  one thread per (view, vertex): sums its (item, corner) slots in slot order (fp64 accumulator),
//                        and, for the fused pair, pushes the normal's gradient through the vertex normalisation.
//   face gather (bwd)    one thread per (view, vertex): for each incident face, the face-normal gradient through the
//                        clamp-normalisation and the cross product, corner by corner.
// Every sum has a fixed order: all results are bitwise reproducible from run to run.
// Clamp semantics are autograd's: where a norm is below its eps the denominator is a constant in the derivative.
#include "gol_common.h"
#include "gol_vec3.h"

namespace {

constexpr float kFaceEps = 1e-5f;   // face_normals' eps (geom.py:327): vert_normals never overrides it
constexpr int kItemRow = 16;        // lanes per item (one DPP row)

using namespace gol_vec3;

// sum over the faces of vertex v of cross / max(|cross|, 1e-5), in slot (= face) order -- the order scatter_add_ visits
__device__ __forceinline__ V3 vertex_normal_sum(const float* __restrict__ vb, const int32_t* __restrict__ vi,
                                                const int32_t* __restrict__ vf_start,
                                                const int32_t* __restrict__ vf_slot, int v, int V, int F) {
  V3 s = {0.f, 0.f, 0.f};
  const int j1 = vf_start[v + 1];
  for (int j = vf_start[v]; j < j1; ++j) {
    const int f = vf_slot[j] / 3;
    int a, b, c;
    if ((unsigned)f >= (unsigned)F || !ids3(vi, f, V, a, b, c)) continue;
    const V3 p0 = ld3(vb + 3 * a);
    const V3 cr = cross(ld3(vb + 3 * b) - p0, ld3(vb + 3 * c) - p0);
    s = s + cr / fmaxf(norm(cr), kFaceEps);
  }
  return s;
}

__global__ __launch_bounds__(256) void vert_normals_fwd_kernel(int B, int V, int F, const float* __restrict__ verts,
                                                               const int32_t* __restrict__ vi,
                                                               const int32_t* __restrict__ vf_start,
                                                               const int32_t* __restrict__ vf_slot, float eps,
                                                               float* __restrict__ vn) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * V) return;
  const int b = (int)(i / V), v = (int)(i - (size_t)b * V);
  const V3 s = vertex_normal_sum(verts + (size_t)b * V * 3, vi, vf_start, vf_slot, v, V, F);
  st3(vn + i * 3, s / fmaxf(norm(s), eps));
}

// g_vn -> g_s (the gradient of the un-normalised vertex sum), one thread per (view, vertex)
__global__ __launch_bounds__(256) void vert_normals_gs_kernel(int B, int V, int F, const float* __restrict__ verts,
                                                              const int32_t* __restrict__ vi,
                                                              const int32_t* __restrict__ vf_start,
                                                              const int32_t* __restrict__ vf_slot, float eps,
                                                              const float* __restrict__ g_vn, float* __restrict__ g_s) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * V) return;
  const int b = (int)(i / V), v = (int)(i - (size_t)b * V);
  const V3 s = vertex_normal_sum(verts + (size_t)b * V * 3, vi, vf_start, vf_slot, v, V, F);
  st3(g_s + i * 3, normalize_bwd(s, ld3(g_vn + i * 3), eps));
}

// g_s -> g_verts through the face normalisation and the cross product; ACCUMULATE adds to what g_verts holds
template <bool ACCUMULATE>
__global__ __launch_bounds__(256) void vert_normals_face_bwd_kernel(int B, int V, int F, const float* __restrict__ verts,
                                                                    const int32_t* __restrict__ vi,
                                                                    const int32_t* __restrict__ vf_start,
                                                                    const int32_t* __restrict__ vf_slot,
                                                                    const float* __restrict__ g_s,
                                                                    float* __restrict__ g_verts) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * V) return;
  const int b = (int)(i / V), v = (int)(i - (size_t)b * V);
  const float* vb = verts + (size_t)b * V * 3;
  const float* gb = g_s + (size_t)b * V * 3;
  V3 acc = {0.f, 0.f, 0.f};
  const int j1 = vf_start[v + 1];
  for (int j = vf_start[v]; j < j1; ++j) {
    const int slot = vf_slot[j], f = slot / 3, k = slot - 3 * f;
    int ia, ib, ic;
    if ((unsigned)f >= (unsigned)F || !ids3(vi, f, V, ia, ib, ic)) continue;
    const V3 p0 = ld3(vb + 3 * ia);
    const V3 e1 = ld3(vb + 3 * ib) - p0, e2 = ld3(vb + 3 * ic) - p0;
    // the unit face normal went to each of its three vertices
    const V3 g_n = ld3(gb + 3 * ia) + ld3(gb + 3 * ib) + ld3(gb + 3 * ic);
    const V3 g_c = normalize_bwd(cross(e1, e2), g_n, kFaceEps);
    const V3 g_e1 = cross(e2, g_c), g_e2 = cross(g_c, e1);   // c = e1 x e2
    if (k == 0) acc = acc - (g_e1 + g_e2);
    else if (k == 1) acc = acc + g_e1;
    else acc = acc + g_e2;
  }
  if (ACCUMULATE) acc = acc + ld3(g_verts + i * 3);
  st3(g_verts + i * 3, acc);
}

struct Texel {
  bool covered;
  int a, b, c;
  float w0, w1, w2;
};
__device__ __forceinline__ Texel load_texel(const int32_t* __restrict__ texel_rec, const int32_t* __restrict__ triples,
                                            size_t t, int T, int V) {
  const int4 r = reinterpret_cast<const int4*>(texel_rec)[t];
  Texel x;
  x.covered = (unsigned)r.x < (unsigned)T && ids3(triples, r.x, V, x.a, x.b, x.c);
  x.w0 = __int_as_float(r.y); x.w1 = __int_as_float(r.z); x.w2 = __int_as_float(r.w);
  return x;
}

// values[B,V,C] -> out[B,C,P]; the sum order of geom.py:314 (corner 0 + corner 1, then corner 2)
__global__ __launch_bounds__(256) void values_to_uv_fwd_kernel(int B, int V, int C, int P, int T,
                                                               const float* __restrict__ values,
                                                               const int32_t* __restrict__ texel_rec,
                                                               const int32_t* __restrict__ triples,
                                                               float* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)P) return;
  const Texel x = load_texel(texel_rec, triples, t, T, V);
  for (int b = 0; b < B; ++b) {
    const float* vb = values + (size_t)b * V * C;
    float* o = out + (size_t)b * C * P + t;
    for (int c = 0; c < C; ++c)
      o[(size_t)c * P] = x.covered ? vb[(size_t)x.a * C + c] * x.w0 + vb[(size_t)x.b * C + c] * x.w1 +
                                         vb[(size_t)x.c * C + c] * x.w2
                                   : 0.f;
  }
}

__device__ __forceinline__ V3 interp(const float* __restrict__ vb, const Texel& x) {
  return ld3(vb + 3 * x.a) * x.w0 + ld3(vb + 3 * x.b) * x.w1 + ld3(vb + 3 * x.c) * x.w2;
}

// verts, vn [B,V,3] -> postex, tn [B,3,P]
__global__ __launch_bounds__(256) void uvgeom_fwd_kernel(int B, int V, int P, int T, const float* __restrict__ verts,
                                                         const float* __restrict__ vn,
                                                         const int32_t* __restrict__ texel_rec,
                                                         const int32_t* __restrict__ triples, float norm_eps,
                                                         float* __restrict__ postex, float* __restrict__ tn) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)P) return;
  const Texel x = load_texel(texel_rec, triples, t, T, V);
  for (int b = 0; b < B; ++b) {
    V3 p = {0.f, 0.f, 0.f}, n = {0.f, 0.f, 0.f};
    if (x.covered) {
      p = interp(verts + (size_t)b * V * 3, x);
      n = interp(vn + (size_t)b * V * 3, x);
      n = n / fmaxf(norm(n), norm_eps);
    }
    float* po = postex + (size_t)b * 3 * P + t;
    float* no = tn + (size_t)b * 3 * P + t;
    po[0] = p.x; po[(size_t)P] = p.y; po[2 * (size_t)P] = p.z;
    no[0] = n.x; no[(size_t)P] = n.y; no[2 * (size_t)P] = n.z;
  }
}

// One 16-lane row per (view, item).  The whole wave reaches the DPP sums together: rows past the end carry zeros.
// item_sums[(row * 3 + k) * C + c] = sum over the item's texels of bary_k * g_out[b, c, texel]
__global__ __launch_bounds__(256) void values_to_uv_item_kernel(int B, int C, int P, int I,
                                                                const int32_t* __restrict__ texel_rec,
                                                                const int32_t* __restrict__ item_start,
                                                                const int32_t* __restrict__ texel_of,
                                                                const float* __restrict__ g_out,
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
  for (int c = 0; c < C; ++c) {
    const float* g = g_out + (b * C + c) * (size_t)P;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int j = s0 + lane; j < s1; j += kItemRow) {
      const int t = texel_of[j];
      if ((unsigned)t >= (unsigned)P) continue;
      const int4 r = reinterpret_cast<const int4*>(texel_rec)[t];
      const float gv = g[t];
      a0 += __int_as_float(r.y) * gv; a1 += __int_as_float(r.z) * gv; a2 += __int_as_float(r.w) * gv;
    }
    a0 = gol_row_sum_to_lane15(a0); a1 = gol_row_sum_to_lane15(a1); a2 = gol_row_sum_to_lane15(a2);
    if (valid && lane == kItemRow - 1) {
      float* o = item_sums + row * 3 * C + c;
      o[0] = a0; o[C] = a1; o[2 * C] = a2;
    }
  }
}

// item_sums[row * 18 + k * 3 + c] (positions), [row * 18 + 9 + k * 3 + c] (un-normalised normals)
__global__ __launch_bounds__(256) void uvgeom_item_kernel(int B, int V, int P, int T, int I,
                                                          const int32_t* __restrict__ texel_rec,
                                                          const int32_t* __restrict__ triples,
                                                          const int32_t* __restrict__ item_start,
                                                          const int32_t* __restrict__ item_tid,
                                                          const int32_t* __restrict__ texel_of, float norm_eps,
                                                          const float* __restrict__ vn,
                                                          const float* __restrict__ g_postex,
                                                          const float* __restrict__ g_tn,
                                                          float* __restrict__ item_sums) {
  const size_t row = (size_t)blockIdx.x * (256 / kItemRow) + (threadIdx.x / kItemRow);
  const int lane = threadIdx.x % kItemRow;
  const bool valid = row < (size_t)B * I;
  int s0 = 0, s1 = 0;
  size_t b = 0;
  V3 na = {0.f, 0.f, 0.f}, nb = na, nc = na;
  if (valid) {
    b = row / I;
    const int item = (int)(row - b * I);
    const int tid = item_tid[item];
    int ia, ib, ic;
    if ((unsigned)tid < (unsigned)T && ids3(triples, tid, V, ia, ib, ic)) {
      s0 = item_start[item]; s1 = item_start[item + 1];
      const float* vb = vn + b * V * 3;
      na = ld3(vb + 3 * ia); nb = ld3(vb + 3 * ib); nc = ld3(vb + 3 * ic);
    }
  }
  float acc[18];
#pragma unroll
  for (int q = 0; q < 18; ++q) acc[q] = 0.f;
  const float* gp = g_postex ? g_postex + b * 3 * (size_t)P : nullptr;
  const float* gt = g_tn ? g_tn + b * 3 * (size_t)P : nullptr;
  for (int j = s0 + lane; j < s1; j += kItemRow) {
    const int t = texel_of[j];
    if ((unsigned)t >= (unsigned)P) continue;
    const int4 r = reinterpret_cast<const int4*>(texel_rec)[t];
    const float w[3] = {__int_as_float(r.y), __int_as_float(r.z), __int_as_float(r.w)};
    if (gp) {
      const float g[3] = {gp[t], gp[(size_t)P + t], gp[2 * (size_t)P + t]};
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[k * 3 + c] += w[k] * g[c];
    }
    if (gt) {
      const V3 x = na * w[0] + nb * w[1] + nc * w[2];
      const V3 gx = normalize_bwd(x, V3{gt[t], gt[(size_t)P + t], gt[2 * (size_t)P + t]}, norm_eps);
      const float g[3] = {gx.x, gx.y, gx.z};
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[9 + k * 3 + c] += w[k] * g[c];
    }
  }
#pragma unroll
  for (int q = 0; q < 18; ++q) acc[q] = gol_row_sum_to_lane15(acc[q]);
  if (valid && lane == kItemRow - 1) {
    float* o = item_sums + row * 18;
#pragma unroll
    for (int q = 0; q < 18; ++q) o[q] = acc[q];
  }
}

// g_values[b, v, c] = sum over the vertex's (item, corner) slots, in slot order
__global__ __launch_bounds__(256) void values_to_uv_gather_kernel(int B, int V, int C, int I,
                                                                  const int32_t* __restrict__ vt_start,
                                                                  const int32_t* __restrict__ vt_slot,
                                                                  const float* __restrict__ item_sums,
                                                                  float* __restrict__ g_values) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * V) return;
  const size_t b = i / V;
  const int v = (int)(i - b * V);
  const int j0 = vt_start[v], j1 = vt_start[v + 1];
  const float* base = item_sums + b * I * 3 * C;
  for (int c = 0; c < C; ++c) {
    double s = 0.0;
    for (int j = j0; j < j1; ++j) {
      const int slot = vt_slot[j];
      if ((unsigned)slot < 3u * (unsigned)I) s += (double)base[(size_t)slot * C + c];
    }
    g_values[i * C + c] = (float)s;
  }
}

// g_verts[b, v] = position part; g_s[b, v] = the normal part pushed through the vertex normalisation
__global__ __launch_bounds__(256) void uvgeom_gather_kernel(int B, int V, int F, int I, const float* __restrict__ verts,
                                                            const int32_t* __restrict__ vi,
                                                            const int32_t* __restrict__ vf_start,
                                                            const int32_t* __restrict__ vf_slot,
                                                            const int32_t* __restrict__ vt_start,
                                                            const int32_t* __restrict__ vt_slot, float vn_eps,
                                                            const float* __restrict__ item_sums,
                                                            float* __restrict__ g_s, float* __restrict__ g_verts) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * V) return;
  const size_t b = i / V;
  const int v = (int)(i - b * V);
  const float* base = item_sums + b * I * 18;
  double p[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
  const int j1 = vt_start[v + 1];
  for (int j = vt_start[v]; j < j1; ++j) {
    const int slot = vt_slot[j];
    if ((unsigned)slot >= 3u * (unsigned)I) continue;
    const int item = slot / 3, k = slot - 3 * item;
    const float* o = base + (size_t)item * 18 + k * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) { p[c] += (double)o[c]; n[c] += (double)o[9 + c]; }
  }
  st3(g_verts + i * 3, V3{(float)p[0], (float)p[1], (float)p[2]});
  const V3 s = vertex_normal_sum(verts + b * V * 3, vi, vf_start, vf_slot, v, V, F);
  st3(g_s + i * 3, normalize_bwd(s, V3{(float)n[0], (float)n[1], (float)n[2]}, vn_eps));
}

inline bool fits_int(long long n) { return n > 0 && n < (1ll << 31); }

}  // namespace

extern "C" int gol_vert_normals_fwd(int B, int V, int F, const float* verts, const int32_t* vi, const int32_t* vf_start,
                                    const int32_t* vf_slot, float eps, float* vn, void* stream) {
  GOL_REQUIRE(B > 0 && V > 0 && F >= 0, "B, V must be positive");
  GOL_REQUIRE(verts && vi && vf_start && vf_slot && vn, "null pointer");
  GOL_REQUIRE(fits_int((long long)B * V * 3), "B * V * 3 must fit 31 bits");
  hipLaunchKernelGGL(vert_normals_fwd_kernel, dim3(gol_cdiv((long long)B * V, 256)), dim3(256), 0, (hipStream_t)stream, B, V,
                     F, verts, vi, vf_start, vf_slot, eps, vn);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_vert_normals_bwd(int B, int V, int F, const float* verts, const int32_t* vi, const int32_t* vf_start,
                                    const int32_t* vf_slot, float eps, const float* g_vn, float* g_s, float* g_verts,
                                    void* stream) {
  GOL_REQUIRE(B > 0 && V > 0 && F >= 0, "B, V must be positive");
  GOL_REQUIRE(verts && vi && vf_start && vf_slot && g_vn && g_s && g_verts, "null pointer");
  GOL_REQUIRE(fits_int((long long)B * V * 3), "B * V * 3 must fit 31 bits");
  const dim3 grid(gol_cdiv((long long)B * V, 256));
  hipLaunchKernelGGL(vert_normals_gs_kernel, grid, dim3(256), 0, (hipStream_t)stream, B, V, F, verts, vi, vf_start, vf_slot,
                     eps, g_vn, g_s);
  GOL_CHECK_LAUNCH();
  hipLaunchKernelGGL(vert_normals_face_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, B, V, F, verts, vi,
                     vf_start, vf_slot, (const float*)g_s, g_verts);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_values_to_uv_fwd(int B, int V, int C, int S, int T, const float* values, const int32_t* texel_rec,
                                    const int32_t* triples, float* out, void* stream) {
  GOL_REQUIRE(B > 0 && V > 0 && C > 0 && S > 0 && T >= 0, "B, V, C, S must be positive");
  GOL_REQUIRE(values && texel_rec && out && (triples || T == 0), "null pointer");
  GOL_REQUIRE(fits_int((long long)S * S) && fits_int((long long)V * C), "S * S and V * C must fit 31 bits");
  hipLaunchKernelGGL(values_to_uv_fwd_kernel, dim3(gol_cdiv((long long)S * S, 256)), dim3(256), 0, (hipStream_t)stream, B, V,
                     C, S * S, T, values, texel_rec, triples, out);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_values_to_uv_bwd(int B, int V, int C, int S, int T, int I, const int32_t* texel_rec,
                                    const int32_t* item_start, const int32_t* texel_of, const int32_t* vt_start,
                                    const int32_t* vt_slot, const float* g_out, float* item_sums, float* g_values,
                                    void* stream) {
  GOL_REQUIRE(B > 0 && V > 0 && C > 0 && S > 0 && T >= 0 && I >= 0, "B, V, C, S must be positive");
  GOL_REQUIRE(texel_rec && vt_start && g_out && g_values, "null pointer");
  GOL_REQUIRE(I == 0 || (item_start && texel_of && vt_slot && item_sums), "null pointer");
  GOL_REQUIRE(fits_int((long long)S * S) && fits_int((long long)V * C) && (long long)I * 3 * C < (1ll << 31),
              "S * S, V * C and I * 3 * C must fit 31 bits");
  if (I > 0) {
    hipLaunchKernelGGL(values_to_uv_item_kernel, dim3(gol_cdiv((long long)B * I, 256 / kItemRow)), dim3(256), 0,
                       (hipStream_t)stream, B, C, S * S, I, texel_rec, item_start, texel_of, g_out, item_sums);
    GOL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(values_to_uv_gather_kernel, dim3(gol_cdiv((long long)B * V, 256)), dim3(256), 0, (hipStream_t)stream, B,
                     V, C, I, vt_start, vt_slot, (const float*)item_sums, g_values);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_uvgeom_fwd(int B, int V, int F, int S, int T, const float* verts, const int32_t* vi,
                              const int32_t* vf_start, const int32_t* vf_slot, const int32_t* texel_rec,
                              const int32_t* triples, float vn_eps, float norm_eps, float* vn, float* postex, float* tn,
                              void* stream) {
  GOL_REQUIRE(S > 0 && T >= 0, "S must be positive");
  GOL_REQUIRE(texel_rec && postex && tn && (triples || T == 0), "null pointer");
  GOL_REQUIRE(fits_int((long long)S * S), "S * S must fit 31 bits");
  const int rc = gol_vert_normals_fwd(B, V, F, verts, vi, vf_start, vf_slot, vn_eps, vn, stream);
  if (rc != GOL_OK) return rc;
  hipLaunchKernelGGL(uvgeom_fwd_kernel, dim3(gol_cdiv((long long)S * S, 256)), dim3(256), 0, (hipStream_t)stream, B, V,
                     S * S, T, verts, (const float*)vn, texel_rec, triples, norm_eps, postex, tn);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_uvgeom_bwd(int B, int V, int F, int S, int T, int I, const float* verts, const int32_t* vi,
                              const int32_t* vf_start, const int32_t* vf_slot, const int32_t* texel_rec,
                              const int32_t* triples, const int32_t* item_start, const int32_t* item_tid,
                              const int32_t* texel_of, const int32_t* vt_start, const int32_t* vt_slot, float vn_eps,
                              float norm_eps, const float* vn, const float* g_postex, const float* g_tn, float* item_sums,
                              float* g_s, float* g_verts, void* stream) {
  GOL_REQUIRE(B > 0 && V > 0 && F >= 0 && S > 0 && T >= 0 && I >= 0, "B, V, S must be positive");
  GOL_REQUIRE(verts && vi && vf_start && vf_slot && texel_rec && vt_start && vn && g_s && g_verts, "null pointer");
  GOL_REQUIRE(I == 0 || (triples && item_start && item_tid && texel_of && vt_slot && item_sums), "null pointer");
  GOL_REQUIRE(fits_int((long long)S * S) && fits_int((long long)B * V * 3) && (long long)I * 18 < (1ll << 31),
              "S * S, B * V * 3 and I * 18 must fit 31 bits");
  if (I > 0) {
    hipLaunchKernelGGL(uvgeom_item_kernel, dim3(gol_cdiv((long long)B * I, 256 / kItemRow)), dim3(256), 0,
                       (hipStream_t)stream, B, V, S * S, T, I, texel_rec, triples, item_start, item_tid, texel_of, norm_eps,
                       vn, g_postex, g_tn, item_sums);
    GOL_CHECK_LAUNCH();
  }
  const dim3 grid(gol_cdiv((long long)B * V, 256));
  hipLaunchKernelGGL(uvgeom_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, B, V, F, I, verts, vi, vf_start, vf_slot,
                     vt_start, vt_slot, vn_eps, (const float*)item_sums, g_s, g_verts);
  GOL_CHECK_LAUNCH();
  hipLaunchKernelGGL(vert_normals_face_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, B, V, F, verts, vi,
                     vf_start, vf_slot, (const float*)g_s, g_verts);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
