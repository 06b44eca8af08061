// lbs.hip -- skeleton solve and linear blend skinning with gradients, gfx950 (wave64).
//
// Replaces the reference's per-frame PyTorch of ca_code/utils/lbs.py: ParameterTransform.forward (:39-46),
// solve_skeleton_state (:340-385, a Python loop over the joints with one device-to-host read of the parent index per joint
// and about a dozen small ATen kernels per joint), states_to_matrix (:388-429), LinearBlendSkinning.skinning (:226-254, a
// gathered [B,V,8,3,4] matrix tensor) and the two elementwise lines of LBSModule.pose (:725-731).  The skeleton is constant
// for a model's lifetime; goliath_amd/lbs.py:Skeleton packs it once:
//   parents[J]                          int32, -1 = root; a parent's index is smaller than its child's
//   level_start[L+1], level_joints[J]   the joints by tree level (roots = level 0), ascending inside a level
//   child_start[J+1], child_slot[J-R]   joint -> children, ascending
//   bind_inv[J,8]                       double: bt, br, bs of states_to_matrix (:392-394)
//   transform[7J,P], transform_t[P,7J]  the parameter transform in both layouts (either direction reads it coalesced)
//   jv_start[J+1], jv_slot[E]           joint -> (vertex, slot) of its NON-ZERO weights, slot = vertex * K + k, ascending
//   item_start[I+1], ji_start[J+1]      every joint's run cut into items of at most 64 entries; a joint's item range
// Kernels:
//   skeleton fwd   one workgroup per view.  Pose vector in LDS; one lane per row of the parameter transform; then the
//                  chain level by level: lanes are the joints of a level, parent states are read from LDS, one barrier
//                  per level.  All of it in double (B * J lanes of work): states and matrices are the float roundings of
//                  the float64 result.
//   skin fwd       one lane per (view, vertex); the view's matrices in LDS; zero-weight slots are skipped.
//   skin bwd       vertex pass (one lane per (view, vertex): sum_k w_k R_k^T g); item pass (one 16-lane row per (view,
//                  item): w g (x) [v,1], summed over the row by DPP moves); joint pass (one lane per (view, joint, entry):
//                  the joint's items in order).
//   skeleton bwd   one workgroup per view: the forward chain again, then the levels in reverse -- every joint gathers its
//                  children's contributions through the children CSR (local transforms kept in LDS) --, the local
//                  transforms' own derivative, and the transposed
//                  parameter transform with one lane per parameter.
// Every sum has a fixed order and there are no atomics: outputs and gradients are bitwise reproducible.
#include "gol_common.h"
#include "gol_lbs_math.h"

namespace {

using namespace gol_lbs;

constexpr int kBlock = 256;
constexpr int kItemRow = 16;             // lanes per item (one DPP row)
constexpr size_t kMaxLds = 64 * 1024;    // dynamic LDS a launch may ask for without an attribute

__device__ __forceinline__ State load_state(const double* __restrict__ s) {
  return {{s[0], s[1], s[2]}, {s[3], s[4], s[5], s[6]}, s[7]};
}
__device__ __forceinline__ void store_state(double* __restrict__ s, const State& x) {
  s[0] = x.t.x; s[1] = x.t.y; s[2] = x.t.z; s[3] = x.q.x; s[4] = x.q.y; s[5] = x.q.z; s[6] = x.q.w; s[7] = x.s;
}
__device__ __forceinline__ State add(const State& a, const State& b) { return {a.t + b.t, a.q + b.q, a.s + b.s}; }

// what the forward chain reads (both skeleton kernels)
struct ChainArgs {
  int J, NP, NS, L, scales_stride;
  const float *poses, *scales, *transform_t, *transform_offsets, *joint_offset, *joint_rotation;
  const int32_t *parents, *level_start, *level_joints;
};

__device__ __forceinline__ Q4 pre_rotation(const ChainArgs& a, int j) {
  const float* r = a.joint_rotation + 4 * j;
  return {r[0], r[1], r[2], r[3]};
}

// pose -> LDS, the parameter transform (one lane per row, p ascending), the chain by levels.  Leaves S[J,8] and p7[7J] in
// LDS behind a barrier.  `emit(j, state, lt, lr, ls)` runs once per joint.  The only place of the forward with
// trigonometry: one sincos body (gol_lbs_math.h:half_trig).
template <typename Emit>
__device__ __forceinline__ void solve_chain(const ChainArgs& a, int b, double* __restrict__ S, double* __restrict__ p7,
                                            float* __restrict__ pose, Emit emit) {
  const int tid = threadIdx.x, J = a.J, P = a.NP + a.NS, R = 7 * J;
  for (int p = tid; p < P; p += kBlock)
    pose[p] = p < a.NP ? a.poses[(size_t)b * a.NP + p] : a.scales[(size_t)b * a.scales_stride + (p - a.NP)];
  __syncthreads();
  for (int r = tid; r < R; r += kBlock) {
    double acc = 0.0;
    for (int p = 0; p < P; ++p) acc += (double)a.transform_t[(size_t)p * R + r] * (double)pose[p];
    p7[r] = acc + (double)a.transform_offsets[r];
  }
  __syncthreads();
  for (int l = 0; l < a.L; ++l) {
    const int i1 = min(a.level_start[l + 1], J);
    for (int i = max(a.level_start[l], 0) + tid; i < i1; i += kBlock) {
      const int j = a.level_joints[i];
      if ((unsigned)j >= (unsigned)J) continue;
      D3 lt; Q4 lr; double ls;
      const float* o = a.joint_offset + 3 * j;
      local_transform(p7 + 7 * j, D3{o[0], o[1], o[2]}, pre_rotation(a, j), lt, lr, ls);
      const int par = a.parents[j];
      const State st = (unsigned)par < (unsigned)J ? compose(load_state(S + 8 * par), lt, lr, ls) : State{lt, lr, ls};
      store_state(S + 8 * j, st);
      emit(j, st, lt, lr, ls);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void lbs_skeleton_fwd_kernel(ChainArgs a, const double* __restrict__ bind_inv,
                                                                  float* __restrict__ states, float* __restrict__ mats) {
  extern __shared__ double lds[];
  double* S = lds;
  double* p7 = S + 8 * a.J;
  float* pose = reinterpret_cast<float*>(p7 + 7 * a.J);
  const int b = blockIdx.x;
  solve_chain(a, b, S, p7, pose, [&](int j, const State& st, D3, Q4, double) {
    const size_t bj = (size_t)b * a.J + j;
    if (states) {
      float4* o = reinterpret_cast<float4*>(states + bj * 8);
      o[0] = make_float4((float)st.t.x, (float)st.t.y, (float)st.t.z, (float)st.q.x);
      o[1] = make_float4((float)st.q.y, (float)st.q.z, (float)st.q.w, (float)st.s);
    }
    if (mats) {
      double m[12];
      state_to_matrix(st, load_state(bind_inv + 8 * j), m);
      float4* o = reinterpret_cast<float4*>(mats + bj * 12);
#pragma unroll
      for (int r = 0; r < 3; ++r)
        o[r] = make_float4((float)m[4 * r], (float)m[4 * r + 1], (float)m[4 * r + 2], (float)m[4 * r + 3]);
    }
  });
}

__global__ __launch_bounds__(kBlock) void lbs_skeleton_bwd_kernel(ChainArgs a, const double* __restrict__ bind_inv,
                                                                  const float* __restrict__ transform,
                                                                  const int32_t* __restrict__ child_start,
                                                                  const int32_t* __restrict__ child_slot,
                                                                  const float* __restrict__ g_states,
                                                                  const float* __restrict__ g_mats,
                                                                  float* __restrict__ g_poses,
                                                                  float* __restrict__ g_scales) {
  extern __shared__ double lds[];
  const int J = a.J, P = a.NP + a.NS, tid = threadIdx.x, b = blockIdx.x;
  double* S = lds;            // states
  double* G = S + 8 * J;      // their gradients
  double* Lc = G + 8 * J;     // local transforms (lt, lr, ls), kept so that the reverse passes need no trigonometry
  double* p7 = Lc + 8 * J;
  float* pose = reinterpret_cast<float*>(p7 + 7 * J);
  solve_chain(a, b, S, p7, pose,
              [&](int j, const State&, D3 lt, Q4 lr, double ls) { store_state(Lc + 8 * j, State{lt, lr, ls}); });
  // the gradient every joint's state receives from the outputs
  for (int j = tid; j < J; j += kBlock) {
    const size_t bj = (size_t)b * J + j;
    State g = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, 0.0};
    if (g_states) {
      const float* s = g_states + bj * 8;
      g = {{s[0], s[1], s[2]}, {s[3], s[4], s[5], s[6]}, s[7]};
    }
    if (g_mats) {
      double gm[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) gm[q] = (double)g_mats[bj * 12 + q];
      g = add(g, state_to_matrix_bwd(load_state(S + 8 * j), load_state(bind_inv + 8 * j), gm));
    }
    store_state(G + 8 * j, g);
  }
  __syncthreads();
  // levels in reverse: a joint adds what its children (one level down, final by now) hand up, in child order
  for (int l = a.L - 2; l >= 0; --l) {
    const int i1 = min(a.level_start[l + 1], J);
    for (int i = max(a.level_start[l], 0) + tid; i < i1; i += kBlock) {
      const int j = a.level_joints[i];
      if ((unsigned)j >= (unsigned)J) continue;
      const State sj = load_state(S + 8 * j);
      State g = load_state(G + 8 * j);
      const int c1 = min(child_start[j + 1], J);
      for (int ci = max(child_start[j], 0); ci < c1; ++ci) {
        const int c = child_slot[ci];
        if ((unsigned)c >= (unsigned)J) continue;
        const State lc = load_state(Lc + 8 * c);
        D3 glt; Q4 glr; double gls;
        State gp;
        compose_bwd(sj, lc.t, lc.q, lc.s, load_state(G + 8 * c), gp, glt, glr, gls);
        g = add(g, gp);
      }
      store_state(G + 8 * j, g);
    }
    __syncthreads();
  }
  // local transforms -> the gradient of the 7 parameters of every joint (written over p7: a lane touches its own 7 only)
  for (int j = tid; j < J; j += kBlock) {
    const State lc = load_state(Lc + 8 * j), g = load_state(G + 8 * j);
    D3 glt; Q4 glr; double gls;
    const int par = a.parents[j];
    if ((unsigned)par < (unsigned)J) {
      State gp;
      compose_bwd(load_state(S + 8 * par), lc.t, lc.q, lc.s, g, gp, glt, glr, gls);
    } else {
      glt = g.t; glr = g.q; gls = g.s;
    }
    double gp7[7];
    local_transform_bwd(p7 + 7 * j, pre_rotation(a, j), lc.s, glt, glr, gls, gp7);
#pragma unroll
    for (int q = 0; q < 7; ++q) p7[7 * j + q] = gp7[q];
  }
  __syncthreads();
  // the transposed parameter transform: lanes are parameters, rows ascending
  for (int p = tid; p < P; p += kBlock) {
    double acc = 0.0;
    for (int r = 0; r < 7 * J; ++r) acc += (double)transform[(size_t)r * P + p] * p7[r];
    if (p < a.NP) {
      if (g_poses) g_poses[(size_t)b * a.NP + p] = (float)acc;
    } else if (g_scales) {
      g_scales[(size_t)b * a.NS + (p - a.NP)] = (float)acc;
    }
  }
}

// the vertex the skinning sees: verts_unposed (or the rest mesh, shared by the views) + template
__device__ __forceinline__ D3 skin_input(const float* __restrict__ verts, int verts_batched,
                                         const float* __restrict__ template_verts, int b, int v, int V) {
  const float* p = verts + ((size_t)(verts_batched ? b : 0) * V + v) * 3;
  D3 x = {p[0], p[1], p[2]};
  if (template_verts) x = x + D3{template_verts[3 * v], template_verts[3 * v + 1], template_verts[3 * v + 2]};
  return x;
}
__device__ __forceinline__ D3 scaled(D3 x, const float* __restrict__ global_scaling) {
  if (global_scaling) x = {x.x * (double)global_scaling[0], x.y * (double)global_scaling[1], x.z * (double)global_scaling[2]};
  return x;
}

// one influence of a vertex: BWD = false: acc += w M [x,1];  BWD = true: acc += w R^T x
template <bool BWD>
__device__ __forceinline__ void skin_slot(const float* __restrict__ M, int J, int j, float w, D3 x, D3& acc) {
  if (w == 0.f || (unsigned)j >= (unsigned)J) return;   // a padded slot contributes exactly nothing
  const float* m = M + 12 * j;
  D3 t;
  if (BWD)
    t = {(double)m[0] * x.x + (double)m[4] * x.y + (double)m[8] * x.z,
         (double)m[1] * x.x + (double)m[5] * x.y + (double)m[9] * x.z,
         (double)m[2] * x.x + (double)m[6] * x.y + (double)m[10] * x.z};
  else
    t = {(double)m[0] * x.x + (double)m[1] * x.y + (double)m[2] * x.z + (double)m[3],
         (double)m[4] * x.x + (double)m[5] * x.y + (double)m[6] * x.z + (double)m[7],
         (double)m[8] * x.x + (double)m[9] * x.y + (double)m[10] * x.z + (double)m[11]};
  acc = acc + t * (double)w;
}

// BWD = false: out[b,v] = (sum_k w_k M_k [x,1]) * global_scaling;  BWD = true: out[b,v] = sum_k w_k R_k^T (g * scaling).
// The xyz rows of a workgroup's 256 vertices go through LDS, so that global loads and stores are consecutive floats
// across the lanes; weights and indices are read 16 bytes at a time when K is a multiple of 4.
template <bool BWD>
__global__ __launch_bounds__(kBlock) void lbs_skin_vertex_kernel(int V, int J, int K, const float* __restrict__ mats,
                                                                 const float* __restrict__ verts, int verts_batched,
                                                                 const float* __restrict__ template_verts,
                                                                 const float* __restrict__ global_scaling,
                                                                 const int32_t* __restrict__ skin_indices,
                                                                 const float* __restrict__ skin_weights,
                                                                 const float* __restrict__ g_out,
                                                                 float* __restrict__ out) {
  extern __shared__ float M[];
  __shared__ float xyz[3 * kBlock], tpl[3 * kBlock];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int v0 = blockIdx.x * kBlock, n3 = 3 * min(kBlock, V - v0);
  for (int i = tid; i < J * 12; i += kBlock) M[i] = mats[(size_t)b * J * 12 + i];
  const float* src = BWD ? g_out + ((size_t)b * V + v0) * 3 : verts + ((size_t)(verts_batched ? b : 0) * V + v0) * 3;
  const bool add_template = !BWD && template_verts;
  for (int i = tid; i < n3; i += kBlock) {
    xyz[i] = src[i];
    if (add_template) tpl[i] = template_verts[(size_t)v0 * 3 + i];
  }
  __syncthreads();
  const int v = v0 + tid;
  D3 acc = {0.0, 0.0, 0.0};
  if (v < V) {
    D3 x = {xyz[3 * tid], xyz[3 * tid + 1], xyz[3 * tid + 2]};
    if (add_template) x = x + D3{tpl[3 * tid], tpl[3 * tid + 1], tpl[3 * tid + 2]};
    if (BWD) x = scaled(x, global_scaling);
    if (K % 4 == 0) {
      const float4* w4 = reinterpret_cast<const float4*>(skin_weights + (size_t)v * K);
      const int4* j4 = reinterpret_cast<const int4*>(skin_indices + (size_t)v * K);
      for (int k = 0; k < K / 4; ++k) {
        const float4 w = w4[k];
        const int4 j = j4[k];
        skin_slot<BWD>(M, J, j.x, w.x, x, acc);
        skin_slot<BWD>(M, J, j.y, w.y, x, acc);
        skin_slot<BWD>(M, J, j.z, w.z, x, acc);
        skin_slot<BWD>(M, J, j.w, w.w, x, acc);
      }
    } else {
      for (int k = 0; k < K; ++k)
        skin_slot<BWD>(M, J, skin_indices[(size_t)v * K + k], skin_weights[(size_t)v * K + k], x, acc);
    }
    if (!BWD) acc = scaled(acc, global_scaling);
  }
  __syncthreads();   // every lane has read its row of xyz
  if (v < V) { xyz[3 * tid] = (float)acc.x; xyz[3 * tid + 1] = (float)acc.y; xyz[3 * tid + 2] = (float)acc.z; }
  __syncthreads();
  float* dst = out + ((size_t)b * V + v0) * 3;
  for (int i = tid; i < n3; i += kBlock) dst[i] = xyz[i];
}

// sum over the 16 lanes of a DPP row, valid in lane 15 of the row: the two halves of the double move separately (lanes
// without a source read 0.0), the add is a plain v_add_f64
template <int CTRL>
__device__ __forceinline__ double row_shifted(double v) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)bits, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(bits >> 32), CTRL, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double row_sum_to_lane15(double v) {
  v += row_shifted<0x111>(v);   // row_shr:1
  v += row_shifted<0x112>(v);   // row_shr:2
  v += row_shifted<0x114>(v);   // row_shr:4
  v += row_shifted<0x118>(v);   // row_shr:8
  return v;
}

// One 16-lane row per (view, item); the whole wave reaches the row sums together: rows past the end carry zeros.
// item_sums[row * 12 + 4 r + c] = sum over the item's entries of w * (g * scaling)[r] * [x,1][c]
__global__ __launch_bounds__(kBlock) void lbs_skin_item_kernel(int B, int V, int K, int E, int I,
                                                               const float* __restrict__ verts, int verts_batched,
                                                               const float* __restrict__ template_verts,
                                                               const float* __restrict__ global_scaling,
                                                               const float* __restrict__ skin_weights,
                                                               const int32_t* __restrict__ item_start,
                                                               const int32_t* __restrict__ jv_slot,
                                                               const float* __restrict__ g_out,
                                                               double* __restrict__ item_sums) {
  const size_t row = (size_t)blockIdx.x * (kBlock / kItemRow) + (threadIdx.x / kItemRow);
  const int lane = threadIdx.x % kItemRow;
  const bool valid = row < (size_t)B * I;
  int e0 = 0, e1 = 0, b = 0;
  if (valid) {
    b = (int)(row / I);
    const int item = (int)(row - (size_t)b * I);
    e0 = max(item_start[item], 0);
    e1 = min(item_start[item + 1], E);
  }
  double acc[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) acc[q] = 0.0;
  for (int e = e0 + lane; e < e1; e += kItemRow) {
    const int slot = jv_slot[e];
    if ((unsigned)slot >= (unsigned)V * (unsigned)K) continue;
    const int v = slot / K;
    const double w = (double)skin_weights[slot];
    const float* gp = g_out + ((size_t)b * V + v) * 3;
    const D3 g = scaled(D3{gp[0], gp[1], gp[2]}, global_scaling) * w;
    const D3 x = skin_input(verts, verts_batched, template_verts, b, v, V);
    const double gr[3] = {g.x, g.y, g.z}, xc[4] = {x.x, x.y, x.z, 1.0};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[4 * r + c] += gr[r] * xc[c];
  }
#pragma unroll
  for (int q = 0; q < 12; ++q) acc[q] = row_sum_to_lane15(acc[q]);
  if (valid && lane == kItemRow - 1) {
    double* o = item_sums + row * 12;
#pragma unroll
    for (int q = 0; q < 12; ++q) o[q] = acc[q];
  }
}

// g_mats[b, j, q] = the sum over the joint's items, in item order
__global__ __launch_bounds__(kBlock) void lbs_skin_joint_kernel(int B, int J, int I, const int32_t* __restrict__ ji_start,
                                                                const double* __restrict__ item_sums,
                                                                float* __restrict__ g_mats) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (size_t)B * J * 12) return;
  const int q = (int)(i % 12);
  const size_t bj = i / 12;
  const int b = (int)(bj / J), j = (int)(bj - (size_t)b * J);
  const int i0 = max(ji_start[j], 0), i1 = min(ji_start[j + 1], I);
  const double* base = item_sums + (size_t)b * I * 12 + q;
  double s = 0.0;
  for (int it = i0; it < i1; ++it) s += base[(size_t)it * 12];
  g_mats[i] = (float)s;
}

inline bool fits_int(long long n) { return n > 0 && n < (1ll << 31); }

}  // namespace

#define GOL_LBS_CHAIN_ARGS                                                                                         \
  ChainArgs a = {J, NP, NS, L, scales_stride, poses, scales, transform_t, transform_offsets, joint_offset, joint_rotation, \
                 parents, level_start, level_joints}

extern "C" int gol_lbs_skeleton_fwd(int B, int J, int NP, int NS, int L, const float* poses, const float* scales,
                                    int scales_stride, const float* transform_t, const float* transform_offsets,
                                    const float* joint_offset, const float* joint_rotation, const double* bind_inv,
                                    const int32_t* parents, const int32_t* level_start, const int32_t* level_joints,
                                    float* states, float* mats, void* stream) {
  GOL_REQUIRE(B > 0 && J > 0 && NP >= 0 && NS >= 0 && NP + NS > 0 && L > 0 && L <= J, "B, J, NP + NS, L must be positive");
  GOL_REQUIRE(scales_stride == 0 || scales_stride == NS, "scales_stride must be 0 (one row for all views) or NS");
  GOL_REQUIRE((poses || NP == 0) && (scales || NS == 0) && transform_t && transform_offsets && joint_offset &&
                  joint_rotation && bind_inv && parents && level_start && level_joints && (states || mats),
              "null pointer");
  const size_t lds = (size_t)15 * J * sizeof(double) + (size_t)(NP + NS) * sizeof(float);
  GOL_REQUIRE(lds <= kMaxLds && fits_int((long long)B * J * 12), "the skeleton does not fit the LDS (15 J doubles + P floats)");
  GOL_LBS_CHAIN_ARGS;
  hipLaunchKernelGGL(lbs_skeleton_fwd_kernel, dim3(B), dim3(kBlock), lds, (hipStream_t)stream, a, bind_inv, states, mats);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_lbs_skeleton_bwd(int B, int J, int NP, int NS, int L, const float* poses, const float* scales,
                                    int scales_stride, const float* transform, const float* transform_t,
                                    const float* transform_offsets, const float* joint_offset,
                                    const float* joint_rotation, const double* bind_inv, const int32_t* parents,
                                    const int32_t* level_start, const int32_t* level_joints, const int32_t* child_start,
                                    const int32_t* child_slot, const float* g_states, const float* g_mats,
                                    float* g_poses, float* g_scales, void* stream) {
  GOL_REQUIRE(B > 0 && J > 0 && NP >= 0 && NS >= 0 && NP + NS > 0 && L > 0 && L <= J, "B, J, NP + NS, L must be positive");
  GOL_REQUIRE(scales_stride == 0 || scales_stride == NS, "scales_stride must be 0 (one row for all views) or NS");
  GOL_REQUIRE((poses || NP == 0) && (scales || NS == 0) && transform && transform_t && transform_offsets && joint_offset &&
                  joint_rotation && bind_inv && parents && level_start && level_joints && child_start &&
                  (child_slot || L == 1) && (g_poses || g_scales),
              "null pointer");
  const size_t lds = (size_t)31 * J * sizeof(double) + (size_t)(NP + NS) * sizeof(float);
  GOL_REQUIRE(lds <= kMaxLds && fits_int((long long)B * J * 12), "the skeleton does not fit the LDS (31 J doubles + P floats)");
  GOL_LBS_CHAIN_ARGS;
  hipLaunchKernelGGL(lbs_skeleton_bwd_kernel, dim3(B), dim3(kBlock), lds, (hipStream_t)stream, a, bind_inv, transform,
                     child_start, child_slot, g_states, g_mats, g_poses, g_scales);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_lbs_skin_fwd(int B, int V, int J, int K, const float* mats, const float* verts, int verts_batched,
                                const float* template_verts, const float* global_scaling, const int32_t* skin_indices,
                                const float* skin_weights, float* out, void* stream) {
  GOL_REQUIRE(B > 0 && V > 0 && J > 0 && K > 0, "B, V, J, K must be positive");
  GOL_REQUIRE(B <= 65535, "B must fit a grid dimension");
  GOL_REQUIRE(mats && verts && skin_indices && skin_weights && out, "null pointer");
  GOL_REQUIRE((size_t)J * 12 * sizeof(float) + 6 * kBlock * sizeof(float) <= kMaxLds, "J * 12 floats must fit the LDS");
  GOL_REQUIRE(fits_int((long long)B * V * 3) && fits_int((long long)V * K), "B * V * 3 and V * K must fit 31 bits");
  hipLaunchKernelGGL(lbs_skin_vertex_kernel<false>, dim3(gol_cdiv(V, kBlock), B), dim3(kBlock), (size_t)J * 12 * sizeof(float),
                     (hipStream_t)stream, V, J, K, mats, verts, verts_batched, template_verts, global_scaling, skin_indices,
                     skin_weights, (const float*)nullptr, out);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_lbs_skin_bwd(int B, int V, int J, int K, int E, int I, const float* mats, const float* verts,
                                int verts_batched, const float* template_verts, const float* global_scaling,
                                const int32_t* skin_indices, const float* skin_weights, const int32_t* item_start,
                                const int32_t* jv_slot, const int32_t* ji_start, const float* g_out, double* item_sums,
                                float* g_verts, float* g_mats, void* stream) {
  GOL_REQUIRE(B > 0 && V > 0 && J > 0 && K > 0, "B, V, J, K must be positive");
  GOL_REQUIRE(E >= 0 && I >= 0, "E and I must not be negative");
  GOL_REQUIRE(B <= 65535, "B must fit a grid dimension");
  GOL_REQUIRE(mats && verts && skin_indices && skin_weights && g_out && (g_verts || g_mats), "null pointer");
  GOL_REQUIRE(!g_mats || (ji_start && (I == 0 || (item_start && jv_slot && item_sums))), "null pointer");
  GOL_REQUIRE((size_t)J * 12 * sizeof(float) + 6 * kBlock * sizeof(float) <= kMaxLds, "J * 12 floats must fit the LDS");
  GOL_REQUIRE(fits_int((long long)B * V * 3) && fits_int((long long)V * K) && fits_int((long long)B * J * 12) &&
                  (long long)B * I * 12 < (1ll << 31),
              "B * V * 3, V * K, B * J * 12 and B * I * 12 must fit 31 bits");
  if (g_verts) {
    hipLaunchKernelGGL(lbs_skin_vertex_kernel<true>, dim3(gol_cdiv(V, kBlock), B), dim3(kBlock),
                       (size_t)J * 12 * sizeof(float), (hipStream_t)stream, V, J, K, mats, verts, verts_batched,
                       template_verts, global_scaling, skin_indices, skin_weights, g_out, g_verts);
    GOL_CHECK_LAUNCH();
  }
  if (g_mats) {
    if (I > 0) {
      hipLaunchKernelGGL(lbs_skin_item_kernel, dim3(gol_cdiv((long long)B * I, kBlock / kItemRow)), dim3(kBlock), 0,
                         (hipStream_t)stream, B, V, K, E, I, verts, verts_batched, template_verts, global_scaling,
                         skin_weights, item_start, jv_slot, g_out, item_sums);
      GOL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(lbs_skin_joint_kernel, dim3(gol_cdiv((long long)B * J * 12, kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, B, J, I, ji_start, (const double*)item_sums, g_mats);
    GOL_CHECK_LAUNCH();
  }
  return GOL_OK;
}
