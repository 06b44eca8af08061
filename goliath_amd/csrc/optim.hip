// optim.hip -- the tail of a training iteration as three streaming passes: gradient scrub, global-norm clip and the
// Adam / AdamW step over every parameter tensor at once (gol_optim_*, include/goliath_hip.h).
//
// Work is dealt by a chunk table: workgroup c handles elements [chunk_off[c], chunk_off[c] + kChunk) of segment
// chunk_seg[c], a segment being one parameter tensor that has a gradient.  kChunk = 4096 floats = 256 lanes x 4 float4:
// every lane of a workgroup issues its 16-byte loads up front (4 per array, 16 in the Adam pass = 256 B per lane), so a
// CU holds well over the ~50 KB in flight that the copy ceiling needs (6.3 TB/s x ~2 us / 256 CUs) at any occupancy the
// register count leaves.  A segment whose pointers are not all 16-byte aligned (a gradient that is a view into a
// communication bucket) takes the scalar path; a tensor's last 1-3 elements are handled by three lanes.
// No atomics: every sum has a fixed order (lane, then gol_block_sum of gol_stream.h: DPP ladder over the wave, LDS over the
// waves), so the norm, the coefficient and the step are bitwise reproducible.
#include "gol_stream.h"

namespace {

using namespace gol_stream;   // f4 / gfloat / gf4 / global_floats, kBlock, kChunk, kVecIters, chunk_elems

constexpr int kFinalBlock = 1024;
constexpr int kCoef = 8;                         // floats per segment written by optim_prepare_kernel

enum { kScrub = GOL_OPTIM_SCRUB, kClip = GOL_OPTIM_CLIP, kWriteBack = GOL_OPTIM_WRITE_BACK, kAllFlags = 7 };

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

struct Chunk {
  int seg;
  int n;          // elements of this chunk, 1..kChunk (0: nothing to do)
  int64_t off;
};

__device__ __forceinline__ Chunk chunk_of(const int32_t* chunk_seg, const int64_t* chunk_off, const int64_t* seg_numel,
                                          int n_seg) {
  Chunk c;
  c.seg = chunk_seg[blockIdx.x];
  c.off = chunk_off[blockIdx.x];
  c.n = 0;
  if (c.seg >= 0 && c.seg < n_seg && c.off >= 0) {
    const int64_t rem = seg_numel[c.seg] - c.off;
    c.n = chunk_elems(rem > 0 ? rem : 0);
  }
  return c;
}

__device__ __forceinline__ void stat_add(float x, double& sq, double& bad) {
  if (finite_f(x)) sq += (double)x * (double)x;
  else bad += 1.0;
}

__global__ __launch_bounds__(kBlock) void optim_grad_stats_kernel(int n_seg, const int32_t* __restrict__ chunk_seg,
                                                                   const int64_t* __restrict__ chunk_off,
                                                                   const int64_t* __restrict__ seg_g,
                                                                   const int64_t* __restrict__ seg_numel,
                                                                   double* __restrict__ partial) {
  __shared__ double sh[kBlock / GOL_WAVE];
  const Chunk c = chunk_of(chunk_seg, chunk_off, seg_numel, n_seg);
  double sq = 0.0, bad = 0.0;
  if (c.n > 0) {
    const gfloat* g = global_floats(seg_g[c.seg], c.off);
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
      const int nv = c.n >> 2;
      f4 x[kVecIters];
#pragma unroll
      for (int k = 0; k < kVecIters; ++k) {
        const int i = threadIdx.x + k * kBlock;
        x[k] = i < nv ? reinterpret_cast<const gf4*>(g)[i] : f4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int k = 0; k < kVecIters; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) stat_add(x[k][e], sq, bad);
      }
      const int i = (nv << 2) + threadIdx.x;
      if (threadIdx.x < 3 && i < c.n) stat_add(g[i], sq, bad);
    } else {
      for (int i = threadIdx.x; i < c.n; i += kBlock) stat_add(g[i], sq, bad);
    }
  }
  sq = gol_block_sum<double, kBlock / GOL_WAVE>(sq, sh);
  bad = gol_block_sum<double, kBlock / GOL_WAVE>(bad, sh);
  if (threadIdx.x == 0) {
    partial[2 * (size_t)blockIdx.x] = sq;
    partial[2 * (size_t)blockIdx.x + 1] = bad;
  }
}

__global__ __launch_bounds__(kFinalBlock) void optim_finalize_kernel(int n_chunks, const double* __restrict__ partial,
                                                                      double max_norm, double* __restrict__ stats,
                                                                      int64_t* __restrict__ nonfinite) {
  __shared__ double sh[kFinalBlock / GOL_WAVE];
  double sq = 0.0, bad = 0.0;
  for (int c = threadIdx.x; c < n_chunks; c += kFinalBlock) {
    sq += partial[2 * (size_t)c];
    bad += partial[2 * (size_t)c + 1];
  }
  sq = gol_block_sum<double, kFinalBlock / GOL_WAVE>(sq, sh);
  bad = gol_block_sum<double, kFinalBlock / GOL_WAVE>(bad, sh);
  if (threadIdx.x == 0) {
    const double norm = sqrt(sq);
    const double coef = max_norm / (norm + 1e-6);   // clip_grad_norm_'s rule
    stats[0] = norm;
    stats[1] = coef < 1.0 ? coef : 1.0;             // (+inf / NaN-free: norm is finite, max_norm > 0 or +inf)
    nonfinite[0] = (int64_t)bad;
  }
}

// one thread per segment: advance the step counter and turn the group's hyper-parameters into the float constants of this
// step, computed in double the way torch computes them in Python floats
__global__ void optim_prepare_kernel(int n_seg, int n_groups, const int64_t* __restrict__ seg_step,
                                     const int32_t* __restrict__ seg_group, const double* __restrict__ groups,
                                     float* __restrict__ seg_coef) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seg) return;
  const int gi = seg_group[s];
  float* c = seg_coef + (size_t)s * kCoef;
  if (gi < 0 || gi >= n_groups) {   // a broken table: leave the tensor as it is
    c[6] = 0.f;
    return;
  }
  const double* G = groups + (size_t)gi * GOL_OPTIM_GROUP_DOUBLES;
  const double lr = G[0], b1 = G[1], b2 = G[2], eps = G[3], wd = G[4];
  const bool decoupled = G[5] != 0.0;
  float* step = reinterpret_cast<float*>(seg_step[s]);
  const float t = *step + 1.f;
  *step = t;
  const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
  c[0] = (float)(decoupled ? 1.0 - lr * wd : 1.0);   // p *= c0
  c[1] = (float)(decoupled ? 0.0 : wd);              // g += c1 p
  c[2] = (float)(1.0 - b1);
  c[3] = (float)b2;
  c[4] = (float)(1.0 - b2);
  c[5] = (float)(-(lr / bc1));
  c[6] = (float)sqrt(bc2);                           // > 0; 0 marks a segment to skip
  c[7] = (float)eps;
}

struct AdamCoef {
  float decay, l2, w1, b2, w2, neg_step, bc2_sqrt, eps, clip;
  int flags;
};

// torch's _single_tensor_adam, operation for operation
__device__ __forceinline__ void adam_elem(const AdamCoef& k, float& p, float& g, float& m, float& v) {
  if ((k.flags & kScrub) && !finite_f(g)) g = 0.f;
  g *= k.clip;                            // (1 without clipping)
  float gg = g;
  if (k.l2 != 0.f) gg += k.l2 * p;        // grad.add(param, alpha=weight_decay)
  if (k.decay != 1.f) p *= k.decay;       // param.mul_(1 - lr * weight_decay)
  m += k.w1 * (gg - m);                   // exp_avg.lerp_(grad, 1 - beta1)
  v = v * k.b2 + (k.w2 * gg) * gg;        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  p += (k.neg_step * m) / denom;          // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__device__ __forceinline__ void adam_scalar(const AdamCoef& k, gfloat* p, gfloat* g, gfloat* m, gfloat* v, int i) {
  float pp = p[i], gg = g[i], mm = m[i], vv = v[i];
  adam_elem(k, pp, gg, mm, vv);
  p[i] = pp, m[i] = mm, v[i] = vv;
  if (k.flags & kWriteBack) g[i] = gg;
}

// the float4 groups [0, nv) of a chunk, all 16 loads of a lane issued before the first use; FULL: nv = kChunk / 4, no lane
// is idle and no load is predicated
template <bool FULL>
__device__ __forceinline__ void adam_vec(const AdamCoef& k, gfloat* p, gfloat* g, gfloat* m, gfloat* v, int nv) {
  f4 P[kVecIters], G[kVecIters], M[kVecIters], V[kVecIters];
#pragma unroll
  for (int j = 0; j < kVecIters; ++j) {
    const int i = threadIdx.x + j * kBlock;
    if (FULL || i < nv) {
      G[j] = reinterpret_cast<const gf4*>(g)[i];
      P[j] = reinterpret_cast<const gf4*>(p)[i];
      M[j] = reinterpret_cast<const gf4*>(m)[i];
      V[j] = reinterpret_cast<const gf4*>(v)[i];
    }
  }
#pragma unroll
  for (int j = 0; j < kVecIters; ++j) {
    const int i = threadIdx.x + j * kBlock;
    if (FULL || i < nv) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pp = P[j][e], gg = G[j][e], mm = M[j][e], vv = V[j][e];
        adam_elem(k, pp, gg, mm, vv);
        P[j][e] = pp, G[j][e] = gg, M[j][e] = mm, V[j][e] = vv;
      }
      reinterpret_cast<gf4*>(p)[i] = P[j];
      reinterpret_cast<gf4*>(m)[i] = M[j];
      reinterpret_cast<gf4*>(v)[i] = V[j];
      if (k.flags & kWriteBack) reinterpret_cast<gf4*>(g)[i] = G[j];
    }
  }
}

__global__ __launch_bounds__(kBlock) void optim_adam_kernel(int n_seg, const int32_t* __restrict__ chunk_seg,
                                                             const int64_t* __restrict__ chunk_off,
                                                             const int64_t* __restrict__ seg_p,
                                                             const int64_t* __restrict__ seg_g,
                                                             const int64_t* __restrict__ seg_m,
                                                             const int64_t* __restrict__ seg_v,
                                                             const int64_t* __restrict__ seg_numel,
                                                             const float* __restrict__ seg_coef,
                                                             const double* __restrict__ stats, int flags) {
  const Chunk c = chunk_of(chunk_seg, chunk_off, seg_numel, n_seg);
  if (c.n <= 0) return;
  const float* sc = seg_coef + (size_t)c.seg * kCoef;
  if (sc[6] == 0.f) return;
  AdamCoef k;
  k.decay = sc[0], k.l2 = sc[1], k.w1 = sc[2], k.b2 = sc[3], k.w2 = sc[4], k.neg_step = sc[5], k.bc2_sqrt = sc[6];
  k.eps = sc[7];
  k.flags = flags;
  k.clip = (flags & kClip) ? (float)stats[1] : 1.f;
  gfloat* p = global_floats(seg_p[c.seg], c.off);
  gfloat* g = global_floats(seg_g[c.seg], c.off);
  gfloat* m = global_floats(seg_m[c.seg], c.off);
  gfloat* v = global_floats(seg_v[c.seg], c.off);
  const uintptr_t align = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
                          reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v);
  if ((align & 15) != 0) {
    for (int i = threadIdx.x; i < c.n; i += kBlock) adam_scalar(k, p, g, m, v, i);
  } else if (c.n == kChunk) {
    adam_vec<true>(k, p, g, m, v, kChunk / 4);
  } else {
    const int nv = c.n >> 2;
    adam_vec<false>(k, p, g, m, v, nv);
    const int i = (nv << 2) + threadIdx.x;
    if (threadIdx.x < 3 && i < c.n) adam_scalar(k, p, g, m, v, i);
  }
}

}  // namespace

extern "C" int gol_optim_chunk_elems(void) { return kChunk; }

extern "C" int gol_optim_grad_stats(int n_chunks, int n_seg, const int32_t* chunk_seg, const int64_t* chunk_off,
                                    const int64_t* seg_g, const int64_t* seg_numel, double* partial, void* stream) {
  GOL_REQUIRE(n_chunks >= 0 && n_seg >= 0, "negative count");
  if (n_chunks == 0) return GOL_OK;
  GOL_REQUIRE(chunk_seg && chunk_off && seg_g && seg_numel && partial, "null pointer");
  hipLaunchKernelGGL(optim_grad_stats_kernel, dim3(n_chunks), dim3(kBlock), 0, (hipStream_t)stream, n_seg, chunk_seg,
                     chunk_off, seg_g, seg_numel, partial);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_optim_finalize(int n_chunks, const double* partial, double max_norm, double* stats, int64_t* nonfinite,
                                  void* stream) {
  GOL_REQUIRE(n_chunks >= 0 && stats && nonfinite && (partial || n_chunks == 0), "bad size or null pointer");
  GOL_REQUIRE(max_norm > 0.0, "max_norm must be positive (+inf = no clipping)");
  hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(kFinalBlock), 0, (hipStream_t)stream, n_chunks, partial, max_norm,
                     stats, nonfinite);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_optim_adam_step(int n_chunks, int n_seg, int n_groups, const int32_t* chunk_seg, const int64_t* chunk_off,
                                   const int64_t* seg_p, const int64_t* seg_g, const int64_t* seg_m, const int64_t* seg_v,
                                   const int64_t* seg_step, const int64_t* seg_numel, const int32_t* seg_group,
                                   const double* groups, const double* stats, float* seg_coef, int flags, void* stream) {
  if (flags & ~kAllFlags) {
    gol_set_error("%s: amsgrad, maximize and host-side (non-capturable) steps are not supported (flags %d)", __func__, flags);
    return GOL_ERR_UNSUPPORTED;
  }
  GOL_REQUIRE(n_chunks >= 0 && n_seg >= 0 && n_groups >= 0, "negative count");
  if (n_seg == 0) return GOL_OK;
  GOL_REQUIRE(chunk_seg && chunk_off && seg_p && seg_g && seg_m && seg_v && seg_step && seg_numel && seg_group && groups &&
                  seg_coef, "null pointer");
  GOL_REQUIRE(!(flags & kClip) || stats, "clipping needs the stats of gol_optim_finalize");
  hipLaunchKernelGGL(optim_prepare_kernel, dim3(gol_cdiv(n_seg, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n_seg,
                     n_groups, seg_step, seg_group, groups, seg_coef);
  GOL_CHECK_LAUNCH();
  if (n_chunks == 0) return GOL_OK;
  hipLaunchKernelGGL(optim_adam_kernel, dim3(n_chunks), dim3(kBlock), 0, (hipStream_t)stream, n_seg, chunk_seg, chunk_off,
                     seg_p, seg_g, seg_m, seg_v, seg_numel, seg_coef, stats, flags);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
