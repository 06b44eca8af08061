// uvtex.hip -- URHand's texture tail, between the decoder's `relight_preds["tex"]` and the RGBA textures the renderer
// takes, as ONE pass forward and ONE pass backward over the [B,C,S,S] texture, gfx950.
//
// Replaces (/root/reference/ca_code):
//   models/urhand.py:721-741  forward_tex: gain / bias split by channel count, tex_mean * gain + bias * tex_std
//   nn/color_cal.py:211-241   CalV5.forward as a per-view 3x3 matrix + bias (goliath_amd.imgtail.cal_v5_matrix)
//   models/urhand.py:747      clamp_(0, 255)                                     -> texrec_before_warp
//   utils/seams.py:21-25      resample_tex: bilinear grid_sample (border, align_corners=False) + lerp by the seam weights
//   models/urhand.py:824-826  ones_like + cat into RGBA (also :788-790 for phys_tex: gol_pack_rgba_*)
//   models/urhand.py:828-832, :843-847  normal colours: bmm with Rt[:, :3, :3]^T, (1 - n) * 127.5, cat with ones
// Streaming kernels: one 256-thread workgroup per 1024 consecutive texels of one view, four consecutive texels per lane
// (16-byte loads and stores when S*S is a multiple of 4, scalar ones otherwise).  A texel on the seam band (weight != 0)
// recomputes the clamped value at its four bilinear taps from tex / tex_mean / the cal instead of reading it back, so the
// forward never waits on its own output.  The backward is a gather over the transposed tap list (CSR by destination
// texel, goliath_amd.uvtex.pack_seams): no atomics, every sum in a fixed order, bitwise reproducible.  The 12 sums of
// the cal gradient per view are block-reduced into per-workgroup partial sums, as in imgtail.hip.
#include "gol_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kV = 4;                    // texels per lane
constexpr int kChunk = kBlock * kV;      // texels per workgroup

struct TexArgs {
  int B, C, S, mean_batched;
  int vec;                // 16-byte accesses: S*S % 4 == 0 and every image pointer 16-byte aligned
  const float* tex;       // [B,C,S,S], C in {2,4,6}
  const float* mean;      // [B,3,S,S] or [1,3,S,S]
  float tex_std;
  const float* M;         // [B,3,3] or null (identity)
  const float* bvec;      // [B,3] or null
  const float* uvs;       // [S,S,2] or null (no resample)
  const float* weights;   // [S,S] or null (with uvs)
};

struct Cal {
  float m[3][3], b[3];
};

__device__ __forceinline__ Cal load_cal(const TexArgs& a, int v) {
  Cal w;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int j = 0; j < 3; ++j) w.m[c][j] = a.M ? a.M[(size_t)v * 9 + c * 3 + j] : (c == j ? 1.f : 0.f);
    w.b[c] = a.bvec ? a.bvec[(size_t)v * 3 + c] : 0.f;
  }
  return w;
}

// four consecutive floats starting at p[i]; n = how many of them exist
__device__ __forceinline__ void ld4(const float* __restrict__ p, size_t i, int n, bool vec, float (&o)[kV]) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(p + i);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < kV; ++k) o[k] = k < n ? p[i + k] : 0.f;
  }
}
__device__ __forceinline__ void st4(float* __restrict__ p, size_t i, int n, bool vec, const float (&o)[kV]) {
  if (vec) {
    *reinterpret_cast<float4*>(p + i) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int k = 0; k < kV; ++k)
      if (k < n) p[i + k] = o[k];
  }
}

// uncalibrated colour tex_mean * gain + bias * tex_std from the loaded channels (tex_mean clamped to [0, 255] by the
// callers: urhand.py:740 clamps forward_tex's local tex_mean in place, through a detached alias, before :741 uses it); the (gain, bias) channel of colour j
// (urhand.py:721-729): C = 2 -> (0, 1), C = 4 -> (j, 3), C = 6 -> (j, 3 + j)
__device__ __forceinline__ void raw_of(int C, const float (&t)[6], const float (&mean)[3], float tex_std, float (&raw)[3]) {
  const float g1 = t[0], b1 = C == 2 ? t[1] : t[3];
  raw[0] = mean[0] * g1 + b1 * tex_std;
  raw[1] = mean[1] * (C == 2 ? g1 : t[1]) + (C == 6 ? t[4] : b1) * tex_std;
  raw[2] = mean[2] * (C == 2 ? g1 : t[2]) + (C == 6 ? t[5] : b1) * tex_std;
}

__device__ __forceinline__ void cal_of(const Cal& w, const float (&raw)[3], float (&x)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = w.m[c][0] * raw[0] + w.m[c][1] * raw[1] + w.m[c][2] * raw[2] + w.b[c];
}

__device__ __forceinline__ float clamp255(float x) { return fminf(fmaxf(x, 0.f), 255.f); }

// pre = clamp(cal(tex_mean * gain + bias * tex_std), 0, 255) at texel q (0 <= q < S*S) of view v
__device__ __forceinline__ void pre_at(const TexArgs& a, const Cal& w, int v, size_t hw, size_t q, float (&o)[3]) {
  const float* tq = a.tex + (size_t)v * a.C * hw + q;
  const float* mq = a.mean + (a.mean_batched ? (size_t)v * 3 * hw : 0) + q;
  float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 6; ++c)
    if (c < a.C) t[c] = tq[c * hw];
  const float mean[3] = {clamp255(mq[0]), clamp255(mq[hw]), clamp255(mq[2 * hw])};
  float raw[3], x[3];
  raw_of(a.C, t, mean, a.tex_std, raw);
  cal_of(w, raw, x);
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = clamp255(x[c]);
}

__global__ __launch_bounds__(kBlock) void uvtex_fwd_kernel(TexArgs a, float* __restrict__ before, float* __restrict__ rgba) {
  const int v = blockIdx.y;
  const size_t hw = (size_t)a.S * a.S;
  const size_t p0 = (size_t)blockIdx.x * kChunk + (size_t)threadIdx.x * kV;
  if (p0 >= hw) return;
  const int n = hw - p0 < (size_t)kV ? (int)(hw - p0) : kV;
  const bool vec = a.vec != 0;
  const Cal w = load_cal(a, v);
  float t[6][kV], mean[3][kV];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    if (c < a.C) ld4(a.tex + ((size_t)v * a.C + c) * hw, p0, n, vec, t[c]);
    else t[c][0] = t[c][1] = t[c][2] = t[c][3] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) ld4(a.mean + ((a.mean_batched ? (size_t)v * 3 : 0) + c) * hw, p0, n, vec, mean[c]);
  float sw[kV] = {0.f, 0.f, 0.f, 0.f};
  if (a.weights) ld4(a.weights, p0, n, vec, sw);
  float pre[3][kV], out[3][kV];
#pragma unroll
  for (int k = 0; k < kV; ++k) {
    const float tk[6] = {t[0][k], t[1][k], t[2][k], t[3][k], t[4][k], t[5][k]};
    const float mk[3] = {clamp255(mean[0][k]), clamp255(mean[1][k]), clamp255(mean[2][k])};
    float raw[3], x[3];
    raw_of(a.C, tk, mk, a.tex_std, raw);
    cal_of(w, raw, x);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c][k] = pre[c][k] = clamp255(x[c]);
  }
  if (a.weights) {
    const float Sm1 = (float)(a.S - 1);
#pragma unroll
    for (int k = 0; k < kV; ++k) {
      if (k >= n || sw[k] == 0.f) continue;   // off the seam band: out = pre exactly
      // grid_sample, bilinear, align_corners=False, padding_mode="border": the sample point is clipped into the image,
      // the taps are floor and floor + 1, a tap outside the image contributes nothing
      const float u = a.uvs[(p0 + k) * 2], vv = a.uvs[(p0 + k) * 2 + 1];
      const float x = fminf(fmaxf(u * (float)a.S - 0.5f, 0.f), Sm1), y = fminf(fmaxf(vv * (float)a.S - 0.5f, 0.f), Sm1);
      const float xf = floorf(x), yf = floorf(y);
      const int x0 = (int)xf, y0 = (int)yf;
      const float fx = x - xf, fy = y - yf;
      float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int xi = x0 + dx, yi = y0 + dy;
          if (xi >= a.S || yi >= a.S) continue;   // x0, y0 >= 0 after the clip
          const float bw = (dx ? fx : 1.f - fx) * (dy ? fy : 1.f - fy);
          float q[3];
          pre_at(a, w, v, hw, (size_t)yi * a.S + xi, q);
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += bw * q[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c][k] = (1.f - sw[k]) * pre[c][k] + sw[k] * acc[c];
    }
  }
  const float one[kV] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    st4(before + ((size_t)v * 3 + c) * hw, p0, n, vec, pre[c]);
    st4(rgba + ((size_t)v * 4 + c) * hw, p0, n, vec, out[c]);
  }
  st4(rgba + ((size_t)v * 4 + 3) * hw, p0, n, vec, one);
}

// g_pre[t] = (1 - w[t]) g[t] + sum_{e in row(t)} coeff[e] g[src[e]] (+ g_before[t]); through the clamp mask
// (0 <= x <= 255 passes, torch's), cal_M^T and the gain / bias products.  partials[(v * gridDim.x + block) * 16 + k]:
// bias 0..2 | M 3..11 | unused 12..15.
__global__ __launch_bounds__(kBlock) void uvtex_bwd_kernel(TexArgs a, const int* __restrict__ row_start,
                                                           const int* __restrict__ src, const float* __restrict__ coeff,
                                                           const float* __restrict__ g_rgba,
                                                           const float* __restrict__ g_before, float* __restrict__ g_tex,
                                                           float* __restrict__ partials) {
  __shared__ float s_red[kBlock / GOL_WAVE][16];
  const int v = blockIdx.y, tid = threadIdx.x;
  const size_t hw = (size_t)a.S * a.S;
  const size_t p0 = (size_t)blockIdx.x * kChunk + (size_t)tid * kV;
  const bool live = p0 < hw;
  const int n = !live ? 0 : hw - p0 < (size_t)kV ? (int)(hw - p0) : kV;
  const bool vec = a.vec != 0;
  float sums[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) sums[k] = 0.f;
  if (live) {
    const Cal w = load_cal(a, v);
    const float* gv = g_rgba + (size_t)v * 4 * hw;
    float t[6][kV], mean[3][kV], g[3][kV];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      if (c < a.C) ld4(a.tex + ((size_t)v * a.C + c) * hw, p0, n, vec, t[c]);
      else t[c][0] = t[c][1] = t[c][2] = t[c][3] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ld4(a.mean + ((a.mean_batched ? (size_t)v * 3 : 0) + c) * hw, p0, n, vec, mean[c]);
      ld4(gv + c * hw, p0, n, vec, g[c]);
    }
    if (a.weights) {
      float sw[kV];
      ld4(a.weights, p0, n, vec, sw);
#pragma unroll
      for (int k = 0; k < kV; ++k) {
        if (k >= n) continue;
        const float om = 1.f - sw[k];
        float acc[3] = {om * g[0][k], om * g[1][k], om * g[2][k]};
        const int e1 = row_start[p0 + k + 1];
        for (int e = row_start[p0 + k]; e < e1; ++e) {
          const float ce = coeff[e];
          const float* gs = gv + src[e];
          acc[0] += ce * gs[0]; acc[1] += ce * gs[hw]; acc[2] += ce * gs[2 * hw];
        }
        g[0][k] = acc[0]; g[1][k] = acc[1]; g[2][k] = acc[2];
      }
    }
    if (g_before) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float gb[kV];
        ld4(g_before + ((size_t)v * 3 + c) * hw, p0, n, vec, gb);
#pragma unroll
        for (int k = 0; k < kV; ++k) g[c][k] += gb[k];
      }
    }
    float gt[6][kV] = {};
#pragma unroll
    for (int k = 0; k < kV; ++k) {
      const float tk[6] = {t[0][k], t[1][k], t[2][k], t[3][k], t[4][k], t[5][k]};
      const float mk[3] = {clamp255(mean[0][k]), clamp255(mean[1][k]), clamp255(mean[2][k])};
      float raw[3], x[3], gx[3], gr[3];
      raw_of(a.C, tk, mk, a.tex_std, raw);
      cal_of(w, raw, x);
#pragma unroll
      for (int c = 0; c < 3; ++c) gx[c] = (k < n && x[c] >= 0.f && x[c] <= 255.f) ? g[c][k] : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sums[c] += gx[c];
#pragma unroll
        for (int j = 0; j < 3; ++j) sums[3 + c * 3 + j] += gx[c] * raw[j];
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) gr[j] = w.m[0][j] * gx[0] + w.m[1][j] * gx[1] + w.m[2][j] * gx[2];
      const float gg[3] = {gr[0] * mk[0], gr[1] * mk[1], gr[2] * mk[2]};
      const float gb[3] = {gr[0] * a.tex_std, gr[1] * a.tex_std, gr[2] * a.tex_std};
      if (a.C == 2) {
        gt[0][k] = gg[0] + gg[1] + gg[2];
        gt[1][k] = gb[0] + gb[1] + gb[2];
      } else {
        gt[0][k] = gg[0]; gt[1][k] = gg[1]; gt[2][k] = gg[2];
        if (a.C == 4) {
          gt[3][k] = gb[0] + gb[1] + gb[2];
        } else {
          gt[3][k] = gb[0]; gt[4][k] = gb[1]; gt[5][k] = gb[2];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c)
      if (c < a.C) st4(g_tex + ((size_t)v * a.C + c) * hw, p0, n, vec, gt[c]);
  }
  if (!partials) return;   // no cal: nothing to reduce (uniform over the grid)
  // 12 block sums: three 4-way wave reductions (results in lanes 15/31/47/63), then across the waves through LDS
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k4 = 0; k4 < 3; ++k4) {
    const float r = gol_wave_sum4(sums[4 * k4], sums[4 * k4 + 1], sums[4 * k4 + 2], sums[4 * k4 + 3]);
    if ((lane & 15) == 15) s_red[wave][4 * k4 + (lane >> 4)] = r;
  }
  __syncthreads();
  if (tid < 16) {
    const size_t blk = (size_t)v * gridDim.x + blockIdx.x;
    partials[blk * 16 + tid] = tid < 12 ? s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid] : 0.f;
  }
}

// out[:, :3] = clamp(x * scale, lo, hi), out[:, 3] = 1
__global__ __launch_bounds__(kBlock) void pack_rgba_fwd_kernel(int S, int vec4, float scale, float lo, float hi,
                                                               const float* __restrict__ x, float* __restrict__ out) {
  const int v = blockIdx.y;
  const size_t hw = (size_t)S * S;
  const size_t p0 = (size_t)blockIdx.x * kChunk + (size_t)threadIdx.x * kV;
  if (p0 >= hw) return;
  const int n = hw - p0 < (size_t)kV ? (int)(hw - p0) : kV;
  const bool vec = vec4 != 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float xv[kV];
    ld4(x + ((size_t)v * 3 + c) * hw, p0, n, vec, xv);
#pragma unroll
    for (int k = 0; k < kV; ++k) xv[k] = fminf(fmaxf(xv[k] * scale, lo), hi);
    st4(out + ((size_t)v * 4 + c) * hw, p0, n, vec, xv);
  }
  const float one[kV] = {1.f, 1.f, 1.f, 1.f};
  st4(out + ((size_t)v * 4 + 3) * hw, p0, n, vec, one);
}

// g_x = scale * [lo <= x * scale <= hi] * g_out[:, :3]
__global__ __launch_bounds__(kBlock) void pack_rgba_bwd_kernel(int S, int vec4, float scale, float lo, float hi,
                                                               const float* __restrict__ x,
                                                               const float* __restrict__ g_out, float* __restrict__ g_x) {
  const int v = blockIdx.y;
  const size_t hw = (size_t)S * S;
  const size_t p0 = (size_t)blockIdx.x * kChunk + (size_t)threadIdx.x * kV;
  if (p0 >= hw) return;
  const int n = hw - p0 < (size_t)kV ? (int)(hw - p0) : kV;
  const bool vec = vec4 != 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float xv[kV], gv[kV];
    ld4(x + ((size_t)v * 3 + c) * hw, p0, n, vec, xv);
    ld4(g_out + ((size_t)v * 4 + c) * hw, p0, n, vec, gv);
#pragma unroll
    for (int k = 0; k < kV; ++k) {
      const float y = xv[k] * scale;
      gv[k] = (y >= lo && y <= hi) ? gv[k] * scale : 0.f;
    }
    st4(g_x + ((size_t)v * 3 + c) * hw, p0, n, vec, gv);
  }
}

// out[:, c] = (1 - sum_j R[c][j] n[j]) * 127.5, out[:, 3] = 1; R = Rt[v][:3, :3], rows 4 floats apart
__global__ __launch_bounds__(kBlock) void normal_rgba_kernel(int S, int vec4, int rt_stride, const float* __restrict__ nml,
                                                             const float* __restrict__ Rt, float* __restrict__ out) {
  const int v = blockIdx.y;
  const size_t hw = (size_t)S * S;
  const size_t p0 = (size_t)blockIdx.x * kChunk + (size_t)threadIdx.x * kV;
  if (p0 >= hw) return;
  const int n = hw - p0 < (size_t)kV ? (int)(hw - p0) : kV;
  const bool vec = vec4 != 0;
  float nv[3][kV];
#pragma unroll
  for (int j = 0; j < 3; ++j) ld4(nml + ((size_t)v * 3 + j) * hw, p0, n, vec, nv[j]);
  const float* R = Rt + (size_t)v * rt_stride;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float r0 = R[c * 4], r1 = R[c * 4 + 1], r2 = R[c * 4 + 2];
    float o[kV];
#pragma unroll
    for (int k = 0; k < kV; ++k) o[k] = (1.f - (nv[0][k] * r0 + nv[1][k] * r1 + nv[2][k] * r2)) * 127.5f;
    st4(out + ((size_t)v * 4 + c) * hw, p0, n, vec, o);
  }
  const float one[kV] = {1.f, 1.f, 1.f, 1.f};
  st4(out + ((size_t)v * 4 + 3) * hw, p0, n, vec, one);
}

int check_size(const char* fn, int B, int S) {
  if (B < 0 || S <= 0) { gol_set_error("%s: bad size", fn); return GOL_ERR_INVALID_ARG; }
  if (B > 65535) { gol_set_error("%s: B > 65535", fn); return GOL_ERR_INVALID_ARG; }
  if (S > 16384) { gol_set_error("%s: S > 16384", fn); return GOL_ERR_INVALID_ARG; }
  return GOL_OK;
}

int check_tex(const char* fn, const TexArgs& a) {
  const int rc = check_size(fn, a.B, a.S);
  if (rc != GOL_OK) return rc;
  if (a.C != 2 && a.C != 4 && a.C != 6) { gol_set_error("%s: C must be 2, 4 or 6", fn); return GOL_ERR_INVALID_ARG; }
  if (a.B && (!a.tex || !a.mean)) { gol_set_error("%s: null texture", fn); return GOL_ERR_INVALID_ARG; }
  if ((a.M == nullptr) != (a.bvec == nullptr)) { gol_set_error("%s: cal_M and cal_b go together", fn); return GOL_ERR_INVALID_ARG; }
  return GOL_OK;
}

// 16-byte accesses are possible: S*S is a multiple of 4 and every (non-null) image pointer is 16-byte aligned
template <typename... P>
int vec_ok(int S, P... ptrs) {
  uintptr_t bits = ((size_t)S * S) & 3;
  for (const void* p : {static_cast<const void*>(ptrs)...}) bits |= reinterpret_cast<uintptr_t>(p) & 15;
  return bits == 0;
}

dim3 grid_of(int B, int S) { return dim3(gol_cdiv((long long)S * S, kChunk), B); }

}  // namespace

extern "C" int64_t gol_uvtex_partial_floats(int B, int S) {
  return (int64_t)B * gol_cdiv((long long)S * S, kChunk) * 16;
}

extern "C" int gol_uvtex_fwd(int B, int C, int S, int mean_batched, const float* tex, const float* tex_mean, float tex_std,
                             const float* cal_M, const float* cal_b, const float* uvs, const float* weights,
                             float* texrec_before_warp, float* tex_rgba, void* stream) {
  const TexArgs a{B, C, S, mean_batched, vec_ok(S, tex, tex_mean, weights, texrec_before_warp, tex_rgba),
                  tex, tex_mean, tex_std, cal_M, cal_b, uvs, weights};
  const int rc = check_tex("gol_uvtex_fwd", a);
  if (rc != GOL_OK) return rc;
  GOL_REQUIRE((uvs == nullptr) == (weights == nullptr), "uvs and weights go together");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(texrec_before_warp && tex_rgba, "null output");
  uvtex_fwd_kernel<<<grid_of(B, S), kBlock, 0, (hipStream_t)stream>>>(a, texrec_before_warp, tex_rgba);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_uvtex_bwd(int B, int C, int S, int mean_batched, const float* tex, const float* tex_mean, float tex_std,
                             const float* cal_M, const float* cal_b, const float* weights, const int32_t* row_start,
                             const int32_t* src, const float* coeff, const float* g_tex_rgba,
                             const float* g_texrec_before_warp, float* g_tex, float* partials, void* stream) {
  const TexArgs a{B, C, S, mean_batched, vec_ok(S, tex, tex_mean, weights, g_tex_rgba, g_texrec_before_warp, g_tex),
                  tex, tex_mean, tex_std, cal_M, cal_b, nullptr, weights};
  const int rc = check_tex("gol_uvtex_bwd", a);
  if (rc != GOL_OK) return rc;
  GOL_REQUIRE(!weights || row_start, "seam weights need the tap list (row_start; src and coeff may be empty)");
  GOL_REQUIRE((cal_M != nullptr) == (partials != nullptr), "partials go with the cal");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(g_tex_rgba && g_tex, "null pointer");
  uvtex_bwd_kernel<<<grid_of(B, S), kBlock, 0, (hipStream_t)stream>>>(a, row_start, src, coeff, g_tex_rgba,
                                                                       g_texrec_before_warp, g_tex, partials);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_pack_rgba_fwd(int B, int S, float scale, float lo, float hi, const float* x, float* out, void* stream) {
  const int rc = check_size("gol_pack_rgba_fwd", B, S);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && out, "null pointer");
  pack_rgba_fwd_kernel<<<grid_of(B, S), kBlock, 0, (hipStream_t)stream>>>(S, vec_ok(S, x, out), scale, lo, hi, x, out);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_pack_rgba_bwd(int B, int S, float scale, float lo, float hi, const float* x, const float* g_out,
                                 float* g_x, void* stream) {
  const int rc = check_size("gol_pack_rgba_bwd", B, S);
  if (rc != GOL_OK) return rc;
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(x && g_out && g_x, "null pointer");
  pack_rgba_bwd_kernel<<<grid_of(B, S), kBlock, 0, (hipStream_t)stream>>>(S, vec_ok(S, x, g_out, g_x), scale, lo, hi, x, g_out, g_x);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_normal_rgba(int B, int S, int rt_stride, const float* nml, const float* Rt, float* out, void* stream) {
  const int rc = check_size("gol_normal_rgba", B, S);
  if (rc != GOL_OK) return rc;
  GOL_REQUIRE(rt_stride == 12 || rt_stride == 16, "Rt must be [B,3,4] or [B,4,4]");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(nml && Rt && out, "null pointer");
  normal_rgba_kernel<<<grid_of(B, S), kBlock, 0, (hipStream_t)stream>>>(S, vec_ok(S, nml, out), rt_stride, nml, Rt, out);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
