// viewtex.hip -- camera images unwrapped into UV space and the mean texture over many views, gfx950.  Forward only.
//
// What run_gen_texmean.py:83-108 does per camera through ca_code/utils/tex.py:21-63 with ca_code/utils/geom.py:834-910:
//   gol_face_visibility   compute_face_visibility (geom.py:834-845): which faces a view's index image shows
//   gol_view_texture      compute_uv_visiblity_face + compute_view_texture (geom.py:847-910) and, in accumulate mode, the
//                         script's `tex_total += tex_img; tex_cnt += tex_mask.float()` (run_gen_texmean.py:102-103)
//   gol_texmean_finalize  `tex_total /= tex_cnt + 1e-5`, the row flip and the BGR swap (run_gen_texmean.py:105-108)
//
// A per-texel gather without any reduction, in two passes.  Pass 1: one lane per camera pixel stores the constant 1 to
// face_vis[b, index] (plain byte stores: every lane that hits a byte writes the same value; a pixel whose left neighbour
// holds the same index leaves the store to it).  Pass 2: one lane per UV texel, row-major -- the topology loads and every
// store are full wave lines, only the three vertex gathers, the visibility byte and the image fetch are scattered.  The
// lane keeps its texel's vertex triple, barycentrics and face in registers and walks the B views; K and Rt of a view are
// read through scalar loads (the view index is wave-uniform).  In accumulate mode the running sums start from the loaded
// accumulators and take the views in order: a texel belongs to one lane, so the result needs no atomics, is reproducible
// and equals B successive `tex_total += tex` bit for bit.
//
// Arithmetic per view (fp32, nothing contracted except the two matrix products, which accumulate by FMA over ascending k
// as a GEMM does): xyz = v0 b0 + v1 b1 + v2 b2 (geom.py:884-886); p_cam = R xyz + t, p = K p_cam with the full 3x3 K,
// pix = p.xy / p.z (project_points_multi, geom.py:611-623); g = 2 (pix / size) - 1 (geom.py:890); grid_sample's
// un-normalisation ((g + 1) size - 1) / 2, border clamp to [0, size - 1], round to nearest even, fetch (geom.py:892).
// STATED: only the face index image decides visibility -- a sample behind the camera (p.z < 0) is taken like any other,
// the reference has no depth test; p.z == 0 or a non-finite pixel coordinate gives the texel 0 for that view (the
// reference's result there is unspecified); a texel that is not visible, or not covered, reads nothing and gives exactly
// 0 even where the image holds NaN (the reference: NaN * 0 = NaN); vertex or face ids out of range count as -1.
#include <math.h>

#include "gol_common.h"

namespace {

// one lane per camera pixel; blockIdx.y = the view
__global__ __launch_bounds__(256) void face_visibility_kernel(int F, int HW, int W, const int32_t* __restrict__ index_img,
                                                              uint8_t* __restrict__ face_vis) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= HW) return;
  const int32_t* img = index_img + (size_t)b * HW;
  const int f = img[i];
  if (f < 0 || f >= F) return;
  if (i % W > 0 && img[i - 1] == f) return;   // the left neighbour stores the same byte
  face_vis[(size_t)b * F + f] = 1;
}

// the scalars of a launch; the pointers are kernel parameters of their own so that they can be __restrict__ (the loads of
// K and Rt inside the view loop stay scalar only while the compiler knows the loop's stores cannot touch them)
struct ViewTexDims {
  int B, V, F, H, W, P;
  long long verts_bstride;     // floats between two views' vertices; 0 = one mesh for all views
  int has_threshold;
  float threshold;
};

// one lane per UV texel; the views in order
__global__ __launch_bounds__(256) void view_texture_kernel(
    ViewTexDims a, const float* __restrict__ verts, const float* __restrict__ image, const float* __restrict__ K,
    const float* __restrict__ Rt, const int32_t* __restrict__ index_image_uv, const float* __restrict__ bary_image_uv,
    const int32_t* __restrict__ face_index_uv, const uint8_t* __restrict__ face_vis, float* __restrict__ tex,
    uint8_t* __restrict__ mask, float* __restrict__ total, float* __restrict__ cnt) {
#pragma clang fp contract(off)   // the reference's products and sums, each rounded as it rounds them
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.P) return;
  int i0 = -1, i1 = -1, i2 = -1;
  float b0 = 0.f, b1 = 0.f, b2 = 0.f;
  if (index_image_uv) {   // (NULL: the mask alone is wanted)
    i0 = index_image_uv[3 * (size_t)p]; i1 = index_image_uv[3 * (size_t)p + 1]; i2 = index_image_uv[3 * (size_t)p + 2];
    b0 = bary_image_uv[3 * (size_t)p]; b1 = bary_image_uv[3 * (size_t)p + 1]; b2 = bary_image_uv[3 * (size_t)p + 2];
  }
  const int face = face_index_uv[p];
  // geom.py:880: a texel is covered when its first vertex id is not -1; ids out of range count as -1
  const bool covered = i0 >= 0 && i0 < a.V && i1 >= 0 && i1 < a.V && i2 >= 0 && i2 < a.V;
  const bool has_face = face >= 0 && face < a.F;
  const size_t HW = (size_t)a.H * a.W;
  const float fW = (float)a.W, fH = (float)a.H;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, n = 0.f;
  if (total) {
    acc0 = total[p]; acc1 = total[(size_t)a.P + p]; acc2 = total[2 * (size_t)a.P + p];
    n = cnt[p];
  }
  for (int b = 0; b < a.B; ++b) {
    const bool vis = has_face && face_vis[(size_t)b * a.F + face] != 0;
    float r = 0.f, g = 0.f, bl = 0.f;
    if (vis && covered) {
      const float* v = verts + (size_t)b * a.verts_bstride;
      const float* k = K + 9 * (size_t)b;     // wave-uniform: scalar loads
      const float* rt = Rt + 12 * (size_t)b;
      const float x = v[3 * i0] * b0 + v[3 * i1] * b1 + v[3 * i2] * b2;
      const float y = v[3 * i0 + 1] * b0 + v[3 * i1 + 1] * b1 + v[3 * i2 + 1] * b2;
      const float z = v[3 * i0 + 2] * b0 + v[3 * i1 + 2] * b1 + v[3 * i2 + 2] * b2;
      const float cx = __fmaf_rn(rt[2], z, __fmaf_rn(rt[1], y, rt[0] * x)) + rt[3];
      const float cy = __fmaf_rn(rt[6], z, __fmaf_rn(rt[5], y, rt[4] * x)) + rt[7];
      const float cz = __fmaf_rn(rt[10], z, __fmaf_rn(rt[9], y, rt[8] * x)) + rt[11];
      const float px = __fmaf_rn(k[2], cz, __fmaf_rn(k[1], cy, k[0] * cx));
      const float py = __fmaf_rn(k[5], cz, __fmaf_rn(k[4], cy, k[3] * cx));
      const float pz = __fmaf_rn(k[8], cz, __fmaf_rn(k[7], cy, k[6] * cx));
      const float ux = px / pz, uy = py / pz;
      if (pz != 0.f && fabsf(ux) < INFINITY && fabsf(uy) < INFINITY) {
        const float gx = 2.0f * (ux / fW) - 1.0f, gy = 2.0f * (uy / fH) - 1.0f;
        float sx = ((gx + 1.f) * fW - 1.f) / 2.f, sy = ((gy + 1.f) * fH - 1.f) / 2.f;
        sx = fminf(fW - 1.f, fmaxf(sx, 0.f));
        sy = fminf(fH - 1.f, fmaxf(sy, 0.f));
        // the clamp keeps both inside the image, also after rounding
        const int col = (int)rintf(sx), row = (int)rintf(sy);
        const float* px0 = image + (size_t)b * 3 * HW + (size_t)row * a.W + col;
        r = px0[0]; g = px0[HW]; bl = px0[2 * HW];
        if (a.has_threshold) {   // geom.py:907-908
          const float keep = (r <= a.threshold && g <= a.threshold && bl <= a.threshold) ? 1.f : 0.f;
          r *= keep; g *= keep; bl *= keep;
        }
      }
    }
    if (tex) {
      float* t = tex + (size_t)b * 3 * a.P + p;
      t[0] = r; t[a.P] = g; t[2 * (size_t)a.P] = bl;
    }
    if (mask) mask[(size_t)b * a.P + p] = vis ? 1 : 0;
    acc0 += r; acc1 += g; acc2 += bl;
    n += vis ? 1.f : 0.f;
  }
  if (total) {
    total[p] = acc0; total[(size_t)a.P + p] = acc1; total[2 * (size_t)a.P + p] = acc2;
    cnt[p] = n;
  }
}

// one lane per output float
__global__ __launch_bounds__(256) void texmean_finalize_kernel(int S_h, int S_w, const float* __restrict__ total,
                                                               const float* __restrict__ cnt, float eps, int flip_rows,
                                                               int bgr, float* __restrict__ out) {
  const size_t P = (size_t)S_h * S_w;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * P) return;
  const size_t q = i / 3;
  const int ch = (int)(i - 3 * q);
  const int r_out = (int)(q / S_w), c = (int)(q - (size_t)r_out * S_w);
  const int r = flip_rows ? S_h - 1 - r_out : r_out;
  const size_t p = (size_t)r * S_w + c;
  out[i] = total[(size_t)(bgr ? 2 - ch : ch) * P + p] / (cnt[p] + eps);
}

}  // namespace

extern "C" int gol_face_visibility(int B, int F, int H, int W, const int32_t* index_img, uint8_t* face_vis, void* stream) {
  GOL_REQUIRE(B >= 0 && F >= 0 && H > 0 && W > 0, "bad size");
  GOL_REQUIRE((long long)H * W < 2147483647LL && (long long)B * F < 2147483647LL, "image or face table too large");
  GOL_REQUIRE(B <= 65535, "at most 65535 views per call");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(index_img != nullptr, "null index_img");
  GOL_REQUIRE(F == 0 || face_vis != nullptr, "null face_vis");
  hipStream_t s = (hipStream_t)stream;
  if (F == 0) return GOL_OK;
  if (hipMemsetAsync(face_vis, 0, (size_t)B * F, s) != hipSuccess) {
    gol_set_error("%s: hipMemsetAsync failed", __func__);
    return GOL_ERR_LAUNCH;
  }
  face_visibility_kernel<<<dim3(gol_cdiv((long long)H * W, 256), B), 256, 0, s>>>(F, H * W, W, index_img, face_vis);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_view_texture(int B, int V, int F, int H, int W, int S_h, int S_w, const float* verts,
                                int64_t verts_bstride, const float* image, const float* K, const float* Rt,
                                const int32_t* index_image_uv, const float* bary_image_uv, const int32_t* face_index_uv,
                                const uint8_t* face_vis, int has_threshold, float intensity_threshold, float* tex,
                                uint8_t* mask, float* total, float* cnt, void* stream) {
  GOL_REQUIRE(B >= 0 && V >= 0 && F >= 0 && H > 0 && W > 0 && S_h > 0 && S_w > 0, "bad size");
  GOL_REQUIRE((long long)S_h * S_w < 2147483647LL / 4 && (long long)H * W < 2147483647LL, "image too large");
  GOL_REQUIRE((long long)V * 3 < 2147483647LL && (long long)B * F < 2147483647LL, "mesh too large");
  GOL_REQUIRE(verts_bstride == 0 || verts_bstride >= (int64_t)V * 3, "verts_bstride must be 0 or at least 3 V");
  GOL_REQUIRE((total == nullptr) == (cnt == nullptr), "total and cnt go together");
  GOL_REQUIRE(face_index_uv != nullptr, "null face_index_uv");
  if (B == 0 || (!tex && !mask && !total)) return GOL_OK;
  if (tex || total) {   // (the mask alone needs neither the mesh nor the images)
    GOL_REQUIRE(index_image_uv && bary_image_uv, "null topology image");
    GOL_REQUIRE(image && K && Rt, "null image, K or Rt");
    GOL_REQUIRE(V == 0 || verts != nullptr, "null verts");
  } else {
    index_image_uv = nullptr;
  }
  GOL_REQUIRE(F == 0 || face_vis != nullptr, "null face_vis");
  ViewTexDims a;
  a.B = B; a.V = V; a.F = F; a.H = H; a.W = W; a.P = S_h * S_w;
  a.verts_bstride = verts_bstride;
  a.has_threshold = has_threshold != 0; a.threshold = intensity_threshold;
  view_texture_kernel<<<gol_cdiv(a.P, 256), 256, 0, (hipStream_t)stream>>>(
      a, verts, image, K, Rt, index_image_uv, bary_image_uv, face_index_uv, face_vis, tex, mask, total, cnt);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_texmean_finalize(int S_h, int S_w, const float* total, const float* cnt, float eps, int flip_rows,
                                    int bgr, float* out, void* stream) {
  GOL_REQUIRE(S_h > 0 && S_w > 0 && (long long)S_h * S_w < 2147483647LL / 4, "bad size");
  GOL_REQUIRE(total && cnt && out, "null pointer");
  GOL_REQUIRE(out != total && out != cnt, "in place is not supported");
  texmean_finalize_kernel<<<gol_cdiv(3LL * S_h * S_w, 256), 256, 0, (hipStream_t)stream>>>(S_h, S_w, total, cnt, eps,
                                                                                             flip_rows, bgr, out);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
