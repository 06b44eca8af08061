// uvtopo.hip -- the constant UV topology images of a mesh (face / vertex index, barycentrics, impaint), gfx950.
//
// What GeometryModule.__init__ (ca_code/utils/geom.py:197-249) builds once per model with pytorch3d's CUDA
// rasterize_meshes (geom.py:31-66) and a scikit-learn KD-tree over up to 1024^2 texels (geom.py:145-194):
//   gol_uv_face_index   make_uv_face_index (geom.py:31-66): which UV triangle holds each texel
//   gol_uv_topology     make_uv_vert_index + make_uv_barys + bary_coords (geom.py:69-142) and the valid mask (:228)
//   gol_nearest_valid   the KD-tree query of index_image_impaint (geom.py:158-172), exact in integers
//   gol_impaint_gather  its three indexed copies (geom.py:180-191, 238-244) from ONE source map
//
// Coverage is not a second rasteriser: gol_mesh_raster_flat (meshraster.hip: gol_mesh_raster's kernel without the depth
// test, lowest face index first) runs on v_pix = (u W, v H, 1).  PINNED by the
// reference's own lines: texel (r, c) is sampled at uv = ((c + 0.5) / W, (r + 0.5) / H), v mirrored first when flip_uv --
// the grid make_uv_barys evaluates the barycentrics on (geom.py:133-139), which make_uv_face_index's `1 - vt` brings
// pytorch3d's +X-left / +Y-up image to; the barycentrics are bary_coords' arithmetic in fp32, operation for operation
// (anchored at the triangle's THIRD vertex, denom pushed away from 0 by eps = 1e-6 keeping its sign, b2 = 1 - b0 - b1),
// not the rasteriser's.  STATED, pytorch3d being absent: a texel centre exactly ON an edge is covered here (inside is
// >= 0 on un-normalised edge functions anchored at the face's first vertex, either winding), where pytorch3d is believed
// to leave it empty; zero-area faces are skipped; where faces overlap (all at z = 1) the lowest face index wins.
//
// Nearest valid texel: squared Euclidean distance over integer (row, col), ties to the lexicographically smallest
// (row, col), accepted while d^2 <= max_d2 (the host turns the reference's strict `dists < distance_threshold` into that
// integer).  Two passes.  Columns: one lane per column walks down, then up, and leaves each texel's nearest valid row in
// its own column (the upper row on a tie: lexicographically smaller, and the only candidate of that column that can be
// the overall winner).  Rows: one workgroup per 256 texels of a row stages that row of nearest rows in LDS, 256 columns
// at a time, and every invalid texel minimises (d^2, source row, source column) over the columns |c - c'| <= dmax,
// dmax = floor(sqrt(max_d2)) clipped to the image.  Any H, W and threshold; no atomics, bitwise reproducible.
#include "gol_common.h"

namespace {

__global__ __launch_bounds__(256) void uv_pix_kernel(int Vt, int H, int W, int flip_uv, const float* __restrict__ vt,
                                                     float* __restrict__ v_pix) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Vt) return;
  const float u = vt[2 * i], v = flip_uv ? 1.f - vt[2 * i + 1] : vt[2 * i + 1];
  v_pix[3 * i] = u * (float)W;
  v_pix[3 * i + 1] = v * (float)H;
  v_pix[3 * i + 2] = 1.f;
}

// one thread per texel
__global__ __launch_bounds__(256) void uv_topology_kernel(int F, int Vt, int H, int W, int flip_uv,
                                                          const int32_t* __restrict__ face_img,
                                                          const int32_t* __restrict__ vi, const int32_t* __restrict__ vti,
                                                          const float* __restrict__ vt, int64_t* __restrict__ index_image,
                                                          int64_t* __restrict__ face_index_image,
                                                          float* __restrict__ bary_image, uint8_t* __restrict__ valid_mask) {
#pragma clang fp contract(off)   // bary_coords' products and differences, each rounded as the reference rounds them
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (c >= W || r >= H) return;
  const size_t p = (size_t)r * W + c;
  int f = face_img[p];
  int t0 = -1, t1 = -1, t2 = -1;
  if (f >= 0 && f < F) { t0 = vti[3 * f]; t1 = vti[3 * f + 1]; t2 = vti[3 * f + 2]; }
  if (t0 < 0 || t0 >= Vt || t1 < 0 || t1 >= Vt || t2 < 0 || t2 >= Vt) f = -1;
  int64_t i0 = -1, i1 = -1, i2 = -1;
  float b0 = 0.f, b1 = 0.f, b2 = 0.f;
  if (f >= 0) {
    i0 = vi[3 * f]; i1 = vi[3 * f + 1]; i2 = vi[3 * f + 2];
    const float px = ((float)c + 0.5f) / (float)W, py = ((float)r + 0.5f) / (float)H;
    const float ax = vt[2 * t0], bx = vt[2 * t1], cx = vt[2 * t2];
    float ay = vt[2 * t0 + 1], by = vt[2 * t1 + 1], cy = vt[2 * t2 + 1];
    if (flip_uv) { ay = 1.f - ay; by = 1.f - by; cy = 1.f - cy; }
    const float x = px - cx, x1 = ax - cx, x2 = bx - cx;
    const float y = py - cy, y1 = ay - cy, y2 = by - cy;
    float denom = y2 * x1 - y1 * x2;
    const float n0 = y2 * x - x2 * y;
    const float n1 = x1 * y - y1 * x;
    denom = denom >= 0.f ? fmaxf(denom, 1.0e-6f) : fminf(denom, -1.0e-6f);
    b0 = n0 / denom;
    b1 = n1 / denom;
    b2 = 1.f - b0 - b1;
  }
  index_image[3 * p] = i0; index_image[3 * p + 1] = i1; index_image[3 * p + 2] = i2;
  face_index_image[p] = f;
  bary_image[3 * p] = b0; bary_image[3 * p + 1] = b1; bary_image[3 * p + 2] = b2;
  valid_mask[p] = f >= 0;
}

// column pass: near[r, c] = the valid row nearest to r in column c (the upper one on a tie), -1 if the column has none
__global__ __launch_bounds__(64) void nearest_col_kernel(int H, int W, const uint8_t* __restrict__ valid,
                                                         int32_t* __restrict__ near) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= W) return;
  int last = -1;
  for (int r = 0; r < H; ++r) {
    const size_t p = (size_t)r * W + c;
    if (valid[p]) last = r;
    near[p] = last;
  }
  int next = -1;
  for (int r = H - 1; r >= 0; --r) {
    const size_t p = (size_t)r * W + c;
    if (valid[p]) next = r;
    const int up = near[p];
    near[p] = up < 0 ? next : (next < 0 || r - up <= next - r) ? up : next;
  }
}

constexpr int kRowChunk = 256;  // columns of a row staged per round (a window of 256 + 2 dmax columns takes several)

// row pass: one workgroup per 256 texels of a row
__global__ __launch_bounds__(256) void nearest_row_kernel(int H, int W, int dmax, long long max_d2,
                                                          const uint8_t* __restrict__ valid,
                                                          const int32_t* __restrict__ near, int32_t* __restrict__ src) {
  __shared__ int32_t s_near[kRowChunk];
  const int tid = threadIdx.x, r = blockIdx.y, c0 = blockIdx.x * 256, c = c0 + tid;
  const int c_last = min(c0 + 255, W - 1);
  const int lo = max(0, c0 - dmax), hi = min(W - 1, c_last + dmax);   // the columns any texel of this workgroup can reach
  const bool want = c < W && !valid[(size_t)r * W + c];
  long long best_d2 = -1;
  int best_row = 0, best_col = 0;
  for (int base = lo; base <= hi; base += kRowChunk) {
    const int n = min(kRowChunk, hi - base + 1);
    __syncthreads();
    for (int i = tid; i < n; i += 256) s_near[i] = near[(size_t)r * W + base + i];
    __syncthreads();
    // offsets c' - c that reach this chunk from some texel of the workgroup (uniform bounds, per-lane predicate)
    const int off_lo = max(-dmax, base - c_last), off_hi = min(dmax, base + n - 1 - c0);
    if (want) {
      for (int off = off_lo; off <= off_hi; ++off) {
        const int i = c + off - base;
        if (i < 0 || i >= n) continue;
        const int nr = s_near[i];   // consecutive lanes, consecutive words: no bank conflict
        if (nr < 0) continue;
        const long long g = r - nr;
        const long long d2 = (long long)off * off + g * g;
        // columns ascend: on equal (d2, row) the earlier (smaller) column stays
        if (best_d2 < 0 || d2 < best_d2 || (d2 == best_d2 && nr < best_row)) { best_d2 = d2; best_row = nr; best_col = c + off; }
      }
    }
  }
  if (c < W) src[(size_t)r * W + c] = (want && best_d2 >= 0 && best_d2 <= max_d2) ? best_row * W + best_col : -1;
}

// up to three images of 4-byte words, w words per texel: out[p] = in[src[p] >= 0 ? src[p] : p]
struct GatherImg { int w; const uint32_t* in; uint32_t* out; };
struct GatherArgs { GatherImg img[3]; };

__global__ __launch_bounds__(256) void impaint_gather_kernel(long long P, const int32_t* __restrict__ src, GatherArgs a) {
  const GatherImg g = a.img[blockIdx.y];
  if (g.w <= 0 || g.in == nullptr) return;
  const long long n = P * g.w, stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const long long p = i / g.w;
    const int k = (int)(i - p * g.w);
    const int s = src[p];
    g.out[i] = g.in[(s >= 0 && s < P ? (long long)s : p) * g.w + k];
  }
}

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" int64_t gol_uv_face_index_workspace_bytes(int Vt, int F, int H, int W) {
  // the rasteriser's workspace | v_pix[Vt,3] | its depth image (not kept)
  if (Vt < 0 || F < 0 || H < 0 || W < 0) return 0;
  return (int64_t)(align16((size_t)gol_mesh_raster_workspace_bytes(1, F)) + align16((size_t)Vt * 3 * sizeof(float)) +
                   align16((size_t)H * W * sizeof(float)));
}

extern "C" int gol_uv_face_index(int Vt, int F, int H, int W, int flip_uv, const float* vt, const int32_t* vti,
                                 int32_t* face_img, void* workspace, void* stream) {
  GOL_REQUIRE(Vt >= 0 && F >= 0 && H > 0 && W > 0, "bad size");
  GOL_REQUIRE((long long)H * W < 2147483647LL, "image too large");
  GOL_REQUIRE(face_img != nullptr && workspace != nullptr, "null output or workspace");
  GOL_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  GOL_REQUIRE(Vt == 0 || vt != nullptr, "null vt");
  GOL_REQUIRE(F == 0 || vti != nullptr, "null vti");
  hipStream_t s = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace);
  float* v_pix = reinterpret_cast<float*>(ws + align16((size_t)gol_mesh_raster_workspace_bytes(1, F)));
  float* depth = reinterpret_cast<float*>(reinterpret_cast<char*>(v_pix) + align16((size_t)Vt * 3 * sizeof(float)));
  if (Vt > 0) uv_pix_kernel<<<gol_cdiv(Vt, 256), 256, 0, s>>>(Vt, H, W, flip_uv, vt, v_pix);
  GOL_CHECK_LAUNCH();
  return gol_mesh_raster_flat(1, Vt, F, H, W, v_pix, vti, face_img, depth, workspace, stream);
}

extern "C" int gol_uv_topology(int F, int Vt, int H, int W, int flip_uv, const int32_t* face_img, const int32_t* vi,
                               const int32_t* vti, const float* vt, int64_t* index_image, int64_t* face_index_image,
                               float* bary_image, uint8_t* valid_mask, void* stream) {
  GOL_REQUIRE(Vt >= 0 && F >= 0 && H > 0 && W > 0, "bad size");
  GOL_REQUIRE((long long)H * W < 2147483647LL && H <= 4 * 65535, "image too large");
  GOL_REQUIRE(face_img && index_image && face_index_image && bary_image && valid_mask, "null image");
  GOL_REQUIRE(F == 0 || (vi && vti && vt), "null input");
  uv_topology_kernel<<<dim3(gol_cdiv(W, 64), gol_cdiv(H, 4)), 256, 0, (hipStream_t)stream>>>(
      F, Vt, H, W, flip_uv, face_img, vi, vti, vt, index_image, face_index_image, bary_image, valid_mask);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_nearest_valid(int H, int W, int64_t max_d2, const uint8_t* valid, int32_t* col_near, int32_t* src,
                                 void* stream) {
  GOL_REQUIRE(H > 0 && W > 0, "bad size");
  GOL_REQUIRE((long long)H * W < 2147483647LL && H <= 65535, "image too large");
  GOL_REQUIRE(valid && col_near && src, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  // dmax = floor(sqrt(max_d2)), clipped to the image: a column farther away cannot hold an accepted source
  long long dmax = 0;
  if (max_d2 > 0) {
    const long long cap = W - 1;
    dmax = (long long)sqrt((double)max_d2);
    if (dmax > cap) dmax = cap;
    while (dmax < cap && (dmax + 1) * (dmax + 1) <= max_d2) ++dmax;
    while (dmax > 0 && dmax * dmax > max_d2) --dmax;
  }
  nearest_col_kernel<<<gol_cdiv(W, 64), 64, 0, s>>>(H, W, valid, col_near);
  nearest_row_kernel<<<dim3(gol_cdiv(W, 256), H), 256, 0, s>>>(H, W, (int)dmax, (long long)max_d2, valid, col_near, src);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_impaint_gather(int64_t P, const int32_t* src, int w0, const uint32_t* in0, uint32_t* out0, int w1,
                                  const uint32_t* in1, uint32_t* out1, int w2, const uint32_t* in2, uint32_t* out2,
                                  void* stream) {
  GOL_REQUIRE(P >= 0 && P < 2147483647LL, "bad size");
  GOL_REQUIRE(w0 >= 0 && w1 >= 0 && w2 >= 0, "bad word count");
  GOL_REQUIRE((in0 == nullptr) == (out0 == nullptr) && (in1 == nullptr) == (out1 == nullptr) &&
                  (in2 == nullptr) == (out2 == nullptr), "an image needs both its input and its output");
  GOL_REQUIRE(in0 != out0 || in0 == nullptr, "in place is not supported");
  GOL_REQUIRE((in1 != out1 || in1 == nullptr) && (in2 != out2 || in2 == nullptr), "in place is not supported");
  if (P == 0) return GOL_OK;
  GOL_REQUIRE(src != nullptr, "null src");
  GatherArgs a;
  a.img[0] = {w0, in0, out0};
  a.img[1] = {w1, in1, out1};
  a.img[2] = {w2, in2, out2};
  const int wmax = w0 > w1 ? (w0 > w2 ? w0 : w2) : (w1 > w2 ? w1 : w2);
  if (wmax == 0) return GOL_OK;
  const long long blocks = (P * wmax + 255) / 256;
  impaint_gather_kernel<<<dim3((unsigned)(blocks < 8192 ? blocks : 8192), 3), 256, 0, (hipStream_t)stream>>>((long long)P, src, a);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
