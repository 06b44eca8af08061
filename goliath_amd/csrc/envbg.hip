// envbg.hip -- the environment background of the relight visualisation (compose_envmap), forward only, gfx950.
//
// Replaces ca_code/utils/envmap.py:325-345 compose_envmap and what it calls: envmap_to_image (:169-227, without the
// fisheye `D` path) and envmap_to_mirrorball (:230-248).  The reference runs, per view, a bicubic grid_sample at full
// resolution, a depthwise 101 x 101 conv2d (10,201 taps per pixel for a filter that is the outer product of one 101-tap
// vector with itself), a second bicubic lookup for the mirror ball and some ten elementwise kernels.  Here:
//   gol_envbg_image    sample (1 launch) [+ row pass + column pass of the separable blur, 202 taps per pixel]
//   gol_envbg_compose  composite + mirror ball in one pass
// Directions, angles and the sampling coordinates are evaluated in double (a few hundred operations per pixel -- noise next
// to the blur): the lookup position in a 1024-wide map then carries no float32 rounding of atan2 / acos.  The bicubic
// weights (A = -0.75, PyTorch's grid_sample) and all sums are float32.
#include "gol_common.h"

namespace {

constexpr int TAPS = 101;    // envmap.py:220  linspace(-4, 4, 101)
constexpr int HALO = 50;     // conv2d(padding=50): ZERO padding
constexpr int ROW_W = 256;   // row pass: one workgroup = ROW_R rows x 256 columns, strip + halo in LDS
constexpr int ROW_R = 8;
constexpr int ROW_Q = 4;     // adjacent outputs per lane of the row pass
constexpr int COL_W = 64;    // column pass: one workgroup = 64 rows x 64 columns; every LDS / global row segment is 64 floats
constexpr int COL_H = 64;
constexpr int COL_Q = 4;     // outputs per register block of the column pass (each staged value feeds up to 4 sums)

struct Taps { float k[TAPS]; };   // by-value kernel argument: a tap is a scalar operand, not a load per lane
// k[i] == k[100 - i] bit for bit (gol_envbg_blur_taps): the kernels read the lower half only, 51 scalar registers
__device__ __forceinline__ float tap(const Taps& taps, int t) { return taps.k[t < TAPS - 1 - t ? t : TAPS - 1 - t]; }

// ---- PyTorch's bicubic grid_sample: cubic convolution, A = -0.75 ----------------------------------------------------
__device__ __forceinline__ void cubic_weights(double t, float w[4]) {
  const double A = -0.75;
  double x = t + 1.0;
  w[0] = (float)(((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A);
  x = t;
  w[1] = (float)(((A + 2.0) * x - (A + 3.0)) * x * x + 1.0);
  x = 1.0 - t;
  w[2] = (float)(((A + 2.0) * x - (A + 3.0)) * x * x + 1.0);
  x = 2.0 - t;
  w[3] = (float)(((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A);
}

// env[3,He,We] of one view, looked up in direction (dx, dy, dz): u = atan2(dx, dz) / pi, v = 2 acos(dy) / pi - 1,
// grid_sample(mode='bicubic', padding_mode='border', align_corners=True): the position is NOT clipped, each of the 4 x 4
// tap indices is.  acos' argument is clamped (the reference returns NaN beyond +-1).
__device__ __forceinline__ void env_lookup(const float* __restrict__ env, int He, int We, double dx, double dy, double dz,
                                           float out[3]) {
  const double inv_pi = 0.31830988618379067154;
  const double u = atan2(dx, dz) * inv_pi;
  const double v = 2.0 * (acos(fmin(fmax(dy, -1.0), 1.0)) * inv_pi) - 1.0;
  const double ix = (u + 1.0) * 0.5 * (double)(We - 1);
  const double iy = (v + 1.0) * 0.5 * (double)(He - 1);
  const double fx = floor(ix), fy = floor(iy);
  float wx[4], wy[4];
  cubic_weights(ix - fx, wx);
  cubic_weights(iy - fy, wy);
  const int x0 = (int)fx - 1, y0 = (int)fy - 1;
  int xi[4], yi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xi[i] = min(max(x0 + i, 0), We - 1);
    yi[i] = min(max(y0 + i, 0), He - 1);
  }
  const int plane = He * We;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* row = env + c * plane + yi[j] * We;
      const float r = row[xi[0]] * wx[0] + row[xi[1]] * wx[1] + row[xi[2]] * wx[2] + row[xi[3]] * wx[3];
      acc += r * wy[j];
    }
    out[c] = acc;
  }
}

// out_y = sum_x R[x][y] d[x]  (einsum "bxy,bhwx->bhwy": the transpose of the camera rotation)
__device__ __forceinline__ void rotate_t(const float* __restrict__ R, double x, double y, double z, double& ox, double& oy,
                                         double& oz) {
  ox = (double)R[0] * x + (double)R[3] * y + (double)R[6] * z;
  oy = (double)R[1] * x + (double)R[4] * y + (double)R[7] * z;
  oz = (double)R[2] * x + (double)R[5] * y + (double)R[8] * z;
}

// ---- launch 1: the environment seen through every pixel, dst[B,3,H,W] ---------------------------------------------------
__global__ __launch_bounds__(256) void sample_kernel(int H, int W, int He, int We, const float* __restrict__ envbg,
                                                     const float* __restrict__ K, const float* __restrict__ R,
                                                     double focal_scale, float* __restrict__ dst) {
  const int b = blockIdx.y;
  const int HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const float* Kb = K + b * 9;
  double dx = ((double)x - (double)Kb[2]) / ((double)Kb[0] * focal_scale);
  double dy = ((double)y - (double)Kb[5]) / ((double)Kb[4] * focal_scale);
  double rx, ry, rz;
  rotate_t(R + b * 9, dx, dy, 1.0, rx, ry, rz);
  const double inv = 1.0 / fmax(sqrt(rx * rx + ry * ry + rz * rz), 1e-12);   // F.normalize's eps
  float c[3];
  env_lookup(envbg + (size_t)b * 3 * He * We, He, We, rx * inv, ry * inv, rz * inv, c);
  float* o = dst + (size_t)b * 3 * HW + p;
  o[0] = c[0];
  o[HW] = c[1];
  o[2 * (size_t)HW] = c[2];
}

// ---- launch 2: 101 taps along x.  grid (cdiv(W,256), cdiv(H,8), B*3); a lane owns 4 adjacent columns of a row (a wave one
// 256-wide row, the four waves four rows at a time): 26 ds_read_b128 feed 4 x 101 FMAs, each staged value up to 4 sums ------
__global__ __launch_bounds__(256) void blur_row_kernel(int H, int W, const float* __restrict__ src, float* __restrict__ dst,
                                                       const Taps taps) {
  __shared__ __attribute__((aligned(16))) float s[ROW_R][ROW_W + 2 * HALO];   // 356 floats per row: rows stay 16-byte aligned
  const int x0 = blockIdx.x * ROW_W, y0 = blockIdx.y * ROW_R;
  const size_t plane = (size_t)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < ROW_R * (ROW_W + 2 * HALO); i += 256) {
    const int r = i / (ROW_W + 2 * HALO), c = i - r * (ROW_W + 2 * HALO);
    const int gx = x0 - HALO + c, gy = y0 + r;
    s[r][c] = (gx >= 0 && gx < W && gy < H) ? src[plane + (size_t)gy * W + gx] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gx = x0 + ROW_Q * lane;
#pragma unroll 1
  for (int r = wave; r < ROW_R; r += 4) {
    const float4* row = reinterpret_cast<const float4*>(&s[r][ROW_Q * lane]);
    float acc[ROW_Q];
#pragma unroll
    for (int q = 0; q < ROW_Q; ++q) acc[q] = 0.f;
#pragma unroll
    for (int m = 0; m < (TAPS + ROW_Q - 1 + 3) / 4; ++m) {   // 26 x 4 = the 104 staged values the 4 outputs read
      const float4 v4 = row[m];
      const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < ROW_Q; ++q)
          if (4 * m + e - q >= 0 && 4 * m + e - q < TAPS) acc[q] += tap(taps, 4 * m + e - q) * v[e];
    }
    if (y0 + r < H) {
      float* o = dst + plane + (size_t)(y0 + r) * W + gx;
#pragma unroll
      for (int q = 0; q < ROW_Q; ++q)
        if (gx + q < W) o[q] = acc[q];
    }
  }
}

// ---- launch 3: 101 taps along y.  grid (cdiv(W,64), cdiv(H,64), B*3); a lane owns one column of the tile and 16 of its
// rows, every LDS and global access is a 64-float row segment ---------------------------------------------------------------
__global__ __launch_bounds__(256) void blur_col_kernel(int H, int W, const float* __restrict__ src, float* __restrict__ dst,
                                                       const Taps taps) {
  __shared__ float s[COL_H + 2 * HALO][COL_W];   // 164 x 64 floats = 41,984 bytes
  const int x0 = blockIdx.x * COL_W, y0 = blockIdx.y * COL_H;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const int cx = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int gx = x0 + cx;
  for (int r = g; r < COL_H + 2 * HALO; r += 4) {
    const int gy = y0 - HALO + r;
    s[r][cx] = (gx < W && gy >= 0 && gy < H) ? src[plane + (size_t)gy * W + gx] : 0.f;
  }
  __syncthreads();
  constexpr int PER = COL_H / 4;   // 16 output rows per lane
#pragma unroll 1
  for (int o = g * PER; o < (g + 1) * PER; o += COL_Q) {
    float acc[COL_Q];
#pragma unroll
    for (int q = 0; q < COL_Q; ++q) acc[q] = 0.f;
#pragma unroll
    for (int j = 0; j < TAPS + COL_Q - 1; ++j) {
      const float v = s[o + j][cx];
#pragma unroll
      for (int q = 0; q < COL_Q; ++q)
        if (j - q >= 0 && j - q < TAPS) acc[q] += tap(taps, j - q) * v;
    }
#pragma unroll
    for (int q = 0; q < COL_Q; ++q) {
      const int gy = y0 + o + q;
      if (gx < W && gy < H) dst[plane + (size_t)gy * W + gx] = acc[q];
    }
  }
}

// ---- composite + mirror ball: out = render + (1 - alpha) clamp(bg, 0, 1); the bottom-right ball x ball pixels inside the
// unit disc show the environment reflected by a sphere (envmap.py:230-248) -------------------------------------------------
__global__ __launch_bounds__(256) void compose_kernel(int H, int W, int He, int We, const float* __restrict__ render,
                                                      const float* __restrict__ alpha, const float* __restrict__ bg,
                                                      const float* __restrict__ envbg, const float* __restrict__ R, int ball,
                                                      float* __restrict__ out) {
  const int b = blockIdx.y;
  const int HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const size_t base = (size_t)b * 3 * HW + p;
  const float one_minus_a = 1.f - alpha[(size_t)b * HW + p];
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float v = fminf(fmaxf(bg[base + (size_t)k * HW], 0.f), 1.f);
    c[k] = render[base + (size_t)k * HW] + one_minus_a * v;
  }
  const int bx = x - (W - ball), by = y - (H - ball);
  if (ball > 0 && bx >= 0 && by >= 0) {
    // torch.linspace(-1, 1, ball): from the start in the lower half, from the end in the upper half
    const double step = ball > 1 ? 2.0 / (double)(ball - 1) : 0.0;
    const double px = bx < ball / 2 ? -1.0 + step * bx : 1.0 - step * (ball - 1 - bx);
    const double py = by < ball / 2 ? -1.0 + step * by : 1.0 - step * (ball - 1 - by);
    const double zsq = px * px + py * py;
    if (zsq < 1.0) {
      const double nz = -sqrt(fmax(1.0 - zsq, 0.0));
      const double rx0 = -2.0 * nz * px, ry0 = -2.0 * nz * py, rz0 = -2.0 * nz * nz + 1.0;
      double rx, ry, rz;
      rotate_t(R + b * 9, rx0, ry0, rz0, rx, ry, rz);   // (not normalised, like the reference)
      env_lookup(envbg + (size_t)b * 3 * He * We, He, We, rx, ry, rz, c);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out[base + (size_t)k * HW] = c[k];
}

}  // namespace

// k[i] = exp(-t_i^2) / sum_j exp(-t_j^2), t = linspace(-4, 4, 101): the reference's 2-D kernel is the outer product of k
// with itself, normalised by the 2-D sum = (sum k)^2
extern "C" int gol_envbg_blur_taps(double* taps) {
  GOL_REQUIRE(taps, "null pointer");
  const double step = 8.0 / (TAPS - 1);
  double sum = 0.0;
  for (int i = 0; i < TAPS; ++i) {
    const double t = i < TAPS / 2 ? -4.0 + step * i : 4.0 - step * (TAPS - 1 - i);
    taps[i] = exp(-t * t);
  }
  for (int i = 0; i < TAPS / 2; ++i) sum += taps[i] + taps[TAPS - 1 - i];   // symmetric pairs, smallest first
  sum += taps[TAPS / 2];
  for (int i = 0; i < TAPS; ++i) taps[i] /= sum;
  return GOL_OK;
}

extern "C" int64_t gol_envbg_scratch_floats(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return 2 * (int64_t)B * 3 * H * W;
}

extern "C" int gol_envbg_image(int B, int H, int W, int He, int We, const float* envbg, const float* K, const float* R,
                               double focal_scale, int blur, float* scratch, float* bg, void* stream) {
  GOL_REQUIRE(B >= 0 && H >= 0 && W >= 0, "bad sizes");
  if (B == 0 || H == 0 || W == 0) return GOL_OK;
  GOL_REQUIRE(He >= 1 && We >= 1, "empty environment map");
  GOL_REQUIRE(envbg && K && R && bg, "null pointer");
  GOL_REQUIRE(blur == 0 || blur == 1, "blur must be 0 or 1");
  GOL_REQUIRE(!blur || scratch, "blur needs gol_envbg_scratch_floats(B,H,W) floats of scratch");
  GOL_REQUIRE((long long)B * 3 <= 65535, "B*3 > 65535");
  GOL_REQUIRE((long long)H * W < (1ll << 31) && (long long)He * We * 3 < (1ll << 31), "image or map too large");
  GOL_REQUIRE(gol_cdiv(H, ROW_R) <= 65535 && gol_cdiv(H, COL_H) <= 65535, "H too large");
  hipStream_t st = (hipStream_t)stream;
  const size_t planes = (size_t)B * 3 * H * W;
  float* s0 = blur ? scratch : bg;
  sample_kernel<<<dim3(gol_cdiv((long long)H * W, 256), B), 256, 0, st>>>(H, W, He, We, envbg, K, R, focal_scale, s0);
  GOL_CHECK_LAUNCH();
  if (!blur) return GOL_OK;
  double kd[TAPS];
  gol_envbg_blur_taps(kd);
  Taps taps;
  for (int i = 0; i < TAPS; ++i) taps.k[i] = (float)kd[i];
  float* s1 = scratch + planes;
  blur_row_kernel<<<dim3(gol_cdiv(W, ROW_W), gol_cdiv(H, ROW_R), B * 3), 256, 0, st>>>(H, W, s0, s1, taps);
  GOL_CHECK_LAUNCH();
  blur_col_kernel<<<dim3(gol_cdiv(W, COL_W), gol_cdiv(H, COL_H), B * 3), 256, 0, st>>>(H, W, s1, bg, taps);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_envbg_compose(int B, int H, int W, int He, int We, const float* render, const float* alpha,
                                 const float* bg, const float* envbg, const float* R, int ball, float* out, void* stream) {
  GOL_REQUIRE(B >= 0 && H >= 0 && W >= 0, "bad sizes");
  if (B == 0 || H == 0 || W == 0) return GOL_OK;
  GOL_REQUIRE(render && alpha && bg && out, "null pointer");
  GOL_REQUIRE(ball >= 0 && ball <= H && ball <= W, "the mirror ball does not fit into the image");
  GOL_REQUIRE(ball == 0 || (envbg && R && He >= 1 && We >= 1), "the mirror ball needs the environment map and R");
  GOL_REQUIRE(B <= 65535, "B > 65535");
  GOL_REQUIRE((long long)H * W < (1ll << 31) && (long long)He * We * 3 < (1ll << 31), "image or map too large");
  compose_kernel<<<dim3(gol_cdiv((long long)H * W, 256), B), 256, 0, (hipStream_t)stream>>>(H, W, He, We, render, alpha, bg,
                                                                                         envbg, R, ball, out);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
