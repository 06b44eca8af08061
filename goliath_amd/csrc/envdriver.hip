// envdriver.hip -- the per-frame work of the env-relight driver (EnvSpinDecorator.forward), forward only, gfx950.
//
// Replaces ca_code/utils/light_decorator.py:120-143 with what it calls, ca_code/utils/envmap.py:141-166 rotate_envmap_mat:
// per view and frame the reference resamples the whole 3 x 512 x 1024 map with a CPU grid_sample, takes a percentile of it,
// reduces it to the 16 x 32 light probe with an antialiased CPU interpolate and uploads a 6 MB background.  Here:
//   launch 1  rotate_kernel    every pixel of every view: direction, rotation, u / v, bilinear border lookup; writes the
//                              background envbg (16-byte stores) and the unscaled rotated map into scratch
//   launch 2  probe_kernel     one workgroup per (view, probe cell): the cell's window of the rotated map times the outer
//                              product of the two 1-D tap tables, all three channels, summed in a fixed order
//   launch 3  finalize_kernel  one workgroup per view: S = sum probe sin((i + 0.5) pi / 16), then envmap, light_intensity,
//                              norm_scale and (view 0) the frame's mip scale, left in device memory for gol_shade_in
// Angles, the lookup position and the bilinear blend are evaluated in double and rounded once (as envbg.hip does: the
// position in a 1024-wide map then carries no float32 rounding of atan2 / acos); the window sums and S run in double over
// the float32 rotated map.  No atomics: each output has one owner, sums go through gol_block_sum.
#include "gol_stream.h"

#include <math.h>

namespace {

using namespace gol_stream;

constexpr int PROBE_H = 16, PROBE_W = 32, PROBE = PROBE_H * PROBE_W;   // light_decorator.py:128-130
constexpr int THREADS = 256, WAVES = THREADS / GOL_WAVE;
constexpr int PIX = 4;   // adjacent pixels (flat index inside a plane) per lane of launch 1: one 16-byte store per plane

struct Rot { double r[9]; };

// envmap.py:147-164 for pixel (y, x) of an H x W map: the direction of the OUTPUT pixel, rotated, looked up in `image`
// [3,H,W] with grid_sample(bilinear, align_corners=False, padding_mode="border").
__device__ __forceinline__ void rotated_sample(const float* __restrict__ image, int H, int W, const Rot& R, double st,
                                               double ct, int x, float out[3]) {
  const double kPi = 3.1415926;                       // envmap.py:148-149: the truncated constant
  const double inv_pi = 0.31830988618379067154;       // :158-159 use 1 / np.pi
  const double phi = ((double)(x - W / 2) + 0.5) * kPi * 2.0 / (double)W;
  double sp, cp;
  sincos(phi, &sp, &cp);
  const double vx = st * sp, vy = ct, vz = st * cp;   // :152
  // :154-155 matmul(vec, rot_mat.T): out_j = sum_k vec_k rot[j][k]
  double dx = R.r[0] * vx + R.r[1] * vy + R.r[2] * vz;
  double dy = R.r[3] * vx + R.r[4] * vy + R.r[5] * vz;
  double dz = R.r[6] * vx + R.r[7] * vy + R.r[8] * vz;
  dx = fmin(fmax(dx, -1.0), 1.0);                     // :156
  dy = fmin(fmax(dy, -1.0), 1.0);
  dz = fmin(fmax(dz, -1.0), 1.0);
  const double u = atan2(dx, dz) * inv_pi;            // :158
  const double v = 2.0 * (acos(dy) * inv_pi) - 1.0;   // :159-160
  // grid_sample, align_corners=False: ((g + 1) size - 1) / 2, border padding clips the POSITION to [0, size - 1]
  const double ix = fmin(fmax(((u + 1.0) * (double)W - 1.0) * 0.5, 0.0), (double)(W - 1));
  const double iy = fmin(fmax(((v + 1.0) * (double)H - 1.0) * 0.5, 0.0), (double)(H - 1));
  const double fx = floor(ix), fy = floor(iy);
  const double wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
  const int x0 = (int)fx, y0 = (int)fy;
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);   // the tap beyond the border carries weight 0
  const int plane = H * W;
  const float* r0 = image + y0 * W;
  const float* r1 = image + y1 * W;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double t00 = r0[c * plane + x0], t01 = r0[c * plane + x1], t10 = r1[c * plane + x0], t11 = r1[c * plane + x1];
    out[c] = (float)(wy0 * (wx0 * t00 + wx1 * t01) + wy1 * (wx0 * t10 + wx1 * t11));
  }
}

// ---- launch 1.  grid (cdiv(H W, 4 x 256), B); a lane owns PIX consecutive pixels of the flat plane.  VEC: H W % 4 == 0 and
// both destinations 16-byte aligned -> one f4 store per plane; otherwise scalar stores behind a bound test -----------------
template <bool VEC>
__global__ __launch_bounds__(THREADS) void rotate_kernel(int H, int W, const float* __restrict__ image,
                                                         const float* __restrict__ rot, float perc90,
                                                         float* __restrict__ rotated, float* __restrict__ envbg) {
  const int b = blockIdx.y;
  const int HW = H * W;
  const int p0 = (blockIdx.x * THREADS + threadIdx.x) * PIX;
  if (p0 >= HW) return;
  Rot R;
#pragma unroll
  for (int i = 0; i < 9; ++i) R.r[i] = (double)rot[b * 9 + i];   // wave-uniform: scalar loads
  float val[3][PIX];
  int yprev = -1;
  double st = 0.0, ct = 1.0;
#pragma unroll
  for (int k = 0; k < PIX; ++k) {
    const int p = min(p0 + k, HW - 1);   // (a lane past the end repeats the last pixel; its stores are masked below)
    const int y = p / W, x = p - y * W;
    if (y != yprev) {
      sincos(((double)y + 0.5) * 3.1415926 / (double)H, &st, &ct);   // envmap.py:148
      yprev = y;
    }
    float c[3];
    rotated_sample(image, H, W, R, st, ct, x, c);
    val[0][k] = c[0];
    val[1][k] = c[1];
    val[2][k] = c[2];
  }
  const size_t base = (size_t)b * 3 * HW + p0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float bg[PIX];
#pragma unroll
    for (int k = 0; k < PIX; ++k) bg[k] = ((val[c][k] / perc90) * 255.f) / 255.f;   // light_decorator.py:124-126, :159
    const size_t o = base + (size_t)c * HW;
    if (VEC) {
      *reinterpret_cast<gf4*>(global_out(rotated + o)) = f4{val[c][0], val[c][1], val[c][2], val[c][3]};
      if (envbg) *reinterpret_cast<gf4*>(global_out(envbg + o)) = f4{bg[0], bg[1], bg[2], bg[3]};
    } else {
#pragma unroll
      for (int k = 0; k < PIX; ++k) {
        if (p0 + k < HW) {
          rotated[o + k] = val[c][k];
          if (envbg) envbg[o + k] = bg[k];
        }
      }
    }
  }
}

// ---- launch 2.  grid (512, B).  Cell (i, j) = sum_{ky, kx} wy[i][ky] wx[j][kx] rotated[c][ys[i] + ky][xs[j] + kx]: thread t
// takes the window elements t, t + 256, ... (row-major inside the window) of all three channels, then three fixed-order
// workgroup sums.  Rows / columns are clamped to the map: a table can not make the kernel read outside it ----------------
__global__ __launch_bounds__(THREADS) void probe_kernel(int H, int W, const float* __restrict__ rotated,
                                                        const int32_t* __restrict__ tap_y_start,
                                                        const double* __restrict__ tap_y_w, int ky,
                                                        const int32_t* __restrict__ tap_x_start,
                                                        const double* __restrict__ tap_x_w, int kx,
                                                        double* __restrict__ probe) {
  __shared__ double sh[WAVES];
  const int cell = blockIdx.x, b = blockIdx.y;
  const int i = cell / PROBE_W, j = cell - i * PROBE_W;
  const int ys = tap_y_start[i], xs = tap_x_start[j];
  const double* wy = tap_y_w + (size_t)i * ky;
  const double* wx = tap_x_w + (size_t)j * kx;
  const size_t HW = (size_t)H * W;
  const float* src = rotated + (size_t)b * 3 * HW;
  double acc[3] = {0.0, 0.0, 0.0};
  const int n = ky * kx;
  for (int e = threadIdx.x; e < n; e += THREADS) {
    const int ry = e / kx, rx = e - ry * kx;
    const double w = wy[ry] * wx[rx];
    const int y = min(max(ys + ry, 0), H - 1), x = min(max(xs + rx, 0), W - 1);
    const size_t o = (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += w * (double)src[c * HW + o];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = gol_block_sum<double, WAVES>(acc[c], sh);
    if (threadIdx.x == 0) probe[((size_t)b * 3 + c) * PROBE + cell] = s;
  }
}

// ---- launch 3.  grid B.  light_decorator.py:132-143 and :151-153 ------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void finalize_kernel(const double* __restrict__ probe, double env_scale,
                                                           float* __restrict__ envmap, float* __restrict__ light_intensity,
                                                           float* __restrict__ norm_scale, float* __restrict__ mip_scale) {
  __shared__ double sh[WAVES];
  __shared__ double total;
  const int b = blockIdx.x, t = threadIdx.x;
  const double* p = probe + (size_t)b * 3 * PROBE;
  double acc = 0.0;
  for (int e = t; e < 3 * PROBE; e += THREADS) {
    const int row = (e % PROBE) / PROBE_W;
    acc += p[e] * sin(((double)row + 0.5) * 3.14159265358979323846 / (double)PROBE_H);   // :132-137
  }
  const double s = gol_block_sum<double, WAVES>(acc, sh);
  if (t == 0) total = s;
  __syncthreads();
  const double S = total;
  for (int e = t; e < 3 * PROBE; e += THREADS) {
    const int c = e / PROBE, cell = e - c * PROBE;
    const float v = (float)(env_scale * p[e] / S);                                        // :138
    envmap[(size_t)b * 3 * PROBE + e] = v;
    light_intensity[((size_t)b * PROBE + cell) * 3 + c] = v;                              // :143 view(3, -1).t()
  }
  if (t == 0) {
    const float ns = (float)(env_scale / S);                                              // :139
    norm_scale[b] = ns;
    // :151-153.  Rounded ONCE from the double product: a float32 product of float32(2 pi) and the rounded norm_scale can be
    // off by more than an ulp, which is more than the reference's own float32 result sometimes is
    if (b == 0) mip_scale[0] = (float)(6.283185307179586 * (env_scale / S));
  }
}


}  // namespace

extern "C" int64_t gol_envspin_scratch_floats(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  // the rotated map [B,3,H,W] (float), then the probe [B,3,16,32] in double
  return (int64_t)B * 3 * H * W + 2 * (int64_t)B * 3 * PROBE;
}

extern "C" int gol_envspin_frame(int B, int H, int W, const float* image, const float* rot, const int32_t* tap_y_start,
                                 const double* tap_y_w, int ky, const int32_t* tap_x_start, const double* tap_x_w, int kx,
                                 float perc90, double env_scale, float* scratch, float* envbg, float* envmap,
                                 float* light_intensity, float* norm_scale, float* mip_scale, void* stream) {
  GOL_REQUIRE(B >= 0, "bad sizes");
  GOL_REQUIRE(H >= PROBE_H && W >= PROBE_W && W % 2 == 0, "the map must be at least 16 x 32 with an even width");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(image && rot && tap_y_start && tap_y_w && tap_x_start && tap_x_w, "null input");
  GOL_REQUIRE(scratch && envmap && light_intensity && norm_scale && mip_scale, "null output");
  GOL_REQUIRE(ky >= 1 && ky <= H && kx >= 1 && kx <= W, "tap counts must be 1 ... H and 1 ... W");
  GOL_REQUIRE(B <= 65535, "B > 65535");
  GOL_REQUIRE((long long)H * W * 3 < (1ll << 31), "map too large");
  GOL_REQUIRE((long long)ky * kx < (1ll << 31), "window too large");
  GOL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "scratch must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long long HW = (long long)H * W;
  float* rotated = scratch;
  double* probe = reinterpret_cast<double*>(scratch + (size_t)B * 3 * HW);   // B 3 H W is even (W is): 8-byte aligned
  const dim3 grid(gol_cdiv(HW, PIX * THREADS), B);
  if (HW % PIX == 0 && gol_aligned16(rotated) && (!envbg || gol_aligned16(envbg)))
    rotate_kernel<true><<<grid, THREADS, 0, st>>>(H, W, image, rot, perc90, rotated, envbg);
  else
    rotate_kernel<false><<<grid, THREADS, 0, st>>>(H, W, image, rot, perc90, rotated, envbg);
  GOL_CHECK_LAUNCH();
  probe_kernel<<<dim3(PROBE, B), THREADS, 0, st>>>(H, W, rotated, tap_y_start, tap_y_w, ky, tap_x_start, tap_x_w, kx, probe);
  GOL_CHECK_LAUNCH();
  finalize_kernel<<<B, THREADS, 0, st>>>(probe, env_scale, envmap, light_intensity, norm_scale, mip_scale);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
