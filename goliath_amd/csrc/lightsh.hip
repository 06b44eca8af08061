// lightsh.hip -- head-relative light positions and the SH light coefficients of a frame in ONE launch, forward only, gfx950.
//
// Replaces ca_code/models/rgca.py:175-191 (AutoEncoder.forward) and :590-613 (PrimDecoder.forward's random back-light) with
// what they call, ca_code/utils/sh.py:118-127 dir2sh_torch.  The reference evaluates the (deg+1)^2 real spherical harmonics
// one function at a time -- each a chain of tiny elementwise kernels over [B,L], each starting with a device-to-host sync
// (`th.max(th.abs(x)) > 1.0`, sh.py:55).  Here a lane owns a light and builds all of its basis values by the same
// recurrences (sh.py:54-78), for every order m at once:
//   gol_sh_basis_fwd   dirs[M,3] -> coeffs[M,(deg+1)^2]                                    (dir2sh_torch)
//   gol_light_sh_fwd   a workgroup per batch element: (p - t) @ R, F.normalize, the basis, and the intensity-weighted sum
//                      over the lights through LDS in a fixed order (no atomics: bitwise repeatable)
// The problem is tiny (a few thousand lights) and latency-bound: what counts is the ONE launch.  Loops run to the
// compile-time degree 8 and are fully unrolled -- the recurrence state is a handful of registers; a smaller `deg` only
// skips the stores (wave-uniform tests).
#include "gol_common.h"

#include <math.h>

namespace {

constexpr int MAXDEG = 8;                            // the reference's n_diff_sh
constexpr int MAXCOEF = (MAXDEG + 1) * (MAXDEG + 1);  // 81
constexpr int THREADS = 256;
constexpr int CHUNK = 128;   // lights staged per pass of the fused kernel: 128 x 81 floats = 41,472 bytes of LDS

struct ShNorm { float k[MAXCOEF]; };   // by-value kernel argument (gol_sh_norm_constants rounded to float32)

// All (deg+1)^2 values of one direction, written to out[n*n + n + m] (the reference's order: n outer, m = -n..n inner).
// sh.py's semantics, not a textbook's: theta = acos(clamp(z)), the Legendre argument cos(theta) = clamp(z, -1, 1);
// sin(theta) = sqrt(max((1 + x)(1 - x), 1e-8)) (a floor of 1e-4: m > 0 terms stay small but non-zero at the poles);
// phi = atan2(y, x) of the RAW components, so cos(m phi) / sin(m phi) come from the angle-addition recurrence on
// (x, y) / rho -- scaled by max(|x|, |y|) first so that rho neither under- nor overflows -- and atan2(+-0, +-0) is 0 or
// +-pi: cos = sign(x), sin = 0.  The direction itself is NOT normalised here (dir2sh_torch does not).
// NORM = false leaves the constant N out (the fused kernel applies it once per output, after the sum over the lights).
template <bool NORM>
__device__ __forceinline__ void sh_eval(float x, float y, float z, int deg, const ShNorm& nrm, float* __restrict__ out) {
  const float ct = fminf(fmaxf(z, -1.f), 1.f);
  const float st = sqrtf(fmaxf((1.f + ct) * (1.f - ct), 1e-8f));
  const float s = fmaxf(fabsf(x), fabsf(y));
  float cx = copysignf(1.f, x), sy = 0.f;
  if (s > 0.f) {
    const float xs = x / s, ys = y / s;             // the larger one is +-1: rho in [1, sqrt 2]
    const float ir = 1.f / sqrtf(xs * xs + ys * ys);
    cx = xs * ir;
    sy = ys * ir;
  }
  float cm = 1.f, sm = 0.f;   // cos(m phi), sin(m phi)
  float pmm = 1.f;            // P_m^m = (-1)^m (2m - 1)!! sin^m(theta)
#pragma unroll
  for (int m = 0; m <= MAXDEG; ++m) {
    if (m > 0) {
      const float c = cm * cx - sm * sy;
      sm = sm * cx + cm * sy;
      cm = c;
      pmm = -pmm * (float)(2 * m - 1) * st;
    }
    if (m > deg) break;
    float p0 = pmm, p1 = 0.f;   // P_{n-2}^m, P_{n-1}^m of the upward recurrence in n
#pragma unroll
    for (int n = m; n <= MAXDEG; ++n) {
      float p;
      if (n == m) {
        p = pmm;
      } else if (n == m + 1) {
        p = ct * (float)(2 * m + 1) * pmm;
        p1 = p;
      } else {
        p = (ct * (float)(2 * n - 1) * p1 - (float)(n + m - 1) * p0) * (1.f / (float)(n - m));
        p0 = p1;
        p1 = p;
      }
      if (n <= deg) {
        const int k = n * n + n;
        if (m == 0) {
          out[k] = NORM ? nrm.k[k] * p : p;
        } else {
          out[k + m] = NORM ? nrm.k[k + m] * cm * p : cm * p;
          out[k - m] = NORM ? nrm.k[k - m] * sm * p : sm * p;
        }
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void sh_basis_kernel(int M, int deg, const float* __restrict__ dirs,
                                                           float* __restrict__ coeffs, const ShNorm nrm) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= M) return;
  const int ncoef = (deg + 1) * (deg + 1);
  const float* d = dirs + (size_t)i * 3;
  sh_eval<true>(d[0], d[1], d[2], deg, nrm, coeffs + (size_t)i * ncoef);
}

// grid B.  Per chunk of CHUNK lights: lanes 0..CHUNK-1 (two waves) take one light each -- head-relative position,
// F.normalize, the un-normalised basis cos / sin(m phi) P_n^m into sY[light][ncoef], the intensity into sI[light][3]; then
// thread (c, k) of the first 3 ncoef adds its chunk's products in light order to its ONE accumulator, and multiplies by the
// constant N_k at the end (the 81 constants as scalar operands of the per-light code would not fit the SGPR file beside
// the rest).  A padded light (zero intensity) adds Y * 0 = +-0 to the accumulator: exactly nothing.
__global__ __launch_bounds__(THREADS) void light_sh_kernel(int L, int deg, int C, const float* __restrict__ light_pos,
                                                           const float* __restrict__ light_intensity,
                                                           const float* __restrict__ head_pose,
                                                           float* __restrict__ headrel_light_pos,
                                                           float* __restrict__ light_sh, const ShNorm nrm) {
  __shared__ float sY[CHUNK * MAXCOEF];
  __shared__ float sI[CHUNK * 3];
  const int b = blockIdx.x, t = threadIdx.x;
  const int ncoef = (deg + 1) * (deg + 1);
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, T[3] = {0.f, 0.f, 0.f};
  if (head_pose) {   // head_pose[b] = [R | t], 3 x 4 row-major (wave-uniform: scalar loads)
    const float* hp = head_pose + (size_t)b * 12;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i * 3 + j] = hp[i * 4 + j];
      T[i] = hp[i * 4 + 3];
    }
  }
  const int oc = t / ncoef, ok = t - oc * ncoef;   // this thread's output (channel, coefficient)
  const bool owner = t < 3 * ncoef;
  float acc = 0.f;
  for (int l0 = 0; l0 < L; l0 += CHUNK) {
    const int n = min(CHUNK, L - l0);
    if (t < n) {
      const size_t l = (size_t)b * L + l0 + t;
      const float* p = light_pos + l * 3;
      const float dx = p[0] - T[0], dy = p[1] - T[1], dz = p[2] - T[2];
      const float hx = dx * R[0] + dy * R[3] + dz * R[6];   // (p - t) @ R
      const float hy = dx * R[1] + dy * R[4] + dz * R[7];
      const float hz = dx * R[2] + dy * R[5] + dz * R[8];
      if (headrel_light_pos) {
        float* o = headrel_light_pos + l * 3;
        o[0] = hx;
        o[1] = hy;
        o[2] = hz;
      }
      const float inv = 1.f / fmaxf(sqrtf(hx * hx + hy * hy + hz * hz), 1e-12f);   // F.normalize's eps
      sh_eval<false>(hx * inv, hy * inv, hz * inv, deg, nrm, sY + t * ncoef);
      const float* in = light_intensity + l * C;
#pragma unroll
      for (int c = 0; c < 3; ++c) sI[t * 3 + c] = in[C == 3 ? c : 0];
    }
    __syncthreads();
    if (owner) {
#pragma unroll 4
      for (int j = 0; j < n; ++j) acc = fmaf(sY[j * ncoef + ok], sI[j * 3 + oc], acc);
    }
    __syncthreads();
  }
  if (owner) light_sh[((size_t)b * 3 + oc) * ncoef + ok] = nrm.k[ok] * acc;
}

ShNorm norm_f32() {
  double kd[MAXCOEF];
  gol_sh_norm_constants(MAXDEG, kd);
  ShNorm nrm;
  for (int i = 0; i < MAXCOEF; ++i) nrm.k[i] = (float)kd[i];
  return nrm;
}

}  // namespace

// KVal(|m|, n) = sqrt((2n + 1) / (4 pi) (n - |m|)! / (n + |m|)!) (sh.py:13-26), times sqrt(2) for m != 0 (sh.py:80-86)
extern "C" int gol_sh_norm_constants(int deg, double* out) {
  GOL_REQUIRE(deg >= 0 && deg <= MAXDEG, "deg must be 0 ... 8");
  GOL_REQUIRE(out, "null pointer");
  const double four_pi = 12.566370614359172954;
  for (int n = 0; n <= deg; ++n) {
    for (int m = -n; m <= n; ++m) {
      const int am = m < 0 ? -m : m;
      double prod = 1.0;   // (n + |m|)! / (n - |m|)!
      for (int i = n - am + 1; i <= n + am; ++i) prod *= (double)i;
      const double k = sqrt((double)(2 * n + 1) / four_pi * (1.0 / prod));
      out[n * n + n + m] = am ? sqrt(2.0) * k : k;
    }
  }
  return GOL_OK;
}

extern "C" int gol_sh_basis_fwd(int M, int deg, const float* dirs, float* coeffs, void* stream) {
  GOL_REQUIRE(M >= 0, "bad sizes");
  GOL_REQUIRE(deg >= 0 && deg <= MAXDEG, "deg must be 0 ... 8");
  if (M == 0) return GOL_OK;
  GOL_REQUIRE(dirs && coeffs, "null pointer");
  GOL_REQUIRE((long long)M * MAXCOEF < (1ll << 31), "M too large");
  sh_basis_kernel<<<gol_cdiv(M, THREADS), THREADS, 0, (hipStream_t)stream>>>(M, deg, dirs, coeffs, norm_f32());
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_light_sh_fwd(int B, int L, int deg, const float* light_pos, const float* light_intensity,
                                int intensity_channels, const float* head_pose, float* headrel_light_pos, float* light_sh,
                                void* stream) {
  GOL_REQUIRE(B >= 0 && L >= 0, "bad sizes");
  GOL_REQUIRE(deg >= 0 && deg <= MAXDEG, "deg must be 0 ... 8");
  GOL_REQUIRE(intensity_channels == 1 || intensity_channels == 3, "intensity_channels must be 1 or 3");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(light_sh && (L == 0 || (light_pos && light_intensity)), "null pointer");
  GOL_REQUIRE((long long)B * L * 3 < (1ll << 31), "B * L too large");
  light_sh_kernel<<<B, THREADS, 0, (hipStream_t)stream>>>(L, deg, intensity_channels, light_pos, light_intensity, head_pose,
                                                          headrel_light_pos, light_sh, norm_f32());
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
