// envprefilter.hip -- the SG prefilter of an environment map (one level of the relight pyramid), forward only, gfx950.
//
// Replaces ca_code/utils/envmap.py:305-323 prefilterEnvmapSG with what it calls per sample, :251-281 importance_sample_sg
// and :284-302 dir2uv / sample_uv: a Python loop over the samples, each iteration two dozen ATen kernels, boolean-mask
// writes (a host sync each) and a grid_sample over the whole level.  Here:
//   launch 1  pack_kernel       the planar [B,3,He,We] map -> [B,He,We,4] texels of 16 bytes in scratch: a bilinear corner is
//                               one 16-byte load for all three channels
//   launch 2  prefilter_kernel  ONE WAVE PER OUTPUT TEXEL, four waves per workgroup.  The frame (t, b) of the texel is formed
//                               once, from wave-uniform loads; lane l takes the samples l, l + 64, ... in ascending order and
//                               adds their colours in double; the 64 partial sums of each channel go through the DPP ladder
//                               (gol_wave_sum_to_lane63) and lane 63 writes the mean, rounded once.  No LDS, no atomics: the
//                               order of every sum is fixed by S alone, not by the grid.
// The smallest level of the pyramid (64 x 128) is 8192 waves = 8 per SIMD of a 256-CU part, so splitting a texel's samples
// over the lanes of a wave fills the machine where one lane per texel would leave it at 1/64.
// Everything is evaluated in double from the float32 inputs (as envdriver.hip and envbg.hip do): phi, erfinv, the frame,
// the normalisation, atan2 / acos, the lookup position and the blend.  The reference's float32 error sits in the lookup
// POSITION (u carries 6e-8, times We / 2 texels, times a texel-to-texel step of the order of the map's maximum); a float32
// kernel in another evaluation order would have an error of the same size and no reason to stay inside 2 x the reference's.
// The draws when no xi is given: Philox-4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11), key =
// (seed low, seed high), counter = (g low, g high, texel, b) with g = sample_offset + i; outputs 0 and 1, each >> 8 and
// times 2^-24.
#include "gol_common.h"

#include <math.h>

namespace {

constexpr int THREADS = 256, WAVES = THREADS / GOL_WAVE;

typedef float f4 __attribute__((ext_vector_type(4)));

// ---- launch 1.  One lane per texel of the map ---------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void pack_kernel(int B, int HWe, const float* __restrict__ env,
                                                       f4* __restrict__ packed) {
  const int e = blockIdx.x * THREADS + threadIdx.x;   // B HWe < 2^29
  if (e >= B * HWe) return;
  const int b = e / HWe, p = e - b * HWe;
  const float* src = env + (size_t)b * 3 * HWe + p;
  packed[e] = f4{src[0], src[HWe], src[2 * (size_t)HWe], 0.f};
}

struct Philox2 { float x, y; };

__device__ __forceinline__ Philox2 philox_uniform2(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                                   uint32_t c3) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Philox2{(float)(c0 >> 8) * 0x1p-24f, (float)(c1 >> 8) * 0x1p-24f};
}

struct Frame { double t[3], b[3], n[3]; };

// envmap.py:272-278, the operations as torch.cross / F.normalize order them and not contracted: where a component is an
// exact zero (n on the z axis) its SIGN decides on which border of the map atan2 puts the sample
__device__ __forceinline__ Frame make_frame(float nxf, float nyf, float nzf) {
#pragma clang fp contract(off)
  Frame f;
  const double nx = nxf, ny = nyf, nz = nzf;
  const bool m = nzf < 0.999f;
  const double ux = m ? 0.0 : 1.0, uy = 0.0, uz = m ? 1.0 : 0.0;
  const double cx = uy * nz - uz * ny, cy = uz * nx - ux * nz, cz = ux * ny - uy * nx;
  const double len = fmax(sqrt(cx * cx + cy * cy + cz * cz), 1e-12);
  f.t[0] = cx / len, f.t[1] = cy / len, f.t[2] = cz / len;
  f.b[0] = ny * f.t[2] - nz * f.t[1];
  f.b[1] = nz * f.t[0] - nx * f.t[2];
  f.b[2] = nx * f.t[1] - ny * f.t[0];
  f.n[0] = nx, f.n[1] = ny, f.n[2] = nz;
  return f;
}

// ---- launch 2.  grid cdiv(B H W, 4); wave w of a workgroup owns texel 4 blockIdx.x + w --------------------------------------
__global__ __launch_bounds__(THREADS) void prefilter_kernel(int B, int HW, int He, int We, int S, double sqrt2sigma,
                                                            double erf_cut, const float* __restrict__ v,
                                                            const f4* __restrict__ packed, const float* __restrict__ xi,
                                                            uint32_t seed_lo, uint32_t seed_hi, uint64_t sample_offset,
                                                            float* __restrict__ out) {
  const int lane = threadIdx.x & (GOL_WAVE - 1);
  const int texel = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES + threadIdx.x / GOL_WAVE);   // b HW + p, < 2^31
  if (texel >= B * HW) return;                                                                     // (the whole wave)
  const int b = texel / HW, p = texel - b * HW;
  const float* vb = v + (size_t)b * 3 * HW + p;
  const Frame f = make_frame(vb[0], vb[HW], vb[2 * (size_t)HW]);
  const f4* map = packed + (size_t)b * He * We;
  const double inv_pi = 0.31830988618379067154;   // envmap.py:289-290 use 1 / np.pi
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
  for (int i = lane; i < S; i += GOL_WAVE) {
    float x0f, x1f;
    if (xi) {
      const float* x = xi + (((size_t)i * B + b) * 2) * HW + p;
      x0f = x[0];
      x1f = x[HW];
    } else {
      const uint64_t g = sample_offset + (uint64_t)i;
      const Philox2 r = philox_uniform2(seed_lo, seed_hi, (uint32_t)g, (uint32_t)(g >> 32), (uint32_t)p, (uint32_t)b);
      x0f = r.x;
      x1f = r.y;
    }
    // :259-267
    double sp, cp, st, ct;
    sincospi(2.0 * (double)x0f, &sp, &cp);
    const double theta = sqrt2sigma * erfinv((double)x1f * erf_cut);
    sincospi(theta * inv_pi, &st, &ct);   // theta in [0, pi]: no large-argument reduction to carry along
    const double hx = cp * st, hy = sp * st, hz = ct;
    // :280-281
    double dx = f.t[0] * hx + f.b[0] * hy + f.n[0] * hz;
    double dy = f.t[1] * hx + f.b[1] * hy + f.n[1] * hz;
    double dz = f.t[2] * hx + f.b[2] * hy + f.n[2] * hz;
    const double len = fmax(sqrt(dx * dx + dy * dy + dz * dz), 1e-12);
    dx /= len, dy /= len, dz /= len;
    // :289-291; the clamp is this kernel's (the reference's acos gives NaN an ulp outside)
    const double u = inv_pi * atan2(dx, dz);
    const double w = 2.0 * (inv_pi * acos(fmin(fmax(dy, -1.0), 1.0))) - 1.0;
    // grid_sample, align_corners=False: ((g + 1) size - 1) / 2; border padding clips the POSITION to [0, size - 1].  fmax /
    // fmin drop a NaN, so no input can move a fetch outside the map
    const double ix = fmin(fmax(((u + 1.0) * (double)We - 1.0) * 0.5, 0.0), (double)(We - 1));
    const double iy = fmin(fmax(((w + 1.0) * (double)He - 1.0) * 0.5, 0.0), (double)(He - 1));
    const double fx = floor(ix), fy = floor(iy);
    const double wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
    const int tx0 = (int)fx, ty0 = (int)fy;
    const int tx1 = min(tx0 + 1, We - 1), ty1 = min(ty0 + 1, He - 1);   // the tap beyond the border carries weight 0
    const f4 t00 = map[ty0 * We + tx0], t01 = map[ty0 * We + tx1], t10 = map[ty1 * We + tx0], t11 = map[ty1 * We + tx1];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      acc[c] += wy0 * (wx0 * (double)t00[c] + wx1 * (double)t01[c]) + wy1 * (wx0 * (double)t10[c] + wx1 * (double)t11[c]);
  }
  // lanes that took no sample (S < 64) add exact zeros
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = gol_wave_sum_to_lane63(acc[c]);
    if (lane == GOL_WAVE - 1) out[((size_t)b * 3 + c) * HW + p] = (float)(s / (double)S);
  }
}

}  // namespace

extern "C" int64_t gol_envprefilter_scratch_floats(int B, int He, int We) {
  if (B <= 0 || He <= 0 || We <= 0) return 0;
  return 4 * (int64_t)B * He * We;
}

extern "C" int gol_envprefilter_sg(int B, int H, int W, int He, int We, int S, double sigma, const float* v,
                                   const float* env_tex, const float* xi, int64_t seed, int64_t sample_offset,
                                   float* scratch, float* out, void* stream) {
  GOL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && He >= 1 && We >= 1, "bad sizes");
  GOL_REQUIRE(S >= 1, "num_samples must be at least 1");
  GOL_REQUIRE(sigma > 0.0 && sigma < INFINITY, "sigma must be positive and finite");
  GOL_REQUIRE(v && env_tex && scratch && out, "null pointer");
  GOL_REQUIRE(sample_offset >= 0, "sample_offset must not be negative");
  GOL_REQUIRE((long long)B * H * W < (1ll << 31) - THREADS, "B H W too large");
  GOL_REQUIRE(4ll * B * He * We < (1ll << 31), "map too large");
  GOL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "scratch must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int HWe = He * We, HW = H * W;
  f4* packed = reinterpret_cast<f4*>(scratch);
  pack_kernel<<<gol_cdiv((long long)B * HWe, THREADS), THREADS, 0, st>>>(B, HWe, env_tex, packed);
  GOL_CHECK_LAUNCH();
  const double sqrt2sigma = sqrt(2.0) * sigma;                        // envmap.py:261
  const double erf_cut = erf(3.14159265358979323846 / sqrt2sigma);   // :262 math.erf(np.pi / sqrt2sigma)
  const uint64_t sd = (uint64_t)seed;
  prefilter_kernel<<<gol_cdiv((long long)B * HW, WAVES), THREADS, 0, st>>>(
      B, HW, He, We, S, sqrt2sigma, erf_cut, v, packed, xi, (uint32_t)sd, (uint32_t)(sd >> 32), (uint64_t)sample_offset, out);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
