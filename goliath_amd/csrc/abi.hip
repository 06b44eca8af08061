// abi.hip -- library identification and error reporting for libgoliath_hip.so.
#include <cstdarg>
#include <cstdio>

#include "gol_common.h"

static thread_local char g_err[512] = "";

void gol_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* gol_version(void) { return "goliath_hip 0.1.0 gfx950"; }
extern "C" const char* gol_last_error(void) { return g_err; }

// ---- self-test hook for the wave64 cross-lane primitives (tests/test_gpu_primitives.py) ----------
__global__ void selftest_wave_sum4_kernel(const float* __restrict__ in, float* __restrict__ out) {
  const int l = threadIdx.x;
  const float r = gol_wave_sum4(in[l], in[64 + l], in[128 + l], in[192 + l]);
  out[l] = r;
  out[64 + l] = gol_wave_sum_to_lane63(in[l]);
}
extern "C" int gol_selftest_wave_sum4(const float* in256, float* out128, void* stream) {
  selftest_wave_sum4_kernel<<<1, 64, 0, (hipStream_t)stream>>>(in256, out128);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

// in512: eight rows of 64 lane values; out64[l] = what gol_wave_sum8 returns in lane l (tests/test_gpu_wave_sum8.py)
__global__ void selftest_wave_sum8_kernel(const float* __restrict__ in, float* __restrict__ out) {
  const int l = threadIdx.x;
  out[l] = gol_wave_sum8(in[l], in[64 + l], in[128 + l], in[192 + l], in[256 + l], in[320 + l], in[384 + l], in[448 + l]);
}
extern "C" int gol_selftest_wave_sum8(const float* in512, float* out64, void* stream) {
  selftest_wave_sum8_kernel<<<1, 64, 0, (hipStream_t)stream>>>(in512, out64);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

// in384: six rows of 64 lane values (s0, s1, s2, m0, my, myy); dx64: the factor of every lane (equal in lanes l and l + 16);
// out64[l] = what gol_wave_colsum returns in lane l (tests/test_gpu_wave_colsum.py)
__global__ void selftest_wave_colsum_kernel(const float* __restrict__ in, const float* __restrict__ dx,
                                            float* __restrict__ out) {
  const int l = threadIdx.x;
  out[l] = gol_wave_colsum(in[l], in[64 + l], in[128 + l], in[192 + l], in[256 + l], in[320 + l], dx[l]);
}
extern "C" int gol_selftest_wave_colsum(const float* in384, const float* dx64, float* out64, void* stream) {
  selftest_wave_colsum_kernel<<<1, 64, 0, (hipStream_t)stream>>>(in384, dx64, out64);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
