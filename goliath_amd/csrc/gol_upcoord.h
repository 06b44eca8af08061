// gol_upcoord.h -- the integer-ratio coordinate rule of the exact 2x bilinear resize (align_corners=True), shared by the
// fp32 operators (gol_upconv.h: upconv.hip, upcat.hip) and the split-bf16 one (upconvx.hip): the row / column tables, the
// first row of U that reaches a source row, and the blend expression.  Lifted out of gol_upconv.h as it stood; it defines no
// tile constants, so it sits beside either family's core header.  Everything is inline and file-local.
#pragma once
#include "gol_common.h"

namespace {

// Tables of n rows (or columns) origin .. origin + n - 1 of U: source offsets a = r0 * mul, b = r1 * mul and the fraction;
// a = -1 marks a row outside [0, nout).
__device__ __forceinline__ void up_fill_axis(int* s_a, int* s_b, float* s_f, int n, int origin, int nsrc, int nout, int mul,
                                             int tid) {
  for (int t = tid; t < n; t += 256) {
    const int r = origin + t;
    int a = -1, b = 0;
    float f = 0.f;
    if (r >= 0 && r < nout) {
      const int nr = r * (nsrc - 1), d = nout - 1;  // (nout = 2 nsrc >= 2)
      const int q = nr / d;
      f = (float)(nr - q * d) / (float)d;
      a = q * mul;
      b = min(q + 1, nsrc - 1) * mul;
    }
    s_a[t] = a;
    s_b[t] = b;
    s_f[t] = f;
  }
}

// first row of U with r (nsrc-1)/(nout-1) > i - 1: no earlier row reaches source row i
__device__ __forceinline__ int up_first_row(int i, int nsrc, int nout) {
  return (i <= 0 || nsrc <= 1) ? 0 : ((i - 1) * (nout - 1)) / (nsrc - 1) + 1;
}

// U at row fraction fr, column fraction fc from its up-to-2x2 source texels: up_stage_u's expression (gol_upconv.h keeps it
// written out: calling this from there changes the register allocation of upconv.hip and upcat.hip, and they are to compile
// to what they compiled to before the rule moved here)
__device__ __forceinline__ float up_blend(float fr, float fc, float x00, float x01, float x10, float x11) {
  return (1.f - fr) * ((1.f - fc) * x00 + fc * x01) + fr * ((1.f - fc) * x10 + fc * x11);
}

}  // namespace
