// gol_raster.h -- tile / wave / staging helpers shared by the tile rasterizers (raster.hip: 3 channels + extra,
// raster_nd.hip: C channels).  Everything here is inline and file-local (anonymous namespace): each kernel file gets its
// own copy, exactly as when it lived in raster.hip.
#pragma once
#include "gol_common.h"

namespace {

constexpr int kBatch = 256;
// conics are staged in LDS pre-multiplied by log2(e) -- alpha = opacity * 2^(-sigma') is one v_exp_f32 with a negated
// operand instead of a multiply + exp per pixel -- and the diagonal terms by the 1/2 of sigma = (a dx^2 + c dy^2) / 2 +
// b dx dy as well (GOL_SC_A / GOL_SC_B, applied where the records are written); kUnA / kUnB bring the true conic back
// where the backward needs it
constexpr float kUnA = GOL_UN_A, kUnB = GOL_UN_B;
#ifdef GOL_EXACT_MATH
// TEST-ONLY exact-math twin (goliath_amd/build.py, variant "exact"): the conic is staged unscaled, sigma is evaluated in
// the order the CPU oracle (and gsplat) writes it -- 0.5 (a dx^2 + c dy^2) + b dx dy, every product and sum rounded
// separately -- exp goes through double precision (correctly rounded to fp32) and the transmittance recurrence is
// T (1 - alpha) instead of T - alpha T.  With bit-identical inputs the alpha >= 1/255 and T <= 1e-4 decisions then
// coincide with the oracle's: what remains between the two is rounding noise, no threshold flips.
__device__ __forceinline__ float exact_sigma(float a, float b, float c, float dx, float dy) {
#pragma clang fp contract(off)
  const float t1 = (a * dx) * dx, t2 = (c * dy) * dy, t3 = (b * dx) * dy;
  const float h = 0.5f * (t1 + t2);
  return h + t3;
}
__device__ __forceinline__ float exact_exp_neg(float s) { return (float)exp(-(double)s); }
__device__ __forceinline__ float exact_next_T(float T, float alpha) {
#pragma clang fp contract(off)
  const float om = 1.f - alpha;
  return T * om;
}
#endif

struct TileCoord { int tile, tx, ty; bool ok; };

// XCD-aware remap.  Consecutive workgroups land on different XCDs (observed: block b -> XCD b % 8), so
// XCD x is given tile rows x, x+8, x+16, ...: inside a die consecutive workgroups walk along a tile
// row (neighbouring tiles share most of their Gaussians -> L2 hits), while the rows of every die are
// spread over the whole image so the dies stay balanced (contiguous image eighths per die left most of
// the chip idle: the head covers only the middle rows).  Speed only -- any mapping is correct.
__device__ __forceinline__ TileCoord tile_of_block(int bid, int T, int tiles_x) {
  const int tiles_y = T / tiles_x;
  const int xcd = bid & 7, j = bid >> 3;
  TileCoord tc;
  const int row_local = j / tiles_x;
  tc.tx = j - row_local * tiles_x;
  tc.ty = row_local * 8 + xcd;
  tc.ok = tc.ty < tiles_y;
  tc.tile = tc.ty * tiles_x + tc.tx;
  return tc;
}

typedef float f1 __attribute__((ext_vector_type(1)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef int i1 __attribute__((ext_vector_type(1)));
typedef int i2 __attribute__((ext_vector_type(2)));

// Wave footprints.  PPL = pixels per lane.
//   PPL = 2 (the default): 2 waves per 16x16 tile, wave w owns the 16x8 half (rows 8w..8w+7), lane = (x = lane & 15, row
//           pair lane >> 4) owns two vertically adjacent pixels -- the per-pixel recurrences run on 2-vectors (packed fp32
//           VALU ops) and the per-Gaussian work of a visit is shared by 128 pixels: the fewest instructions per pixel.
//   PPL = 1 (round 4, launches of one or two views): 4 waves per tile, wave w owns the 8x8 quadrant (x half w & 1, y half
//           w >> 1), one pixel per lane.  ~9 % more instructions in total, but a wave's chain through the tile's list -- which
//           IS the duration of a single-view launch: 2942 non-empty tiles of 670 entries on average and up to 1280 fit on
//           the chip at once, the launch ends when the longest list does (measured: raster_bwd 227 us for one view, 131 us
//           per view in an 8-view launch; with every list clipped to 512 entries 130 us) -- is ~0.55x as long: the 8x8
//           footprint is culled against 21 % more entries and a visit costs ~0.7x the instructions.
template <int PPL> struct Pix;
template <> struct Pix<2> { typedef f2 fv; typedef i2 iv; static constexpr int kWaves = 2; };
template <> struct Pix<1> { typedef f1 fv; typedef i1 iv; static constexpr int kWaves = 4; };

template <int PPL>
__device__ __forceinline__ void wave_rect(int wave, float tile_x0, float tile_y0, float& x0, float& x1, float& y0, float& y1) {
  if (PPL == 2) {
    x0 = tile_x0 + 0.5f; x1 = x0 + 15.f; y0 = tile_y0 + (float)(wave * 8) + 0.5f; y1 = y0 + 7.f;
  } else {
    x0 = tile_x0 + (float)((wave & 1) * 8) + 0.5f; x1 = x0 + 7.f; y0 = tile_y0 + (float)((wave >> 1) * 8) + 0.5f; y1 = y0 + 7.f;
  }
}

// bit w of the mask = the alpha >= 1/255 region of a Gaussian can reach the footprint of wave w:
// exact ellipse-vs-rectangle test (minimum of sigma over the footprint's pixel centres against ln(255*opacity)),
// conservative only by a rounding margin; degenerate conics -> all.  tau, 1/a, 1/c and the validity flag come from the
// record (gol_common.h: computed once per Gaussian by the projection).
template <int PPL>
__device__ __forceinline__ int wave_mask(float gx, float gy, float ca, float cb, float cc, float tau, float ia, float ic,
                                         float exact, float tile_x0, float tile_y0) {
  constexpr int NW = Pix<PPL>::kWaves;
  if (!(tau >= 0.f)) return 0;  // alpha < 1/255 everywhere (also NaN opacity: skipped by gsplat too)
  if (exact == 0.f) return (1 << NW) - 1;
  int m = 0;
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    float x0, x1, y0, y1;
    wave_rect<PPL>(q, tile_x0, tile_y0, x0, x1, y0, y1);
    const float ms = gol_min_sigma_rect(gx, gy, ca, cb, cc, ia, ic, x0, x1, y0, y1);
    m |= (ms <= tau) ? (1 << q) : 0;
  }
  return m;
}

// pixel coordinates of a lane: column j, first row i0 (the lane's PPL pixels are rows i0 .. i0 + PPL - 1)
template <int PPL>
__device__ __forceinline__ void lane_pixel(int tx, int ty, int wave, int lane, int& j, int& i0) {
  if (PPL == 2) { j = tx * 16 + (lane & 15); i0 = ty * 16 + wave * 8 + (lane >> 4) * 2; }
  else { j = tx * 16 + (wave & 1) * 8 + (lane & 7); i0 = ty * 16 + (wave >> 1) * 8 + (lane >> 3); }
}

// stage one list entry: four 16-byte loads from the Gaussian's 64-byte record
// LDS row of a staged list entry: a = (x, y, conic a', conic b'), b = (conic c', opacity, r, g), c = (b, extra)
struct __attribute__((aligned(16))) StagedRow { float4 a, b; float2 c; float2 pad; };

struct Staged { float4 a, b; float2 c; int mask; };
template <int PPL>
__device__ __forceinline__ Staged stage_entry(const float* __restrict__ records, size_t g, float tile_x0, float tile_y0) {
  const float4* R = reinterpret_cast<const float4*>(records + g * GOL_SPLAT_RECORD);
  const float4 q0 = R[0], q1 = R[1], q2 = R[2], q3 = R[3];
  Staged s;
  s.a = q0;                              // x, y, a', b'
  s.b = q1;                              // c', opacity, r, g
  s.c = make_float2(q2.x, q2.y);         // b, extra
  s.mask = wave_mask<PPL>(q0.x, q0.y, q0.z * kUnA, q0.w * kUnB, q1.x * kUnA, q2.z, q2.w, q3.x, q3.y, tile_x0, tile_y0);
  return s;
}

template <typename V, int P>
__device__ __forceinline__ bool any_live(const V& live) {
  unsigned u = 0u;
#pragma unroll
  for (int q = 0; q < P; ++q) u |= __float_as_uint(live[q]);
  return u != 0u;
}

}  // namespace
