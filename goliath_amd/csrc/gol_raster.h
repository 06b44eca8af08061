// gol_raster.h -- what the tile rasterizers (raster.hip: 3 channels + extra, raster_nd.hip: C channels) have in common.
// Tile / wave / staging helpers and the per-visit core that decides what is rendered: visit_falloff (sigma and
// exp(-sigma), the only GOL_EXACT_MATH branch of that math), fwd_step / fwd_take, bwd_taken / bwd_recur / bwd_moments /
// lane_sum, wave_last_entry, true_conic, and the host side of a launch (raster_grid,
// GOL_RASTER_CHECK_DIMS, with_ppl).  Per kernel stay the LDS layouts, batch sizes, colour sums and the LAZY bookkeeping of
// the fused forward.  Everything here is inline and file-local (anonymous namespace): each kernel file gets its own copy.
#pragma once
#include <type_traits>

#include "gol_common.h"

namespace {

constexpr int kBatch = 256;
// conics are staged in LDS pre-multiplied by log2(e) -- alpha = opacity * 2^(-sigma') is one v_exp_f32 with a negated
// operand instead of a multiply + exp per pixel -- and the diagonal terms by the 1/2 of sigma = (a dx^2 + c dy^2) / 2 +
// b dx dy as well (GOL_SC_A / GOL_SC_B, applied where the records are written); kUnA / kUnB bring the true conic back
// where the cull test and the backward's merges need it
constexpr float kUnA = GOL_UN_A, kUnB = GOL_UN_B;
__device__ __forceinline__ float3 true_conic(float a, float b, float c) { return make_float3(a * kUnA, b * kUnB, c * kUnA); }
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
//
// The groups of 8 tile rows are not walked from top to bottom either: with the head in the middle rows that order starts
// and ends every launch with bands of empty tiles, whose workgroups only write constants -- memory traffic with no busy
// tile resident beside it.  row_order deals the R groups out over the launch from the three thirds of the image in turn
// (top, middle, bottom, top, ...), so consecutive groups never come from the same third and the empty rows are spread
// evenly between the busy ones.  The top third is walked upwards from its last group, the other two downwards from their
// first: the launch begins next to the middle and the group left over when 3 does not divide R is the image's first --
// walked top to bottom it was the top third's last, and a launch of one view, whose duration is its longest lists' chain,
// ended on busy tiles with nothing beside them (--views 1: 1.2 % slower than the plain order, profiles/raster_row_order_ab.txt).
// A bijection on [0, R) for every R: the p with p % 3 == 0, 1, 2 number ceil(R / 3), ceil((R - 1) / 3) and
// ceil((R - 2) / 3), which are the lengths of the three bands laid end to end.
__device__ __forceinline__ int row_order(int p, int R) {
  const int band = p % 3, k = p / 3;
  const int n0 = (R + 2) / 3, n1 = (R + 1) / 3;
  return band == 0 ? n0 - 1 - k : k + n0 + (band > 1 ? n1 : 0);
}

__device__ __forceinline__ TileCoord tile_of_block(int bid, int T, int tiles_x) {
  const int tiles_y = T / tiles_x;
  const int xcd = bid & 7, j = bid >> 3;
  TileCoord tc;
  const int slot_row = j / tiles_x;
  tc.tx = j - slot_row * tiles_x;   // (the tiles of one row stay consecutive workgroups of one die)
  const int row_local = row_order(slot_row, (tiles_y + 7) >> 3);
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
  const float3 cn = true_conic(q0.z, q0.w, q1.x);
  s.mask = wave_mask<PPL>(q0.x, q0.y, cn.x, cn.y, cn.z, q2.z, q2.w, q3.x, q3.y, tile_x0, tile_y0);
  return s;
}
// the same with the wave mask the forward of this render left for the entry (its staging ran wave_mask<PPL> on the same
// tile, record and footprints: the same bits): no reach test, and the record's last 16 bytes are not read
__device__ __forceinline__ Staged stage_entry_masked(const float* __restrict__ records, size_t g, int mask) {
  const float4* R = reinterpret_cast<const float4*>(records + g * GOL_SPLAT_RECORD);
  const float4 q0 = R[0], q1 = R[1], q2 = R[2];
  Staged s;
  s.a = q0; s.b = q1; s.c = make_float2(q2.x, q2.y); s.mask = mask;
  return s;
}

template <typename V, int P>
__device__ __forceinline__ bool any_live(const V& live) {
  unsigned u = 0u;
#pragma unroll
  for (int q = 0; q < P; ++q) u |= __float_as_uint(live[q]);
  return u != 0u;
}

// ---- the per-visit core: one wave looks at one staged list entry ---------------------------------------------------------
template <int PPL> using fvec = typename Pix<PPL>::fv;
template <int PPL> using ivec = typename Pix<PPL>::iv;

// sigma of the (staged) conic at the lane's pixels and e = exp(-gsplat's sigma); alpha = opacity * e
template <int PPL>
__device__ __forceinline__ void visit_falloff(float ca, float cb, float cc, float dx, const fvec<PPL>& dy, fvec<PPL>& sigma,
                                              fvec<PPL>& e) {
#ifndef GOL_EXACT_MATH
  sigma = (ca * dx * dx + cc * dy * dy) + (cb * dx) * dy;  // log2e * gsplat's sigma
#pragma unroll
  for (int q = 0; q < PPL; ++q) e[q] = __builtin_amdgcn_exp2f(-sigma[q]);
#else
#pragma unroll
  for (int q = 0; q < PPL; ++q) { sigma[q] = exact_sigma(ca, cb, cc, dx, dy[q]); e[q] = exact_exp_neg(sigma[q]); }
#endif
}

// Forward: what the entry does to each pixel.  alpha = min(cap, opacity * e); live = 1 while the pixel composites.
// Yields vis = alpha T (unmasked), next_T = T (1 - alpha), take[] and the lane masks of the pixels that stop here;
// returns the union of those masks.
template <int PPL>
__device__ __forceinline__ unsigned long long fwd_step(const fvec<PPL>& sigma, fvec<PPL> alpha, const fvec<PPL>& live,
                                                       const fvec<PPL>& T_cur, fvec<PPL>& vis, fvec<PPL>& next_T,
                                                       bool (&take)[PPL], unsigned long long (&stop)[PPL]) {
  alpha *= live;
  vis = alpha * T_cur;
#ifndef GOL_EXACT_MATH
  next_T = T_cur - vis;  // = T (1 - alpha)
#else
#pragma unroll
  for (int q = 0; q < PPL; ++q) next_T[q] = exact_next_T(T_cur[q], alpha[q]);
#endif
  // contributes: !(sigma < 0 || alpha < 1/255); stops: T (1 - alpha) <= 1e-4 (the stopping entry is not taken); one
  // compare per pixel -- all as scalar lane masks (ballots of the plain compares; written with bools the compiler issues
  // a second, NaN-aware compare for the negation).  (An early-out for visits without a taker, as the backward has it,
  // does not pay here: 602-612 vs 613 us)
  unsigned long long any_stop = 0ull;
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    const unsigned long long mc = gol_ballot(!(sigma[q] < 0.f)) & gol_ballot(!(alpha[q] < GOL_ALPHA_FLOOR));
    const unsigned long long ms = gol_ballot(next_T[q] <= GOL_T_STOP);
    take[q] = __builtin_amdgcn_inverse_ballot_w64(mc & ~ms);
    stop[q] = mc & ms;
    any_stop |= stop[q];
  }
  return any_stop;
}

// Forward: vis becomes the taken pixels' weight (0 elsewhere) and T advances where the entry is taken
template <int PPL>
__device__ __forceinline__ void fwd_take(const bool (&take)[PPL], const fvec<PPL>& next_T, fvec<PPL>& vis, fvec<PPL>& T_cur) {
#pragma unroll
  for (int q = 0; q < PPL; ++q) vis[q] = take[q] ? vis[q] : 0.f;
#ifndef GOL_EXACT_MATH
  T_cur -= vis;                   // unchanged where the entry is not taken
#else
#pragma unroll
  for (int q = 0; q < PPL; ++q) T_cur[q] = take[q] ? next_T[q] : T_cur[q];
#endif
}

// Backward: raw = opacity e, the uncapped alpha, and the lane masks mv[] of the pixels that took entry li (within the pixel's
// list && !(sigma < 0 || alpha < 1/255): ballots of the plain compares, the ballot of a combined bool costs a v_cndmask +
// v_cmp); returns their union.  The alpha of the test is min(cap, raw); the compare is made on raw itself, which decides the
// same for every input: the cap lies above 1/255, so min(cap, raw) < 1/255 exactly when raw < 1/255, and a NaN raw (v_min
// returns the cap for it) is "not below" either way.
template <int PPL>
__device__ __forceinline__ unsigned long long bwd_taken(float opacity, const fvec<PPL>& e, const fvec<PPL>& sigma, int li,
                                                        const ivec<PPL>& bin_final, fvec<PPL>& raw,
                                                        unsigned long long (&mv)[PPL]) {
  static_assert(GOL_ALPHA_CAP_BWD > GOL_ALPHA_FLOOR, "bwd_taken tests the uncapped alpha against the floor");
  raw = opacity * e;
  unsigned long long many = 0ull;
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    mv[q] = gol_ballot(li <= bin_final[q]) & gol_ballot(!(sigma[q] < 0.f)) & gol_ballot(!(raw[q] < GOL_ALPHA_FLOOR));
    many |= mv[q];
  }
  return many;
}

// Backward: T steps back over the entry (T_cur becomes the transmittance in front of it); ra = 1 / (1 - alpha),
// fac = alpha T = the entry's compositing weight.  The ONE mask of a visit is applied here, to raw: it leaves as raw_m.
template <int PPL>
__device__ __forceinline__ void bwd_recur(const unsigned long long (&mv)[PPL], fvec<PPL>& raw, fvec<PPL>& T_cur,
                                          fvec<PPL>& alpha, fvec<PPL>& ra, fvec<PPL>& fac) {
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    // an entry the pixel did not take enters with raw_m = 0 and so with alpha = 0: 1 / (1 - 0) = 1 exactly, so T and the
    // running sums pass through unchanged without further selects (the composite R of bwd_moments likewise), and its gop,
    // a multiple of raw_m, is 0 as well
    raw[q] = __builtin_amdgcn_inverse_ballot_w64(mv[q]) ? raw[q] : 0.f;
    // min(cap, raw_m), written as the instruction: fminf on the result of a select is compiled to v_max x, x (a
    // canonicalisation that the product under the select does not need) + v_min, and v_med3 wants the cap in a register
    asm("v_min_f32_e32 %0, %2, %1" : "=v"(alpha[q]) : "v"(raw[q]), "i"(__builtin_bit_cast(int, GOL_ALPHA_CAP_BWD)));
  }
  const fvec<PPL> one_m = 1.f - alpha;
#pragma unroll
  for (int q = 0; q < PPL; ++q) ra[q] = __builtin_amdgcn_rcpf(one_m[q]);
  const fvec<PPL> T_new = T_cur * ra;
  fac = alpha * T_new;
  T_cur = T_new;
}

// Backward: v_alpha and gop = raw_m v_alpha with its first two moments in dy, per pixel (lane_sum adds a lane's pixels up).
// gsplat: v_alpha = sum_c (rgb_c T - buffer_c ra) v_out_c + T_final ra (v_out_alpha - <bg, v_out>) with buffer_c = sum over
// the Gaussians behind of rgb_c alpha T.  All channels enter through ONE dot product with the upstream gradient, w =
// <colour, v_out>, so the colour buffers collapse into a running scalar q = sum_behind fac w and v_alpha = T w - ra (q - tail),
// tail = T_final (v_out_alpha - <bg, v_out>).  With T_behind = T (1 - alpha), the transmittance behind the entry,
// ra (q - tail) = T R for R = (q - tail) / T_behind: R is the back-to-front COMPOSITE of w over what lies behind the entry
// (background included) and is carried instead of q and tail --
//   v_alpha = T (w - R),   R <- R (1 - alpha) + alpha w = R + alpha (w - R),   R_start = <bg, v_out> - v_out_alpha
// -- one running quantity, no T_final factor, no division, and no difference of two sums scaled up by ra when alpha is
// near its cap.  An entry the pixel did not take has alpha = 0 (bwd_recur) and leaves R as it is.
// d loss / d sigma per pixel is -opacity e v_alpha = -gop: gop carries the (wave-uniform) opacity already, because the
// masked quantity is raw_m = opacity e (0 for a pixel that did not take the entry: no select here).  The lanes reduce the
// moments of gop; the merges negate them, and the zeroth moment is opacity * v_opacity (divided once per entry there)
template <int PPL>
__device__ __forceinline__ void bwd_moments(const fvec<PPL>& raw_m, const fvec<PPL>& w, const fvec<PPL>& T_cur,
                                            const fvec<PPL>& alpha, const fvec<PPL>& dy,
                                            fvec<PPL>& R, fvec<PPL>& gop, fvec<PPL>& gy, fvec<PPL>& gyy) {
  const fvec<PPL> d = w - R;
  const fvec<PPL> v_alpha = T_cur * d;
  R += alpha * d;
  gop = raw_m * v_alpha;
  gy = gop * dy;
  gyy = gy * dy;
}
template <int PPL>
__device__ __forceinline__ float lane_sum(const fvec<PPL>& x) {
  float s = x[0];
#pragma unroll
  for (int q = 1; q < PPL; ++q) s += x[q];
  return s;
}

// Backward start bound of a wave: the last list entry that any of its pixels took (wave-uniform)
template <int PPL>
__device__ __forceinline__ int wave_last_entry(const ivec<PPL>& bin_final) {
  int wmax = bin_final[0];
#pragma unroll
  for (int q = 1; q < PPL; ++q) wmax = max(wmax, bin_final[q]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) wmax = max(wmax, __shfl_xor(wmax, off, 64));
  return __builtin_amdgcn_readfirstlane(wmax);
}

// ---- host side of a launch -----------------------------------------------------------------------------------------------
// grid.x of every raster launch: one workgroup per tile slot per view, tile rows padded to a multiple of 8 (tile_of_block)
inline int64_t raster_grid(int B, int img_h, int img_w) {
  return (int64_t)B * 8 * (((img_h + 15) / 16 + 7) / 8) * ((img_w + 15) / 16);
}

// size checks of the four raster entries (a macro: GOL_REQUIRE names the entry it fails in); the kernels address a view's
// images with 32-bit byte offsets, bytes_per_pixel for the widest of them (0: the kernel has no such offsets)
#define GOL_RASTER_CHECK_DIMS(bytes_per_pixel, too_large_msg)                                                           \
  do {                                                                                                                  \
    GOL_REQUIRE(B >= 0 && N >= 0, "negative size");                                                                     \
    GOL_REQUIRE(block == 16, "only block_width == 16 is implemented (the reference's value, render_gsplat.py:28)");     \
    GOL_REQUIRE(img_h > 0 && img_w > 0, "empty image");                                                                 \
    GOL_REQUIRE(raster_grid(B, img_h, img_w) < (1ll << 31), "too many tiles");                                          \
    GOL_REQUIRE((uint64_t)img_h * (uint64_t)img_w * (uint64_t)(bytes_per_pixel) < (1ull << 32), too_large_msg);         \
  } while (0)

// fn(std::integral_constant<int, ppl>) for ppl = 1 | 2: a launch spells its argument list once
template <typename F>
inline void with_ppl(int ppl, F&& fn) {
  if (ppl == 2) fn(std::integral_constant<int, 2>());
  else fn(std::integral_constant<int, 1>());
}
constexpr std::true_type kYes{}; constexpr std::false_type kNo{};   // compile-time switches of a launch lambda

}  // namespace
