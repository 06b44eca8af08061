// gol_common.h -- device helpers shared by the gfx950 kernels of libgoliath_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>

#include "../../include/goliath_hip.h"

// ---- gsplat 0.1.11 constants; one place, named ------------------
#define GOL_BLUR 0.3f
#define GOL_FOV_CLAMP 1.3f
#define GOL_EIG_FLOOR 0.1f
#define GOL_RADIUS_SIGMAS 3.0f
#define GOL_Z_EPS 1e-6f
#define GOL_ALPHA_CAP_FWD 0.999f
#define GOL_ALPHA_CAP_BWD 0.99f /* upstream backward.cu clamps at 0.99, forward at 0.999 */
#define GOL_ALPHA_FLOOR (1.f / 255.f)
#define GOL_T_STOP 1e-4f
#define GOL_COMP_EPS 1e-6f

#define GOL_WAVE 64

void gol_set_error(const char* fmt, ...);

#define GOL_REQUIRE(cond, msg)                                         \
  do {                                                                 \
    if (!(cond)) {                                                     \
      gol_set_error("%s: %s", __func__, msg);                          \
      return GOL_ERR_INVALID_ARG;                                      \
    }                                                                  \
  } while (0)

#define GOL_CHECK_LAUNCH()                                             \
  do {                                                                 \
    hipError_t e_ = hipGetLastError();                                 \
    if (e_ != hipSuccess) {                                            \
      gol_set_error("%s: %s", __func__, hipGetErrorString(e_));        \
      return GOL_ERR_LAUNCH;                                           \
    }                                                                  \
  } while (0)

static inline int gol_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline bool gol_aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// ---- wave64 reductions through DPP (no LDS traffic) ---------------------------------------
// Sum over the 64 lanes; the total is valid in lane 63 (row_shr 1,2,3 + row_bcast 15/31,
// the classic GCN/CDNA reduction ladder; bound_ctrl=0 makes out-of-row sources read 0).
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
__device__ __forceinline__ float gol_dpp_mov0(float v) {
  // old = 0 with bound_ctrl so disabled / out-of-range lanes contribute 0
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, BANK_MASK, false));
}

// v + (v shifted right by 8 lanes inside its row of 16, 0 shifted in) as ONE v_add_f32_dpp.  Written as assembly: when
// only lane 15 of a row consumes the result the compiler sinks the add into the consumer's branch and leaves a
// v_mov 0 + v_mov_dpp + v_add triple behind (the DPP combiner works inside one basic block).  The s_nop covers the
// two wait states a DPP read needs after a VALU write of its source (the hazard recognizer does not look into asm).
__device__ __forceinline__ float gol_add_row_shr8(float v) {
  float r;
  asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(r) : "v"(v));
  return r;
}
// rows 1 and 3 add lane 15 of the row before them / rows 2 and 3 add lane 31 (the last two steps of a 64-lane sum):
// one v_add_f32_dpp each (masked-off rows keep their value) instead of v_mov 0 + v_mov_dpp + v_add
__device__ __forceinline__ float gol_add_row_bcast15(float v) {
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(v));
  return v;
}
__device__ __forceinline__ float gol_add_row_bcast31(float v) {
  asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(v));
  return v;
}

// sums of the four 16-lane rows, valid in lanes 15, 31, 47, 63 (4 fused v_add_f32_dpp)
__device__ __forceinline__ float gol_row_sum_to_lane15(float v) {
  v += gol_dpp_mov0<0x111>(v);  // row_shr:1
  v += gol_dpp_mov0<0x112>(v);  // row_shr:2
  v += gol_dpp_mov0<0x114>(v);  // row_shr:4
  return gol_add_row_shr8(v);   // row_shr:8
}

// Four wave-wide sums for the price of ~1.5: gfx950's v_permlane32_swap / v_permlane16_swap fold
// two registers into one per step (upper half of x <-> lower half of y, then odd rows <-> even
// rows), so 64-lane sums of (a, b, c, d) cost 3 swaps + 3 adds + 4 DPP row adds = 10 instructions
// instead of 4 x 6.  Results: lane 15 = sum(a), lane 31 = sum(b), lane 47 = sum(c), lane 63 = sum(d).
__device__ __forceinline__ float gol_swap32_sum(float x, float y) {
  const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y),
                                                  false, false);
  const unsigned r0 = r[0], r1 = r[1];  // (bit_cast straight from a vector element miscompiles)
  return __uint_as_float(r0) + __uint_as_float(r1);  // [x_lo+x_hi | y_lo+y_hi]
}
__device__ __forceinline__ float gol_swap16_sum(float x, float y) {
  const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y),
                                                  false, false);
  const unsigned r0 = r[0], r1 = r[1];
  return __uint_as_float(r0) + __uint_as_float(r1);  // rows [x01, y01, x23, y23]
}
__device__ __forceinline__ float gol_wave_sum4(float a, float b, float c, float d) {
  const float ac = gol_swap32_sum(a, c);   // lower 32 lanes: a, upper 32: c
  const float bd = gol_swap32_sum(b, d);   // lower: b, upper: d
  const float q = gol_swap16_sum(ac, bd);  // rows: a, b, c, d
  return gol_row_sum_to_lane15(q);
}

// Eight wave-wide sums in 17 instructions instead of 2 x 10.  Two 4-way folds leave P (rows: a0 a1 a2 a3) and Q (rows: a4 a5
// a6 a7) with 16 partials per row; a row then needs no full ladder of its own: P + row_ror:8(P) holds the 8 pair sums of
// a P row in both halves of the row, the same add on Q overwrites the upper half (bank_mask 0xc: lanes 8-15 of each row)
// with the pair sums of the Q row, and row_shr 1, 2, 4 (sources left of the row read 0) add the 8 pair sums of each half up.
// Results: lane 16 r + 7 = sum(a_r), lane 16 r + 15 = sum(a_{4 + r}), r = 0..3:
//   lane   7  15  23  31  39  47  55  63
//   sum   a0  a4  a1  a5  a2  a6  a3  a7
// The masked rotate add is assembly like gol_add_row_shr8 (no builtin adds into part of a row; its s_nop covers the
// VALU-write -> DPP-read hazard), and so is the last add, which only the result lanes consume (the compiler would sink it
// into their branch and split it up).  The first rotate add feeds the next one in the same basic block: the DPP combiner
// fuses it, and the hazard recognizer then places only the wait states the schedule leaves open.
__device__ __forceinline__ float gol_wave_sum8(float a0, float a1, float a2, float a3, float a4, float a5, float a6,
                                               float a7) {
  const float p02 = gol_swap32_sum(a0, a2), p13 = gol_swap32_sum(a1, a3);
  const float q02 = gol_swap32_sum(a4, a6), q13 = gol_swap32_sum(a5, a7);
  float p = gol_swap16_sum(p02, p13);        // rows: a0, a1, a2, a3
  const float q = gol_swap16_sum(q02, q13);  // rows: a4, a5, a6, a7
  p += gol_dpp_mov0<0x128>(p);  // row_ror:8
  asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xc" : "+v"(p) : "v"(q));
  p += gol_dpp_mov0<0x111>(p);  // row_shr:1
  p += gol_dpp_mov0<0x112>(p);  // row_shr:2
  float r;
  asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(r) : "v"(p));
  return r;
}

// Nine wave-wide sums of a 4 x 16 lane grid (lane = 16 r + x) in 20 instructions, when three of them are x-moments of two
// of the others: from a lane's six partial sums (s0, s1, s2, m0, my, myy) and a factor dx that depends on the column x only,
//   sum(s0), sum(s1), sum(s2), sum(myy), M0 = sum(m0), My = sum(my), Mx = sum(dx m0), Mxx = sum(dx^2 m0), Mxy = sum(dx my).
// With C0(x) and C1(x) the column sums of m0 and my over the four rows, Mx = sum_x dx C0, Mxx = sum_x dx^2 C0 and Mxy =
// sum_x dx C1: only six values cross the rows, and the products are formed on column sums, not per lane ahead of the fold.
//   1. cross-row: two 4-way folds of the six values.  P gets the column sums of (s0, s2, s1, myy), one per row; the fold
//      of (m0, my) swapped with its own copy leaves Q with rows (C0, C0, C1, C1).
//   2. on column sums: rows 1 and 3 of Q times dx (a row-masked DPP multiply, the other rows keep their value): rows
//      (C0, dx C0, C1, dx C1); U = Q dx has dx^2 C0 in row 1 (its other rows are not used).
//   3. in-row: X + row_ror:8(X) holds a row's 8 pair sums in both halves (gol_wave_sum8); the halves of P and Q are folded
//      once more with row_ror:4 into banks 1 and 3 (lanes 4-7: the quad sums of P, lanes 12-15: those of Q), the quad sums
//      of U go into bank 0, and row_shr 1 and 2 add the four quad sums of each bank up.
// Results, lane 16 r + c of the returned register:
//   lane      3     7    15    19    23    31    35    39    47    51    55    63
//   sum      (Mx)   s0   M0    Mxx   s2    Mx    -     s1    My    -     myy   Mxy          (lanes 16 r + 11: not a sum)
// Precondition: dx is the same in lanes l and l + 16 (a function of l & 15); lanes that break it get sums of no meaning.
// Stages 2 and 3 are one block of assembly (no builtin multiplies or adds into part of a register, and the compiler would
// sink what only the result lanes consume into their branch): a DPP read needs two wait states after a VALU write of its
// source, and inside the block the steps of P, Q and U are interleaved so that they fill most of each other's.
__device__ __forceinline__ float gol_wave_colsum(float s0, float s1, float s2, float m0, float my, float myy, float dx) {
  const float a01 = gol_swap32_sum(s0, s1), a2y = gol_swap32_sum(s2, myy);
  const float c = gol_swap32_sum(m0, my);   // rows 0, 1: halves of C0; rows 2, 3: halves of C1
  float p = gol_swap16_sum(a01, a2y);       // rows: s0, s2, s1, myy
  float q = gol_swap16_sum(c, c);           // rows: C0, C0, C1, C1
  float u;
  asm("s_nop 1\n\t"
      "v_mul_f32_dpp %1, %1, %3 quad_perm:[0,1,2,3] row_mask:0xa bank_mask:0xf\n\t"   // rows 1, 3: dx C0, dx C1
      "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"             // pair sums of P
      "v_mul_f32_e32 %2, %1, %3\n\t"                                                  // row 1: dx^2 C0
      "v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"             // lanes 8-15: pair sums of Q
      "s_nop 0\n\t"
      "v_add_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"             // pair sums of U
      "v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"             // banks 1, 3: quad sums of P, Q
      "s_nop 0\n\t"
      "v_add_f32_dpp %0, %2, %2 row_ror:4 row_mask:0xf bank_mask:0x1\n\t"             // bank 0: quad sums of U
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1"
      : "+v"(p), "+v"(q), "=&v"(u)
      : "v"(dx));
  return p;
}

// element at a 32-bit BYTE offset from a (wave-uniform) base pointer: the SGPR-base + VGPR-offset addressing form
// (64-bit per-lane address arithmetic costs several quarter-rate vector instructions per access)
template <typename T>
__device__ __forceinline__ T* gol_at(T* base, unsigned byte_off) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(const_cast<typename std::remove_const<T>::type*>(base)) + byte_off);
}

// a wave-uniform pointer pinned to SGPRs: loads through gol_at(gol_uniform(base), lane_offset) take the scalar-base +
// 32-bit lane-offset form (otherwise the loop-invariant lane part is folded into a 64-bit per-lane base: 2 VGPRs per load)
template <typename T>
__device__ __forceinline__ T* gol_uniform(T* q) {
  const uint64_t v = reinterpret_cast<uint64_t>(q);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<T*>(((uint64_t)hi << 32) | lo);
}

// lane mask of a predicate as a scalar (s_and with exec); HIP's __ballot(int) goes through an int (v_cndmask + v_cmp_ne)
__device__ __forceinline__ unsigned long long gol_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// returns the wave-wide sum in lane 63 (other lanes hold partial sums)
__device__ __forceinline__ float gol_wave_sum_to_lane63(float v) {
  v += gol_dpp_mov0<0x111>(v);              // row_shr:1
  v += gol_dpp_mov0<0x112>(v);              // row_shr:2
  v += gol_dpp_mov0<0x114>(v);              // row_shr:4  (lanes 4..15 of a row now hold 8-sums..)
  v = gol_add_row_shr8(v);                  // row_shr:8  -> lane 15 of each row = row sum
  v = gol_add_row_bcast15(v);               // row_bcast:15 into rows 1 and 3
  return gol_add_row_bcast31(v);            // row_bcast:31 into rows 2 and 3
}

// The same ladder on doubles, in the same order.  v + (the DPP-selected lane's v, 0 where the selection leaves the row /
// the row is masked off): the two halves of the double travel as two 32-bit DPP moves.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double gol_dpp_add0(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
  return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double gol_wave_sum_to_lane63(double v) {
  v = gol_dpp_add0<0x111, 0xf>(v);          // row_shr:1
  v = gol_dpp_add0<0x112, 0xf>(v);          // row_shr:2
  v = gol_dpp_add0<0x114, 0xf>(v);          // row_shr:4
  v = gol_dpp_add0<0x118, 0xf>(v);          // row_shr:8   -> lane 15 of each row = the row's sum
  v = gol_dpp_add0<0x142, 0xa>(v);          // row_bcast:15 into rows 1 and 3
  return gol_dpp_add0<0x143, 0xc>(v);       // row_bcast:31 into rows 2 and 3
}

__device__ __forceinline__ float gol_readlane63(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// ---- alpha >= 1/255 reach test (shared by binning and raster) -----------------------------------
// A Gaussian (centre g, conic a,b,c, opacity op) contributes at pixel p only if
//   op * exp(-sigma(p)) >= 1/255  <=>  sigma(p) = 0.5 d^T C d <= ln(255 op) =: tau     
// gol_alpha_tau returns a slightly inflated tau (conservative against rounding; < 0 means "never").
// k == 1 is still "reachable": the opacity (float)(1.f / 255.f) gives 255.f * op == 1.f exactly, and at a pixel centre that
// coincides with the Gaussian's centre (sigma == 0) alpha = op is not below the rasterizer's 1/255 cut -- gsplat composites it.
__device__ __forceinline__ float gol_alpha_tau(float op) {
  _Pragma("clang fp contract(on)")
  const float k = 255.f * op;
  return (k >= 1.f) ? __logf(k) * 1.001f + 1e-3f : -1.f;
}
// minimum of sigma over the axis-aligned rectangle [x0,x1] x [y0,y1] (exact: the quadratic is convex,
// so the minimum is 0 inside or lies on one of the four edges)
// (ia = 1 / a and ic = 1 / c are per-Gaussian: callers testing many rectangles pass them in)
__device__ __forceinline__ float gol_min_sigma_rect(float gx, float gy, float a, float b, float c, float ia, float ic,
                                                    float x0, float x1, float y0, float y1) {
  if (gx >= x0 && gx <= x1 && gy >= y0 && gy <= y1) return 0.f;
  float m = 3.0e38f;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float dx = (e ? x1 : x0) - gx;
    const float dy = fminf(fmaxf(-b * dx * ic, y0 - gy), y1 - gy);
    m = fminf(m, 0.5f * (a * dx * dx + c * dy * dy) + b * dx * dy);
    const float ey = (e ? y1 : y0) - gy;
    const float ex = fminf(fmaxf(-b * ey * ia, x0 - gx), x1 - gx);
    m = fminf(m, 0.5f * (a * ex * ex + c * ey * ey) + b * ex * ey);
  }
  return m;
}

// ---- packed per-Gaussian raster record (GOL_SPLAT_RECORD floats = 64 bytes = one HBM sector) ------------------------
// Everything the rasterizer stages for a list entry, written once per (view, Gaussian) by the projection (or by
// gol_splat_pack for the gsplat-compatible operators) and fetched with four 16-byte loads from ONE aligned 64-byte line
// -- the five separate attribute arrays of rounds 1-2 cost up to five sectors per entry (PMC: 109 B fetched for 40 B
// used).  The conic is stored the way the pixel loops want it: pre-multiplied by log2(e) (alpha = opacity * 2^-sigma' is
// one v_exp_f32) and the diagonal terms by the 1/2 of sigma = (a dx^2 + c dy^2) / 2 + b dx dy as well; GOL_UN_A / GOL_UN_B
// bring the true conic back.  The exact-math test build stores it unscaled.
//   [0] x  [1] y  [2] a'  [3] b' | [4] c'  [5] opacity  [6] r  [7] g | [8] b  [9] extra (depth)  [10] tau  [11] 1/a |
//   [12] 1/c  [13] exact (1 = the ellipse tests are valid, 0 = degenerate conic: "reaches everything")  [14-15] pad
// tau = gol_alpha_tau(opacity) (< 0: alpha < 1/255 everywhere), 1/a and 1/c of the TRUE conic: the per-entry part of the
// alpha >= 1/255 reach test, hoisted out of the staging loops of both raster passes.
#ifndef GOL_EXACT_MATH
#define GOL_SC_A (0.5f * 1.4426950408889634f)
#define GOL_SC_B 1.4426950408889634f
#define GOL_UN_A (2.f * 0.6931471805599453f)
#define GOL_UN_B 0.6931471805599453f
#else
#define GOL_SC_A 1.f
#define GOL_SC_B 1.f
#define GOL_UN_A 1.f
#define GOL_UN_B 1.f
#endif

__device__ __forceinline__ void gol_record_write(float* __restrict__ rec, float x, float y, float ca, float cb, float cc,
                                                 float op, float r, float g, float b, float extra) {
  _Pragma("clang fp contract(on)")   // written from two kernels (projection, shading epilogue): same bits from both
  const bool exact = (ca * cc - cb * cb > 0.f) && ca > 0.f && cc > 0.f;
  float4* R = reinterpret_cast<float4*>(rec);
  R[0] = make_float4(x, y, ca * GOL_SC_A, cb * GOL_SC_B);
  R[1] = make_float4(cc * GOL_SC_A, op, r, g);
  R[2] = make_float4(b, extra, gol_alpha_tau(op), exact ? 1.f / ca : 0.f);
  R[3] = make_float4(exact ? 1.f / cc : 0.f, exact ? 1.f : 0.f, 0.f, 0.f);
}

__device__ __forceinline__ float gol_fast_exp(float x) { return __expf(x); }
__device__ __forceinline__ float gol_rcp(float x) { return __frcp_rn(x); }
