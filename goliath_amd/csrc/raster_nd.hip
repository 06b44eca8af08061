// raster_nd.hip -- tile rasterizer of depth-sorted 2-D Gaussians with C colour channels, forward + backward, gfx950.
//
// Replaces gsplat 0.1.11 nd_rasterize_forward / nd_rasterize_backward_kernel (what gsplat's rasterize_gaussians runs for
// colors[N, C] with C != 3; not in the reference tree, whose only call site passes 3 channels, render_gsplat.py:65-104;
// gsplat's own nd kernels are not available here either).  Semantics SURVEY.md A.3 / A.4; the contract is the C-generic
// restatement of oracle/gsplat_oracle.c (orc_rasterize_fwd / orc_rasterize_bwd), which the 3-channel kernels of
// raster.hip also match.  Colours are interleaved [B,H,W,C] images and a dense colors[B,N,C] array; the geometry comes
// from the same 64-byte records (GOL_SPLAT_RECORD) as the 3-channel path, whose r, g, b fields are not read here.
// CDNA4 design -- the fast parts of raster.hip (gol_raster.h), with the colours split into chunks:
//   * one workgroup per 16x16 tile, the same Pix<PPL> wave footprints, tile -> XCD mapping, LDS staging of the tile list
//     in batches and half-mask ballot skip of the entries whose alpha >= 1/255 region misses a wave's pixels;
//   * CHUNKS: a workgroup composites CK in {1, 2, 4, 8, 16} channels (CK x PPL accumulators per lane).  C is covered by
//     chunks of 16 (one launch, grid.y = chunk; a remainder r = C % 16 of 9..15 is one more chunk there, its upper
//     channels masked) and, for r = 1..8, one chunk of the next power of two >= r, masked likewise (5 -> one chunk of 8,
//     12 -> one chunk of 16, 40 -> 16 + 16 + 8): C <= 16 walks the tile lists ONCE; every further chunk re-walks them.  The alpha / T decisions do not depend on the colours, so every chunk
//     takes the same entries; the chunk holding channel 0 writes final_Ts / final_idx;
//   * a chunk's colours are staged into LDS beside the geometry, per batch (at most 256 x 16 x 4 B = 16 KiB);
//   * backward: v_alpha is linear in the upstream image gradient, so each chunk adds its own share of v_xy / v_conic /
//     v_opacity (the v_out_alpha term goes to the chunk of channel 0 only) and writes only its slice of v_colors.  The
//     CK colour sums and the 6 geometry moments of a visit are reduced over the wave four at a time (gol_wave_sum4; eight at a time,
//     gol_wave_sum8, where they make an even number of fours: chunks of 1, 2, 8 and 16 channels),
//     parked in per-wave LDS slots, merged across the waves once per batch and leave the workgroup as one float atomic
//     per Gaussian per tile per component, issued by consecutive lanes (a Gaussian's colour atomics share cache lines).
#include "gol_raster.h"

namespace {

constexpr int kChunkMax = 16;   // channels per chunk (CK <= 16: 16 x PPL accumulators per lane, 16 KiB of staged colours)
constexpr int kBatchNdB = 64;   // backward batch (per-wave gradient slots live in LDS; one 64-entry ballot per batch)

// colours c0 .. c0 + nc - 1 of Gaussian g into an LDS row of CK floats (zeros above nc: masked channels composite 0)
template <int CK>
__device__ __forceinline__ void stage_colors(float* __restrict__ row, const float* __restrict__ colors, size_t g, int C,
                                             int c0, int nc) {
  const float* col = colors + g * (size_t)C + c0;
#pragma unroll
  for (int c = 0; c < CK; ++c) row[c] = (c < nc) ? col[c] : 0.f;
}

// Forward (gsplat's exact final_idx: the !LAZY variant of raster_fwd_kernel).  grid.x = tile slots x views, grid.y = the
// chunks of this launch (channels c_first + CK * blockIdx.y ..).
template <int CK, int PPL>
__global__ __launch_bounds__(64 * Pix<PPL>::kWaves) void raster_nd_fwd_kernel(
    int N, int C, int c_first, int img_h, int img_w, int tiles_x, int tiles_y, const int2* __restrict__ tile_bins,
    const int32_t* __restrict__ sorted_ids, int64_t capacity, const float* __restrict__ records,
    const float* __restrict__ colors, const float* __restrict__ background, float* __restrict__ out_img,
    float* __restrict__ final_Ts, int32_t* __restrict__ final_idx, int n_views) {
  typedef typename Pix<PPL>::fv fv;
  typedef typename Pix<PPL>::iv iv;
  constexpr int NW = Pix<PPL>::kWaves, NT = 64 * NW;
  __shared__ float4 s_a[kBatch];      // x, y, conic.a', conic.b'
  __shared__ float2 s_b[kBatch];      // conic.c', opacity
  __shared__ int32_t s_mask[kBatch];  // wave mask
  __shared__ __attribute__((aligned(16))) float s_col[kBatch * CK];
  const int T = tiles_x * tiles_y;
  const int view = blockIdx.x % n_views, slot = blockIdx.x / n_views;
  const TileCoord tc = tile_of_block(slot, T, tiles_x);
  if (!tc.ok) return;
  const int c0 = c_first + (int)blockIdx.y * CK;
  const int nc = min(CK, C - c0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int j, i0;
  lane_pixel<PPL>(tc.tx, tc.ty, wave, lane, j, i0);
  bool in[PPL];
  fv py, live;
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    in[q] = (i0 + q < img_h) && (j < img_w);
    py[q] = (float)(i0 + q) + 0.5f;
    live[q] = in[q] ? 1.f : 0.f;   // (a float multiplied into alpha, as in raster_fwd_kernel)
  }
  const float px = (float)j + 0.5f;

  const int2 range = tile_bins[(size_t)view * T + tc.tile];
  const int32_t* ids = sorted_ids + (size_t)view * capacity;
  const size_t goff = (size_t)view * N;

  fv T_cur = 1.f;
  iv cur_idx = 0;
  fv acc[CK];
#pragma unroll
  for (int c = 0; c < CK; ++c) acc[c] = 0.f;

  const int n_batches = (range.y - range.x + kBatch - 1) / kBatch;
  for (int bb = 0; bb < n_batches; ++bb) {
    if (__syncthreads_and(!any_live<fv, PPL>(live))) break;  // also protects the LDS batch from being overwritten early
    const int batch_start = range.x + bb * kBatch;
    for (int k = tid; k < kBatch; k += NT) {
      const int idx = batch_start + k;
      if (idx < range.y) {
        const size_t g = goff + (size_t)ids[idx];
        const Staged st = stage_entry<PPL>(records, g, (float)(tc.tx * 16), (float)(tc.ty * 16));
        s_a[k] = st.a; s_b[k] = make_float2(st.b.x, st.b.y); s_mask[k] = st.mask;
        stage_colors<CK>(s_col + k * CK, colors, g, C, c0, nc);
      } else {
        s_mask[k] = 0;
      }
    }
    __syncthreads();
    const int batch_size = min(kBatch, range.y - batch_start);
    for (int chunk = 0; chunk < batch_size; chunk += 64) {
      unsigned long long bits = gol_ballot((s_mask[chunk + lane] >> wave) & 1);
      while (bits) {
        if (gol_ballot(any_live<fv, PPL>(live)) == 0ull) { chunk = batch_size; break; }  // this wave's footprint is finished
        const int t = chunk + __builtin_ctzll(bits);
        bits &= bits - 1;
        const float4 a4 = s_a[t];
        const float2 b2 = s_b[t];
        const float dx = a4.x - px;
        const fv dy = a4.y - py;
        fv sigma, e, alpha, vis, next_T;
        visit_falloff<PPL>(a4.z, a4.w, b2.x, dx, dy, sigma, e);
#pragma unroll
        for (int q = 0; q < PPL; ++q) alpha[q] = fminf(GOL_ALPHA_CAP_FWD, b2.y * e[q]);
        bool take[PPL];
        unsigned long long stop_m[PPL];
        fwd_step<PPL>(sigma, alpha, live, T_cur, vis, next_T, take, stop_m);
#pragma unroll
        for (int q = 0; q < PPL; ++q) live[q] = __builtin_amdgcn_inverse_ballot_w64(stop_m[q]) ? 0.f : live[q];
        fwd_take<PPL>(take, next_T, vis, T_cur);
        const float* col = s_col + t * CK;
#pragma unroll
        for (int c = 0; c < CK; ++c) acc[c] += col[c] * vis;
#pragma unroll
        for (int q = 0; q < PPL; ++q) cur_idx[q] = take[q] ? (batch_start + t) : cur_idx[q];
      }
    }
  }

  // [B,H,W,C]: wave-uniform per-view / per-channel base pointers + one 32-bit byte offset per lane (< 4 GiB: checked)
  const unsigned hw = (unsigned)img_h * (unsigned)img_w;
  const size_t vplane = (size_t)view * hw;
  float* __restrict__ o_img = out_img + (size_t)C * vplane + c0;
  float* __restrict__ o_T = final_Ts + vplane;
  int32_t* __restrict__ o_idx = final_idx + vplane;
  const bool first = c0 == 0;
  float bg[CK];
#pragma unroll
  for (int c = 0; c < CK; ++c) bg[c] = (c < nc) ? background[c0 + c] : 0.f;
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    if (!in[q]) continue;
    const unsigned pix = (unsigned)(i0 + q) * (unsigned)img_w + (unsigned)j;
    const float Tq = T_cur[q];
    if (first) { *gol_at(o_T, pix * 4u) = Tq; *gol_at(o_idx, pix * 4u) = cur_idx[q]; }
    const unsigned bimg = pix * (unsigned)C * 4u;
#pragma unroll
    for (int c = 0; c < CK; ++c)
      if (c < nc) *gol_at(o_img + c, bimg) = acc[c][q] + Tq * bg[c];
  }
}

// Backward.  Same workgroup / wave / lane layout and batch walk as raster_bwd_kernel (dense gradient arrays), on CK
// channels.  Per-visit wave sums: the CK colour sums  sum_pix fac v_out_c  and the moments of gop = opacity vis v_alpha
// (m0 = opacity * v_opacity, mx, my, mxx, mxy, myy; see raster_bwd_kernel), NS = CK + 6 of them, reduced four at a time.
template <int CK, int PPL>
__global__ __launch_bounds__(64 * Pix<PPL>::kWaves) void raster_nd_bwd_kernel(
    int N, int C, int c_first, int img_h, int img_w, int tiles_x, int tiles_y, const int2* __restrict__ tile_bins,
    const int32_t* __restrict__ sorted_ids, int64_t capacity, const float* __restrict__ records,
    const float* __restrict__ colors, const float* __restrict__ background, const float* __restrict__ final_Ts,
    const int32_t* __restrict__ final_idx, const float* __restrict__ v_out_img, const float* __restrict__ v_out_alpha,
    float* __restrict__ v_xy, float* __restrict__ v_conic, float* __restrict__ v_colors, float* __restrict__ v_opacity,
    int n_views) {
  typedef typename Pix<PPL>::fv fv;
  typedef typename Pix<PPL>::iv iv;
  constexpr int NW = Pix<PPL>::kWaves, NT = 64 * NW;
  constexpr int NS = CK + 6, NG = (NS + 3) / 4, kRow = 4 * NG;   // sums per visit, 4-way groups, LDS slot row
  static_assert(NW * kBatchNdB == NT, "s_touched is cleared one element per thread");
  __shared__ float4 s_a[kBatchNdB];   // x, y, conic.a', conic.b'
  __shared__ float2 s_b[kBatchNdB];   // conic.c', opacity
  __shared__ int32_t s_mask[kBatchNdB];
  __shared__ int32_t s_id[kBatchNdB];
  __shared__ __attribute__((aligned(16))) float s_col[kBatchNdB * CK];
  __shared__ __attribute__((aligned(16))) float s_acc[NW][kBatchNdB][kRow];
  __shared__ int32_t s_touched[NW][kBatchNdB];
  __shared__ int32_t s_wmax[NW];
  const int T = tiles_x * tiles_y;
  const int view = blockIdx.x % n_views, slot = blockIdx.x / n_views;
  const TileCoord tc = tile_of_block(slot, T, tiles_x);
  if (!tc.ok) return;
  const int2 range = tile_bins[(size_t)view * T + tc.tile];
  if (range.y <= range.x) return;
  const int c0 = c_first + (int)blockIdx.y * CK;
  const int nc = min(CK, C - c0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int j, i0;
  lane_pixel<PPL>(tc.tx, tc.ty, wave, lane, j, i0);
  const float px = (float)j + 0.5f;
  const int32_t* ids = sorted_ids + (size_t)view * capacity;
  const size_t goff = (size_t)view * N;
  fv py, T_final, voa = 0.f;
  iv bin_final;
  fv vo[CK];
#pragma unroll
  for (int c = 0; c < CK; ++c) vo[c] = 0.f;
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    const bool in = (i0 + q < img_h) && (j < img_w);
    py[q] = (float)(i0 + q) + 0.5f;
    const size_t p = in ? ((size_t)view * img_h + i0 + q) * img_w + j : 0;
    T_final[q] = in ? final_Ts[p] : 1.f;
    bin_final[q] = in ? final_idx[p] : (range.x - 1);
    if (in) {
      const float* g = v_out_img + p * (size_t)C + c0;
#pragma unroll
      for (int c = 0; c < CK; ++c) vo[c][q] = (c < nc) ? g[c] : 0.f;
      // the alpha output's gradient enters once, with the chunk of channel 0
      if (v_out_alpha && c0 == 0) voa[q] = v_out_alpha[p];
    }
  }

  const int wmax = wave_last_entry<PPL>(bin_final);
  if (lane == 0) s_wmax[wave] = wmax;
  __syncthreads();
  int bmax = s_wmax[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) bmax = max(bmax, s_wmax[w]);
  bmax = min(bmax, range.y - 1);
  if (bmax < range.x) return;

  // (the background is read here, behind the barrier: held across it, 16 uniform values spill SGPRs)
  fv bgdot = 0.f;
#pragma unroll
  for (int c = 0; c < CK; ++c) bgdot += ((c < nc) ? background[c0 + c] : 0.f) * vo[c];
  fv T_cur = T_final;
  fv R = bgdot - voa;  // composite of <colour, v_out> over what lies behind (this chunk's channels; see bwd_moments)

  // this lane's column: lanes 15, 31, 47, 63 hold sums 4 g + 0 .. 3 of group g; with an even number of groups they are
  // reduced in pairs (17 instructions per pair instead of 20) and lane 8 k + 7 holds sum 8 p + k of pair p
  constexpr bool kSum8 = NG % 2 == 0;
  float* acc_lane = &s_acc[wave][0][kSum8 ? lane >> 3 : lane >> 4];
  const int n_batches = (bmax - range.x + kBatchNdB) / kBatchNdB;
  for (int bb = 0; bb < n_batches; ++bb) {
    __syncthreads();
    const int batch_end = bmax - bb * kBatchNdB;
    const int batch_size = min(kBatchNdB, batch_end + 1 - range.x);
    if (tid < kBatchNdB) {
      if (tid < batch_size) {
        const int gid = ids[batch_end - tid];
        const size_t g = goff + (size_t)gid;
        const Staged st = stage_entry<PPL>(records, g, (float)(tc.tx * 16), (float)(tc.ty * 16));
        s_a[tid] = st.a; s_b[tid] = make_float2(st.b.x, st.b.y); s_mask[tid] = st.mask;
        s_id[tid] = gid;
        stage_colors<CK>(s_col + tid * CK, colors, g, C, c0, nc);
      } else {
        s_mask[tid] = 0;
      }
    }
    (&s_touched[0][0])[tid] = 0;
    __syncthreads();

    const int t0 = max(0, batch_end - wmax);
    unsigned long long bits = gol_ballot((s_mask[lane] >> wave) & 1);  // kBatchNdB == 64: one chunk
    if (t0 > 0) bits &= ~0ull << t0;
    while (bits) {
      const int t = __builtin_ctzll(bits);
      bits &= bits - 1;
      const float4 a4 = s_a[t];
      const float2 b2 = s_b[t];
      const int li = batch_end - t;
      const float dx = a4.x - px;
      const fv dy = a4.y - py;
      fv sigma, vis, raw, alpha, ra, fac;
      visit_falloff<PPL>(a4.z, a4.w, b2.x, dx, dy, sigma, vis);
      unsigned long long mv[PPL];
      if (bwd_taken<PPL>(b2.y, vis, sigma, li, bin_final, raw, mv) == 0ull) continue;
      bwd_recur<PPL>(mv, raw, T_cur, alpha, ra, fac);
      // w = <colour, v_out> over this chunk's channels (see bwd_moments)
      const float* col = s_col + t * CK;
      fv w = 0.f;
#pragma unroll
      for (int c = 0; c < CK; ++c) w += col[c] * vo[c];
      fv gop, gy, gyy;
      bwd_moments<PPL>(raw, w, T_cur, alpha, dy, R, gop, gy, gyy);
      float s[kRow];
#pragma unroll
      for (int c = 0; c < CK; ++c) {
        s[c] = fac[0] * vo[c][0];
#pragma unroll
        for (int q = 1; q < PPL; ++q) s[c] = __builtin_fmaf(fac[q], vo[c][q], s[c]);
      }
      const float m0 = lane_sum<PPL>(gop), my = lane_sum<PPL>(gy), myy = lane_sum<PPL>(gyy);
      const float mx = m0 * dx;
      s[CK + 0] = m0; s[CK + 1] = mx; s[CK + 2] = my; s[CK + 3] = mx * dx; s[CK + 4] = my * dx; s[CK + 5] = myy;
#pragma unroll
      for (int k = NS; k < kRow; ++k) s[k] = 0.f;
      if constexpr (kSum8) {
        // even slots first, odd ones after them: lane 8 k + 7 then holds slot 8 p + k of pair p (see gol_wave_sum8)
        float r[NG / 2];
#pragma unroll
        for (int p = 0; p < NG / 2; ++p)
          r[p] = gol_wave_sum8(s[8 * p], s[8 * p + 2], s[8 * p + 4], s[8 * p + 6],
                               s[8 * p + 1], s[8 * p + 3], s[8 * p + 5], s[8 * p + 7]);
        if ((lane & 7) == 7) {
          float* a = gol_at(acc_lane, (unsigned)t * (unsigned)(kRow * sizeof(float)));
#pragma unroll
          for (int p = 0; p < NG / 2; ++p) a[8 * p] = r[p];
          s_touched[wave][t] = 1;
        }
      } else {
        float r[NG];
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) r[gi] = gol_wave_sum4(s[4 * gi], s[4 * gi + 1], s[4 * gi + 2], s[4 * gi + 3]);
        if ((lane & 15) == 15) {
          float* a = gol_at(acc_lane, (unsigned)t * (unsigned)(kRow * sizeof(float)));
#pragma unroll
          for (int gi = 0; gi < NG; ++gi) a[4 * gi] = r[gi];
          s_touched[wave][t] = 1;
        }
      }
    }
    __syncthreads();
    // merge the waves' slots; component k of entry t: colour k (k < CK) or a geometry gradient from the moments.
    // Consecutive threads take consecutive components of one entry: its colour atomics share cache lines.
    for (int idx = tid; idx < batch_size * NS; idx += NT) {
      const int t = idx / NS, k = idx - t * NS;
      if (k < CK && k >= nc) continue;
      bool any = false;
#pragma unroll
      for (int w = 0; w < NW; ++w) any = any || (s_touched[w][t] != 0);
      if (!any) continue;
      const size_t g = goff + (size_t)s_id[t];
      const float4 a4 = s_a[t];
      const float2 b2 = s_b[t];
      // moments of gop = opacity e v_alpha (bwd_moments): d loss / d sigma = -gop, so the sigma sums are the negated moments,
      // and v_opacity = m0 / opacity -- a true division; a touched entry was taken with opacity e >= 1/255, so opacity > 0
      const float3 cn = true_conic(a4.z, a4.w, b2.x);
      const float ca = cn.x, cb = cn.y, cc = cn.z;
      int k1 = k, k2 = k;
      float w1 = 1.f, w2 = 0.f;
      float* dst;
      if (k < CK) {
        dst = v_colors + g * (size_t)C + c0 + k;
      } else {
        const int m = k - CK;
        k1 = (m == 1 || m == 2) ? CK + 1 : k;
        k2 = CK + 2;
        w1 = (m == 0) ? 1.f : (m == 1) ? -ca : (m == 2) ? -cb : (m == 4) ? -1.f : -0.5f;
        w2 = (m == 1) ? -cb : (m == 2) ? -cc : 0.f;
        dst = (m == 0) ? v_opacity + g : (m <= 2) ? v_xy + 2 * g + (m - 1) : v_conic + 3 * g + (m - 3);
      }
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const bool tw = s_touched[w][t] != 0;
        s1 += tw ? s_acc[w][t][k1] : 0.f;
        s2 += tw ? s_acc[w][t][k2] : 0.f;
      }
      atomicAdd(dst, k == CK ? s1 / b2.y : w1 * s1 + w2 * s2);
    }
  }
}

// How the launches cover C channels: n16 chunks of 16 as grid.y of one launch -- a remainder of 9..15 channels is one more,
// masked, chunk of that launch -- and, for a remainder r of 1..8, one tail chunk of the next power of two >= r
// (tail = 1, 2, 4 or 8; 0 = none) starting at channel tail_first.
struct NdPlan { int n16, tail, tail_first; };
NdPlan nd_plan(int C) {
  const int r = C % kChunkMax;
  NdPlan p;
  p.n16 = C / kChunkMax + (r > 8 ? 1 : 0);
  p.tail = (r == 0 || r > 8) ? 0 : r <= 1 ? 1 : r <= 2 ? 2 : r <= 4 ? 4 : 8;
  p.tail_first = (C / kChunkMax) * kChunkMax;
  return p;
}

// fn(std::integral_constant<int, CK>, chunks in grid.y, first channel) for every launch of nd_plan(C); false: no such CK
template <typename F>
bool for_nd_launches(int C, F&& fn) {
  const NdPlan pl = nd_plan(C);
  if (pl.n16 > 0) fn(std::integral_constant<int, 16>(), pl.n16, 0);
  switch (pl.tail) {
    case 0: break;
    case 1: fn(std::integral_constant<int, 1>(), 1, pl.tail_first); break;
    case 2: fn(std::integral_constant<int, 2>(), 1, pl.tail_first); break;
    case 4: fn(std::integral_constant<int, 4>(), 1, pl.tail_first); break;
    case 8: fn(std::integral_constant<int, 8>(), 1, pl.tail_first); break;
    default: return false;
  }
  return true;
}

}  // namespace

extern "C" int gol_rasterize_nd_fwd(int B, int N, int C, int img_h, int img_w, int block, const int32_t* tile_bins,
                                    const int32_t* sorted_ids, int64_t capacity, const float* records, const float* colors,
                                    const float* background, float* out_img, float* final_Ts, int32_t* final_idx,
                                    int pixels_per_lane, void* stream) {
  GOL_REQUIRE(C >= 1, "C >= 1 colour channels");
  GOL_REQUIRE(C <= 16 * 65535, "too many colour channels (at most 1048560: one launch row of 16-channel chunks)");
  GOL_RASTER_CHECK_DIMS((uint64_t)C * 4ull, "image too large (32-bit byte offsets inside a view: H * W * C * 4 bytes)");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(tile_bins && background && out_img && final_Ts && final_idx, "null pointer");
  GOL_REQUIRE(capacity == 0 || sorted_ids, "null sorted_ids");
  GOL_REQUIRE(N == 0 || (records && colors), "null Gaussian records / colors");
  GOL_REQUIRE(pixels_per_lane >= 0 && pixels_per_lane <= 2, "pixels_per_lane: 0 (choose by B), 1 or 2");
  int ppl = pixels_per_lane;
  if (ppl == 0) gol_raster_plan(B, &ppl);
  const int tiles_x = (img_w + 15) / 16, tiles_y = (img_h + 15) / 16;
  const unsigned gx = (unsigned)raster_grid(B, img_h, img_w);
  const int2* bins = reinterpret_cast<const int2*>(tile_bins);
  hipStream_t s = (hipStream_t)stream;
  const bool covered = for_nd_launches(C, [&](auto ck_c, int n_chunks, int c_first) {
    with_ppl(ppl, [&](auto ppl_c) {
      constexpr int CK = decltype(ck_c)::value, PPL = decltype(ppl_c)::value;
      raster_nd_fwd_kernel<CK, PPL><<<dim3(gx, n_chunks), 64 * Pix<PPL>::kWaves, 0, s>>>(
          N, C, c_first, img_h, img_w, tiles_x, tiles_y, bins, sorted_ids, capacity, records, colors, background, out_img,
          final_Ts, final_idx, B);
    });
  });
  GOL_REQUIRE(covered, "no kernel instance for this chunk width");
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_rasterize_nd_bwd(int B, int N, int C, int img_h, int img_w, int block, const int32_t* tile_bins,
                                    const int32_t* sorted_ids, int64_t capacity, const float* records, const float* colors,
                                    const float* background, const float* final_Ts, const int32_t* final_idx,
                                    const float* v_out_img, const float* v_out_alpha, float* v_xy, float* v_conic,
                                    float* v_colors, float* v_opacity, void* stream) {
  GOL_REQUIRE(C >= 1, "C >= 1 colour channels");
  GOL_REQUIRE(C <= 16 * 65535, "too many colour channels (at most 1048560: one launch row of 16-channel chunks)");
  GOL_RASTER_CHECK_DIMS((uint64_t)C * 4ull, "image too large (32-bit byte offsets inside a view: H * W * C * 4 bytes)");
  if (B == 0 || N == 0 || capacity == 0) return GOL_OK;
  GOL_REQUIRE(tile_bins && sorted_ids && background && final_Ts && final_idx, "null pointer");
  GOL_REQUIRE(v_out_img, "null v_out_img");
  GOL_REQUIRE(records && colors, "null Gaussian records / colors");
  GOL_REQUIRE(v_xy && v_conic && v_colors && v_opacity, "null gradient output");
  const int tiles_x = (img_w + 15) / 16, tiles_y = (img_h + 15) / 16;
  const unsigned gx = (unsigned)raster_grid(B, img_h, img_w);
  const int2* bins = reinterpret_cast<const int2*>(tile_bins);
  hipStream_t s = (hipStream_t)stream;
  // two pixels per lane (as the 3-channel backward): the per-visit wave sums are paid once per 128 pixels
  const bool covered = for_nd_launches(C, [&](auto ck_c, int n_chunks, int c_first) {
    constexpr int CK = decltype(ck_c)::value;
    raster_nd_bwd_kernel<CK, 2><<<dim3(gx, n_chunks), 128, 0, s>>>(
        N, C, c_first, img_h, img_w, tiles_x, tiles_y, bins, sorted_ids, capacity, records, colors, background, final_Ts,
        final_idx, v_out_img, v_out_alpha, v_xy, v_conic, v_colors, v_opacity, B);
  });
  GOL_REQUIRE(covered, "no kernel instance for this chunk width");
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
