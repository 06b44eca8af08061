// raster.hip -- tile rasterizer of depth-sorted 2-D Gaussians, forward + backward, gfx950.
//
// Replaces gsplat 0.1.11 rasterize_forward / rasterize_backward_kernel (3-channel specialisation;
// not in the reference tree; call sites /root/reference/ca_code/utils/render_gsplat.py:65-78 and
// :91-104; semantics SURVEY.md A.3 / A.4).  CDNA4 design:
//   * one 128-thread workgroup per 16x16 tile = 2 wave64s, each wave owns a 16x8 half and each lane two
//     vertically adjacent pixels: the per-pixel recurrences run on 2-vectors, i.e. packed fp32 VALU ops
//     (v_pk_fma/mul/add_f32), and the cross-lane gradient reduction of the backward is paid once per 128 pixels;
//   * the tile's sorted list is staged through LDS in batches as three records per Gaussian; the per-Gaussian
//     reads in the pixel loop are wave-uniform ds_read_b128 broadcasts;
//   * at staging time every Gaussian gets a 2-bit half mask from the exact ellipse-vs-rectangle test of its
//     alpha >= 1/255 region, so a wave skips (scalar loop over a 64-bit ballot) Gaussians that cannot touch its
//     half -- gsplat's 3-sigma tile bbox is far looser than the 1/255 cut;
//   * colour and the optional 4th "extra" channel (depth) are composited in ONE pass instead of
//     the reference's two rasterize calls (render_gsplat.py:65-104);
//   * backward: per-Gaussian gradients are reduced over the 64 lanes four-at-a-time with
//     v_permlane32_swap / v_permlane16_swap + DPP row adds (no LDS, no atomics), parked in per-wave LDS
//     slots, merged across the waves once per batch and leave the workgroup as one float atomic per Gaussian per
//     tile per component (gsplat: one per 32-lane warp => 8x more); with 64-byte gradient records
//     (GOL_GRAD_RECORD) the 10 atomics of a Gaussian share a cache line and are issued by 16 adjacent lanes --
//     the memory-side atomic units, which cost 25 % of the kernel with dense [N,k] arrays, drop out of the profile;
//   * tile -> workgroup mapping interleaves tile rows over the 8 XCDs (tile_of_block).
#include <cstdlib>

#include "gol_raster.h"

namespace {

constexpr int kBgGroup = 4;   // tiles per group of the forward's empty-run path (2, 4 and 8 are built; see gol_rasterize_fwd)

// Forward.  One workgroup per 16x16 tile (PPL = 2: 128 threads, PPL = 1: 256; see Pix).
// LAZY (the fused path, planar images): everything that only changes when a pixel STOPS -- its liveness, the index the
// backward may start from, the "is this half finished" test -- moves out of the per-visit instruction stream into a
// wave-uniform branch taken only on visits where some pixel of the half stops (a pixel stops once; a visit costs 7 vector
// instructions less).  final_idx then holds, per pixel, an UPPER BOUND of the index of its last contributor that excludes
// the entry it stopped at: stop index - 1, or the end of the list for a pixel that never stopped.  The backward only needs
// that (entries between the true last contributor and the bound fail its alpha >= 1/255 test again).  !LAZY (the
// gsplat-compatible operator): gsplat's exact final_idx.
template <bool EXTRA, bool LAZY, int PPL>
__global__ __launch_bounds__(64 * Pix<PPL>::kWaves) void raster_fwd_kernel(
    int N, int img_h, int img_w, int planar, int tiles_x, int tiles_y, const int2* __restrict__ tile_bins,
    const int32_t* __restrict__ sorted_ids, int64_t capacity, const float* __restrict__ records,
    const float* __restrict__ background, float* __restrict__ out_img,
    float* __restrict__ out_extra, float* __restrict__ final_Ts, int32_t* __restrict__ final_idx,
    float* __restrict__ out_alpha, float* __restrict__ out_extra_norm, float norm_lo,
    const float* __restrict__ l1_target, const float* __restrict__ l1_mask, int l1_mask_c,
    uint8_t* __restrict__ l1_sign, float* __restrict__ l1_partial, int n_views, int bg_group, int bg_vec16,
    uint8_t* __restrict__ stage_mask) {
  typedef typename Pix<PPL>::fv fv;
  typedef typename Pix<PPL>::iv iv;
  constexpr int NW = Pix<PPL>::kWaves, NT = 64 * NW;
  __shared__ float s_l1[NW];
  // (separate arrays: the 48-byte rows of the backward kernel, which save it an address register move per visit, cost the
  // forward 3-5 % -- measured side by side on one box, profiles/r03g_raster_ab.txt)
  __shared__ float4 s_a[kBatch];  // x, y, conic.a, conic.b
  __shared__ float4 s_b[kBatch];  // conic.c, opacity, r, g
  __shared__ float2 s_c[kBatch];  // b, extra  (an 8-byte stride on purpose: with a 16-byte one the compiler issues all
                                  // three reads of a visit at the loop top from one address register, and the forward
                                  // runs 3-4 % slower -- profiles/r03g_raster_ab.txt)
  __shared__ int32_t s_mask[kBatch];  // wave mask
  const int T = tiles_x * tiles_y;
  // workgroup g = slot * B + view (the view is the fastest index: the workgroups of all views of a launch are handed out
  // together -- the last view's long lists do not start when the others are already done; with B = 8 a view also stays
  // on one die, with B = 4 on two)
  const int view = blockIdx.x % n_views, slot = blockIdx.x / n_views;
  const TileCoord tc = tile_of_block(slot, T, tiles_x);
  if (!tc.ok) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // Runs of empty tiles (bg_group = G > 0: planar images of even width, see gol_rasterize_fwd).  A group is G consecutive
  // tiles of one tile row -- consecutive workgroups of one die (tile_of_block).  Every workgroup reads the group's G list
  // ranges (wave-uniform: scalar loads).  Some tile has entries: all of them run the per-tile code below, unchanged.  The
  // whole group is empty: its first workgroup writes the constant outputs of the WHOLE region as full rows (8 or 16 bytes
  // per lane instead of 4-byte accesses to 64-byte row segments) and sums the fused L1 of every tile; the others return at
  // once -- they neither hold a workgroup place through two memory round trips nor touch the image.  The constants are formed
  // with the per-tile epilogue's expressions and the L1 keeps its lane-to-pixel map and order of additions: same bits.
  int2 range;   // the tile's own list range (with groups: picked from the group's ranges, no second round trip)
  auto fill_group = [&](auto g_c) -> bool {
    constexpr int G = decltype(g_c)::value;
    const int tx0 = tc.tx & ~(G - 1), n = min(G, tiles_x - tx0);
    const size_t tile0 = (size_t)view * T + (size_t)(tc.tile - (tc.tx - tx0));
    int entries = 0;
#pragma unroll
    for (int t = 0; t < G; ++t) {
      const int2 r = tile_bins[tile0 + min(t, n - 1)];
      entries |= (r.y > r.x) ? 1 : 0;
      if (t == tc.tx - tx0) range = r;
    }
    if (entries) return false;
    if (tc.tx != tx0) return true;
    const unsigned hw = (unsigned)img_h * (unsigned)img_w;
    const size_t vplane = (size_t)view * hw;
    const float Tq = 1.f, ex = 0.f;
    const float c0 = 0.f + Tq * background[0], c1 = 0.f + Tq * background[1], c2 = 0.f + Tq * background[2];
    const float al = 1.f - Tq;
    const float nrm = ex / fminf(fmaxf(1.f - Tq, norm_lo), 1.f);
    float* __restrict__ o_T = final_Ts + vplane;
    float* __restrict__ o_img = out_img + 3 * vplane;
    float* __restrict__ o_img1 = o_img + hw;
    float* __restrict__ o_img2 = o_img + 2u * hw;
    float* __restrict__ o_ex = (EXTRA && out_extra) ? out_extra + vplane : nullptr;
    float* __restrict__ o_alpha = out_alpha ? out_alpha + vplane : nullptr;
    float* __restrict__ o_norm = (EXTRA && out_extra_norm) ? out_extra_norm + vplane : nullptr;
    const int x0 = tx0 * 16, y0 = tc.ty * 16;
    const int rw = min(x0 + 16 * G, img_w) - x0, nrows = min(16, img_h - y0);   // rw: a multiple of the store width
    auto fill_rows = [&](auto v_c) {
      constexpr int V = decltype(v_c)::value;               // floats per lane and store
      typedef float vt __attribute__((ext_vector_type(V)));
      typedef int it __attribute__((ext_vector_type(V)));
      constexpr int CPR = 16 * G / V, RPP = NT / CPR;       // lanes along a full row; rows per pass of the workgroup
      const int col = (tid % CPR) * V, r0 = tid / CPR;
#pragma unroll
      for (int k = 0; k * RPP < 16; ++k) {
        const int r = r0 + k * RPP;
        if (col < rw && r < nrows) {
          const unsigned b4 = ((unsigned)(y0 + r) * (unsigned)img_w + (unsigned)(x0 + col)) * 4u;
          *reinterpret_cast<vt*>(gol_at(o_T, b4)) = vt(Tq);
          if (!LAZY) *reinterpret_cast<it*>(gol_at(final_idx + vplane, b4)) = it(0);   // gsplat's exact final_idx
          *reinterpret_cast<vt*>(gol_at(o_img, b4)) = vt(c0);
          *reinterpret_cast<vt*>(gol_at(o_img1, b4)) = vt(c1);
          *reinterpret_cast<vt*>(gol_at(o_img2, b4)) = vt(c2);
          if (o_ex) *reinterpret_cast<vt*>(gol_at(o_ex, b4)) = vt(ex);
          if (o_alpha) *reinterpret_cast<vt*>(gol_at(o_alpha, b4)) = vt(al);
          if (o_norm) *reinterpret_cast<vt*>(gol_at(o_norm, b4)) = vt(nrm);
        }
      }
    };
    if (bg_vec16) fill_rows(std::integral_constant<int, 4>());
    else fill_rows(std::integral_constant<int, 2>());
    if (!l1_target) return true;
    // fused L1 of the group's tiles: the target (and mask) values of up to four tiles are in flight before the first is used
    // (all of a group of two or four; eight tiles x two pixels per lane x six values would cost the kernel a wave per SIMD)
    const float* __restrict__ i_tgt = l1_target + 3 * vplane;
    const float* __restrict__ i_mask = l1_mask ? l1_mask + (size_t)l1_mask_c * vplane : nullptr;
    float* s_part = reinterpret_cast<float*>(s_a);           // [G][NW] wave sums (the batch arrays are idle on this path)
    constexpr int CH = G < 4 ? G : 4;
    auto l1_tiles = [&](auto m_c) {
      constexpr int MC = decltype(m_c)::value;               // mask channels: 0 (none), 1 or 3
      const float cs[3] = {c0, c1, c2};
#pragma unroll
      for (int tb = 0; tb < G; tb += CH) {
        if (tb >= n) break;
        float tg[CH][PPL][3], mk[CH][PPL][3];
        bool ok[CH][PPL];
#pragma unroll
        for (int t = 0; t < CH; ++t) {
          int tj, ti0;
          lane_pixel<PPL>(tx0 + tb + t, tc.ty, wave, lane, tj, ti0);
#pragma unroll
          for (int q = 0; q < PPL; ++q) {
            ok[t][q] = (ti0 + q < img_h) && (tj < img_w);
            // a pixel outside the image (or in a tile past the row's end) reads the nearest pixel inside and is dropped below
            const unsigned b4 = ((unsigned)min(ti0 + q, img_h - 1) * (unsigned)img_w + (unsigned)min(tj, img_w - 1)) * 4u;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              tg[t][q][c] = *gol_at(i_tgt + (size_t)c * hw, b4);
              mk[t][q][c] = MC == 0 ? 1.f : (MC == 3 || c == 0) ? *gol_at(i_mask + (size_t)c * hw, b4) : mk[t][q][0];
            }
          }
        }
#pragma unroll
        for (int t = 0; t < CH; ++t) {
          float l1_acc = 0.f;
#pragma unroll
          for (int q = 0; q < PPL; ++q) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float d = (cs[c] - tg[t][q][c]) * mk[t][q][c];
              l1_acc += ok[t][q] ? fabsf(d) : 0.f;
            }
          }
          const float ws = gol_wave_sum_to_lane63(l1_acc);
          if (lane == 63) s_part[(tb + t) * NW + wave] = ws;
        }
      }
    };
    if (!i_mask) l1_tiles(std::integral_constant<int, 0>());
    else if (l1_mask_c == 3) l1_tiles(std::integral_constant<int, 3>());
    else l1_tiles(std::integral_constant<int, 1>());
    __syncthreads();
    if (tid < n) {
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) tot += s_part[tid * NW + w];
      l1_partial[tile0 + tid] = tot;
    }
    return true;
  };
  // (two pixels per lane only: launches of one or two views, which take the four-wave layout, last as long as their longest
  // list's chain and gain nothing from the groups, while the larger kernel ran 6 % longer -- profiles/raster_fwd_bg_ab.txt)
  if (PPL == 2 && bg_group) {   // (kernel-uniform)
    const bool done = bg_group == 2 ? fill_group(std::integral_constant<int, 2>())
                    : bg_group == 4 ? fill_group(std::integral_constant<int, 4>())
                                    : fill_group(std::integral_constant<int, 8>());
    if (done) return;
  } else {
    range = tile_bins[(size_t)view * T + tc.tile];
  }

  int j, i0;
  lane_pixel<PPL>(tc.tx, tc.ty, wave, lane, j, i0);
  bool in[PPL];
  fv py, live;
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    in[q] = (i0 + q < img_h) && (j < img_w);
    py[q] = (float)(i0 + q) + 0.5f;
    // 1 while the pixel still composites, 0 once it stopped (or lies outside the image).  Carried as a FLOAT in a VGPR
    // and multiplied into alpha: a dead pixel then fails the alpha >= 1/255 test by itself.  As loop-carried booleans the
    // same state lived in SGPR lane masks and cost ~30 scalar instructions per visit to maintain (PMC: the scalar pipes
    // of this kernel were as busy as the vector pipes, 76 % / 78 %).
    live[q] = in[q] ? 1.f : 0.f;
  }
  const float px = (float)j + 0.5f;

  const int32_t* ids = sorted_ids + (size_t)view * capacity;
  const size_t goff = (size_t)view * N;
  // (optional) the wave mask of every staged entry, one byte at the entry's list index, for the backward of this render: a
  // batch is staged whole, and a pixel's final_idx lies in a batch that was staged, so every entry the backward can
  // start from or pass has its byte.  (Two pixels per lane only: the backward's own footprint unless it is forced, and in
  // the four-wave forward the store costs the <no extra, lazy> instance a wave per SIMD, 64 -> 66 VGPRs.)
  uint8_t* __restrict__ o_mask = (PPL == 2 && stage_mask) ? stage_mask + (size_t)view * capacity : nullptr;

  fv T_cur = 1.f;
  iv cur_idx = 0;
  fv acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;

  const int n_batches = (range.y - range.x + kBatch - 1) / kBatch;
  for (int bb = 0; bb < n_batches; ++bb) {
    if (__syncthreads_and(!any_live<fv, PPL>(live))) break;  // also protects the LDS batch from being overwritten early
    const int batch_start = range.x + bb * kBatch;
    for (int k = tid; k < kBatch; k += NT) {
      const int idx = batch_start + k;
      if (idx < range.y) {
        const Staged st = stage_entry<PPL>(records, goff + (size_t)ids[idx], (float)(tc.tx * 16), (float)(tc.ty * 16));
        s_a[k] = st.a; s_b[k] = st.b; s_c[k] = st.c; s_mask[k] = st.mask;
        if (PPL == 2 && o_mask) *gol_at(o_mask, (unsigned)idx) = (uint8_t)st.mask;   // consecutive threads, consecutive bytes
      } else {
        s_mask[k] = 0;
      }
    }
    __syncthreads();
    const int batch_size = min(kBatch, range.y - batch_start);
    // Each wave walks ONLY the entries whose alpha >= 1/255 region touches its footprint: one ballot per
    // 64 entries, then a scalar loop over the set bits (s_ff1) -- culled entries cost nothing.
    for (int chunk = 0; chunk < batch_size; chunk += 64) {
      unsigned long long bits = gol_ballot((s_mask[chunk + lane] >> wave) & 1);
      if (LAZY && gol_ballot(any_live<fv, PPL>(live)) == 0ull) break;  // footprint finished
      while (bits) {
        if (!LAZY && gol_ballot(any_live<fv, PPL>(live)) == 0ull) { chunk = batch_size; break; }  // this wave's footprint is finished
        const int t = chunk + __builtin_ctzll(bits);
        bits &= bits - 1;
        const float4 a4 = s_a[t];
        const float4 b4 = s_b[t];
        const float2 c2 = s_c[t];
        // branch-free pixel update: selects instead of exec-mask regions (the loop is issue-bound)
        const float dx = a4.x - px;
        const fv dy = a4.y - py;
        fv sigma, e, alpha, vis, next_T;
        visit_falloff<PPL>(a4.z, a4.w, b4.x, dx, dy, sigma, e);
#pragma unroll
        for (int q = 0; q < PPL; ++q) alpha[q] = fminf(GOL_ALPHA_CAP_FWD, b4.y * e[q]);
        bool take[PPL];
        unsigned long long stop_m[PPL];
        const unsigned long long any_stop = fwd_step<PPL>(sigma, alpha, live, T_cur, vis, next_T, take, stop_m);
        bool half_done = false;
        if (!LAZY || any_stop != 0ull) {   // LAZY: wave-uniform and rare -- some pixel stops here
#pragma unroll
          for (int q = 0; q < PPL; ++q) {
            const bool stop = __builtin_amdgcn_inverse_ballot_w64(stop_m[q]);
            live[q] = stop ? 0.f : live[q];
            if (LAZY) cur_idx[q] = stop ? (batch_start + t - 1) : cur_idx[q];
          }
          if (LAZY) half_done = gol_ballot(any_live<fv, PPL>(live)) == 0ull;
        }
        fwd_take<PPL>(take, next_T, vis, T_cur);
        acc0 += b4.z * vis; acc1 += b4.w * vis; acc2 += c2.x * vis;
        if (EXTRA) acc3 += c2.y * vis;
        if (!LAZY) {
#pragma unroll
          for (int q = 0; q < PPL; ++q) cur_idx[q] = take[q] ? (batch_start + t) : cur_idx[q];
        }
        if (LAZY && half_done) { chunk = batch_size; break; }
      }
    }
  }
  if (LAZY) {   // a pixel that never stopped may have taken entries up to the end of the list
#pragma unroll
    for (int q = 0; q < PPL; ++q) cur_idx[q] = live[q] != 0.f ? range.y - 1 : cur_idx[q];
  }

  // planar: [B,3,H,W] (what the model consumes, rgca.py:139); else gsplat's [B,H,W,3].
  // Addressing: wave-uniform per-view base pointers (scalar registers) + one 32-bit pixel offset per lane, so every
  // access is the SGPR-base + VGPR-offset form -- the epilogue runs for ALL tiles (71 % of them empty at the benchmarked
  // views) and 64-bit per-lane address arithmetic was a visible share of the kernel's vector instructions.
  const unsigned hw = (unsigned)img_h * (unsigned)img_w;
  const size_t vplane = (size_t)view * hw;
  float* __restrict__ o_T = final_Ts + vplane;
  int32_t* __restrict__ o_idx = final_idx + vplane;
  float* __restrict__ o_img = out_img + 3 * vplane;
  float* __restrict__ o_ex = (EXTRA && out_extra) ? out_extra + vplane : nullptr;
  float* __restrict__ o_alpha = out_alpha ? out_alpha + vplane : nullptr;
  float* __restrict__ o_norm = (EXTRA && out_extra_norm) ? out_extra_norm + vplane : nullptr;
  const float* __restrict__ i_tgt = l1_target ? l1_target + 3 * vplane : nullptr;
  const float* __restrict__ i_mask = l1_mask ? l1_mask + (size_t)l1_mask_c * vplane : nullptr;
  uint8_t* __restrict__ o_sign = l1_target ? l1_sign + vplane : nullptr;
  const float bg0 = background[0], bg1 = background[1], bg2 = background[2];
  // channel planes as separate uniform bases (non-planar: element 3 * pix + c)
  float* __restrict__ o_img1 = o_img + (planar ? hw : 1u);
  float* __restrict__ o_img2 = o_img + (planar ? 2u * hw : 2u);
  // a tile without entries: its final_idx / sign bytes are never read (the backward skips the tile: its range is
  // empty) -- 5 of the 41 bytes per pixel that the epilogue moves for the ~70 % empty tiles of a head-and-shoulders view
  // (final_T = 1 is still written: render_gsplat.render returns it)
  const bool bwd_state = range.y > range.x;
  float l1_acc = 0.f;
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    if (!in[q]) continue;
    const unsigned pix = (unsigned)(i0 + q) * (unsigned)img_w + (unsigned)j;
    const unsigned b4 = pix * 4u;                  // byte offset inside a one-channel plane (checked < 4 GiB on the host)
    const unsigned bimg = planar ? b4 : 3u * b4;
    const float Tq = T_cur[q];
    const float c0 = acc0[q] + Tq * bg0, c1 = acc1[q] + Tq * bg1, c2 = acc2[q] + Tq * bg2, ex = acc3[q];
    *gol_at(o_T, b4) = Tq;
    if (bwd_state || !LAZY) *gol_at(o_idx, b4) = cur_idx[q];
    *gol_at(o_img, bimg) = c0; *gol_at(o_img1, bimg) = c1; *gol_at(o_img2, bimg) = c2;
    if (o_ex) *gol_at(o_ex, b4) = ex;
    // optional fused epilogue of AutoEncoder.render (rgca.py:137,144-145): alpha = 1 - T, depth / clamp(alpha, lo, 1)
    if (o_alpha) *gol_at(o_alpha, b4) = 1.f - Tq;
    if (o_norm) *gol_at(o_norm, b4) = ex / fminf(fmaxf(1.f - Tq, norm_lo), 1.f);
    // optional fused masked L1 against a target image (rgb_l1, ca_code/loss/__init__.py:391-411; planar layout): the
    // |difference| goes into a per-tile partial sum and its sign -- the loss gradient up to mask x scalar -- into ONE
    // byte per pixel (2 bits per channel: sign + 1), which the backward decodes as its upstream image gradient: the two
    // separate passes over the image of the loss disappear, and the epilogue writes 1 instead of 12 bytes per pixel for
    // it (the epilogue's traffic is not hidden: 71 % of the tiles of the benchmarked views are empty and do nothing else)
    if (i_tgt) {
      const float m0 = i_mask ? *gol_at(i_mask, b4) : 1.f;
      const float cs[3] = {c0, c1, c2};
      unsigned code = 0u;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float m = (i_mask && l1_mask_c == 3) ? *gol_at(i_mask + (size_t)c * hw, b4) : m0;
        const float d = (cs[c] - *gol_at(i_tgt + (size_t)c * hw, b4)) * m;
        l1_acc += fabsf(d);
        code |= (d > 0.f ? 2u : (d < 0.f ? 0u : 1u)) << (2 * c);
      }
      if (bwd_state) *gol_at(o_sign, pix) = (uint8_t)code;
    }
  }
  if (l1_target) {  // (kernel-uniform) per-tile sum of |difference|: the caller adds the tiles up (deterministic)
    const float ws = gol_wave_sum_to_lane63(l1_acc);
    if (lane == 63) s_l1[wave] = ws;
    __syncthreads();
    if (tid == 0) {
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) tot += s_l1[w];
      l1_partial[(size_t)view * T + tc.tile] = tot;
    }
  }
}

// loss value of the fused L1: l1_out[0] = scale * sum(l1_partial[0 .. n)), one workgroup, fixed summation order.  (Folding
// this into the raster launch itself -- the last workgroup to finish adds the partial sums up -- was measured in round 4:
// the device-scope fence every workgroup then needs before its ticket writes back / invalidates L2 and took the 8-view step
// from 2.9 to 6.7 ms; a 3 us kernel of its own replaces the ATen reduction + multiply of rounds 1-3.)
__global__ __launch_bounds__(1024) void l1_sum_kernel(int n, const float* __restrict__ l1_partial, float scale,
                                                      float* __restrict__ l1_out) {
  __shared__ float s_w[16];
  // 16-byte loads, four of them in flight per lane (a plain strided loop waits for every load: 33 us for 86 k floats)
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  const int n4 = n >> 2;
  const float4* p4 = reinterpret_cast<const float4*>(l1_partial);
  int i = threadIdx.x;
  for (; i + 3 * 1024 < n4; i += 4 * 1024) {
    const float4 v0 = p4[i], v1 = p4[i + 1024], v2 = p4[i + 2048], v3 = p4[i + 3072];
    a0 += (v0.x + v0.y) + (v0.z + v0.w); a1 += (v1.x + v1.y) + (v1.z + v1.w);
    a2 += (v2.x + v2.y) + (v2.z + v2.w); a3 += (v3.x + v3.y) + (v3.z + v3.w);
  }
  for (; i < n4; i += 1024) { const float4 v = p4[i]; a0 += (v.x + v.y) + (v.z + v.w); }
  if ((int)threadIdx.x < (n & 3)) a1 += l1_partial[4 * n4 + threadIdx.x];
  const float ws = gol_wave_sum_to_lane63((a0 + a1) + (a2 + a3));
  if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += s_w[w];
    l1_out[0] = tot * scale;
  }
}

constexpr int kBatchB = 64;   // backward batch (smaller: per-wave gradient slots live in LDS)
constexpr int kAcc = 12;      // r g b M0 | Mx My Mxx Mxy | Myy extra - -   (M = moments of gop, M0 = opacity * v_opacity; see the loop)

// ---- backward ------------------------------------------------------------------------------------
// Same workgroup / wave / lane layout as the forward (Pix).  With two pixels per lane the per-pixel recurrences of the
// two pixels are independent, so the body is written on 2-vectors and maps onto packed fp32 VALU ops (v_pk_fma/mul/add_f32:
// two pixels per instruction), and the cross-lane reduction of the 10 per-Gaussian sums -- the largest single cost
// of the one-pixel-per-lane kernel -- is paid once per 128 pixels instead of once per 64.
static_assert(kBatchB == 64, "raster_bwd_kernel ballots one 64-entry chunk per batch");

template <bool EXTRA, bool PACKED, int PPL>
__global__ __launch_bounds__(64 * Pix<PPL>::kWaves) void raster_bwd_kernel(
    int N, int img_h, int img_w, int planar, int tiles_x, int tiles_y, const int2* __restrict__ tile_bins,
    const int32_t* __restrict__ sorted_ids, int64_t capacity, const float* __restrict__ records,
    const float* __restrict__ background,
    const float* __restrict__ final_Ts, const int32_t* __restrict__ final_idx,
    const float* __restrict__ v_out_img, const float* __restrict__ v_out_extra,
    const float* __restrict__ v_out_alpha, float* __restrict__ v_xy, float* __restrict__ v_conic,
    float* __restrict__ v_colors, float* __restrict__ v_extra, float* __restrict__ v_opacity,
    const uint8_t* __restrict__ v_sign, const float* __restrict__ v_sign_mask, int v_sign_mask_c,
    const float* __restrict__ v_img_scale, float v_img_scale_mul, int n_views, const uint8_t* __restrict__ stage_mask) {
  typedef typename Pix<PPL>::fv fv;
  typedef typename Pix<PPL>::iv iv;
  constexpr int NW = Pix<PPL>::kWaves, NT = 64 * NW;
  __shared__ StagedRow s_e[kBatchB];  // one 48-byte row per entry: the reads of a visit share their address register
  __shared__ int32_t s_mask[kBatchB];
  __shared__ int32_t s_id[kBatchB];
  __shared__ __attribute__((aligned(16))) float s_acc[NW][kBatchB][kAcc];
  __shared__ int32_t s_touched[NW][kBatchB];
  __shared__ int32_t s_wmax[NW];
  const int T = tiles_x * tiles_y;
  const int view = blockIdx.x % n_views, slot = blockIdx.x / n_views;   // (see raster_fwd_kernel)
  const TileCoord tc = tile_of_block(slot, T, tiles_x);
  if (!tc.ok) return;
  const int2 range = tile_bins[(size_t)view * T + tc.tile];
  if (range.y <= range.x) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int j, i0;
  lane_pixel<PPL>(tc.tx, tc.ty, wave, lane, j, i0);
  const float px = (float)j + 0.5f;
  const size_t hw = (size_t)img_h * img_w;
  const int32_t* ids = sorted_ids + (size_t)view * capacity;
  const size_t goff = (size_t)view * N;
  bool in[PPL];
  size_t pp[PPL];
  fv py, T_final;
  iv bin_final;
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    in[q] = (i0 + q < img_h) && (j < img_w);
    py[q] = (float)(i0 + q) + 0.5f;
    pp[q] = in[q] ? ((size_t)view * img_h + i0 + q) * img_w + j : 0;
    T_final[q] = in[q] ? final_Ts[pp[q]] : 1.f;
    bin_final[q] = in[q] ? final_idx[pp[q]] : (range.x - 1);
  }
  fv T_cur = T_final;
  fv vo0 = 0.f, vo1 = 0.f, vo2 = 0.f, vo3 = 0.f, voa = 0.f;
  {
    // upstream image gradient = v_out_img (optional) + the fused L1's term: (sign code - 1) x mask x v_img_scale, with the
    // sign codes the forward epilogue left (one byte per pixel) and the scalar g / n as a device value (no sync)
    const float vsc = (v_img_scale ? v_img_scale[0] : 1.f) * v_img_scale_mul;
    const size_t os = planar ? hw : 1;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
      if (!in[q]) continue;
      const size_t p = pp[q];
      const int i = i0 + q;
      const size_t o = planar ? (size_t)view * 3 * hw + (size_t)i * img_w + j : 3 * p;
      float g0 = 0.f, g1 = 0.f, g2 = 0.f;
      if (v_out_img) { g0 = v_out_img[o]; g1 = v_out_img[o + os]; g2 = v_out_img[o + 2 * os]; }
      if (v_sign) {
        const unsigned code = v_sign[p];
        float m0 = vsc, m1 = vsc, m2 = vsc;
        if (v_sign_mask) {
          const float* mk = v_sign_mask + (size_t)view * v_sign_mask_c * hw + (size_t)i * img_w + j;
          m0 *= mk[0]; m1 *= (v_sign_mask_c == 3) ? mk[hw] : mk[0]; m2 *= (v_sign_mask_c == 3) ? mk[2 * hw] : mk[0];
        }
        g0 += (float)((int)(code & 3u) - 1) * m0;
        g1 += (float)((int)((code >> 2) & 3u) - 1) * m1;
        g2 += (float)((int)((code >> 4) & 3u) - 1) * m2;
      }
      vo0[q] = g0; vo1[q] = g1; vo2[q] = g2;
      if (EXTRA && v_out_extra) vo3[q] = v_out_extra[p];
      if (v_out_alpha) voa[q] = v_out_alpha[p];
    }
  }
  // composite of <colour, v_out> over what lies behind the current entry: at the start, the background (see bwd_moments)
  fv R = (background[0] * vo0 + background[1] * vo1 + background[2] * vo2) - voa;

  const int wmax = wave_last_entry<PPL>(bin_final);
  if (lane == 0) s_wmax[wave] = wmax;
  __syncthreads();
  int bmax = s_wmax[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) bmax = max(bmax, s_wmax[w]);
  bmax = min(bmax, range.y - 1);
  if (bmax < range.x) return;

  // this lane's column of the slot rows.  PPL = 1: lane 8 k + 7 holds sum k of the first eight (gol_wave_sum8).  PPL = 2:
  // the lanes 8 k + 7 and lane 19 hold the nine sums of gol_wave_colsum, in the slot order kColSlot (a nibble per k):
  //   lane   7  15  23  31  39  47  55  63 | 19
  //   slot   0   3   2   4   1   5   8   7 |  6
  constexpr unsigned kColSlot = 0x78514230u;
  const bool res_lane = (lane & 7) == 7 || (PPL == 2 && lane == 19);
  const int acc_col = PPL == 1 ? lane >> 3 : lane == 19 ? 6 : (int)((kColSlot >> (4 * (lane >> 3))) & 15u);
  float* acc_lane = &s_acc[wave][0][acc_col];
  const int n_batches = (bmax - range.x + kBatchB) / kBatchB;
  // A batch is staged through two dependent loads (list id -> the Gaussian's record).  The id of the NEXT batch's entry is
  // fetched while this batch is being worked on, so that only the record gather is left behind the barrier (nothing hides it
  // in the tail of a launch, when a SIMD is down to one or two waves).
  auto entry_id = [&](int bb2) {
    const int e = bmax - bb2 * kBatchB - tid;
    return (tid < kBatchB && e >= range.x) ? ids[e] : 0;
  };
  // stage_mask (kernel-uniform; NULL = run the reach test here): the wave masks this render's forward staged with the same
  // footprints, one byte per list entry.  The byte rides the id's prefetch, and staging is three 16-byte loads and no test
  const uint8_t* __restrict__ i_mask = stage_mask ? stage_mask + (size_t)view * capacity : nullptr;
  auto entry_mask = [&](int bb2) {
    const int e = bmax - bb2 * kBatchB - tid;
    return (i_mask && tid < kBatchB && e >= range.x) ? (int)i_mask[e] : 0;
  };
  int gid_next = entry_id(0), mask_next = entry_mask(0);
  // (PACKED) bytes of a gradient record as a value the compiler cannot see through: with the constant, id * 64 + base
  // becomes a 64-bit shift and a 64-bit add per atomic; with an opaque factor it is one v_mad_u64_u32
  unsigned rec_bytes = GOL_GRAD_RECORD * sizeof(float);
  if (PACKED) asm volatile("" : "+s"(rec_bytes));
  for (int bb = 0; bb < n_batches; ++bb) {
    __syncthreads();
    const int batch_end = bmax - bb * kBatchB;
    const int batch_size = min(kBatchB, batch_end + 1 - range.x);
    const int gid = gid_next, mask = mask_next;
    if (tid < kBatchB) {
      if (tid < batch_size) {
        const Staged st = i_mask ? stage_entry_masked(records, goff + (size_t)gid, mask)
                                 : stage_entry<PPL>(records, goff + (size_t)gid, (float)(tc.tx * 16), (float)(tc.ty * 16));
        s_e[tid].a = st.a; s_e[tid].b = st.b; s_e[tid].c = st.c; s_mask[tid] = st.mask;
        s_id[tid] = gid;
      } else {
        s_mask[tid] = 0;
      }
    }
    if (bb + 1 < n_batches) { gid_next = entry_id(bb + 1); mask_next = entry_mask(bb + 1); }
    __syncthreads();

    const int t0 = max(0, batch_end - wmax);
    unsigned long long bits = gol_ballot((s_mask[lane] >> wave) & 1);  // kBatchB == 64: one chunk
    if (t0 > 0) bits &= ~0ull << t0;
    // the entries this wave reduces in this batch, as a wave-uniform 64-bit mask (scalar operations only); stored once,
    // after the loop -- not as one LDS write per visit into a row that has to be cleared per batch
    unsigned long long touched = 0ull;
    while (bits) {
      const int t = __builtin_ctzll(bits);
      bits &= bits - 1;
      const float4 a4 = s_e[t].a;
      const float4 b4 = s_e[t].b;
      const float2 c2 = s_e[t].c;
      const int li = batch_end - t;
      const float dx = a4.x - px;
      const fv dy = a4.y - py;
      fv sigma, vis, raw, alpha, ra, fac;
      visit_falloff<PPL>(a4.z, a4.w, b4.x, dx, dy, sigma, vis);
      unsigned long long mv[PPL];
      if (bwd_taken<PPL>(b4.y, vis, sigma, li, bin_final, raw, mv) == 0ull) continue;
      bwd_recur<PPL>(mv, raw, T_cur, alpha, ra, fac);
      // all channels enter through ONE dot product with the upstream gradient (see bwd_moments)
      fv w = b4.z * vo0 + b4.w * vo1 + c2.x * vo2;
      if (EXTRA) w += c2.y * vo3;
      fv gop, gy, gyy;
      bwd_moments<PPL>(raw, w, T_cur, alpha, dy, R, gop, gy, gyy);
      // the colour sums of the lane's pixels (PPL = 2: one multiply + one scalar FMA per colour sum -- written on scalars:
      // from the 2-vector form the compiler builds v_mul + v_pk_fma and throws the packed op's upper half away)
      float g0s, g1s, g2s, g3 = 0.f;
      if (PPL == 2) {
        g0s = __builtin_fmaf(fac[0], vo0[0], fac[PPL - 1] * vo0[PPL - 1]);
        g1s = __builtin_fmaf(fac[0], vo1[0], fac[PPL - 1] * vo1[PPL - 1]);
        g2s = __builtin_fmaf(fac[0], vo2[0], fac[PPL - 1] * vo2[PPL - 1]);
        if (EXTRA) g3 = __builtin_fmaf(fac[0], vo3[0], fac[PPL - 1] * vo3[PPL - 1]);
      } else {
        g0s = fac[0] * vo0[0]; g1s = fac[0] * vo1[0]; g2s = fac[0] * vo2[0];
        if (EXTRA) g3 = fac[0] * vo3[0];
      }
      const float m0 = lane_sum<PPL>(gop), my = lane_sum<PPL>(gy), myy = lane_sum<PPL>(gyy);
      if constexpr (PPL == 2) {
        // dx is constant down a column of lanes (lane = 16 r + x): only the six plain sums cross the rows, the three
        // x-moments are formed on the column sums of m0 and my (gol_wave_colsum); nine results, one slot write per lane
        // the depth gradient's sum keeps its 6-instruction DPP ladder (total in lane 63)
        const float r3 = EXTRA ? gol_wave_sum_to_lane63(g3) : 0.f;
        const float r0 = gol_wave_colsum(g0s, g1s, g2s, m0, my, myy, dx);
        if (res_lane) {
          // slot row t of this wave + a 32-bit byte offset (plain pointer arithmetic on the int t becomes a v_mad_u64_u32,
          // and so does the offset's own multiply when one store is all that uses it: kept in an SGPR, it is one v_add_u32)
          unsigned row_t = (unsigned)t * (unsigned)(kAcc * sizeof(float));
          asm("" : "+s"(row_t));
          float* a = gol_at(acc_lane, row_t);
          a[0] = r0;
          if (EXTRA && lane == 63) a[9 - 7] = r3;   // (lane 63's base points at slot 7; without EXTRA no merge uses slot 9)
        }
      } else {
        const float mx = m0 * dx, mxx = mx * dx, mxy = my * dx;
        // the first eight sums in one 8-way reduction: lane 16 r + 7 gets argument r, lane 16 r + 15 argument 4 + r, so with
        // the even slots first and the odd ones after them lane 8 k + 7 holds slot k
        const float r0 = gol_wave_sum8(g0s, g2s, mx, mxx, g1s, m0, my, mxy);
        // the 9th (and 10th) sum: a 6-instruction DPP ladder each (total in lane 63) instead of a second 4-way reduction
        const float r2 = gol_wave_sum_to_lane63(myy);
        const float r3 = EXTRA ? gol_wave_sum_to_lane63(g3) : 0.f;
        if (res_lane) {
          // slot row t of this wave + a 32-bit byte offset (plain pointer arithmetic on the int t becomes a v_mad_u64_u32)
          float* a = gol_at(acc_lane, (unsigned)t * (unsigned)(kAcc * sizeof(float)));
          a[0] = r0;
          if (lane == 63) { a[8 - 7] = r2; a[9 - 7] = r3; }  // (lane 63's base points at slot 7)
        }
      }
      touched |= 1ull << t;
    }
    // lane l owns the flag of entry l (kBatchB == 64): every flag of the row is written, the zeros too, so the row needs no
    // clearing; the last readers of the previous batch's flags (the merge) are behind the barrier at the top of the batch
    s_touched[wave][lane] = (int32_t)((touched >> lane) & 1ull);
    __syncthreads();
    if (PACKED) {
      // gradients live in 64-byte records [r g b | opacity | x y | conic a b c | extra | pad]: 16 consecutive
      // lanes own one Gaussian's record, so an atomic instruction touches 4 cache lines instead of 64
      // The merge of a batch: two phases with a barrier between them.
      // Phase 1, one thread per entry (wave 0; an entry past batch_size has no flag set): the waves' slot rows are summed
      // and the entry's weights formed ONCE -- not once per (entry, component) lane, which cost ~590 VALU per full batch
      // against ~70 now -- and the finished record goes back into wave 0's row in record order.  Each thread reads all
      // rows of its own entry before it writes one of them.
      if (tid < kBatchB) {
        int tw[NW];   // the flags of all waves in flight together
#pragma unroll
        for (int w = 0; w < NW; ++w) tw[w] = s_touched[w][tid];
        float s[kAcc];
#pragma unroll
        for (int k = 0; k < kAcc; ++k) s[k] = 0.f;
        bool any = false;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          if (tw[w]) {
            any = true;
            const float4* q = reinterpret_cast<const float4*>(&s_acc[w][tid][0]);
            const float4 q0 = q[0], q1 = q[1], q2 = q[2];
            s[0] += q0.x; s[1] += q0.y; s[2] += q0.z; s[3] += q0.w;
            s[4] += q1.x; s[5] += q1.y; s[6] += q1.z; s[7] += q1.w;
            s[8] += q2.x; s[9] += q2.y;
          }
        }
        if (any) {
          // (the three merges keep their own arithmetic form of the weights: a common one changes these kernels' code)
          // slots 3..8 hold moments of gop = opacity e v_alpha (bwd_moments): v_sigma-sums = -moment (conic back from its
          // log2e scaling with ln 2), v_opacity = M0 / opacity -- a true division, once per entry; a touched entry was taken
          // with opacity e >= 1/255, so opacity > 0
          const float4 a4 = s_e[tid].a;
          const float4 b4 = s_e[tid].b;
          const float cc = b4.x;
          const float wxx = -a4.z * kUnA, wxy = -a4.w * kUnB, wyy = -cc * kUnA;
          float4* o = reinterpret_cast<float4*>(&s_acc[0][tid][0]);
          o[0] = make_float4(s[0], s[1], s[2], s[3] / b4.y);
          o[1] = make_float4(wxx * s[4] + wxy * s[5], wxy * s[4] + wyy * s[5], -0.5f * s[6], -s[7]);
          *reinterpret_cast<float2*>(o + 2) = make_float2(-0.5f * s[8], s[9]);
          s_touched[0][tid] = 1;
        }
      }
      __syncthreads();
      // Phase 2: lane (t, c) adds component c of entry t's record; the lane's component, and with it the address part that
      // does not depend on the entry, stays the same over the loop (NT is a multiple of 16)
      const int c = tid & 15;
      if (c <= (EXTRA ? 9 : 8)) {
        float* rec_c = v_colors + goff * 16 + c;
        // A fixed trip count (entries past batch_size have no flag set) in chunks of four entries per lane whose LDS reads
        // are in flight together.  One entry per iteration (flag, then id and value: two dependent LDS round trips each)
        // makes the merge a latency chain per batch; 8 views per launch hide it behind other waves, the shorter launches
        // of the two-stream step and of single views do not (step 2.67 -> 2.66 ms with that loop, 2.61 ms with this one).
        // Whole batches in flight (kCh = kIt, phase 1 alike) gain another 0.2 % but cost the 4-wave kernel two waves per SIMD.
        constexpr int kIt = kBatchB * 16 / NT, kCh = 4;
        static_assert(kIt % kCh == 0, "the merge issues its atomics in chunks of kCh entries per lane");
#pragma unroll
        for (int i0 = 0; i0 < kIt; i0 += kCh) {
          int flag[kCh], id[kCh];
          float val[kCh];
#pragma unroll
          for (int i = 0; i < kCh; ++i) {
            const int t = (tid >> 4) + (i0 + i) * (NT / 16);
            flag[i] = s_touched[0][t]; id[i] = s_id[t]; val[i] = s_acc[0][t][c];
          }
#pragma unroll
          for (int i = 0; i < kCh; ++i) {
            // record of the entry: id x rec_bytes + rec_c as ONE v_mad_u64_u32 (see rec_bytes)
            if (flag[i]) {
              char* r = reinterpret_cast<char*>(rec_c) + (uint64_t)(unsigned)id[i] * rec_bytes;
              atomicAdd(reinterpret_cast<float*>(r), val[i]);
            }
          }
        }
      }
    } else if (tid < batch_size) {
      float a[kAcc];
#pragma unroll
      for (int k = 0; k < kAcc; ++k) a[k] = 0.f;
      bool any = false;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (s_touched[w][tid]) {
          any = true;
          const float4* q = reinterpret_cast<const float4*>(&s_acc[w][tid][0]);
          const float4 q0 = q[0], q1 = q[1], q2 = q[2];
          a[0] += q0.x; a[1] += q0.y; a[2] += q0.z; a[3] += q0.w;
          a[4] += q1.x; a[5] += q1.y; a[6] += q1.z; a[7] += q1.w;
          a[8] += q2.x; a[9] += q2.y;
        }
      }
      if (any) {
        const size_t g = goff + (size_t)s_id[tid];
        const float4 a4 = s_e[tid].a;
        const float4 b4 = s_e[tid].b;
        // slots 3..8 are moments of gop = opacity e v_alpha: v_sigma-sums = -moment, v_opacity = M0 / opacity (> 0: see
        // the packed merge, whose weights these are with the sign factored out of the x / y sums)
        const float3 cn = true_conic(a4.z, a4.w, b4.x);
        atomicAdd(v_colors + 3 * g, a[0]); atomicAdd(v_colors + 3 * g + 1, a[1]); atomicAdd(v_colors + 3 * g + 2, a[2]);
        atomicAdd(v_opacity + g, a[3] / b4.y);
        atomicAdd(v_xy + 2 * g, -(cn.x * a[4] + cn.y * a[5]));
        atomicAdd(v_xy + 2 * g + 1, -(cn.y * a[4] + cn.z * a[5]));
        atomicAdd(v_conic + 3 * g, -0.5f * a[6]); atomicAdd(v_conic + 3 * g + 1, -a[7]);
        atomicAdd(v_conic + 3 * g + 2, -0.5f * a[8]);
        if (EXTRA && v_extra) atomicAdd(v_extra + g, a[9]);
      }
    }
  }
}

// DIAGNOSTIC (bench.py's algorithmic roofline): per view, the number of (pixel, list entry) pairs up to the pixel's
// final_idx ("tested": what any per-pixel compositor has to look at) and of those with alpha >= 1/255 ("taken": what is
// composited and differentiated).  One thread per pixel, no staging: slow and simple.
__global__ __launch_bounds__(256) void raster_count_pairs_kernel(int N, int img_h, int img_w, int tiles_x, int tiles_y,
                                                                 const int2* __restrict__ tile_bins,
                                                                 const int32_t* __restrict__ sorted_ids, int64_t capacity,
                                                                 const float* __restrict__ records,
                                                                 const int32_t* __restrict__ final_idx,
                                                                 unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_cnt[2];
  const int view = blockIdx.y, tile = blockIdx.x, T = tiles_x * tiles_y;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int j = tx * 16 + (threadIdx.x & 15), i = ty * 16 + (threadIdx.x >> 4);
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0ull;
  __syncthreads();
  const int2 range = tile_bins[(size_t)view * T + tile];
  unsigned long long tested = 0, taken = 0;
  if (i < img_h && j < img_w && range.y > range.x) {
    const int last = min(range.y - 1, final_idx[((size_t)view * img_h + i) * img_w + j]);
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    for (int li = range.x; li <= last; ++li) {
      const float4* R = reinterpret_cast<const float4*>(records + ((size_t)view * N + sorted_ids[(size_t)view * capacity + li]) * GOL_SPLAT_RECORD);
      const float4 q0 = R[0], q1 = R[1];
      const float dx = q0.x - px, dy = q0.y - py;
      f1 sg, e;
      visit_falloff<1>(q0.z, q0.w, q1.x, dx, f1(dy), sg, e);
      const float alpha = fminf(GOL_ALPHA_CAP_FWD, q1.y * e[0]);
      ++tested;
      taken += (!(sg[0] < 0.f) && !(alpha < GOL_ALPHA_FLOOR)) ? 1 : 0;
    }
  }
  atomicAdd(&s_cnt[0], tested);
  atomicAdd(&s_cnt[1], taken);
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(counts + 2 * view + threadIdx.x, s_cnt[threadIdx.x]);
}

// gsplat-compatible operators hand over separate attribute arrays: pack them into records (the fused path's projection
// writes the records itself); colors == NULL: r = g = b = 0 (the N-channel rasterizer stages its colours separately)
__global__ __launch_bounds__(256) void splat_pack_kernel(size_t n, const float* __restrict__ xys,
                                                         const float* __restrict__ conics,
                                                         const float* __restrict__ colors,
                                                         const float* __restrict__ extra,
                                                         const float* __restrict__ opacities,
                                                         float* __restrict__ records) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  gol_record_write(records + e * GOL_SPLAT_RECORD, xys[2 * e], xys[2 * e + 1], conics[3 * e], conics[3 * e + 1],
                   conics[3 * e + 2], opacities[e], colors ? colors[3 * e] : 0.f, colors ? colors[3 * e + 1] : 0.f,
                   colors ? colors[3 * e + 2] : 0.f, extra ? extra[e] : 0.f);
}

// GOL_RASTER_STAGE_MASK=0: the forward writes no wave masks and the backward runs its own reach test whatever it is handed
// (A/B runs and the parity test; read on every call like GOL_RASTER_BG_GROUP -- they switch it inside one process)
inline bool stage_mask_on() {
  const char* e = getenv("GOL_RASTER_STAGE_MASK");
  return !(e && e[0] == '0' && e[1] == 0);
}

}  // namespace

// The forward's wave footprint for a launch of B views (GOL_RASTER_PPL = 1 | 2 overrides it for experiments).  One or two
// views do not fill the chip for the whole launch: all their workgroups are resident at once, every SIMD keeps the waves it
// was dealt, and the launch lasts until the most loaded SIMD is done (per-workgroup timeline, profiles/r04_raster_tail.txt:
// 2942 workgroups of a view start within 5 us, half of them are done after 120 us, the last one after 257 us; an 8-view
// launch takes 131-148 us per view).  Four waves per tile spread a tile's work over more SIMDs: forward 121 -> 106 us for
// one view; in the backward the 17 % extra instructions of the finer footprint cancel the gain (236 -> 240 us): it keeps
// two pixels per lane.  From three views on the instruction count decides.
extern "C" int gol_raster_plan(int B, int* fwd_pixels_per_lane) {
  static const int forced = getenv("GOL_RASTER_PPL") ? atoi(getenv("GOL_RASTER_PPL")) : 0;
  if (fwd_pixels_per_lane) *fwd_pixels_per_lane = (forced == 1 || forced == 2) ? forced : (B <= 2 ? 1 : 2);
  return GOL_OK;
}

extern "C" int gol_raster_count_pairs(int B, int N, int img_h, int img_w, const int32_t* tile_bins, const int32_t* sorted_ids,
                                      int64_t capacity, const float* records, const int32_t* final_idx, uint64_t* counts,
                                      void* stream) {
  GOL_REQUIRE(B >= 0 && N >= 0 && img_h > 0 && img_w > 0, "bad size");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(tile_bins && final_idx && counts && (capacity == 0 || sorted_ids) && (N == 0 || records), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(uint64_t) * 2 * (size_t)B, s) != hipSuccess) {
    gol_set_error("gol_raster_count_pairs: hipMemsetAsync failed");
    return GOL_ERR_LAUNCH;
  }
  const int tiles_x = (img_w + 15) / 16, tiles_y = (img_h + 15) / 16;
  raster_count_pairs_kernel<<<dim3(tiles_x * tiles_y, B), 256, 0, s>>>(
      N, img_h, img_w, tiles_x, tiles_y, reinterpret_cast<const int2*>(tile_bins), sorted_ids, capacity, records, final_idx,
      reinterpret_cast<unsigned long long*>(counts));
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_splat_pack(int B, int N, const float* xys, const float* conics, const float* colors,
                              const float* extra, const float* opacities, float* records, void* stream) {
  GOL_REQUIRE(B >= 0 && N >= 0, "negative size");
  if (B == 0 || N == 0) return GOL_OK;
  GOL_REQUIRE(xys && conics && opacities && records, "null pointer");
  const size_t n = (size_t)B * N;
  splat_pack_kernel<<<gol_cdiv((long long)n, 256), 256, 0, (hipStream_t)stream>>>(n, xys, conics, colors, extra, opacities,
                                                                                 records);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_rasterize_fwd(int B, int N, int img_h, int img_w, int block, int planar, const int32_t* tile_bins,
                                 const int32_t* sorted_ids, int64_t capacity, const float* records, int with_extra,
                                 const float* background, float* out_img,
                                 float* out_extra, float* final_Ts, int32_t* final_idx, float* out_alpha,
                                 float* out_extra_norm, float norm_lo, const float* l1_target, const float* l1_mask,
                                 int l1_mask_c, uint8_t* l1_sign, float* l1_partial, float* l1_out, float l1_scale,
                                 uint8_t* stage_mask, int pixels_per_lane, void* stream) {
  GOL_RASTER_CHECK_DIMS(12, "image too large (32-bit byte offsets inside a view)");
  if (B == 0) return GOL_OK;
  GOL_REQUIRE(tile_bins && background && out_img && final_Ts && final_idx, "null pointer");
  GOL_REQUIRE(capacity == 0 || sorted_ids, "null sorted_ids");
  GOL_REQUIRE(N == 0 || records, "null Gaussian records");
  GOL_REQUIRE((!out_extra && !out_extra_norm) || with_extra || N == 0, "out_extra / out_extra_norm need the extra channel");
  GOL_REQUIRE(!with_extra || out_extra || out_extra_norm, "extra without an output for it");
  GOL_REQUIRE(!l1_target || (planar && l1_sign && l1_partial), "the fused L1 needs planar images, l1_sign and l1_partial");
  GOL_REQUIRE(!l1_mask || (l1_target && (l1_mask_c == 1 || l1_mask_c == 3)), "l1_mask: 1 or 3 channels, with l1_target");
  GOL_REQUIRE(!l1_out || l1_target, "l1_out needs l1_target");
  const int tiles_x = (img_w + 15) / 16, tiles_y = (img_h + 15) / 16;
  const dim3 grid((unsigned)raster_grid(B, img_h, img_w));
  const int2* bins = reinterpret_cast<const int2*>(tile_bins);
  hipStream_t s = (hipStream_t)stream;
  GOL_REQUIRE(pixels_per_lane >= 0 && pixels_per_lane <= 2, "pixels_per_lane: 0 (choose by B), 1 or 2");
  // one pixel per lane (4 waves per tile) for launches of one or two views: their duration is the longest list's chain
  // through one wave, which the finer footprint shortens to ~0.55x for ~9 % more instructions in total (see Pix)
  int ppl = pixels_per_lane;
  if (ppl == 0) gol_raster_plan(B, &ppl);
  // Runs of empty tiles are filled by one workgroup per group of bg_group tiles (see raster_fwd_kernel).  GOL_RASTER_BG_GROUP
  // = 0 | 2 | 4 | 8 overrides the group size; it is read on every call (A/B runs and the parity test switch it inside one
  // process).  The row stores are 16 bytes per lane where every row of every plane starts on a 16-byte boundary, else 8; an
  // odd width, gsplat's interleaved layout, a plane that is not 8-byte aligned and the four-wave layout (one pixel per lane)
  // keep the per-tile epilogue.
  int bg_group = kBgGroup, bg_vec16 = 0;
  if (const char* e = getenv("GOL_RASTER_BG_GROUP")) bg_group = atoi(e);
  GOL_REQUIRE(bg_group == 0 || bg_group == 2 || bg_group == 4 || bg_group == 8, "GOL_RASTER_BG_GROUP: 0, 2, 4 or 8");
  if (!planar || (img_w & 1) || ppl != 2) bg_group = 0;
  if (bg_group) {
    uintptr_t bits = 0;
    for (const void* p : {(const void*)out_img, (const void*)final_Ts, (const void*)out_extra, (const void*)out_alpha,
                          (const void*)out_extra_norm})
      bits |= reinterpret_cast<uintptr_t>(p);
    bg_vec16 = (img_w % 4 == 0 && bits % 16 == 0) ? 1 : 0;
    if (bits % 8 != 0) bg_group = 0;
  }
  auto launch = [&](auto ex_c, auto lazy_c) {
    with_ppl(ppl, [&](auto ppl_c) {
      constexpr bool EX = decltype(ex_c)::value, LZ = decltype(lazy_c)::value;
      constexpr int PPL = decltype(ppl_c)::value;
      raster_fwd_kernel<EX, LZ, PPL><<<grid, 64 * Pix<PPL>::kWaves, 0, s>>>(
          N, img_h, img_w, planar, tiles_x, tiles_y, bins, sorted_ids, capacity, records, background, out_img, out_extra,
          final_Ts, final_idx, out_alpha, EX ? out_extra_norm : nullptr, norm_lo, l1_target, l1_mask, l1_mask_c, l1_sign,
          l1_partial, B, bg_group, bg_vec16, stage_mask_on() ? stage_mask : nullptr);
    });
  };
  const bool ex = out_extra || out_extra_norm;
  // planar = the fused path: final_idx is the backward's start bound (see raster_fwd_kernel); gsplat's layout: exact
  if (ex && planar) launch(kYes, kYes);
  else if (ex) launch(kYes, kNo);
  else if (planar) launch(kNo, kYes);
  else launch(kNo, kNo);
  if (l1_out) l1_sum_kernel<<<1, 1024, 0, s>>>(B * tiles_x * tiles_y, l1_partial, l1_scale, l1_out);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}

extern "C" int gol_rasterize_bwd(int B, int N, int img_h, int img_w, int block, int planar, const int32_t* tile_bins,
                                 const int32_t* sorted_ids, int64_t capacity, const float* records, int with_extra,
                                 const float* background, const float* final_Ts,
                                 const int32_t* final_idx, const float* v_out_img, const float* v_out_extra,
                                 const float* v_out_alpha, float* v_xy, float* v_conic, float* v_colors,
                                 float* v_extra, float* v_opacity, int grad_stride, const uint8_t* v_sign,
                                 const float* v_sign_mask, int v_sign_mask_c, const float* v_img_scale,
                                 float v_img_scale_mul, const uint8_t* stage_mask, int stage_mask_ppl, int pixels_per_lane,
                                 void* stream) {
  GOL_RASTER_CHECK_DIMS(0, "");   // 0: no 32-bit image offsets in this kernel, no image-size bound
  if (B == 0 || N == 0 || capacity == 0) return GOL_OK;
  GOL_REQUIRE(tile_bins && sorted_ids && background && final_Ts && final_idx, "null pointer");
  GOL_REQUIRE(v_out_img || v_sign, "no upstream image gradient (v_out_img or v_sign)");
  GOL_REQUIRE(!v_sign || planar, "the sign image of the fused L1 goes with planar images");
  GOL_REQUIRE(!v_sign_mask || (v_sign && (v_sign_mask_c == 1 || v_sign_mask_c == 3)), "v_sign_mask: 1 or 3 channels, with v_sign");
  GOL_REQUIRE(records, "null Gaussian records");
  GOL_REQUIRE(v_xy && v_conic && v_colors && v_opacity, "null gradient output");
  GOL_REQUIRE(!(v_out_extra || v_extra) || with_extra, "extra-channel gradients need the extra channel");
  GOL_REQUIRE(grad_stride == 0 || grad_stride == GOL_GRAD_RECORD, "grad_stride must be 0 (dense arrays) or 16 (records)");
  const bool packed = grad_stride == GOL_GRAD_RECORD;
  if (packed)
    GOL_REQUIRE(v_opacity == v_colors + 3 && v_xy == v_colors + 4 && v_conic == v_colors + 6 &&
                    (!v_extra || v_extra == v_colors + 9),
                "record layout is [rgb | opacity | xy | conic | extra | pad] (GOL_GRAD_RECORD floats)");
  const int tiles_x = (img_w + 15) / 16, tiles_y = (img_h + 15) / 16;
  const dim3 grid((unsigned)raster_grid(B, img_h, img_w));
  const int2* bins = reinterpret_cast<const int2*>(tile_bins);
  hipStream_t s = (hipStream_t)stream;
  GOL_REQUIRE(pixels_per_lane >= 0 && pixels_per_lane <= 2, "pixels_per_lane: 0 (2), 1 or 2");
  GOL_REQUIRE(stage_mask_ppl >= 0 && stage_mask_ppl <= 2, "stage_mask_ppl: the forward's pixels_per_lane (1 or 2), 0 = no masks");
  const int ppl = pixels_per_lane ? pixels_per_lane : 2;
  // the forward's wave masks are this launch's only if it staged with the same footprints; else they are computed here
  // (the forward writes them with two pixels per lane only, see raster_fwd_kernel)
  const uint8_t* masks = (stage_mask && stage_mask_ppl == 2 && ppl == 2 && stage_mask_on()) ? stage_mask : nullptr;
  const bool ex = with_extra && (v_out_extra || v_extra);
  auto launch = [&](auto ex_c, auto packed_c) {
    with_ppl(ppl, [&](auto ppl_c) {
      constexpr bool EX = decltype(ex_c)::value, PK = decltype(packed_c)::value;
      constexpr int PPL = decltype(ppl_c)::value;
      raster_bwd_kernel<EX, PK, PPL><<<grid, 64 * Pix<PPL>::kWaves, 0, s>>>(
          N, img_h, img_w, planar, tiles_x, tiles_y, bins, sorted_ids, capacity, records, background, final_Ts, final_idx,
          v_out_img, EX ? v_out_extra : nullptr, v_out_alpha, v_xy, v_conic, v_colors, EX ? v_extra : nullptr, v_opacity,
          v_sign, v_sign_mask, v_sign_mask_c, v_img_scale, v_img_scale_mul, B, masks);
    });
  };
  if (ex && packed) launch(kYes, kYes);
  else if (ex) launch(kYes, kNo);
  else if (packed) launch(kNo, kYes);
  else launch(kNo, kNo);
  GOL_CHECK_LAUNCH();
  return GOL_OK;
}
