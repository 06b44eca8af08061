/*
 * goliath_hip.h -- C ABI of libgoliath_hip.so, the MI355X (gfx950) implementation of the
 * Relightable-Gaussian-Codec-Avatar render hot path of facebookresearch/goliath.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 / int32 data unless it says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream);
 *   - functions only enqueue work (no allocation, no host sync) and return GOL_OK or a negative
 *     gol_status; outputs are caller-owned and pre-allocated, exactly like the reference's
 *     pybind entry points (sg.cu:177-283, mvpraymarch.cpp:107-409, utils.cpp:46-137);
 *   - "[B,N,3]" = row-major, B views (batch elements) x N Gaussians;
 *   - re-entrant given distinct streams and distinct output/scratch buffers.  Process-wide state is limited to
 *     the thread-local last-error text and a monotone per-device cache of the dynamic-LDS limits already
 *     granted to the binning kernels (atomics; a race only repeats an idempotent hipFuncSetAttribute).
 *
 * Each entry cites the reference interface it replaces (paths relative to /root/reference,
 * "gsplat:" = the third-party gsplat==0.1.11 the reference calls).
 */
#ifndef GOLIATH_HIP_H
#define GOLIATH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GOL_OK = 0,
  GOL_ERR_INVALID_ARG = -1,   /* bad size / null pointer / unsupported option */
  GOL_ERR_LAUNCH = -2,        /* hipGetLastError() != hipSuccess after a launch */
  GOL_ERR_UNSUPPORTED = -3
} gol_status;

/* Library / build identification ("goliath_hip <ver> gfx950"). */
const char* gol_version(void);
/* Text of the last error on this thread (static storage). */
const char* gol_last_error(void);
/* Self-test of the wave64 reduction primitives: in256 = 4 x 64 floats (a,b,c,d per lane);
 * out128[0..63] = per-lane result of the 4-way swap reduction (lanes 15/31/47/63 = sums of
 * a/b/c/d), out128[64..127] = per-lane result of the DPP ladder (lane 63 = sum of a). */
int gol_selftest_wave_sum4(const float* in256, float* out128, void* stream);
/* The 8-way reduction: in512 = 8 x 64 floats (a0 .. a7 per lane); out64 = its per-lane result.  Lane 16 r + 7 holds
 * sum(a_r) and lane 16 r + 15 sum(a_{4+r}), r = 0..3; the other lanes hold partial sums. */
int gol_selftest_wave_sum8(const float* in512, float* out64, void* stream);
/* The column-first reduction of the two-pixel raster backward: in384 = 6 x 64 floats (s0, s1, s2, m0, my, myy per lane),
 * dx64 = the factor dx of every lane, equal in lanes l and l + 16; out64 = its per-lane result.  Lanes 7, 39, 23, 55 hold
 * sum(s0), sum(s1), sum(s2), sum(myy); lanes 15, 31, 47, 63 sum(m0), sum(dx m0), sum(my), sum(dx my); lane 19 sum(dx^2 m0). */
int gol_selftest_wave_colsum(const float* in384, const float* dx64, float* out64, void* stream);

/* ------------------------------------------------------------------------------------------
 * sgutils -- spherical-Gaussian specular lobe evaluation.
 * Replaces sgutilslib.evaluate_gaussian_fwd / _bwd (extensions/sgutils/sg.cu:177-226, 228-278;
 * kernels sg.cu:27-76, 78-175), called from extensions/sgutils/sgutils.py:27-29, 50-62.
 *   lobe_dirs[N,D,3] lobe_sigmas[N,D] light_values[N,L,3] light_pts[N,L,3] prim_pts[N,D,3]
 *   n_lights[N] int32, w_type in {0,1,2,3}.
 * fwd writes integral[N,D,3] (every element).  bwd writes grad_dirs[N,D,3], grad_sigmas[N,D]
 * and, when grad_light_values != NULL, ACCUMULATES into grad_light_values[N,L,3] (caller zeroes).
 * ---------------------------------------------------------------------------------------- */
int gol_sg_eval_fwd(int N, int D, int L, const float* lobe_dirs, const float* lobe_sigmas,
                    const float* light_values, const float* light_pts, const float* prim_pts,
                    const int32_t* n_lights, float* integral, int w_type, void* stream);
int gol_sg_eval_bwd(int N, int D, int L, const float* lobe_dirs, const float* lobe_sigmas,
                    const float* light_values, const float* light_pts, const float* prim_pts,
                    const int32_t* n_lights, const float* grad_integral, float* grad_dirs,
                    float* grad_sigmas, float* grad_light_values, int w_type, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gaussian projection (EWA).  Replaces gsplat: project_gaussians forward/backward
 * (call site ca_code/utils/render_gsplat.py:49-63; semantics SURVEY.md A.1, A.5).
 * Batched over B views: viewmats[B,12] (row-major 3x4 world->camera), intrins[B,4]=(fx,fy,cx,cy)
 * live on the device so no host sync is needed to read K (cf. rgca.py:123-126 .item() x4).
 * Outputs for culled Gaussians are zero (radii = num_tiles_hit = 0).  cov3d and num_tiles_hit may be NULL (not written);
 * gol_project_bwd with cov3d == NULL recomputes Sigma from the scales and quaternions (the forward's own arithmetic).
 * Optional fused extras (pass NULL to skip):
 *   opacities[B,N] -> opac_eff[B,N] = opacity * compensation   (render_gsplat.py:72)
 *   colors[B,N,3] (+ opacities) -> records[B,N,GOL_SPLAT_RECORD]: the rasterizer's packed per-Gaussian records
 *   (see gol_rasterize_fwd) with the depth as the 4th channel -- the fused path never assembles them separately.
 * ---------------------------------------------------------------------------------------- */
int gol_project_fwd(int B, int N, const float* means3d, const float* scales, float glob_scale,
                    const float* quats, const float* viewmats, const float* intrins, int img_h,
                    int img_w, int block, float clip_thresh, float* cov3d, float* xys,
                    float* depths, int32_t* radii, float* conics, float* compensation,
                    int32_t* num_tiles_hit, const float* opacities, float* opac_eff, const float* colors,
                    float* records, void* stream);
/* v_* inputs may be NULL (treated as zero).  If opacities != NULL the op also differentiates
 * opac_eff = opacity*compensation: v_opac_eff[B,N] in, v_opacity[B,N] out.
 * grad_stride = 0: v_xy[B,N,2], v_depth[B,N], v_conic[B,N,3], v_opac_eff[B,N] are dense arrays;
 * grad_stride = s > 0: they are fields of per-Gaussian records of s floats (element e at pointer + e*s), e.g. the
 * GOL_GRAD_RECORD-float records gol_rasterize_bwd accumulates into. */
int gol_project_bwd(int B, int N, const float* means3d, const float* scales, float glob_scale,
                    const float* quats, const float* viewmats, const float* intrins,
                    const float* cov3d, const int32_t* radii, const float* conics,
                    const float* compensation, const float* v_xy, const float* v_depth,
                    const float* v_conic, const float* v_compensation, const float* opacities,
                    const float* v_opac_eff, int grad_stride, float* v_mean3d, float* v_scale, float* v_quat,
                    float* v_opacity, void* stream);
/* The same with its upstream gradients taken from the rasterizer's per-Gaussian gradient records (grad_records
 * [B,N,GOL_GRAD_RECORD]: rgb | opacity | xy | conic a b c | depth | pad, gol_rasterize_bwd) and cov3d recomputed; v_colors
 * [B,N,3] (may be NULL) additionally receives the records' colour gradient as a dense array -- the consumer (the shading
 * tail's backward) then reads 12 contiguous bytes per Gaussian instead of a strided view of the records. */
int gol_project_bwd_records(int B, int N, const float* means3d, const float* scales, float glob_scale,
                            const float* quats, const float* viewmats, const float* intrins, const int32_t* radii,
                            const float* conics, const float* compensation, const float* opacities,
                            const float* grad_records, int with_depth, float* v_mean3d, float* v_scale, float* v_quat,
                            float* v_opacity, float* v_colors, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tile binning + per-tile depth sort.  Replaces gsplat: cumsum + map_gaussian_to_intersects +
 * torch.sort(int64) + get_tile_bin_edges without the host sync on the
 * intersection count.  Order inside a tile: ascending (depth bits, gaussian id) -- a
 * deterministic instance of gsplat's unspecified tie order.
 *   conics[B,N,3], opacities[B,N]  optional (both or neither): when given, (Gaussian, tile) pairs
 *                   whose alpha >= 1/255 ellipse cannot reach the tile are not stored.  This is
 *                   output-preserving (the rasterizer would skip them at every pixel, A.3).
 *   capacity        max intersections stored per view
 *   tile_count[B,T] int32 scratch
 *   tile_bins[B,T,2] out: [start,end) into the view's segment of sorted_ids
 *   isect_keys[B,capacity] uint64 scratch
 *   sorted_ids[B,capacity] out: Gaussian ids, tile by tile, front to back
 *   n_isect[B] out: number of list slots the view needs (> capacity means overflow: the excess
 *                   intersections were dropped and the render is incomplete).  Without conics this is gsplat's exact
 *                   intersection count; with conics it is an upper bound (the tight tile boxes, ~1.2x the pruned
 *                   lists: the count pass reserves, the scatter pass tests) and a view's lists have slack between them
 *   reach_scratch   unused since round 3 (pass NULL; kept for ABI stability)
 * ---------------------------------------------------------------------------------------- */
int gol_bin_sort(int B, int N, const float* xys, const float* depths, const int32_t* radii,
                 const float* conics, const float* opacities, int img_h, int img_w, int block,
                 int64_t capacity, int32_t* tile_count, int32_t* tile_bins, uint64_t* isect_keys,
                 int32_t* sorted_ids, int32_t* n_isect, uint64_t* reach_scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tile rasterizer.  Replaces gsplat: rasterize_forward / rasterize_backward, 3-channel
 * specialisation (call sites render_gsplat.py:65-78, 91-104; semantics SURVEY.md A.3, A.4).
 * Gaussian attributes come as PACKED RECORDS records[B,N,GOL_SPLAT_RECORD] (64 bytes = one HBM sector per Gaussian):
 *   [0] x [1] y [2] a' [3] b' | [4] c' [5] opacity [6] r [7] g | [8] b [9] extra [10] tau [11] 1/a | [12] 1/c [13] exact [14-15] pad
 *   (a', b', c' = the conic scaled for the pixel loops, tau / 1/a / 1/c / exact = the per-Gaussian part of the
 *   alpha >= 1/255 reach test; goliath_amd/csrc/gol_common.h) written by gol_project_fwd (fused path) or by
 *   gol_splat_pack from xys[B,N,2], conics[B,N,3], colors[B,N,3] (NULL = 0: records for gol_rasterize_nd_*, which
 *   stage their colours separately), extra[B,N] (NULL = 0), opacities[B,N] (the
 *   gsplat-compatible operators): a list entry costs one aligned 64-byte fetch instead of up to five sectors of five arrays.
 * One launch composites the colour and, with with_extra != 0, the 4th channel "extra" of the records
 * (the depth pass of render_gsplat.py:91-104 fused into the colour pass; its background is 0).
 *   planar = 0: out_img / v_out_img are [B,H,W,3] (gsplat); planar = 1: [B,3,H,W] (what
 *   AutoEncoder.render stacks, rgca.py:139 -- saves the permute copy in the backward).
 *   background[3]; out_extra[B,H,W]; final_Ts[B,H,W]; final_idx[B,H,W] int32:
 *   planar = 0: index into the view's sorted_ids segment of the last contributing Gaussian, 0 if none (gsplat's);
 *   planar = 1: the index gol_rasterize_bwd starts the pixel's walk from -- an upper bound of the above that excludes
 *   the entry the pixel stopped at (stop index - 1; end of the tile's list for a pixel that never reached T <= 1e-4).
 * fwd optional fused epilogue of AutoEncoder.render (rgca.py:137,144-145), NULL = off: out_alpha[B,H,W] = 1 - final_T and
 *   out_extra_norm[B,H,W] = extra image / clamp(1 - final_T, norm_lo, 1)  (the reference divides depth by alpha.clamp(0.05, 1));
 *   with out_extra_norm given, out_extra (the un-normalised image) may be NULL -- one image write less.
 * bwd ACCUMULATES into v_xy[B,N,2] v_conic[B,N,3] v_colors[B,N,3] v_opacity[B,N]
 * (and v_extra[B,N]) which the caller zeroes; v_out_alpha / v_out_extra may be NULL.
 * grad_stride = 0: the five gradient outputs are dense arrays (gsplat's layout);
 * grad_stride = GOL_GRAD_RECORD: they are fields of ONE zeroed buffer rec[B,N,GOL_GRAD_RECORD] of 64-byte records
 *   [rgb 0-2 | opacity 3 | xy 4-5 | conic 6-8 | extra 9 | pad], i.e. v_colors = rec, v_opacity = rec+3, v_xy = rec+4,
 *   v_conic = rec+6, v_extra = rec+9 (checked): the float atomics of a Gaussian then hit one cache line and 16
 *   consecutive lanes issue them together -- the memory-side atomic units see 1/10 of the requests.
 * Optional fused masked L1 loss (rgb_l1, ca_code/loss/__init__.py:391-411), planar layout only: with l1_target[B,3,H,W]
 *   (l1_mask[B,l1_mask_c,H,W], l1_mask_c = 1 or 3, or NULL) the forward also writes l1_sign[B,H,W], ONE BYTE per pixel
 *   holding sign((rgb_c - target_c) * mask_c) + 1 of channel c in bits 2c..2c+1, and l1_partial[B, tiles] = per-tile sums
 *   of |(rgb - target) * mask| (tiles = ceil(W/16) * ceil(H/16); loss = sum(l1_partial) / (B*3*H*W)).
 *   l1_out (NULL = the caller adds l1_partial up): l1_out[0] = l1_scale * sum(l1_partial), by a one-workgroup kernel
 *   enqueued behind the raster launch (fixed summation order: deterministic).
 *   The backward's upstream image gradient is  v_out_img (NULL = 0)  +  (code_c - 1) * mask_c * v_img_scale[0]  of
 *   v_sign[B,H,W] (NULL = none; v_sign_mask[B,v_sign_mask_c,H,W] or NULL = 1; v_img_scale device scalar, NULL = 1, times the
 *   host scalar v_img_scale_mul), so passing v_sign = l1_sign, v_sign_mask = l1_mask, v_img_scale = d loss_total / d l1
 *   (the autograd gradient of the loss value, as it is) and v_img_scale_mul = 1 / (B*3*H*W) back-propagates the
 *   loss without the two extra passes over the image a separate loss kernel needs; at least one of v_out_img / v_sign.
 * pixels_per_lane (fwd and bwd): the wave footprint.  2 = two waves per 16x16 tile, 16x8 pixels each, two pixels per lane
 *   (fewest instructions per pixel: launches that fill the chip); 1 = four waves per tile, 8x8 pixels each (~9-17 % more
 *   instructions, but a tile's work is spread over more SIMDs: launches of one or two views, whose workgroups are all
 *   resident at once and which last until the most loaded SIMD is done);
 *   0 = the forward chooses by B (gol_raster_plan), the backward takes 2.  Same images, final_T / final_idx and gradients
 *   either way (a footprint only skips entries none of its pixels can take), up to the summation order of the gradient atomics.
 *   In the fused path (planar = 1) final_idx / l1_sign of pixels in tiles WITHOUT list entries are not written (the
 *   backward never reads them; final_T = 1 is).
 * stage_mask[B,capacity] (NULL = off), one byte per list entry at the index of its sorted_ids entry: the forward stores the
 *   wave mask it staged the entry with (bit w = the entry's alpha >= 1/255 region reaches the footprint of wave w; every
 *   entry up to a tile's largest final_idx is written, a tile without entries writes nothing; a forward that runs with one
 *   pixel per lane writes nothing at all).  The backward of the SAME
 *   lists and records takes the buffer back with stage_mask_ppl = the pixels_per_lane that forward ran with (gol_raster_plan
 *   for 0) and then skips its own reach test per entry -- the same bits, computed once; unless both ran with two pixels per lane, or if
 *   stage_mask is NULL, it computes the masks itself.  GOL_RASTER_STAGE_MASK=0 in the
 *   environment (set for the whole render, read per call) turns both sides off.
 * ---------------------------------------------------------------------------------------- */
#define GOL_GRAD_RECORD 16
#define GOL_SPLAT_RECORD 16
int gol_splat_pack(int B, int N, const float* xys, const float* conics, const float* colors, const float* extra,
                   const float* opacities, float* records, void* stream);
int gol_rasterize_fwd(int B, int N, int img_h, int img_w, int block, int planar, const int32_t* tile_bins,
                      const int32_t* sorted_ids, int64_t capacity, const float* records, int with_extra,
                      const float* background, float* out_img,
                      float* out_extra, float* final_Ts, int32_t* final_idx, float* out_alpha,
                      float* out_extra_norm, float norm_lo, const float* l1_target, const float* l1_mask, int l1_mask_c,
                      uint8_t* l1_sign, float* l1_partial, float* l1_out, float l1_scale, uint8_t* stage_mask,
                      int pixels_per_lane, void* stream);
int gol_rasterize_bwd(int B, int N, int img_h, int img_w, int block, int planar, const int32_t* tile_bins,
                      const int32_t* sorted_ids, int64_t capacity, const float* records, int with_extra,
                      const float* background, const float* final_Ts,
                      const int32_t* final_idx, const float* v_out_img, const float* v_out_extra,
                      const float* v_out_alpha, float* v_xy, float* v_conic, float* v_colors,
                      float* v_extra, float* v_opacity, int grad_stride, const uint8_t* v_sign, const float* v_sign_mask,
                      int v_sign_mask_c, const float* v_img_scale, float v_img_scale_mul, const uint8_t* stage_mask,
                      int stage_mask_ppl, int pixels_per_lane, void* stream);
/* Diagnostic (bench.py's algorithmic roofline of the raster kernels): counts[B,2] (uint64) = per view the number of
 * (pixel, list entry) pairs up to the pixel's final_idx ("tested") and of those with alpha >= 1/255 ("taken" = composited),
 * from the state a planar gol_rasterize_fwd left (tile_bins, sorted_ids, records, final_idx). */
int gol_raster_count_pairs(int B, int N, int img_h, int img_w, const int32_t* tile_bins, const int32_t* sorted_ids,
                           int64_t capacity, const float* records, const int32_t* final_idx, uint64_t* counts, void* stream);
/* What pixels_per_lane = 0 means for the forward of a launch of B views (1 for B <= 2, else 2). */
int gol_raster_plan(int B, int* fwd_pixels_per_lane);

/* ------------------------------------------------------------------------------------------
 * N-channel tile rasterizer.  Replaces gsplat: nd_rasterize_forward / nd_rasterize_backward (what rasterize_gaussians
 * runs for colors[N, C], C != 3; semantics SURVEY.md A.3, A.4 -- the same alpha caps, cuts and stopping rule as
 * gol_rasterize_fwd / _bwd, which it equals channel by channel for C = 3).  gsplat's layouts, any C >= 1:
 *   records[B,N,GOL_SPLAT_RECORD] as for gol_rasterize_fwd (only the geometry is read: gol_splat_pack with colors = NULL
 *   fills them); colors[B,N,C] dense, interleaved; background[C]; out_img / v_out_img [B,H,W,C]; final_Ts[B,H,W];
 *   final_idx[B,H,W] int32 = gsplat's (index into the view's sorted_ids segment of the last contributing Gaussian,
 *   0 if none); tile_bins / sorted_ids / capacity from gol_bin_sort.  H * W * C * 4 bytes per view must stay < 4 GiB.
 * fwd OVERWRITES out_img, final_Ts, final_idx.  pixels_per_lane as for gol_rasterize_fwd (0 = gol_raster_plan(B)).
 * bwd ACCUMULATES into v_xy[B,N,2] v_conic[B,N,3] v_colors[B,N,C] v_opacity[B,N] (dense arrays; the caller zeroes them);
 *   v_out_img is required, v_out_alpha[B,H,W] may be NULL (= 0).
 * Channels are processed in chunks of at most 16; C > 16 walks each tile list once per chunk.
 * ---------------------------------------------------------------------------------------- */
int gol_rasterize_nd_fwd(int B, int N, int C, int img_h, int img_w, int block, const int32_t* tile_bins,
                         const int32_t* sorted_ids, int64_t capacity, const float* records, const float* colors,
                         const float* background, float* out_img, float* final_Ts, int32_t* final_idx,
                         int pixels_per_lane, void* stream);
int gol_rasterize_nd_bwd(int B, int N, int C, int img_h, int img_w, int block, const int32_t* tile_bins,
                         const int32_t* sorted_ids, int64_t capacity, const float* records, const float* colors,
                         const float* background, const float* final_Ts, const int32_t* final_idx,
                         const float* v_out_img, const float* v_out_alpha, float* v_xy, float* v_conic,
                         float* v_colors, float* v_opacity, void* stream);

/* ------------------------------------------------------------------------------------------
 * One render direction of a batch of views as ONE call (csrc/render.hip): what AutoEncoder.render issues per view from
 * Python -- project_gaussians -> rasterize_gaussians(colour) -> rasterize_gaussians(depth), ca_code/utils/render_gsplat.py:49-104,
 * in the view loop of ca_code/models/rgca.py:112-151 -- becomes gol_render_fwd = gol_project_fwd (+ packed records) +
 * gol_bin_sort + gol_rasterize_fwd (planar images, fused alpha / depth-normalisation / optional L1 epilogue) and
 * gol_render_bwd = gol_rasterize_bwd (64-byte gradient records, zeroed here) + gol_project_bwd, enqueued on `stream` out
 * of ONE caller-provided workspace.  gol_render_layout fills the byte offsets of the workspace's sub-buffers
 * (all 256-byte aligned; `total` = bytes to allocate) -- the caller reads n_isect[B] (int32, overflow check as for
 * gol_bin_sort), radii[B,N], final_T / final_idx[B,H,W], sorted_ids[B,capacity], tile_bins[B,T,2] there; stage_mask[B,capacity]
 * (bytes) carries the raster forward's wave masks to gol_render_bwd.
 * The forward leaves everything the backward needs in the workspace: keep it (and the inputs) until gol_render_bwd.
 *   out_img[B,3,H,W]; out_alpha[B,H,W] = 1 - final_T; with_depth: out_depth_norm[B,H,W] = depth / clamp(alpha, norm_lo, 1)
 *   and optionally out_depth[B,H,W] (NULL = skip); l1_target / l1_mask / l1_partial[B,T] / l1_out (NULL = partial sums
 *   only) / l1_scale as for gol_rasterize_fwd.
 *   bwd: v_img[B,3,H,W] / v_depth[B,H,W] (w.r.t. the UN-normalised depth image) / v_alpha[B,H,W] may be NULL;
 *   use_l1_sign != 0 adds the fused L1's gradient (v_img_scale = device scalar d loss / d l1, v_img_scale_mul = 1 / (B*3*H*W));
 *   grad_records[B,N,GOL_GRAD_RECORD] scratch; v_colors[B,N,3] (may be NULL): d loss / d colour as a dense array (it is
 *   also the first three floats of every record).
 * ---------------------------------------------------------------------------------------- */
typedef struct gol_render_ws {
  int64_t cov3d, xys, depths, radii, conics, comp, nth, opac_eff, records, tile_count, tile_bins, keys, sorted_ids,
      n_isect, final_T, final_idx, l1_sign, stage_mask, total;
} gol_render_ws;
int gol_render_layout(int B, int N, int img_h, int img_w, int64_t capacity, int with_l1, gol_render_ws* layout);
int gol_render_fwd(int B, int N, int img_h, int img_w, float glob_scale, float clip_thresh, const float* means,
                   const float* scales, const float* quats, const float* opacity, const float* colors,
                   const float* viewmats, const float* intrins, const float* background, int with_depth, float norm_lo,
                   int64_t capacity, void* workspace, const gol_render_ws* layout, float* out_img, float* out_depth,
                   float* out_alpha, float* out_depth_norm, const float* l1_target, const float* l1_mask, int l1_mask_c,
                   float* l1_partial, float* l1_out, float l1_scale, void* stream);
int gol_render_bwd(int B, int N, int img_h, int img_w, float glob_scale, const float* means, const float* scales,
                   const float* quats, const float* opacity, const float* viewmats, const float* intrins,
                   const float* background, int64_t capacity, void* workspace, const gol_render_ws* layout,
                   const float* v_img, const float* v_depth, const float* v_alpha, int use_l1_sign, const float* l1_mask,
                   int l1_mask_c, const float* v_img_scale, float v_img_scale_mul, float* grad_records, float* v_mean,
                   float* v_scale, float* v_quat, float* v_opacity, float* v_colors, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused RGCA shading tail.  Replaces the chain of ATen kernels in PrimDecoder.forward after the
 * two transposed-conv decoders (ca_code/models/rgca.py:505-588, training extra :590-618), incl.
 * the specular term: point lights = evaluate_gaussian w_type 0 (extensions/sgutils/sg.cu:27-175,
 * rgca.py:559-570) or environment = dir2uv + mipmap_grid_sample (ca_code/utils/envmap.py:284-292,
 * ca_code/utils/mipmap_sampler.py:13-69, rgca.py:548-556).
 * The decoder outputs are read ONCE in their native planar NCHW layout (coalesced per channel
 * plane): no permute().view() copies of the 125-channel tensor.
 * All pointers device memory; structs themselves are host memory, read before the call returns.
 * ---------------------------------------------------------------------------------------- */
#define GOL_MAX_MIPS 8
typedef struct {
  int32_t B, N;              /* views, Gaussians per view (N = S*S)                              */
  int32_t n_color_coef;      /* SH coefficients carried per colour channel: (n_color_sh+1)^2 = 16 */
  int32_t n_mono_coef;       /* monochrome SH coefficients: (n_diff_sh+1)^2 - n_color_coef = 65   */
  const float* f_vnocond;    /* [B, 3*n_color_coef + n_mono_coef + 12, N]  (rgca.py:494-495)      */
  const float* f_vcond;      /* [B, 4, N]                                   (rgca.py:498-503)      */
  const float* postex;       /* [B, 3, N] uv position map                   (rgca.py:483-484)      */
  const float* tn;           /* [B, 3, N] normalised uv normal map          (rgca.py:488-491)      */
  const float* albedo;       /* [N, 3]                                      (rgca.py:462-464)      */
  const float* light_sh;     /* [B, 3, n_color_coef + n_mono_coef]          (rgca.py:187-191)      */
  const float* light_sh_rand;/* same shape or NULL: training-only random light (rgca.py:590-616)  */
  const float* campos;       /* [B, 3] head-relative camera position                              */
  /* specular, point lights (used when n_mips == 0) */
  int32_t L;
  const float* light_intensity; /* [B, L, 3] */
  const float* light_pos;       /* [B, L, 3] */
  const int32_t* n_lights;      /* [B]       */
  /* specular, prefiltered environment (n_mips > 0) */
  int32_t n_mips;
  const float* mips[GOL_MAX_MIPS];  /* level i: [B, 3, mip_h[i], mip_w[i]] */
  int32_t mip_h[GOL_MAX_MIPS], mip_w[GOL_MAX_MIPS];
  const float* lightrot;        /* [B, 3, 3] ROTATIONS (orthonormal rows): the lookup direction lightrot x reflect(view, normal)
                                 * must be a unit vector -- the polar angle is formed as atan2(|r_xz|, r_y) and its derivative as
                                 * -1 / |r_xz|, which equal the reference's acos(r_y) (envmap.py:289) and its derivative only
                                 * for |r| = 1; the host side checks it (shade.py) */
  /* optional: the same levels repacked by gol_envmap_pack to [B, h, w, 16] footprint records (a bilinear lookup = one
   * aligned 64-byte fetch); all levels or none (NULL) */
  const float* mips_packed[GOL_MAX_MIPS];
  float primscale_min, primscale_max; /* rgca.py:47 (0.1, 20) */
  /* 1: ONE pyramid lights all B views -- every level is [1,3,h,w] (packed: [1,h,w,16]) and only `lightrot` differs per
   * view.  This is what the reference's relight driver feeds: EnvSpinDecorator.mipmap() expands one registered pyramid over
   * the batch (ca_code/utils/light_decorator.py:96-100) and rotates the lookup, not the map (:112-118, rgca.py:548-550).
   * 0: one pyramid per view, levels [B,...] as above. */
  int32_t mips_shared;
  /* every env-map sample (value and its u / v derivatives) is multiplied by this; 0 is read as 1.  The relight driver scales
   * the registered pyramid by 2 pi norm_scale[0] per FRAME (light_decorator.py:147-149): with the factor here the unscaled
   * pyramid is packed once per environment and nothing is re-packed when the spin index changes. */
  float mips_scale;
  /* NULL (the default): the host float above.  Otherwise one float in device memory, read by the kernels in place of
   * mips_scale (which is then ignored; the value is used as it is, 0 included): the relight driver's 2 pi norm_scale[0]
   * (light_decorator.py:151-153) as gol_envspin_frame leaves it, so that no host code waits for the frame's scale.  All four
   * entries (forward, backward, both *_project_*) read it. */
  const float* mips_scale_dev;
} gol_shade_in;

typedef struct {  /* every field [B,N,k] row-major like the reference's preds (rgca.py:574-588) */
  float* color;            /* 3 */
  float* opacity;          /* 1 */
  float* primpos;          /* 3 */
  float* primqvec;         /* 4 */
  float* primscale;        /* 3 clamped */
  float* primscale_preclip;/* 3 */
  float* sigma;            /* 1 */
  float* spec_vis;         /* 1 */
  float* spec_nml;         /* 3 */
  float* spec_dnml;        /* 3 */
  float* diff_color;       /* 3 */
  float* spec_color;       /* 3 */
  float* primnmlbase;      /* 3 */
  float* color_rand;       /* 3, or NULL when light_sh_rand == NULL */
  float* diff_sum;         /* 3: sum_k sh_k * L_k before albedo (saved for the backward) */
  float* env_saved;        /* 9, optional (NULL = off), env mode only: the env-map sample (value rgb, d/du rgb, d/dv rgb)
                              saved so the backward does not repeat the 8 texel gathers per Gaussian */
} gol_shade_out;

typedef struct {  /* upstream gradients, same shapes as gol_shade_out; any may be NULL (= 0) */
  const float *color, *opacity, *primpos, *primqvec, *primscale, *primscale_preclip, *sigma, *spec_vis,
      *spec_nml, *spec_dnml, *diff_color, *spec_color, *primnmlbase, *color_rand;
} gol_shade_out_grad;

typedef struct {  /* written in full */
  float* f_vnocond;        /* [B, C, N] */
  float* f_vcond;          /* [B, 4, N] */
  float* postex;           /* [B, 3, N] */
  float* tn;               /* [B, 3, N] */
  float* albedo_per_view;  /* [B, N, 3]  (sum over B = gradient of the shared albedo) */
  float* albedo;           /* [N, 3] or NULL: that sum, written by a second small kernel of the same call */
} gol_shade_in_grad;

/* src[B,3,h,w] (the layout of EnvSpinDecorator's mip pyramid, light_decorator.py:100-140) ->
 * dst[B,h,w,16]: record (y, x) = the four taps (y,x) (y,x+1) (y+1,x) (y+1,x+1) of the bilinear footprint whose top-left
 * texel it is, each as (r, g, b, 0), taps beyond the border zero -- 64 bytes, one HBM sector per lookup (4x the memory
 * of the map; packed once per environment, the host side caches it). */
int gol_envmap_pack(int B, int h, int w, const float* src, float* dst, void* stream);
int gol_shade_fwd(const gol_shade_in* in, const gol_shade_out* out, void* stream);
/* `saved` = the gol_shade_out of the forward (reads color_rand, diff_sum, env_saved). */
int gol_shade_bwd(const gol_shade_in* in, const gol_shade_out* saved, const gol_shade_out_grad* g,
                  const gol_shade_in_grad* gin, void* stream);

/* Shading WITH the projection fused in (north_star: "streaming stages fused"; rgca.py:505-588 -> render_gsplat.py:49-63).
 * The cameras of the B views are known before the decoder runs (AutoEncoder.forward builds headrel_Rt first,
 * rgca.py:175-195), so the shading kernel projects the Gaussians it has just produced while their position, quaternion,
 * clamped scale, opacity and colour are still in registers, and writes what binning and the rasterizer read; the render
 * direction then starts at the tile count (gol_render_fwd_projected) and ends at the gradient records
 * (gol_render_bwd_projected), which gol_shade_project_bwd pushes through the projection's vjp in its own prologue.
 * gol_project_fwd / gol_project_bwd stay for the gsplat-compatible operators and for Gaussians that do not come out of
 * the shading tail.  Same arithmetic (csrc/gol_project.h) either way. */
typedef struct {
  const float* viewmats;     /* [B,12] world -> camera, row-major 3x4                                   */
  const float* intrins;      /* [B,4]  fx, fy, cx, cy                                                   */
  int32_t img_h, img_w;
  float glob_scale, clip_thresh;
  /* written by gol_shade_project_fwd, read by binning / raster / gol_shade_project_bwd: shapes of gol_project_fwd's outputs */
  float* xys;                /* [B,N,2] */
  float* depths;             /* [B,N]   */
  int32_t* radii;            /* [B,N]   */
  float* conics;             /* [B,N,3] */
  float* comp;               /* [B,N]   */
  float* opac_eff;           /* [B,N]   opacity x compensation (render_gsplat.py:72)                    */
  float* records;            /* [B,N,GOL_SPLAT_RECORD] the rasterizer's packed records (colour + depth) */
} gol_shade_proj;
int gol_shade_project_fwd(const gol_shade_in* in, const gol_shade_out* out, const gol_shade_proj* proj, void* stream);
/* The render direction of Gaussians gol_shade_project_fwd has projected: gol_render_fwd minus its first kernel,
 * gol_render_bwd minus its last (the workspace then holds only tile lists and per-pixel state:
 * gol_render_layout_projected; the layout's xys ... records offsets are -1). */
int gol_render_layout_projected(int B, int N, int img_h, int img_w, int64_t capacity, int with_l1, gol_render_ws* layout);
int gol_render_fwd_projected(int B, int N, const gol_shade_proj* proj, const float* background, int with_depth,
                             float norm_lo, int64_t capacity, void* workspace, const gol_render_ws* layout,
                             float* out_img, float* out_depth, float* out_alpha, float* out_depth_norm,
                             const float* l1_target, const float* l1_mask, int l1_mask_c, float* l1_partial, float* l1_out,
                             float l1_scale, void* stream);
int gol_render_bwd_projected(int B, int N, const gol_shade_proj* proj, const float* background, int64_t capacity,
                             void* workspace, const gol_render_ws* layout, const float* v_img, const float* v_depth,
                             const float* v_alpha, int use_l1_sign, const float* l1_mask, int l1_mask_c,
                             const float* v_img_scale, float v_img_scale_mul, float* grad_records, void* stream);
/* grad_records[B,N,GOL_GRAD_RECORD] = the output of gol_render_bwd_projected; its colour / opacity / position /
 * quaternion / scale gradients are ADDED to the matching fields of `g` (other consumers of those outputs). */
int gol_shade_project_bwd(const gol_shade_in* in, const gol_shade_out* saved, const gol_shade_out_grad* g,
                          const gol_shade_proj* proj, const float* grad_records, int with_depth,
                          const gol_shade_in_grad* gin, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mixture-of-Volumetric-Primitives ray marcher + its helpers (BASELINE config 5).
 * Replaces utilslib.compute_raydirs_forward (extensions/utils/utils.cpp:46-82, kernel
 * utils_kernel.cu:11-51) and mvpraymarchlib.compute_aabb / raymarch_forward / raymarch_backward
 * (extensions/mvpraymarch/mvpraymarch.cpp:145-400; kernels mvpraymarch_subset_kernel.h:7-228,
 * bvh.cu:157-201) for the configuration every model in the reference uses: algo 0 (no warp field),
 * fixed-order BVH (implicit heap, children 2i+1 / 2i+2), channels-last template, additive
 * accumulation.  Unlike the reference (stream 0, no device guard) everything runs on `stream`.
 *   raypos/raydir[N,H,W,3] tminmax[N,H,W,2] primpos[N,K,3] primrot[N,K,3,3] primscale[N,K,3]
 *   tplate[N,K,TD,TH,TW,4] nodeaabb[N,2K-1,2,3]
 * march_fwd writes rayrgba[N,H,W,4] (every element) and, when non-NULL, raysat[N,H,W,3]; when
 * shadow[N,K,TD,TH,TW,2] is non-NULL it is ACCUMULATED into (primsplatter.h:29-36).
 * march_bwd ACCUMULATES into grad_primpos/rot/scale and grad_tplate (caller zeroes them,
 * mvpraymarch.py:258-264).
 * ---------------------------------------------------------------------------------------- */
int gol_raydirs_fwd(int N, int H, int W, const float* viewpos, const float* viewrot, const float* focal,
                    const float* princpt, const float* pixelcoords /* NULL = (w,h) grid */, float volradius,
                    float* raypos, float* raydir, float* tminmax, void* stream);
int gol_mvp_aabb(int N, int K, const float* primpos, const float* primrot, const float* primscale,
                 float* nodeaabb, void* stream);
int gol_mvp_march_fwd(int N, int H, int W, int K, const float* raypos, const float* raydir, float stepsize,
                      const float* tminmax, const float* nodeaabb, const float* primpos,
                      const float* primrot, const float* primscale, const float* tplate, int TD, int TH,
                      int TW, float fadescale, float fadeexp, float* rayrgba, float* raysat, float* shadow,
                      void* stream);
int gol_mvp_march_bwd(int N, int H, int W, int K, const float* raypos, const float* raydir, float stepsize,
                      const float* tminmax, const float* nodeaabb, const float* primpos,
                      const float* primrot, const float* primscale, const float* tplate, int TD, int TH,
                      int TW, float fadescale, float fadeexp, const float* raysat, const float* grad_rayrgba,
                      float* grad_primpos, float* grad_primrot, float* grad_primscale, float* grad_tplate,
                      void* stream);

/* algo 1 of the reference operator (mvpraymarch_kernel.cu:92-97, PrimSamplerTW<true>, primsampler.h:53-61, 83-87): every
 * box carries a warp field warp[N,K,WD,WH,WW,3] (channels-last, the layout raymarch_forward receives with chlast = true,
 * mvpraymarch.py:686); a sample at box position y0 reads its template at y1 = trilinear(warp_k, y0) -- y1 may leave the
 * box: missing corners read 0 -- while the fade term stays a function of y0.  Backward: additionally grad_warp
 * [N,K,WD,WH,WW,3] (ACCUMULATED, caller zeroes) and d y1 / d y0 in the chain to the box transform.  The gradient chain is
 * the one of the reference's own PyTorch fixture (mvpraymarch.py:603-626, pinned by tests/golden/mvp_golden.npz set "w");
 * the CUDA sampler hands the already warped position to its backward (primsampler.h:64 overwrites y0, :71-86 use it),
 * which differs from that fixture as soon as the warp is not the identity.  No model of the reference emits a warp. */
int gol_mvp_march_warp_fwd(int N, int H, int W, int K, const float* raypos, const float* raydir, float stepsize,
                           const float* tminmax, const float* nodeaabb, const float* primpos,
                           const float* primrot, const float* primscale, const float* tplate, int TD, int TH,
                           int TW, const float* warp, int WD, int WH, int WW, float fadescale, float fadeexp,
                           float* rayrgba, float* raysat, float* shadow, void* stream);
int gol_mvp_march_warp_bwd(int N, int H, int W, int K, const float* raypos, const float* raydir, float stepsize,
                           const float* tminmax, const float* nodeaabb, const float* primpos,
                           const float* primrot, const float* primscale, const float* tplate, int TD, int TH,
                           int TW, const float* warp, int WD, int WH, int WW, float fadescale, float fadeexp,
                           const float* raysat, const float* grad_rayrgba, float* grad_primpos, float* grad_primrot,
                           float* grad_primscale, float* grad_tplate, float* grad_warp, void* stream);

/* Light-batched shadow march of the teacher model (ca_code/models/hand_teacher_mvp.py:271-358, no_grad): N = B*L ray
 * images (L = `group` lights per frame, consecutive), but the primitive transforms, the AABB tree and the template exist
 * once per FRAME: primpos/primrot/primscale [B,K,.], nodeaabb [B,2K-1,2,3], tplate [B,K,TD,TH,TW,4] -- or, with
 * alpha_only, [B,K,TD,TH,TW] (the reference fills the colour channels with the constant 255 and never looks at the
 * marched colour).  The reference materialises L copies of all of them (expand().reshape(), :273-349).
 * shadow [N,K,TD,TH,TW,2] is ACCUMULATED (caller zeroes), exactly like raymarch_forward's `shadow` argument;
 * rayrgba [N,H,W,4] may be NULL. */
int gol_mvp_shadow_march(int N, int group, int H, int W, int K, const float* raypos, const float* raydir,
                         float stepsize, const float* tminmax, const float* nodeaabb, const float* primpos,
                         const float* primrot, const float* primscale, const float* tplate, int alpha_only,
                         int TD, int TH, int TW, float fadescale, float fadeexp, float* rayrgba, float* shadow,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * URHand per-texel-per-light UV feature loops (BASELINE config 4).  Replace the broadcast PyTorch
 * expressions of ConvTeacherDecoder.forward: ca_code/models/urhand.py:419-445 (Lambert + Phong^p
 * features) and :508-567 (GGX/Schlick features + physically based texture).  All images planar:
 *   p_uv[B,3,HW] nml[B,3,HW] cam_pos[B,3] light_pos[B,L,3] light_intensity[B,L]
 *   shadow_map[B,L,HW] or NULL; GGX only: roughness[B,HW] tex_mean[B,3,HW] (0..255), fresnel
 *   pow[n_pow] = spec_powers (urhand.py:277: 1, 16, 32)
 *                domain: every pow[k] >= 1 (s^p = exp2(p log2 s) is NaN at p = 0, s = 0)
 * phong: diff[B,HW] = diff_feature_raw, spec[B,n_pow,HW] = spec_feature_raw.
 * ggx:   feat[B,1+n_pow,HW] = feat_p (urhand.py:558), rgb[B,3,HW] = phys_tex before the global
 *        scale of :567.  Backward writes g_* in full (no accumulation); lights, camera and the
 *        shadow map receive no gradient (data / computed under no_grad in the reference).
 * ---------------------------------------------------------------------------------------- */
#define GOL_UV_MAX_POW 4
typedef struct {
  int32_t B, L, HW, n_pow;
  float pow[GOL_UV_MAX_POW];
  float fresnel;
  const float *p_uv, *nml, *cam_pos, *light_pos, *light_intensity, *shadow_map, *roughness, *tex_mean;
} gol_uvlight_in;
int gol_uvlight_phong_fwd(const gol_uvlight_in* in, float* diff, float* spec, void* stream);
int gol_uvlight_phong_bwd(const gol_uvlight_in* in, const float* u_diff, const float* u_spec, float* g_p_uv,
                          float* g_nml, void* stream);
int gol_uvlight_ggx_fwd(const gol_uvlight_in* in, float* feat, float* rgb, void* stream);
int gol_uvlight_ggx_bwd(const gol_uvlight_in* in, const float* u_feat, const float* u_rgb, float* g_p_uv,
                        float* g_nml, float* g_roughness, float* g_tex, void* stream);

/* ------------------------------------------------------------------------------------------
 * Masked L1 image loss ("next" row).  Replaces the ATen chain of rgb_l1
 * (ca_code/loss/__init__.py:391-411): ((pred - target) * mask).abs().mean().
 *   pred, target [B,C,HW]; mask NULL, [B,1,HW] (mask_c = 1) or [B,C,HW] (mask_c = C)
 * fwd writes partial[B*C*gol_l1_blocks(HW)] per-workgroup sums (loss = sum(partial)/(B*C*HW));
 * bwd writes g_pred = sign((pred-target)*mask) * mask * g_loss[0] / (B*C*HW)  (g_loss: device scalar).
 * ---------------------------------------------------------------------------------------- */
int gol_l1_blocks(int HW);
int gol_l1_fwd(int B, int C, int HW, int mask_c, const float* pred, const float* target, const float* mask,
               float* partial, void* stream);
int gol_l1_bwd(int B, int C, int HW, int mask_c, const float* pred, const float* target, const float* mask,
               const float* g_loss, float* g_pred, void* stream);

/* ------------------------------------------------------------------------------------------
 * Light-contracted last decoder layer ("next" row).  Replaces
 *   ConvTranspose2dWNUB(16 -> C_out, 4, 2, 1)  (ca_code/models/rgca.py:427,455; ca_code/nn/layers.py:331-397)
 * followed by the SH contraction of rgca.py:506-514,528-530, for weights the host has already contracted
 * with the light (goliath_amd/tail.py):
 *   out[b,ch,oy,ox] = sum_{ci,ky,kx} x[b,ci,iy,ix] weff[b',ci,ch,ky,kx]   (oy = 2 iy - 1 + ky, b' = wB==1 ? 0 : b)
 *                     + (ch < E ? sum_k lc[k,b,ch] bias[k,oy,ox] : bias[nd + ch - E, oy, ox])
 *   x [B,16,h,w]; weff [wB,16,CH,4,4]; lc [nd,B,E] (E = 0|3|6 contracted channels, nd SH planes; plane-major so a plane's B*E
 *   coefficients are one contiguous scalar load);
 *   bias [nd + CH - E, 2h, 2w]; out [B,CH,2h,2w].
 * bwd (any of g_x / g_weff / g_bias may be NULL = not wanted):
 *   g_x [B,16,h,w] written; needs weff_t = weff permuted to [wB,CH,4,4,16];
 *   g_weff [wB,16,CH,4,4] ACCUMULATES (caller zeroes), fp32 MFMA; needs x; w_scratch (optional, see below) avoids atomics;
 *   g_bias [nd + CH - E, 2h, 2w] written.
 * ---------------------------------------------------------------------------------------- */
int gol_tail_conv_fwd(int B, int Ci, int h, int w, int CH, int E, int nd, int wB, const float* x, const float* weff,
                      const float* lc, const float* bias, float* out, void* stream);
int gol_tail_conv_bwd(int B, int Ci, int h, int w, int CH, int E, int nd, int wB, const float* x, const float* weff_t,
                      const float* lc, const float* g_out, float* g_x, float* g_weff, float* g_bias, float* w_scratch,
                      void* stream);
/* floats of optional scratch for g_weff: with it the per-workgroup partial sums are written out and reduced by a second
 * kernel instead of being added with float atomics (NULL = atomics). */
long long gol_tail_conv_bwd_scratch_floats(int B, int h, int w, int CH);

/* ------------------------------------------------------------------------------------------
 * Hidden decoder layer as one operator (profiles/LOG.md open item 6).  Replaces
 *   ConvTranspose2dWNUB(Ci -> Co, 4, 2, 1) + LeakyReLU(leak)
 * (ca_code/nn/layers.py:331-397, weight norm layers.py:157-244, stacked at ca_code/models/rgca.py:408-426,429-454:
 * one MIOpen transposed convolution, an ATen add of the untied bias and an ATen leaky_relu per layer):
 *   y[b,co,Y,X] = lrelu( sum_{ci,ky,kx} x[b,ci,iy,ix] w_eff[ci,co,ky,kx] + bias[co,Y,X] ),  Y = 2 iy - 1 + ky, X = 2 ix - 1 + kx
 *   x [B,Ci,h,w]; w_eff [Ci,Co,4,4] (the weight norm already applied, goliath_amd/tail.py:wn_weight); bias [Co,2h,2w];
 *   y [B,Co,2h,2w]; leak > 0.  fp32 MFMA, exact fp32.  Nothing but y is written.
 * Ci must be a multiple of 8 and Co a multiple of 16, otherwise GOL_ERR_UNSUPPORTED; w_eff, w_eff_t, y, g_y and g_bias
 * must be 16-byte aligned.
 * bwd forms g_pre = g_y * (y > 0 ? 1 : leak) while loading (any of g_x / g_w / g_bias may be NULL = not wanted, at no cost):
 *   g_x [B,Ci,h,w] written; needs w_eff_t = w_eff permuted to [Co,4 (kx),Ci,4 (ky)];
 *   g_w [Ci,Co,4,4] written; needs x and scratch[gol_trunk_conv_bwd_scratch_floats] (per-workgroup partial sums added
 *       in a fixed order by a second kernel: no float atomics, bitwise reproducible);
 *   g_bias [Co,2h,2w] written (= sum_b g_pre).
 * ---------------------------------------------------------------------------------------- */
int gol_trunk_conv_fwd(int B, int Ci, int Co, int h, int w, float leak, const float* x, const float* w_eff,
                       const float* bias, float* y, void* stream);
long long gol_trunk_conv_bwd_scratch_floats(int B, int Ci, int Co, int h, int w);
int gol_trunk_conv_bwd(int B, int Ci, int Co, int h, int w, float leak, const float* x, const float* w_eff_t,
                       const float* y, const float* g_y, float* g_x, float* g_w, float* g_bias, float* scratch,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Encoder layer as one operator.  Replaces
 *   Conv2dWNUB(Ci -> Co, 4, 2, 1) + LeakyReLU(leak)
 * (ca_code/nn/layers.py:276-328,472, weight norm layers.py:157-244, stacked eight times at ca_code/models/rgca.py:281-298:
 * one MIOpen convolution, an ATen add of the untied bias and an ATen leaky_relu per layer), and for the first layer the
 * `color / 255.0 - 0.5` in front of the stack (rgca.py:314) as the affine (in_scale, in_shift) of the load:
 *   xin[b,ci,r,c]  = in_scale * x[b,ci,r,c] + in_shift   inside the image, 0 outside (the zero pad comes AFTER the affine)
 *   y[b,co,Y,X]    = lrelu( sum_{ci,ky,kx} xin[b,ci,2Y-1+ky,2X-1+kx] w_eff[co,ci,ky,kx] + bias[co,Y,X] )
 *   x [B,Ci,H,W], H and W even; w_eff [Co,Ci,4,4] (the weight norm already applied, goliath_amd/tail.py:wn_weight);
 *   bias [Co,H/2,W/2]; y [B,Co,H/2,W/2]; leak > 0.  fp32 MFMA, exact fp32.  Nothing but y is written.
 * Co must be a multiple of 16 and Ci a multiple of 8 or one of 1..4 (a K stage is then zero-padded on the weight side; no
 * channel of x that does not exist is read), H and W even: otherwise GOL_ERR_UNSUPPORTED.  w_eff, y, g_y and g_bias must
 * be 16-byte aligned.
 * bwd forms g_pre = g_y * (y > 0 ? 1 : leak) while loading (any of g_x / g_w / g_bias may be NULL = not wanted, at no cost):
 *   g_x [B,Ci,H,W] written: in_scale * sum_{co,ky,kx} g_pre[b,co,Y,X] w_eff[co,ci,ky,kx] over 2Y-1+ky = r, 2X-1+kx = c;
 *       needs w_eff in the forward's layout [Co,Ci,4,4] (no permuted copy);
 *   g_w [Co,Ci,4,4] written (= sum_{b,Y,X} g_pre xin); needs x and scratch[gol_enc_conv_bwd_scratch_floats] (per-workgroup
 *       partial sums added in a fixed order by a second kernel: no float atomics, bitwise reproducible);
 *   g_bias [Co,H/2,W/2] written (= sum_b g_pre).
 * ---------------------------------------------------------------------------------------- */
int gol_enc_conv_fwd(int B, int Ci, int Co, int H, int W, float leak, float in_scale, float in_shift, const float* x,
                     const float* w_eff, const float* bias, float* y, void* stream);
long long gol_enc_conv_bwd_scratch_floats(int B, int Ci, int Co, int H, int W);
int gol_enc_conv_bwd(int B, int Ci, int Co, int H, int W, float leak, float in_scale, float in_shift, const float* x,
                     const float* w_eff, const float* y, const float* g_y, float* g_x, float* g_w, float* g_bias,
                     float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Texture-decoder layer of URHand as one operator: exact 2x bilinear resize (align_corners=True) + weight-normalised
 * 3x3 / stride 1 / pad 1 convolution + epilogue.  Replaces, per layer of the two texture branches of
 * ConvTeacherDecoder.forward (ca_code/models/urhand.py:583-608; layers built at :302-323 from la.Conv2dWNUB(.., 3, 1, 1)
 * and la.Conv2dWN(.., 3, 1, 1, bias=False), ca_code/nn/layers.py:276-328, weight norm layers.py:157-244),
 *   F.interpolate(x, (2 Hi, 2 Wi), mode="bilinear", align_corners=True), the MIOpen convolution and
 *   mode 0 (texmod0, urhand.py:592-597): the ATen add of the untied bias and leaky_relu,
 *   mode 1 (texmod1, urhand.py:600-606): the ATen multiply by the other branch's activation, add of gainbias, * 0.707107:
 *   U[b,ci,r,c]   = bilinear(x[b,ci]) at (r (Hi-1)/(H-1), c (Wi-1)/(W-1)), H = 2 Hi, W = 2 Wi, by the integer-ratio rule
 *                   r0 = (r (Hi-1)) div (H-1), frac = float((r (Hi-1)) mod (H-1)) / float(H-1), r1 = min(r0+1, Hi-1)
 *                   (same per column): pinned against float64, not against the library's fp32 `dst * scale`
 *   acc[b,co,r,c] = sum_{ci,ky,kx} Upad[b,ci,r-1+ky,c-1+kx] w_eff[co,ci,ky,kx]     (Upad = U inside the image, 0 outside)
 *   mode 0:  y = lrelu(acc + bias[co,r,c], leak), leak > 0
 *   mode 1:  y = (acc * gate[b,co,r,c] + gb[b,co,r,c]) * scale                      (gb may be NULL: no add)
 *   x [B,Ci,Hi,Wi]; w_eff [Co,Ci,3,3] (the weight norm already applied, goliath_amd/tail.py:wn_weight); bias [Co,H,W];
 *   gate, gb, y [B,Co,H,W].  fp32 MFMA, exact fp32.  U never exists in memory; nothing but y is written.
 * Ci must be a multiple of 8 and Co a multiple of 16 or one of 1..4 (zero weight rows), otherwise GOL_ERR_UNSUPPORTED.
 * bwd forms g_pre = g_y * (y > 0 ? 1 : leak) (mode 0; needs y) or scale * gate * g_y (mode 1; needs gate) while loading;
 * any of the outputs may be NULL = not wanted, at no cost:
 *   g_x [B,Ci,Hi,Wi] written: the bilinear adjoint of the transposed convolution of g_pre, gathered per source texel from
 *       a region of g_U kept on chip (no atomics); needs w_eff;
 *   g_w [Co,Ci,3,3] written (= sum_{b,r,c} g_pre Upad, U recomputed from x); needs x and
 *       scratch[gol_upconv_bwd_scratch_floats] (per-workgroup partial sums added in a fixed order by a second kernel: no
 *       float atomics, bitwise reproducible);
 *   mode 0: g_bias [Co,H,W] written (= sum_b g_pre);
 *   mode 1: g_gate [B,Co,H,W] = scale * g_y * acc (acc recomputed: needs x and w_eff) and g_gb [B,Co,H,W] = scale * g_y.
 * ---------------------------------------------------------------------------------------- */
int gol_upconv_fwd(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale, const float* x,
                   const float* w_eff, const float* bias, const float* gate, const float* gb, float* y, void* stream);
long long gol_upconv_bwd_scratch_floats(int B, int Ci, int Co, int Hi, int Wi);
int gol_upconv_bwd(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale, const float* x,
                   const float* w_eff, const float* y, const float* gate, const float* g_y, float* g_x, float* g_w,
                   float* g_bias, float* g_gate, float* g_gb, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Decoder level of URHand's DisplacementUNet as one operator: LeakyReLU of the previous layer's output + exact 2x
 * bilinear resize (align_corners=True) + concat with the encoder's skip + weight-normalised 3x3 / stride 1 / pad 1
 * convolution + untied bias (+ tanh and an affine at the last level).  Replaces, per level 1..n of the two decoder branches of
 * DisplacementUNet.forward (ca_code/models/urhand.py:217-226 and :231-239; layers built at :164-193 from
 * la.Conv2dWNUB(.., 3, 1, 1), ca_code/nn/layers.py:276-328),
 *   F.leaky_relu(x, 0.2), F.interpolate(x, size=x_prev.shape[2:4], mode="bilinear", align_corners=True),
 *   th.cat([x, x_prev], 1), the MIOpen convolution, the ATen add of the untied bias and, after the last level, tanh and
 *   x * output_scale (:227-228) or (x + 1) / 4 + 0.3 (:240-241):
 *   L             = xa > 0 ? xa : leak * xa          (the adjoint at xa == 0 takes leak, as torch)
 *   U             = bilinear 2x of L by the integer-ratio rule of gol_upconv_* above (H = 2 Hi, W = 2 Wi)
 *   X             = concat(U, xb) over channels: U is channels 0..Ca-1 of the weight, xb is channels Ca..Ca+Cb-1
 *   acc[b,co,r,c] = sum_{k,ky,kx} Xpad[b,k,r-1+ky,c-1+kx] w_eff[co,k,ky,kx]            (Xpad = X inside the image, 0 outside)
 *   act 0:  y = acc + bias[co,r,c]                   (the next level applies the leaky itself)
 *   act 1:  y = tanh(acc + bias[co,r,c]) * out_scale + out_shift
 *           (displacement: out_scale = output_scale, out_shift = 0; roughness: out_scale = 0.25, out_shift = 0.55)
 *   xa [B,Ca,Hi,Wi] (the previous layer's output BEFORE its activation); xb [B,Cb,H,W]; w_eff [Co,Ca+Cb,3,3] (the weight
 *   norm already applied, goliath_amd/tail.py:wn_weight); bias [Co,H,W]; y [B,Co,H,W].  fp32 MFMA, exact fp32.  L, U and X
 *   never exist in memory; nothing but y is written.
 * Ca and Cb must be positive multiples of 8 and Co a multiple of 8 or one of 1..4 (zero weight rows), B <= 65535, any
 * Hi, Wi >= 1; otherwise GOL_ERR_UNSUPPORTED.  A null pointer with positive sizes is GOL_ERR_INVALID_ARG; B == 0 is GOL_OK
 * without a launch.
 * bwd forms g_pre = g_y (act 0) or g_y * out_scale * (1 - t^2) with t = (y - out_shift) / out_scale recovered from y
 * (act 1; needs y) while loading; any of the outputs may be NULL = not wanted, at no cost:
 *   g_xa [B,Ca,Hi,Wi] written: the bilinear adjoint of the transposed convolution of g_pre over channels 0..Ca-1, gathered
 *       per source texel from a region of g_U kept on chip (no atomics), times the leaky mask of xa; needs xa and w_eff;
 *   g_xb [B,Cb,H,W] written: the transposed convolution of g_pre over channels Ca.. (mirrored taps, no flipped copy of
 *       the weight); needs w_eff;
 *   g_w [Co,Ca+Cb,3,3] written (= sum_{b,r,c} g_pre Xpad, U recomputed from xa); needs xa, xb and
 *       scratch[gol_upcat_conv_bwd_scratch_floats] (per-workgroup partial sums added in a fixed order by a second kernel:
 *       no float atomics, bitwise reproducible);
 *   g_bias [Co,H,W] written (= sum_b g_pre).
 * No host sync, no allocation: both calls can be captured as a linear graph.
 * ---------------------------------------------------------------------------------------- */
int gol_upcat_conv_fwd(int B, int Ca, int Cb, int Co, int Hi, int Wi, int act, float leak, float out_scale,
                       float out_shift, const float* xa, const float* xb, const float* w_eff, const float* bias, float* y,
                       void* stream);
long long gol_upcat_conv_bwd_scratch_floats(int B, int Ca, int Cb, int Co, int Hi, int Wi);
int gol_upcat_conv_bwd(int B, int Ca, int Cb, int Co, int Hi, int Wi, int act, float leak, float out_scale,
                       float out_shift, const float* xa, const float* xb, const float* w_eff, const float* y,
                       const float* g_y, float* g_xa, float* g_xb, float* g_w, float* g_bias, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Front of URHand's FeatEncoderUNet as one operator: the weight-normalised 7x7 / stride 1 / pad 3 projection and the
 * first 4x4 / stride 2 / pad 1 feature layer, both without bias and with nothing between them.  Replaces, in
 * FeatEncoderUNet.forward (ca_code/models/urhand.py:100-102; layers built at :91-93 from la.Conv2dWN(.., bias=False),
 * ca_code/nn/layers.py:470),
 *   x = self.proj(x); x = self.feat_mod[0](x)
 * two MIOpen convolutions and, backward, their weight-gradient convolutions and the input gradient of the second:
 *   h[b,m,r,c]  = sum_{cx,ky,kx} xpad[b,cx,r-3+ky,c-3+kx] w_p[m,cx,ky,kx]     0 <= r < H, 0 <= c < W; xpad = x inside the
 *                                                                               image, 0 outside
 *   y[b,co,Y,X] = sum_{m,ky,kx}  hpad[b,m,2Y-1+ky,2X-1+kx] w_f[co,m,ky,kx]    hpad = h inside the image and EXACTLY 0
 *                                                                               outside (not the 7x7 response of the
 *                                                                               zero-extended x at positions out there)
 *   x [B,Cx,H,W]; w_p [Cm,Cx,7,7] and w_f [Co,Cm,4,4] are EFFECTIVE weights (the weight norm already applied,
 *   goliath_amd/tail.py:wn_weight); y [B,Co,H/2,W/2].  fp32 MFMA (v_mfma_f32_16x16x4_f32) in both GEMMs, exact fp32.
 *   h never exists in memory: nothing but y is written.
 * bwd produces the two weight gradients only -- the operator has no input gradient (the model feeds it a detached
 * tensor, urhand.py:585); either output may be NULL = not wanted, at no cost, the other one bitwise unchanged:
 *   g_w_f [Co,Cm,4,4] written = sum_{b,Y,X} g_y[b,co,Y,X] hpad[b,m,2Y-1+ky,2X-1+kx], h recomputed from x; needs x, w_p;
 *   g_w_p [Cm,Cx,7,7] written = sum_{b,r,c} g_h[b,m,r,c] xpad[b,cx,r-3+ky,c-3+kx], g_h = the stride-2 transposed
 *       convolution of g_y with w_f restricted to the image, formed per tile on chip, never written; needs x, w_f.
 *   Both need scratch[gol_featenc_front_bwd_scratch_floats]: a workgroup owns a block of the weight and walks a run of
 *   tiles, its partial sum leaves once and a second kernel adds the partials in a fixed order (no float atomics, bitwise
 *   reproducible).  4 -> 64 -> 192 at 1024^2, B = 1: 9,961,472 floats = 38.0 MiB.
 * Supported: Cx in 1..8 (the K stage is zero-padded on the weight side: no channel of x that does not exist is read),
 * Cm % 16 == 0, Co % 16 == 0, H and W even and >= 2, B <= 65535: everything else returns GOL_ERR_UNSUPPORTED
 * (gol_featenc_front_bwd_scratch_floats: 0).  A null pointer with positive sizes returns GOL_ERR_INVALID_ARG; B == 0
 * returns GOL_OK without a launch (bwd: the outputs it is given are zeroed).  w_f must be 16-byte aligned.  No host sync,
 * no allocation: both calls can be captured as a linear graph.
 * ---------------------------------------------------------------------------------------- */
int gol_featenc_front_fwd(int B, int Cx, int Cm, int Co, int H, int W, const float* x, const float* w_p,
                          const float* w_f, float* y, void* stream);
long long gol_featenc_front_bwd_scratch_floats(int B, int Cx, int Cm, int Co, int H, int W);
int gol_featenc_front_bwd(int B, int Cx, int Cm, int Co, int H, int W, const float* x, const float* w_p,
                          const float* w_f, const float* g_y, float* g_w_p, float* g_w_f, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * gol_conv3_fwd / gol_conv3_bwd_x: a layer of the frozen VGG19 feature network of the masked perceptual loss
 * (ca_code/loss/vgg.py:17-88; `vgg`, ca_code/loss/perceptual.py:55-58) as one operator: 3x3 / stride 1 / zero padding 1
 * convolution + bias + ReLU, optionally on the normalised image and optionally followed by the 2x2 max-pool.  Replaces
 * the MIOpen convolution, the ATen bias add, relu, max_pool2d and the normalisation passes.  fp32 MFMA
 * (v_mfma_f32_16x16x4_f32), exact fp32.
 *   x [B,Ci,H,W]; weight [Co,Ci,3,3]; bias [Co]; y [B,Co,H,W], or with pool p [B,Co,H/2,W/2] and pos (bytes) of p's shape.
 *   acc[b,co,r,c] = sum_{ci,ky,kx} xpad[b,ci,r-1+ky,c-1+kx] weight[co,ci,ky,kx]         (xpad = x inside the image, 0 outside)
 *   y = relu(acc + bias[co])
 * image_in (Ci == 3): the operand is n = (clamp(x / 255.f, 0, 1) - mean_c) / std_c, formed while loading, with
 *   mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225) (vgg.py:62-65): IEEE division, that operation order, no
 *   contraction, so x = 255 gives exactly 1.  The zero padding is zero in NORMALISED space: a pixel outside the image
 *   contributes 0, not (0 - mean) / std.  K = 27 is padded to 28.
 * pool (2x2 max, stride 2, floor): only p and pos are written; y never exists.  pos is the window position of the maximum,
 *   0..3 row-major; the first maximum in that order wins a tie.  A last odd row or column feeds nothing.  Tiles have an
 *   even origin and an even size, so no window straddles workgroups.  H < 2 or W < 2 with pool: GOL_ERR_UNSUPPORTED.
 * gol_conv3_bwd_x: the input gradient only (the weights are frozen).  y = the forward's y, or p with pool (then g_y is g_p
 *   [B,Co,H/2,W/2] and pos the forward's bytes).  g_pre is formed while loading:
 *     without pool  g_pre = g_y where y > 0, else 0
 *     with pool     g_pre[r,c] = g_p[r/2,c/2] where pos names (r,c) and p > 0, else 0: a window whose maximum is 0 passes
 *                   nothing, a row or column dropped by the floor receives 0
 *   g_x [B,Ci,H,W] written = the transposed 3x3 convolution of g_pre, read from the same weight with mirrored taps (no
 *   flipped copy).  image_in: g_x is the gradient of the IMAGE, g_n / std_c / 255 where 0 <= x / 255 <= 1 (edges inclusive,
 *   as torch's clamp backward), else 0; needs x; Ci = 3 runs as a 16-row tile with zero weights.  Without image_in x may
 *   be NULL.  No atomics, no scratch: bitwise reproducible.
 * Supported: Ci == 3 with image_in, Ci % 8 == 0 without; Co % 16 == 0; any H, W >= 1; B <= 65535: everything else returns
 * GOL_ERR_UNSUPPORTED.  A null pointer with positive sizes returns GOL_ERR_INVALID_ARG; B == 0 returns GOL_OK without a
 * launch.  No host sync, no allocation: one launch each, capturable as a linear graph.
 * ---------------------------------------------------------------------------------------- */
int gol_conv3_fwd(int B, int Ci, int Co, int H, int W, int image_in, int pool, const float* x, const float* weight,
                  const float* bias, float* y, unsigned char* pos, void* stream);
int gol_conv3_bwd_x(int B, int Ci, int Co, int H, int W, int image_in, int pool, const float* x, const float* weight,
                    const float* y, const unsigned char* pos, const float* g_y, float* g_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * gol_conv3x_pack / gol_conv3x_fwd / gol_conv3x_bwd_x: the layer of gol_conv3_fwd / gol_conv3_bwd_x (without image_in) at
 * precision "bf16x3": a split-bf16 product on v_mfma_f32_16x16x32_bf16, for the wide layers of the network.
 *   split(v): hi = bf16_rne(v), lo = bf16_rne(v - float(hi))      (round to nearest even; the subtraction is exact in fp32)
 *   acc[b,co,r,c] = sum_{ci,ky,kx} (lo_x hi_w + hi_x lo_w + hi_x hi_w)    over xpad[b,ci,r-1+ky,c-1+kx], weight[co,ci,ky,kx]
 *   Products are exact, the sum is fp32, the lo lo term is dropped: |acc - exact| <= 3.1 2^-16 sum |x||w|, 4.5e-6 rel-L2
 *   measured against float64.  Inputs are finite and of ordinary magnitude: a subnormal lo is not handled (it may be
 *   flushed), inf / NaN are not defined.  Zero padding splits to (0, 0).
 * gol_conv3x_pack splits the weight ONCE into packed[gol_conv3x_packed_elems(Co, Ci)] (16-bit elements, 16-byte aligned):
 *   [hi | lo][tap][Co / 8][Ci / 8][8 co][8 ci].  The same buffer serves both directions: the forward reads a block's rows,
 *   the backward transposes the block on its way to LDS and mirrors the taps.  gol_conv3x_packed_elems returns 0 for an
 *   unsupported (Co, Ci).
 * gol_conv3x_fwd: x [B,Ci,H,W] is split while it is loaded; y = relu(acc + bias[co]) [B,Co,H,W], or with pool only
 *   p [B,Co,H/2,W/2] and pos (bytes): gol_conv3_fwd's semantics -- 2x2 max, stride 2, floor; pos = the window position of
 *   the maximum, 0..3 row-major, the first maximum in that order wins; a last odd row or column feeds nothing.
 * gol_conv3x_bwd_x: gol_conv3_bwd_x's: y = the forward's y, or p with pool (then g_y is g_p and pos the forward's bytes);
 *   g_pre = g_y where y > 0 (with pool: g_p where pos names the element and p > 0), else 0, formed while loading and THEN
 *   split; g_x [B,Ci,H,W] written = the transposed convolution of g_pre in the same three products.
 * Supported: Ci % 32 == 0, Co % 32 == 0, any H, W >= 1 (>= 2 with pool), B <= 65535: everything else returns
 * GOL_ERR_UNSUPPORTED (there is no image layer: Ci = 3 stays on gol_conv3_fwd).  A null pointer with positive sizes returns
 * GOL_ERR_INVALID_ARG; B == 0 returns GOL_OK without a launch.  No atomics, no scratch, no host sync, no allocation: one
 * launch each, bitwise reproducible, capturable as a linear graph.
 * ---------------------------------------------------------------------------------------- */
long long gol_conv3x_packed_elems(int Co, int Ci);
int gol_conv3x_pack(int Co, int Ci, const float* weight, unsigned short* packed, void* stream);
int gol_conv3x_fwd(int B, int Ci, int Co, int H, int W, int pool, const float* x, const unsigned short* packed,
                   const float* bias, float* y, unsigned char* pos, void* stream);
int gol_conv3x_bwd_x(int B, int Ci, int Co, int H, int W, int pool, const unsigned short* packed, const float* y,
                     const unsigned char* pos, const float* g_y, float* g_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * gol_conv4x_*: a linear, bias-free 4x4 / stride 2 / zero padding 1 convolution at precision "bf16x3" (the split product
 * of gol_conv3x_*, on v_mfma_f32_16x16x32_bf16) with forward, input gradient and weight gradient: the feature layers
 * feat_mod[0..3] of URHand's FeatEncoderUNet on their EFFECTIVE weights.  Replaces, in FeatEncoderUNet.forward
 * (ca_code/models/urhand.py:102; layers built at :93 from la.Conv2dWN(n_in, n_out, 4, 2, 1, bias=False),
 * ca_code/nn/layers.py:470),
 *   x = self.feat_mod[i](x)
 * one fp32 MIOpen convolution and, backward, its input-gradient and weight-gradient convolutions:
 *   y  [b,co,Y,X]     = sum_{ci,ky,kx} xpad[b,ci,2Y-1+ky,2X-1+kx] w[co,ci,ky,kx]      xpad = x inside the image, 0 outside
 *   g_x[b,ci,r,c]     = sum_{co,ky,kx} g_y[b,co,Y,X] w[co,ci,ky,kx]                   over 2Y-1+ky = r, 2X-1+kx = c
 *   g_w[co,ci,ky,kx]  = sum_{b,Y,X}    g_y[b,co,Y,X] xpad[b,ci,2Y-1+ky,2X-1+kx]
 *   x [B,Ci,H,W]; w, g_w [Co,Ci,4,4]; y, g_y [B,Co,H/2,W/2]; g_x [B,Ci,H,W].  Every product a b is
 *   lo_a hi_b + hi_a lo_b + hi_a hi_b with split(v): hi = bf16_rne(v), lo = bf16_rne(v - float(hi)); BOTH operands of all
 *   three directions are split (x and g_y while they are staged); products are exact, the sum is fp32, lo lo is dropped:
 *   |result - exact| <= 3.1 2^-16 sum |a||b|.  Inputs finite and of ordinary magnitude, as for gol_conv3x_*.
 * gol_conv4x_pack splits w ONCE per call into packed[gol_conv4x_packed_elems(Co, Ci)] (16-bit elements, 16-byte aligned):
 *   [hi | lo][16 taps][Co / 8][Ci / 8][8 co][8 ci]; the same buffer serves fwd and bwd_x (which transposes a block on its way
 *   to LDS).  gol_conv4x_packed_elems returns 0 for an unsupported (Co, Ci).
 * gol_conv4x_bwd_x: g_x written (8-byte aligned); g_x == NULL: no launch.
 * gol_conv4x_bwd_w: reads the fp32 x and g_y; K (the pixels) is split over workgroups, whose partials go to
 *   scratch[gol_conv4x_bwd_w_scratch_floats] and are added in block order by a second kernel (no float atomics).  The scratch
 *   is blocks x 16 Co Ci floats with blocks = about 512 / ((Ci / 32) ceil(Co / 64)), at most one per 32 output pixels of a
 *   row: never more than (512 + (Ci / 32) ceil(Co / 64)) x 32768 floats, whatever B, H and W.  g_w == NULL: no launch.
 * Supported: Ci % 32 == 0, Co % 32 == 0, H and W even and >= 2, B <= 65535: everything else returns GOL_ERR_UNSUPPORTED
 * before any launch (gol_conv4x_bwd_w_scratch_floats: 0).  A null pointer that is needed returns GOL_ERR_INVALID_ARG;
 * B == 0 returns GOL_OK without a kernel (bwd_w zeroes g_w).  Offsets are 64-bit across planes.  Every output element is a
 * fixed-order sum: bitwise reproducible.  No host sync, no allocation: capturable as a linear graph.
 * ---------------------------------------------------------------------------------------- */
long long gol_conv4x_packed_elems(int Co, int Ci);
int gol_conv4x_pack(int Co, int Ci, const float* weight, unsigned short* packed, void* stream);
int gol_conv4x_fwd(int B, int Ci, int Co, int H, int W, const float* x, const unsigned short* packed, float* y,
                   void* stream);
int gol_conv4x_bwd_x(int B, int Ci, int Co, int H, int W, const unsigned short* packed, const float* g_y, float* g_x,
                     void* stream);
long long gol_conv4x_bwd_w_scratch_floats(int B, int Ci, int Co, int H, int W);
int gol_conv4x_bwd_w(int B, int Ci, int Co, int H, int W, const float* x, const float* g_y, float* g_w, float* scratch,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * gol_conv3ub_*: a 3x3 / stride 1 / zero padding 1 convolution of the channel concatenation of TWO tensors + untied bias +
 * LeakyReLU at precision "bf16x3" (the split product of gol_conv3x_*, on v_mfma_f32_16x16x32_bf16) with forward and all four
 * gradients: one level of the UNet of the MVP teacher on its EFFECTIVE weight.  Replaces, in OLATRGBDecoder.forward_rgb
 * (ca_code/models/hand_teacher_mvp.py:444-467; layers built at :206-241 from nn.Sequential(la.Conv2dWNUB(n_in, n_out,
 * kernel_size=3, height, width, stride=1, padding=1), nn.LeakyReLU(0.2, inplace=True)), ca_code/nn/layers.py),
 *   x = th.cat([x, x_prev], dim=1)        (:460 with joint_feat, :466 with the skip; absent in the encoder)
 *   x = layer(x)                          (:447, :467: F.conv2d + bias[None] + leaky_relu_)
 * and, backward, the activation's, the bias add's, both convolution gradients' and the concatenation's kernels:
 *   xcat = cat(xa [B,Ca,H,W], xb [B,Cb,H,W]) along channels, Ci = Ca + Cb; never written.  Cb == 0: xb is not read.
 *   pre[b,co,r,c]  = sum_{ci,ky,kx} xcat_pad[b,ci,r-1+ky,c-1+kx] w[co,ci,ky,kx] + bias[co,r,c]     bias [Co,H,W]
 *   y              = pre > 0 ? pre : leak pre                                                      y [B,Co,H,W], leak > 0
 *   g_pre          = y > 0 ? g_y : leak g_y      (from the SAVED y: the activation is in place; at y == 0: leak, as torch)
 *   g_xa, g_xb     = rows [0,Ca) and [Ca,Ci) of sum_{co,ky,kx} g_pre[b,co,r+1-ky,c+1-kx] w[co,ci,ky,kx]
 *   g_w[co,ci,ky,kx] = sum_{b,r,c} g_pre[b,co,r,c] xcat_pad[b,ci,r-1+ky,c-1+kx]                    g_w [Co,Ci,3,3]
 *   g_bias[co,r,c] = sum_b g_pre[b,co,r,c]                                                         fp32, b ascending
 *   Every product a b of the three convolutions is lo_a hi_b + hi_a lo_b + hi_a hi_b with split(v): hi = bf16_rne(v),
 *   lo = bf16_rne(v - float(hi)); BOTH operands are split (x and g_pre while they are staged, g_pre AFTER it is formed);
 *   products are exact, the sum is fp32, lo lo is dropped: |result - exact| <= 3.1 2^-16 sum |a||b|.  Zero padding splits
 *   to (0, 0).  Inputs finite and of ordinary magnitude, as for gol_conv3x_*.
 * gol_conv3ub_pack splits w ONCE per call into packed[gol_conv3ub_packed_elems(Co, Ci)] (16-bit elements, 16-byte aligned):
 *   [hi | lo][tap][Co / 8][Cip / 8][8 co][8 ci] with Cip = Ci rounded up to a multiple of 32 and zeros for the channels
 *   past Ci; the same buffer serves fwd and bwd_x (which transposes a block on its way to LDS and mirrors the taps).
 *   gol_conv3ub_packed_elems = 2 x 9 x Co x Cip, or 0 for an unsupported (Co, Ci).
 * gol_conv3ub_bwd_x: g_xa [B,Ca,H,W] and g_xb [B,Cb,H,W] written; only rows < Ci are written; a NULL g_xa or g_xb skips
 *   that tensor's rows (both NULL: no launch).
 * gol_conv3ub_bwd_w: reads the fp32 xa, xb, y and g_y; K (the pixels) is split over workgroups, whose partials go to
 *   scratch[gol_conv3ub_bwd_w_scratch_floats] and are added in block order by a second kernel (no float atomics).  The
 *   scratch is blocks x 9 Co Ci floats with blocks = about 512 / ((Cip / 32) ceil(Co / 64)), at most one per 32 pixels of
 *   a row: never more than (512 + (Cip / 32) ceil(Co / 64)) x 18432 floats, whatever B, H and W.  g_w == NULL: no launch.
 * gol_conv3ub_bwd_bias: one streaming pass over y and g_y.  g_bias == NULL: no launch.
 * Supported: Co % 32 == 0; Ca > 0, Ca % 8 == 0, Cb % 8 == 0, and Ca % 32 == 0 whenever Cb > 0 (a K stage of 32 channels
 * reads one source); Ci need NOT be a multiple of 32 (the loaders supply zeros for the channels past Ci and read nothing
 * for them); any H, W >= 1; B <= 65535 (gol_conv3ub_pack: Co % 32 == 0, Ci % 8 == 0; gol_conv3ub_bwd_bias: Co % 32 == 0).
 * Everything else returns GOL_ERR_UNSUPPORTED before any launch (gol_conv3ub_bwd_w_scratch_floats: 0).  A null pointer
 * that is needed, B < 0 or leak <= 0 returns GOL_ERR_INVALID_ARG; B == 0 returns GOL_OK without a kernel (bwd_w and
 * bwd_bias zero their outputs).  Offsets are 64-bit across planes.  Every output element is a fixed-order sum: bitwise
 * reproducible.  No host sync, no allocation: capturable as a linear graph.
 * ---------------------------------------------------------------------------------------- */
long long gol_conv3ub_packed_elems(int Co, int Ci);
int gol_conv3ub_pack(int Co, int Ci, const float* weight, unsigned short* packed, void* stream);
int gol_conv3ub_fwd(int B, int Ca, int Cb, int Co, int H, int W, float leak, const float* xa, const float* xb,
                    const unsigned short* packed, const float* bias, float* y, void* stream);
int gol_conv3ub_bwd_x(int B, int Ca, int Cb, int Co, int H, int W, float leak, const unsigned short* packed, const float* y,
                      const float* g_y, float* g_xa, float* g_xb, void* stream);
long long gol_conv3ub_bwd_w_scratch_floats(int B, int Ca, int Cb, int Co, int H, int W);
int gol_conv3ub_bwd_w(int B, int Ca, int Cb, int Co, int H, int W, float leak, const float* xa, const float* xb,
                      const float* y, const float* g_y, float* g_w, float* scratch, void* stream);
int gol_conv3ub_bwd_bias(int B, int Co, int H, int W, float leak, const float* y, const float* g_y, float* g_bias,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * gol_upconvx_*: the texture-decoder layer of gol_upconv_* above at precision "bf16x3".  Replaces the same lines of
 * ConvTeacherDecoder.forward (ca_code/models/urhand.py:583-608; layers built at :302-323): F.interpolate(x, (2 Hi, 2 Wi),
 * mode="bilinear", align_corners=True), the MIOpen convolution and the epilogue of texmod0 (:592-597) or texmod1 (:600-606),
 * and their backward kernels.  The formulas are gol_upconv_*'s, with the same integer-ratio coordinate rule and the same modes:
 *   U[b,ci,r,c]   = bilinear(x[b,ci]) by the integer-ratio rule, blended in fp32          (H = 2 Hi, W = 2 Wi; never written)
 *   acc[b,co,r,c] = sum_{ci,ky,kx} Upad[b,ci,r-1+ky,c-1+kx] w[co,ci,ky,kx]
 *   mode 0:  y = lrelu(acc + bias[co,r,c], leak), leak > 0       mode 1:  y = (acc * gate + gb) * scale   (gb may be NULL)
 *   g_pre = g_y * (y > 0 ? 1 : leak) (mode 0; needs y) or scale * gate * g_y (mode 1; needs gate), formed in fp32
 *   g_x = bilinear adjoint of sum_{co,ky,kx} g_pre[b,co,r+1-ky,c+1-kx] w[co,ci,ky,kx];  g_w = sum_{b,r,c} g_pre Upad
 *   g_gate = scale * g_y * acc (acc recomputed), g_gb = scale * g_y
 *   The only difference: every product a b of the three convolutions is lo_a hi_b + hi_a lo_b + hi_a hi_b with split(v):
 *   hi = bf16_rne(v), lo = bf16_rne(v - float(hi)); BOTH operands are split while they are staged (U AFTER the fp32 blend,
 *   g_pre AFTER it is formed); products are exact, the sum is fp32, lo lo is dropped: |result - exact| <= 3.1 2^-16
 *   sum |a||b|.  Padding splits to (0, 0).  Inputs finite and of ordinary magnitude, as for gol_conv3x_*.
 * gol_upconvx_pack splits w_eff [Co,Ci,3,3] ONCE per call into packed[gol_upconvx_packed_elems(Co, Ci)] (16-bit elements,
 *   16-byte aligned): [hi | lo][tap][Cop / 8][Ci / 8][8 co][8 ci] with Cop = Co rounded up to a multiple of 32 and zeros for
 *   the rows past Co (gol_conv3ub_pack's layout padded on the Co side; that entry is not reused because its channel rule,
 *   Co % 32 == 0, is pinned by its tests).  The same buffer serves fwd, bwd_x (which transposes a block on its way to LDS and
 *   mirrors the taps) and bwd_gate.  gol_upconvx_packed_elems = 2 x 9 x Cop x Ci, or 0 for an unsupported (Co, Ci).
 * gol_upconvx_fwd: x [B,Ci,Hi,Wi]; bias [Co,H,W] (mode 0); gate, gb, y [B,Co,H,W].  Nothing but y is written.
 * gol_upconvx_bwd_x: g_x [B,Ci,Hi,Wi] written; per tile of 2 x 14 texels the region of g_U that reaches it (8 x 32 pixels)
 *   is kept on chip and every texel gathers its up-to-5x5 pixels in fp32 (no atomics).  g_x == NULL: no launch.
 * gol_upconvx_bwd_w: g_w [Co,Ci,3,3] written; reads the fp32 x, y or gate, and g_y (U recomputed).  K (the pixels, in chunks
 *   of 32 of an output row) is split over workgroups, whose partials go to scratch[gol_upconvx_bwd_w_scratch_floats] and are
 *   added in block order by a second kernel (no float atomics).  The scratch is blocks x 9 Co Ci floats with
 *   blocks = min(ceil(512 / pairs), chunks) rounded so that no block is empty, pairs = (Ci / 32) ceil(Co / 64),
 *   chunks = B H ceil(W / 32): never more than (512 + pairs) x 18432 floats, whatever B, Hi and Wi.  g_w == NULL: no launch.
 * gol_upconvx_bwd_gate (mode 1): g_gate [B,Co,H,W] = scale * g_y * acc with acc recomputed by the forward kernel; g_gb (may
 *   be NULL) rides along.  g_gate == NULL: no launch, and g_gb is NOT written.
 * g_bias (mode 0) and g_gb without g_gate (mode 1) hold no product: they are gol_upconv_bwd's streaming pass, called with
 *   every other output NULL.
 * Supported: Ci % 32 == 0, Co % 16 == 0 (six of the seven layer shapes; 16 -> 4 stays on gol_upconv_*), Hi, Wi >= 1,
 * B <= 65535; everything else returns GOL_ERR_UNSUPPORTED before any launch (the size queries: 0).  A negative size, a mode
 * other than 0 / 1, leak <= 0 in mode 0 or a null pointer that is needed returns GOL_ERR_INVALID_ARG before any launch;
 * B == 0 returns GOL_OK without a kernel (bwd_w zeroes g_w).  Offsets are 64-bit across planes.  Every output element is a
 * fixed-order sum: bitwise reproducible.  No host sync, no allocation: capturable as a linear graph.
 * ---------------------------------------------------------------------------------------- */
long long gol_upconvx_packed_elems(int Co, int Ci);
int gol_upconvx_pack(int Co, int Ci, const float* weight, unsigned short* packed, void* stream);
int gol_upconvx_fwd(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale, const float* x,
                    const unsigned short* packed, const float* bias, const float* gate, const float* gb, float* y,
                    void* stream);
int gol_upconvx_bwd_x(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale, const unsigned short* packed,
                      const float* y, const float* gate, const float* g_y, float* g_x, void* stream);
long long gol_upconvx_bwd_w_scratch_floats(int B, int Ci, int Co, int Hi, int Wi);
int gol_upconvx_bwd_w(int B, int Ci, int Co, int Hi, int Wi, int mode, float leak, float scale, const float* x,
                      const float* y, const float* gate, const float* g_y, float* g_w, float* scratch, void* stream);
int gol_upconvx_bwd_gate(int B, int Ci, int Co, int Hi, int Wi, float scale, const float* x, const unsigned short* packed,
                         const float* g_y, float* g_gate, float* g_gb, void* stream);

/* ------------------------------------------------------------------------------------------
 * gol_mbconv_front_fwd / gol_mbconv_front_bwd_x: the front of an MBConv block of the frozen EfficientNet-B0 feature
 * network of the `effnet` / `effnet_phys` losses (ca_code/loss/effnet.py:45-51 runs torchvision's
 * efficientnet_b0().features[0:4]; registered at ca_code/loss/perceptual.py:60-69): expand 1x1 + BN + SiLU, depthwise
 * k x k / stride s + BN, and the squeeze of the squeeze-excite, as one operator.  Replaces the MIOpen 1x1 and depthwise
 * convolutions, two batch_norm and two silu passes and the adaptive average pool; the expanded tensor never exists in
 * memory.  BatchNorm is folded into (weight, bias) by the caller.  Expand in exact fp32 on v_mfma_f32_16x16x4_f32.
 *   x [B,Ci,H,W]; w_e [Ce,Ci]; b_e [Ce]; w_d [Ce,k,k]; b_d [Ce]; p = (k - 1) / 2; Ho = (H + 2p - k) / stride + 1, Wo alike
 *   e = SiLU(sum_ci w_e[c,ci] x[b,ci] + b_e[c])      (expand = 0: e = x, Ci == Ce, w_e and b_e may be NULL)
 *   z [B,Ce,Ho,Wo] = sum_taps w_d[c,ky,kx] epad[b,c, ro stride - p + ky, co stride - p + kx] + b_d[c]   (pre-activation)
 *   epad = e inside the image, 0 outside (NOT SiLU(b_e))
 *   partials [B,Ce,T] (double), T = gol_mbconv_front_tiles(H, W, k, stride): per output tile the sum of SiLU(z) over the
 *   tile, taken from the accumulators in a fixed order; ssum[b,c] = sum_t partials[b,c,t] is the caller's.
 *   SiLU(v) = v / (1 + expf(-v)), accurate expf, IEEE division.
 * gol_mbconv_front_bwd_x: the input gradient only (the weights are frozen).  z = the forward's z.
 *   g_zt = g_z + g_ssum[b,c] SiLU'(z), SiLU'(v) = sg (1 + v (1 - sg)), sg = 1 / (1 + expf(-v)), formed while loading
 *   g_e = the transposed depthwise convolution of g_zt, read from the same w_d with mirrored taps
 *   g_x [B,Ci,H,W] written = sum_c w_e[c,ci] g_e SiLU'(e_pre), e_pre recomputed from x; expand = 0: g_x = g_e (x may be NULL)
 *   No atomics, no scratch: bitwise reproducible.
 * Supported: k 3 or 5; stride 1 or 2; Ci % 8 == 0; Ce % 16 == 0; Ci == Ce without expand; any H, W >= 1; B <= 65535:
 * everything else returns GOL_ERR_UNSUPPORTED (gol_mbconv_front_tiles: 0).  A null pointer with positive sizes returns
 * GOL_ERR_INVALID_ARG; B == 0 returns GOL_OK without a launch.  No host sync, no allocation: one launch each, capturable
 * as a linear graph.
 * ---------------------------------------------------------------------------------------- */
int gol_mbconv_front_tiles(int H, int W, int k, int stride);
int gol_mbconv_front_fwd(int B, int Ci, int Ce, int H, int W, int k, int stride, int expand, const float* x,
                         const float* w_e, const float* b_e, const float* w_d, const float* b_d, float* z, double* partials,
                         void* stream);
int gol_mbconv_front_bwd_x(int B, int Ci, int Ce, int H, int W, int k, int stride, int expand, const float* x,
                           const float* w_e, const float* b_e, const float* w_d, const float* z, const float* g_z,
                           const float* g_ssum, float* g_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * SSIM image loss ("next" row).  Replaces `ssim` / `_ssim`
 * (ca_code/utils/ssim.py:25-65) as used by rgb_ssim (ca_code/loss/__init__.py:478-494): 11x11 Gaussian
 * window (sigma 1.5, zero padding), C1 = 0.01^2, C2 = 0.03^2, masked mean.
 *   img1 (target), img2 (prediction: the differentiated argument) [B,C,H,W]; mask NULL, [B,1,H,W] or [B,C,H,W]
 * fwd writes partial[B*C*gol_ssim_blocks(H,W)] = per-workgroup sums of ssim_map*mask (caller: sum / denominator)
 *     and, when dmap != NULL, dmap[3,B,C,H,W] = mask * d ssim / d (mu2, E[img2^2], E[img1*img2]) for the backward;
 * bwd writes g_img2 = g_scale[0] * d(sum of ssim_map*mask)/d img2   (g_scale: device scalar, e.g. -g_loss/denominator).
 * ---------------------------------------------------------------------------------------- */
int gol_ssim_blocks(int H, int W);
int gol_ssim_fwd(int B, int C, int H, int W, int mask_c, const float* img1, const float* img2, const float* mask,
                 float* partial, float* dmap, void* stream);
int gol_ssim_bwd(int B, int C, int H, int W, const float* img1, const float* img2, const float* dmap,
                 const float* g_scale, float* g_img2, void* stream);

/* ------------------------------------------------------------------------------------------
 * URHand shadow-map lookup with 3x3 PCF.  Replaces the per-texel part of get_shadow_map
 * (ca_code/utils/shadowmap.py:30-96; projection ca_code/utils/geom.py:599-631): forward only (the reference
 * calls it under no_grad, ca_code/models/urhand.py:404,492).
 *   depth [B*L,dh,dw] light-camera depth images (0 = empty; from the mesh rasteriser), Rt [B*L,3,4] = [R | t] with
 *   p_cam = R p + t, intrinsics fx,fy,cx,cy (the reference uses 1000,1000,dw/2,dh/2), postex [B,3,H,W] texel
 *   positions, nml [B,3,H,W] or NULL (no back-face term) -> out [B*L,1,H,W] = in_shadow, or exp(-in_shadow/exp_scale)
 *   when exp_scale > 0 (urhand.py:416 uses 8).
 * ---------------------------------------------------------------------------------------- */
int gol_shadow_pcf(int B, int L, int H, int W, int dh, int dw, const float* depth, const float* Rt, float fx, float fy,
                   float cx, float cy, const float* postex, const float* nml, float exp_scale, float* out,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Image tail of AutoEncoder.forward between the rasterizer and the losses, one pass each way over
 * rgb[B,3,H,W]:  out = blur( cal(rgb) + (1 - alpha) * bg * bg_scale )
 *   cal      CalV5.forward, ca_code/nn/color_cal.py:211-241, as cal_M[B,3,3] / cal_b[B,3] (both NULL = identity):
 *            cal(rgb)[c] = sum_j cal_M[b,c,j] * rgb[j] + cal_b[b,c]  (grey cameras: three identical rows)
 *   alpha[B,H,W], bg[B,3,H,W] (both NULL = no composite), bg_scale[B] or NULL: ca_code/models/rgca.py:226-230
 *   blur_w[B,3] (NULL = no blur): LearnableBlur.forward, ca_code/nn/dof_cal.py:44-56, softmaxed weights of
 *            (identity, gaussian_blur 3x3, gaussian_blur 7x7), torchvision semantics (reflect padding, H, W >= 4)
 * bwd: g_rgb[B,3,H,W] is written; `partials` (gol_imgtail_partial_floats(B,H,W) floats, [B, tiles, 16]) receives
 *   per-workgroup partial sums of the parameter gradients -- columns 0..2 blur_w, 3..5 cal_b, 6..14 cal_M (row-major)
 *   -- to be summed over `tiles` by the caller (no float atomics).  No gradient to alpha / bg (alpha is detached in the
 *   reference, rgca.py:137).
 * ---------------------------------------------------------------------------------------- */
int64_t gol_imgtail_partial_floats(int B, int H, int W);
int gol_imgtail_fwd(int B, int H, int W, const float* rgb, const float* alpha, const float* bg,
                    const float* bg_scale, const float* cal_M, const float* cal_b, const float* blur_w,
                    float* out, void* stream);
int gol_imgtail_bwd(int B, int H, int W, const float* rgb, const float* alpha, const float* bg,
                    const float* bg_scale, const float* cal_M, const float* cal_b, const float* blur_w,
                    const float* g_out, float* g_rgb, float* partials, void* stream);

/* ------------------------------------------------------------------------------------------
 * Triangle-mesh z-buffer rasterizer: the index / depth / barycentric images the reference obtains from the third-party
 * drtk (drtk.rasterize + drtk.render, ca_code/utils/render_drtk.py:44-46); consumer on the hot path: the per-light depth
 * render of the shadow map (ca_code/utils/shadowmap.py:39-50).  Forward only.
 *   v_pix[B,V,3] = (pixel x, pixel y, camera z) per vertex, vi[F,3] int32 vertex indices (shared by the B meshes)
 *   index_img[B,H,W] int32: nearest covering face, -1 = none;  depth_img[B,H,W]: its depth, 0 = none;
 *   bary_img[B,3,H,W] (may be NULL): perspective-correct barycentrics of the sample.
 * Conventions (drtk's source is not in the reference tree): sample at the pixel centre (j + 0.5, i + 0.5); coverage =
 * all edge functions >= 0, either winding; faces with a vertex at z <= 0 are skipped; depth ties -> lower face index.
 * Coverage is decided in fp32 on un-normalised edge functions anchored at the face's first vertex.  The decision is EXACT
 * (a sample on a shared edge is covered by both neighbours, one on the outline is covered) only while every product of an
 * edge-vector component of the face with a sample offset from its first vertex fits 24 bits: e.g. vertices on a
 * quarter-pixel grid and faces a few tens of pixels across.  Outside that range (finer grids, larger faces, any generic
 * mesh) a sample within fp32 rounding of an edge may be taken or rejected by either neighbour -- also by both: on-edge
 * samples of a shared edge are not guaranteed watertight there; samples farther than rounding from every edge are.
 * Also skipped: a face with a vertex index outside [0, V), a non-finite x / y, a NaN z, zero area, or an extent above
 * ~1e34 pixels (its area overflows fp32).
 * workspace: gol_mesh_raster_workspace_bytes(B, F) bytes of device scratch (face records, packed tile bounds, the
 * per-view tile boxes and their in-box tile prefix).  The images are cleared by a streaming fill; only tiles inside a
 * view's mesh box are rasterized, by a fixed grid of workgroups that strides over them.
 * ---------------------------------------------------------------------------------------- */
int64_t gol_mesh_raster_workspace_bytes(int B, int F);
int gol_mesh_raster(int B, int V, int F, int H, int W, const float* v_pix, const int32_t* vi, int32_t* index_img,
                    float* depth_img, float* bary_img, void* workspace, void* stream);
/* gol_mesh_raster_flat: the same rasteriser (same setup, coverage rules, workspace and images) for a mesh whose faces all
 * lie at ONE depth, such as UV triangles: z only has to be > 0, there is no depth test, among the faces that cover a
 * sample the LOWEST FACE INDEX wins, and depth_img holds 1 where covered.  (gol_mesh_raster's tie rule needs exactly
 * equal interpolated depths; for coplanar faces those differ in the last bit of w0 + w1 + w2.)  No barycentric image. */
int gol_mesh_raster_flat(int B, int V, int F, int H, int W, const float* v_pix, const int32_t* vi, int32_t* index_img,
                         float* depth_img, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Textured mesh render after gol_mesh_raster, forward and backward: the rest of the reference's drtk layer
 * (ca_code/utils/render_drtk.py:44-70: drtk.render's differentiable depth / barycentrics, drtk.interpolate of the uv,
 * grid_sample of the texture, drtk.edge_grad_estimator), as goliath_amd.meshraster.RenderLayer composes it in PyTorch.
 *   v_pix[B,V,3], vi[F,3] int32 as for gol_mesh_raster; vt[Vt,2] uv in [0,1], vti[F,3] int32 uv ids; tex[B,C,Ht,Wt]
 *   (planar, any C >= 1); index_img[B,H,W] int32, depth_img[B,H,W], bary_img[B,3,H,W] as gol_mesh_raster wrote them.
 *   A pixel whose face or uv / vertex ids are out of range counts as empty.
 * fwd writes (every element) vt_img[B,2,H,W] = sum_k bary_k (2 vt[vti[f,k]] - 1), render[B,C,H,W] =
 *   grid_sample(tex, vt_img, bilinear, align_corners=False, zero padding) * mask, mask[B,1,H,W] = (index >= 0); 0 where empty.
 * bwd ACCUMULATES (caller zeroes) g_tex[B,C,Ht,Wt] (NULL = not wanted) and g_v_pix[B,V,3] (NULL = not wanted): from
 *   g_render[B,C,H,W] and the optional g_vt_img[B,2,H,W], g_bary_img[B,3,H,W], g_depth_img[B,H,W] (NULL = zero), chained
 *   through the perspective-correct barycentrics of the pixel's face re-evaluated from v_pix (anchored at the face's first
 *   vertex, sampled at (j + 0.5, i + 0.5), w_k = b_k / z_k, bary = w / sum w, depth = 1 / sum w: all nine coordinates).
 *   v_pix is needed when g_v_pix is given.  Visibility (index_img) is held fixed.
 * edge_bwd ACCUMULATES into g_v_pix the discontinuity term of meshraster._EdgeGrad (right / lower neighbour pairs whose
 *   faces differ and share no mesh edge; occluder = nearer face, empty = +inf; its edge crossing the pair's segment
 *   nearest to the middle, within one pixel; coefficient sum_c (g_p + g_q) (img_p - img_q) / 2 times d_ac^2 /
 *   (d_ac^2 + d_al^2), chained into the edge's two endpoints' image coordinates; nothing to z).  render = the forward's
 *   render, g_render its upstream gradient.  edge_stats (int32[2], may be NULL) ACCUMULATES {pairs kept, pairs without a
 *   crossing within a pixel}.
 * No workspace.  Float-atomic order makes g_tex and g_v_pix nondeterministic in the last bits.
 * ---------------------------------------------------------------------------------------- */
int gol_mesh_render_fwd(int B, int F, int Vt, int C, int H, int W, int Ht, int Wt, const float* vt, const int32_t* vti,
                        const float* tex, const int32_t* index_img, const float* bary_img, float* vt_img, float* render,
                        float* mask, void* stream);
int gol_mesh_render_bwd(int B, int V, int F, int Vt, int C, int H, int W, int Ht, int Wt, const float* v_pix,
                        const int32_t* vi, const float* vt, const int32_t* vti, const float* tex, const int32_t* index_img,
                        const float* bary_img, const float* g_render, const float* g_vt_img, const float* g_bary_img,
                        const float* g_depth_img, float* g_tex, float* g_v_pix, void* stream);
int gol_mesh_render_edge_bwd(int B, int V, int F, int C, int H, int W, const float* v_pix, const int32_t* vi,
                             const int32_t* index_img, const float* depth_img, const float* render,
                             const float* g_render, float* g_v_pix, int32_t* edge_stats, void* stream);

/* ------------------------------------------------------------------------------------------
 * uvgeom: tracked mesh -> UV position / normal maps, forward and backward (csrc/uvgeom.hip).  Replaces the reference's
 * per-step PyTorch of ca_code/utils/geom.py:308-346 (values_to_uv, face_normals, vert_normals) as called by
 * PrimDecoder.forward (ca_code/models/rgca.py:483-491), ConvTeacherDecoder.forward (ca_code/models/urhand.py:375-394, 447)
 * and hand_mvp.py:231-236, 394.  The topology arrays are packed once by goliath_amd.uvgeom.UVTopology (all int32):
 *   vi[F,3]; vf_start[V+1], vf_slot[3F]: vertex -> (face, corner) slots, slot = 3 face + corner, ascending per vertex;
 *   texel_rec[S*S,4]: triple id (-1 = uncovered, geom.py:310) and the bit patterns of the texel's three barycentrics;
 *   triples[T,3]: the distinct vertex triples; item_start[I+1], item_tid[I], texel_of[M]: the covered texels grouped by
 *   triple, every triple's run cut into items of at most 64 texels; vt_start[V+1], vt_slot[3I]: vertex -> (item, corner)
 *   slots, slot = 3 item + corner.  Ids out of range count as absent (uncovered texel, skipped face).
 * gol_vert_normals_fwd: vert_normals(verts, vi, eps) (geom.py:337-346): vn[B,V,3] = s / max(|s|, eps), s = the sum over
 *   the vertex's faces of cross / max(|cross|, 1e-5) (geom.py:327-334), summed in face order.
 * gol_vert_normals_bwd: g_vn[B,V,3] -> g_verts[B,V,3] (every element written); g_s[B,V,3] is scratch.
 * gol_values_to_uv_fwd: values_to_uv (geom.py:308-324) for values[B,V,C], any C >= 1: out[B,C,S,S], every element
 *   written, 0 where uncovered.
 * gol_values_to_uv_bwd: g_out[B,C,S,S] -> g_values[B,V,C] (every element written); item_sums[B,I,3,C] is scratch.
 * gol_uvgeom_fwd: the pair of rgca.py:483-491 in one call: vn[B,V,3] as gol_vert_normals_fwd(eps = vn_eps) writes it
 *   (kept by the caller for the backward), postex[B,3,S,S] = to_uv(verts), tn[B,3,S,S] = x / max(|x|, norm_eps) with
 *   x = to_uv(vn) (F.normalize over the channels: norm_eps = 1e-12; urhand.py:394 uses 1e-5).
 * gol_uvgeom_bwd: g_postex, g_tn [B,3,S,S] (NULL = zero) -> g_verts[B,V,3] (every element written);
 *   item_sums[B,I,18] and g_s[B,V,3] are scratch.
 * A norm below its eps makes the denominator a constant in the derivative (autograd's clamp).  No atomics: every sum
 * has a fixed order and all outputs are bitwise reproducible.
 * ---------------------------------------------------------------------------------------- */
int gol_vert_normals_fwd(int B, int V, int F, const float* verts, const int32_t* vi, const int32_t* vf_start,
                         const int32_t* vf_slot, float eps, float* vn, void* stream);
int gol_vert_normals_bwd(int B, int V, int F, const float* verts, const int32_t* vi, const int32_t* vf_start,
                         const int32_t* vf_slot, float eps, const float* g_vn, float* g_s, float* g_verts, void* stream);
int gol_values_to_uv_fwd(int B, int V, int C, int S, int T, const float* values, const int32_t* texel_rec,
                         const int32_t* triples, float* out, void* stream);
int gol_values_to_uv_bwd(int B, int V, int C, int S, int T, int I, const int32_t* texel_rec, const int32_t* item_start,
                         const int32_t* texel_of, const int32_t* vt_start, const int32_t* vt_slot, const float* g_out,
                         float* item_sums, float* g_values, void* stream);
int gol_uvgeom_fwd(int B, int V, int F, int S, int T, const float* verts, const int32_t* vi, const int32_t* vf_start,
                   const int32_t* vf_slot, const int32_t* texel_rec, const int32_t* triples, float vn_eps, float norm_eps,
                   float* vn, float* postex, float* tn, void* stream);
int gol_uvgeom_bwd(int B, int V, int F, int S, int T, int I, const float* verts, const int32_t* vi,
                   const int32_t* vf_start, const int32_t* vf_slot, const int32_t* texel_rec, const int32_t* triples,
                   const int32_t* item_start, const int32_t* item_tid, const int32_t* texel_of, const int32_t* vt_start,
                   const int32_t* vt_slot, float vn_eps, float norm_eps, const float* vn, const float* g_postex,
                   const float* g_tn, float* item_sums, float* g_s, float* g_verts, void* stream);

/* ------------------------------------------------------------------------------------------
 * uvframes: URHand's per-texel tangent frames, normal map and view conditioning, forward and backward
 * (csrc/uvframes.hip).  Replaces, in ConvTeacherDecoder.forward, ca_code/models/urhand.py:366-392 (pass 1), :467-486
 * (pass 2) and :573-578 (view conditioning) with the helpers they call: compute_tbn_uv_given_normal
 * (ca_code/utils/geom.py:432-470), xyz2normals (geom.py:665-686), vert_normals (geom.py:337-346).  On top of uvgeom's
 * arrays for index_image (texel_rec, triples, item_start, texel_of) goliath_amd.uvframes.UVFramesTopology packs:
 *   tri_const[T,4] float: (f, vt01.y, vt02.y, 0) of tri_uv = vt[v2uv[triple, 0]] (urhand.py:369: the FIRST uv slot of a
 *     vertex), fin = vt01.x vt02.y - vt01.y vt02.x, |fin| < 1e-8 -> +1e-8, f = 1 / fin (geom.py:451-454), in float32;
 *   tri_item_start[T+1]: a triple's run of items; vq_start[V+1], vq_slot[3T]: vertex -> (triple, corner), slot = 3 t + k;
 *   ntexel_rec, ntriples, nitem_start, ntexel_of, nvt_start, nvt_slot (Tn triples, In items): uvgeom's arrays for the
 *     image vi[face_index_image], the vertex triple mode 0 interpolates normals over (urhand.py:377).
 * Per (view, triple): t0 = raw / max(|raw|, 1e-5), raw = f (v01 vt02.y - v02 vt01.y) (geom.py:456-459).
 * Per (view, covered texel): the normal n,
 *   mode 0 (urhand.py:375-383): n = x / max(|x|, 1e-5), x = sum_k bary_k vn[ntriple_k], vn = gol_vert_normals_fwd(eps 1e-5);
 *   mode 1 (urhand.py:467-468): n = c / max(|c|, 1e-8), c = U x V, U = (p[r+1,c] - p[r-1,c]) / -2,
 *           V = (p[r,c+1] - p[r,c-1]) / -2 on posmap, zeros beyond the map, neighbours read whether covered or not;
 *   b = n x t0, b /= max(|b|, 1e-5); t = b x n, t /= max(|t|, 1e-5) (geom.py:462-469); rows (t, -b, s n), s = -1 with
 *   flip_normal (urhand.py:385-392, :479-486).  v = d / max(|d|, 1e-12), d = cam_pos - posmap (urhand.py:573).
 * gol_uvframes_fwd writes every element of nml[B,3,S,S] = row 2, of viewout[B,3,S,S] = rows . v (NULL = not wanted; needs
 *   cam_pos[B,3] and posmap[B,3,S,S]) and of frames[B,S,S,3,3] (NULL = not wanted); zeros where uncovered.  vn[B,V,3]
 *   (mode 0) and t0[B,T,3] are written for the backward.
 * gol_uvframes_bwd: g_nml, g_viewout, g_frames (NULL = zero) -> g_verts[B,V,3], g_posmap[B,3,S,S] (mode 1's stencil and
 *   the view term; NULL allowed in mode 0 without g_cam_pos) and g_cam_pos[B,3] (NULL = not wanted), each fully written.
 *   scratch: gol_uvframes_bwd_scratch_floats(...) floats, 8-byte aligned.
 * A norm below its clamp makes the denominator a constant in the derivative, at equality the gradient passes; fin's clamp
 * is a topology constant.  No atomics: every sum has a fixed order, all outputs are bitwise reproducible.
 * ---------------------------------------------------------------------------------------- */
long long gol_uvframes_bwd_scratch_floats(int B, int V, int S, int T, int I, int In, int mode);
int gol_uvframes_fwd(int B, int V, int F, int S, int T, int Tn, int mode, int flip_normal, const float* verts,
                     const int32_t* vi, const int32_t* vf_start, const int32_t* vf_slot, const int32_t* texel_rec,
                     const int32_t* triples, const float* tri_const, const int32_t* ntexel_rec, const int32_t* ntriples,
                     const float* posmap, const float* cam_pos, float* vn, float* t0, float* nml, float* viewout,
                     float* frames, void* stream);
int gol_uvframes_bwd(int B, int V, int F, int S, int T, int Tn, int I, int In, int mode, int flip_normal,
                     const float* verts, const int32_t* vi, const int32_t* vf_start, const int32_t* vf_slot,
                     const int32_t* texel_rec, const int32_t* triples, const float* tri_const,
                     const int32_t* item_start, const int32_t* texel_of, const int32_t* tri_item_start,
                     const int32_t* vq_start, const int32_t* vq_slot, const int32_t* ntexel_rec, const int32_t* ntriples,
                     const int32_t* nitem_start, const int32_t* ntexel_of, const int32_t* nvt_start,
                     const int32_t* nvt_slot, const float* posmap, const float* cam_pos, const float* vn, const float* t0,
                     const float* g_nml, const float* g_viewout, const float* g_frames, float* scratch, float* g_verts,
                     float* g_posmap, float* g_cam_pos, void* stream);

/* ------------------------------------------------------------------------------------------
 * uvtex: URHand's texture tail between the decoder's relight_preds["tex"] and the RGBA textures the renderer takes, one
 * pass forward and one pass backward (csrc/uvtex.hip).  Replaces, in AutoEncoder.forward_tex / forward,
 * ca_code/models/urhand.py:721-729 + :741 (gain / bias), :743-745 into CalV5.forward (ca_code/nn/color_cal.py:211-241, as
 * the per-view cal_M[B,3,3] / cal_b[B,3] of goliath_amd.imgtail.cal_v5_matrix; NULL = no cal), :747 (clamp), :805-807
 * into resample_tex (ca_code/utils/seams.py:21-25) and :824-825 (alpha packing).
 *   tex[B,C,S,S], C = 2: (gain, bias) shared by the colours; C = 4: gain 0..2, bias 3; C = 6: gain 0..2, bias 3..5.
 *   tex_mean[B,3,S,S] (mean_batched != 0) or [1,3,S,S] (0), used clamped to [0, 255]: urhand.py:740 clamps it in place
 *   (through a detached alias) before :741 reads it -- a no-op for a colour mean; tex_std a scalar (urhand.py:666).
 *   pre[c] = clamp(sum_j cal_M[c][j] (tex_mean[j] gain[j] + bias[j] tex_std) + cal_b[c], 0, 255)
 *   out    = (1 - w) pre + w bilinear(pre, uv),  uvs[S,S,2], weights[S,S] (both NULL = no resample: out = pre)
 * bilinear is grid_sample's (align_corners=False, padding_mode="border"): sample point x = clip(u S - 0.5, 0, S - 1),
 * likewise y; taps floor and floor + 1; a tap at index S contributes nothing.  The taps' pre values are recomputed, not
 * read back; texels with w == 0 take no taps and get out = pre exactly.
 * gol_uvtex_fwd writes texrec_before_warp[B,3,S,S] = pre and tex_rgba[B,4,S,S] = (out, 1).
 * gol_uvtex_bwd: g_tex_rgba[B,4,S,S] (channel 3 ignored), g_texrec_before_warp[B,3,S,S] (NULL = zero) -> g_tex[B,C,S,S]
 *   and, with a cal, partials[gol_uvtex_partial_floats(B, S)] = [B, blocks, 16] per-workgroup sums (0..2: cal_b,
 *   3..11: cal_M row-major, 12..15: zero) that the caller adds over `blocks`.  The seam adjoint is a gather over the
 *   transposed tap list goliath_amd.uvtex.pack_seams builds (CSR by destination texel t: entries row_start[t] ..
 *   row_start[t+1] hold src = the band texel whose sample reads t, coeff = w[src] * bilinear weight):
 *     g_pre[t] = (1 - w[t]) g[t] + sum_e coeff[e] g[src[e]] + g_texrec_before_warp[t]
 *   then the clamp mask (torch's: passes where 0 <= x <= 255), cal_M^T, and the gain / bias products (a shared gain or
 *   bias channel gets the sum over the colours).  No gradient to tex_mean (a buffer, detached at urhand.py:778), uvs or
 *   weights.  No atomics: every output is bitwise reproducible.
 * gol_pack_rgba_fwd / _bwd: out[B,4,S,S] = (clamp(x scale, lo, hi), 1) for x[B,3,S,S] (urhand.py:788-790 + :826 with
 *   scale 255); g_x = scale [lo <= x scale <= hi] g_out[:, :3].
 * gol_normal_rgba (forward only, the reference detaches): urhand.py:828-832 and :843-847, out[B,4,S,S], channel
 *   c = (1 - sum_j R[c][j] nml[j]) 127.5, channel 3 = 1, R = Rt[:, :3, :3] of Rt[B,3,4] (rt_stride 12) or [B,4,4] (16).
 * ---------------------------------------------------------------------------------------- */
int64_t gol_uvtex_partial_floats(int B, int S);
int gol_uvtex_fwd(int B, int C, int S, int mean_batched, const float* tex, const float* tex_mean, float tex_std,
                  const float* cal_M, const float* cal_b, const float* uvs, const float* weights,
                  float* texrec_before_warp, float* tex_rgba, void* stream);
int gol_uvtex_bwd(int B, int C, int S, int mean_batched, const float* tex, const float* tex_mean, float tex_std,
                  const float* cal_M, const float* cal_b, const float* weights, const int32_t* row_start,
                  const int32_t* src, const float* coeff, const float* g_tex_rgba, const float* g_texrec_before_warp,
                  float* g_tex, float* partials, void* stream);
int gol_pack_rgba_fwd(int B, int S, float scale, float lo, float hi, const float* x, float* out, void* stream);
int gol_pack_rgba_bwd(int B, int S, float scale, float lo, float hi, const float* x, const float* g_out, float* g_x,
                      void* stream);
int gol_normal_rgba(int B, int S, int rt_stride, const float* nml, const float* Rt, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * uvtopo: the constant UV topology images GeometryModule.__init__ registers (ca_code/utils/geom.py:197-249), without
 * pytorch3d and without the KD-tree (csrc/uvtopo.hip).  Built once per model; forward only, no atomics, reproducible.
 * Texel (r, c) of an [H,W] image is sampled at uv = ((c + 0.5) / W, (r + 0.5) / H); flip_uv != 0 mirrors v (1 - v, in
 * fp32) first.  That sample point is the reference's own (geom.py:133-139) and so are the barycentric arithmetic and the
 * impaint semantics; coverage exactly ON an edge (covered here) and the winner among overlapping faces (lowest index)
 * are this library's stated conventions: pytorch3d's are not in the reference tree.
 * gol_uv_face_index: make_uv_face_index (geom.py:31-66) after its `1 - vt`: face_img[H,W] int32 = the UV triangle
 *   vti[F,3] (int32 ids into vt[Vt,2]) that holds the texel's sample, -1 = none, by gol_mesh_raster_flat on
 *   v_pix = (u W, v H, 1): gol_mesh_raster's coverage rules, the lowest face index where faces overlap.  workspace: gol_uv_face_index_workspace_bytes(Vt, F, H, W)
 *   bytes, 16-byte aligned.
 * gol_uv_topology: make_uv_vert_index (geom.py:69-83), make_uv_barys / bary_coords (geom.py:86-142) and the valid mask
 *   (geom.py:228) from face_img: index_image[H,W,3] int64 = vi[face] (-1 where empty), face_index_image[H,W] int64,
 *   bary_image[H,W,3] = bary_coords of the sample in the triangle's uv (anchored at its third vertex, denom clamped away
 *   from 0 by 1e-6 keeping its sign, b2 = 1 - b0 - b1; no contraction; 0 where empty), valid_mask[H,W] bytes 0 / 1.
 *   A face id outside [0, F) or a uv id outside [0, Vt) counts as empty.  Every element is written.
 * gol_nearest_valid: the KD-tree query of index_image_impaint (geom.py:158-172): for every texel with valid == 0 the
 *   valid texel at the smallest squared distance over integer (row, col), ties to the lexicographically smallest
 *   (row, col), accepted while d^2 <= max_d2: src[H,W] int32 = row * W + col of the source, -1 for valid texels and for
 *   texels without an accepted source (every element written).  col_near[H,W] int32 is scratch.  H <= 65535.
 * gol_impaint_gather: the copies of geom.py:180-191 / 238-244 for up to three images at once, as 4-byte words:
 *   out_k[p] = in_k[src[p] >= 0 ? src[p] : p] for the w_k words of texel p (int64 x 3: w = 6; fp32 x 3: w = 3; in_k NULL =
 *   image absent); out of place.
 * ---------------------------------------------------------------------------------------- */
int64_t gol_uv_face_index_workspace_bytes(int Vt, int F, int H, int W);
int gol_uv_face_index(int Vt, int F, int H, int W, int flip_uv, const float* vt, const int32_t* vti, int32_t* face_img,
                      void* workspace, void* stream);
int gol_uv_topology(int F, int Vt, int H, int W, int flip_uv, const int32_t* face_img, const int32_t* vi,
                    const int32_t* vti, const float* vt, int64_t* index_image, int64_t* face_index_image,
                    float* bary_image, uint8_t* valid_mask, void* stream);
int gol_nearest_valid(int H, int W, int64_t max_d2, const uint8_t* valid, int32_t* col_near, int32_t* src, void* stream);
int gol_impaint_gather(int64_t P, const int32_t* src, int w0, const uint32_t* in0, uint32_t* out0, int w1,
                       const uint32_t* in1, uint32_t* out1, int w2, const uint32_t* in2, uint32_t* out2, void* stream);

/* ------------------------------------------------------------------------------------------
 * viewtex: camera images unwrapped into UV space and their mean over many views (csrc/viewtex.hip): the per-camera body
 * of ca_code/scripts/run_gen_texmean.py:83-108 through ca_code/utils/tex.py:21-63.  Forward only, no atomics, no host
 * sync, bitwise reproducible.
 * gol_face_visibility: compute_face_visibility (ca_code/utils/geom.py:834-845) without its per-view th.unique:
 *   index_img[B,H,W] int32 (-1 = empty) -> face_vis[B,F] bytes, zeroed on the stream first, then 1 for every face index
 *   found in view b.  An index outside [-1, F) is IGNORED (the reference's indexed write would raise).
 * gol_view_texture: compute_uv_visiblity_face + compute_view_texture (geom.py:847-910) for B views at once.
 *   verts: view b's [V,3] at verts + b * verts_bstride floats (0 = one posed mesh seen by B cameras); image[B,3,H,W];
 *   K[B,3,3]; Rt[B,3,4]; index_image_uv[S_h,S_w,3] int32, bary_image_uv[S_h,S_w,3], face_index_uv[S_h,S_w] int32 (-1 =
 *   empty; ids outside the mesh count as -1); face_vis[B,F] from gol_face_visibility.  Per view and texel, in fp32 in the
 *   reference's order: xyz = sum_k verts[idx_k] bary_k; p = K (R xyz + t) with the full 3x3 K; pix = p.xy / p.z;
 *   g = 2 (pix / (W, H)) - 1; grid_sample(nearest, align_corners=False, border): ((g + 1) size - 1) / 2 clamped to
 *   [0, size - 1], rounded to nearest even; value = (index_image_uv[..., 0] != -1 ? rgb : 0) * vis with
 *   vis = face_index_uv != -1 && face_vis[b, face_index_uv]; with has_threshold != 0 the value is multiplied by
 *   all_c(value_c <= intensity_threshold) (geom.py:907-908).
 *   With mask as the only output (compute_uv_visiblity_face alone) everything but face_index_uv and face_vis may be NULL.
 *   Outputs, any subset (NULL = not wanted; total and cnt go together):
 *     tex[B,3,S_h,S_w], mask[B,1,S_h,S_w] bytes 0 / 1 (= vis): every element written;
 *     total[3,S_h,S_w] += sum_b tex_b and cnt[S_h,S_w] += sum_b vis_b: the sums are formed in view order starting from
 *     the value found in the accumulator -- bit-identical to B successive `tex_total += tex; tex_cnt += mask`
 *     (run_gen_texmean.py:102-103).
 *   STATED: only the face index image decides visibility: a sample behind the camera (p.z < 0) is taken like any other
 *   (the reference has no depth test).  p.z == 0 or a non-finite pixel coordinate gives the texel 0 for that view (the
 *   reference's result there is unspecified).  A texel that is not visible gives exactly 0 even where the image holds
 *   NaN (the reference: NaN * 0 = NaN).  The reference's normal_image / normal_threshold are unused there and have no
 *   counterpart here.
 * gol_texmean_finalize: out[S_h,S_w,3] = total / (cnt + eps) (run_gen_texmean.py:105-106); flip_rows != 0 mirrors the
 *   rows, bgr != 0 swaps the channels to BGR (:106-108, up to the cv2.imwrite).  Out of place.
 * ---------------------------------------------------------------------------------------- */
int gol_face_visibility(int B, int F, int H, int W, const int32_t* index_img, uint8_t* face_vis, void* stream);
int gol_view_texture(int B, int V, int F, int H, int W, int S_h, int S_w, const float* verts, int64_t verts_bstride,
                     const float* image, const float* K, const float* Rt, const int32_t* index_image_uv,
                     const float* bary_image_uv, const int32_t* face_index_uv, const uint8_t* face_vis,
                     int has_threshold, float intensity_threshold, float* tex, uint8_t* mask, float* total, float* cnt,
                     void* stream);
int gol_texmean_finalize(int S_h, int S_w, const float* total, const float* cnt, float eps, int flip_rows, int bgr,
                         float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * lbs: skeleton solve and linear blend skinning, forward and backward (csrc/lbs.hip).  Replaces the reference's per-frame
 * PyTorch of ca_code/utils/lbs.py as called by URHand (ca_code/models/urhand.py:767) and hand_mvp / hand_teacher_mvp
 * (ca_code/models/hand_mvp.py:390).  The constants are packed once by goliath_amd.lbs.Skeleton (int32 unless stated):
 *   parents[J] (-1 = root, a parent's index is smaller than its child's); level_start[L+1], level_joints[J]: the joints
 *   by tree level; child_start[J+1], child_slot[]: joint -> children, ascending; bind_inv[J,8] (double): bt, br, bs of
 *   states_to_matrix (lbs.py:392-394); transform[7J,P] and its transpose transform_t[P,7J], transform_offsets[7J],
 *   P = NP + NS (lbs.py:39-46); joint_offset[J,3], joint_rotation[J,4] (xyzw); skin_indices, skin_weights [V,K];
 *   jv_slot[E]: the (vertex, slot) pairs with a non-zero weight grouped by joint, slot = vertex * K + k, ascending per
 *   joint; item_start[I+1]: every joint's run cut into items of at most 64 entries; ji_start[J+1]: a joint's items.
 * gol_lbs_skeleton_fwd: poses[B,NP] and scales (row b at scales + b * scales_stride; stride 0 = one row for all views)
 *   -> states[B,J,8] (translation, rotation xyzw, scale: solve_skeleton_state, lbs.py:340-385, with Quaternion.batchFromXYZ's
 *   half angles, quaternion.py:285-320) and mats[B,J,3,4] = states_to_matrix(bind_state, states) (lbs.py:388-429).  Either
 *   output may be NULL.  One workgroup per view, the arithmetic in double.
 * gol_lbs_skeleton_bwd: g_states, g_mats (either may be NULL = zero) -> g_poses[B,NP], g_scales[B,NS] (either may be
 *   NULL), every element written.
 * gol_lbs_skin_fwd: out[B,V,3] = (sum_k w_k mats[idx_k] [x,1]) * global_scaling with x = verts + template_verts
 *   (skinning, lbs.py:226-254, between the two lines of LBSModule.pose, lbs.py:725-731).  verts is [B,V,3], or [V,3]
 *   shared by the views with verts_batched = 0 (lbs.py:331-334); template_verts[V,3] and global_scaling[3] may be NULL.
 *   A slot of weight 0 contributes nothing, whatever its index.
 * gol_lbs_skin_bwd: g_out[B,V,3] -> g_verts[B,V,3] (the gradient of x) and g_mats[B,J,3,4], every element written; either
 *   may be NULL; item_sums[B,I,12] (double) is scratch.
 * No atomics: every sum has a fixed order and all outputs are bitwise reproducible.  No host sync, no allocation.
 * ---------------------------------------------------------------------------------------- */
int gol_lbs_skeleton_fwd(int B, int J, int NP, int NS, int L, const float* poses, const float* scales, int scales_stride,
                         const float* transform_t, const float* transform_offsets, const float* joint_offset,
                         const float* joint_rotation, const double* bind_inv, const int32_t* parents,
                         const int32_t* level_start, const int32_t* level_joints, float* states, float* mats,
                         void* stream);
int gol_lbs_skeleton_bwd(int B, int J, int NP, int NS, int L, const float* poses, const float* scales, int scales_stride,
                         const float* transform, const float* transform_t, const float* transform_offsets,
                         const float* joint_offset, const float* joint_rotation, const double* bind_inv,
                         const int32_t* parents, const int32_t* level_start, const int32_t* level_joints,
                         const int32_t* child_start, const int32_t* child_slot, const float* g_states,
                         const float* g_mats, float* g_poses, float* g_scales, void* stream);
int gol_lbs_skin_fwd(int B, int V, int J, int K, const float* mats, const float* verts, int verts_batched,
                     const float* template_verts, const float* global_scaling, const int32_t* skin_indices,
                     const float* skin_weights, float* out, void* stream);
int gol_lbs_skin_bwd(int B, int V, int J, int K, int E, int I, const float* mats, const float* verts, int verts_batched,
                     const float* template_verts, const float* global_scaling, const int32_t* skin_indices,
                     const float* skin_weights, const int32_t* item_start, const int32_t* jv_slot,
                     const int32_t* ji_start, const float* g_out, double* item_sums, float* g_verts, float* g_mats,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * optim: gradient scrub, global-norm clip and the Adam / AdamW step over all parameter tensors (csrc/optim.hip).
 * Replaces the tail of the reference's training iteration, ca_code/utils/train.py:209-215: the two boolean-mask writes per
 * parameter tensor (`p.grad.data[isnan(..)] = 0`, `[isinf(..)] = 0`: a host sync each), `clip_grad_norm_(params, 1.0)` and
 * `optimizer.step()` of torch.optim.Adam / AdamW -- four passes over the gradients and a sync per tensor -- by one read of
 * the gradients (grad_stats + finalize) and one pass over p, g, exp_avg, exp_avg_sq (adam_step).
 * A SEGMENT is one float32 parameter tensor that has a gradient, described by device arrays of length n_seg: seg_p, seg_g,
 *   seg_m, seg_v, seg_step hold 64-bit device addresses (of the parameter, its gradient, exp_avg, exp_avg_sq, all
 *   contiguous float32 of seg_numel elements, and of the tensor's float32 step counter); seg_group is the row of `groups`.
 * A CHUNK c is elements [chunk_off[c], chunk_off[c] + gol_optim_chunk_elems()) of segment chunk_seg[c], cut at the
 *   segment's end; the chunks tile every segment once.  One workgroup per chunk.  16-byte accesses where a segment's
 *   pointers are 16-byte aligned, scalar ones otherwise.
 * groups[n_groups, GOL_OPTIM_GROUP_DOUBLES] (double): lr, beta1, beta2, eps, weight_decay, decoupled (0 = L2 decay added
 *   to the gradient, torch.optim.Adam; 1 = p *= 1 - lr * weight_decay, AdamW), two spare.
 * gol_optim_chunk_elems: the compile-time chunk size, in elements.
 * gol_optim_grad_stats: partial[c] = (sum of g^2 over the chunk's FINITE entries, number of non-finite entries), both double
 *   (train.py:209-211: a non-finite entry is 0 to the norm).
 * gol_optim_finalize: sums the partials in index order in double (one workgroup) -> stats[0] = total_norm, stats[1] =
 *   clip_coef = min(1, max_norm / (total_norm + 1e-6)) (clip_grad_norm_'s rule, train.py:212), nonfinite[0] = the count.
 *   max_norm = +inf: no clipping (clip_coef = 1).
 * gol_optim_adam_step: first, per segment, step += 1 on the device and the step's constants into seg_coef[n_seg,8]
 *   (scratch); then per element g = isfinite(g) ? g : 0 (GOL_OPTIM_SCRUB), g *= stats[1] (GOL_OPTIM_CLIP), the cleaned g
 *   stored (GOL_OPTIM_WRITE_BACK: the post-state of train.py:209-212), and torch's single-tensor Adam in its operation
 *   order (train.py:215).  stats may be NULL without GOL_OPTIM_CLIP.  Any other flag (amsgrad, maximize, steps kept on
 *   the host) returns GOL_ERR_UNSUPPORTED.
 * No float atomics: bitwise reproducible.  No host sync, no allocation: a whole step captures as a graph.
 * ---------------------------------------------------------------------------------------- */
#define GOL_OPTIM_GROUP_DOUBLES 8
#define GOL_OPTIM_SCRUB 1
#define GOL_OPTIM_CLIP 2
#define GOL_OPTIM_WRITE_BACK 4
int gol_optim_chunk_elems(void);
int gol_optim_grad_stats(int n_chunks, int n_seg, const int32_t* chunk_seg, const int64_t* chunk_off, const int64_t* seg_g,
                         const int64_t* seg_numel, double* partial, void* stream);
int gol_optim_finalize(int n_chunks, const double* partial, double max_norm, double* stats, int64_t* nonfinite,
                       void* stream);
int gol_optim_adam_step(int n_chunks, int n_seg, int n_groups, const int32_t* chunk_seg, const int64_t* chunk_off,
                        const int64_t* seg_p, const int64_t* seg_g, const int64_t* seg_m, const int64_t* seg_v,
                        const int64_t* seg_step, const int64_t* seg_numel, const int32_t* seg_group, const double* groups,
                        const double* stats, float* seg_coef, int flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * regloss: the per-Gaussian regularisers of the training loss (csrc/regloss.hip).  Each replaces a chain of ATen
 * launches over a [B,N,3] tensor by one read pass forward and one read + one write pass backward.
 * A CHUNK is gol_regloss_chunk_elems() consecutive elements (flat penalties) or a quarter as many rows (backlit); one
 * workgroup per chunk, 16-byte accesses on full chunks of 16-byte aligned tensors, scalar ones otherwise.
 * gol_regloss_fwd: partial[cdiv(n, chunk)] (double) = per-chunk sums of f(x[i]); the caller forms sum(partial) / n.
 * gol_regloss_bwd: g_x[i] = g_scale[0] * f'(x[i]) for every i; g_scale is a DEVICE scalar (upstream gradient / n).
 *   kind                    f(x)                                                     replaces ca_code/loss/__init__.py
 *   GOL_REGLOSS_BOUND       x < p0 ? 1 / max(x, 1e-7) : (x > p1 ? (x - p1)^2 : 0)    :560-573 bound_primscale (p0 = min_scale,
 *                           f' = x < p0 ? (x >= 1e-7 ? -1/x^2 : 0) : (x > p1 ? 2 (x - p1) : 0)              p1 = max_scale)
 *   GOL_REGLOSS_NEG_SQ      min(x, 0)^2,  f' = 2 min(x, 0)                           :576-578 negcolor
 *   GOL_REGLOSS_SQ          x^2,  f' = 2 x                                           :581-583 l2_reg
 *   GOL_REGLOSS_ABS         |x|,  f' = sign(x), 0 at 0                               :585-590 list_l1_reg (one call per term)
 *   GOL_REGLOSS_ALPHAPRIOR  log(0.1 + x) + log(1.1 - x) + 2.20727                    :609-622 alphaprior
 *                           f' = 1 / (0.1 + x) - 1 / (1.1 - x)
 *   (p0, p1 are read by GOL_REGLOSS_BOUND only.)  float32 arithmetic in torch's operation order, IEEE division, accurate
 *   logf; only finite inputs are specified.
 * gol_backlit_fwd / _bwd: ca_code/loss/__init__.py:592-600 backlit_reg.  color[m,c], cosw[m]; w = max(-cosw, 0)^2.
 *   fwd: partial[cdiv(m, chunk / 4), 2] (double) = per-chunk (sum_c w * max(color, 0), sum w) -- a row's w counts ONCE; the
 *   caller forms num / (1 + den).  bwd: g_color[r,j] = g_scale[0] * w[r] * (color[r,j] > 0), g_scale = upstream / (1 + den)
 *   on the device.  cosw receives no gradient.  Any c >= 1; c == 3 is the 16-byte path (a lane owns four rows).
 * An unknown kind, a negative count or a null pointer with a positive count returns GOL_ERR_INVALID_ARG; a count of 0
 * returns GOL_OK without a launch.  Fixed-order sums in double, no float atomics: bitwise reproducible.  No host sync, no
 * allocation: captures as a linear graph.
 * ---------------------------------------------------------------------------------------- */
typedef enum {
  GOL_REGLOSS_BOUND = 0,
  GOL_REGLOSS_NEG_SQ = 1,
  GOL_REGLOSS_SQ = 2,
  GOL_REGLOSS_ABS = 3,
  GOL_REGLOSS_ALPHAPRIOR = 4
} gol_regloss_kind;
int gol_regloss_chunk_elems(void);
int gol_regloss_fwd(int kind, int64_t n, float p0, float p1, const float* x, double* partial, void* stream);
int gol_regloss_bwd(int kind, int64_t n, float p0, float p1, const float* x, const float* g_scale, float* g_x,
                    void* stream);
int gol_backlit_fwd(int64_t m, int c, const float* color, const float* cosw, double* partial, void* stream);
int gol_backlit_bwd(int64_t m, int c, const float* color, const float* cosw, const float* g_scale, float* g_color,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * imgfam: the image-sized work around the L2 / focus image losses (csrc/imgfam.hip).  Each entry replaces a chain of ATen
 * launches over full images by one read pass (and, where something is produced, one write pass).
 * gol_imgloss_fwd / _bwd / _finalize: a masked elementwise penalty over pred, target [B,C,HW] (float32).
 *   residual x = (pred - target) * m, m = mask * (1 - veto): mask float32 [B,1,HW] (mask_c = 1) or [B,C,HW] (mask_c = C) or
 *   NULL (factor 1, mask_c unread); veto bytes [B,1,HW] or NULL (factor 1) -- the storage of a torch.bool depth_disc_mask,
 *   a non-zero byte vetoes the pixel.  With a = |x| and g = g_scale[0]:
 *   kind               loss per element     gradient w.r.t. pred                  replaces ca_code/loss/__init__.py
 *   GOL_IMGLOSS_ABS    a                    sign(x) m g, 0 at 0                   :391-411 rgb_l1's chain
 *   GOL_IMGLOSS_SQ     x x                  (g (2 x)) m                           :366-386 rgb_l2, :415-445 psnr,
 *                                                                                 :555-557 pose_shadow_l2
 *   GOL_IMGLOSS_EXPW   a expf(a / 255.f)    (g expf(a / 255.f)) sign(x) m         :496-517 rgb_l1_focus, :519-538 rgb_l1_phys
 *                                           (the weight is detached there: it has no derivative)
 *   A CHUNK is gol_imgloss_chunk_elems() consecutive floats of one (b,c) plane, one workgroup each: 16-byte accesses on full
 *   chunks of 16-byte aligned planes, scalar ones with the same elements per lane otherwise (the same bits either way).
 *   fwd: partial[B*C * cdiv(HW, chunk)] (double) = the chunk sums, plane-major.
 *   finalize: one workgroup adds partial[0 .. n_chunks) in a fixed order in double: loss[0] = (float)(sum / n), sum[0] = sum.
 *   bwd: g_pred[B,C,HW] written in full; g_scale is a DEVICE scalar (upstream gradient / n).
 *   float32 arithmetic in torch's operation order without contraction, IEEE division, accurate expf; only finite inputs are
 *   specified.  B*C <= 65535.  An unknown kind, a mask_c that is neither 1 nor C, or a null pointer with positive sizes
 *   returns GOL_ERR_INVALID_ARG; B == 0 or HW == 0 returns GOL_OK without a launch.
 * gol_depth_disc_mask: ca_code/utils/geom.py:768-794 depth_discontuity_mask.  depth [B,H,W] float32 -> out [B,H,W] bytes
 *   (0 / 1): the two 3x3 Sobel kernels with zero padding, a centre fires when sqrtf(gx gx + gy gy) > threshold, and an
 *   output pixel is set when any in-image centre of its pool x pool window fires (avg_pool2d with zero padding > 0).
 *   pool 1, 3 or 5 (the reference's default is 3), else GOL_ERR_UNSUPPORTED.  (The reference's kscale is unused there.)
 * gol_mask_erode: ca_code/utils/image.py:393-422 erode.  x [B,H,W], float32 (x_is_u8 = 0) or bytes (x_is_u8 = 1: the
 *   storage of a torch.bool) -> out [B,H,W] float32 0 / 1: 1 iff no in-image pixel of the ks x ks window has 1 - x > 0
 *   (bytes: is 0); pixels outside the image do not veto (the zero-padded complement).  DEFINED FOR x IN [0,1]: the
 *   reference sums 1 - x over the window, which a value above 1 could cancel.  ks odd in 1 .. 31, else GOL_ERR_UNSUPPORTED.
 * Both mask operators: one workgroup per 64 x 16 output tile, tile + halo staged in LDS; B <= 65535.
 * Fixed-order sums in double, no atomics: bitwise reproducible.  No host sync, no allocation: captures as a linear graph.
 * ---------------------------------------------------------------------------------------- */
typedef enum {
  GOL_IMGLOSS_ABS = 0,
  GOL_IMGLOSS_SQ = 1,
  GOL_IMGLOSS_EXPW = 2
} gol_imgloss_kind;
int gol_imgloss_chunk_elems(void);
int gol_imgloss_fwd(int kind, int B, int C, int HW, int mask_c, const float* pred, const float* target, const float* mask,
                    const uint8_t* veto, double* partial, void* stream);
int gol_imgloss_finalize(int64_t n_chunks, int64_t n, const double* partial, float* loss, double* sum, void* stream);
int gol_imgloss_bwd(int kind, int B, int C, int HW, int mask_c, const float* pred, const float* target, const float* mask,
                    const uint8_t* veto, const float* g_scale, float* g_pred, void* stream);
int gol_depth_disc_mask(int B, int H, int W, int pool, float threshold, const float* depth, uint8_t* out, void* stream);
int gol_mask_erode(int B, int H, int W, int ks, int x_is_u8, const void* x, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Environment background of the relight visualisation, forward only (csrc/envbg.hip).  Replaces
 * ca_code/utils/envmap.py:325-345 compose_envmap with what it calls, as run_vis_relight.py:110-122 reaches it through
 * ca_code/models/rgca.py:232-245.  envbg[B,3,He,We] is the equirectangular map, K[B,3,3] the intrinsics, R[B,3,3] the
 * camera rotation Rt[:, :3, :3]; all images are planar [B,3,H,W] float32.
 * gol_envbg_image: envmap.py:169-227 envmap_to_image for D = None.  Per pixel d = ((x - K02) / (K00 focal_scale),
 *   (y - K12) / (K11 focal_scale), 1), d' = R^T d (out_y = sum_x R[x][y] d[x]) normalised with F.normalize's eps 1e-12,
 *   u = atan2(d'x, d'z) / pi, v = 2 acos(d'y) / pi - 1 (evaluated in double; acos' argument clamped to [-1, 1]), then
 *   grid_sample(mode='bicubic', padding_mode='border', align_corners=True): A = -0.75, ix = (u + 1) / 2 (We - 1) unclipped,
 *   each of the 4 x 4 tap indices clamped to the map.  blur = 1 (the reference's blurbg=True): the 101 x 101 kernel
 *   exp(-t_i^2) exp(-t_j^2) / sum, t = linspace(-4, 4, 101), conv2d(padding=50) ZERO padding, applied as a row pass and a
 *   column pass with the weights of gol_envbg_blur_taps (computed on the host in double, handed to the kernels as 101
 *   floats); the reference's trailing interpolate(size=(h, w)) is the identity.  blur = 0: one launch, scratch may be NULL;
 *   blur = 1: three launches, scratch = gol_envbg_scratch_floats(B,H,W) floats (two [B,3,H,W] planes).  bg is not clamped.
 * gol_envbg_compose: the rest of compose_envmap in one pass: out = render + (1 - alpha) clamp(bg, 0, 1), alpha[B,1,H,W];
 *   then, in the bottom-right ball x ball pixels (the reference: 200), envmap.py:230-248 envmap_to_mirrorball in place:
 *   p = linspace(-1, 1, ball) both ways, zsq = px^2 + py^2, inside zsq < 1: nz = -sqrt(1 - zsq), ref = -2 nz (px, py, nz)
 *   + (0, 0, 1), rotated by R^T, NOT normalised, the same u / v and an unblurred, unclamped bicubic lookup of envbg
 *   replaces the pixel.  ball = 0: no ball (envbg / R may be NULL).  ball > H or ball > W: GOL_ERR_INVALID_ARG.
 *   out must not overlap an input.
 * B * 3 <= 65535, H * W < 2^31.  No host sync, no allocation, no atomics: bitwise reproducible, captures as a linear graph.
 * ---------------------------------------------------------------------------------------- */
int gol_envbg_blur_taps(double* taps /* [101] */);
int64_t gol_envbg_scratch_floats(int B, int H, int W);
int gol_envbg_image(int B, int H, int W, int He, int We, const float* envbg, const float* K, const float* R,
                    double focal_scale, int blur, float* scratch, float* bg, void* stream);
int gol_envbg_compose(int B, int H, int W, int He, int We, const float* render, const float* alpha, const float* bg,
                      const float* envbg, const float* R, int ball, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Light transform and SH light coefficients of a frame, forward only (csrc/lightsh.hip).  Replaces
 * ca_code/models/rgca.py:175-191 (AutoEncoder.forward: headrel_light_pos, headrel_light_sh) and :590-613 (PrimDecoder.forward's
 * random back-light) with what they call, ca_code/utils/sh.py:118-127 dir2sh_torch (81 functions evaluated one at a time,
 * each with a device-to-host sync at sh.py:55).  Coefficient order: n = 0..deg outer, m = -n..n inner, index n*n + n + m;
 * deg is 0 ... 8.  The reference's semantics (sh.py:54-103): the Legendre argument is clamp(z, -1, 1), sin(theta) =
 * sqrt(max((1 + x)(1 - x), 1e-8)), phi = atan2(y, x) of the raw components (atan2(0, 0) = 0); Y = N cos(m phi) P_n^m for
 * m > 0, N sin(|m| phi) P_n^|m| for m < 0, N P_n^0 for m = 0, with P by the upward recurrences of sh.py:58-78.
 * gol_sh_norm_constants: host code, no GPU.  The (deg+1)^2 constants N in float64: KVal(|m|, n) = sqrt((2n + 1) / (4 pi)
 *   (n - |m|)! / (n + |m|)!) (sh.py:13-26), times sqrt(2) for m != 0 (sh.py:80-86).  The kernels use these rounded to float32.
 * gol_sh_basis_fwd: dirs[M,3] -> coeffs[M,(deg+1)^2] = dir2sh_torch(deg, dirs); dirs are NOT normalised (as there).
 * gol_light_sh_fwd: light_pos[B,L,3], light_intensity[B,L,intensity_channels] (1 = the reference's .expand(-1, -1, 3), or
 *   3), head_pose[B,3,4] = [R | t] (NULL = identity).  headrel_light_pos[B,L,3] = (p - t) @ R (NULL = not wanted);
 *   light_sh[B,3,(deg+1)^2][b,c,k] = sum_l Y_k(d_l) I[b,l,c] with d_l = F.normalize(headrel_light_pos[b,l]) =
 *   v / max(|v|, 1e-12) (a zero vector stays zero).  The sum runs in light order into one accumulator per output through
 *   LDS: a light of zero intensity (the dataloader's padding) contributes exactly nothing.
 * Every output is finite for finite input.  One launch each, no host sync, no allocation, no atomics: bitwise
 * reproducible, graph-capturable.  M * 81 < 2^31, B * L * 3 < 2^31.
 * ---------------------------------------------------------------------------------------- */
int gol_sh_norm_constants(int deg, double* out /* [(deg+1)^2] */);
int gol_sh_basis_fwd(int M, int deg, const float* dirs, float* coeffs, void* stream);
int gol_light_sh_fwd(int B, int L, int deg, const float* light_pos, const float* light_intensity, int intensity_channels,
                     const float* head_pose, float* headrel_light_pos, float* light_sh, void* stream);

/* ------------------------------------------------------------------------------------------
 * The per-frame work of the env-relight driver, forward only (csrc/envdriver.hip).  Replaces
 * ca_code/utils/light_decorator.py:120-143 (EnvSpinDecorator.forward, per view) with what it calls,
 * ca_code/utils/envmap.py:141-166 rotate_envmap_mat: a CPU grid_sample of the whole map, a percentile of it, an antialiased
 * CPU interpolate to the 16 x 32 light probe and a 6 MB upload per view.  At most three launches per call, any B.
 * gol_envspin_frame parameters:
 *   B, H, W          views (light_decorator.py:109 batch_size) and the size of the map (:58: 512 x 1024); H >= 16, W >= 32,
 *                    W even (envmap.py:149 arange(-W//2, W//2)), else GOL_ERR_INVALID_ARG
 *   image[3,H,W]     self.image (:61-62), the unrotated map, on the device
 *   rot[B,9]         rot_mat (:119) of every view, row-major
 *   tap_y_start[16], tap_y_w[16,ky], tap_x_start[32], tap_x_w[32,kx]
 *                    thf.interpolate(new_env[None], (16, 32), mode="bilinear", antialias=True) (:128-130) as two 1-D tables:
 *                    per output row (column) the first source row (column) with a non-zero weight and its ky (kx) weights
 *                    from there on, padded with zeros, in double; probe[c,i,j] = sum wy[i][a] wx[j][b] new_env[c, ys_i + a,
 *                    xs_j + b].  Source indices are clamped to the map by the kernel.
 *   perc90           np.percentile(self.image, 90) (:123), > 0
 *   env_scale        self.env_scale (:138-139)
 *   scratch          gol_envspin_scratch_floats(B,H,W) floats, 8-byte aligned (16 for the vector stores)
 *   envbg[B,3,H,W]   ((new_env / perc90) * 255) / 255 (:124-126, :159), each operation rounded to float32; NULL = not wanted
 *   envmap[B,3,16,32]          env_scale probe / S_b, S_b = sum probe sin((i + 0.5) pi / 16) (:132-141)
 *   light_intensity[B,512,3]   the same values, new_env.view(3, -1).t() (:143)
 *   norm_scale[B]              env_scale / S_b (:139)
 *   mip_scale[1]               2 pi env_scale / S_0 = 2 pi norm_scale[0], the `scale` of self.mipmap (:151-153), formed in
 *                              double and rounded once (the reference multiplies two float32 numbers: up to an ulp more error);
 *                              what gol_shade_in.mips_scale_dev points at
 * new_env is envmap.py:147-164 as written: theta = (y + 0.5) 3.1415926 / H, phi = (x - W/2 + 0.5) 3.1415926 2 / W,
 * vec = (sin theta sin phi, cos theta, sin theta cos phi), d = rot vec (:154-155 matmul(vec, rot_mat.T)), clamped to
 * [-1, 1], u = atan2(dx, dz) / pi, v = 2 acos(dy) / pi - 1, grid_sample(bilinear, align_corners=False,
 * padding_mode="border"): ix = ((u + 1) W - 1) / 2 clipped to [0, W - 1] (the u = +-1 seam clamps, it does not wrap).
 * Angles, position and blend are evaluated in double and rounded once; the probe and S_b are double sums over the float32
 * new_env in a fixed order.  No host sync, no allocation, no atomics: two calls are bitwise equal, view b of a batch equals
 * the same view alone, and the call captures as a graph of one linear chain.
 * ---------------------------------------------------------------------------------------- */
int64_t gol_envspin_scratch_floats(int B, int H, int W);
int gol_envspin_frame(int B, int H, int W, const float* image, const float* rot, const int32_t* tap_y_start,
                      const double* tap_y_w, int ky, const int32_t* tap_x_start, const double* tap_x_w, int kx,
                      float perc90, double env_scale, float* scratch, float* envbg, float* envmap, float* light_intensity,
                      float* norm_scale, float* mip_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Primitive assembly of the MVP hand model (csrc/mvpprims.hip): what hand_mvp.AutoEncoder does between its decoders and
 * the ray march.
 * gol_mvp_template_fwd / _bwd replace ca_code/models/hand_mvp.py:171-185 (cat, view, permute(0,3,5,1,4,6,2), reshape of
 *   the texture slabs) together with the valid_prims selection of ca_code/utils/render_raymarcher.py:41-47
 *   (template[:, valid_prims].contiguous(), a nonzero with a host sync) and, for the teacher, the alpha-only rearrangement
 *   and valid_prims * primalpha masking of ca_code/models/hand_teacher_mvp.py:305-311.
 *     rgb[B,TD,3,Sy,Sx] (NULL: one-channel template) alpha[B,TD,1,Sy,Sx]   Sy = ny TH, Sx = nx TW, K = ny nx; only 4-byte
 *                                                                          alignment is asked of them
 *     out[B,Kout,TD,TH,TW,C], C = 4 (rgb + alpha) or 1 (rgb == NULL), 16-byte aligned:
 *       out[b, slot[k], z, y, x, c] = slab_c[b, z, py TH + y, px TW + x],  k = py nx + px
 *     slot[K] int32: the primitive's index in `out`, or -1 (outside 0 .. Kout-1) for not written; NULL = identity (then
 *       Kout == K).  Every index 0 .. Kout-1 must occur once, or `out` keeps unwritten primitives.
 *     live[K] int32, NULL = all 1: 0 writes zeros into the slot instead of data (the input is then not read).
 *     out_full[B,K,TD,TH,TW,C], NULL = not wanted: identity slots, all data, from the same loads (preds["primrgba"]).
 *     act != 0 fuses relu(rgb_scale x + rgb_shift) on the colour planes (hand_mvp.py:472: 25 x + 100) and relu(x) on alpha
 *       (:434); the product and the sum are rounded separately (PyTorch's composition bit for bit, no FMA: near the
 *       kink 25 x cancels against 100).  act == 0 is a pure move.
 *   The input of a primitive that is dropped (slot -1, no out_full) is not read.  _bwd is the transpose: g_out / g_out_full
 *   (either may be NULL = zero) -> g_rgb (NULL for one channel) and g_alpha, written COMPLETELY (zeros for dropped and dead
 *   primitives; no zero-filled allocation needed); with act the relu mask is recomputed from rgb / alpha, which may be NULL
 *   otherwise.  No atomics, no LDS, bitwise repeatable; all offsets 64-bit; Sy Sx < 2^31, B <= 65535.
 * gol_mvp_primtransf_fwd / _bwd replace hand_mvp.py:410-425 with axisangle_to_matrix (:477-510), one lane per primitive:
 *     primpos = posbase + rotbase delta_pos, primrot = rotbase A(delta_rvec), primscale = prim_scale delta_scale, with A as
 *     written there: theta = sqrt(1e-5 + |r|^2), n = r / theta (not unit length), diagonal n_i^2 + (1 - n_i^2) cos theta,
 *     off-diagonal n_i n_j (1 - cos theta) -+ n_k sin theta.  posbase[B,K,3] and rotbase[B,K,3,3] carry no gradient
 *     (no_grad in the reference); _bwd gives the three delta gradients analytically (NULL upstream gradient = zero) and is
 *     finite at delta_rvec = 0.  B K 9 < 2^31.
 * ---------------------------------------------------------------------------------------- */
int gol_mvp_template_fwd(int B, int TD, int TH, int TW, int ny, int nx, const float* rgb, const float* alpha,
                         const int32_t* slot, const int32_t* live, int Kout, int act, float rgb_scale, float rgb_shift,
                         float* out, float* out_full, void* stream);
int gol_mvp_template_bwd(int B, int TD, int TH, int TW, int ny, int nx, const float* rgb, const float* alpha,
                         const int32_t* slot, const int32_t* live, int Kout, int act, float rgb_scale, float rgb_shift,
                         const float* g_out, const float* g_out_full, float* g_rgb, float* g_alpha, void* stream);
int gol_mvp_primtransf_fwd(int B, int K, const float* posbase, const float* rotbase, const float* delta_pos,
                           const float* delta_rvec, const float* delta_scale, float prim_scale, float* primpos,
                           float* primrot, float* primscale, void* stream);
int gol_mvp_primtransf_bwd(int B, int K, const float* rotbase, const float* delta_rvec, float prim_scale,
                           const float* g_primpos, const float* g_primrot, const float* g_primscale, float* g_delta_pos,
                           float* g_delta_rvec, float* g_delta_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * The SG prefilter of an environment map, forward only (csrc/envprefilter.hip).  Replaces
 * ca_code/utils/envmap.py:305-323 prefilterEnvmapSG with what it calls per sample, :251-281 importance_sample_sg and
 * :284-302 dir2uv / sample_uv (two dozen ATen kernels, four boolean-mask writes and a grid_sample over the whole level per
 * sample; ca_code/utils/light_decorator.py:64-92 calls it with 4096 samples for each of the three prefiltered levels of the
 * relight pyramid).  Two launches per call: the repack of the map into 16-byte texels, then one wave per output texel.
 * gol_envprefilter_sg parameters:
 *   B, H, W          batch and the size of the direction grid = of the output
 *   He, We           the size of the map; independent of H, W.  All >= 1
 *   S                samples per texel (num_samples), >= 1
 *   sigma            the lobe width, > 0 and finite
 *   v[B,3,H,W]       the direction n of every output texel (used as given, not normalised: envmap.py:277-280)
 *   env_tex[B,3,He,We]   the map, planar
 *   xi[S,B,2,H,W]    the uniform draws, in the order the reference's rand_like(v[:, :2]) returns them in iteration i; or NULL:
 *                    a Philox-4x32-10 draw with key (seed low, seed high) and counter (g low, g high, y W + x, b),
 *                    g = sample_offset + i; outputs 0 and 1 of the block, each >> 8 and times 2^-24: [0, 1), never 1.
 *                    A draw depends on its key and counter only: S samples in one call see the draws of two calls of S / 2
 *                    with sample_offset 0 and S / 2
 *   seed, sample_offset   read only when xi is NULL; sample_offset >= 0
 *   scratch          gol_envprefilter_scratch_floats(B, He, We) floats, 16-byte aligned: the packed map [B,He,We,4]
 *   out[B,3,H,W]     (sum_i colour_i) / S
 * Per sample: phi = 2 pi Xi0, theta = sqrt2 sigma erfinv(Xi1 erf(pi / (sqrt2 sigma))), H = (cos phi sin theta,
 * sin phi sin theta, cos theta); up = (0,0,1) if n_z < 0.999 else (1,0,0), t = normalize(up x n), b = n x t,
 * d = normalize(t H_x + b H_y + n H_z) (normalize divides by max(norm, 1e-12)); u = atan2(d_x, d_z) / pi,
 * v = 2 acos(d_y) / pi - 1; grid_sample(bilinear, align_corners=False, padding_mode="border"): ix = ((u + 1) We - 1) / 2
 * clipped to [0, We - 1] (the u = +-1 seam clamps, it does not wrap).  The pdf the reference computes and drops is not
 * computed.  One deviation: d_y is clamped to [-1, 1] before acos (the reference gives NaN when normalize lands an ulp
 * outside).  The frame (t, b) is formed once per texel and erf(pi / (sqrt2 sigma)) once per call, on the host.  Everything
 * is evaluated in double from the float32 inputs and the mean is rounded once.  Lane l of a texel's wave adds the samples
 * l, l + 64, ... in ascending order, the 64 partial sums go through one fixed ladder: no atomics, two calls are bitwise
 * equal, and nothing depends on the grid.  No host sync, no allocation.  B H W < 2^31, 4 B He We < 2^31.
 * ---------------------------------------------------------------------------------------- */
int64_t gol_envprefilter_scratch_floats(int B, int He, int We);
int gol_envprefilter_sg(int B, int H, int W, int He, int We, int S, double sigma, const float* v, const float* env_tex,
                        const float* xi, int64_t seed, int64_t sample_offset, float* scratch, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * olat: the MVP teacher's per-light work around its UNet (csrc/olat.hip), OLATRGBDecoder.forward_rgb of
 * ca_code/models/hand_teacher_mvp.py.  Primitives are X x Y x Z voxels (primsize), npy x npx of them tile the UV map
 * [Sy,Sx] = [npy Y, npx X]: texel (h Y + y, w X + x) belongs to primitive k = h npx + w, K = npy npx.
 * shadow[B L,K,Z,Y,X] is what gol_mvp_shadow_march's caller returns (value / (weight + 1e-5)), in the march's own layout.
 * gol_olat_features_fwd replaces :371-439, the UNet input x[B L,7 Z,Sy,Sx] (forward only: the reference runs these lines
 *   under no_grad).  primpos[B,K,3], primrot[B,K,3,3], primscale[B,K,3], valid_prims[K] (float 0 / 1), light_pos[B,L,3],
 *   campos[B,3]; lin_x[X], lin_y[Y], lin_z[Z] = torch.linspace(-1, 1, .) as device arrays.  Per texel and z:
 *     local = (lin_z[i % Z], lin_y[(i / Z) % Y], lin_x[i / (Y Z)]) with i = (z Y + y) X + x -- the reference's
 *       meshgrid([lz, ly, lx]).transpose(1, 3).reshape(3, -1) viewed as [Z,Y,X] (:379-400), AS WRITTEN: for a primitive
 *       that is not a cube this is not the voxel's own coordinate, and shipped checkpoints were trained with it;
 *     p = volradius (primpos + R (local / primscale)),  d = (src - p) / max(|src - p|, 1e-12),  out_f = valid sum_e R[e][f] d_e
 *   channel 3 z + f: src = light_pos[b,l]; channel 3 Z + 3 z + f: src = campos[b], the same for every light of a frame;
 *   channel 6 Z + z: 1 - shadow[bl,k,z,y,x] (not masked, as there).  A primitive with valid == 0 gets exact zeros in
 *   channels [0, 6 Z) whatever its transform holds; where src == p the direction is the zero vector.
 * gol_olat_combine_fwd / _bwd replace :468-488.  tex[B L,4 Z,Sy,Sx] viewed [B,L,Z,4,Sy,Sx]; light_intensity[B,L,3].
 *     s = use_shadow ? shadow : 1 / (1 + exp(-tex_0)),  texolat_c = 25 tex_{1+c} + 100 (product and sum rounded separately),
 *     rgb[B,Z,3,Sy,Sx] = sum_l (s relu(texolat_c)) I[b,l,c] in light order,  primshadow[B,Z,3,Sy,Sx] = (sum_l shadow) / L in
 *     all three channels, dense;  texolat[B,L,Z,3,Sy,Sx] is written when non-NULL (training).
 *   _bwd: g_rgb[B,Z,3,Sy,Sx] and g_texolat (NULL = absent) -> g_tex, every element written:
 *     g_tex_0 = s (1 - s) sum_c g_rgb_c relu(texolat_c) I_c, exactly 0 with use_shadow;
 *     g_tex_{1+c} = 25 (g_texolat_c + [texolat_c > 0] s I_c g_rgb_c): the relu passes nothing at exactly 0, as torch's.
 *   Everything is recomputed from tex; shadow is read only with use_shadow (NULL allowed otherwise).  No gradient to
 *   light_intensity or shadow.
 * A lane owns four consecutive texels of a row (16-byte accesses) when X % 4 == 0 and the maps are 16-byte aligned, one
 * otherwise; z and the lights are loops inside the lane.  No atomics, no scratch, no host sync: bitwise reproducible,
 * graph-capturable.  Sy Sx < 2^31, B L < 2^28, B <= 65535 (features), B Z <= 65535 (combine).
 * ---------------------------------------------------------------------------------------- */
int gol_olat_features_fwd(int B, int L, int X, int Y, int Z, int npx, int npy, const float* primpos,
                          const float* primrot, const float* primscale, const float* valid_prims,
                          const float* light_pos, const float* campos, const float* shadow, float volradius,
                          const float* lin_x, const float* lin_y, const float* lin_z, float* x, void* stream);
int gol_olat_combine_fwd(int B, int L, int X, int Y, int Z, int npx, int npy, int use_shadow, const float* tex,
                         const float* light_intensity, const float* shadow, float* rgb, float* texolat,
                         float* primshadow, void* stream);
int gol_olat_combine_bwd(int B, int L, int X, int Y, int Z, int npx, int npy, int use_shadow, const float* tex,
                         const float* light_intensity, const float* shadow, const float* g_rgb,
                         const float* g_texolat, float* g_tex, void* stream);

/* ------------------------------------------------------------------------------------------
 * mvptail: the last layer of the MVP hand model's two decoders written straight into the primitive template
 * (csrc/mvptail.hip).  Replaces, for both decoders of ca_code/models/hand_mvp.py, the closing
 * ConvTranspose2dWNUB(16 -> TD C, 4, 2, 1) with its untied bias (:338-340, :384, :455), relu(25 x + 100) (:472) / relu
 * (:434) and the template assembly of gol_mvp_template_fwd (:172-185, render_raymarcher.py:41-47): the [B,3TD,Sy,Sx] and
 * [B,TD,Sy,Sx] slabs are never written.  Sy = 2h = ny TH, Sx = 2w = nx TW, K = ny nx.
 *     x_rgb[B,16,h,w] (NULL: the one-channel template), w_rgb[16,3TD,4,4] (effective weight, ConvTranspose2d layout),
 *     bias_rgb[3TD,Sy,Sx]; x_alpha[B,16,h,w], w_alpha[16,TD,4,4], bias_alpha[TD,Sy,Sx];
 *     slot[K], live[K], Kout: as for gol_mvp_template_fwd (slot NULL = identity, then Kout == K; live NULL = all 1)
 *     pre_rgb[b,3z+c,Y,X] = sum_{ci,ky,kx} x_rgb[b,ci,iy,ix] w_rgb[ci,3z+c,ky,kx] + bias_rgb[3z+c,Y,X],  Y = 2 iy - 1 + ky,
 *       X = 2 ix - 1 + kx; pre_alpha the same
 *     out[b, slot[k], z, Y mod TH, X mod TW, c] = relu(rgb_scale pre_rgb + rgb_shift)  (c < 3),  relu(pre_alpha)  (c = 3),
 *       k = (Y div TH) nx + (X div TW); out[B,Kout,TD,TH,TW,4], 16-byte aligned, or [B,Kout,TD,TH,TW] with x_rgb == NULL
 *   The conv is exact fp32 (v_mfma_f32_16x16x4_f32), the bias is added to the finished sum, and the affine is rounded as
 *   PyTorch composes it: the product, then the sum (no FMA; near the kink 25 x cancels against 100), as gol_mvp_template_fwd
 *   does with act != 0.  A primitive with slot < 0 is not written and tiles that only reach such primitives are not computed;
 *   live == 0 writes zeros.  Every index 0 .. Kout-1 must occur once in slot, or `out` keeps unwritten primitives.
 * gol_mvp_tail_bwd: g_out and the saved out, both in template layout; C = 4 or 1 names the layout.
 *     g_pre = g_out [out > 0], times rgb_scale on the colours, zero for dropped and dead primitives
 *     g_x_rgb, g_x_alpha [B,16,h,w]; g_w_rgb[16,3TD,4,4], g_w_alpha[16,TD,4,4]; g_bias_rgb[3TD,Sy,Sx], g_bias_alpha[TD,Sy,Sx]:
 *       each written completely (zeros where nothing arrives), each may be NULL = not wanted
 *     w_rgb_t[3TD,4,4,16], w_alpha_t[TD,4,4,16]: the weights with the input channel last (needed for g_x_*)
 *     scratch: gol_mvp_tail_bwd_scratch_floats(B, h, w, TD, C) floats, needed for g_x_* and g_w_*
 *   Staged: one pass reads g_out / out with 16-byte loads, writes g_pre slab-shaped into scratch and sums it over the
 *   views, in view order, into the bias gradients; the input gradient is a gather, the weight gradient a split-K GEMM
 *   whose partial sums a second kernel adds in a fixed order.  No float atomics: two calls are bitwise equal.  g_out == NULL,
 *   B == 0 or Kout == 0 zero the outputs.
 * Supported: Ci = 16, 1 <= TD <= 10 (GOL_ERR_UNSUPPORTED otherwise); TH, TW >= 1 with ny TH = 2h, nx TW = 2w;
 * B, h <= 65535; (2h+2)(2w+2) < 2^25.  All offsets 64-bit.  No allocation, no host sync.
 * ---------------------------------------------------------------------------------------- */
int gol_mvp_tail_fwd(int B, int Ci, int h, int w, int TD, int TH, int TW, int ny, int nx, const float* x_rgb,
                     const float* w_rgb, const float* bias_rgb, const float* x_alpha, const float* w_alpha,
                     const float* bias_alpha, const int32_t* slot, const int32_t* live, int Kout, float rgb_scale,
                     float rgb_shift, float* out, void* stream);
long long gol_mvp_tail_bwd_scratch_floats(int B, int h, int w, int TD, int C);
int gol_mvp_tail_bwd(int B, int Ci, int h, int w, int TD, int TH, int TW, int ny, int nx, int C, const float* x_rgb,
                     const float* w_rgb_t, const float* x_alpha, const float* w_alpha_t, const int32_t* slot,
                     const int32_t* live, int Kout, float rgb_scale, const float* g_out, const float* out,
                     float* g_x_rgb, float* g_x_alpha, float* g_w_rgb, float* g_w_alpha, float* g_bias_rgb,
                     float* g_bias_alpha, float* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOLIATH_HIP_H */
