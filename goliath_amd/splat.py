"""Differentiable Gaussian-splat render path (host side) on top of the C ABI.

Three layers, all backed by libgoliath_hip.so (no CPU fallback):

  project_gaussians / rasterize_gaussians   gsplat-0.1.11-compatible operators, the signatures
        the reference calls at ca_code/utils/render_gsplat.py:49-63 and :65-104.
  render_views(...)                         the fused, batched, host-sync-free path: all B views
        of a batch in ONE launch sequence (project+count -> scan -> scatter -> per-tile sort ->
        colour+depth raster), replacing the Python view loop and its 4 `.item()` syncs per view
        (ca_code/models/rgca.py:119-138) and gsplat's `cum_tiles_hit[-1].item()`.

Host/device contract: Gaussian attributes are fp32 [B,N,.] tensors resident in HBM; intrinsics and
view matrices are read by the kernels from device memory.
"""
import ctypes
import math
import os

import torch

from . import _lib, views as _views
from ._lib import c_float, c_i64, c_int, fptr, ptr, stream_ptr

BLOCK = 16  # tile width; the reference's only value (render_gsplat.py:28)
GRAD_RECORD = 16  # include/goliath_hip.h: GOL_GRAD_RECORD
SPLAT_RECORD = 16  # include/goliath_hip.h: GOL_SPLAT_RECORD (the rasterizer's packed per-Gaussian record, 64 bytes)

def _tiles(img_h, img_w, block=BLOCK):
    return ((img_w + block - 1) // block) * ((img_h + block - 1) // block)


# --------------------------------------------------------------------------------------------
# Intersection-capacity planning (replaces gsplat's host sync on the intersection count).
# --------------------------------------------------------------------------------------------
class CapacityPlanner:
    """Per-shape capacity (max Gaussian/tile list slots per view) of the batched render path.

    mode "adaptive" (default): a call BLOCKS on its own counts only while that can matter -- the shape is new, or the
        last observed count came within 1.5x of the capacity.  Blocking means: the whole forward is launched at the
        planned capacity, then the host waits on an event recorded right after binning (the true counts land in a
        pre-allocated pinned buffer; the raster kernels are still queued behind the wait) and, if a view overflowed,
        binning + raster are re-run at a grown capacity INSIDE the same call, in stream order, before any consumer
        can read the image.  With 2x head-room in the plan the steady state of a training run never blocks: the counts
        are read back when their copy has landed (next call) and only move the plan.  Should the lists then still
        outgrow a 1.5x margin within ONE step, that step rendered with truncated lists (the deepest entries of the
        fullest tiles dropped): a CapacityWarning (a RuntimeWarning shown EVERY time, not once per call site) says so,
        `truncated` counts it, the capacity is raised, and every call of that shape BLOCKS on its own counts again until
        one checked call has passed (`force_block`) -- an eager loop running ahead of the GPU renders at most the steps
        that were already queued with the old capacity.  No exception reaches the caller
        (ca_code/utils/train.py:170-214 knows none of ours); GOLIATH_CAPACITY_MODE=verify never truncates at all.
    mode "verify": every call blocks and repairs in place (rounds 1-2 default): nothing is ever truncated, and an
        eager loop can never run ahead of the GPU (measured: 1.35 ms of host wait per 8-view step).
    mode "async": nothing waits; the counts are inspected at the NEXT call and an overflow raises
        (after growing the capacity) -- for benchmark loops that must not block the host.
    frozen: while a HIP graph is captured / replayed: no host copies; check_frozen() afterwards.
    Capacities only grow (a stale, smaller observation never shrinks them).
    """

    def __init__(self):
        self.capacity = {}
        self.mode = os.environ.get("GOLIATH_CAPACITY_MODE", "adaptive")
        self.pending = []        # deferred checks: (event, pinned counts, capacity, key)
        self.frozen = False      # True while a HIP graph is captured / replayed: no polling, no host copies
        self.frozen_log = []     # (n_isect tensor, capacity) of the calls made while frozen -> check_frozen()
        self.reruns = 0          # blocking calls whose forward had to be re-run at a grown capacity
        self.truncated = 0       # adaptive mode: steps found (after the fact) to have rendered with truncated lists
        self.last_worst = {}     # key -> most recent observed count
        self.force_block = set() # keys whose last deferred check found an overflow: blocking calls until one passes
        self._pinned = {}        # B -> free list of pinned int32[B] buffers (allocated once, recycled)

    def check_frozen(self):
        """After graph replays: did any captured render overflow the capacity it was captured with?"""
        for n_isect, capacity in self.frozen_log:
            worst = int(n_isect.max()) if n_isect.numel() else 0
            if worst > capacity:
                raise _lib.GoliathHipError(f"a captured render_views call overflowed its intersection capacity "
                                           f"({worst} > {capacity}): re-capture with a larger capacity")

    def must_block(self, key):
        """Does this call have to wait for its own counts?"""
        if self.mode == "verify" or os.environ.get("GOLIATH_STRICT_CAPACITY", "0") == "1":
            return True
        if self.mode == "async":
            return False
        seen, cap = self.last_worst.get(key), self.capacity.get(key)
        return key in self.force_block or seen is None or cap is None or seen * 1.5 > cap

    def passed(self, key):
        """A checked (blocking) call of this shape completed without truncation."""
        self.force_block.discard(key)

    def get(self, key):
        return self.capacity.get(key)

    def initial(self, N, T):
        return int(min(2**31 - 1, max(1 << 16, 16 * N + T)))

    def set(self, key, counts_max):
        """Plan for `counts_max` intersections per view with 2x head-room (lists grow from step to step during
        training); never shrinks an existing plan."""
        want = int(min(2**31 - 1, max(1 << 16, int(counts_max * 2.0) + 4096)))
        self.capacity[key] = max(self.capacity.get(key, 0), want)
        return self.capacity[key]

    def observe(self, key, worst, capacity):
        """Grow early, before it overflows."""
        self.last_worst[key] = worst
        if key not in self.capacity or worst * 1.5 > capacity:
            self.set(key, worst)

    def _take_pinned(self, B):
        free = self._pinned.setdefault(B, [])
        return free.pop() if free else torch.empty(B, dtype=torch.int32, pin_memory=True)

    def fetch(self, n_isect):
        """Blocking read of the per-view counts through a recycled pinned buffer: waits only for the work queued
        BEFORE this point of the current stream (binning), not for what the caller enqueued after it."""
        B = n_isect.numel()
        host = self._take_pinned(B)
        host.copy_(n_isect, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return host, ev

    def finish(self, host, ev):
        ev.synchronize()
        worst = int(host.max()) if host.numel() else 0
        self._pinned[host.numel()].append(host)
        return worst

    def note(self, key, n_isect, capacity):
        host, ev = self.fetch(n_isect)
        self.pending.append((ev, host, capacity, key))

    def poll(self, block=False):
        still, overflow = [], None
        for ev, host, capacity, key in self.pending:
            if block:
                ev.synchronize()
            if ev.query():
                worst = int(host.max()) if host.numel() else 0
                self._pinned[host.numel()].append(host)
                if worst > capacity:
                    self.last_worst[key] = worst
                    self.set(key, worst)
                    self.force_block.add(key)
                    overflow = (worst, capacity, key)
                else:
                    self.observe(key, worst, capacity)
            else:
                still.append((ev, host, capacity, key))
        self.pending = still
        if overflow is not None:
            worst, capacity, key = overflow
            msg = (f"a previous render_views call overflowed its intersection capacity ({worst} > {capacity}): its tile "
                   f"lists were truncated. Capacity was raised to {self.capacity[key]}")
            if self.mode == "async":
                raise _lib.GoliathHipError(msg + " -- re-run the step (GOLIATH_CAPACITY_MODE=verify repairs inside the "
                                                 "call instead).")
            import sys
            import warnings

            self.truncated += 1
            # shown on EVERY occurrence (a truncated step is a wrong step) without touching the process-wide filter list: the
            # per-location "already shown" registry is a fresh dict each time, so the user's own filters (-W error, ignore)
            # still decide what happens
            try:
                frame = sys._getframe(2)      # the caller of render_views (what stacklevel=3 pointed at)
            except ValueError:
                frame = sys._getframe(0)
            warnings.warn_explicit(msg + "; calls of this shape check their own counts before returning until one has passed "
                                         "(GOLIATH_CAPACITY_MODE=verify checks every call).", CapacityWarning,
                                   frame.f_code.co_filename, frame.f_lineno, module=frame.f_globals.get("__name__"), registry={})


class CapacityWarning(RuntimeWarning):
    """A render_views call was found, after the fact, to have rendered with truncated tile lists (adaptive mode)."""


PLANNER = CapacityPlanner()


class _Workspace:
    """Scratch + intermediate buffers of one forward call (kept alive by the autograd node)."""

    def __init__(self, B, N, T, capacity, device):
        self.capacity = capacity
        self.tile_count = torch.zeros(B, T, dtype=torch.int32, device=device)
        self.tile_bins = torch.empty(B, T, 2, dtype=torch.int32, device=device)
        self.keys = torch.empty(B, max(capacity, 1), dtype=torch.int64, device=device)
        self.sorted_ids = torch.empty(B, max(capacity, 1), dtype=torch.int32, device=device)
        self.n_isect = torch.empty(B, dtype=torch.int32, device=device)
        self.reach = torch.empty(B, max(N, 1), dtype=torch.int64, device=device)  # pass-1 -> pass-3 tile masks


# One marshaller per C-ABI entry called stage by stage: the header's positional order lives here only.  Keywords are the
# header's names (block = BLOCK, stream = the current one); a pointer is a GPU tensor (checked), a device address or None.
_F32, _I32, _I64, _U8 = torch.float32, torch.int32, torch.int64, torch.uint8


def _p(x, dtype=_F32, name="tensor"):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else ptr(x, dtype, name)


def _abi_bin_sort(*, B, N, xys, depths, radii, conics=None, opacities=None, img_h, img_w, capacity, tile_count, tile_bins,
                  isect_keys, sorted_ids, n_isect, reach_scratch=None):
    _lib.call("gol_bin_sort", c_int(B), c_int(N), _p(xys), _p(depths), _p(radii, _I32), _p(conics), _p(opacities),
              c_int(img_h), c_int(img_w), c_int(BLOCK), c_i64(capacity), _p(tile_count, _I32), _p(tile_bins, _I32),
              _p(isect_keys, _I64), _p(sorted_ids, _I32), _p(n_isect, _I32), _p(reach_scratch, _I64), stream_ptr())


def _abi_project_fwd(*, B, N, means3d, scales, glob_scale, quats, viewmats, intrins, img_h, img_w, clip_thresh, cov3d=None,
                     xys, depths, radii, conics, compensation, num_tiles_hit=None, opacities=None, opac_eff=None,
                     colors=None, records=None):
    _lib.call("gol_project_fwd", c_int(B), c_int(N), _p(means3d, name="means3d"), _p(scales, name="scales"),
              c_float(glob_scale), _p(quats, name="quats"), _p(viewmats, name="viewmat"), _p(intrins, name="intrins"),
              c_int(img_h), c_int(img_w), c_int(BLOCK), c_float(clip_thresh), _p(cov3d), _p(xys), _p(depths),
              _p(radii, _I32), _p(conics), _p(compensation), _p(num_tiles_hit, _I32), _p(opacities, name="opacity"),
              _p(opac_eff), _p(colors, name="colors"), _p(records), stream_ptr())


def _abi_project_bwd(*, B, N, means3d, scales, glob_scale, quats, viewmats, intrins, cov3d=None, radii, conics, compensation,
                     v_xy=None, v_depth=None, v_conic=None, v_compensation=None, opacities=None, v_opac_eff=None,
                     grad_stride=0, v_mean3d, v_scale, v_quat, v_opacity=None):
    _lib.call("gol_project_bwd", c_int(B), c_int(N), _p(means3d), _p(scales), c_float(glob_scale), _p(quats),
              _p(viewmats), _p(intrins), _p(cov3d), _p(radii, _I32), _p(conics), _p(compensation), _p(v_xy), _p(v_depth),
              _p(v_conic), _p(v_compensation), _p(opacities), _p(v_opac_eff), c_int(grad_stride), _p(v_mean3d),
              _p(v_scale), _p(v_quat), _p(v_opacity), stream_ptr())


def _abi_rasterize_fwd(*, B, N, img_h, img_w, planar, tile_bins, sorted_ids, capacity, records, with_extra, background,
                       out_img, out_extra=None, final_Ts, final_idx, out_alpha=None, out_extra_norm=None, norm_lo=0.0,
                       l1_target=None, l1_mask=None, l1_mask_c=0, l1_sign=None, l1_partial=None, l1_out=None,
                       l1_scale=1.0, stage_mask=None, pixels_per_lane=0):
    _lib.call("gol_rasterize_fwd", c_int(B), c_int(N), c_int(img_h), c_int(img_w), c_int(BLOCK), c_int(planar),
              _p(tile_bins, _I32), _p(sorted_ids, _I32), c_i64(capacity), _p(records), c_int(with_extra),
              _p(background), _p(out_img), _p(out_extra), _p(final_Ts), _p(final_idx, _I32), _p(out_alpha),
              _p(out_extra_norm), c_float(norm_lo), _p(l1_target), _p(l1_mask), c_int(l1_mask_c), _p(l1_sign, _U8),
              _p(l1_partial), _p(l1_out), c_float(l1_scale), _p(stage_mask, _U8), c_int(pixels_per_lane), stream_ptr())


def _abi_rasterize_bwd(*, B, N, img_h, img_w, planar, tile_bins, sorted_ids, capacity, records, with_extra, background,
                       final_Ts, final_idx, v_out_img=None, v_out_extra=None, v_out_alpha=None, v_xy, v_conic, v_colors,
                       v_extra=None, v_opacity, grad_stride=0, v_sign=None, v_sign_mask=None, v_sign_mask_c=0,
                       v_img_scale=None, v_img_scale_mul=1.0, stage_mask=None, stage_mask_ppl=0, pixels_per_lane=0):
    _lib.call("gol_rasterize_bwd", c_int(B), c_int(N), c_int(img_h), c_int(img_w), c_int(BLOCK), c_int(planar),
              _p(tile_bins, _I32), _p(sorted_ids, _I32), c_i64(capacity), _p(records), c_int(with_extra), _p(background),
              _p(final_Ts), _p(final_idx, _I32), _p(v_out_img), _p(v_out_extra), _p(v_out_alpha), _p(v_xy), _p(v_conic),
              _p(v_colors), _p(v_extra), _p(v_opacity), c_int(grad_stride), _p(v_sign, _U8), _p(v_sign_mask),
              c_int(v_sign_mask_c), _p(v_img_scale), c_float(v_img_scale_mul), _p(stage_mask, _U8), c_int(stage_mask_ppl),
              c_int(pixels_per_lane), stream_ptr())


def _abi_rasterize_nd_fwd(*, B, N, C, img_h, img_w, tile_bins, sorted_ids, capacity, records, colors, background, out_img,
                          final_Ts, final_idx, pixels_per_lane=0):
    _lib.call("gol_rasterize_nd_fwd", c_int(B), c_int(N), c_int(C), c_int(img_h), c_int(img_w), c_int(BLOCK),
              _p(tile_bins, _I32), _p(sorted_ids, _I32), c_i64(capacity), _p(records), _p(colors), _p(background),
              _p(out_img), _p(final_Ts), _p(final_idx, _I32), c_int(pixels_per_lane), stream_ptr())


def _abi_rasterize_nd_bwd(*, B, N, C, img_h, img_w, tile_bins, sorted_ids, capacity, records, colors, background, final_Ts,
                          final_idx, v_out_img, v_out_alpha=None, v_xy, v_conic, v_colors, v_opacity):
    _lib.call("gol_rasterize_nd_bwd", c_int(B), c_int(N), c_int(C), c_int(img_h), c_int(img_w), c_int(BLOCK),
              _p(tile_bins, _I32), _p(sorted_ids, _I32), c_i64(capacity), _p(records), _p(colors), _p(background),
              _p(final_Ts), _p(final_idx, _I32), _p(v_out_img), _p(v_out_alpha), _p(v_xy), _p(v_conic), _p(v_colors),
              _p(v_opacity), stream_ptr())


def _bin_sort(B, N, xys, depths, radii, img_h, img_w, ws, conics=None, opacities=None):
    """conics + opacities given -> (Gaussian, tile) pairs that cannot reach alpha >= 1/255 are pruned
    (output-preserving); omitted -> gsplat's exact 3-sigma tile lists."""
    _abi_bin_sort(B=B, N=N, xys=xys, depths=depths, radii=radii, conics=conics, opacities=opacities, img_h=img_h,
                  img_w=img_w, capacity=ws.capacity, tile_count=ws.tile_count, tile_bins=ws.tile_bins, isect_keys=ws.keys,
                  sorted_ids=ws.sorted_ids, n_isect=ws.n_isect, reach_scratch=ws.reach)


def _project_fwd(B, N, means, scales, glob_scale, quats, viewmats, intrins, img_h, img_w, clip,
                 opacities=None, colors=None):
    """colors (with opacities) given: also returns the rasterizer's packed records[B,N,16] (depth as the 4th channel)."""
    f = dict(dtype=torch.float32, device=means.device)
    records = torch.empty(B, N, SPLAT_RECORD, **f) if colors is not None else None
    cov3d, xys, conics = (torch.empty(B, N, k, **f) for k in (6, 2, 3))
    depths, comp = torch.empty(B, N, **f), torch.empty(B, N, **f)
    radii, nth = (torch.empty(B, N, dtype=torch.int32, device=means.device) for _ in range(2))
    opac_eff = torch.empty(B, N, **f) if opacities is not None else None
    _abi_project_fwd(B=B, N=N, means3d=means, scales=scales, glob_scale=glob_scale, quats=quats, viewmats=viewmats,
                     intrins=intrins, img_h=img_h, img_w=img_w, clip_thresh=clip, cov3d=cov3d, xys=xys, depths=depths,
                     radii=radii, conics=conics, compensation=comp, num_tiles_hit=nth, opacities=opacities,
                     opac_eff=opac_eff, colors=colors, records=records)
    out = (cov3d, xys, depths, radii, conics, comp, nth, opac_eff)
    return out + (records,) if colors is not None else out


def _pack_records(B, N, xys, conics, colors, extra, opacities):
    """gol_splat_pack: the rasterizer's packed records from gsplat-style attribute arrays (colors None: r = g = b = 0, the
    records of the N-channel rasterizer)."""
    records = torch.empty(B, N, SPLAT_RECORD, dtype=torch.float32, device=xys.device)
    _lib.call("gol_splat_pack", c_int(B), c_int(N), fptr(xys), fptr(conics), fptr(colors), fptr(extra), fptr(opacities),
              fptr(records), stream_ptr())
    return records


def _f32c(t):
    return t.to(torch.float32).contiguous()


# --------------------------------------------------------------------------------------------
# gsplat-0.1.11-compatible operators
# --------------------------------------------------------------------------------------------
class _ProjectGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3d, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, img_height, img_width,
                block_width, clip_thresh):
        if block_width != BLOCK:
            raise NotImplementedError("goliath_amd implements block_width=16 (the reference's value)")
        N = means3d.shape[0]
        dev = means3d.device
        means3d, scales, quats = _f32c(means3d), _f32c(scales), _f32c(quats)
        vm = _f32c(viewmat).reshape(-1)[:12].contiguous().view(1, 12)
        intr = torch.tensor([[fx, fy, cx, cy]], dtype=torch.float32).to(dev, non_blocking=True)
        with _lib.device_guard(dev):
            cov3d, xys, depths, radii, conics, comp, nth, _ = _project_fwd(
                1, N, means3d, scales, float(glob_scale), quats, vm, intr, img_height, img_width,
                float(clip_thresh))
        ctx.save_for_backward(means3d, scales, quats, vm, intr, cov3d[0], radii[0], conics[0], comp[0])
        ctx.glob_scale = float(glob_scale)
        ctx.set_materialize_grads(False)
        outs = (xys[0], depths[0], radii[0], conics[0], comp[0], nth[0], cov3d[0])
        ctx.mark_non_differentiable(outs[2], outs[5])
        return outs

    @staticmethod
    def backward(ctx, v_xys, v_depths, v_radii, v_conics, v_compensation, v_num_tiles_hit, v_cov3d):
        means3d, scales, quats, vm, intr, cov3d, radii, conics, comp = ctx.saved_tensors
        N = means3d.shape[0]
        v_mean = torch.empty_like(means3d)
        v_scale = torch.empty_like(scales)
        v_quat = torch.empty_like(quats)
        c = lambda t: None if t is None else _f32c(t)
        # converted gradients are bound to locals so they outlive the launch
        g_xy, g_depth, g_conic, g_comp = c(v_xys), c(v_depths), c(v_conics), c(v_compensation)
        with _lib.device_guard(means3d.device):
            _abi_project_bwd(B=1, N=N, means3d=means3d, scales=scales, glob_scale=ctx.glob_scale, quats=quats, viewmats=vm,
                             intrins=intr, cov3d=cov3d, radii=radii, conics=conics, compensation=comp, v_xy=g_xy,
                             v_depth=g_depth, v_conic=g_conic, v_compensation=g_comp, v_mean3d=v_mean, v_scale=v_scale,
                             v_quat=v_quat)
        return (v_mean, v_scale, None, v_quat) + (None,) * 9



def project_gaussians(means3d, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, img_height, img_width,
                      block_width, clip_thresh=0.01):
    """gsplat.project_gaussians (0.1.11): returns (xys, depths, radii, conics, compensation,
    num_tiles_hit, cov3d); gradients flow to means3d, scales, quats."""
    if means3d.dim() != 2 or means3d.shape[1] != 3:
        raise ValueError("means3d must have dimensions (N, 3)")
    return _ProjectGaussians.apply(means3d, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, img_height,
                                   img_width, block_width, clip_thresh)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, opacity, img_height, img_width,
                block_width, background, return_alpha):
        dev = xys.device
        N, C = xys.shape[0], colors.shape[-1]
        xys, depths, conics, colors = _f32c(xys), _f32c(depths), _f32c(conics), _f32c(colors)
        opacity = _f32c(opacity).reshape(-1)
        radii = radii.to(torch.int32).contiguous()
        background = _f32c(background)
        # gsplat semantics: host sync on the intersection count (rasterize.py)
        n_isect = int(num_tiles_hit.to(torch.int64).sum().item()) if N > 0 else 0
        ctx.n_isect = n_isect
        ctx.dims = (img_height, img_width)
        if n_isect < 1:
            # background-only image and final_T = 0 (alpha = 1)
            out_img = torch.ones(img_height, img_width, C, device=dev) * background
            final_Ts = torch.zeros(img_height, img_width, device=dev)
            ctx.save_for_backward(xys, conics, colors, opacity, background)
        else:
            T = _tiles(img_height, img_width)
            ws = _Workspace(1, N, T, n_isect, dev)
            out_img = torch.empty(1, img_height, img_width, C, device=dev)
            final_Ts = torch.empty(1, img_height, img_width, device=dev)
            final_idx = torch.empty(1, img_height, img_width, dtype=torch.int32, device=dev)
            with _lib.device_guard(dev):
                _bin_sort(1, N, xys, depths, radii, img_height, img_width, ws, conics, opacity)
                if C == 3:
                    records = _pack_records(1, N, xys, conics, colors, None, opacity)
                    _abi_rasterize_fwd(B=1, N=N, img_h=img_height, img_w=img_width, planar=0, tile_bins=ws.tile_bins,
                                       sorted_ids=ws.sorted_ids, capacity=ws.capacity, records=records, with_extra=0,
                                       background=background, out_img=out_img, final_Ts=final_Ts, final_idx=final_idx)
                else:   # gsplat's nd_rasterize_forward: geometry records without colour, colours as they are
                    records = _pack_records(1, N, xys, conics, None, None, opacity)
                    _abi_rasterize_nd_fwd(B=1, N=N, C=C, img_h=img_height, img_w=img_width, tile_bins=ws.tile_bins,
                                          sorted_ids=ws.sorted_ids, capacity=ws.capacity, records=records, colors=colors,
                                          background=background, out_img=out_img, final_Ts=final_Ts, final_idx=final_idx)
            ctx.ws = ws
            ctx.save_for_backward(xys, conics, colors, opacity, background, final_Ts, final_idx, records)
            out_img, final_Ts = out_img[0], final_Ts[0]
        if return_alpha:
            return out_img, 1 - final_Ts
        return out_img

    @staticmethod
    def backward(ctx, v_out_img, v_out_alpha=None):
        saved = ctx.saved_tensors
        xys, conics, colors, opacity, background = saved[:5]
        N = xys.shape[0]
        v_xy = torch.zeros_like(xys)
        v_conic = torch.zeros_like(conics)
        v_colors = torch.zeros_like(colors)
        v_opacity = torch.zeros(N, device=xys.device)
        if ctx.n_isect >= 1 and v_out_img is not None:
            final_Ts, final_idx, records = saved[5], saved[6], saved[7]
            H, W = ctx.dims
            ws = ctx.ws
            va = None if v_out_alpha is None else _f32c(v_out_alpha)
            vo = _f32c(v_out_img)
            with _lib.device_guard(xys.device):
                if colors.shape[-1] == 3:
                    _abi_rasterize_bwd(B=1, N=N, img_h=H, img_w=W, planar=0, tile_bins=ws.tile_bins,
                                       sorted_ids=ws.sorted_ids, capacity=ws.capacity, records=records, with_extra=0,
                                       background=background, final_Ts=final_Ts, final_idx=final_idx, v_out_img=vo,
                                       v_out_alpha=va, v_xy=v_xy, v_conic=v_conic, v_colors=v_colors, v_opacity=v_opacity)
                else:
                    _abi_rasterize_nd_bwd(B=1, N=N, C=colors.shape[-1], img_h=H, img_w=W, tile_bins=ws.tile_bins,
                                          sorted_ids=ws.sorted_ids, capacity=ws.capacity, records=records, colors=colors,
                                          background=background, final_Ts=final_Ts, final_idx=final_idx, v_out_img=vo,
                                          v_out_alpha=va, v_xy=v_xy, v_conic=v_conic, v_colors=v_colors,
                                          v_opacity=v_opacity)
        # ctx.ws stays: a second backward through this node (retain_graph=True, per-loss backward calls) needs the tile
        # lists again; autograd frees them with the graph
        return (v_xy, None, None, v_conic, None, v_colors, v_opacity[:, None]) + (None,) * 5


def rasterize_gaussians(xys, depths, radii, conics, num_tiles_hit, colors, opacity, img_height, img_width,
                        block_width, background=None, return_alpha=False):
    """gsplat.rasterize_gaussians (0.1.11): colors[N, C] for any C >= 1 (uint8 colours are divided by 255), background[C]
    (None: ones), returns out_img[H, W, C] (and alpha[H, W] with return_alpha); gradients flow to xys, conics, colors and
    opacity.  C == 3 runs the 3-channel kernels (gol_rasterize_fwd / _bwd, what the reference calls,
    render_gsplat.py:65-104), every other C the N-channel ones (gol_rasterize_nd_fwd / _bwd, gsplat's nd_rasterize_*)."""
    assert block_width > 1 and block_width <= 16, "block_width must be between 2 and 16"
    if block_width != BLOCK:
        raise NotImplementedError("goliath_amd implements block_width=16 (the reference's value)")
    if colors.dtype == torch.uint8:
        colors = colors.float() / 255
    if xys.ndimension() != 2 or xys.size(1) != 2:
        raise ValueError("xys must have dimensions (N, 2)")
    if colors.ndimension() != 2:
        raise ValueError("colors must have dimensions (N, D)")
    if background is not None:
        assert background.shape[0] == colors.shape[-1], "incorrect shape of background color tensor"
    else:
        background = torch.ones(colors.shape[-1], dtype=torch.float32, device=colors.device)
    if opacity.ndimension() != 2 or opacity.shape[1] != 1:
        opacity = opacity.reshape(-1, 1)
    return _RasterizeGaussians.apply(xys.contiguous(), depths.contiguous(), radii.contiguous(),
                                     conics.contiguous(), num_tiles_hit.contiguous(), colors.contiguous(),
                                     opacity.contiguous(), img_height, img_width, block_width,
                                     background.contiguous(), return_alpha)


# --------------------------------------------------------------------------------------------
# Fused, batched, sync-free path
# --------------------------------------------------------------------------------------------
class RenderLayout(ctypes.Structure):
    """include/goliath_hip.h: gol_render_ws -- byte offsets of the sub-buffers of a render workspace."""
    _fields_ = [(n, ctypes.c_int64) for n in (
        "cov3d", "xys", "depths", "radii", "conics", "comp", "nth", "opac_eff", "records", "tile_count", "tile_bins",
        "keys", "sorted_ids", "n_isect", "final_T", "final_idx", "l1_sign", "stage_mask", "total")]


_LAYOUTS = {}


def _layout(B, N, img_h, img_w, capacity, with_l1, projected=False):
    """projected: the projection's outputs live in a views.Projected (written by the shading kernel), not in the workspace."""
    key = (B, N, img_h, img_w, capacity, with_l1, projected)
    L = _LAYOUTS.get(key)
    if L is None:
        L = RenderLayout()
        _lib.call("gol_render_layout_projected" if projected else "gol_render_layout", c_int(B), c_int(N), c_int(img_h),
                  c_int(img_w), c_i64(capacity), c_int(with_l1), ctypes.byref(L))
        if len(_LAYOUTS) > 256:
            _LAYOUTS.clear()
        _LAYOUTS[key] = L
    return L


def _ws_view(ws, off, dtype, shape):
    """Typed view of a workspace sub-buffer (no copy)."""
    return ws[off:off + math.prod(shape) * dtype.itemsize].view(dtype).view(shape)


def _fwd_ppl(B):
    """gol_raster_plan: the wave footprint (pixels per lane) a raster forward of B views runs with when it is left the choice
    -- what the staged forward below wrote its stage_mask with, as gol_render_bwd works it out for the fused call."""
    ppl = c_int(0)
    _lib.load().gol_raster_plan(c_int(B), ctypes.byref(ppl))   # (host only: not an ABI call the instrumented pass times)
    return ppl.value


def _render_fwd_staged(B, N, src, attrs, background, with_depth, norm_lo, cap, ws, L, out_img, out_depth, alpha, depth_norm,
                       l1_target, l1_mask, l1_mask_c, l1_partial, l1_out, l1_scale):
    """gol_render_fwd[_projected] stage by stage (what csrc/render.hip composes), for _lib.TIMING.  src: the views'
    gol_shade_proj; attrs = (means, scales, quats, opacity, colors): unfused, project them into `src` first."""
    a = ws.data_ptr()
    if attrs is not None:
        means, scales, quats, opacity, colors = attrs
        _abi_project_fwd(B=B, N=N, means3d=means, scales=scales, glob_scale=src.glob_scale, quats=quats,
                         viewmats=src.viewmats, intrins=src.intrins, img_h=src.img_h, img_w=src.img_w,
                         clip_thresh=src.clip_thresh, xys=src.xys, depths=src.depths, radii=src.radii, conics=src.conics,
                         compensation=src.comp, opacities=opacity, opac_eff=src.opac_eff, colors=colors,
                         records=src.records)
    _abi_bin_sort(B=B, N=N, xys=src.xys, depths=src.depths, radii=src.radii, conics=src.conics, opacities=src.opac_eff,
                  img_h=src.img_h, img_w=src.img_w, capacity=cap, tile_count=a + L.tile_count, tile_bins=a + L.tile_bins,
                  isect_keys=a + L.keys, sorted_ids=a + L.sorted_ids, n_isect=a + L.n_isect)
    _abi_rasterize_fwd(B=B, N=N, img_h=src.img_h, img_w=src.img_w, planar=1, tile_bins=a + L.tile_bins,
                       sorted_ids=a + L.sorted_ids, capacity=cap, records=src.records, with_extra=int(with_depth),
                       background=background, out_img=out_img, out_extra=out_depth, final_Ts=a + L.final_T,
                       final_idx=a + L.final_idx, out_alpha=alpha, out_extra_norm=depth_norm, norm_lo=norm_lo,
                       l1_target=l1_target, l1_mask=l1_mask, l1_mask_c=l1_mask_c,
                       l1_sign=a + L.l1_sign if l1_target is not None else None, l1_partial=l1_partial, l1_out=l1_out,
                       l1_scale=l1_scale, stage_mask=a + L.stage_mask)


def _render_bwd_staged(B, N, src, attrs, grads, background, cap, ws, L, v_img, v_depth, v_alpha, use_l1, l1_mask, v_scale,
                       v_scale_mul, rec):
    """gol_render_bwd[_projected] stage by stage: the raster backward into the zeroed records rec[B,N,GRAD_RECORD] (rgb |
    opacity | xy | conic | depth | pad); unfused (attrs = (means, scales, quats, opacity)): the projection backward."""
    a = ws.data_ptr()
    field = lambda k: rec.data_ptr() + 4 * k
    use_depth = v_depth is not None
    rec.zero_()
    _abi_rasterize_bwd(B=B, N=N, img_h=src.img_h, img_w=src.img_w, planar=1, tile_bins=a + L.tile_bins,
                       sorted_ids=a + L.sorted_ids, capacity=cap, records=src.records, with_extra=int(use_depth),
                       background=background, final_Ts=a + L.final_T, final_idx=a + L.final_idx, v_out_img=v_img,
                       v_out_extra=v_depth, v_out_alpha=v_alpha, v_xy=field(4), v_conic=field(6), v_colors=field(0),
                       v_extra=field(9) if use_depth else None, v_opacity=field(3), grad_stride=GRAD_RECORD,
                       v_sign=a + L.l1_sign if use_l1 else None, v_sign_mask=l1_mask,
                       v_sign_mask_c=0 if l1_mask is None else l1_mask.shape[1], v_img_scale=v_scale,
                       v_img_scale_mul=v_scale_mul, stage_mask=a + L.stage_mask, stage_mask_ppl=_fwd_ppl(B))
    if attrs is not None:
        means, scales, quats, opacity = attrs
        v_mean, v_scale_g, v_quat, v_opacity = grads
        _abi_project_bwd(B=B, N=N, means3d=means, scales=scales, glob_scale=src.glob_scale, quats=quats,
                         viewmats=src.viewmats, intrins=src.intrins, radii=src.radii, conics=src.conics,
                         compensation=src.comp, v_xy=field(4), v_depth=field(9) if use_depth else None, v_conic=field(6),
                         opacities=opacity, v_opac_eff=field(3), grad_stride=GRAD_RECORD, v_mean3d=v_mean,
                         v_scale=v_scale_g, v_quat=v_quat, v_opacity=v_opacity)


class _RenderViews(torch.autograd.Function):
    """The fused path: ONE C-ABI call per direction (gol_render_fwd / gol_render_bwd, csrc/render.hip) out of one
    workspace allocation; the host work of a direction is that call plus the allocation of its outputs.  With
    _lib.TIMING set (bench.py's instrumented pass) the same work runs as one ABI call per stage instead."""

    @staticmethod
    def forward(ctx, means, scales, quats, opacity, colors, viewmats, intrins, background, img_h, img_w,
                glob_scale, clip_thresh, with_depth, capacity, depth_norm_lo, plan_key, l1_target, l1_mask,
                raw_depth, records, pack, view_set, res):
        # records / pack / view_set given (a views.Projected): the Gaussians were projected by the shading kernel -- means ...
        # colors are None, the call starts at the tile count and its backward ends at the gradient records (= the gradient of
        # `records`, which the shading backward pushes through the projection's vjp)
        projected = records is not None
        B, N = (records if projected else means).shape[:2]
        dev = (records if projected else means).device
        pj = _views.proj_struct(view_set, records, pack) if projected else None
        attrs = None if projected else (means, scales, quats, opacity, colors)
        T = _tiles(img_h, img_w)
        with_l1 = 1 if l1_target is not None else 0
        f = dict(dtype=torch.float32, device=dev)
        out_img = torch.empty(B, 3, img_h, img_w, **f)   # planar, as the model consumes it
        out_depth = torch.empty(B, img_h, img_w, **f) if with_depth and raw_depth else None
        # alpha = 1 - T and depth / clamp(alpha, lo, 1) come out of the raster epilogue (rgca.py:137,144-145)
        alpha = torch.empty(B, img_h, img_w, **f)
        depth_norm = torch.empty(B, img_h, img_w, **f) if with_depth else None
        # optional fused L1 against a target image: per-tile sums here, the sign codes (the loss gradient up to mask x
        # scalar; one byte per pixel) in the workspace
        l1_partial = torch.empty(B, T, **f) if with_l1 else None
        # the loss value itself: sum(l1_partial) / (B*3*H*W), added up by the last workgroup of the raster launch
        l1_out = torch.empty(1, **f) if with_l1 else None
        l1_inv_n = 1.0 / max(B * 3 * img_h * img_w, 1)
        l1_mask_c = 0 if l1_mask is None else l1_mask.shape[1]

        def run(cap):
            L = _layout(B, N, img_h, img_w, cap, with_l1, projected)
            ws = torch.empty(max(L.total, 1), dtype=torch.uint8, device=dev)
            # the cameras and screen-space buffers the call bins and rasterizes; unfused: projected into the workspace
            a = ws.data_ptr()
            src = pj if projected else _views.ShadeProj(
                fptr(viewmats).value, fptr(intrins).value, img_h, img_w, glob_scale, clip_thresh, a + L.xys, a + L.depths,
                a + L.radii, a + L.conics, a + L.comp, a + L.opac_eff, a + L.records)
            if _lib.TIMING is not None:
                _render_fwd_staged(B, N, src, attrs, background, with_depth, depth_norm_lo, cap, ws, L, out_img, out_depth,
                                   alpha, depth_norm, l1_target, l1_mask, l1_mask_c, l1_partial, l1_out, l1_inv_n)
            else:
                entry = (("gol_render_fwd_projected", c_int(B), c_int(N), ctypes.byref(pj)) if projected else
                         ("gol_render_fwd", c_int(B), c_int(N), c_int(img_h), c_int(img_w), c_float(glob_scale),
                          c_float(clip_thresh), fptr(means), fptr(scales), fptr(quats), fptr(opacity), fptr(colors),
                          fptr(viewmats), fptr(intrins)))
                _lib.call(*entry, fptr(background), c_int(1 if with_depth else 0), c_float(depth_norm_lo), c_i64(cap),
                          ctypes.c_void_p(ws.data_ptr()), ctypes.byref(L), fptr(out_img), fptr(out_depth), fptr(alpha),
                          fptr(depth_norm), fptr(l1_target), fptr(l1_mask), c_int(l1_mask_c), fptr(l1_partial),
                          fptr(l1_out), c_float(l1_inv_n), stream_ptr())
            n_isect = _ws_view(ws, L.n_isect, torch.int32, (B,))
            pending = PLANNER.fetch(n_isect) if plan_key is not None and B > 0 else None
            return ws, L, src, n_isect, pending

        with _lib.device_guard(dev):
            ws, L, src, n_isect, pending = run(capacity)
            if pending is not None:
                # the counts were final after the tile scan; the raster is still queued behind this wait
                worst = PLANNER.finish(*pending)
                if worst > capacity:
                    # some lists were truncated: grow and redo the call into the SAME output buffers, in stream
                    # order, before anything downstream can read them
                    capacity = PLANNER.set(plan_key, worst)
                    PLANNER.last_worst[plan_key] = worst
                    PLANNER.reruns += 1
                    ws, L, src, n_isect, pending = run(capacity)
                    PLANNER.finish(*pending)
                else:
                    PLANNER.observe(plan_key, worst, capacity)
                PLANNER.passed(plan_key)
        res.bind((B, N, img_h, img_w, T), ws, L, capacity, src, pack if projected else ws, records if projected else ws)
        ctx.L, ctx.capacity, ctx.src = L, capacity, src
        ctx.cfg = (img_h, img_w, glob_scale, with_depth, depth_norm_lo, with_l1)
        ctx.l1_inv_n = l1_inv_n
        l1 = l1_out.reshape(()) if with_l1 else None  # == mean(|(rgb - target) * mask|)
        ctx.view_set = view_set   # (keeps the cameras `src` points at alive)
        ctx.save_for_backward(means, scales, quats, opacity, viewmats, intrins, background, ws, l1_mask, records, pack)
        ctx.mark_non_differentiable(ws, n_isect)
        ctx.set_materialize_grads(False)
        return out_img, alpha, out_depth, depth_norm, l1, ws, n_isect

    @staticmethod
    def backward(ctx, v_img, v_alpha, v_depth, v_depth_norm, v_l1, *_non_differentiable):
        means, scales, quats, opacity, viewmats, intrins, background, ws, l1_mask, records, pack = ctx.saved_tensors
        img_h, img_w, glob_scale, with_depth, depth_norm_lo, with_l1 = ctx.cfg
        projected = records is not None
        B, N = (records if projected else means).shape[:2]
        dev = ws.device
        L = ctx.L
        if v_depth_norm is not None:  # depth_norm = depth / clamp(alpha.detach(), lo, 1), alpha = 1 - final_T
            final_Ts = _ws_view(ws, L.final_T, torch.float32, (B, img_h, img_w))
            g = v_depth_norm / (1.0 - final_Ts).clamp(depth_norm_lo, 1.0)
            v_depth = g if v_depth is None else v_depth + g
        if not with_l1:
            v_l1 = None
        if v_img is None and v_alpha is None and v_depth is None and v_l1 is None:
            return (None,) * 23
        # fused L1: d loss / d rgb = (sign code - 1) * mask * (v_l1 / n).  The raster backward decodes the sign bytes itself
        # and adds the term to v_img (if the image has another consumer); the scalar goes in as a device value: no sync,
        # no pass over the image
        # d loss / d l1 goes in as it is (a device scalar), 1 / n as a host scalar beside it: no kernel of its own
        v_scale = None
        if v_l1 is not None:
            v_scale = v_l1.to(torch.float32).reshape(1).contiguous()
        if v_img is None and v_l1 is None:
            v_img = torch.zeros(B, 3, img_h, img_w, device=dev)
        use_depth = with_depth and v_depth is not None
        # converted upstream gradients stay bound to locals until the launches below are issued
        v_img_c = None if v_img is None else _f32c(v_img)
        v_depth_c = _f32c(v_depth) if use_depth else None
        v_alpha_c = None if v_alpha is None else _f32c(v_alpha)
        # 64-byte gradient records per Gaussian (include/goliath_hip.h: GOL_GRAD_RECORD), zeroed by the call: a Gaussian's
        # float atomics hit one cache line and are issued by 16 adjacent lanes
        rec = torch.empty(B, N, GRAD_RECORD, device=dev)
        use_mask = l1_mask if v_l1 is not None else None
        attrs = None if projected else (means, scales, quats, opacity)
        grads = None if projected else tuple(torch.empty_like(t) for t in attrs)   # v_mean, v_scale, v_quat, v_opacity
        with _lib.device_guard(dev):
            if _lib.TIMING is not None:
                _render_bwd_staged(B, N, ctx.src, attrs, grads, background, ctx.capacity, ws, L, v_img_c, v_depth_c,
                                   v_alpha_c, v_l1 is not None, use_mask, v_scale, ctx.l1_inv_n, rec)
                v_color = None if projected else rec[..., :3]   # (the single call writes a dense copy instead)
            else:
                shared = (fptr(background), c_i64(ctx.capacity), ctypes.c_void_p(ws.data_ptr()), ctypes.byref(L),
                          fptr(v_img_c), fptr(v_depth_c), fptr(v_alpha_c), c_int(1 if v_l1 is not None else 0),
                          fptr(use_mask), c_int(0 if use_mask is None else use_mask.shape[1]), fptr(v_scale),
                          c_float(ctx.l1_inv_n), fptr(rec))
                if projected:
                    _lib.call("gol_render_bwd_projected", c_int(B), c_int(N), ctypes.byref(ctx.src), *shared, stream_ptr())
                else:
                    # dense copy of the records' colour gradient (written by the projection backward)
                    v_color = torch.empty(B, N, 3, device=dev)
                    _lib.call("gol_render_bwd", c_int(B), c_int(N), c_int(img_h), c_int(img_w), c_float(glob_scale),
                              fptr(means), fptr(scales), fptr(quats), fptr(opacity), fptr(viewmats), fptr(intrins), *shared,
                              *(fptr(g) for g in grads), fptr(v_color), stream_ptr())
        # (the workspace stays alive with the node: retain_graph / a second backward re-reads the tile lists)
        if projected:
            return (None,) * 19 + (rec, None, None, None)
        return grads + (v_color,) + (None,) * 18


_BLACK = {}


class _LazyRender(dict):
    """Result of render_views: the images are plain entries; the diagnostics (typed views into the call's buffers:
    radii, final_T, final_idx, sorted_ids, tile_bins) are created on first access."""

    def bind(self, dims, ws, L, cap, src, arrays, records):
        """What the forward rendered with: workspace, layout, capacity, and the gol_shade_proj `src` whose per-Gaussian
        arrays and records live in the tensors `arrays` and `records` (the workspace, or a Projected's pack and records)."""
        self._dims, self._ws, self._L, self._cap, self._src, self._arrays, self._records = dims, ws, L, cap, src, arrays, records

    def __missing__(self, key):
        B, N, H, W, T = self._dims
        ws, L = self._ws, self._L
        if key == "radii":
            buf = self._arrays.view(-1).view(torch.uint8)   # the workspace, or a views.Projected's pack
            v = _ws_view(buf, (self._src.radii or 0) - buf.data_ptr(), torch.int32, (B, N))
        elif key == "final_T":
            v = _ws_view(ws, L.final_T, torch.float32, (B, 1, H, W))
        elif key == "final_idx":
            v = _ws_view(ws, L.final_idx, torch.int32, (B, H, W))
        elif key == "sorted_ids":
            v = _ws_view(ws, L.sorted_ids, torch.int32, (B, max(self._cap, 1)))
        elif key == "tile_bins":
            v = _ws_view(ws, L.tile_bins, torch.int32, (B, T, 2))
        else:
            raise KeyError(key)
        self[key] = v
        return v


def raster_pair_counts(res):
    """Diagnostic: [B,2] int64 = per view the (pixel, list entry) pairs a render_views result tested (entries up to each
    pixel's final_idx) and took (alpha >= 1/255) -- gol_raster_count_pairs on the call's workspace."""
    B, N, H, W, T = res._dims
    ws, L = res._ws, res._L
    a = ws.data_ptr()
    counts = torch.empty(B, 2, dtype=torch.int64, device=ws.device)
    with _lib.device_guard(ws.device):
        _lib.call("gol_raster_count_pairs", c_int(B), c_int(N), c_int(H), c_int(W), _p(a + L.tile_bins),
                  _p(a + L.sorted_ids), c_i64(res._cap), _p(res._src.records), _p(a + L.final_idx), _p(counts, _I64),
                  stream_ptr())
    return counts


def render_views(means, scales, quats, opacity, colors, viewmats, intrins, img_h, img_w,
                 background=None, glob_scale=1.0, clip_thresh=0.1, with_depth=True, capacity=None, depth_norm_lo=0.05,
                 l1_target=None, l1_mask=None, raw_depth=True, projected=None, extra_colors=None):
    """Render B views in one launch sequence.

    means[B,N,3] scales[B,N,3] quats[B,N,4] opacity[B,N] or [B,N,1] colors[B,N,3]  (fp32, GPU)
    viewmats[B,3,4] (or [B,12]; world->camera, row-major), intrins[B,4] = (fx, fy, cx, cy)
    Returns dict(render[B,3,H,W], alpha[B,1,H,W] (= 1 - final_T), depth[B,1,H,W] (un-normalised,
    like render_gsplat.py:105-106), depth_norm[B,1,H,W] (= depth / clamp(alpha.detach(), depth_norm_lo, 1),
    rgca.py:144-145), final_T, radii[B,N] int32, n_isect[B] int32, final_idx[B,H,W], sorted_ids[B,cap], tile_bins[B,T,2]).
    `capacity` given: the caller sized the intersection buffers and checks `n_isect` itself; omitted: planned
    (CapacityPlanner) -- an overflow is repaired inside this call and never surfaces.
    l1_target[B,3,H,W] (+ l1_mask[B,1|3,H,W]): also returns "l1_loss" = mean(|(render - target) * mask|), the masked
    L1 of rgb_l1 (ca_code/loss/__init__.py:391-411), computed in the raster epilogue and back-propagated by the raster
    backward itself (no separate passes over the image; no gradient to target / mask).
    raw_depth=False: only depth_norm is produced (what AutoEncoder.render returns, rgca.py:144-145) -- the forward
    writes one image less; "depth" is then absent from the result.
    projected (a views.Projected out of shading_tail(..., views=...)): the Gaussians are already projected onto these
    cameras by the shading kernel; means ... intrins are ignored (pass None), glob_scale / clip_thresh are the ViewSet's.
    extra_colors[B,N,Ce] (forward-only: with grad mode on and an input that requires grad this raises): Ce further
    channels composited over the SAME tile lists and records -- one gol_rasterize_nd_fwd call after the forward has settled
    its lists (the planner's overflow repair included), black background -- returned as "extra"[B,Ce,H,W].  What the
    relight visualisation's diffuse / specular breakdown needs (rgca.py:239-243) without projecting, binning and sorting
    the same Gaussians again.
    """
    if extra_colors is not None:
        BN = tuple((projected.records if projected is not None else means).shape[:2])
        if extra_colors.dim() != 3 or tuple(extra_colors.shape[:2]) != BN or extra_colors.shape[2] < 1:
            raise ValueError("extra_colors must be [B,N,Ce]")
        ins = (means, scales, quats, opacity, colors, extra_colors) + (() if projected is None else (projected.records,))
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ins):
            raise _lib.GoliathHipError("render_views(extra_colors=...) is forward-only: call it under torch.no_grad() or "
                                       "with detached inputs")
        if not extra_colors.is_cuda:
            raise _lib.GoliathHipError("render_views needs CUDA(HIP) tensors; there is no CPU path")
    if projected is not None:
        B, N = projected.records.shape[:2]
        dev = projected.records.device
        if (projected.views.height, projected.views.width) != (img_h, img_w):
            raise ValueError("projected for another image size")
        means = scales = quats = opacity = colors = viewmats = intrins = None
        glob_scale, clip_thresh = projected.views.glob_scale, projected.views.clip_thresh
    else:
        B, N = means.shape[:2]
        dev = means.device
        if not means.is_cuda:
            raise _lib.GoliathHipError("render_views needs CUDA(HIP) tensors; there is no CPU path")
        means, scales, quats, colors = _f32c(means), _f32c(scales), _f32c(quats), _f32c(colors)
        opacity = _f32c(opacity).reshape(B, N)
        viewmats = _f32c(viewmats).reshape(B, viewmats[0].numel() if B else 12)[:, :12].contiguous()
        intrins = _f32c(intrins).reshape(B, 4)
    if background is None:
        background = _BLACK.get(dev)   # render_gsplat.py:38-39 (one constant per device: no fill kernel per call)
        if background is None:
            background = _BLACK[dev] = torch.zeros(3, device=dev)
    background = _f32c(background)
    T = _tiles(img_h, img_w)
    key = (B, N, img_h, img_w, dev.index)
    plan_key, deferred = None, False
    if capacity is None:
        planned = PLANNER.get(key)
        if PLANNER.frozen:
            if planned is None:
                raise _lib.GoliathHipError("render_views inside a graph capture needs a calibrated capacity: run the "
                                           "same shapes once eagerly first")
        else:
            if PLANNER.pending:
                PLANNER.poll()   # counts of earlier calls that have landed meanwhile (async mode: raises on an overflow)
                planned = PLANNER.get(key)
            if planned is None or PLANNER.must_block(key):
                plan_key = key   # the forward waits for its own counts and repairs an overflow in place
            else:
                deferred = True
        capacity = planned if planned is not None else PLANNER.initial(N, T)
    if l1_target is not None:
        l1_target = _f32c(l1_target.detach())
        if tuple(l1_target.shape) != (B, 3, img_h, img_w):
            raise ValueError("l1_target must be [B,3,H,W]")
        if l1_mask is not None:
            l1_mask = _f32c(l1_mask.detach())
            if l1_mask.dim() != 4 or l1_mask.shape[0] != B or l1_mask.shape[1] not in (1, 3):
                raise ValueError("l1_mask must be [B,1,H,W] or [B,3,H,W]")
    else:
        l1_mask = None
    res = _LazyRender()
    img, alpha, depth, depth_norm, l1, _, n_isect = _RenderViews.apply(
        means, scales, quats, opacity, colors, viewmats, intrins, background, img_h, img_w, float(glob_scale),
        float(clip_thresh), bool(with_depth), int(capacity), float(depth_norm_lo), plan_key, l1_target, l1_mask,
        bool(raw_depth), None if projected is None else projected.records, None if projected is None else projected.pack,
        None if projected is None else projected.views, res)
    # res._cap: the capacity the forward rendered with (grown if the checked call had to re-run)
    if PLANNER.frozen:
        PLANNER.frozen_log.append((n_isect, res._cap))
    elif deferred and B > 0:
        PLANNER.note(key, n_isect, res._cap)
    res["render"], res["alpha"], res["n_isect"] = img, alpha[:, None], n_isect
    # per-pixel index of the last contributor in its view's depth-sorted list, and that list: res["final_idx"],
    # res["sorted_ids"], res["tile_bins"], res["final_T"], res["radii"] (views into the call's workspace, made on access)
    if with_depth:
        if depth is not None:
            res["depth"] = depth[:, None]
        res["depth_norm"] = depth_norm[:, None]  # depth / clamp(alpha.detach(), depth_norm_lo, 1)
    if l1 is not None:
        res["l1_loss"] = l1
    if extra_colors is not None:
        res["extra"] = _raster_extra(res, extra_colors)
    return res


def _raster_extra(res, extra_colors):
    """extra_colors[B,N,Ce] composited by the N-channel rasterizer over the tile lists and geometry records the render_views
    result `res` was rasterized with (its own final_T / final_idx go to buffers of their own: the result's stay as they
    are); [B,Ce,H,W].  Shape and device of extra_colors were checked at the top of render_views."""
    B, N, H, W, _ = res._dims
    ws, L = res._ws, res._L
    extra_colors = _f32c(extra_colors.detach())
    Ce = extra_colors.shape[2]
    dev = ws.device
    out = torch.empty(B, H, W, Ce, dtype=torch.float32, device=dev)
    if B == 0 or N == 0:
        return out.zero_().permute(0, 3, 1, 2).contiguous()
    final_Ts = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    final_idx = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    a = ws.data_ptr()
    with _lib.device_guard(dev):
        _abi_rasterize_nd_fwd(B=B, N=N, C=Ce, img_h=H, img_w=W, tile_bins=a + L.tile_bins, sorted_ids=a + L.sorted_ids,
                              capacity=res._cap, records=res._src.records, colors=extra_colors,
                              background=torch.zeros(Ce, dtype=torch.float32, device=dev), out_img=out, final_Ts=final_Ts,
                              final_idx=final_idx)
    return out.permute(0, 3, 1, 2).contiguous()
