"""Mesh render layer on top of `gol_mesh_raster` (csrc/meshraster.hip): what the reference gets from drtk.

    transform(verts, K, Rt)                 drtk.transform as called at ca_code/utils/render_drtk.py:42
    rasterize(v_pix, vi, h, w)              drtk.rasterize + drtk.render (:44-46): index_img, depth_img, bary_img
    RenderLayer(h, w, vi, vt, vti)          ca_code/utils/render_drtk.py:14-82 (same constructor / forward / dict keys)
drtk is a third-party dependency that is NOT in the reference tree (requirements.txt:6); the sampling conventions are
stated in csrc/meshraster.hip (pixel centres at (j + 0.5, i + 0.5), as pytorch3d's cameras_from_opencv_projection places
them for the reference's other back-end, render_pytorch3d.py:49-51; if drtk samples at integer coordinates instead the
shadow depth map is shifted by half a pixel -- not verifiable here, and below the 3x3 PCF footprint of its only consumer).
The hot-path consumer is the shadow-map depth render (ca_code/utils/shadowmap.py:39-50, under no_grad in
ca_code/models/urhand.py:404,492).

Round 4: the layer is DIFFERENTIABLE like drtk's (the model's final textured render, urhand.py:684, called with
edge_grad=self.training): `render(v_pix, vi, index_img)` re-evaluates depth and perspective-correct barycentrics of the
rasterized faces as differentiable functions of v_pix (drtk.render; the visibility, i.e. index_img, comes from
gol_mesh_raster and is held fixed), textures / vertex attributes get their gradients through interpolate + grid_sample,
and `edge_grad_estimator` adds the gradient a discontinuity contributes -- a silhouette or an occlusion boundary moves
when the occluder's vertices move -- as drtk.edge_grad_estimator does (identity in the forward).  These are host-side
PyTorch on top of the HIP rasterizer's images (one image per frame: not a hot loop).  drtk's source is absent: the
estimator's conventions are stated in its docstring and checked against finite differences of a 16x supersampled
render (tests/test_mesh_edge_grad.py) -- PARITY UNPINNED like the forward.
"""
import ctypes
from typing import List, Optional

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import c_int, fptr, iptr, stream_ptr


def transform(verts: torch.Tensor, K: torch.Tensor, Rt: torch.Tensor) -> torch.Tensor:
    """verts[B,V,3] (world), K[B,3,3], Rt[B,3,4] -> v_pix[B,V,3] = (pixel x, pixel y, camera-space z)."""
    v_cam = verts @ Rt[:, :3, :3].transpose(1, 2) + Rt[:, None, :3, 3]
    z = v_cam[..., 2:3]
    uv = (v_cam / z.clamp(min=1e-8)) @ K.transpose(1, 2)
    return torch.cat([uv[..., :2], z], dim=-1)


def rasterize(v_pix: torch.Tensor, vi: torch.Tensor, height: int, width: int, with_bary: bool = True):
    """v_pix[B,V,3], vi[F,3] -> index_img[B,H,W] int32 (-1 = empty), depth_img[B,H,W] (0 = empty),
    bary_img[B,3,H,W] (perspective-correct; None unless with_bary)."""
    if not v_pix.is_cuda:
        raise _lib.GoliathHipError("rasterize needs CUDA(HIP) tensors; there is no CPU path")
    v_pix = v_pix.detach().to(torch.float32).contiguous()
    vi = vi.to(device=v_pix.device, dtype=torch.int32).contiguous()
    B, V = v_pix.shape[:2]
    Fc = vi.shape[0]
    dev = v_pix.device
    index_img = torch.empty(B, height, width, dtype=torch.int32, device=dev)
    depth_img = torch.empty(B, height, width, device=dev)
    bary_img = torch.empty(B, 3, height, width, device=dev) if with_bary else None
    fn = _lib.load().gol_mesh_raster_workspace_bytes
    fn.restype = ctypes.c_int64
    ws = torch.empty(max(int(fn(c_int(B), c_int(Fc))), 4) // 4, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        _lib.call("gol_mesh_raster", c_int(B), c_int(V), c_int(Fc), c_int(height), c_int(width), fptr(v_pix), iptr(vi),
                  iptr(index_img), fptr(depth_img), fptr(bary_img), iptr(ws), stream_ptr())
    return index_img, depth_img, bary_img


def interpolate(attr: torch.Tensor, ati: torch.Tensor, index_img: torch.Tensor, bary_img: torch.Tensor) -> torch.Tensor:
    """drtk.interpolate: per-vertex attributes attr[B,Va,C] with their own face table ati[F,3] -> [B,C,H,W]."""
    B, H, W = index_img.shape
    idx = index_img.clamp(min=0).long().reshape(B, -1)                      # [B,P]
    tri = ati.long()[idx]                                                    # [B,P,3]
    C = attr.shape[-1]
    vals = torch.gather(attr, 1, tri.reshape(B, -1, 1).expand(-1, -1, C)).reshape(B, -1, 3, C)   # [B,P,3,C]
    out = (vals * bary_img.reshape(B, 3, -1).permute(0, 2, 1)[..., None]).sum(2)  # [B,P,C]
    out = out * (index_img.reshape(B, -1, 1) >= 0)
    return out.permute(0, 2, 1).reshape(B, -1, H, W)


def render(v_pix: torch.Tensor, vi: torch.Tensor, index_img: torch.Tensor):
    """drtk.render (render_drtk.py:45): depth_img[B,H,W] and bary_img[B,3,H,W] of the faces in index_img as DIFFERENTIABLE
    functions of v_pix[B,V,3] (visibility fixed) -- the arithmetic of csrc/meshraster.hip: barycentrics anchored at the face's
    first vertex, sample at the pixel centre (j + 0.5, i + 0.5), perspective-correct (linear in 1 / z); 0 where no face."""
    B, H, W = index_img.shape
    hit = index_img >= 0
    tri = vi.long()[index_img.clamp(min=0).long()]                                 # [B,H,W,3] vertex ids
    P = v_pix[torch.arange(B, device=v_pix.device)[:, None, None, None], tri]      # [B,H,W,3,3]: (x, y, z) of a, b, c
    a, b, c = P[..., 0, :], P[..., 1, :], P[..., 2, :]
    px = torch.arange(W, device=v_pix.device, dtype=v_pix.dtype)[None, None, :] + 0.5
    py = torch.arange(H, device=v_pix.device, dtype=v_pix.dtype)[None, :, None] + 0.5
    area = (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])
    area = torch.where(hit, area, torch.ones_like(area))
    dx, dy = px - a[..., 0], py - a[..., 1]
    b1 = ((c[..., 1] - a[..., 1]) * dx + (a[..., 0] - c[..., 0]) * dy) / area
    b2 = ((a[..., 1] - b[..., 1]) * dx + (b[..., 0] - a[..., 0]) * dy) / area
    b0 = 1.0 - b1 - b2
    w = torch.stack([b0 / a[..., 2], b1 / b[..., 2], b2 / c[..., 2]], 1)            # [B,3,H,W]
    iz = w.sum(1)
    iz = torch.where(hit, iz, torch.ones_like(iz))
    depth = torch.where(hit, 1.0 / iz, torch.zeros_like(iz))
    bary = torch.where(hit[:, None], w / iz[:, None], torch.zeros_like(w))
    return depth, bary


class _EdgeGrad(torch.autograd.Function):
    """drtk.edge_grad_estimator (render_drtk.py:64-70): identity on `img`; the backward gives v_pix the gradient that the
    image's DISCONTINUITIES carry.  Convention (stated, drtk's source is absent):
      * a discontinuity lies between two horizontally or vertically adjacent pixel centres p, q whose faces differ and do not
        share a mesh edge (two faces with a common edge continue each other: no discontinuity) -- one of them may be empty;
      * it is the edge of the OCCLUDER (the face nearer to the camera; an empty pixel never occludes) that crosses the
        segment p-q; its crossing point x* along the segment is a differentiable function of that edge's two vertices;
      * moving x* towards q by d extends p's colour over the strip d: with box-filtered pixels
        d loss / d x* = <(g_p + g_q) / 2, img_p - img_q>  (g = upstream gradient), chained into the edge's vertices;
      * rows and columns each see the whole displacement of an edge: the horizontal crossings are weighted with n_x^2, the
        vertical ones with n_y^2 (n = the edge's unit normal)."""

    @staticmethod
    def forward(ctx, v_pix, vi, img, index_img, depth_img):
        ctx.save_for_backward(v_pix, vi, img, index_img, depth_img)
        return img.view_as(img)

    @staticmethod
    def backward(ctx, g):
        v_pix, vi, img, index_img, depth_img = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, g, None, None
        B, H, W = index_img.shape
        vi = vi.long()
        inf = torch.full_like(depth_img, float("inf"))
        z = torch.where(index_img >= 0, depth_img, inf)
        leaf = v_pix.detach().requires_grad_(True)
        total = leaf.new_zeros(())
        with torch.enable_grad():
            for axis in (0, 1):   # 0: q is the right neighbour (crossing along x), 1: q is the lower neighbour (along y)
                sl_p = (slice(None), slice(None), slice(0, W - 1)) if axis == 0 else (slice(None), slice(0, H - 1), slice(None))
                sl_q = (slice(None), slice(None), slice(1, W)) if axis == 0 else (slice(None), slice(1, H), slice(None))
                ip, iq = index_img[sl_p], index_img[sl_q]
                cand = (ip != iq)
                # (torch.nonzero is the one host sync of this backward -- the candidate count sizes every tensor below; an
                # empty candidate set flows through as zero-length tensors, no second sync on `.any()`)
                bb, ii, jj = torch.nonzero(cand, as_tuple=True)
                if bb.numel() == 0:
                    continue
                fp, fq = ip[bb, ii, jj].long(), iq[bb, ii, jj].long()
                tp, tq = vi[fp.clamp(min=0)], vi[fq.clamp(min=0)]                          # [n,3]
                shared = (tp[:, :, None] == tq[:, None, :]).any(2).sum(1)
                keep = ~((fp >= 0) & (fq >= 0) & (shared >= 2))
                zp, zq = z[sl_p][bb, ii, jj], z[sl_q][bb, ii, jj]
                occ_is_p = zp <= zq
                # (no compaction by `keep`: boolean indexing would be a second host sync; the dropped candidates -- two faces
                # that share a mesh edge continue each other -- get coefficient 0 below)
                keep_w = keep.to(leaf.dtype)
                tri = torch.where(occ_is_p[:, None], tp, tq)                               # occluder's vertex ids [n,3]
                P = leaf[bb[:, None], tri]                                                 # [n,3,3]
                # along = coordinate that varies from p to q, across = the fixed one
                al, ac = (0, 1) if axis == 0 else (1, 0)
                c_fix = (ii if axis == 0 else jj).to(leaf.dtype) + 0.5                     # y of the row / x of the column
                s_p = (jj if axis == 0 else ii).to(leaf.dtype) + 0.5                       # coordinate of p along the segment
                e0, e1 = P, P.roll(-1, 1)                                                   # the three edges (a-b, b-c, c-a)
                d_ac = e1[..., ac] - e0[..., ac]
                crosses = ((e0[..., ac] - c_fix[:, None]) * (e1[..., ac] - c_fix[:, None]) <= 0) & (d_ac != 0)
                t = (c_fix[:, None] - e0[..., ac]) / torch.where(d_ac != 0, d_ac, torch.ones_like(d_ac))
                xs = e0[..., al] + t * (e1[..., al] - e0[..., al])                         # [n,3] crossing points
                dist = torch.where(crosses, (xs.detach() - (s_p[:, None] + 0.5)).abs(), torch.full_like(xs, float("inf")))
                best = dist.argmin(1)
                ok = dist.gather(1, best[:, None])[:, 0] <= 1.0     # the crossing lies within a pixel of the segment's middle
                x_star = xs.gather(1, best[:, None])[:, 0]
                cp = img[:, :, sl_p[1], sl_p[2]][bb, :, ii, jj]                            # [n,C]
                cq = img[:, :, sl_q[1], sl_q[2]][bb, :, ii, jj]
                gp = g[:, :, sl_p[1], sl_p[2]][bb, :, ii, jj]
                gq = g[:, :, sl_q[1], sl_q[2]][bb, :, ii, jj]
                # every crossing direction by itself accounts for the whole strip an edge sweeps (an edge of length L and
                # normal n crosses L |n_x| rows, its crossing point moves by d / n_x per row: L d in total; the same for the
                # columns), so the two are blended with n_x^2 + n_y^2 = 1: each direction counts where it is well conditioned
                d_al = (e1[..., al] - e0[..., al]).gather(1, best[:, None])[:, 0].detach()
                d_ac_b = d_ac.gather(1, best[:, None])[:, 0].detach()
                weight = d_ac_b * d_ac_b / (d_ac_b * d_ac_b + d_al * d_al).clamp(min=1e-30)
                coef = (0.5 * (gp + gq) * (cp - cq)).sum(1) * ok.to(leaf.dtype) * weight * keep_w
                total = total + (coef.detach() * torch.where(ok & keep, x_star, torch.zeros_like(x_star))).sum()
                # discontinuities whose occluder edge does not cross within a pixel get NO gradient: counted -- opt-in
                # (GOLIATH_EDGE_STATS=1 or meshraster.COLLECT_EDGE_STATS = True), per device, on the device (no extra sync)
                if COLLECT_EDGE_STATS:
                    st = EDGE_STATS.setdefault(leaf.device, {"edges": None, "dropped": None})
                    n_e, n_d = keep.sum(), (keep & ~ok).sum()
                    st["edges"] = n_e if st["edges"] is None else st["edges"] + n_e
                    st["dropped"] = n_d if st["dropped"] is None else st["dropped"] + n_d
            if total.requires_grad:
                (gv,) = torch.autograd.grad(total, leaf)
            else:
                gv = torch.zeros_like(leaf)
        return gv, None, g, None, None


# Opt-in running totals of the backward passes, keyed by DEVICE (a second GPU's backward must not add into cuda:0's tensors):
# EDGE_STATS[device] = {"edges": discontinuities seen, "dropped": those without a crossing occluder edge within a pixel (no
# gradient)}, both 0-dim device tensors.  Off by default (an extra reduction per backward and a process-global mutation nobody
# may read); reset with EDGE_STATS.clear().
import os as _os

COLLECT_EDGE_STATS = _os.environ.get("GOLIATH_EDGE_STATS", "0") == "1"
EDGE_STATS = {}


def edge_grad_estimator(v_pix, vi, bary_img, img, index_img, depth_img=None):
    """drtk.edge_grad_estimator (same arguments; depth_img: the rasterizer's depth image, recomputed from bary_img-free
    data when omitted)."""
    if depth_img is None:
        depth_img = render(v_pix.detach(), vi, index_img)[0]
    return _EdgeGrad.apply(v_pix, vi, img, index_img, depth_img.detach())


class RenderLayer(torch.nn.Module):
    """render_drtk.RenderLayer (ca_code/utils/render_drtk.py:14-82) with the same constructor, forward arguments and
    output dict."""

    def __init__(self, h, w, vi, vt, vti, flip_uvs=False):
        super().__init__()
        self.h, self.w = h, w
        self.register_buffer("vi", vi, persistent=False)
        self.register_buffer("vt", vt.clone(), persistent=False)
        self.register_buffer("vti", vti, persistent=False)
        self.flip_uvs = flip_uvs
        if flip_uvs:
            self.vt[:, 1] = 1 - self.vt[:, 1]
        self.register_buffer("image_size", torch.as_tensor([h, w], dtype=torch.int32))

    def forward(self, verts: torch.Tensor, tex: torch.Tensor, K: torch.Tensor, Rt: torch.Tensor,
                background: Optional[torch.Tensor] = None, output_filters: Optional[List[str]] = None,
                edge_grad: bool = True):
        assert output_filters is None
        assert background is None
        v_pix = transform(verts, K=K, Rt=Rt)
        index_img, depth_img, bary_img = rasterize(v_pix, self.vi, self.h, self.w)
        need_vert_grad = torch.is_grad_enabled() and v_pix.requires_grad
        if need_vert_grad:
            # the same depth / barycentrics as differentiable functions of v_pix (visibility from the rasterizer, fixed)
            depth_img, bary_img = render(v_pix, self.vi, index_img)
        vt_img = interpolate((self.vt * 2.0 - 1.0)[None].expand(verts.shape[0], -1, -1), self.vti, index_img, bary_img)
        mask = (index_img != -1)[:, None].float()
        img = F.grid_sample(tex, vt_img.permute(0, 2, 3, 1), mode="bilinear", align_corners=False) * mask
        if edge_grad and need_vert_grad:
            img = edge_grad_estimator(v_pix, self.vi, bary_img, img, index_img, depth_img)
        return {"render": img, "depth_img": depth_img, "v_pix": v_pix, "vt_img": vt_img, "index_img": index_img,
                "bary_img": bary_img, "mask": mask}


# ---- fused HIP textured render (csrc/meshrender.hip) ---------------------------------------------------------------------
# One marshaller per C-ABI entry (keywords = the header's parameter names; a pointer is a GPU tensor, checked, a device
# address or None; stream = the current one).
_F32, _I32 = torch.float32, torch.int32


def _p(x, dtype=_F32, name="tensor"):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else _lib.ptr(x, dtype, name)


def _abi_mesh_render_fwd(*, B, F, Vt, C, H, W, Ht, Wt, vt, vti, tex, index_img, bary_img, vt_img, render, mask):
    _lib.call("gol_mesh_render_fwd", c_int(B), c_int(F), c_int(Vt), c_int(C), c_int(H), c_int(W), c_int(Ht), c_int(Wt),
              _p(vt), _p(vti, _I32), _p(tex), _p(index_img, _I32), _p(bary_img), _p(vt_img), _p(render), _p(mask),
              stream_ptr())


def _abi_mesh_render_bwd(*, B, V, F, Vt, C, H, W, Ht, Wt, v_pix, vi, vt, vti, tex, index_img, bary_img, g_render=None,
                         g_vt_img=None, g_bary_img=None, g_depth_img=None, g_tex=None, g_v_pix=None):
    _lib.call("gol_mesh_render_bwd", c_int(B), c_int(V), c_int(F), c_int(Vt), c_int(C), c_int(H), c_int(W), c_int(Ht),
              c_int(Wt), _p(v_pix), _p(vi, _I32), _p(vt), _p(vti, _I32), _p(tex), _p(index_img, _I32), _p(bary_img),
              _p(g_render), _p(g_vt_img), _p(g_bary_img), _p(g_depth_img), _p(g_tex), _p(g_v_pix), stream_ptr())


def _abi_mesh_render_edge_bwd(*, B, V, F, C, H, W, v_pix, vi, index_img, depth_img, render, g_render, g_v_pix,
                              edge_stats=None):
    _lib.call("gol_mesh_render_edge_bwd", c_int(B), c_int(V), c_int(F), c_int(C), c_int(H), c_int(W), _p(v_pix),
              _p(vi, _I32), _p(index_img, _I32), _p(depth_img), _p(render), _p(g_render), _p(g_v_pix),
              _p(edge_stats, _I32), stream_ptr())


def _f32(t):
    return None if t is None else t.detach().to(torch.float32).contiguous()


class _RenderTextured(torch.autograd.Function):
    """render_textured's forward and backward on the HIP kernels (no host sync: graph-capturable)."""

    @staticmethod
    def forward(ctx, v_pix, vi, vt, vti, tex, index_img, depth_img, bary_img, edge_grad):
        B, H, W = index_img.shape
        C, Ht, Wt = tex.shape[1:]
        dev = v_pix.device
        vi32, vti32 = vi.to(torch.int32).contiguous(), vti.to(torch.int32).contiguous()
        vt32, tex32 = _f32(vt), _f32(tex)
        idx32, depth32, bary32 = index_img.to(torch.int32).contiguous(), _f32(depth_img), _f32(bary_img)
        vt_img = torch.empty(B, 2, H, W, device=dev)
        render = torch.empty(B, C, H, W, device=dev)
        mask = torch.empty(B, 1, H, W, device=dev)
        with _lib.device_guard(dev):
            _abi_mesh_render_fwd(B=B, F=vti32.shape[0], Vt=vt32.shape[0], C=C, H=H, W=W, Ht=Ht, Wt=Wt, vt=vt32, vti=vti32,
                                 tex=tex32, index_img=idx32, bary_img=bary32, vt_img=vt_img, render=render, mask=mask)
        ctx.save_for_backward(_f32(v_pix), vi32, vt32, vti32, tex32, idx32, depth32, bary32, render)
        ctx.edge_grad = bool(edge_grad)
        ctx.dtypes = (v_pix.dtype, tex.dtype)
        ctx.mark_non_differentiable(mask)
        # depth / barycentrics pass through unchanged: the backward chains their gradients into v_pix
        return render, vt_img, depth_img.view_as(depth_img), bary_img.view_as(bary_img), mask

    @staticmethod
    def backward(ctx, g_render, g_vt_img, g_depth_img, g_bary_img, _g_mask):
        v_pix, vi, vt, vti, tex, index_img, depth_img, bary_img, render = ctx.saved_tensors
        need_v, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[4]
        g_v = torch.zeros_like(v_pix) if need_v else None
        g_t = torch.zeros_like(tex) if need_t else None
        g_render, g_vt_img, g_depth_img, g_bary_img = (_f32(g) for g in (g_render, g_vt_img, g_depth_img, g_bary_img))
        B, H, W = index_img.shape
        C, Ht, Wt = tex.shape[1:]
        V, F = v_pix.shape[1], vi.shape[0]
        with _lib.device_guard(v_pix.device):
            if need_v or need_t:
                _abi_mesh_render_bwd(B=B, V=V, F=F, Vt=vt.shape[0], C=C, H=H, W=W, Ht=Ht, Wt=Wt, v_pix=v_pix, vi=vi, vt=vt,
                                     vti=vti, tex=tex, index_img=index_img, bary_img=bary_img, g_render=g_render,
                                     g_vt_img=g_vt_img if need_v else None, g_bary_img=g_bary_img if need_v else None,
                                     g_depth_img=g_depth_img if need_v else None, g_tex=g_t, g_v_pix=g_v)
            if need_v and ctx.edge_grad and g_render is not None:
                stats = torch.zeros(2, dtype=torch.int32, device=v_pix.device) if COLLECT_EDGE_STATS else None
                _abi_mesh_render_edge_bwd(B=B, V=V, F=F, C=C, H=H, W=W, v_pix=v_pix, vi=vi, index_img=index_img,
                                          depth_img=depth_img, render=render, g_render=g_render, g_v_pix=g_v,
                                          edge_stats=stats)
                if stats is not None:   # _EdgeGrad's counters, same meaning, on the device
                    st = EDGE_STATS.setdefault(v_pix.device, {"edges": None, "dropped": None})
                    n_e, n_d = stats[0].long(), stats[1].long()
                    st["edges"] = n_e if st["edges"] is None else st["edges"] + n_e
                    st["dropped"] = n_d if st["dropped"] is None else st["dropped"] + n_d
        g_v = None if g_v is None else g_v.to(ctx.dtypes[0])
        g_t = None if g_t is None else g_t.to(ctx.dtypes[1])
        return g_v, None, None, None, g_t, None, None, None, None


def render_textured(v_pix, vi, vt, vti, tex, index_img, depth_img, bary_img, edge_grad=False):
    """RenderLayer's textured render after the rasterizer as ONE fused HIP op (csrc/meshrender.hip).

    v_pix[B,V,3], vi[F,3], vt[Vt,2] (uv in [0, 1]), vti[F,3], tex[B,C,Ht,Wt]; index_img[B,H,W], depth_img[B,H,W] and
    bary_img[B,3,H,W] as `rasterize` returns them.  Returns (render[B,C,H,W], vt_img[B,2,H,W], depth_img, bary_img,
    mask[B,1,H,W]) with RenderLayer's values: render = grid_sample(tex, vt_img, bilinear, align_corners=False, zero
    padding) * mask.  Differentiable outputs: render, vt_img, depth_img and bary_img; gradients go to tex and to v_pix
    (through the function `render()` evaluates, visibility fixed) and, with edge_grad, v_pix also receives `_EdgeGrad`'s
    discontinuity term.  vi, vt, vti and the images get none.  Every tensor must be on the GPU: there is no CPU path."""
    for name, t in (("v_pix", v_pix), ("vi", vi), ("vt", vt), ("vti", vti), ("tex", tex), ("index_img", index_img),
                    ("depth_img", depth_img), ("bary_img", bary_img)):
        if not t.is_cuda:
            raise _lib.GoliathHipError(f"render_textured: {name} must be a CUDA(HIP) tensor; there is no CPU path")
    if tex.shape[0] != v_pix.shape[0] or index_img.shape[0] != v_pix.shape[0]:
        raise _lib.GoliathHipError("render_textured: v_pix, tex and the images need the same batch size")
    return _RenderTextured.apply(v_pix, vi, vt, vti, tex, index_img, depth_img, bary_img, edge_grad)


class FusedRenderLayer(RenderLayer):
    """RenderLayer (same constructor, forward arguments and output dict) with everything after the rasterizer in one fused
    HIP forward and backward (`render_textured`): no [B,H,W,3,3] gathers and no host sync in the backward, so a training
    step through it can be captured as a graph.  Its numbers are RenderLayer's up to fp32 arithmetic and float-atomic
    order; EDGE_STATS counts with the same meaning."""

    def forward(self, verts: torch.Tensor, tex: torch.Tensor, K: torch.Tensor, Rt: torch.Tensor,
                background: Optional[torch.Tensor] = None, output_filters: Optional[List[str]] = None,
                edge_grad: bool = True):
        assert output_filters is None
        assert background is None
        v_pix = transform(verts, K=K, Rt=Rt)
        index_img, depth_img, bary_img = rasterize(v_pix, self.vi, self.h, self.w)
        need_vert_grad = torch.is_grad_enabled() and v_pix.requires_grad
        img, vt_img, depth_img, bary_img, mask = render_textured(v_pix, self.vi, self.vt, self.vti, tex, index_img,
                                                                 depth_img, bary_img, edge_grad=edge_grad and need_vert_grad)
        return {"render": img, "depth_img": depth_img, "v_pix": v_pix, "vt_img": vt_img, "index_img": index_img,
                "bary_img": bary_img, "mask": mask}
