"""Primitive assembly of the MVP hand model (BASELINE config 5) on the HIP kernels of csrc/mvpprims.hip: what
`hand_mvp.AutoEncoder` does between its decoders and the ray march.

  prim_slots(valid_prims, compact=True) -> (slot, live, Kv)
      the two int32 tables of gol_mvp_template_*, built once per mask and cached on its device
  assemble_template(primrgb, primalpha, primsize, valid_prims=None, compact=True, rgb_affine=None, relu=False, full=False)
      ca_code/models/hand_mvp.py:171-185 (cat / view / permute / reshape of the decoder slabs) with the valid_prims
      selection of ca_code/utils/render_raymarcher.py:41-47 folded in: one read of the slabs, one write of the template,
      forward and backward (an autograd Function)
  prim_transforms(posbase, rotbase, delta_pos, delta_rvec, delta_scale, prim_scale)
      hand_mvp.py:410-425 with axisangle_to_matrix (:477-510): one launch forward, one backward
  hand_mvp_render(self, K, Rt, preds, with_shadow=False)      <- hand_mvp.AutoEncoder.render (:162-205)
  geom_decoder_forward(self, pose, joint, iteration=-1)       <- hand_mvp.GeomDecoder.forward (:386-444)
      installed by goliath_amd.dropin.patch_hand_mvp()

Everything runs on the current stream; after the tables of a mask exist no call waits for the device.  There is no CPU
path.
"""
import sys
import weakref

import torch
import torch.nn.functional as F

from . import _lib, mvp
from ._lib import c_float, c_int, fptr, iptr, stream_ptr

FULL_TEMPLATE_FLAG = "_goliath_full_template"   # set on AutoEncoder by dropin.patch_hand_mvp(full_template=True)


# ------------------------------------------------------------------------------------------------------- ABI marshallers
def _abi_mvp_template_fwd(*, B, TD, TH, TW, ny, nx, rgb, alpha, slot, live, Kout, act, rgb_scale, rgb_shift, out, out_full):
    _lib.call("gol_mvp_template_fwd", c_int(B), c_int(TD), c_int(TH), c_int(TW), c_int(ny), c_int(nx), _p(rgb), _p(alpha),
              _p(slot, iptr), _p(live, iptr), c_int(Kout), c_int(act), c_float(rgb_scale), c_float(rgb_shift), _p(out),
              _p(out_full), stream_ptr())


def _abi_mvp_template_bwd(*, B, TD, TH, TW, ny, nx, rgb, alpha, slot, live, Kout, act, rgb_scale, rgb_shift, g_out,
                          g_out_full, g_rgb, g_alpha):
    _lib.call("gol_mvp_template_bwd", c_int(B), c_int(TD), c_int(TH), c_int(TW), c_int(ny), c_int(nx), _p(rgb), _p(alpha),
              _p(slot, iptr), _p(live, iptr), c_int(Kout), c_int(act), c_float(rgb_scale), c_float(rgb_shift), _p(g_out),
              _p(g_out_full), _p(g_rgb), _p(g_alpha), stream_ptr())


def _abi_mvp_primtransf_fwd(*, B, K, posbase, rotbase, delta_pos, delta_rvec, delta_scale, prim_scale, primpos, primrot,
                            primscale):
    _lib.call("gol_mvp_primtransf_fwd", c_int(B), c_int(K), _p(posbase), _p(rotbase), _p(delta_pos), _p(delta_rvec),
              _p(delta_scale), c_float(prim_scale), _p(primpos), _p(primrot), _p(primscale), stream_ptr())


def _abi_mvp_primtransf_bwd(*, B, K, rotbase, delta_rvec, prim_scale, g_primpos, g_primrot, g_primscale, g_delta_pos,
                            g_delta_rvec, g_delta_scale):
    _lib.call("gol_mvp_primtransf_bwd", c_int(B), c_int(K), _p(rotbase), _p(delta_rvec), c_float(prim_scale), _p(g_primpos),
              _p(g_primrot), _p(g_primscale), _p(g_delta_pos), _p(g_delta_rvec), _p(g_delta_scale), stream_ptr())


def _p(x, typed=fptr):
    import ctypes

    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else typed(x)


def _need_gpu(name, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.GoliathHipError(f"{name} needs CUDA(HIP) tensors; there is no CPU path")


def _f32c(t):
    """float32, contiguous, same storage where it already is both."""
    return t.to(torch.float32).contiguous()


def _aligned16(t):
    """The template side is read and written as 16-byte vectors: a gradient that arrives at an odd address is copied."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


# ---------------------------------------------------------------------------------------------------------- slot tables
class _Tables:
    __slots__ = ("ref", "version", "slot", "live", "Kv", "index")


_TABLES = {}   # (data_ptr, device, compact) -> _Tables, valid while the mask tensor it was built from is alive and unwritten


def _tables(valid_prims, compact=True):
    if not torch.is_tensor(valid_prims) or valid_prims.dim() != 1:
        raise ValueError("valid_prims must be a 1-D mask tensor [K]")
    key = (valid_prims.data_ptr(), str(valid_prims.device), bool(compact))
    hit = _TABLES.get(key)
    if hit is not None and hit.ref() is valid_prims and hit.version == valid_prims._version:
        return hit
    with torch.no_grad():
        keep = valid_prims != 0
        K = keep.numel()
        t = _Tables()
        t.ref, t.version = weakref.ref(valid_prims), valid_prims._version
        if compact:
            # compaction, what Raymarcher's template[:, valid_prims] does: the j-th valid primitive goes to slot j
            t.slot = torch.where(keep, torch.cumsum(keep, 0) - 1, -1).to(torch.int32)
            t.live = None
            t.index = torch.nonzero(keep)[:, 0]           # the one host sync, once per mask
            t.Kv = int(t.index.numel())
        else:
            # every primitive keeps its place; an invalid one is written as zeros (valid_prims * primalpha)
            t.slot = torch.arange(K, dtype=torch.int32, device=keep.device)
            t.live = keep.to(torch.int32)
            t.index = None
            t.Kv = K
    for k in [k for k, v in _TABLES.items() if v.ref() is None]:
        del _TABLES[k]
    _TABLES[key] = t
    return t


def prim_slots(valid_prims, compact=True):
    """(slot[K] int32, live[K] int32 or None, Kv) of a primitive mask (non-zero = valid), on the mask's device.
    compact=True: slot = the primitive's rank among the valid ones, -1 for an invalid one; Kv = their number (what
    `template[:, valid_prims]` keeps).  compact=False: identity slots, live = the mask, Kv = K.  Cached per (data_ptr,
    device) with a weak reference to the mask and its version counter: building the compact table is the only place that
    waits for the device, once per mask."""
    t = _tables(valid_prims, compact)
    return t.slot, t.live, t.Kv


# ---------------------------------------------------------------------------------------------------- template assembly
def _geometry(primrgb, primalpha, primsize):
    TW, TH, TD = (int(v) for v in primsize)      # the reference's primsize is (x, y, z)
    if min(TW, TH, TD) < 1:
        raise ValueError("primsize must be positive")
    if not torch.is_tensor(primalpha) or primalpha.dim() not in (4, 5):
        raise ValueError("primalpha must be [B,TD,1,Sy,Sx] (or [B,TD,Sy,Sx])")
    if primalpha.dim() == 5 and primalpha.shape[2] != 1:
        raise ValueError("primalpha must have one channel")
    B, Sy, Sx = primalpha.shape[0], primalpha.shape[-2], primalpha.shape[-1]
    if primalpha.shape[1] != TD or Sy % TH or Sx % TW:
        raise ValueError(f"primalpha {tuple(primalpha.shape)} does not tile into primitives of size {(TW, TH, TD)}")
    if primrgb is not None:
        if not torch.is_tensor(primrgb) or tuple(primrgb.shape) != (B, TD, 3, Sy, Sx):
            raise ValueError(f"primrgb must be [B,TD,3,Sy,Sx] = {(B, TD, 3, Sy, Sx)}")
        if primrgb.dtype != primalpha.dtype:
            raise ValueError("primrgb and primalpha must have the same dtype")
    if not primalpha.dtype.is_floating_point:
        raise ValueError("the slabs must be floating point")
    return B, TD, TH, TW, Sy // TH, Sx // TW


class _Assemble(torch.autograd.Function):
    @staticmethod
    def forward(ctx, primrgb, primalpha, geom, slot, live, Kout, affine, relu, full):
        B, TD, TH, TW, ny, nx = geom
        rgb = None if primrgb is None else _f32c(primrgb.detach())
        alpha = _f32c(primalpha.detach())
        C = 1 if rgb is None else 4
        shape = (TD, TH, TW) if C == 1 else (TD, TH, TW, C)
        dev = alpha.device
        out = torch.empty((B, Kout, *shape), dtype=torch.float32, device=dev)
        out_full = torch.empty((B, ny * nx, *shape), dtype=torch.float32, device=dev) if full else None
        act = bool(relu or affine is not None)
        scale, shift = (1.0, 0.0) if affine is None else (float(affine[0]), float(affine[1]))
        ctx.args = dict(B=B, TD=TD, TH=TH, TW=TW, ny=ny, nx=nx, slot=slot, live=live, Kout=Kout, act=int(act),
                        rgb_scale=scale, rgb_shift=shift)
        ctx.has_rgb, ctx.full, ctx.dtype = rgb is not None, full, primalpha.dtype
        ctx.alpha_shape = primalpha.shape
        ctx.save_for_backward(*((rgb, alpha) if act else ()))
        if B and (Kout or full):
            with _lib.device_guard(dev):
                _abi_mvp_template_fwd(rgb=rgb, alpha=alpha, out=out if Kout else None, out_full=out_full, **ctx.args)
        out = out.to(primalpha.dtype)
        if full:
            return out, out_full.to(primalpha.dtype)
        return out

    @staticmethod
    def backward(ctx, g_out, g_full=None):
        a = ctx.args
        rgb, alpha = ctx.saved_tensors if a["act"] else (None, None)
        B, TD, ny, nx = a["B"], a["TD"], a["ny"], a["nx"]
        Sy, Sx = ny * a["TH"], nx * a["TW"]
        dev = g_out.device if g_out is not None else g_full.device
        g_out = None if g_out is None or a["Kout"] == 0 else _aligned16(_f32c(g_out))
        g_full = None if g_full is None else _aligned16(_f32c(g_full))
        g_rgb = torch.empty((B, TD, 3, Sy, Sx), dtype=torch.float32, device=dev) if ctx.has_rgb else None
        g_alpha = torch.empty(ctx.alpha_shape, dtype=torch.float32, device=dev)
        if g_out is None and g_full is None:     # nothing came back (Kv = 0): zeros without a launch
            g_alpha.zero_()
            if g_rgb is not None:
                g_rgb.zero_()
        elif B:
            with _lib.device_guard(dev):
                _abi_mvp_template_bwd(rgb=rgb, alpha=alpha, g_out=g_out, g_out_full=g_full, g_rgb=g_rgb, g_alpha=g_alpha,
                                      **a)
        need_rgb = ctx.has_rgb and ctx.needs_input_grad[0]
        return (g_rgb.to(ctx.dtype) if need_rgb else None, g_alpha.to(ctx.dtype) if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None, None)


def assemble_template(primrgb, primalpha, primsize, valid_prims=None, compact=True, rgb_affine=None, relu=False, full=False):
    """Decoder slabs -> channels-last primitive template, differentiable w.r.t. both slabs.

    primrgb[B,TD,3,Sy,Sx] or None, primalpha[B,TD,1,Sy,Sx] (or [B,TD,Sy,Sx]); primsize = (TW, TH, TD), the reference's
    (x, y, z) order.  Returns template[B,K',TD,TH,TW,4] -- with primrgb=None the one-channel [B,K',TD,TH,TW] -- where
    valid_prims=None keeps all K = ny nx primitives, a mask with compact=True keeps the valid ones in order (K' = Kv,
    `template[:, valid_prims]`), and compact=False keeps all K with the invalid ones zeroed (`valid_prims * template`).
    rgb_affine=(scale, shift) applies relu(scale x + shift) to the colour slabs and relu(x) to alpha on the way through
    (for callers that hand over the raw decoder output); relu=True the same with the colours' scale 1, shift 0.
    full=True also returns the full-K template with all data (the reference's preds["primrgba"]) from the same loads.
    Non-contiguous input is made contiguous first; float32 compute, the result has the input's dtype."""
    geom = _geometry(primrgb, primalpha, primsize)
    B, TD, TH, TW, ny, nx = geom
    if rgb_affine is not None and len(rgb_affine) != 2:
        raise ValueError("rgb_affine must be (scale, shift)")
    if valid_prims is not None:
        if not torch.is_tensor(valid_prims) or valid_prims.dim() != 1 or valid_prims.numel() != ny * nx:
            raise ValueError(f"valid_prims must be a mask of the {ny * nx} primitives")
    _need_gpu("assemble_template", primrgb, primalpha, valid_prims)
    if valid_prims is None:
        slot, live, Kout = None, None, ny * nx
    else:
        slot, live, Kout = prim_slots(valid_prims, compact)
    return _Assemble.apply(primrgb, primalpha, geom, slot, live, Kout, rgb_affine, bool(relu), bool(full))


# -------------------------------------------------------------------------------------------------- primitive transforms
class _PrimTransforms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, posbase, rotbase, delta_pos, delta_rvec, delta_scale, prim_scale):
        B, K = delta_pos.shape[:2]
        dtype, dev = delta_pos.dtype, delta_pos.device
        posbase, rotbase, delta_pos, delta_rvec, delta_scale = (_f32c(t.detach()) for t in
                                                                (posbase, rotbase, delta_pos, delta_rvec, delta_scale))
        primpos = torch.empty(B, K, 3, dtype=torch.float32, device=dev)
        primrot = torch.empty(B, K, 3, 3, dtype=torch.float32, device=dev)
        primscale = torch.empty(B, K, 3, dtype=torch.float32, device=dev)
        if B * K:
            with _lib.device_guard(dev):
                _abi_mvp_primtransf_fwd(B=B, K=K, posbase=posbase, rotbase=rotbase, delta_pos=delta_pos,
                                        delta_rvec=delta_rvec, delta_scale=delta_scale, prim_scale=prim_scale,
                                        primpos=primpos, primrot=primrot, primscale=primscale)
        ctx.save_for_backward(rotbase, delta_rvec)
        ctx.prim_scale, ctx.dtype = prim_scale, dtype
        return primpos.to(dtype), primrot.to(dtype), primscale.to(dtype)

    @staticmethod
    def backward(ctx, g_pos, g_rot, g_scale):
        rotbase, delta_rvec = ctx.saved_tensors
        B, K = delta_rvec.shape[:2]
        dev = delta_rvec.device
        g_pos, g_rot, g_scale = (None if g is None else _f32c(g) for g in (g_pos, g_rot, g_scale))
        out = [torch.empty(B, K, 3, dtype=torch.float32, device=dev) for _ in range(3)]
        if B * K:
            with _lib.device_guard(dev):
                _abi_mvp_primtransf_bwd(B=B, K=K, rotbase=rotbase, delta_rvec=delta_rvec, prim_scale=ctx.prim_scale,
                                        g_primpos=g_pos, g_primrot=g_rot, g_primscale=g_scale, g_delta_pos=out[0],
                                        g_delta_rvec=out[1], g_delta_scale=out[2])
        grads = [o.to(ctx.dtype) if need else None for o, need in zip(out, ctx.needs_input_grad[2:5])]
        return (None, None, *grads, None)


def prim_transforms(posbase, rotbase, delta_pos, delta_rvec, delta_scale, prim_scale):
    """posbase[B,K,3], rotbase[B,K,3,3] (no gradient: the reference computes them under no_grad), delta_pos / delta_rvec /
    delta_scale[B,K,3], prim_scale a number -> (primpos[B,K,3], primrot[B,K,3,3], primscale[B,K,3]) =
    (posbase + rotbase delta_pos, rotbase axisangle_to_matrix(delta_rvec), prim_scale delta_scale), differentiable w.r.t.
    the three deltas."""
    if not all(torch.is_tensor(t) for t in (posbase, rotbase, delta_pos, delta_rvec, delta_scale)):
        raise ValueError("prim_transforms takes tensors")
    if delta_pos.dim() != 3 or delta_pos.shape[-1] != 3:
        raise ValueError("delta_pos must be [B,K,3]")
    B, K = delta_pos.shape[:2]
    for name, t, shape in (("posbase", posbase, (B, K, 3)), ("rotbase", rotbase, (B, K, 3, 3)),
                           ("delta_rvec", delta_rvec, (B, K, 3)), ("delta_scale", delta_scale, (B, K, 3))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    for name, t in (("posbase", posbase), ("rotbase", rotbase), ("delta_pos", delta_pos), ("delta_rvec", delta_rvec),
                    ("delta_scale", delta_scale)):
        if not t.dtype.is_floating_point:
            raise ValueError(f"{name} must be floating point")
    if posbase.requires_grad or rotbase.requires_grad:
        raise ValueError("posbase / rotbase carry no gradient (the reference computes them under no_grad): detach them")
    _need_gpu("prim_transforms", posbase, rotbase, delta_pos, delta_rvec, delta_scale)
    return _PrimTransforms.apply(posbase, rotbase, delta_pos, delta_rvec, delta_scale, float(prim_scale))


# --------------------------------------------------------------------------------------------------------- model level
def _home(obj):
    """The module that defines obj's class: where the reference keeps the helpers its forward calls."""
    return sys.modules[type(obj).__module__]


_GRID_CHECKED = {}   # (data_ptr, device, shape) -> (weakref, version, is the standard pixel grid)


def _is_standard_grid(pixel_coords):
    """True when pixel_coords[H,W,2] is the grid hand_mvp.py:149-151 registers ((x, y) of every pixel): gol_raydirs_fwd then
    takes it implicitly.  One comparison (a host sync) per buffer, cached like the slot tables."""
    if not torch.is_tensor(pixel_coords) or pixel_coords.dim() != 3 or pixel_coords.shape[-1] != 2:
        return False
    key = (pixel_coords.data_ptr(), str(pixel_coords.device), tuple(pixel_coords.shape))
    hit = _GRID_CHECKED.get(key)
    if hit is not None and hit[0]() is pixel_coords and hit[1] == pixel_coords._version:
        return hit[2]
    H, W = pixel_coords.shape[:2]
    y, x = torch.meshgrid(torch.arange(H, device=pixel_coords.device), torch.arange(W, device=pixel_coords.device),
                          indexing="ij")
    std = bool(torch.equal(pixel_coords.detach().float(), torch.stack([x, y], dim=-1).float()))
    for k in [k for k, v in _GRID_CHECKED.items() if v[0]() is None]:
        del _GRID_CHECKED[k]
    _GRID_CHECKED[key] = (weakref.ref(pixel_coords), pixel_coords._version, std)
    return std


def hand_mvp_render(self, K, Rt, preds, with_shadow=False):
    """Drop-in for hand_mvp.AutoEncoder.render (hand_mvp.py:162-205): same arguments, same (rayrgb, rayalpha, shadow).
    The template is assembled compacted by ONE kernel from the slabs (no full-K primrgba, no per-step nonzero), the pixel
    grid stays implicit, the primitive transforms are gathered with the cached index.  preds["primrgba"] is set only when
    the patch was installed with full_template=True (only HandMVPSummary reads it).  Under patch_hand_mvp(fused_tail=True)
    preds["primrgb"] / ["primalpha"] are two mvptail.TailHandles and the template comes from mvptail.decode_template (last
    decoder layers included, no slab); a tensor beside a handle, or full_template=True, materialises the handles."""
    B = K.shape[0]
    valid = preds.get("valid_prims", None)
    full = bool(getattr(self, FULL_TEMPLATE_FLAG, False))
    from . import mvptail    # (imports this module)

    if not full and mvptail.handles_fit(preds["primrgb"], preds["primalpha"], self.primsize):
        # patch_hand_mvp(fused_tail=True): both decoders stopped in front of their last layer
        template = mvptail.decode_handles(preds["primrgb"], preds["primalpha"], self.primsize, valid)
    else:
        preds["primrgb"], preds["primalpha"] = mvptail.materialized(preds["primrgb"]), mvptail.materialized(preds["primalpha"])
        res = assemble_template(preds["primrgb"], preds["primalpha"], self.primsize, valid_prims=valid, compact=True, full=full)
        template = res
        if full:
            template, preds["primrgba"] = res

    focal = K[:, :2, :2].contiguous()
    focal = torch.diagonal(focal, dim1=1, dim2=2).contiguous()
    princpt = K[:, :2, 2].contiguous()

    camrot = Rt[:, :3, :3].contiguous()
    campos = -(camrot.transpose(-2, -1) @ Rt[:, :3, 3:4])[..., 0]

    rm = self.raymarcher
    H, W = self.pixel_coords.shape[:2]
    if _is_standard_grid(self.pixel_coords):
        pixelcoords = (W, H)
    else:
        pixelcoords = self.pixel_coords[None].expand(B, -1, -1, -1).contiguous()

    primpos, primrot, primscale = preds["primpos"] / rm.volume_radius, preds["primrot"], preds["primscale"]
    if valid is not None:
        t = _tables(valid, True)
        if t.Kv == 0:      # nothing to march: a zero image, no launch on empty tensors
            zero = torch.zeros(B, 4, H, W, dtype=template.dtype, device=template.device)
            return zero[:, :3].contiguous(), zero[:, 3:4].contiguous(), None
        primpos, primrot, primscale = (torch.index_select(p, 1, t.index) for p in (primpos, primrot, primscale))
    raypos, raydir, tminmax = mvp.compute_raydirs(campos, camrot, focal, princpt, pixelcoords, rm.volume_radius)
    out = mvp.mvpraymarch(raypos, raydir, rm.dt, tminmax, (primpos.contiguous(), primrot.contiguous(), primscale.contiguous()),
                          template=template, warp=None, with_shadow=with_shadow)
    rayrgba, shadow = out if with_shadow else (out, None)
    rayrgba = rayrgba.permute(0, 3, 1, 2)
    return rayrgba[:, :3].contiguous(), rayrgba[:, 3:4].contiguous(), shadow


def geom_decoder_forward(self, pose, joint, iteration=-1):
    """Drop-in for hand_mvp.GeomDecoder.forward (hand_mvp.py:386-444): the same sub-module calls in the same order; the
    tail from the transform deltas to primpos / primrot / primscale (about fifty small launches and as many again backward)
    is one gol_mvp_primtransf_fwd / _bwd.  Under patch_hand_mvp(fused_tail=True) "primalpha" is a mvptail.TailHandle: the
    alpha decoder stops in front of its last layer (a decoder that cannot runs its own lines)."""
    mod = _home(self)
    B = pose.shape[0]

    with torch.no_grad():
        geom_lbs = self.lbs_fn.pose(torch.zeros_like(self.lbs_fn.lbs_template_verts), pose)
        primposbase = (
            mod.make_postex(geom_lbs, self.prim_vidx_img, self.prim_bary_img).permute(0, 2, 3, 1).reshape(B, -1, 3)
        )
        tbn = mod.compute_tbn(geom_lbs, self.geo_fn.vt, self.prim_vidx_img, self.prim_vtidx_img)
        primrotbase = torch.stack(tbn, dim=-2).reshape(B, self.n_prims, 3, 3).permute(0, 1, 3, 2).contiguous()

    delta_pos, delta_rvec, delta_scale = self.transdecoder(joint)

    if self.training and iteration < self.primposstart:
        delta_pos = delta_pos * 0.0
        delta_rvec = delta_rvec * 0.0
        delta_scale = delta_scale * 0.0 + 1.0

    primpos, primrot, primscale = prim_transforms(primposbase, primrotbase, delta_pos, delta_rvec, delta_scale,
                                                  self.prim_scale)

    alpha = None
    if getattr(self, "_goliath_fused_tail", False):   # mvptail.FUSED_TAIL_FLAG: a TailHandle in place of the slab
        from . import mvptail

        alpha = mvptail.tail_handle(self.alphadecoder, joint, self.primsize_z, 1)
    if alpha is None:
        alpha = self.alphadecoder(joint).view(B, self.primsize_z, 1, self.uv_size, self.uv_size)
        alpha = F.relu(alpha)

    return {"primalpha": alpha, "primpos": primpos, "primscale": primscale, "primrot": primrot, "geom_lbs": geom_lbs}
