"""URHand's texture tail between the decoder's `relight_preds["tex"]` and the RGBA textures the renderer takes, fused.

  texture_tail(tex, tex_mean, tex_std, seams, cal_M, cal_b)   one HIP pass forward / one backward (csrc/uvtex.hip) for
      gain / bias            AutoEncoder.forward_tex      ca_code/models/urhand.py:721-741
      colour calibration     CalV5.forward                ca_code/nn/color_cal.py:211-241 (as imgtail.cal_v5_matrix's tensors)
      clamp_(0, 255)                                      urhand.py:747            -> texrec_before_warp
      seam resample          SeamSampler.resample         ca_code/utils/seams.py:21-25, urhand.py:805-807
      alpha packing          ones_like + cat              urhand.py:824-825        -> tex_rgba
  pack_seams(uvs, weights)   the seam constants of a model as device tensors + the transposed (CSR) tap list the backward
                             gathers over; seams_of(seam_sampler) builds it once and caches it on the module
  pack_rgba(x, scale, lo, hi)   (clamp(x * scale, lo, hi), 1) as RGBA: phys_tex, urhand.py:788-790 + :826
  normal_rgba(nml, Rt)          the normal colours of urhand.py:828-832 / :843-847 (forward only: the reference detaches)
`goliath_amd.urhand.autoencoder_forward` runs them where the model's class carries TEXTURE_TAIL_FLAG
(dropin.patch_urhand(texture_tail=True)).
"""
import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import c_float, c_int, fptr, iptr, stream_ptr

TEXTURE_TAIL_FLAG = "_gol_texture_tail"   # class attribute set by dropin.patch_urhand(texture_tail=True)


class SeamPack:
    """A model's seam constants on one device.  uvs[S,S,2], weights[S,S] float32; the transposed tap list: for destination
    texel t the entries row_start[t] .. row_start[t+1] (int32 [S*S+1]) hold src (int32: the band texel whose bilinear
    sample reads t) and coeff (float32: weights[src] * bilinear weight), sorted by (t, tap, src)."""
    __slots__ = ("uvs", "weights", "row_start", "src", "coeff")

    def __init__(self, uvs, weights, row_start, src, coeff):
        self.uvs, self.weights, self.row_start, self.src, self.coeff = uvs, weights, row_start, src, coeff

    @property
    def size(self):
        return self.weights.shape[-1]


def pack_seams(uvs: torch.Tensor, weights: torch.Tensor) -> SeamPack:
    """Pack SeamSampler's `uvs[S,S,2]` and `weights` ([S,S], [1,S,S] or [1,1,S,S]) for texture_tail.  For every texel with
    weight != 0 the up to four taps of grid_sample's bilinear fetch (align_corners=False, padding_mode="border": sample
    point clip(u S - 0.5, 0, S - 1), taps floor and floor + 1, a tap at index S dropped) are emitted as
    (destination texel, weight * bilinear weight) and sorted by destination.  Runs on the tensors' device (CPU tensors
    give a CPU pack: only the GPU kernels refuse it); one host sync, once per model."""
    if uvs.dim() != 3 or uvs.shape[0] != uvs.shape[1] or uvs.shape[2] != 2:
        raise ValueError(f"uvs must be [S,S,2], got {tuple(uvs.shape)}")
    S = uvs.shape[0]
    if weights.numel() != S * S or tuple(weights.shape[-2:]) != (S, S):
        raise ValueError(f"weights must broadcast as [S,S] with S = {S}, got {tuple(weights.shape)}")
    if S * S >= 2 ** 29:
        raise ValueError("S too large for the int32 tap list")
    uvs = uvs.detach().to(torch.float32).contiguous()
    w = weights.detach().to(torch.float32).reshape(S, S).contiguous()
    t = torch.nonzero(w.reshape(-1) != 0).reshape(-1)                     # band texels, ascending
    u, v = uvs.reshape(-1, 2)[t].unbind(-1)
    x = (u * S - 0.5).clamp(0, S - 1)
    y = (v * S - 0.5).clamp(0, S - 1)
    x0, y0 = x.floor(), y.floor()
    fx, fy = x - x0, y - y0
    x0, y0 = x0.long(), y0.long()
    dst, src, coeff = [], [], []
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi < S) & (yi < S)
            bw = (fx if dx else 1 - fx) * (fy if dy else 1 - fy)
            dst.append((yi * S + xi)[ok])
            src.append(t[ok])
            coeff.append((w.reshape(-1)[t] * bw)[ok])
    dst, src, coeff = torch.cat(dst), torch.cat(src), torch.cat(coeff)
    order = torch.sort(dst, stable=True)[1]                               # ties keep the (tap, src) order: deterministic
    counts = torch.bincount(dst, minlength=S * S)
    row_start = torch.zeros(S * S + 1, dtype=torch.int64, device=uvs.device)
    row_start[1:] = torch.cumsum(counts, 0)
    return SeamPack(uvs, w, row_start.to(torch.int32), src[order].to(torch.int32).contiguous(), coeff[order].contiguous())


def seams_of(seam_sampler) -> SeamPack:
    """The SeamPack of a SeamSampler's `uvs` / `weights` buffers, built on first use and cached on the module; rebuilt when
    a buffer's device, shape or storage changes."""
    bufs = (seam_sampler.uvs, seam_sampler.weights)
    key = tuple((b.device, tuple(b.shape), b.data_ptr(), b._version) for b in bufs)
    cached = seam_sampler.__dict__.get("_gol_seam_pack")
    if cached is None or cached[0] != key:
        cached = (key, pack_seams(*bufs))
        seam_sampler.__dict__["_gol_seam_pack"] = cached
    return cached[1]


def _square(t, name, channels):
    if t.dim() != 4 or t.shape[-1] != t.shape[-2]:
        raise ValueError(f"{name} must be [B,C,S,S] with square images, got {tuple(t.shape)}")
    if t.shape[1] not in channels:
        raise ValueError(f"{name} must have {' or '.join(map(str, channels))} channels, got {t.shape[1]}")


class _TextureTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, tex_mean, tex_std, seams, cal_M, cal_b):
        B, C, S, _ = tex.shape
        before = torch.empty(B, 3, S, S, device=tex.device, dtype=torch.float32)
        rgba = torch.empty(B, 4, S, S, device=tex.device, dtype=torch.float32)
        uvs, w = (None, None) if seams is None else (seams.uvs, seams.weights)
        with _lib.device_guard(tex.device):
            _lib.call("gol_uvtex_fwd", c_int(B), c_int(C), c_int(S), c_int(int(tex_mean.shape[0] != 1)), fptr(tex),
                      fptr(tex_mean), c_float(tex_std), fptr(cal_M), fptr(cal_b), fptr(uvs), fptr(w), fptr(before), fptr(rgba),
                      stream_ptr())
        ctx.save_for_backward(tex, tex_mean, cal_M, cal_b)
        ctx.tex_std, ctx.seams = tex_std, seams
        ctx.set_materialize_grads(False)   # an output no loss reads arrives as None, not as an image of zeros
        return before, rgba

    @staticmethod
    def backward(ctx, g_before, g_rgba):
        tex, tex_mean, cal_M, cal_b = ctx.saved_tensors
        seams = ctx.seams
        B, C, S, _ = tex.shape
        dev = tex.device
        if g_rgba is None:
            g_rgba = torch.zeros(B, 4, S, S, device=dev)
        g_rgba = g_rgba.to(torch.float32).contiguous()
        if g_before is not None:
            g_before = g_before.to(torch.float32).contiguous()
        g_tex = torch.empty_like(tex)
        partials = None
        if cal_M is not None:
            fn = _lib.load().gol_uvtex_partial_floats
            fn.restype = ctypes.c_int64
            n = int(fn(c_int(B), c_int(S)))
            partials = torch.empty(B, max(n // max(B, 1) // 16, 1), 16, device=dev)
        w, rs, src, coeff = (None,) * 4 if seams is None else (seams.weights, seams.row_start, seams.src, seams.coeff)
        with _lib.device_guard(dev):
            _lib.call("gol_uvtex_bwd", c_int(B), c_int(C), c_int(S), c_int(int(tex_mean.shape[0] != 1)), fptr(tex),
                      fptr(tex_mean), c_float(ctx.tex_std), fptr(cal_M), fptr(cal_b), fptr(w), iptr(rs), iptr(src), fptr(coeff),
                      fptr(g_rgba), fptr(g_before), fptr(g_tex), fptr(partials), stream_ptr())
        need = ctx.needs_input_grad
        g_M = g_b = None
        if partials is not None and (need[4] or need[5]):
            s = partials.sum(1)   # [B,16]: bias 0..2 | M 3..11 (per-workgroup partial sums, no atomics)
            g_M, g_b = s[:, 3:12].reshape(B, 3, 3), s[:, 0:3]
        return (g_tex if need[0] else None, None, None, None, g_M if need[4] else None, g_b if need[5] else None)


def texture_tail(tex: torch.Tensor, tex_mean: torch.Tensor, tex_std: float, seams: Optional[SeamPack],
                 cal_M: Optional[torch.Tensor] = None, cal_b: Optional[torch.Tensor] = None):
    """(texrec_before_warp[B,3,S,S], tex_rgba[B,4,S,S]) of tex[B,C,S,S] (C = 2: one gain, one bias; 4: three gains, one
    bias; 6: three of each -- urhand.py:721-729), tex_mean[B,3,S,S] or [1,3,S,S] and the scalar tex_std:
        pre = clamp(cal(tex_mean * gain + bias * tex_std), 0, 255),  cal(x)[c] = sum_j cal_M[b,c,j] x[j] + cal_b[b,c]
        out = (1 - w) * pre + w * bilinear(pre, uv)   (seams = pack_seams(...); None = no resample, out = pre)
    texrec_before_warp = pre, tex_rgba = (out, 1).  tex_mean is used clamped to [0, 255], as urhand.py:740 leaves it (a
    no-op for a colour mean).  Gradients reach tex, cal_M and cal_b, from tex_rgba[:, :3] and from
    texrec_before_warp.  NO gradient goes to tex_mean (a buffer of the model, detached at urhand.py:778), to the seam data
    or to tex_std; tex_rgba's alpha takes none.  The clamp passes the gradient where 0 <= x <= 255 (torch's mask).  The
    backward uses no atomics: two runs on the same inputs give bit-identical gradients."""
    _square(tex, "tex", (2, 4, 6))
    _square(tex_mean, "tex_mean", (3,))
    B, _, S, _ = tex.shape
    if tex_mean.shape[0] not in (1, B) or tex_mean.shape[-1] != S:
        raise ValueError(f"tex_mean must be [B,3,S,S] or [1,3,S,S] for tex {tuple(tex.shape)}, got {tuple(tex_mean.shape)}")
    if (cal_M is None) != (cal_b is None):
        raise ValueError("cal_M and cal_b go together")
    if cal_M is not None and (tuple(cal_M.shape) != (B, 3, 3) or tuple(cal_b.shape) != (B, 3)):
        raise ValueError(f"cal_M / cal_b must be [B,3,3] / [B,3], got {tuple(cal_M.shape)} / {tuple(cal_b.shape)}")
    if seams is not None and seams.size != S:
        raise ValueError(f"the seam pack is for S = {seams.size}, the texture has S = {S}")
    for name, t in (("tex", tex), ("tex_mean", tex_mean), ("cal_M", cal_M), ("cal_b", cal_b)):
        if t is not None and not t.is_cuda:
            raise _lib.GoliathHipError(f"texture_tail needs CUDA(HIP) tensors ({name} is on {t.device}); there is no CPU path")
    if seams is not None:
        if seams.weights.device != tex.device:
            raise _lib.GoliathHipError(f"the seam pack is on {seams.weights.device}, the texture on {tex.device}")
    c = lambda t: None if t is None else t.to(torch.float32).contiguous()
    return _TextureTail.apply(c(tex), c(tex_mean.detach()), float(tex_std), seams, c(cal_M), c(cal_b))


class _PackRGBA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, lo, hi):
        B, _, S, _ = x.shape
        out = torch.empty(B, 4, S, S, device=x.device, dtype=torch.float32)
        with _lib.device_guard(x.device):
            _lib.call("gol_pack_rgba_fwd", c_int(B), c_int(S), c_float(scale), c_float(lo), c_float(hi), fptr(x), fptr(out),
                      stream_ptr())
        ctx.save_for_backward(x)
        ctx.args = (scale, lo, hi)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        B, _, S, _ = x.shape
        scale, lo, hi = ctx.args
        g = g.to(torch.float32).contiguous()
        g_x = torch.empty_like(x)
        with _lib.device_guard(x.device):
            _lib.call("gol_pack_rgba_bwd", c_int(B), c_int(S), c_float(scale), c_float(lo), c_float(hi), fptr(x), fptr(g),
                      fptr(g_x), stream_ptr())
        return g_x, None, None, None


def pack_rgba(x: torch.Tensor, scale: float = 255.0, lo: float = 0.0, hi: float = 255.0) -> torch.Tensor:
    """out[B,4,S,S] with out[:, :3] = clamp(x * scale, lo, hi) and out[:, 3] = 1 for x[B,3,S,S] (urhand.py:788-790 + :826).
    The gradient to x is scale where lo <= x * scale <= hi (torch's clamp mask), 0 elsewhere."""
    _square(x, "x", (3,))
    if not x.is_cuda:
        raise _lib.GoliathHipError("pack_rgba needs CUDA(HIP) tensors; there is no CPU path")
    return _PackRGBA.apply(x.to(torch.float32).contiguous(), float(scale), float(lo), float(hi))


def normal_rgba(nml: torch.Tensor, Rt: torch.Tensor) -> torch.Tensor:
    """The normal colours of urhand.py:828-832 / :843-847 as RGBA [B,4,S,S]: channel c = (1 - sum_j Rt[b,c,j] nml[b,j]) *
    127.5, channel 3 = 1, for nml[B,3,S,S] and Rt[B,3,4] or [B,4,4].  Forward only, without gradient (the reference
    detaches the normals); S comes from the tensor."""
    _square(nml, "nml", (3,))
    B, _, S, _ = nml.shape
    if Rt.dim() != 3 or Rt.shape[0] != B or tuple(Rt.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"Rt must be [B,3,4] or [B,4,4] with B = {B}, got {tuple(Rt.shape)}")
    if not nml.is_cuda or not Rt.is_cuda:
        raise _lib.GoliathHipError("normal_rgba needs CUDA(HIP) tensors; there is no CPU path")
    nml = nml.detach().to(torch.float32).contiguous()
    Rt = Rt.detach().to(torch.float32).contiguous()
    out = torch.empty(B, 4, S, S, device=nml.device, dtype=torch.float32)
    with _lib.device_guard(nml.device):
        _lib.call("gol_normal_rgba", c_int(B), c_int(S), c_int(Rt.shape[1] * 4), fptr(nml), fptr(Rt), fptr(out), stream_ptr())
    return out
