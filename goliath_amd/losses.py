"""Image losses on top of the C ABI ("next" row).

  rgb_l1(preds, targets, ...)   <- ca_code/loss/__init__.py:391-411  (same signature / keys)
  l1_image(pred, target, mask)  the fused op: one read pass forward, one read + one write pass backward

and the per-Gaussian regularisers (csrc/regloss.hip): one read pass forward, one read + one write pass backward each
  penalty_mean(x, kind, p0, p1)  mean of an elementwise penalty (BOUND, NEG_SQ, SQ, ABS, ALPHAPRIOR)
  backlit(color, cos_weight)     sum(w * relu(color)) / (1 + sum(w)), w = relu(-cos_weight)^2
  bound_primscale, negcolor, l2_reg, list_l1_reg, backlit_reg, alphaprior, mask_l1
                                <- ca_code/loss/__init__.py:560-600, 609-622, 450-453  (same signatures / keys)

and the masked image penalties (csrc/imgfam.hip): kernel + finalize forward, one kernel backward, the mean on the device
  image_penalty(pred, target, kind, mask, veto)  mean of |x|, x^2 or |x| exp(|x| / 255) of x = (pred - target) mask (1 - veto)
  rgb_l2, psnr, rgb_l1_focus, rgb_l1_phys, pose_shadow_l2
                                <- ca_code/loss/__init__.py:366-386, 415-445, 496-538, 555-557  (same signatures / keys)
"""
from typing import Optional

import torch

from . import _lib
from ._lib import c_float, c_i64, c_int, fptr, ptr, stream_ptr


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask):
        B, C = pred.shape[:2]
        HW = pred[0, 0].numel()
        mask_c = 0 if mask is None else mask.shape[1]
        nb = _lib.load().gol_l1_blocks(HW)
        partial = torch.empty(B * C * nb, device=pred.device)
        with _lib.device_guard(pred.device):
            _lib.call("gol_l1_fwd", c_int(B), c_int(C), c_int(HW), c_int(mask_c), fptr(pred), fptr(target), fptr(mask),
                      fptr(partial), stream_ptr())
        ctx.save_for_backward(pred, target, mask)
        return partial.sum() / (B * C * HW)

    @staticmethod
    def backward(ctx, g):
        pred, target, mask = ctx.saved_tensors
        B, C = pred.shape[:2]
        HW = pred[0, 0].numel()
        mask_c = 0 if mask is None else mask.shape[1]
        out = torch.empty_like(pred)
        g = g.to(torch.float32).reshape(1).contiguous()
        with _lib.device_guard(pred.device):
            _lib.call("gol_l1_bwd", c_int(B), c_int(C), c_int(HW), c_int(mask_c), fptr(pred), fptr(target), fptr(mask),
                      fptr(g), fptr(out), stream_ptr())
        return out, None, None


def l1_image(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mean(|(pred - target) * mask|) for [B,C,H,W] images; mask [B,1,H,W] or [B,C,H,W] or None."""
    if not pred.is_cuda:
        raise _lib.GoliathHipError("l1_image needs CUDA(HIP) tensors; there is no CPU path")
    c = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    return _L1.apply(pred.to(torch.float32).contiguous(), c(target), c(mask))


def erode_mask(mask: torch.Tensor, ks: int) -> torch.Tensor:
    """ca_code/utils/image.py:393-422 erode(): a pixel survives iff every pixel of its ks x ks window (zero-padded
    complement) is set.  Returns a float mask of 0 / 1.  (A ks x ks box filter of the complement on a tiny tensor:
    plain torch, it has no gradient and is not on the per-pixel hot path.)"""
    assert ks % 2 == 1
    x = mask.to(torch.float32)
    if x.dim() == 3:
        x = x[:, None]
    flip = 1.0 - x
    w = torch.ones(1, 1, ks, ks, device=x.device)
    hit = torch.nn.functional.conv2d(flip.reshape(-1, 1, *x.shape[-2:]), w, padding=ks // 2) > 0
    return 1.0 - hit.reshape(x.shape).to(torch.float32)


def rgb_l1(preds, targets, src_key: str = "rendered_rgb", tgt_key: str = "image", mask_key: str = "image_mask",
           ddisc_key: str = "depth_disc_mask", mask_erode: Optional[int] = None):
    """Same semantics as the reference's rgb_l1 (ca_code/loss/__init__.py:391-411), incl. `mask_erode`."""
    mask = targets.get(mask_key, preds.get(mask_key, None))
    if mask_erode is not None:
        if mask is None:
            mask = torch.ones_like(preds[src_key])
        mask = (erode_mask(mask, mask_erode) > 0).to(torch.float32)  # .to(th.bool) in the reference
    if ddisc_key in preds:
        d = preds[ddisc_key]
        inv = (~d).float() if d.dtype == torch.bool else (1 - d)
        mask = inv if mask is None else mask * inv
    return l1_image(preds[src_key], targets[tgt_key], None if mask is None else mask.float())


class _Ssim(torch.autograd.Function):
    """Masked-mean SSIM of (target, pred); differentiable in pred (ca_code/utils/ssim.py:25-65)."""

    @staticmethod
    def forward(ctx, pred, target, mask):
        B, C, H, W = pred.shape
        mask_c = 0 if mask is None else mask.shape[1]
        nb = _lib.load().gol_ssim_blocks(H, W)
        partial = torch.empty(B * C * nb, device=pred.device)
        dmap = torch.empty(3, B, C, H, W, device=pred.device) if ctx.needs_input_grad[0] else None
        with _lib.device_guard(pred.device):
            _lib.call("gol_ssim_fwd", c_int(B), c_int(C), c_int(H), c_int(W), c_int(mask_c), fptr(target), fptr(pred),
                      fptr(mask), fptr(partial), fptr(dmap), stream_ptr())
        if mask is None:
            denom = torch.full((), float(B * C * H * W), device=pred.device)
        else:  # ssim.py:44-49: the mask is expanded to the image's channels before it is summed
            denom = (mask.sum() * (C // mask_c)).clamp(min=1)
        ctx.save_for_backward(pred, target, dmap, denom)
        return partial.sum() / denom

    @staticmethod
    def backward(ctx, g):
        pred, target, dmap, denom = ctx.saved_tensors
        B, C, H, W = pred.shape
        out = torch.empty_like(pred)
        gs = (g.to(torch.float32) / denom).reshape(1).contiguous()
        with _lib.device_guard(pred.device):
            _lib.call("gol_ssim_bwd", c_int(B), c_int(C), c_int(H), c_int(W), fptr(target), fptr(pred), fptr(dmap),
                      fptr(gs), fptr(out), stream_ptr())
        return out, None, None


def ssim_image(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ssim(target, pred, mask=mask) of ca_code/utils/ssim.py for [B,C,H,W] images (window 11, size_average)."""
    if not pred.is_cuda:
        raise _lib.GoliathHipError("ssim_image needs CUDA(HIP) tensors; there is no CPU path")
    c = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    return _Ssim.apply(pred.to(torch.float32).contiguous(), c(target), c(mask))


def rgb_ssim(preds, targets, src_key: str = "rendered_rgb", tgt_key: str = "image", mask_key: str = "image_mask",
             normalize_mask: bool = True):
    """Same semantics as the reference's rgb_ssim (ca_code/loss/__init__.py:478-494)."""
    mask = targets.get(mask_key, preds.get(mask_key, None))
    if mask is None or normalize_mask:
        return 1.0 - ssim_image(preds[src_key], targets[tgt_key], None if mask is None else mask.float())
    return 1.0 - ssim_image(mask * preds[src_key], mask * targets[tgt_key])


# ---- per-Gaussian regularisers (gol_regloss_*, gol_backlit_*) ---------------------------------------------------------
BOUND, NEG_SQ, SQ, ABS, ALPHAPRIOR = range(5)   # gol_regloss_kind of include/goliath_hip.h


def regloss_chunk_elems():
    return _lib.load().gol_regloss_chunk_elems()


class _Penalty(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind, p0, p1):
        n = x.numel()
        nb = -(-n // regloss_chunk_elems())
        partial = torch.empty(nb, device=x.device, dtype=torch.float64)
        with _lib.device_guard(x.device):
            _lib.call("gol_regloss_fwd", c_int(kind), c_i64(n), c_float(p0), c_float(p1), fptr(x),
                      ptr(partial, torch.float64), stream_ptr())
        ctx.save_for_backward(x)
        ctx.args = (kind, p0, p1)
        return (partial.sum() / n).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        (x,) = ctx.saved_tensors
        kind, p0, p1 = ctx.args
        n = x.numel()
        out = torch.empty_like(x)
        gs = (g.to(torch.float32) / n).reshape(1).contiguous()
        with _lib.device_guard(x.device):
            _lib.call("gol_regloss_bwd", c_int(kind), c_i64(n), c_float(p0), c_float(p1), fptr(x), fptr(gs), fptr(out),
                      stream_ptr())
        return out, None, None, None


def penalty_mean(x: torch.Tensor, kind: int, p0: float = 0.0, p1: float = 0.0) -> torch.Tensor:
    """mean(f(x)) over all elements of x for the penalty `kind` (BOUND: p0 = min, p1 = max; the others read no parameter);
    f and f' as listed at gol_regloss_fwd in include/goliath_hip.h.  A float32 scalar, differentiable in x."""
    if not x.is_cuda:
        raise _lib.GoliathHipError("penalty_mean needs CUDA(HIP) tensors; there is no CPU path")
    if x.numel() == 0:
        raise ValueError("penalty_mean of an empty tensor")
    return _Penalty.apply(x.to(torch.float32).contiguous(), int(kind), float(p0), float(p1))


class _Backlit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, cosw):
        C = color.shape[-1]
        M = cosw.numel()
        nb = -(-M // (regloss_chunk_elems() // 4))
        partial = torch.empty(nb, 2, device=color.device, dtype=torch.float64)
        with _lib.device_guard(color.device):
            _lib.call("gol_backlit_fwd", c_i64(M), c_int(C), fptr(color), fptr(cosw), ptr(partial, torch.float64),
                      stream_ptr())
        num, den = partial.sum(0).unbind(0)
        denom = 1.0 + den
        ctx.save_for_backward(color, cosw, denom)
        return (num / denom).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        color, cosw, denom = ctx.saved_tensors
        out = torch.empty_like(color)
        gs = (g.to(torch.float64) / denom).to(torch.float32).reshape(1).contiguous()
        with _lib.device_guard(color.device):
            _lib.call("gol_backlit_bwd", c_i64(cosw.numel()), c_int(color.shape[-1]), fptr(color), fptr(cosw), fptr(gs),
                      fptr(out), stream_ptr())
        return out, None


def backlit(color: torch.Tensor, cos_weight: torch.Tensor) -> torch.Tensor:
    """sum(w * relu(color)) / (1 + sum(w)) with w = relu(-cos_weight)^2: color [..., C], cos_weight [..., 1] (or [...]),
    one weight per colour row, counted once in the denominator.  Differentiable in color only: the model builds
    cos_weight under no_grad, and one that requires grad raises."""
    if not (color.is_cuda and cos_weight.is_cuda):
        raise _lib.GoliathHipError("backlit needs CUDA(HIP) tensors; there is no CPU path")
    if cos_weight.requires_grad:
        raise ValueError("backlit: cos_weight receives no gradient (build it under no_grad, or detach it)")
    if color.numel() == 0:
        raise ValueError("backlit of an empty tensor")
    if tuple(cos_weight.shape) not in (tuple(color.shape[:-1]) + (1,), tuple(color.shape[:-1])):
        raise ValueError(f"backlit: cos_weight {tuple(cos_weight.shape)} does not give one weight per row of color "
                         f"{tuple(color.shape)}")
    return _Backlit.apply(color.to(torch.float32).contiguous(), cos_weight.to(torch.float32).contiguous())


def bound_primscale(preds, batch=None, key: str = "primscale_preclip", min_scale: float = 0.1, max_scale: float = 20.0):
    """Same semantics as the reference's bound_primscale (ca_code/loss/__init__.py:560-573)."""
    return penalty_mean(preds[key], BOUND, min_scale, max_scale)


def negcolor(preds, batch=None, key: str = "diff_color"):
    """Same semantics as the reference's negcolor (ca_code/loss/__init__.py:576-578)."""
    return penalty_mean(preds[key], NEG_SQ)


def l2_reg(preds, batch=None, key: str = "spec_dnml"):
    """Same semantics as the reference's l2_reg (ca_code/loss/__init__.py:581-583)."""
    return penalty_mean(preds[key], SQ)


def list_l1_reg(preds, batch=None, key: str = "spec_dnml"):
    """Same semantics as the reference's list_l1_reg (ca_code/loss/__init__.py:585-590): the sum of the terms' means."""
    loss = 0
    for term in preds[key]:
        loss = loss + penalty_mean(term, ABS)
    return loss


def backlit_reg(preds, batch=None, key: str = "color_rand", cos_key: str = "cos_weight"):
    """Same semantics as the reference's backlit_reg (ca_code/loss/__init__.py:592-600)."""
    return backlit(preds[key], preds[cos_key])


def alphaprior(preds, batch=None, key: str = "alpha"):
    """Same semantics as the reference's alphaprior (ca_code/loss/__init__.py:609-622)."""
    return penalty_mean(preds[key], ALPHAPRIOR)


def mask_l1(preds, targets, src_key: str = "rendered_mask", tgt_key: str = "image_mask"):
    """Same semantics as the reference's mask_l1 (ca_code/loss/__init__.py:450-453): l1_image without a mask."""
    pred, target = preds[src_key], targets[tgt_key]
    if pred.dim() < 2:
        pred, target = pred.reshape(1, 1, -1), target.reshape(1, 1, -1)
    return l1_image(pred, target.expand_as(pred) if target.shape != pred.shape else target)


# ---- masked image penalties (gol_imgloss_*, csrc/imgfam.hip) ----------------------------------------------------------
IMG_ABS, IMG_SQ, IMG_EXPW = range(3)   # gol_imgloss_kind of include/goliath_hip.h


def imgloss_chunk_elems():
    return _lib.load().gol_imgloss_chunk_elems()


def _imgloss_args(kind, pred, target, mask, veto):
    B, C = pred.shape[:2]
    HW = pred[0, 0].numel()
    mask_c = 0 if mask is None else mask.shape[1]
    return (c_int(kind), c_int(B), c_int(C), c_int(HW), c_int(mask_c), fptr(pred), fptr(target), fptr(mask),
            ptr(veto, torch.uint8))


class _ImagePenalty(torch.autograd.Function):
    """kernel, finalize forward; kernel backward (plus the one scalar division upstream / n)."""

    @staticmethod
    def forward(ctx, pred, target, mask, veto, kind):
        B, C = pred.shape[:2]
        HW = pred[0, 0].numel()
        n = B * C * HW
        nb = B * C * -(-HW // imgloss_chunk_elems())
        partial = torch.empty(nb, device=pred.device, dtype=torch.float64)
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        total = torch.empty((), device=pred.device, dtype=torch.float64)
        with _lib.device_guard(pred.device):
            _lib.call("gol_imgloss_fwd", *_imgloss_args(kind, pred, target, mask, veto), ptr(partial, torch.float64),
                      stream_ptr())
            _lib.call("gol_imgloss_finalize", c_i64(nb), c_i64(n), ptr(partial, torch.float64), fptr(loss),
                      ptr(total, torch.float64), stream_ptr())
        ctx.save_for_backward(pred, target, mask, veto)
        ctx.kind = kind
        return loss

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        pred, target, mask, veto = ctx.saved_tensors
        out = torch.empty_like(pred)
        gs = (g.to(torch.float32) / pred.numel()).reshape(1).contiguous()
        with _lib.device_guard(pred.device):
            _lib.call("gol_imgloss_bwd", *_imgloss_args(ctx.kind, pred, target, mask, veto), fptr(gs), fptr(out),
                      stream_ptr())
        return out, None, None, None, None


def image_penalty(pred: torch.Tensor, target: torch.Tensor, kind: int, mask: Optional[torch.Tensor] = None,
                  veto: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mean(f((pred - target) * mask * (1 - veto))) over [B,C,...] images for the penalty `kind` (IMG_ABS |x|, IMG_SQ x^2,
    IMG_EXPW |x| exp(|x| / 255) with the weight detached; f and its gradient as listed at gol_imgloss_fwd in
    include/goliath_hip.h).  mask: float [B,1,...] or [B,C,...] or None; veto: torch.bool (or uint8) [B,1,...] or None, read
    as bytes without a conversion pass.  A float32 scalar, differentiable in pred only."""
    if not (pred.is_cuda and target.is_cuda):
        raise _lib.GoliathHipError("image_penalty needs CUDA(HIP) tensors; there is no CPU path")
    if pred.dim() < 3 or pred.numel() == 0:
        raise ValueError(f"image_penalty: pred {tuple(pred.shape)} is not a non-empty [B,C,...] image")
    if target.shape != pred.shape:
        target = target.expand_as(pred)
    planes = lambda t: t.shape[0] == pred.shape[0] and t.shape[2:] == pred.shape[2:]
    if mask is not None and not (mask.dim() == pred.dim() and planes(mask) and mask.shape[1] in (1, pred.shape[1])):
        raise ValueError(f"image_penalty: mask {tuple(mask.shape)} does not fit pred {tuple(pred.shape)}")
    if veto is not None:
        if veto.dtype not in (torch.bool, torch.uint8):
            raise ValueError("image_penalty: veto must be torch.bool or torch.uint8 (fold a float one into the mask)")
        if not (veto.dim() == pred.dim() and planes(veto) and veto.shape[1] == 1):
            raise ValueError(f"image_penalty: veto {tuple(veto.shape)} does not fit pred {tuple(pred.shape)}")
        veto = veto.detach().contiguous()
        veto = veto.view(torch.uint8) if veto.dtype == torch.bool else veto
    c = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    return _ImagePenalty.apply(pred.to(torch.float32).contiguous(), c(target), c(mask), veto, int(kind))


def _hip_erode(mask: torch.Tensor, ks: int) -> torch.Tensor:
    from . import imageops

    return imageops.erode_planes(mask, ks)


def _image_mask(mask, ddisc, mask_erode):
    """The mask product of the reference's image losses (ca_code/loss/__init__.py:376-385, 498-507) as (mask, veto): the
    erosion on gol_mask_erode, a boolean depth_disc_mask handed on as the kernel's veto, a float one folded into the mask in
    torch (`mask * (1 - ddisc)`, the reference's `try` branch)."""
    if mask_erode is not None:
        mask = _hip_erode(mask, mask_erode)      # erode(mask.to(th.float32), ks).to(th.bool), kept as float 0 / 1
    veto = None
    if ddisc is not None:
        if ddisc.dtype == torch.bool:
            veto = ddisc
        else:
            mask = (1 - ddisc) if mask is None else mask * (1 - ddisc)
    if veto is not None and (veto.dim() < 3 or veto.shape[1] != 1):   # not one flag per pixel: fold it in torch
        mask, veto = ((~veto).to(torch.float32) if mask is None else mask * ~veto), None
    return (None if mask is None else mask.to(torch.float32)), veto


def _masked_penalty(kind, pred, target, mask, ddisc, mask_erode):
    if not (pred.is_cuda and target.is_cuda):
        raise _lib.GoliathHipError("the fused image losses need CUDA(HIP) tensors; there is no CPU path")
    mask, veto = _image_mask(mask, ddisc, mask_erode)
    return image_penalty(pred, target, kind, mask, veto)


def rgb_l2(preds, targets, src_key: str = "rendered_rgb", tgt_key: str = "image", mask_key: str = "image_mask",
           ddisc_key: str = "depth_disc_mask", mask_erode: Optional[int] = None):
    """Same semantics as the reference's rgb_l2 (ca_code/loss/__init__.py:366-386); an absent mask costs no pass (with
    `mask_erode` it is a mask of ones, one channel)."""
    mask = targets.get(mask_key, preds.get(mask_key, None))
    if mask is None and mask_erode is not None:
        mask = torch.ones_like(preds[src_key][:, :1])
    return _masked_penalty(IMG_SQ, preds[src_key], targets[tgt_key], mask, preds.get(ddisc_key, None), mask_erode)


def psnr(preds, targets, src_key: str = "rendered_rgb", tgt_key: str = "image", mask_key: str = "image_mask",
         data_range: float = 1., ddisc_key: str = "depth_disc_mask", mask_erode: Optional[int] = None):
    """Same semantics as the reference's psnr (ca_code/loss/__init__.py:415-445): formed from the fused mean squared error
    on the device in float32; the two constants are float32 logarithms taken on the host, so nothing is copied or synced."""
    msqerr = rgb_l2(preds, targets, src_key, tgt_key, mask_key, ddisc_key, mask_erode)
    two_log_range = float(2 * torch.log(torch.tensor(data_range, dtype=torch.float32)))
    scale = float(10 / torch.log(torch.tensor(10.)))
    return (two_log_range - torch.log(msqerr)) * scale


def _focus(preds, targets, pred_key, mask_erode, self_mask):
    mask = preds['rendered_mask'].detach() if self_mask else targets['image_mask']
    return _masked_penalty(IMG_EXPW, preds[pred_key], targets["image"], mask, preds['depth_disc_mask'], mask_erode)


def rgb_l1_focus(preds, targets, mask_erode=None, img_blur=False, self_mask=False):
    """Same semantics as the reference's rgb_l1_focus (ca_code/loss/__init__.py:496-517)."""
    return _focus(preds, targets, "rendered_rgb_blur" if img_blur else "rendered_rgb", mask_erode, self_mask)


def rgb_l1_phys(preds, targets, mask_erode=None, img_blur=False, self_mask=False):
    """Same semantics as the reference's rgb_l1_phys (ca_code/loss/__init__.py:519-538; `img_blur` is unused there too)."""
    return _focus(preds, targets, "rendered_phys_rgb", mask_erode, self_mask)


def pose_shadow_l2(preds, batch=None):
    """Same semantics as the reference's pose_shadow_l2 (ca_code/loss/__init__.py:555-557): the target is detached."""
    pred, target = preds["pose_shadow_map"], preds["shadow_map"]
    if not (pred.is_cuda and target.is_cuda):
        raise _lib.GoliathHipError("pose_shadow_l2 needs CUDA(HIP) tensors; there is no CPU path")
    if pred.dim() < 3:
        pred, target = pred.reshape(1, 1, -1), target.expand_as(pred).reshape(1, 1, -1)
    return image_penalty(pred, target, IMG_SQ)
