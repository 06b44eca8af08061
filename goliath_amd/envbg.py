"""The environment background of the relight visualisation (run_vis_relight.py:110-122 -> rgca.py:232-245), fused.

  env_background(envbg, K, Rt, height, width, focal_scale=0.2, blur=True)
      envmap_to_image  ca_code/utils/envmap.py:169-227 (no fisheye `D` path): the equirectangular map seen through every
      pixel, bicubic, then the 101 x 101 Gaussian blur as two 101-tap passes (csrc/envbg.hip: gol_envbg_image)
  compose_envmap(render, alpha, envbg, K, Rt)
      compose_envmap   ca_code/utils/envmap.py:325-345, same signature and argument meaning: the clamped background behind
      the render and the 200 x 200 mirror ball (envmap.py:230-248) in the bottom-right corner (gol_envbg_compose)
  blur_taps()          the 101 separable weights, float64

Forward only: with grad mode on and an input that requires grad these raise (the drop-in then keeps the reference path).
There is no CPU path.
"""
import ctypes

import torch

from . import _lib
from ._lib import c_double, c_int, fptr, stream_ptr

BALL = 200    # envmap.py:326
TAPS = 101    # envmap.py:220


def blur_taps() -> torch.Tensor:
    """k / sum(k) for k = exp(-linspace(-4, 4, 101)^2) in float64: the reference's 2-D kernel (envmap.py:220-222) is the
    outer product of this vector with itself.  The one definition is the library's (gol_envbg_blur_taps, host code: no GPU
    needed), the values gol_envbg_image rounds to float32 for its kernels."""
    buf = (ctypes.c_double * TAPS)()
    rc = _lib.load().gol_envbg_blur_taps(buf)
    if rc != 0:
        raise _lib.GoliathHipError(f"gol_envbg_blur_taps failed ({rc})")
    return torch.tensor(list(buf), dtype=torch.float64)


def _check(name, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise _lib.GoliathHipError(f"{name} needs CUDA(HIP) tensors; there is no CPU path")
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise _lib.GoliathHipError(f"{name} is forward-only: call it under torch.no_grad() or with detached inputs")


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def _scratch(B, H, W, dev):
    fn = _lib.load().gol_envbg_scratch_floats
    fn.restype = ctypes.c_int64
    return torch.empty(max(int(fn(c_int(B), c_int(H), c_int(W))), 1), dtype=torch.float32, device=dev)


def _image(envbg, K, R, H, W, focal_scale, blur):
    B, _, He, We = envbg.shape
    bg = torch.empty(B, 3, H, W, dtype=torch.float32, device=envbg.device)
    scratch = _scratch(B, H, W, envbg.device) if blur else None
    with _lib.device_guard(envbg.device):
        _lib.call("gol_envbg_image", c_int(B), c_int(H), c_int(W), c_int(He), c_int(We), fptr(envbg), fptr(K), fptr(R),
                  c_double(focal_scale), c_int(1 if blur else 0), fptr(scratch), fptr(bg), stream_ptr())
    return bg


def _inputs(envbg, K, Rt):
    if envbg.dim() != 4 or envbg.shape[1] != 3:
        raise ValueError("envbg must be [B,3,He,We]")
    B = envbg.shape[0]
    if tuple(K.shape) != (B, 3, 3) or Rt.dim() != 3 or Rt.shape[0] != B or Rt.shape[1] < 3 or Rt.shape[2] < 3:
        raise ValueError("K must be [B,3,3] and Rt [B,3,3] or [B,3,4]")
    return _f32c(envbg), _f32c(K), _f32c(Rt[:, :3, :3])


def env_background(envbg: torch.Tensor, K: torch.Tensor, Rt: torch.Tensor, height: int, width: int,
                   focal_scale: float = 0.2, blur: bool = True) -> torch.Tensor:
    """envmap_to_image(width, height, envbg, K[:, :2, 2], K, Rt[:, :3, :3], focal_scale, blurbg=blur): bg[B,3,H,W], not
    clamped.  envbg[B,3,He,We], K[B,3,3], Rt[B,3,4] (or [B,3,3])."""
    _check("env_background", envbg, K, Rt)
    envbg, K, R = _inputs(envbg, K, Rt)
    return _image(envbg, K, R, int(height), int(width), float(focal_scale), bool(blur))


def compose_envmap(render: torch.Tensor, alpha: torch.Tensor, envbg: torch.Tensor, K: torch.Tensor,
                   Rt: torch.Tensor) -> torch.Tensor:
    """ca_code/utils/envmap.py:325-345: render[B,3,H,W] + (1 - alpha[B,1,H,W]) * clamp(blurred background, 0, 1), with the
    mirror ball over the bottom-right 200 x 200 pixels.  `K[:, :2, 2]` is the principal point, `K` the focal, `Rt[:, :3, :3]`
    the rotation.  An image with a side below 200 is a ValueError (the reference fails on its slice assignment)."""
    if render.dim() != 4 or render.shape[1] != 3:
        raise ValueError("render must be [B,3,H,W]")
    B, _, H, W = render.shape
    if H < BALL or W < BALL:
        raise ValueError(f"compose_envmap needs an image of at least {BALL} x {BALL} pixels for the mirror ball, got {H} x {W}")
    if alpha.numel() != B * H * W:
        raise ValueError("alpha must be [B,1,H,W]")
    _check("compose_envmap", render, alpha, envbg, K, Rt)
    envbg, K, R = _inputs(envbg, K, Rt)
    if envbg.shape[0] != B:
        raise ValueError("envbg and render disagree on the batch size")
    render, alpha = _f32c(render), _f32c(alpha).reshape(B, 1, H, W)
    bg = _image(envbg, K, R, H, W, 0.2, True)
    out = torch.empty_like(render)
    with _lib.device_guard(render.device):
        _lib.call("gol_envbg_compose", c_int(B), c_int(H), c_int(W), c_int(envbg.shape[2]), c_int(envbg.shape[3]),
                  fptr(render), fptr(alpha), fptr(bg), fptr(envbg), fptr(R), c_int(BALL), fptr(out), stream_ptr())
    return out
