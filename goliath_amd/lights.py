"""The lights of a frame: head-relative positions and SH light coefficients in ONE launch (csrc/lightsh.hip).

  sh_norm_constants(deg)                     the (deg+1)^2 normalisation constants, float64 (host code: no GPU needed)
  dir2sh(deg, dirs[...,3])                   ca_code/utils/sh.py:118-127 dir2sh_torch -> [...,(deg+1)^2]
  headrel_light_sh(light_pos, light_intensity, head_pose, deg)
      ca_code/models/rgca.py:175-191: headrel_light_pos[B,L,3] = (light_pos - t) @ R and headrel_light_sh[B,3,(deg+1)^2] =
      sum over the lights of dir2sh_torch(deg, F.normalize(headrel_light_pos)) x intensity
  random_light_sh(deg, batch, device, dtype)
      the training-only random back-light of rgca.py:590-613: (light_dir[B,1,3], light_sh[B,3,(deg+1)^2]), unit intensity

Forward only -- every input is batch data and the reference propagates no gradient through these lines to anything
trainable: with grad mode on and an input that requires grad these raise (the drop-in then keeps the reference path).
No host sync, no atomics (bitwise repeatable), launched on the current stream.  There is no CPU path.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import c_int, fptr, stream_ptr

MAX_DEG = 8


def _deg(deg) -> int:
    deg = int(deg)
    if not 0 <= deg <= MAX_DEG:
        raise ValueError(f"the SH degree must be 0 ... {MAX_DEG}, got {deg}")
    return deg


def sh_norm_constants(deg: int) -> torch.Tensor:
    """KVal(|m|, n) (times sqrt 2 for m != 0) of sh.py:13-26, 80-86 in the reference's coefficient order (n outer, m = -n..n
    inner), float64.  The one definition is the library's (gol_sh_norm_constants, host code), the values the kernels round
    to float32."""
    deg = _deg(deg)
    n = (deg + 1) ** 2
    buf = (ctypes.c_double * n)()
    rc = _lib.load().gol_sh_norm_constants(c_int(deg), buf)
    if rc != 0:
        raise _lib.GoliathHipError(f"gol_sh_norm_constants failed ({rc})")
    return torch.tensor(list(buf), dtype=torch.float64)


def _p(x):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else fptr(x)


def _abi_sh_basis_fwd(*, M, deg, dirs, coeffs):
    _lib.call("gol_sh_basis_fwd", c_int(M), c_int(deg), _p(dirs), _p(coeffs), stream_ptr())


def _abi_light_sh_fwd(*, B, L, deg, light_pos, light_intensity, intensity_channels, head_pose, headrel_light_pos, light_sh):
    _lib.call("gol_light_sh_fwd", c_int(B), c_int(L), c_int(deg), _p(light_pos), _p(light_intensity),
              c_int(intensity_channels), _p(head_pose), _p(headrel_light_pos), _p(light_sh), stream_ptr())


def _check(name, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.GoliathHipError(f"{name} needs CUDA(HIP) tensors; there is no CPU path")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise _lib.GoliathHipError(f"{name} is forward-only: call it under torch.no_grad() or with detached inputs")


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def dir2sh(deg: int, dirs: torch.Tensor) -> torch.Tensor:
    """dir2sh_torch(deg, dirs): dirs[...,3] (used as they are, not normalised) -> [...,(deg+1)^2] float32."""
    deg = _deg(deg)
    if dirs.dim() < 1 or dirs.shape[-1] != 3:
        raise ValueError("dirs must be [...,3]")
    _check("dir2sh", dirs)
    d = _f32c(dirs).reshape(-1, 3)
    out = torch.empty(d.shape[0], (deg + 1) ** 2, dtype=torch.float32, device=d.device)
    with _lib.device_guard(d.device):
        _abi_sh_basis_fwd(M=d.shape[0], deg=deg, dirs=d, coeffs=out)
    return out.reshape(*dirs.shape[:-1], (deg + 1) ** 2)


def _light_sh(light_pos, light_intensity, head_pose, deg, want_pos):
    B, L = light_pos.shape[:2]
    C = light_intensity.shape[-1]
    pos = torch.empty(B, L, 3, dtype=torch.float32, device=light_pos.device) if want_pos else None
    out = torch.empty(B, 3, (deg + 1) ** 2, dtype=torch.float32, device=light_pos.device)
    with _lib.device_guard(light_pos.device):
        _abi_light_sh_fwd(B=B, L=L, deg=deg, light_pos=light_pos, light_intensity=light_intensity, intensity_channels=C,
                          head_pose=head_pose, headrel_light_pos=pos, light_sh=out)
    return pos, out


def headrel_light_sh(light_pos: torch.Tensor, light_intensity: torch.Tensor, head_pose, deg: int):
    """light_pos[B,L,3], light_intensity[B,L,1 or 3], head_pose[B,3,4] (None: identity) -> (headrel_light_pos[B,L,3],
    headrel_light_sh[B,3,(deg+1)^2]), one launch."""
    deg = _deg(deg)
    if light_pos.dim() != 3 or light_pos.shape[-1] != 3:
        raise ValueError("light_pos must be [B,L,3]")
    B, L = light_pos.shape[:2]
    if light_intensity.dim() != 3 or tuple(light_intensity.shape[:2]) != (B, L) or light_intensity.shape[-1] not in (1, 3):
        raise ValueError("light_intensity must be [B,L,1] or [B,L,3]")
    if head_pose is not None and tuple(head_pose.shape) != (B, 3, 4):
        raise ValueError("head_pose must be [B,3,4]")
    _check("headrel_light_sh", light_pos, light_intensity, head_pose)
    return _light_sh(_f32c(light_pos), _f32c(light_intensity), None if head_pose is None else _f32c(head_pose), deg, True)


def random_light_sh(deg: int, batch: int, device, dtype):
    """rgca.py:590-613 under no_grad: light_dir = F.normalize(th.rand(batch, 1, 3) - 0.5) (the draw goliath_amd.rgca.
    random_light_sh makes) and its SH coefficients for unit intensity, expanded over the three channels by the kernel."""
    deg = _deg(deg)
    if torch.device(device).type != "cuda":
        raise _lib.GoliathHipError("random_light_sh needs a CUDA(HIP) device; there is no CPU path")
    with torch.no_grad():
        raw = torch.rand(batch, 1, 3, device=device, dtype=dtype) - 0.5
        light_dir = F.normalize(raw, p=2, dim=-1)
        _, light_sh = _light_sh(_f32c(light_dir), torch.ones(batch, 1, 1, dtype=torch.float32, device=raw.device), None, deg,
                                False)
    return light_dir, light_sh.to(dtype)
