"""The SG prefilter that makes an environment map usable by the relight path (ca_code/utils/envmap.py:305-323
prefilterEnvmapSG; ca_code/utils/light_decorator.py:64-94 EnvSpinDecorator._set_lightmap builds the pyramid with it), fused.

  prefilter_sg(sigma, v, env_tex, num_samples=1, *, xi=None, seed=0, sample_offset=0) -> [B,3,H,W]
      prefilterEnvmapSG's positional signature and result, from two launches (csrc/envprefilter.hip: gol_envprefilter_sg)
      instead of num_samples Python iterations of two dozen ATen kernels.  xi[S,B,2,H,W]: the draws the reference's
      rand_like(v[:, :2]) would return, in iteration order (the parity mode).  Without xi the kernel draws its own
      (Philox-4x32-10 keyed by seed, batch element, texel and sample_offset + i): S samples in one call equal two calls of
      S / 2 with sample_offset 0 and S / 2, up to the rounding of the two means.
  level_directions(H, W, device)    the texel-centre directions of light_decorator.py:75-90, [1,3,H,W] float32
  build_pyramid(image[3,H,W], sigma_step=0.2, miplevel=4, num_samples=4096, *, seed=0, xi=None)
      -> the list of [1,3,H/2^i,W/2^i] levels of light_decorator.py:64-92 on the image's device: level 0 the image itself,
      level i >= 1 prefilter_sg(i sigma_step, level_directions, halved^i(image sin row weight)).  xi: one [S,1,2,h,w] tensor
      per prefiltered level.  Without xi level i draws with seed + i - 1.

Forward only: with grad mode on and an input that requires grad these raise.  No host sync; launched on the current stream.
There is no CPU path (level_directions is plain tensor code and runs anywhere).
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import c_double, c_i64, c_int, stream_ptr


def _p(x):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else _lib.ptr(x, torch.float32)


def _abi_envprefilter_sg(*, B, H, W, He, We, S, sigma, v, env_tex, xi, seed, sample_offset, scratch, out):
    _lib.call("gol_envprefilter_sg", c_int(B), c_int(H), c_int(W), c_int(He), c_int(We), c_int(S), c_double(sigma), _p(v),
              _p(env_tex), _p(xi), c_i64(seed), c_i64(sample_offset), _p(scratch), _p(out), stream_ptr())


def _scratch_floats(B, He, We):
    fn = _lib.load().gol_envprefilter_scratch_floats
    fn.restype = ctypes.c_int64
    return int(fn(c_int(B), c_int(He), c_int(We)))


def _signed64(x):
    """Any Python int as the int64 with the same low 64 bits (seeds are often unsigned)."""
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >> 63 else x


def prefilter_sg(sigma, v, env_tex, num_samples=1, *, xi=None, seed=0, sample_offset=0):
    tensors = [("v", v), ("env_tex", env_tex)] + ([("xi", xi)] if xi is not None else [])
    for name, t in tensors:
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a tensor")
        if torch.is_grad_enabled() and t.requires_grad:
            raise _lib.GoliathHipError("prefilter_sg is forward-only: call it under torch.no_grad() or with detached inputs")
    for name, t in tensors:
        if not t.is_cuda:
            raise _lib.GoliathHipError(f"prefilter_sg needs CUDA(HIP) tensors, {name} is on {t.device}; there is no CPU path")
        if t.dtype != torch.float32:
            raise _lib.GoliathHipError(f"{name} must be float32, got {t.dtype}")
    if v.dim() != 4 or v.shape[1] != 3 or env_tex.dim() != 4 or env_tex.shape[1] != 3 or env_tex.shape[0] != v.shape[0]:
        raise ValueError(f"v must be [B,3,H,W] and env_tex [B,3,He,We], got {tuple(v.shape)} and {tuple(env_tex.shape)}")
    B, _, H, W = (int(s) for s in v.shape)
    He, We = int(env_tex.shape[2]), int(env_tex.shape[3])
    S = int(num_samples)
    sigma = float(sigma)
    if S < 1:
        raise ValueError(f"num_samples must be at least 1, got {num_samples}")
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError(f"sigma must be positive and finite, got {sigma}")
    if min(B, H, W, He, We) < 1:
        raise ValueError("empty input")
    if int(sample_offset) < 0:
        raise ValueError("sample_offset must not be negative")
    if xi is not None and tuple(xi.shape) != (S, B, 2, H, W):
        raise ValueError(f"xi must be [num_samples,B,2,H,W] = {(S, B, 2, H, W)}, got {tuple(xi.shape)}")
    dev = v.device
    if env_tex.device != dev or (xi is not None and xi.device != dev):
        raise ValueError("v, env_tex and xi must be on one device")
    v, env_tex = v.detach().contiguous(), env_tex.detach().contiguous()
    xi = None if xi is None else xi.detach().contiguous()
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    scratch = torch.empty(max(_scratch_floats(B, He, We), 4), dtype=torch.float32, device=dev)
    with _lib.device_guard(dev):
        _abi_envprefilter_sg(B=B, H=H, W=W, He=He, We=We, S=S, sigma=sigma, v=v, env_tex=env_tex, xi=xi,
                             seed=_signed64(seed), sample_offset=int(sample_offset), scratch=scratch, out=out)
    return out


def level_directions(H, W, device="cpu"):
    """light_decorator.py:75-90 for a level of H x W texels, the reference's own float32 expressions (so that the
    n_z < 0.999 decision of the sampler falls as it does there), [1,3,H,W] on `device`."""
    H, W = int(H), int(W)
    theta, phi = torch.meshgrid(
        (torch.arange(H, dtype=torch.float32) + 0.5) * np.pi / H,
        (torch.arange(-W // 2, W // 2, dtype=torch.float32) + 0.5) * np.pi * 2 / W, indexing="ij")
    vec = torch.stack([torch.sin(theta) * torch.sin(phi), torch.cos(theta), -torch.sin(theta) * torch.cos(phi)], dim=0)
    return vec.to(device)[None]


def halved_levels(image, miplevel=4):
    """The maps light_decorator.py:64-72 hands to the prefilter: image[None] times the sin row weight, halved i times with
    interpolate(mode="area"), for i = 1 .. miplevel - 1.  Plain tensor code on the image's device."""
    H = image.shape[1]
    multisin = torch.sin((torch.arange(H) + 0.5) * np.pi / H)[None, None, :, None].to(image.device)
    cur = image[None].clone() * multisin
    out = []
    for _ in range(miplevel - 1):
        cur = F.interpolate(cur, None, scale_factor=0.5, mode="area")
        out.append(cur)
    return out


def build_pyramid(image, sigma_step=0.2, miplevel=4, num_samples=4096, *, seed=0, xi=None):
    if not torch.is_tensor(image) or image.dim() != 3 or image.shape[0] != 3:
        raise ValueError("image must be a [3,H,W] tensor")
    if torch.is_grad_enabled() and image.requires_grad:
        raise _lib.GoliathHipError("build_pyramid is forward-only: call it under torch.no_grad() or with a detached image")
    if not image.is_cuda:
        raise _lib.GoliathHipError("build_pyramid needs a CUDA(HIP) image; there is no CPU path")
    if image.dtype != torch.float32:
        raise _lib.GoliathHipError(f"image must be float32, got {image.dtype}")
    miplevel = int(miplevel)
    if miplevel < 1:
        raise ValueError("miplevel must be at least 1")
    if xi is not None and len(xi) != miplevel - 1:
        raise ValueError(f"xi must hold one tensor per prefiltered level ({miplevel - 1})")
    image = image.detach()
    levels = [image[None].clone()]
    for i, env in enumerate(halved_levels(image, miplevel)):
        h, w = int(env.shape[2]), int(env.shape[3])
        if min(h, w) < 1:
            raise ValueError(f"a {tuple(image.shape[1:])} image has no level {i + 1}")
        levels.append(prefilter_sg((i + 1) * sigma_step, level_directions(h, w, image.device), env, num_samples,
                                   xi=None if xi is None else xi[i], seed=int(seed) + i))
    return levels
