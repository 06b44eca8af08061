"""Mask operators on top of the C ABI (csrc/imgfam.hip): one tiled pass each, no host sync, graph-capturable.

  depth_discontinuity_mask(depth, threshold, kscale, pool_ksize)  <- ca_code/utils/geom.py:768-794 depth_discontuity_mask
  erode(x, ks)                                                    <- ca_code/utils/image.py:393-422 erode
"""
import torch

from . import _lib
from ._lib import c_float, c_int, fptr, ptr, stream_ptr


def depth_discontinuity_mask(depth: torch.Tensor, threshold: float = 40.0, kscale: float = 4.0,
                             pool_ksize: int = 3) -> torch.Tensor:
    """depth [B,1,H,W] -> torch.bool [B,1,H,W]: set where a Sobel gradient norm above `threshold` lies within the
    pool_ksize x pool_ksize window (1, 3 or 5).  `kscale` is unused, as in the reference."""
    if not depth.is_cuda:
        raise _lib.GoliathHipError("depth_discontinuity_mask needs a CUDA(HIP) tensor; there is no CPU path")
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"depth_discontinuity_mask: depth {tuple(depth.shape)} is not [B,1,H,W]")
    B, _, H, W = depth.shape
    d = depth.detach().to(torch.float32).contiguous()
    out = torch.empty(depth.shape, device=depth.device, dtype=torch.bool)
    with _lib.device_guard(depth.device):
        _lib.call("gol_depth_disc_mask", c_int(B), c_int(H), c_int(W), c_int(int(pool_ksize)), c_float(float(threshold)),
                  fptr(d), ptr(out.view(torch.uint8), torch.uint8), stream_ptr())
    return out


def erode_planes(x: torch.Tensor, ks: int) -> torch.Tensor:
    """gol_mask_erode over the [...,H,W] planes of a float (values in [0,1]) or boolean x: float32 0 / 1 of x's shape."""
    if not x.is_cuda:
        raise _lib.GoliathHipError("erode needs a CUDA(HIP) tensor; there is no CPU path")
    if x.dim() < 2:
        raise ValueError(f"erode: {tuple(x.shape)} has no [H,W] planes")
    is_u8 = x.dtype in (torch.bool, torch.uint8)
    src = x.detach().contiguous()
    src = src.view(torch.uint8) if x.dtype == torch.bool else (src if is_u8 else src.to(torch.float32))
    H, W = x.shape[-2:]
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    with _lib.device_guard(x.device):
        _lib.call("gol_mask_erode", c_int(x.numel() // max(H * W, 1)), c_int(H), c_int(W), c_int(int(ks)), c_int(int(is_u8)),
                  ptr(src), fptr(out), stream_ptr())
    return out


def erode(x: torch.Tensor, ks: int) -> torch.Tensor:
    """The reference's erode: a pixel survives iff every in-image pixel of its ks x ks window is set (float x: equals 1; the
    operator is defined for values in [0,1]).  ks odd, 1 .. 31.  Returns x's dtype; a 3-D x comes back as [B,1,H,W]."""
    out = erode_planes(x, ks)
    if out.dim() == 3:
        out = out[:, None]
    return out > 0 if x.dtype == torch.bool else out.to(x.dtype)
