"""The env-relight driver's cases and their float64 composition (shared by tests/golden/make_env_driver_golden.py,
tests/test_env_driver_cpu.py and tests/test_gpu_env_driver.py).

The composition is this project's own statement of ca_code/utils/light_decorator.py:120-153 and
ca_code/utils/envmap.py:141-166, every operand float64:
    theta = (y + 0.5) 3.1415926 / H, phi = (x - W/2 + 0.5) 3.1415926 2 / W      (the truncated constant, as written there)
    vec = (sin theta sin phi, cos theta, sin theta cos phi), d = rot vec        (matmul(vec, rot_mat.T))
    clamp to [-1, 1], u = atan2(dx, dz) / pi, v = 2 acos(dy) / pi - 1
    grid_sample(bilinear, align_corners=False, padding_mode="border"): ix = ((u + 1) W - 1) / 2 clipped to [0, W - 1]
    envbg = new_env / perc90; probe = interpolate(new_env, (16, 32), bilinear, antialias=True) (ATen's operator in float64)
    S = sum probe sin((i + 0.5) pi / 16); envmap = env_scale probe / S; light_intensity = envmap.view(3, -1).t()
    norm_scale = env_scale / S; mip_scale = 2 pi norm_scale[0]
"""
import hashlib
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "env_driver_golden.npz")

CYCLE = 256
ENV_SCALE = 18.0
ENVMAP_DIST = 10000.0
SIZES = ((16, 32), (33, 70), (40, 72), (48, 96))
INDEX_BATCHES = ((0,), (7, 128, 201), (-5, 64))
GENERIC_RVEC = (0.3, -1.1, 0.7)
SMOOTH_SIZE = (48, 96)
FULL_SIZE, FULL_INDICES, FULL_SEED = (512, 1024), (7, 201), 512
CUT_EPS = 1e-6   # |dx| below this behind the seam (dz < 0): atan2 sits on its cut, u = +-1 are the two borders of the map
OUTPUTS = ("envbg", "envmap", "light_intensity", "norm_scale", "mip_scale")
# envbg is recorded on every STRIDE-th row at this size, starting at row (view number % STRIDE) -- the file has to stay
# under 1 MB; every other output, and envbg at the smaller sizes, is recorded in full.  err_ref32 is always taken over the
# whole array, and the tests that compare with the float64 composition use the whole array too.
ENVBG_ROW_STRIDE = {(48, 96): 3}


def hdr_image(seed, H, W):
    """HDR-like noise: u v^4 20 (most texels dark, a few bright: neighbouring texels differ by the order of the maximum)."""
    rng = np.random.default_rng(seed)
    u, v = rng.random((3, H, W)), rng.random((3, H, W))
    return torch.from_numpy((u * v ** 4 * 20.0).astype(np.float32))


def smooth_image(H, W):
    """A positive low-order trigonometric polynomial of the pixel angles, one phase per channel."""
    th = ((torch.arange(H, dtype=torch.float64) + 0.5) * math.pi / H)[:, None]
    ph = ((torch.arange(W, dtype=torch.float64) + 0.5) * 2.0 * math.pi / W)[None, :]
    chans = [2.0 + torch.cos(th + 0.4 * c) * torch.sin(ph + 0.9 * c) + 0.5 * torch.cos(2.0 * ph - 0.3 * c) * torch.sin(th) ** 2
             + 0.25 * torch.sin(3.0 * th + c) for c in range(3)]
    return torch.stack(chans).float()


def checksum(image):
    return hashlib.sha256(np.ascontiguousarray(image.numpy()).tobytes()).hexdigest()[:16]


def images():
    """name -> image of every small case set, in a fixed order."""
    out = {f"{H}x{W}": hdr_image(1000 + H, H, W) for H, W in SIZES}
    out["%dx%d_smooth" % SMOOTH_SIZE] = smooth_image(*SMOOTH_SIZE)
    return out


def full_image():
    return hdr_image(FULL_SEED, *FULL_SIZE)


def batches(full=False):
    """(tag, indices or None for the generic rotation) of every small image's calls, or of the full-size image's."""
    index_batches = (FULL_INDICES,) if full else INDEX_BATCHES
    return [("idx" + "_".join(str(i) for i in b), list(b)) for b in index_batches] + [("generic", None)]


def rotate64(image, rot):
    """new_env of one view in float64 and, for the generator's cut test, the smallest |dx| among directions with dz < 0 and
    the [H,W] mask of the pixels where it is below CUT_EPS."""
    image, rot = image.double(), rot.double()
    _, H, W = image.shape
    theta = ((torch.arange(H, dtype=torch.float64) + 0.5) * 3.1415926 / H)[:, None]
    phi = ((torch.arange(W, dtype=torch.float64) - W // 2 + 0.5) * 3.1415926 * 2 / W)[None, :]
    vec = torch.stack([torch.sin(theta) * torch.sin(phi), torch.cos(theta).expand(H, W), torch.sin(theta) * torch.cos(phi)], -1)
    d = (vec[..., None, :] * rot).sum(-1).clamp(-1.0, 1.0)          # d_j = sum_k vec_k rot[j][k]
    dx, dy, dz = d.unbind(-1)
    back = dz < 0
    cut = float(dx[back].abs().min()) if bool(back.any()) else float("inf")
    near = back & (dx.abs() < CUT_EPS)
    u = torch.atan2(dx, dz) / math.pi
    v = 2.0 * torch.acos(dy) / math.pi - 1.0
    ix = (((u + 1.0) * W - 1.0) / 2.0).clamp(0.0, W - 1.0)
    iy = (((v + 1.0) * H - 1.0) / 2.0).clamp(0.0, H - 1.0)
    x0, y0 = ix.floor().long(), iy.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    wx1, wy1 = ix - x0, iy - y0
    g = lambda yy, xx: image[:, yy, xx]
    out = (1 - wy1) * ((1 - wx1) * g(y0, x0) + wx1 * g(y0, x1)) + wy1 * ((1 - wx1) * g(y1, x0) + wx1 * g(y1, x1))
    return out, cut, near


def compose64(image, rots, perc90, env_scale=ENV_SCALE):
    """Every output of one call in float64 (+ "cut": the smallest |dx| behind the seam over the batch, "near_cut": the
    [B,H,W] mask of the pixels closer to it than CUT_EPS)."""
    new, cuts, near = zip(*(rotate64(image, r) for r in rots))
    new = torch.stack(new)
    probe = F.interpolate(new, (16, 32), mode="bilinear", antialias=True)
    sin = torch.sin((torch.arange(16, dtype=torch.float64) + 0.5) * math.pi / 16)[None, None, :, None]
    S = (probe * sin).sum(dim=(1, 2, 3))
    envmap = env_scale * probe / S[:, None, None, None]
    norm_scale = env_scale / S
    return dict(envbg=new / float(perc90), envmap=envmap, light_intensity=envmap.reshape(len(rots), 3, -1).transpose(1, 2),
                norm_scale=norm_scale, mip_scale=(2.0 * math.pi * norm_scale[:1]), cut=min(cuts),
                near_cut=torch.stack(near))


def recorded_rows(H, W, view):
    """The rows of view number `view` of a call whose envbg the fixture holds."""
    stride = ENVBG_ROW_STRIDE.get((H, W), 1)
    return slice(view % stride, None, stride)


def max_err(got, want):
    return float((got.double().cpu() - want.double()).abs().max())
