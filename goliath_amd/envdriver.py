"""The env-relight driver's per-frame work (ca_code/utils/light_decorator.py:102-164 EnvSpinDecorator.forward), fused.

  EnvSpin(image, env_scale, cycle=256, envmap_dist=10000.0, perc90=None, device="cuda")
      the state of one environment: the map on the device (uploaded once), the two tap tables of the antialiased reduction to
      16 x 32, np.percentile(image, 90) (computed once: the reference recomputes the same number per view and frame) and
      sphvec * envmap_dist
  EnvSpin.frame(index=None, lightrot=None)
      -> EnvFrame(envbg, envmap, light_intensity, light_pos, lightrot, norm_scale, mip_scale, n_lights): what :111-162 put
      into `data`, from three launches (csrc/envdriver.hip: gol_envspin_frame).  mip_scale is the `scale` of
      EnvSpinDecorator.mipmap (2 pi norm_scale[0]) as a 1-element device tensor: goliath_amd.shade hands its address to the
      shading kernel, nothing reads it on the host.
  spin_lightrot(index, cycle, device)     :113-119 for the whole batch
  tap_tables(H, W)                        the antialiased bilinear reduction as two 1-D tables (host, float64)

Forward only: with grad mode on and an input that requires grad these raise.  No host sync in frame() when `index` is a
device tensor or `lightrot` is given; launched on the current stream.  There is no CPU path (spin_lightrot and tap_tables
are plain tensor code and run anywhere).
"""
import collections
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import c_double, c_float, c_int, stream_ptr

PROBE_H, PROBE_W = 16, 32   # light_decorator.py:128-130

EnvFrame = collections.namedtuple(
    "EnvFrame", "envbg envmap light_intensity light_pos lightrot norm_scale mip_scale n_lights")


def _p(x, dtype=torch.float32):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else _lib.ptr(x, dtype)


def _abi_envspin_frame(*, B, H, W, image, rot, tap_y_start, tap_y_w, ky, tap_x_start, tap_x_w, kx, perc90, env_scale,
                       scratch, envbg, envmap, light_intensity, norm_scale, mip_scale):
    _lib.call("gol_envspin_frame", c_int(B), c_int(H), c_int(W), _p(image), _p(rot), _p(tap_y_start, torch.int32),
              _p(tap_y_w, torch.float64), c_int(ky), _p(tap_x_start, torch.int32), _p(tap_x_w, torch.float64), c_int(kx),
              c_float(perc90), c_double(env_scale), _p(scratch), _p(envbg), _p(envmap), _p(light_intensity), _p(norm_scale),
              _p(mip_scale), stream_ptr())


def _scratch_floats(B, H, W):
    fn = _lib.load().gol_envspin_scratch_floats
    fn.restype = ctypes.c_int64
    return int(fn(c_int(B), c_int(H), c_int(W)))


def _check_map_size(H, W):
    if H < PROBE_H or W < PROBE_W or W % 2:
        raise ValueError(f"the environment map must be at least {PROBE_H} x {PROBE_W} with an even width, got {H} x {W}")


def _table(M):
    """M[n_out, n_in] (one row per output) -> (start[n_out] int32, w[n_out, k] float64): per row the first non-zero column
    and the weights from there to the row's last non-zero one, padded with zeros to the longest row."""
    spans = []
    for row in M:
        nz = torch.nonzero(row).flatten()
        spans.append((int(nz[0]), int(nz[-1]) + 1))
    k = max(e - s for s, e in spans)
    w = torch.zeros(M.shape[0], k, dtype=torch.float64)
    for i, (s, e) in enumerate(spans):
        w[i, :e - s] = M[i, s:e]
    return torch.tensor([s for s, _ in spans], dtype=torch.int32), w


def tap_tables(H: int, W: int):
    """thf.interpolate(x[None], (16, 32), mode="bilinear", antialias=True) (light_decorator.py:128-130) of an [.,H,W] map as
    two 1-D tables, float64, on the host: the operator is separable and linear, so its response to the one-hot rows
    (eye(H) -> [16,H]) and columns (eye(W) -> [32,W]) is the operator.  Returns (y_start[16], y_w[16,ky], x_start[32],
    x_w[32,kx]); out[c,i,j] = sum_ab y_w[i,a] x_w[j,b] x[c, y_start[i] + a, x_start[j] + b]."""
    H, W = int(H), int(W)
    _check_map_size(H, W)
    with torch.no_grad():
        my = F.interpolate(torch.eye(H, dtype=torch.float64)[None, None], size=(PROBE_H, H), mode="bilinear",
                           antialias=True)[0, 0]
        mx = F.interpolate(torch.eye(W, dtype=torch.float64)[None, None], size=(W, PROBE_W), mode="bilinear",
                           antialias=True)[0, 0].t()
    return (*_table(my), *_table(mx))


def spin_lightrot(index, cycle, device):
    """light_decorator.py:113-119 for every view at once: rvec_to_R of the rotation by 2 pi index / cycle about +y, [B,3,3]
    float32 on `device`.  A list of ints: the angle is formed on the host in float64 and rounded to float32 (as
    th.Tensor([...]).float() does), one small upload.  A tensor: everything happens on `device`.  rvec_to_R
    (envmap.py:20-50) clamps the angle's magnitude n to 1e-6, so index 0 gives rn = 0 and exactly the identity."""
    cycle = float(cycle)
    if torch.is_tensor(index):
        if index.dim() != 1:
            raise ValueError("index must be [B]")
        angle = (2.0 * math.pi * index.detach().to(device=device, dtype=torch.float64) / cycle).float()
    else:
        host = torch.tensor([2.0 * math.pi * int(i) / cycle for i in index], dtype=torch.float64).float()
        angle = host.to(device)
    n = angle.abs().clamp(min=1e-6)
    s = angle / n                       # rn_y: +-1, or 0 for a zero angle
    sn = torch.sin(n) * s               # sin(n) N
    c = 1.0 - ((1.0 - torch.cos(n)) * s) * s   # I + ((1 - cos n) N) @ N on the diagonal
    z, o = torch.zeros_like(c), torch.ones_like(c)
    return torch.stack([c, z, sn, z, o, z, z - sn, z, c], -1).view(-1, 3, 3)   # 0 - sn: +0 for a zero angle, as I + (-0) is


def _sphvec():
    """light_decorator.py:42-52 (the directions of the 16 x 32 probe cells), [3,512] float32."""
    L = PROBE_H
    theta, phi = np.meshgrid((np.arange(L, dtype=np.float32) + 0.5) * np.pi / L,
                             (np.arange(-L, L, dtype=np.float32) + 0.5) * np.pi / L, indexing="ij")
    sph = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], axis=0).reshape((3, -1))
    return torch.from_numpy(sph.astype(np.float32))


class EnvSpin:
    def __init__(self, image, env_scale, cycle=256, envmap_dist=10000.0, perc90=None, device="cuda"):
        if not torch.is_tensor(image) or image.dim() != 3 or image.shape[0] != 3:
            raise ValueError("image must be a [3,H,W] tensor")
        H, W = int(image.shape[1]), int(image.shape[2])
        _check_map_size(H, W)
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.GoliathHipError("EnvSpin needs a CUDA(HIP) device; there is no CPU path")
        host = image.detach().to(torch.float32).cpu()
        if perc90 is None:
            perc90 = np.percentile(host.numpy(), 90)                      # light_decorator.py:123, once
        if not float(perc90) > 0.0:
            raise ValueError(f"perc90 must be positive, got {float(perc90)} (the reference then divides by the frame's maximum)")
        self.H, self.W, self.device = H, W, device
        self.perc90, self.env_scale, self.cycle = float(np.float32(perc90)), float(env_scale), cycle
        self.image = host.to(device).contiguous()
        ys, yw, xs, xw = tap_tables(H, W)
        self.ky, self.kx = yw.shape[1], xw.shape[1]
        self.tap_y_start, self.tap_y_w, self.tap_x_start, self.tap_x_w = (t.to(device).contiguous() for t in (ys, yw, xs, xw))
        self.light_pos = (float(envmap_dist) * _sphvec().t().contiguous()).to(device)[None]     # :144, :158
        self._n_lights = {}

    def frame(self, index=None, lightrot=None, want_envbg=True):
        """One frame of B views, from the spin `index` ([B] ints or a device tensor) or from `lightrot` [B,3,3] on the device.
        want_envbg=False skips the [B,3,H,W] background (returned as None)."""
        if (index is None) == (lightrot is None):
            raise ValueError("give either index or lightrot")
        if lightrot is None:
            if torch.is_tensor(index) and torch.is_grad_enabled() and index.requires_grad:
                raise _lib.GoliathHipError("EnvSpin.frame is forward-only: call it under torch.no_grad() or with detached inputs")
            lightrot = spin_lightrot(index, self.cycle, self.device)
        else:
            if not torch.is_tensor(lightrot) or lightrot.dim() != 3 or tuple(lightrot.shape[1:]) != (3, 3):
                raise ValueError("lightrot must be [B,3,3]")
            if not lightrot.is_cuda:
                raise _lib.GoliathHipError("EnvSpin.frame needs CUDA(HIP) tensors; there is no CPU path")
            if torch.is_grad_enabled() and lightrot.requires_grad:
                raise _lib.GoliathHipError("EnvSpin.frame is forward-only: call it under torch.no_grad() or with detached inputs")
            lightrot = lightrot.detach().to(device=self.device, dtype=torch.float32).contiguous()
        B, H, W, dev = lightrot.shape[0], self.H, self.W, self.device
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        envbg = new(B, 3, H, W) if want_envbg else None
        envmap, light_intensity = new(B, 3, PROBE_H, PROBE_W), new(B, PROBE_H * PROBE_W, 3)
        norm_scale, mip_scale = new(B), new(1)
        scratch = new(max(_scratch_floats(B, H, W), 1))
        with _lib.device_guard(dev):
            _abi_envspin_frame(B=B, H=H, W=W, image=self.image, rot=lightrot, tap_y_start=self.tap_y_start,
                               tap_y_w=self.tap_y_w, ky=self.ky, tap_x_start=self.tap_x_start, tap_x_w=self.tap_x_w,
                               kx=self.kx, perc90=self.perc90, env_scale=self.env_scale, scratch=scratch, envbg=envbg,
                               envmap=envmap, light_intensity=light_intensity, norm_scale=norm_scale, mip_scale=mip_scale)
        n_lights = self._n_lights.get(B)
        if n_lights is None:                                                                    # :161
            n_lights = self._n_lights[B] = torch.full((B, 1), float(PROBE_H * PROBE_W), dtype=torch.float32, device=dev)
        return EnvFrame(envbg, envmap, light_intensity, self.light_pos.expand(B, -1, -1), lightrot, norm_scale, mip_scale,
                        n_lights)
