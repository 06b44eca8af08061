"""Relight-visualisation probe: the `envbg` branch of AutoEncoder.forward (rgca.py:232-245, what run_vis_relight.py:110-122
runs) with dropin.patch_relight_vis() off and on, and its two halves alone.

Setup: one view (run_vis_relight's batch), 2048 x 1334, the Gaussians of tests/scenes.head_scene, a 512 x 1024 environment.
goliath_amd.rgca.autoencoder_forward runs on a stand-in model whose encoder / decoder hand back fixed per-Gaussian
predictions (the decoder is the same work with the flag off and on; it is left out of the frame), so a frame is: render(s)
+ image tail + env background + breakdown.  Without a `projected` hand-over every render projects its Gaussians itself:
flag off = 3 x (project + bin + sort + raster) + the PyTorch compose, flag on = 1 x that + one N-channel list walk + the HIP
compose; the flagged frame's render is also timed without / with the extra channels, and the permute alone.  (In the real
model the first render of either path starts from the shading kernel's records: one projection less on both sides.)

The PyTorch compose timed here is `baseline_compose` below, this project's own composition of the operators the reference
spends its time in (a bicubic grid_sample at full resolution, a depthwise 101 x 101 conv2d with padding 50, a second bicubic
lookup for the 200 x 200 ball, an elementwise composite) -- ca_code is not importable where this runs.  It makes fewer
elementwise passes than the reference (no zeros_like temporaries, the ball blended in its corner only); those passes are
some 0.02 ms each at this size.  tests/ check the HIP operators against the reference itself; the baseline only has to
cost what the reference's operators cost.

Steps are interleaved (off, on, off, on, ...), each timed with its own HIP event pair; medians are reported.
Prints one JSON line (and writes it to --out).

    python tools/relight_vis_probe.py [--steps 20] [--warmup 3] [--gaussians 250000,1048576] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from goliath_amd import _lib, build, envbg, rgca  # noqa: E402
from goliath_amd.render_gs import render_batch  # noqa: E402
from scenes import head_scene  # noqa: E402


def _equirect(env, dx, dy, dz):
    """Bicubic lookup of an equirectangular map env[B,3,He,We] in the directions (dx, dy, dz) [B,h,w]: longitude over pi
    and colatitude mapped to [-1, 1] are grid_sample's normalised coordinates."""
    lon = torch.atan2(dx, dz) / math.pi
    colat = torch.acos(dy) * (2.0 / math.pi) - 1.0
    return F.grid_sample(env, torch.stack((lon, colat), dim=-1), mode="bicubic", padding_mode="border", align_corners=True)


def baseline_compose(render, alpha, env, K, Rt, ball=envbg.BALL, focal_scale=0.2):
    """A PyTorch baseline built from the operators the issue lists for the reference's compose: a bicubic grid_sample of the
    environment at full resolution, a depthwise 101 x 101 conv2d with zero padding 50, a second bicubic lookup for the
    ball x ball mirror ball, and the elementwise composite.  Directions are formed per component by broadcasting."""
    B, _, H, W = render.shape
    dev = render.device
    Rm = Rt[:, :3, :3]
    col = (torch.arange(W, device=dev, dtype=torch.float32)[None, :] - K[:, 0, 2, None]) / (K[:, 0, 0, None] * focal_scale)
    row = (torch.arange(H, device=dev, dtype=torch.float32)[None, :] - K[:, 1, 2, None]) / (K[:, 1, 1, None] * focal_scale)

    def rotated(x, y, z, j):   # component j of R^T (x, y, z)
        return Rm[:, 0, j, None, None] * x + Rm[:, 1, j, None, None] * y + Rm[:, 2, j, None, None] * z

    x, y, one = col[:, None, :], row[:, :, None], torch.ones(1, 1, 1, device=dev)
    d = [rotated(x, y, one, j) for j in range(3)]
    inv = torch.rsqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    seen = _equirect(env, d[0] * inv, d[1] * inv, d[2] * inv)
    taps = envbg.blur_taps().to(device=dev, dtype=torch.float32)
    seen = F.conv2d(seen, torch.outer(taps, taps).expand(3, 1, -1, -1).contiguous(), padding=envbg.TAPS // 2, groups=3)
    out = torch.addcmul(render, 1.0 - alpha, seen.clamp(0.0, 1.0))
    # the mirror ball: the view direction (0, 0, 1) reflected at a unit sphere seen orthographically in the corner
    t = torch.linspace(-1.0, 1.0, ball, device=dev)
    bx, by = t[None, None, :], t[None, :, None]
    r2 = bx * bx + by * by
    h = torch.sqrt((1.0 - r2).clamp(min=0.0))
    rx, ry, rz = 2.0 * h * bx, 2.0 * h * by, 1.0 - 2.0 * h * h
    look = _equirect(env, *(rotated(rx, ry, rz, j) for j in range(3)))
    corner = out[:, :, H - ball:, W - ball:]
    out[:, :, H - ball:, W - ball:] = torch.where((r2 < 1.0)[:, None], look, corner)
    return out


class _FixedDecoder:
    def __init__(self, preds):
        self.preds = preds

    def __call__(self, *a, **k):
        return dict(self.preds)


class _Model:
    """What autoencoder_forward reads of an AutoEncoder, with fixed per-Gaussian predictions."""
    training = False
    cal_enabled = learn_blur_enabled = False
    n_diff_sh = 2

    def __init__(self, preds, H, W):
        self.height, self.width = H, W
        self.encoder = lambda verts, color: {"embs": None}
        self.geomdecoder = lambda embs: {"face_geom": None}
        self.decoder = _FixedDecoder(preds)

    render = rgca.autoencoder_render
    forward = rgca.autoencoder_forward


def _install_stubs():
    for name in ("ca_code", "ca_code.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sh = types.ModuleType("ca_code.utils.sh")
    sh.dir2sh_torch = lambda n, d: torch.zeros(*d.shape[:-1], (n + 1) ** 2, device=d.device)
    env = types.ModuleType("ca_code.utils.envmap")
    env.compose_envmap = baseline_compose
    sys.modules["ca_code.utils.sh"], sys.modules["ca_code.utils.envmap"] = sh, env


def _timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median_ms(fns, steps, warmup):
    """Interleaved: every step runs each of `fns` once, in order; per function the median over the timed steps."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for i, fn in enumerate(fns):
            ms[i].append(_timed_ms(fn))
    return [round(statistics.median(m), 3) for m in ms], [round(min(m), 3) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", default="250000,1048576")
    ap.add_argument("--size", default="2048,1334", help="H,W")
    ap.add_argument("--env", default="512,1024", help="He,We")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relight_vis_probe needs a GPU: nothing is measured without one")
    H, W = (int(v) for v in a.size.split(","))
    He, We = (int(v) for v in a.env.split(","))
    _install_stubs()
    gen = torch.Generator().manual_seed(0)
    env = (torch.rand(1, 3, He, We, generator=gen) * 1.5).cuda()
    res = dict(probe="relight_vis", H=H, W=W, B=1, env=[He, We], steps=a.steps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), source_digest=build.source_digest(), frames={})
    K = Rt = None
    for N in (int(n) for n in a.gaussians.split(",")):
        s = head_scene(N, H, W, seed=0)
        preds = dict(primpos=s["means"][None], primscale=s["scales"][None], primqvec=s["quats"][None],
                     opacity=s["opacity"][None], color=s["colors"][None],
                     diff_color=torch.rand(1, N, 3, generator=gen) - 0.1, spec_color=torch.rand(1, N, 3, generator=gen) - 0.1)
        preds = {k: v.cuda().contiguous() for k, v in preds.items()}
        K = torch.tensor([[[s["fx"], 0.0, s["cx"]], [0.0, s["fy"], s["cy"]], [0.0, 0.0, 1.0]]]).cuda()
        Rt = s["viewmat"][None].cuda()
        batch = dict(head_pose=torch.eye(4)[:3][None].cuda(), campos=torch.zeros(1, 3).cuda(), registration_vertices=None,
                     color=None, light_intensity=torch.ones(1, 4, 1).cuda(), light_pos=torch.randn(1, 4, 3, generator=gen).cuda(),
                     n_lights=torch.full((1, 1), 4.0).cuda(), K=K, Rt=Rt, preconv_envmap=[env], envbg=env)
        m = _Model(preds, H, W)

        def frame(flag):
            def run():
                setattr(_Model, rgca.RELIGHT_VIS_FLAG, flag)
                with torch.no_grad():
                    return m.forward(**batch)["rgb"]
            return run

        off, on = frame(False)(), frame(True)()
        d = (on.double() - off.double())
        parity = dict(rel_l2=float(d.norm() / off.double().norm()), max_abs=float(d.abs().max()))
        (ms_off, ms_on), (min_off, min_on) = _median_ms([frame(False), frame(True)], a.steps, a.warmup)
        res["frames"][str(N)] = dict(off_ms=ms_off, on_ms=ms_on, off_min_ms=min_off, on_min_ms=min_on,
                                     off_fps=round(1000.0 / ms_off, 2), on_fps=round(1000.0 / ms_on, 2),
                                     speedup=round(ms_off / ms_on, 2), on_vs_off=parity)
        # where the flagged frame's time goes: the one render without and with the six extra channels (= the N-channel list
        # walk + its NHWC -> NCHW permute), and that permute alone
        extra = torch.cat([preds["diff_color"], preds["spec_color"]], -1).clamp(min=0.0)
        nhwc = torch.rand(1, H, W, 6, device="cuda")
        with torch.no_grad():
            (ms_r, ms_rx, ms_p), _ = _median_ms([lambda: render_batch(K, Rt, preds, H, W),
                                                 lambda: render_batch(K, Rt, preds, H, W, extra_colors=extra),
                                                 lambda: nhwc.permute(0, 3, 1, 2).contiguous()], a.steps, a.warmup)
        res["frames"][str(N)].update(render_ms=ms_r, render_with_extra_ms=ms_rx, permute_6ch_ms=ms_p)
        del m, preds, batch
    render = torch.rand(1, 3, H, W, generator=gen).cuda()
    alpha = torch.rand(1, 1, H, W, generator=gen).cuda()
    with torch.no_grad():
        ref = lambda: baseline_compose(render, alpha, env, K, Rt)
        hip = lambda: envbg.compose_envmap(render, alpha, env, K, Rt)
        img = lambda: envbg.env_background(env, K, Rt, H, W)
        (ms_ref, ms_hip, ms_img), (min_ref, min_hip, min_img) = _median_ms([ref, hip, img], a.steps, a.warmup)
        # device time of the two ABI calls on their own (events around each call, _lib.TIMING)
        _lib.TIMING = []
        for _ in range(a.steps):
            hip()
        torch.cuda.synchronize()
        per_call = {}
        for name, e0, e1 in _lib.TIMING:
            per_call.setdefault(name, []).append(e0.elapsed_time(e1))
        _lib.TIMING = None
    res["abi_call_ms"] = {k: round(statistics.median(v), 3) for k, v in per_call.items()}
    res["compose"] = dict(torch_ms=ms_ref, hip_ms=ms_hip, hip_image_only_ms=ms_img, torch_min_ms=min_ref, hip_min_ms=min_hip,
                          speedup=round(ms_ref / ms_hip, 1))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
