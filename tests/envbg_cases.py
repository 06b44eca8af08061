"""TEST INFRASTRUCTURE: the seeded inputs of the environment-background tests (tests/test_gpu_relight_vis.py) and of their
golden generator (tests/golden/make_envbg_golden.py), built on the CPU so that both see the same numbers.

A case is (name, B, H, W, He, We, compose): compose=True runs compose_envmap (blurred background + mirror ball), compose=False
envmap_to_image alone with blurbg=False.  The shapes are the smallest that cross every boundary of csrc/envbg.hip:
  ball200     2 x 200 x 200, env 32 x 64    the ball square covers the image; distinct K, R, env per view (batch strides)
  strip1      1 x 232 x 216, env 64 x 128   one partial 256-wide strip of the row pass, partial 64 x 64 column tiles
  strip2      1 x 210 x 331, env 64 x 128   two strips, W not a multiple of 4
  bicubic     2 x 37 x 53,   env 16 x 32    no blur, no ball: view 0 looks backwards (the +-pi seam), view 1 at a pole

Environment: a constant plus longitude / latitude harmonics whose column 0 equals column We - 1 (the seam is continuous),
scaled by sin(theta) (constant at the poles, where u is ill-conditioned), plus a 3 x 4 block of +3 near the view centre that
drives the clamp.  render is uniform in [0, 1]; alpha uniform with the top third 0 and the bottom quarter 1."""
import math

import torch

CASES = (
    ("ball200", 2, 200, 200, 32, 64, True),
    ("strip1", 1, 232, 216, 64, 128, True),
    ("strip2", 1, 210, 331, 64, 128, True),
    ("bicubic", 2, 37, 53, 16, 32, False),
)
BG_CASE = "strip1"   # the case whose blurred, un-clamped background is stored as well
BALL = 200


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    return Rz @ Ry @ Rx


def environment(B, He, We, g):
    """[B,3,He,We] float32."""
    theta = torch.linspace(0.0, math.pi, He, dtype=torch.float64)[:, None]           # row 0 / He - 1: the poles
    phi = torch.linspace(0.0, 2.0 * math.pi, We, dtype=torch.float64)[None, :]        # column 0 == column We - 1
    env = torch.empty(B, 3, He, We, dtype=torch.float64)
    for b in range(B):
        for c in range(3):
            amp = 0.25 + 0.35 * torch.rand(3, generator=g, dtype=torch.float64)
            ph = 2.0 * math.pi * torch.rand(3, generator=g, dtype=torch.float64)
            h = (amp[0] * torch.cos(phi + ph[0]) + amp[1] * torch.cos(2 * phi + ph[1]) * torch.cos(2 * theta)
                 + amp[2] * torch.cos(3 * phi + ph[2]) * torch.sin(3 * theta))
            env[b, c] = 0.5 + torch.sin(theta) * h
        y0 = He // 2 - 1 + int(torch.randint(0, 2, (1,), generator=g))
        x0 = We // 2 - 2 + int(torch.randint(0, 3, (1,), generator=g))
        env[b, :, y0:y0 + 3, x0:x0 + 4] += 3.0
    return env.to(torch.float32)


def build(name):
    """dict(name, B, H, W, He, We, compose, envbg[B,3,He,We], K[B,3,3], Rt[B,3,4], render[B,3,H,W], alpha[B,1,H,W])."""
    idx = [c[0] for c in CASES].index(name)
    _, B, H, W, He, We, compose = CASES[idx]
    g = torch.Generator().manual_seed(7100 + idx)
    envbg = environment(B, He, We, g)
    K = torch.zeros(B, 3, 3, dtype=torch.float64)
    Rt = torch.zeros(B, 3, 4, dtype=torch.float64)
    for b in range(B):
        f = (2.2 + 0.6 * float(torch.rand(1, generator=g))) * W      # x focal_scale 0.2: a field of view around 90 degrees
        K[b, 0, 0], K[b, 1, 1] = f, f * (1.0 + 0.05 * float(torch.rand(1, generator=g)))
        K[b, 0, 2] = 0.5 * W + 7.0 * (float(torch.rand(1, generator=g)) - 0.5)
        K[b, 1, 2] = 0.5 * H + 7.0 * (float(torch.rand(1, generator=g)) - 0.5)
        K[b, 2, 2] = 1.0
        a = 0.35 * (torch.rand(3, generator=g, dtype=torch.float64) - 0.5)
        if name == "bicubic":      # view 0: about-face (u = +-1 in the image); view 1: looking along the map's pole
            a = a * 0.2 + (torch.tensor([0.0, math.pi, 0.0]) if b == 0 else torch.tensor([0.5 * math.pi, 0.0, 0.0])).double()
        Rt[b, :, :3] = _rot(float(a[0]), float(a[1]), float(a[2]))
        Rt[b, :, 3] = 100.0 * (torch.rand(3, generator=g, dtype=torch.float64) - 0.5)
    render = torch.rand(B, 3, H, W, generator=g)
    alpha = torch.rand(B, 1, H, W, generator=g)
    alpha[:, :, :H // 3] = 0.0
    alpha[:, :, H - H // 4:] = 1.0
    return dict(name=name, B=B, H=H, W=W, He=He, We=We, compose=compose, envbg=envbg, K=K.to(torch.float32),
                Rt=Rt.to(torch.float32), render=render, alpha=alpha)


def pixel_uv(case):
    """u, v [B,H,W] (float64) of envmap_to_image's pixel directions, for the generator's coverage assertions."""
    K, R = case["K"].double(), case["Rt"][:, :3, :3].double()
    y, x = torch.meshgrid(torch.arange(case["H"], dtype=torch.float64), torch.arange(case["W"], dtype=torch.float64),
                          indexing="ij")
    d = torch.stack([(x[None] - K[:, 0, 2, None, None]) / (K[:, 0, 0, None, None] * 0.2),
                     (y[None] - K[:, 1, 2, None, None]) / (K[:, 1, 1, None, None] * 0.2),
                     torch.ones(K.shape[0], case["H"], case["W"], dtype=torch.float64)], -1)
    d = torch.einsum("bxy,bhwx->bhwy", R, d)
    d = d / d.norm(dim=-1, keepdim=True)
    return torch.atan2(d[..., 0], d[..., 2]) / math.pi, 2.0 * torch.acos(d[..., 1]) / math.pi - 1.0


def regions(case):
    """(ball, rest): boolean [H,W] masks of the mirror-ball square and of everything else (compose cases)."""
    ball = torch.zeros(case["H"], case["W"], dtype=torch.bool)
    if case["compose"]:
        ball[case["H"] - BALL:, case["W"] - BALL:] = True
    return ball, ~ball
