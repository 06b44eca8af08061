"""The SG prefilter's cases and the torch composition of its math (shared by tests/golden/make_envprefilter_golden.py,
tests/test_envprefilter_api.py and tests/test_gpu_envprefilter.py).

The composition is ca_code/utils/envmap.py:251-323 (prefilterEnvmapSG with importance_sample_sg, dir2uv and sample_uv) with the
draws handed in, in the dtype it is asked for and on the device of its inputs:
    phi = 2 pi Xi0, theta = sqrt2 sigma erfinv(Xi1 erf(pi / (sqrt2 sigma))), H = (cos phi sin theta, sin phi sin theta, cos theta)
    up = (0,0,1) where n_z < 0.999 else (1,0,0), t = normalize(up x n), b = n x t, d = normalize(t H_x + b H_y + n H_z)
    u = atan2(d_x, d_z) / pi, v = 2 acos(d_y) / pi - 1, grid_sample(bilinear, align_corners=False, padding_mode="border")
    out = (sum_i colour_i) / S, the colours added one after the other
One deviation, the kernel's: d_y is clamped to [-1, 1] before acos.
"""
import hashlib
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "envprefilter_golden.npz")

CUT_EPS = 1e-6   # |d_x| below this behind the seam (d_z < 0): atan2 sits on its cut, u = +-1 are the two borders of the map
XI_LAST = float(np.float32(1.0) - np.float32(2.0 ** -24))   # the largest float32 below 1

# the statistics case: level_directions(6, 12), a 16 x 32 noise map, sigma 0.4
STAT_GRID, STAT_MAP, STAT_SIGMA, STAT_MAP_SEED = (6, 12), (16, 32), 0.4, 77
STAT_S, STAT_SEEDS, STAT_CONVERGED_S = (64, 1024), 8, 2 ** 18
# the pyramid case
PYR_SIZE, PYR_S, PYR_SEED, PYR_SIGMA_STEP, PYR_LEVELS = (32, 64), 16, 4242, 0.2, 4


# ---- the composition ------------------------------------------------------------------------------------------------------
def sample_directions(xi, n, sigma):
    """envmap.py:251-281 without the pdf: xi[N,2,H,W], n[N,3,H,W] -> d[N,3,H,W], in n's dtype."""
    xi = xi.to(n.dtype)
    phi = 2.0 * np.pi * xi[:, 0:1]
    sqrt2sigma = math.sqrt(2.0) * sigma
    theta = sqrt2sigma * torch.special.erfinv(xi[:, 1:2] * math.erf(np.pi / sqrt2sigma))
    cos_theta, sin_theta = torch.cos(theta), torch.sin(theta)
    H = torch.cat([torch.cos(phi) * sin_theta, torch.sin(phi) * sin_theta, cos_theta], dim=1)
    m = n[:, 2:3] < 0.999
    zero, one = torch.zeros_like(n[:, 0:1]), torch.ones_like(n[:, 0:1])
    up = torch.cat([torch.where(m, zero, one), zero, torch.where(m, one, zero)], dim=1)
    tangent = F.normalize(torch.cross(up, n, dim=1), dim=1)
    bitangent = torch.cross(n, tangent, dim=1)
    return F.normalize(tangent * H[:, 0:1] + bitangent * H[:, 1:2] + n * H[:, 2:3], dim=1)


def lookup(d, env):
    """envmap.py:284-302: d[N,3,H,W], env[N,3,He,We] -> [N,3,H,W]."""
    u = (1 / np.pi) * torch.atan2(d[:, 0], d[:, 2])
    v = 2 * ((1 / np.pi) * torch.acos(d[:, 1].clamp(-1.0, 1.0))) - 1.0
    return F.grid_sample(env, torch.stack([u, v], -1), padding_mode="border", align_corners=False)


def compose(sigma, v, env, xi, dtype=torch.float64, stats=None):
    """prefilterEnvmapSG(sigma, v, env, S) on the draws xi[S,B,2,H,W], every operand `dtype`.  stats (a dict): adds the number
    of samples with d_z < 0 and 0 < |d_x| < CUT_EPS to stats["near_cut"] and of those with d_z < 0 and d_x == 0 to
    stats["exact_cut"]."""
    v, env = v.to(dtype), env.to(dtype)
    acc = torch.zeros_like(v)
    for x in xi:
        d = sample_directions(x, v, sigma)
        if stats is not None:
            back, ax = d[:, 2] < 0, d[:, 0].abs()
            stats["near_cut"] = stats.get("near_cut", 0) + int((back & (ax < CUT_EPS) & (ax > 0)).sum())
            stats["exact_cut"] = stats.get("exact_cut", 0) + int((back & (ax == 0)).sum())
        acc += lookup(d, env)
    return acc / float(len(xi))


def compose_batched(sigma, v, env, xi, chunk=1024):
    """The float64 mean for B = 1 and many samples: `chunk` samples at a time ride on the batch axis (the sum is then
    torch's, not the sample-after-sample one).  v[1,3,H,W], env[1,3,He,We], xi[S,1,2,H,W] -> [1,3,H,W] float64."""
    v, env = v.double(), env.double()
    total = torch.zeros_like(v)
    for s in range(0, len(xi), chunk):
        x = xi[s:s + chunk, 0]
        d = sample_directions(x, v.expand(len(x), -1, -1, -1), sigma)
        total += lookup(d, env.expand(len(x), -1, -1, -1).contiguous()).sum(0, keepdim=True)
    return total / float(len(xi))


def max_err(got, want):
    return float((got.double().cpu() - want.double().cpu()).abs().max())


def rms_err(got, want):
    return float((got.double().cpu() - want.double().cpu()).pow(2).mean().sqrt())


# ---- the directions ---------------------------------------------------------------------------------------------------------
def level_directions(H, W):
    """light_decorator.py:75-90 restated (the tests compare goliath_amd.envprefilter.level_directions with it)."""
    theta, phi = torch.meshgrid((torch.arange(H, dtype=torch.float32) + 0.5) * np.pi / H,
                                (torch.arange(-W // 2, W // 2, dtype=torch.float32) + 0.5) * np.pi * 2 / W, indexing="ij")
    return torch.stack([torch.sin(theta) * torch.sin(phi), torch.cos(theta), -torch.sin(theta) * torch.cos(phi)], dim=0)[None]


def _unit(x, y, z):
    n = np.array([x, y, z], dtype=np.float64)
    return (n / np.linalg.norm(n)).astype(np.float32)


def hand_grid():
    """v[1,3,3,5]: both poles of the lookup (0, +-1, 0), both ends of the z axis ((0,0,1) takes the other `up`; (0,0,-1) has
    a zero tangent frame and sits ON the atan2 cut), (1,0,0), n_z just below and just above 0.999, a direction 1e-3 off the
    cut whose lobe straddles it, and generic ones."""
    below, above = _unit(0.03, 0.0335, 0.9989), _unit(0.03, -0.0295, 0.9991)
    assert below[2] < np.float32(0.999) <= above[2] and above[2] - below[2] < 3e-4
    rng = np.random.default_rng(31)
    generic = [_unit(*rng.normal(size=3)) for _ in range(6)]
    rows = [np.float32([0, 0, 1]), generic[0], np.float32([0, 1, 0]), below, np.float32([1, 0, 0]),
            generic[1], np.float32([0, 0, -1]), generic[2], _unit(1e-3, 0.2, -1.0), generic[3],
            above, np.float32([0, -1, 0]), generic[4], _unit(-1e-3, -0.4, -1.0), generic[5]]
    return torch.from_numpy(np.stack(rows).reshape(3, 5, 3).transpose(2, 0, 1).copy())[None]


def pole_grid():
    """level_directions(64, 128), the coarsest level of the real pyramid, at rows 30..33 and columns 126, 127, 0, 1: its four
    texels with n_z >= 0.999 (the other `up`) and their neighbours, [1,3,4,4]."""
    full = level_directions(64, 128)
    assert int((full[0, 2] >= 0.999).sum()) == 4
    v = full[:, :, 30:34][:, :, :, [126, 127, 0, 1]].contiguous()
    assert int((v[0, 2] >= 0.999).sum()) == 4
    return v


# ---- the maps -----------------------------------------------------------------------------------------------------------------
def hdr_map(seed, He, We):
    """HDR-like noise u v^4 20: neighbouring texels differ by the order of the maximum."""
    rng = np.random.default_rng(seed)
    u, v = rng.random((3, He, We)), rng.random((3, He, We))
    return torch.from_numpy((u * v ** 4 * 20.0).astype(np.float32))


def smooth_map(He, We):
    th = ((torch.arange(He, dtype=torch.float64) + 0.5) * math.pi / He)[:, None]
    ph = ((torch.arange(We, dtype=torch.float64) + 0.5) * 2.0 * math.pi / We)[None, :]
    chans = [2.0 + torch.cos(th + 0.4 * c) * torch.sin(ph + 0.9 * c) + 0.5 * torch.cos(2.0 * ph - 0.3 * c) * torch.sin(th) ** 2
             + 0.25 * torch.sin(3.0 * th + c) for c in range(3)]
    return torch.stack(chans).float()


def wrap_map(seed, He, We):
    """Noise whose last column equals its first."""
    m = hdr_map(seed, He, We)
    m[:, :, -1] = m[:, :, 0]
    return m


# name -> (grid, maps (one per batch element), S, sigma, seed of the draws)
CASES = {
    "hand_1x1_S3_s0.2": ("hand", [("hdr", 11, 1, 1)], 3, 0.2, 101),
    "hand_5x7_S1_s0.05": ("hand", [("hdr", 12, 5, 7)], 1, 0.05, 102),
    "hand_16x32_S64_s0.6": ("hand", [("hdr", 13, 16, 32)], 64, 0.6, 103),
    "hand_33x70_S130_s3.0_B2": ("hand", [("hdr", 14, 33, 70), ("hdr", 15, 33, 70)], 130, 3.0, 104),
    "hand_smooth33x70_S64_s0.2": ("hand", [("smooth", 0, 33, 70)], 64, 0.2, 105),
    "hand_wrap16x32_S130_s0.6": ("hand", [("wrap", 16, 16, 32)], 130, 0.6, 106),
    "hand_5x7_S3_s3.0_B2": ("hand", [("hdr", 17, 5, 7), ("wrap", 18, 5, 7)], 3, 3.0, 107),
    "pole_16x32_S64_s0.2": ("pole", [("hdr", 19, 16, 32)], 64, 0.2, 108),
    "pole_33x70_S130_s0.05": ("pole", [("hdr", 20, 33, 70)], 130, 0.05, 109),
}


def _map(kind, seed, He, We):
    return {"hdr": hdr_map, "wrap": wrap_map}[kind](seed, He, We) if kind != "smooth" else smooth_map(He, We)


def draws(seed, S, B, H, W):
    """xi[S,B,2,H,W] float32 from numpy.random.default_rng(seed), with Xi1 = 0 and Xi1 = 1 - 2^-24 placed by hand on the
    texel (1, 2) of batch element 0 (first and last sample) where the grid has one."""
    xi = np.random.default_rng(seed).random((S, B, 2, H, W), dtype=np.float32)
    if H > 1 and W > 2:
        xi[0, 0, 1, 1, 2] = 0.0
        xi[S - 1, 0, 1, 1, 2 if S > 1 else 1] = XI_LAST
    return torch.from_numpy(xi)


def case(name):
    """(sigma, v[B,3,H,W], env[B,3,He,We], xi[S,B,2,H,W]) of a parity case; batch element 1 sees the grid mirrored."""
    grid, maps, S, sigma, seed = CASES[name]
    v = hand_grid() if grid == "hand" else pole_grid()
    if len(maps) == 2:
        v = torch.cat([v, v.flip(2, 3)]).contiguous()
    env = torch.stack([_map(*m) for m in maps])
    return sigma, v, env, draws(seed, S, len(maps), v.shape[2], v.shape[3])


def checksum(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()[:16]


# ---- the statistics and the pyramid cases -----------------------------------------------------------------------------------
def stat_case():
    return STAT_SIGMA, level_directions(*STAT_GRID), hdr_map(STAT_MAP_SEED, *STAT_MAP)[None]


def pyramid_image():
    return hdr_map(PYR_SEED, *PYR_SIZE)


def pyramid_draws():
    """One xi[S,1,2,h,w] per prefiltered level, in the order light_decorator.py:70-91 consumes its rand_like calls."""
    rng = np.random.default_rng(PYR_SEED + 1)
    H, W = PYR_SIZE
    return [torch.from_numpy(rng.random((PYR_S, 1, 2, H >> i, W >> i), dtype=np.float32)) for i in range(1, PYR_LEVELS)]


def pyramid_inputs(image, miplevel=PYR_LEVELS):
    """light_decorator.py:64-90 restated without .cuda(): per prefiltered level (sigma index i + 1, directions, halved map)."""
    multisin = torch.sin((torch.arange(image.shape[1]) + 0.5) * np.pi / image.shape[1])[None, None, :, None].to(image.device)
    cur = image[None].clone() * multisin
    out = []
    for i in range(miplevel - 1):
        cur = F.interpolate(cur, None, scale_factor=0.5, mode="area")
        out.append((i + 1, level_directions(cur.shape[2], cur.shape[3]).to(image.device), cur))
    return out
