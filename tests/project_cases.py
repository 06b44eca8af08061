"""Edge scenes of the EWA projection (csrc/gol_project.h), their float32 / float64 oracles and the partition of every
(view, Gaussian) into conditioning classes.  Shared by tests/test_project_edge_scene.py (CPU: is the scene what it claims
to be) and tests/test_gpu_project_edges.py (GPU: HIP against float64, per class).

The scene: a head-sized ellipsoid of Gaussians with scales over more than three decades and un-normalised quaternions, seen
by three cameras in ONE batch -- one at 160 mm, one INSIDE the ellipsoid (Gaussians behind the camera, at the clip plane,
past the 1.3 tan(fov) clamp, larger than the image), one benign view at 700 mm -- each with fx != fy and the principal
point off the centre.  Two (glob_scale, clip) configurations."""
import functools
import math

import torch

from scenes import head_scene, look_at_viewmat

N = 4096 + 37          # the last workgroup of 256 lanes is partial
H, W = 96, 160
BLOCK = 16
CONFIGS = ((1.0, 0.1), (0.37, 25.0))   # (glob_scale, clip)
FOV_CLAMP = 1.3        # gsplat 0.1.11: lim = 1.3 tan(fov / 2)
EPS32 = 2.0 ** -23
MIN_CLASS = 30         # a class is judged in a configuration where it holds at least this many Gaussians: a rel-L2 over a
                       # handful is one Gaussian's rounding against another's, not a property of the kernel

FWD_OUTPUTS = ("xys", "depths", "conics", "comp", "cov3d", "opac_eff")
BWD_OUTPUTS = ("v_mean", "v_scale", "v_quat", "v_opacity")
# every (view, Gaussian) is in exactly one class, the first whose condition holds (float64 quantities only)
CLASSES = ("culled", "no_tile", "fov_clamped", "near_clip", "huge", "cancelling", "needle", "comp_lt_1e-3", "comp_1e-3",
           "comp_1e-2", "rest")
CANCELLING = 300.0     # det_orig = c00 c11 - c01^2 loses this factor of relative accuracy (cancellation_factor)
VISIBLE_CLASSES = CLASSES[2:]


def _eye(dist, azimuth, elevation=0.0):
    return (dist * math.sin(azimuth) * math.cos(elevation), dist * math.sin(elevation),
            -dist * math.cos(azimuth) * math.cos(elevation))


@functools.lru_cache(maxsize=None)
def edge_scene():
    """float32 CPU tensors: means / scales / quats / opacity [B,N,.] (every view sees the same Gaussians), viewmats [B,3,4],
    intrins [B,4] = (fx, fy, cx, cy).  Cached: callers must not write into it."""
    s = head_scene(N, H, W, seed=7, focal=110.0, cam_dist=160.0, scale_range=(0.02, 40.0))
    g = torch.Generator().manual_seed(11)
    quats = s["quats"] * (0.2 + 3.0 * torch.rand(N, 1, generator=g))          # |q| in [0.2, 3.2]
    viewmats = torch.stack([
        s["viewmat"],                                                          # 160 mm, inside the ellipsoid's bounding sphere
        look_at_viewmat(_eye(66.0, -1.1, 0.4), target=(10.0, -15.0, 5.0)),     # INSIDE the ellipsoid: Gaussians behind it
        look_at_viewmat(_eye(700.0, 0.55, -0.2)),                              # the benign view
    ])
    intrins = torch.tensor([[110.0, 95.0, 71.3, 52.9], [88.0, 120.0, 93.6, 41.2], [360.0, 352.0, 78.5, 49.25]])
    B = viewmats.shape[0]
    rep = lambda t: t[None].expand(B, *t.shape).contiguous()
    return dict(means=rep(s["means"]), scales=rep(s["scales"]), quats=rep(quats), opacity=rep(s["opacity"][:, 0]),
                viewmats=viewmats.contiguous(), intrins=intrins, H=H, W=W, B=B, N=N)


@functools.lru_cache(maxsize=None)
def constructed_rows():
    """Identity camera, clip = 0.25 (one view).  Rows: 0 a mean at z == clip exactly, 1 at the next float above it, 2 a scale
    of 500 at the image centre, 3 a centre left of the image whose radius reaches in, 4.. ordinary fillers."""
    n = 16
    g = torch.Generator().manual_seed(3)
    means = torch.cat([torch.randn(n, 2, generator=g) * 20.0, 150.0 + 50.0 * torch.rand(n, 1, generator=g)], 1)
    scales = 0.5 + 3.0 * torch.rand(n, 3, generator=g)
    quats = torch.randn(n, 4, generator=g)
    fx, fy, cx, cy = 110.0, 95.0, 80.0, 48.0
    up = float(torch.nextafter(torch.tensor(0.25), torch.tensor(1.0)))
    means[0] = torch.tensor([0.0, 0.0, 0.25])
    means[1] = torch.tensor([0.0, 0.0, up])
    scales[:2] = 0.05
    means[2] = torch.tensor([0.0, 0.0, 300.0])
    scales[2] = 500.0
    means[3] = torch.tensor([(-20.0 - cx) * 100.0 / fx, 0.0, 100.0])          # lands 20 px left of the image
    scales[3] = 12.0
    viewmat = torch.eye(4)[:3].contiguous()
    return dict(means=means[None].contiguous(), scales=scales[None].contiguous(), quats=quats[None].contiguous(),
                opacity=torch.rand(1, n, generator=g), viewmats=viewmat[None].contiguous(),
                intrins=torch.tensor([[fx, fy, cx, cy]]), H=H, W=W, B=1, N=n, clip=0.25, glob_scale=1.0)


def upstream(scene, seed=21):
    """Dense seeded upstream gradients of every differentiable projection output (float32 values)."""
    g = torch.Generator().manual_seed(seed)
    B, n = scene["B"], scene["N"]
    r = lambda *s: torch.randn(B, n, *s, generator=g)
    return dict(v_xy=r(2), v_depth=r(), v_conic=r(3), v_comp=r(), v_opac_eff=r())


def oracle_fwd(scene, glob_scale, clip, fp64):
    """The C oracle view by view in float32 (oracle/cref.py) or float64 (oracle/cref64.py), stacked to [B,N,.].
    opac_eff = opacity * comp in the oracle's own precision (render_gsplat.py:72)."""
    from oracle import cref, cref64

    dt = torch.float64 if fp64 else torch.float32
    cols = []
    for b in range(scene["B"]):
        fx, fy, cx, cy = (float(v) for v in scene["intrins"][b])
        a = (scene["means"][b], scene["scales"][b], glob_scale, scene["quats"][b], scene["viewmats"][b], fx, fy, cx, cy,
             scene["H"], scene["W"], BLOCK, clip)
        cols.append(cref64.project_fwd(*a) if fp64 else cref.project_gaussians(*a))
    xys, depths, radii, conics, comp, tiles, cov3d = (torch.stack(c) for c in zip(*cols))
    return dict(xys=xys, depths=depths, radii=radii, conics=conics, comp=comp, tiles=tiles, cov3d=cov3d,
                opac_eff=scene["opacity"].to(dt) * comp)


def oracle_bwd(scene, glob_scale, fwd, up, fp64):
    """The C oracle's vjp fed forward outputs `fwd` (of the same precision) and the upstream gradients `up`; the
    opac_eff = opacity * comp product is chained by hand in the oracle's precision.  v_quat is the vjp to the NORMALISED
    quaternion, as at the C ABI."""
    from oracle import cref, cref64

    dt = torch.float64 if fp64 else torch.float32
    opacity = scene["opacity"].to(dt)
    v_comp = up["v_comp"].to(dt) + up["v_opac_eff"].to(dt) * opacity
    cols = []
    for b in range(scene["B"]):
        fx, fy = float(scene["intrins"][b, 0]), float(scene["intrins"][b, 1])
        a = (scene["means"][b], scene["scales"][b], glob_scale, scene["quats"][b], scene["viewmats"][b], fx, fy,
             fwd["cov3d"][b], fwd["radii"][b], fwd["conics"][b], fwd["comp"][b], up["v_xy"][b].to(dt), up["v_depth"][b].to(dt),
             up["v_conic"][b].to(dt), v_comp[b])
        cols.append(cref64.project_bwd(*a) if fp64 else cref.project_gaussians_backward(*a)[2:])
    v_mean, v_scale, v_quat = (torch.stack(c) for c in zip(*cols))
    v_opacity = up["v_opac_eff"].to(dt) * fwd["comp"] * (fwd["radii"] > 0)
    return dict(v_mean=v_mean, v_scale=v_scale, v_quat=v_quat, v_opacity=v_opacity)


def camera_space(scene):
    """float64 camera-space coordinates [B,N,3] of the means."""
    V = scene["viewmats"].double()
    return torch.einsum("brc,bnc->bnr", V[:, :, :3], scene["means"].double()) + V[:, None, :, 3]


def fov_clamped(scene):
    """[B,N] bool: the camera-space direction is past the 1.3 tan(fov / 2) clamp in x or in y (float64)."""
    t = camera_space(scene)
    k = scene["intrins"].double()
    lim_x = (FOV_CLAMP * 0.5 * scene["W"] / k[:, 0])[:, None]
    lim_y = (FOV_CLAMP * 0.5 * scene["H"] / k[:, 1])[:, None]
    return ((t[..., 0] / t[..., 2]).abs() > lim_x) | ((t[..., 1] / t[..., 2]).abs() > lim_y)


def cancellation_factor(f64):
    """(c00 c11 + c01^2) / (c00 c11 - c01^2) of the 2-D covariance before the blur, from the float64 conic (the inverse of
    cov2d + 0.3 I): what the subtraction in det_orig amplifies the rounding of its operands by -- large for a Gaussian whose
    image is a needle, whatever its 3-D shape.  comp = sqrt(det_orig / det) inherits half of it, the gradients through
    comp all of it.  inf where there is no conic."""
    X = f64["conics"]
    det = 1.0 / (X[..., 0] * X[..., 2] - X[..., 1] ** 2)
    c00, c01, c11 = X[..., 2] * det - 0.3, -X[..., 1] * det, X[..., 0] * det - 0.3
    return (c00 * c11 + c01 ** 2) / (c00 * c11 - c01 ** 2).abs()


def classify(scene, glob_scale, clip, f64):
    """name -> [B,N] bool, a partition: the first class of CLASSES whose condition holds.  `f64` = oracle_fwd(..., fp64=True).
    Nothing here looks at a float32 number."""
    tz = camera_space(scene)[..., 2]
    sc = scene["scales"].double()
    cond = {
        "culled": tz <= clip,
        "no_tile": f64["radii"] == 0,
        "fov_clamped": fov_clamped(scene),
        "near_clip": tz < 3.0 * clip + 1.0,
        "huge": f64["radii"] > max(scene["H"], scene["W"]),
        "cancelling": cancellation_factor(f64) > CANCELLING,
        "needle": sc.max(-1).values / sc.min(-1).values > 100.0,
        "comp_lt_1e-3": f64["comp"] < 1e-3,
        "comp_1e-3": f64["comp"] < 1e-2,
        "comp_1e-2": f64["comp"] < 1e-1,
        "rest": torch.ones_like(tz, dtype=torch.bool),
    }
    taken = torch.zeros_like(tz, dtype=torch.bool)
    out = {}
    for name in CLASSES:
        out[name] = cond[name] & ~taken
        taken |= out[name]
    return out


def class_rel_l2(got, want, mask):
    """rel-L2 of `got` against the float64 `want` over the Gaussians of `mask` [B,N]."""
    d = (got.double() - want)[mask]
    return float(d.norm() / want[mask].norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def reference(cfg_index):
    """Everything the CPU side knows about one configuration, computed once and shared (read-only): both oracles forward and
    backward and the classes."""
    scene = edge_scene()
    glob_scale, clip = CONFIGS[cfg_index]
    up = upstream(scene)
    f64 = oracle_fwd(scene, glob_scale, clip, True)
    f32 = oracle_fwd(scene, glob_scale, clip, False)
    return dict(scene=scene, glob_scale=glob_scale, clip=clip, up=up, f64=f64, f32=f32,
                b64=oracle_bwd(scene, glob_scale, f64, up, True), b32=oracle_bwd(scene, glob_scale, f32, up, False),
                classes=classify(scene, glob_scale, clip, f64))


ENSEMBLE = 8


def ensemble_rms(scene, glob_scale, clip, up, classes, post=None):
    """The float32 oracle's rel-L2 against float64 per (class, output) as an EXPECTED value instead of one draw: the root mean
    square over ENSEMBLE copies of the scene whose means, scales and quaternions are moved by at most one float32 rounding
    (x (1 + eps32 u), u uniform in [-1, 1]), each copy judged against the float64 oracle on the same copy, so that only the
    float32 arithmetic's error is measured.  This is the conditioning of a class as float32 sees it: in a class whose
    error is one or two Gaussians' cancellation noise (a projected needle's det_orig = c00 c11 - c01^2 loses
    (c00 c11 + c01^2) / det_orig ~ 1e4 of relative accuracy) a single draw moves by a factor of 3 between copies, and between
    machines whose libm rounds the scene's own construction differently.  Nothing here looks at a HIP number.
    post(bwd, fp64) may rewrite the backward's outputs (the chain through the quaternion normalisation).
    Returns {(class, output): rms}."""
    acc = {}
    for k in range(ENSEMBLE):
        g = torch.Generator().manual_seed(1000 + k)
        copy = dict(scene)
        for name in ("means", "scales", "quats"):
            u = 2.0 * torch.rand(scene[name].shape, generator=g) - 1.0
            copy[name] = (scene[name] * (1.0 + EPS32 * u)).contiguous()
        sides = []
        for fp64 in (False, True):
            f = oracle_fwd(copy, glob_scale, clip, fp64)
            b = oracle_bwd(copy, glob_scale, f, up, fp64)
            sides.append({**f, **(post(b, fp64) if post else b)})
        same = sides[0]["radii"] == sides[1]["radii"]     # a copy may move a Gaussian across a ceil(): not arithmetic error
        for cname, mask in classes.items():
            for o in FWD_OUTPUTS + BWD_OUTPUTS:
                acc.setdefault((cname, o), []).append(class_rel_l2(sides[0][o], sides[1][o], mask & same) ** 2)
    return {key: math.sqrt(sum(v) / len(v)) for key, v in acc.items()}


@functools.lru_cache(maxsize=None)
def conditioning(cfg_index):
    """ensemble_rms of one configuration of the edge scene, computed once (and only when a judged figure asks for it)."""
    r = reference(cfg_index)
    return ensemble_rms(r["scene"], r["glob_scale"], r["clip"], r["up"], r["classes"])
