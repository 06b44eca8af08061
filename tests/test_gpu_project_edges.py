"""GPU: the EWA projection (csrc/gol_project.h: project_point, project_vjp) at the frustum's edges, judged by float64.

The scene (tests/project_cases.py; tests/test_project_edge_scene.py checks it on the CPU) has Gaussians behind the camera,
at the clip plane, past the 1.3 tan(fov) clamp, larger than the image, needles, discs and compensations down to 1e-4, three
different cameras in one launch (fx != fy, principal point off the centre), |q| != 1, glob_scale != 1 and a partial last
workgroup.  There the float32 C oracle's own error against float64 is orders of magnitude above the bars of
test_gpu_splat.py, and differs by orders of magnitude between classes of Gaussians, so HIP is compared with the float64
oracle PER CLASS and held to the project's rule (test_gpu_lbs.py / test_gpu_uvgeom.py):

    rel-L2(HIP, float64)  <=  2 x rel-L2(float32 oracle, float64)  +  4 eps32          over the same Gaussians.

A class is judged in every configuration where it holds at least project_cases.MIN_CLASS Gaussians.  Integer outputs and
zeros are exact.  The ratios go to project_parity.json in the report directory.

Where one draw of the oracle's error is not its level.  172 (class, output) figures are judged, and in the
ill-conditioned classes a figure is the cancellation noise of one or two Gaussians (det_orig = c00 c11 - c01^2 of a
projected needle; the `cancelling` class collects those that are neither clamped, near the clip plane nor huge).  Measured
on an MI355X, 3 figures came out above twice the float32 oracle's -- huge / comp 2.74 and huge / opac_eff 3.52 at
(glob_scale, clip) = (1.0, 0.1), near_clip / v_scale 2.59 at (0.37, 25) -- every other one under 2, the well-conditioned
classes between 0.1 and 1.1.  The oracle's own figure for huge / comp is 2.3e-5 on one host and 7.6e-5 on another whose
libm builds the scene one ulp apart; HIP's is 6.3e-5.  A figure that misses the factor 2 is therefore held, with the same
factor, to the oracle's EXPECTED error for that class and output (project_cases.ensemble_rms: the root mean square over 8
copies of the scene moved by at most one float32 rounding, float32 oracle against float64 oracle on each copy) -- a
conditioning figure made of oracle numbers only; against it the three read 0.80, 0.78 and 1.12.  Both ratios are printed
and recorded.  The one-line mutations of gol_project.h this file was written against (clamped point in the vjp's J,
lim_x / lim_y swapped, glob_scale dropped from v_scale, >= at the clip plane, conics only with a tile) miss the bar by
orders of magnitude or fail an exact check.

All callers of the shared arithmetic are reached: gol_project_fwd / gol_project_bwd (dense), gol_project_bwd_records
(record stride, cov3d recomputed) and the projection fused into the shading kernels (gol_shade_project_fwd / bwd)."""
import ctypes
import functools
import json
import math
import os

import pytest
import torch

import project_cases as pc
from scenes import look_at_viewmat, rel_l2

pytestmark = pytest.mark.gpu

_PARITY = {}


def _write_parity():
    """project_parity.json in the project's report directory (where bench.py leaves its detail report and conftest.py the
    parity ledger), when that directory exists."""
    import bench

    out_dir = os.path.dirname(bench.DETAIL_PATH)
    if os.path.isdir(out_dir):
        json.dump(_PARITY, open(os.path.join(out_dir, "project_parity.json"), "w"), indent=1)


def _dev(scene, B=None, n=None):
    """The scene's first B views and first n Gaussians as contiguous GPU tensors."""
    B, n = B or scene["B"], n or scene["N"]
    d = {k: scene[k][:B, :n].contiguous().cuda() for k in ("means", "scales", "quats", "opacity")}
    d["viewmats"] = scene["viewmats"][:B].reshape(B, 12).contiguous().cuda()
    d["intrins"] = scene["intrins"][:B].contiguous().cuda()
    d.update(B=B, N=n, H=scene["H"], W=scene["W"])
    return d


def _hip_fwd(d, glob_scale, clip):
    from goliath_amd import splat

    cov3d, xys, depths, radii, conics, comp, tiles, opac_eff = splat._project_fwd(
        d["B"], d["N"], d["means"], d["scales"], glob_scale, d["quats"], d["viewmats"], d["intrins"], d["H"], d["W"], clip,
        opacities=d["opacity"])
    return dict(xys=xys, depths=depths, radii=radii, conics=conics, comp=comp, tiles=tiles, cov3d=cov3d, opac_eff=opac_eff)


def _hip_bwd(d, glob_scale, fwd, up):
    """gol_project_bwd with dense upstream gradients and the saved cov3d; outputs start as NaN: every element must be
    written."""
    from goliath_amd import splat

    B, n = d["B"], d["N"]
    nan = lambda *s: torch.full((B, n, *s), float("nan"), device="cuda")
    g = dict(v_mean=nan(3), v_scale=nan(3), v_quat=nan(4), v_opacity=nan())
    splat._abi_project_bwd(B=B, N=n, means3d=d["means"], scales=d["scales"], glob_scale=glob_scale, quats=d["quats"],
                           viewmats=d["viewmats"], intrins=d["intrins"], cov3d=fwd["cov3d"], radii=fwd["radii"],
                           conics=fwd["conics"], compensation=fwd["comp"], v_xy=up["v_xy"], v_depth=up.get("v_depth"),
                           v_conic=up["v_conic"], v_compensation=up.get("v_comp"), opacities=d["opacity"],
                           v_opac_eff=up["v_opac_eff"], v_mean3d=g["v_mean"], v_scale=g["v_scale"], v_quat=g["v_quat"],
                           v_opacity=g["v_opacity"])
    return g


@functools.lru_cache(maxsize=None)
def _hip(cfg):
    """One B = 3 launch of the forward and of the backward per configuration, shared by the tests (read-only)."""
    r = pc.reference(cfg)
    d = _dev(r["scene"])
    up = {k: v[:d["B"], :d["N"]].contiguous().cuda() for k, v in r["up"].items()}
    fwd = _hip_fwd(d, r["glob_scale"], r["clip"])
    bwd = _hip_bwd(d, r["glob_scale"], fwd, up)
    torch.cuda.synchronize()
    return dict(d=d, up=up, fwd=fwd, bwd=bwd, fwd_cpu={k: v.cpu() for k, v in fwd.items()},
                bwd_cpu={k: v.cpu() for k, v in bwd.items()})


def _judge(tag, outputs, hip, o32, f64, classes, names, conditioning):
    """The rule of the module docstring for every (class, output); prints and records every figure, then asserts.
    conditioning() -> {(class, output): project_cases.ensemble_rms figure}, called only if a figure misses the factor 2."""
    rec, bad, cond = {}, [], None
    for cname in names:
        mask = classes[cname]
        n = int(mask.sum())
        if n < pc.MIN_CLASS:
            continue
        for o in outputs[cname] if isinstance(outputs, dict) else outputs:
            e_hip, e_32 = pc.class_rel_l2(hip[o], f64[o], mask), pc.class_rel_l2(o32[o], f64[o], mask)
            ratio = e_hip / (e_32 + 2.0 * pc.EPS32)      # the rule: ratio <= 2
            rec[f"{cname}/{o}"] = dict(n=n, hip=e_hip, oracle32=e_32, ratio=ratio)
            line = f"PROJECT_PARITY {tag} {cname:>12s} {o:>9s} n={n:5d} hip={e_hip:.2e} oracle32={e_32:.2e} ratio={ratio:.2f}"
            if not e_hip <= 2.0 * e_32 + 4.0 * pc.EPS32:
                cond = cond or conditioning()
                e_c = cond[(cname, o)]
                rec[f"{cname}/{o}"].update(oracle32_expected=e_c, ratio_expected=e_hip / (e_c + 2.0 * pc.EPS32))
                line += f"  -> expected oracle32={e_c:.2e} ratio={e_hip / (e_c + 2.0 * pc.EPS32):.2f}"
                if not e_hip <= 2.0 * e_c + 4.0 * pc.EPS32:
                    bad.append((cname, o, n, e_hip, e_32, e_c))
            print(line)
    _PARITY[tag] = rec
    _write_parity()
    assert rec and not bad, (tag, bad)


@pytest.mark.parametrize("cfg", [0, 1])
def test_forward_against_float64_per_class(cfg):
    """gol_project_fwd, B = 3 views in one launch.  The oracle writes cov3d as soon as a Gaussian is in front of the clip
    plane, and the conic before the tile-area test: a Gaussian in front without a tile has both, and nothing else."""
    r, h = pc.reference(cfg), _hip(cfg)["fwd_cpu"]
    cl = r["classes"]
    print()
    # integer outputs: exactly the oracles' (which agree with each other: test_project_edge_scene.py), nothing left out
    for name in ("radii", "tiles"):
        diff = h[name] != r["f32"][name]
        assert not bool(diff.any()), (name, int(diff.sum()), torch.nonzero(diff)[:8].tolist())
        assert torch.equal(h[name], r["f64"][name])
    # culled by the clip plane: every output exactly zero
    for name, v in h.items():
        assert not bool(v[cl["culled"]].any()), name
    # in front without a tile: conic and cov3d judged below, everything else exactly zero
    for name in ("xys", "depths", "radii", "comp", "tiles", "opac_eff"):
        assert not bool(h[name][cl["no_tile"]].any()), name
    outputs = {c: pc.FWD_OUTPUTS for c in pc.VISIBLE_CLASSES}
    outputs["no_tile"] = ("conics", "cov3d")
    _judge(f"fwd glob_scale={r['glob_scale']} clip={r['clip']}", outputs, h, r["f32"], r["f64"], cl, pc.CLASSES[1:],
           lambda: pc.conditioning(cfg))
    assert all(bool(torch.isfinite(v).all()) for v in h.values())


@pytest.mark.parametrize("cfg", [0, 1])
def test_backward_against_float64_per_class(cfg):
    """gol_project_bwd at the ABI (v_quat: the vjp to the normalised quaternion on every side), dense seeded upstream
    gradients of all five outputs, cov3d saved.  Each float32 side is fed its own float32 forward, float64 its own."""
    r, h = pc.reference(cfg), _hip(cfg)
    cl, g = r["classes"], h["bwd_cpu"]
    print()
    assert torch.equal(h["fwd_cpu"]["radii"], r["f64"]["radii"])      # the three sides skip the same Gaussians
    dead = r["f64"]["radii"] == 0
    assert int(dead.sum()) >= pc.MIN_CLASS
    for name, v in g.items():
        assert bool(torch.isfinite(v).all()), name
        assert not bool(v[dead].any()), name
    _judge(f"bwd glob_scale={r['glob_scale']} clip={r['clip']}", pc.BWD_OUTPUTS, g, r["b32"], r["b64"], cl,
           pc.VISIBLE_CLASSES, lambda: pc.conditioning(cfg))


def test_autograd_chained_through_the_quaternion_normalisation():
    """splat.project_gaussians on view 0 with the quaternions normalised by the caller (|q| between 0.2 and 3.2 before): the
    gradient that reaches the raw quaternion is the oracle's v_quat chained by hand through q / |q|, as in
    test_oracle_gsplat_fd.py; means and scales get the ABI's gradients."""
    from goliath_amd import splat

    r = pc.reference(0)
    scene, up, b = r["scene"], r["up"], 0
    fx, fy, cx, cy = (float(v) for v in scene["intrins"][b])
    m = scene["means"][b].cuda().requires_grad_(True)
    sc = scene["scales"][b].cuda().requires_grad_(True)
    q_raw = scene["quats"][b].cuda().requires_grad_(True)
    qn = q_raw / q_raw.norm(dim=-1, keepdim=True)
    out = splat.project_gaussians(m, sc, r["glob_scale"], qn, scene["viewmats"][b].cuda(), fx, fy, cx, cy, scene["H"],
                                  scene["W"], pc.BLOCK, r["clip"])
    xys, depths, radii, conics, comp = out[:5]
    g = {k: up[k][b].cuda() for k in ("v_xy", "v_depth", "v_conic", "v_comp")}
    ((xys * g["v_xy"]).sum() + (depths * g["v_depth"]).sum() + (conics * g["v_conic"]).sum()
     + (comp * g["v_comp"]).sum()).backward()
    # the oracles get the normalised quaternions the kernel got (float32 values), and their own forward outputs
    one = dict(means=scene["means"][b:b + 1], scales=scene["scales"][b:b + 1], quats=qn.detach().cpu()[None],
               opacity=scene["opacity"][b:b + 1], viewmats=scene["viewmats"][b:b + 1], intrins=scene["intrins"][b:b + 1],
               H=scene["H"], W=scene["W"], B=1, N=scene["N"])
    up1 = {k: v[b:b + 1] for k, v in up.items()}
    up1["v_opac_eff"] = torch.zeros_like(up1["v_opac_eff"])

    def chain(bw, fp64):
        raw = scene["quats"][b:b + 1].to(torch.float64 if fp64 else torch.float32)
        n = raw.norm(dim=-1, keepdim=True)
        qh = raw / n
        return dict(bw, v_quat=(bw["v_quat"] - qh * (qh * bw["v_quat"]).sum(-1, keepdim=True)) / n)

    sides = {}
    for fp64 in (False, True):
        f = pc.oracle_fwd(one, r["glob_scale"], r["clip"], fp64)
        sides[fp64] = (f, chain(pc.oracle_bwd(one, r["glob_scale"], f, up1, fp64), fp64))
    assert torch.equal(radii.cpu()[None], sides[True][0]["radii"])
    hip = dict(v_mean=m.grad.cpu()[None], v_scale=sc.grad.cpu()[None], v_quat=q_raw.grad.cpu()[None])
    classes = pc.classify(one, r["glob_scale"], r["clip"], sides[True][0])
    print()
    _judge("autograd view 0, normalisation chained", ("v_mean", "v_scale", "v_quat"), hip, sides[False][1], sides[True][1],
           classes, pc.VISIBLE_CLASSES, lambda: pc.ensemble_rms(one, r["glob_scale"], r["clip"], up1, classes, post=chain))


def test_constructed_rows_at_the_clip_plane_and_the_image_border():
    """Identity camera, clip = 0.25: z == clip is culled, the next float is kept; a scale of 500 and a centre left of the
    image get the oracle's radius and tile count."""
    c = pc.constructed_rows()
    f32 = pc.oracle_fwd(c, c["glob_scale"], c["clip"], False)
    f64 = pc.oracle_fwd(c, c["glob_scale"], c["clip"], True)
    h = {k: v.cpu() for k, v in _hip_fwd(_dev(c), c["glob_scale"], c["clip"]).items()}
    for name, v in h.items():
        assert not bool(v[0, 0].any()), name                             # z == clip exactly: culled, all zeros
    assert int(h["radii"][0, 1]) > 0 and int(h["tiles"][0, 1]) > 0        # nextafter(clip): kept
    assert float(h["depths"][0, 1]) == float(c["means"][0, 1, 2])
    assert torch.equal(h["radii"], f32["radii"]) and torch.equal(h["tiles"], f32["tiles"])
    assert int(h["tiles"][0, 2]) == 60 and float(h["xys"][0, 3, 0]) < 0.0 < int(h["tiles"][0, 3])
    kept = f64["radii"] > 0
    for name in pc.FWD_OUTPUTS:
        e_hip, e_32 = pc.class_rel_l2(h[name], f64[name], kept), pc.class_rel_l2(f32[name], f64[name], kept)
        assert e_hip <= 2.0 * e_32 + 4.0 * pc.EPS32, (name, e_hip, e_32)


@pytest.mark.parametrize("with_depth", [True, False])
def test_gradient_records_give_the_dense_backward_bit_for_bit(with_depth):
    """gol_project_bwd_records reads its upstream gradients out of [B, N, GRAD_RECORD] records (rgb 0-2, v_opac_eff 3, v_xy
    4-5, v_conic 6-8, v_depth 9) and recomputes cov3d with the forward's arithmetic: the same bits as gol_project_bwd fed
    the same values densely with the saved cov3d.  The colour gradient is the record's rgb."""
    from goliath_amd import _lib, splat

    cfg = 1
    r, h = pc.reference(cfg), _hip(cfg)
    d, fwd = h["d"], h["fwd"]
    B, n = d["B"], d["N"]
    gen = torch.Generator().manual_seed(77)
    rec = torch.randn(B, n, splat.GRAD_RECORD, generator=gen).cuda()     # the unused floats 10-15 are noise, too
    nan = lambda *s: torch.full((B, n, *s), float("nan"), device="cuda")
    got = dict(v_mean=nan(3), v_scale=nan(3), v_quat=nan(4), v_opacity=nan())
    v_colors = nan(3)
    fp, c_int, c_float = _lib.fptr, ctypes.c_int, ctypes.c_float
    _lib.call("gol_project_bwd_records", c_int(B), c_int(n), fp(d["means"]), fp(d["scales"]), c_float(r["glob_scale"]),
              fp(d["quats"]), fp(d["viewmats"]), fp(d["intrins"]), _lib.iptr(fwd["radii"]), fp(fwd["conics"]),
              fp(fwd["comp"]), fp(d["opacity"]), fp(rec), c_int(1 if with_depth else 0), fp(got["v_mean"]),
              fp(got["v_scale"]), fp(got["v_quat"]), fp(got["v_opacity"]), fp(v_colors), _lib.stream_ptr())
    up = dict(v_opac_eff=rec[..., 3].contiguous(), v_xy=rec[..., 4:6].contiguous(), v_conic=rec[..., 6:9].contiguous())
    if with_depth:
        up["v_depth"] = rec[..., 9].contiguous()
    want = _hip_bwd(d, r["glob_scale"], fwd, up)
    for name in pc.BWD_OUTPUTS:
        assert bool(torch.isfinite(got[name]).all()), name
        assert torch.equal(got[name], want[name]), (name, rel_l2(got[name], want[name]))
    assert torch.equal(v_colors, rec[..., :3])
    if with_depth:      # ... and float 9 of the record really is read
        no_depth = _hip_bwd(d, r["glob_scale"], fwd, {k: v for k, v in up.items() if k != "v_depth"})
        assert not torch.equal(no_depth["v_mean"], got["v_mean"])
    live = fwd["radii"] > 0
    assert float(got["v_mean"][live].abs().sum()) > 0 and not bool(got["v_mean"][~live].any())


@pytest.mark.parametrize("n", [1, 255, 257])
def test_small_launches_equal_the_rows_of_the_large_one(n):
    """B = 2 and N below, at and above one workgroup: every row bitwise equal to the same row of the N = 4133, B = 3
    launch, forward and backward."""
    cfg = 0
    r, big = pc.reference(cfg), _hip(cfg)
    d = _dev(r["scene"], B=2, n=n)
    fwd = _hip_fwd(d, r["glob_scale"], r["clip"])
    up = {k: v[:2, :n].contiguous() for k, v in big["up"].items()}
    bwd = _hip_bwd(d, r["glob_scale"], fwd, up)
    for name, v in fwd.items():
        assert torch.equal(v, big["fwd"][name][:2, :n]), name
    for name, v in bwd.items():
        assert torch.equal(v, big["bwd"][name][:2, :n]), name


# ------------------------------------------------------------------------------------------ the fused path (shade.hip)
FUSED_B, FUSED_S, FUSED_H, FUSED_W = 3, 64, 272, 224     # a shape of its own: the capacity plan starts from this scene


def _close_off_centre_cameras(t, H, W):
    """K / Rt / campos of bench.make_inputs replaced in place: two cameras INSIDE the head (Gaussians behind them, at the
    clip plane and far past the 1.3 tan(fov) clamp) and one just outside it, none looking at the origin, fx != fy, the
    principal point off the centre."""
    eyes = [(25.0, 10.0, -55.0), (-40.0, -30.0, 35.0), (60.0, 20.0, -125.0)]
    targets = [(-20.0, 15.0, 30.0), (30.0, 20.0, -10.0), (-15.0, -25.0, 0.0)]
    focal = 3000.0 * W / 1334.0
    with torch.no_grad():
        for b, (eye, target) in enumerate(zip(eyes, targets)):
            t["Rt"][b].copy_(look_at_viewmat(eye, target))
            t["campos"][b].copy_(torch.tensor(eye))
            t["K"][b, 0, 0], t["K"][b, 1, 1] = focal * (0.4 + 0.3 * b), focal * (0.45 + 0.2 * b)
            t["K"][b, 0, 2], t["K"][b, 1, 2] = W / 2.0 + 13.7 - 9.0 * b, H / 2.0 - 9.3 + 6.0 * b


@pytest.mark.parametrize("env,extra,rand", [(True, False, False), (True, True, True), (False, True, False)])
def test_fused_projection_equals_the_separate_kernels_at_the_frustum_edges(env, extra, rand):
    """test_gpu_fused_projection.py's comparison with cameras inside the head: every field the shading kernel projected
    and its records equal gol_project_fwd on the attributes it returned, bit for bit; images equal; leaf gradients (through
    gol_shade_project_bwd against gol_project_bwd_records + gol_shade_bwd) to accumulation-order noise."""
    from goliath_amd import splat
    from test_gpu_fused_projection import LEAVES, _inputs, _run

    B, S, H, W = FUSED_B, FUSED_S, FUSED_H, FUSED_W
    N = S * S
    t = _inputs(B, S, H, W, env)
    _close_off_centre_cameras(t, H, W)
    p0, rgb0, a0, d0, l0, g0 = _run(t, H, W, env, False, extra, rand)
    p1, rgb1, a1, d1, l1, g1 = _run(t, H, W, env, True, extra, rand)
    intr = torch.stack([t["K"][:, 0, 0], t["K"][:, 1, 1], t["K"][:, 0, 2], t["K"][:, 1, 2]], -1).contiguous()
    with torch.no_grad():
        ref = splat._project_fwd(B, N, p0["primpos"].contiguous(), p0["primscale"].contiguous(), 1.0,
                                 p0["primqvec"].contiguous(), t["Rt"].reshape(B, 12).contiguous(), intr, H, W, 0.1,
                                 p0["opacity"].reshape(B, N).contiguous(), p0["color"].contiguous())
    cov3d, xys, depths, radii, conics, comp, nth, opac_eff, records = ref
    # the scene is at the edges: counted from the attributes the shading kernel returned
    cam = torch.einsum("brc,bnc->bnr", t["Rt"][:, :, :3].double(), p0["primpos"].detach().double()) + t["Rt"][:, None, :, 3].double()
    tz = cam[..., 2]
    lim_x = (pc.FOV_CLAMP * 0.5 * W / t["K"][:, 0, 0].double())[:, None]
    lim_y = (pc.FOV_CLAMP * 0.5 * H / t["K"][:, 1, 1].double())[:, None]
    clamped = ((cam[..., 0] / tz).abs() > lim_x) | ((cam[..., 1] / tz).abs() > lim_y)
    counts = dict(behind=int((tz <= 0.1).sum()), near_clip=int(((tz > 0.1) & (tz < 1.3)).sum()),
                  clamped_visible=int((clamped & (radii > 0)).sum()), visible=int((radii > 0).sum()),
                  no_tile=int(((tz > 0.1) & (radii == 0)).sum()))
    print("\nFUSED_EDGE_COUNTS", counts)
    assert counts["behind"] >= 300 and counts["near_clip"] >= 10 and counts["clamped_visible"] >= 15
    assert counts["visible"] >= 1500 and counts["no_tile"] >= 100
    assert not bool(radii[tz <= 0.1 - 1e-3].any())
    pr = p1["projected"]
    assert torch.equal(pr.field("radii"), radii)
    for name, want in (("xys", xys), ("depths", depths), ("conics", conics), ("comp", comp), ("opac_eff", opac_eff)):
        assert torch.equal(pr.field(name), want), name
    assert torch.equal(pr.records, records)
    assert torch.equal(rgb0, rgb1) and torch.equal(a0, a1) and torch.equal(d0, d1) and l0 == l1
    assert bool(torch.isfinite(rgb1).all()) and math.isfinite(l1)
    for k in LEAVES:
        assert bool(torch.isfinite(g1[k]).all()), k
        assert rel_l2(g1[k], g0[k]) < 2e-6, k
