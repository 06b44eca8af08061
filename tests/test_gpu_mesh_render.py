"""GPU: the fused textured mesh render (meshraster.render_textured / FusedRenderLayer, csrc/meshrender.hip).

Yardstick: RenderLayer's own PyTorch composition (meshraster.render -> interpolate -> grid_sample * mask ->
edge_grad_estimator), run in float64 on the CPU on the SAME index_img the HIP rasterizer produced: the discrete visibility
is identical and only arithmetic differs.  drtk is absent, so parity with drtk stays unpinned, as for RenderLayer.
Bars are about 10x the measured values; the measured values are quoted next to each bar."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from scenes import icosphere, rel_l2

pytestmark = pytest.mark.gpu


def _camera(B, H, W, focal, dist):
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = focal
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W / 2.0, H / 2.0, 1.0
    Rt = torch.zeros(B, 3, 4)
    for b in range(B):   # a small turn per view about y, camera on the -z side looking +z
        a = 0.3 * b
        Rt[b, :, :3] = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
        Rt[b, 2, 3] = dist
    return K, Rt


def _bumpy(subdiv, B, seed, radius=1.0, shift=(0.0, 0.0, 0.0)):
    v, f = icosphere(subdiv, radius)
    g = torch.Generator().manual_seed(seed)
    v = v[None].repeat(B, 1, 1) * (1.0 + 0.12 * torch.rand(B, v.shape[0], 1, generator=g)) + torch.tensor(shift)
    return v, f


def _two_spheres(B, subdiv=2, behind_face=False):
    """Two overlapping bumpy spheres (silhouettes, occlusion boundaries, shared edges), optionally one more face with a
    vertex behind the camera (the rasterizer skips it; nothing may break)."""
    v0, f0 = _bumpy(subdiv, B, 1, 1.0, (-0.35, 0.1, 0.0))
    v1, f1 = _bumpy(subdiv, B, 2, 0.7, (0.55, -0.15, -0.6))
    verts, faces = torch.cat([v0, v1], 1), torch.cat([f0, f1 + v0.shape[1]])
    if behind_face:
        extra = torch.tensor([[0.2, 0.2, -1.5], [0.5, -0.3, -1.2], [0.1, 0.1, -4.0]])[None].repeat(B, 1, 1)
        faces = torch.cat([faces, torch.tensor([[0, 1, 2]]) + verts.shape[1]])
        verts = torch.cat([verts, extra], 1)
    return verts, faces


def _uv(V, seed, lo=-0.2, hi=1.2):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(V, 2, generator=g)


def _ups(B, C, H, W, which, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = {"render": (B, C, H, W), "vt_img": (B, 2, H, W), "depth_img": (B, H, W), "bary_img": (B, 3, H, W)}
    return {k: torch.randn(*shapes[k], generator=g).cuda() for k in (["render"] if which == "render" else shapes)}


def _reference(layer, verts, tex, K, Rt, index_img, edge_grad, ups):
    """RenderLayer's composition in float64 on the CPU on the given index image: outputs and leaf gradients."""
    from goliath_amd import meshraster

    leaf = {k: t.detach().double().cpu().requires_grad_(True) for k, t in
            (("verts", verts), ("tex", tex), ("K", K), ("Rt", Rt))}
    vi, vti = layer.vi.cpu(), layer.vti.cpu()
    B = verts.shape[0]
    v_pix = meshraster.transform(leaf["verts"], leaf["K"], leaf["Rt"])
    idx = index_img.cpu()
    depth, bary = meshraster.render(v_pix, vi, idx)
    vt_img = meshraster.interpolate((layer.vt.cpu().double() * 2.0 - 1.0)[None].expand(B, -1, -1), vti, idx, bary)
    mask = (idx != -1)[:, None].double()
    img = F.grid_sample(leaf["tex"], vt_img.permute(0, 2, 3, 1), mode="bilinear", align_corners=False) * mask
    if edge_grad:
        img = meshraster.edge_grad_estimator(v_pix, vi, bary, img, idx, depth)
    out = {"render": img, "vt_img": vt_img, "depth_img": depth, "bary_img": bary}
    sum((out[k] * u.double().cpu()).sum() for k, u in ups.items()).backward()
    return {k: t.detach() for k, t in out.items()}, {k: t.grad for k, t in leaf.items()}


def _kink_free(layer, verts, tex, K, Rt, index_img, ups):
    """Zero the upstream gradients (in both runs) at the pixels whose float64 texture sample lies within rounding of a
    texel boundary, flagged a priori on the reference data: the bilinear derivative jumps there, and fp32 and fp64 may
    pick different texel cells (fp32 uv carry ~1e-5 of error, i.e. Wt * 5e-6 texels).  Returns (ups, flagged fraction)."""
    from goliath_amd import meshraster

    with torch.no_grad():
        B = verts.shape[0]
        v_pix = meshraster.transform(verts.double().cpu(), K.double().cpu(), Rt.double().cpu())
        idx = index_img.cpu()
        bary = meshraster.render(v_pix, layer.vi.cpu(), idx)[1]
        vt_img = meshraster.interpolate((layer.vt.cpu().double() * 2.0 - 1.0)[None].expand(B, -1, -1), layer.vti.cpu(),
                                        idx, bary)
        Ht, Wt = tex.shape[-2:]
        ix, iy = ((vt_img[:, 0] + 1) * Wt - 1) / 2, ((vt_img[:, 1] + 1) * Ht - 1) / 2
        tol = max(1e-3, 2e-5 * max(Ht, Wt))
        flag = (((ix - ix.round()).abs() < tol) | ((iy - iy.round()).abs() < tol)) & (idx >= 0)
        keep = (~flag).float().cuda()
    return {k: u * (keep if u.dim() == 3 else keep[:, None]) for k, u in ups.items()}, float(flag.float().mean())


def _judge(tag, out, got, ref_out, want, plain_got, bars):
    """Outputs and leaf gradients against the float64 composition.  Written yardstick for the gradients: the fp32 GPU
    RenderLayer's own distance to the same float64 run (plain_got) -- the vertex and camera gradients sum many pixel terms
    of both signs, and fp32 pixel coordinates of ~1e3 leave ~1e-4 (small scene) to ~1e-3 (2048 x 1334) of that sum to
    rounding in either implementation.  The fused layer may not be more than 1.5x (+1e-6) as far; `bars` are ~10x the
    measured values."""
    errs = {k: rel_l2(out[k].detach().cpu().double(), ref_out[k]) for k in ref_out}
    errs.update({"grad_" + k: rel_l2(got[k].cpu().double(), want[k]) for k in want})
    plain = {"grad_" + k: rel_l2(plain_got[k].cpu().double(), want[k]) for k in want}
    print("MEASURED", tag, {k: "%.2e" % v for k, v in errs.items()}, "fp32 RenderLayer:",
          {k: "%.2e" % v for k, v in plain.items()})
    for k, v in errs.items():
        assert v < bars[k], (k, v, bars[k])
        if k in plain:
            assert v <= 1.5 * plain[k] + 1e-6, (k, v, plain[k])


def _fused(layer, verts, tex, K, Rt, edge_grad, ups):
    leaf = {k: t.detach().cuda().requires_grad_(True) for k, t in (("verts", verts), ("tex", tex), ("K", K), ("Rt", Rt))}
    out = layer(leaf["verts"], leaf["tex"], leaf["K"], leaf["Rt"], edge_grad=edge_grad)
    sum((out[k] * u).sum() for k, u in ups.items()).backward()
    return out, {k: t.grad for k, t in leaf.items()}


@pytest.mark.parametrize("C", [1, 3, 4, 7, 16])
def test_forward_matches_render_layer(C):
    from goliath_amd import meshraster

    B, H, W = 2, 70, 90
    verts, faces = _two_spheres(B, 2, behind_face=True)
    vt = _uv(verts.shape[1], C)
    K, Rt = _camera(B, H, W, 0.8 * W, 4.0)
    tex = torch.rand(B, C, 24, 40, generator=torch.Generator().manual_seed(C)).cuda()
    ref = meshraster.RenderLayer(H, W, faces, vt, faces, flip_uvs=True).cuda()
    fused = meshraster.FusedRenderLayer(H, W, faces, vt, faces, flip_uvs=True).cuda()
    vg = verts.cuda().requires_grad_(True)   # RenderLayer then re-derives depth / barycentrics differentiably
    a = ref(vg, tex, K.cuda(), Rt.cuda())
    b = fused(vg, tex, K.cuda(), Rt.cuda())
    assert set(a) == set(b)
    assert torch.equal(a["index_img"], b["index_img"]) and torch.equal(a["mask"], b["mask"])
    covered = float(a["mask"].mean())
    assert 0.2 < covered < 0.95, covered
    # some samples read outside the texture (zero padding) and the face behind the camera is in the mesh
    assert float((b["vt_img"].abs() > 1.0).float().mean()) > 0.01
    errs = {k: rel_l2(b[k].detach(), a[k].detach()) for k in ("render", "vt_img", "depth_img", "bary_img")}
    print("MEASURED forward C=%d" % C, {k: "%.2e" % v for k, v in errs.items()})
    # measured (every C): render 1.2-1.4e-6, vt_img 1.2-1.4e-7, depth 5.6e-8, bary 1.2e-7
    bars = dict(render=1.5e-5, vt_img=1.5e-6, depth_img=6e-7, bary_img=1.5e-6)
    for k, v in errs.items():
        assert v < bars[k], (k, v)
    assert float((b["render"] * (1 - b["mask"])).detach().abs().max()) == 0.0


@pytest.mark.parametrize("edge_grad", [False, True])
@pytest.mark.parametrize("which", ["render", "all"])
def test_gradients_match_the_float64_composition(edge_grad, which):
    from goliath_amd import meshraster

    B, H, W, C = 2, 96, 120, 3
    verts, faces = _two_spheres(B, 2)
    vt = _uv(verts.shape[1], 5, 0.0, 1.0)
    K, Rt = _camera(B, H, W, 0.8 * W, 4.0)
    tex = torch.rand(B, C, 32, 48, generator=torch.Generator().manual_seed(3))
    layer = meshraster.FusedRenderLayer(H, W, faces, vt, faces).cuda()
    index_img = meshraster.rasterize(meshraster.transform(verts.cuda(), K.cuda(), Rt.cuda()), faces.cuda(), H, W)[0]
    ups, flagged = _kink_free(layer, verts, tex, K, Rt, index_img, _ups(B, C, H, W, which, 11))
    out, got = _fused(layer, verts, tex, K, Rt, edge_grad, ups)
    assert torch.equal(out["index_img"], index_img)
    ref_out, want = _reference(layer, verts, tex, K, Rt, out["index_img"], edge_grad, ups)
    plain = meshraster.RenderLayer(H, W, faces, vt, faces).cuda()
    plain_got = _fused(plain, verts, tex, K, Rt, edge_grad, ups)[1]
    assert flagged < 0.02   # measured 0.0014
    # measured: render 9.3e-6, vt_img 1.1e-6, depth 7.0e-8, bary 1.1e-6; gradients verts 1.2e-4, tex 2.7e-5, K 1.8e-4,
    # Rt 1.4e-4 (every case; the edge term changes none of them beyond the third digit)
    _judge("gradients edge_grad=%s which=%s flagged %.4f" % (edge_grad, which, flagged), out, got, ref_out, want,
           plain_got, dict(render=1e-4, vt_img=1.5e-5, depth_img=1e-6, bary_img=1.5e-5, grad_verts=1.5e-3,
                           grad_tex=3e-4, grad_K=2e-3, grad_Rt=1.5e-3))


def test_urhand_size():
    """2048x1334, C = 4, 1024^2 texture, the hand stand-in of bench.py (icosphere(4), ~90 mm), B = 2, edge_grad=True."""
    from goliath_amd import meshraster

    B, H, W, C = 2, 1334, 2048, 4
    v, faces = icosphere(4, radius=90.0)
    v = v * (1.0 + 0.08 * torch.sin(0.05 * v[:, :1] + 0.07 * v[:, 1:2]))
    verts = v[None].repeat(B, 1, 1)
    # a uv atlas like a hand's (about a texel per pixel: planar projection of the surface) and a smooth texture
    vt = 0.5 + 0.45 * v[:, :2] / v[:, :2].abs().max()
    K, Rt = _camera(B, H, W, 2000.0, 400.0)
    tex = torch.cat([_smooth_field(1024, 1024, C, 4 + b).float() for b in range(B)])
    layer = meshraster.FusedRenderLayer(H, W, faces, vt, faces).cuda()
    index_img = meshraster.rasterize(meshraster.transform(verts.cuda(), K.cuda(), Rt.cuda()), faces.cuda(), H, W)[0]
    ups, flagged = _kink_free(layer, verts, tex, K, Rt, index_img, _ups(B, C, H, W, "all", 12))
    out, got = _fused(layer, verts, tex, K, Rt, True, ups)
    ref = meshraster.RenderLayer(H, W, faces, vt, faces).cuda()
    a = ref(verts.cuda().requires_grad_(True), tex.cuda(), K.cuda(), Rt.cuda())
    assert torch.equal(a["index_img"], out["index_img"]) and torch.equal(a["mask"], out["mask"])
    ref_out, want = _reference(layer, verts, tex, K, Rt, out["index_img"], True, ups)
    plain_got = _fused(ref, verts, tex, K, Rt, True, ups)[1]
    assert flagged < 0.05   # measured 0.020
    # measured: render 5.5e-6, vt_img 1.4e-7, depth 8.1e-8, bary 6.3e-6; gradients verts 9.7e-4, tex 8.1e-5, K 5.6e-4,
    # Rt 5.3e-4
    _judge("urhand size covered %.3f flagged %.4f" % (float(out["mask"].mean()), flagged), out, got, ref_out, want,
           plain_got, dict(render=6e-5, vt_img=2e-6, depth_img=1e-6, bary_img=6e-5, grad_verts=1e-2, grad_tex=8e-4,
                           grad_K=6e-3, grad_Rt=6e-3))


# the scene of tests/test_mesh_edge_grad.py (a far face and a nearer one overlapping its right part), flat colours
EH, EW = 40, 48


def _edge_scene():
    v = torch.tensor([[[6.3, 5.2, 5.0], [41.7, 9.4, 5.0], [17.9, 35.6, 5.0],
                       [24.4, 12.3, 3.0], [44.2, 20.8, 3.0], [27.6, 33.1, 3.0]]], dtype=torch.float64)
    vi = torch.tensor([[0, 1, 2], [3, 4, 5]])
    return v, vi


def _smooth_field(h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64) + 0.5, torch.arange(w, dtype=torch.float64) + 0.5, indexing="ij")
    out = torch.zeros(1, c, h, w, dtype=torch.float64)
    for k in range(c):
        for _ in range(3):
            fx, fy, ph = (torch.rand(3, generator=g, dtype=torch.float64) * torch.tensor([0.25, 0.25, 6.28])).tolist()
            out[0, k] += torch.cos(fx * xx + fy * yy + ph)
    return out


def _aa_functional(v, vi, colors, g, S=16):
    """<g, box-filtered S x supersampled flat-colour render> (numpy z-buffer of the same conventions)."""
    from oracle import mesh_ref

    vs = v.clone()
    vs[..., :2] *= S
    idx, _, _ = mesh_ref.rasterize(vs.numpy(), vi.numpy(), EH * S, EW * S)
    idx = torch.from_numpy(idx)
    img = torch.zeros(1, 3, EH * S, EW * S, dtype=torch.float64)
    for f, c in enumerate(colors):
        img += (idx == f)[:, None].double() * torch.tensor(c, dtype=torch.float64)[None, :, None, None]
    return float((F.avg_pool2d(img, S) * g).sum())


@pytest.mark.parametrize("move", ["translate_far_face", "translate_near_face", "one_vertex_of_the_near_face"])
def test_edge_term_matches_the_supersampled_render(move):
    """The HIP edge term of a flat-coloured two-face scene (each face's uv at the centre of its own texel) against the
    finite-difference derivative of the 16x supersampled render, within 15 % (the bar of tests/test_mesh_edge_grad.py)."""
    from goliath_amd import meshraster

    v, vi = _edge_scene()
    colors = [(0.9, 0.3, 0.1), (0.1, 0.5, 0.8)]
    g = _smooth_field(EH, EW, 3, 7)
    dv = torch.zeros_like(v)
    if move == "translate_far_face":
        dv[0, 0:3, 0], dv[0, 0:3, 1] = 0.8, 0.6
    elif move == "translate_near_face":
        dv[0, 3:6, 0], dv[0, 3:6, 1] = -0.6, 0.8
    else:
        dv[0, 4, 0], dv[0, 4, 1] = 0.7, -0.7
    eps = 0.25
    fd = (_aa_functional(v + eps * dv, vi, colors, g) - _aa_functional(v - eps * dv, vi, colors, g)) / (2 * eps)
    tex = torch.tensor(colors, dtype=torch.float32).t().reshape(1, 3, 1, 2).cuda()    # texel f = colour of face f
    vt = torch.tensor([[0.25, 0.5], [0.75, 0.5]]).cuda()
    vti = torch.tensor([[0, 0, 0], [1, 1, 1]]).cuda()
    leaf = v.float().cuda().requires_grad_(True)
    idx, depth, bary = meshraster.rasterize(leaf, vi.cuda(), EH, EW)
    img = meshraster.render_textured(leaf, vi.cuda(), vt, vti, tex, idx, depth, bary, edge_grad=True)[0]
    (img * g.float().cuda()).sum().backward()
    est = float((leaf.grad.cpu().double() * dv).sum())
    print("MEASURED supersampled %s est %.4f fd %.4f" % (move, est, fd))
    assert abs(fd) > 1.0, fd
    assert abs(est - fd) < 0.15 * abs(fd), (move, est, fd)


def test_captured_step_replays_the_eager_step():
    """Forward + backward of FusedRenderLayer captured once as a graph (no host sync inside): one replay equals the eager
    step on the same buffers."""
    from goliath_amd import graphs, meshraster

    B, H, W, C = 2, 64, 80, 4
    verts, faces = _two_spheres(B, 1)
    K, Rt = _camera(B, H, W, 0.8 * W, 4.0)
    layer = meshraster.FusedRenderLayer(H, W, faces, _uv(verts.shape[1], 9, 0.0, 1.0), faces).cuda()
    vg = verts.cuda().requires_grad_(True)
    tg = torch.rand(B, C, 32, 32, device="cuda").requires_grad_(True)
    Kg, Rtg = K.cuda(), Rt.cuda()
    up = torch.randn(B, C, H, W, device="cuda")

    def step():
        vg.grad, tg.grad = None, None
        out = layer(vg, tg, Kg, Rtg, edge_grad=True)
        (out["render"] * up).sum().backward()
        return out["render"], vg.grad, tg.grad

    cap = graphs.CapturedStep(step)
    img_g, gv_g, gt_g = (t.clone() for t in cap.replay())
    img_e, gv_e, gt_e = step()
    assert torch.equal(img_g, img_e)
    assert rel_l2(gv_g, gv_e) < 1e-5 and rel_l2(gt_g, gt_e) < 1e-5
    assert float(gv_e.abs().sum()) > 0 and float(gt_e.abs().sum()) > 0


def test_edge_stats_count_like_the_pytorch_estimator():
    """EDGE_STATS keeps its meaning (pairs kept, pairs without a crossing occluder edge), on the device."""
    from goliath_amd import meshraster

    B, H, W, C = 1, 64, 80, 3
    verts, faces = _two_spheres(B, 1)
    K, Rt = _camera(B, H, W, 0.8 * W, 4.0)
    vt = _uv(verts.shape[1], 9, 0.0, 1.0)
    tex = torch.rand(B, C, 16, 16, device="cuda")
    up = torch.randn(B, C, H, W, device="cuda")
    counts = {}
    old = meshraster.COLLECT_EDGE_STATS
    try:
        meshraster.COLLECT_EDGE_STATS = True
        for cls in (meshraster.RenderLayer, meshraster.FusedRenderLayer):
            meshraster.EDGE_STATS.clear()
            vg = verts.cuda().requires_grad_(True)
            (cls(H, W, faces, vt, faces).cuda()(vg, tex, K.cuda(), Rt.cuda())["render"] * up).sum().backward()
            st = meshraster.EDGE_STATS[vg.device]
            assert st["edges"].is_cuda
            counts[cls.__name__] = (int(st["edges"]), int(st["dropped"]))
    finally:
        meshraster.COLLECT_EDGE_STATS = old
        meshraster.EDGE_STATS.clear()
    print("MEASURED edge stats", counts)
    (e0, d0), (e1, d1) = counts["RenderLayer"], counts["FusedRenderLayer"]
    assert e0 > 100 and abs(e1 - e0) <= 2 and abs(d1 - d0) <= 2
