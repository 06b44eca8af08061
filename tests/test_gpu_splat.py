"""GPU parity: HIP projection / binning / rasterizer (through the C ABI) vs the CPU oracle of the
gsplat-0.1.11 path (PARITY UNPINNED upstream, see oracle/gsplat_oracle.c).

Bars: integer/index outputs (radii, tile counts, sorted ids) exact up to ulp-flips of ceil()/(int);
floating point rel-L2 <= 1e-4 (north_star), gradients included.
"""
import os

import pytest
import torch

from scenes import head_scene, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4      # north_star bar; the per-assertion bars below are ~10x what profiles/r04_parity_ledger.json measured
TIGHT = 5e-6    # small scenes, identical inputs: measured 3e-8 ... 4e-7


def _cuda(s):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in s.items()}


def _project_both(s, clip=0.1):
    from goliath_amd import splat
    from oracle import cref

    g = _cuda(s)
    hip = splat.project_gaussians(g["means"], g["scales"], 1.0, g["quats"], g["viewmat"], s["fx"], s["fy"],
                                  s["cx"], s["cy"], s["H"], s["W"], 16, clip)
    ref = cref.project_gaussians(s["means"], s["scales"], 1.0, s["quats"], s["viewmat"], s["fx"], s["fy"],
                                 s["cx"], s["cy"], s["H"], s["W"], 16, clip)
    return g, hip, ref


def test_project_forward_config1():
    s = head_scene(10_000, 512, 512, seed=0)
    _, hip, ref = _project_both(s)
    names = ["xys", "depths", "radii", "conics", "comp", "tiles", "cov3d"]
    assert int(ref[5].sum()) > 10_000
    for n, a, b in zip(names, hip, ref):
        if b.dtype == torch.int32:
            assert (a.cpu() != b).float().mean() < 1e-3, n
        else:
            assert rel_l2(a, b) < 1e-5, (n, rel_l2(a, b))


def test_project_culling_edge_cases():
    # behind the camera, at the clip plane, far off-screen, huge and tiny scales
    s = head_scene(64, 128, 128, seed=1)
    s["means"][0] = torch.tensor([0.0, 0.0, -5000.0])  # behind the ring camera
    s["means"][1] = torch.tensor([1e5, 0.0, 0.0])  # far off-screen
    s["scales"][2] = 1e-6
    s["scales"][3] = 500.0
    _, hip, ref = _project_both(s)
    assert torch.equal(hip[2].cpu() > 0, ref[2] > 0)
    assert rel_l2(hip[0], ref[0]) < 1e-5
    assert int(hip[2][0]) == 0 and int(hip[5][0]) == 0


def _lists(hip_proj, s):
    """Sorted lists from the oracle, fed with the HIP projection so both sides bin the same numbers."""
    from oracle import cref

    xys, depths, radii, conics, comp, nth, _ = (t.detach().cpu() for t in hip_proj)
    keys, ids, bins = cref.bin_and_sort(xys, depths, radii, nth, s["H"], s["W"], 16)
    return (xys, depths, radii, conics, comp, nth), ids, bins


def test_bin_sort_matches_oracle_exactly():
    import ctypes

    from goliath_amd import _lib, splat

    s = head_scene(10_000, 512, 512, seed=0)
    g, hip, _ = _project_both(s)
    (xys, depths, radii, conics, comp, nth), ids, bins = _lists(hip, s)
    I = ids.numel()
    T = splat._tiles(s["H"], s["W"])
    ws = splat._Workspace(1, xys.shape[0], T, I, "cuda")
    splat._bin_sort(1, xys.shape[0], hip[0].contiguous(), hip[1].contiguous(), hip[2].contiguous(), s["H"],
                    s["W"], ws)
    assert int(ws.n_isect[0]) == I
    assert torch.equal(ws.tile_bins[0].cpu(), bins) or torch.equal(
        (ws.tile_bins[0, :, 1] - ws.tile_bins[0, :, 0]).cpu(), bins[:, 1] - bins[:, 0])
    assert torch.equal(ws.sorted_ids[0, :I].cpu(), ids)
    # capacity overflow: the count is still exact, the bins stay inside the buffer
    ws2 = splat._Workspace(1, xys.shape[0], T, I // 3, "cuda")
    splat._bin_sort(1, xys.shape[0], hip[0].contiguous(), hip[1].contiguous(), hip[2].contiguous(), s["H"],
                    s["W"], ws2)
    assert int(ws2.n_isect[0]) == I
    assert int(ws2.tile_bins.max()) <= I // 3
    # pruned lists (conics + opacity given): every tile list is a subsequence of gsplat's list and
    # contains every Gaussian that can reach alpha >= 1/255 somewhere in the tile
    opac = (s["opacity"][:, 0] * comp).cuda().contiguous()
    ws3 = splat._Workspace(1, xys.shape[0], T, I, "cuda")
    splat._bin_sort(1, xys.shape[0], hip[0].contiguous(), hip[1].contiguous(), hip[2].contiguous(), s["H"],
                    s["W"], ws3, hip[3].contiguous(), opac)
    I3 = int(ws3.n_isect[0])
    assert 0 < I3 < I
    b3, ids3 = ws3.tile_bins[0].cpu(), ws3.sorted_ids[0].cpu()
    from binning_cases import prune_reference

    live = prune_reference(xys, radii, conics, opac.cpu(), s["H"], s["W"], (ids, bins))   # float64, per pair of `ids`
    assert 0 < int(live.sum()) < I
    for t in range(T):
        full = ids[bins[t, 0]:bins[t, 1]].tolist()
        sub = ids3[b3[t, 0]:b3[t, 1]].tolist()
        it = iter(full)
        assert all(g in it for g in sub), t  # order-preserving subsequence
        must = {g for g, v in zip(full, live[bins[t, 0]:bins[t, 1]]) if v}
        assert must <= set(sub), t           # ... that keeps every Gaussian some pixel centre of the tile can see


@pytest.mark.parametrize("N", [2, 63, 200, 256, 257, 500, 513, 1000, 1024, 1025, 2000, 2048, 2049, 3500, 4096, 4097, 6000,
                               12000, 16384, 16385, 20000])
def test_bin_sort_one_tile_every_size_class(N):
    """All Gaussians on one tile: every size class of the per-tile sort (1/2/4/8 keys per thread in registers, the bucket
    sorts of the tile kernel (<= 2048) and of the long-list kernel (<= 16384 keys in LDS, round 4), the global-memory
    network beyond, and -- through the 100 equal depths -- the decline-and-fall-back path), incl. the class borders."""
    from goliath_amd import splat
    from oracle import cref

    g = torch.Generator().manual_seed(3 + N)
    xys = (torch.rand(N, 2, generator=g) * 10 + 3).cuda()  # all inside tile (0,0)
    depths = (torch.rand(N, generator=g) + 1).cuda()
    if N > 200:
        depths[100:200] = depths[100]  # equal depths -> tie broken by id
    radii = torch.ones(N, dtype=torch.int32).cuda()
    nth = torch.ones(N, dtype=torch.int32)
    _, ids, bins = cref.bin_and_sort(xys.cpu(), depths.cpu(), radii.cpu(), nth, 64, 64, 16)
    ws = splat._Workspace(1, N, 16, N, "cuda")
    splat._bin_sort(1, N, xys, depths, radii, 64, 64, ws)
    assert torch.equal(ws.sorted_ids[0, :N].cpu(), ids)


def test_long_lists_sort_without_the_big_lds_allocation():
    """gol_bin_sort used to FAIL when the device would not grant sort_big_kernel its 147 KB of dynamic
    LDS.  Now the kernel falls back to the compare-exchange network on global memory; GOL_SORT_BIG_NO_LDS=1 takes that path
    on purpose (a static of the library: own process).  One tile with 6000 and 20000 entries, ids exact against the oracle."""
    import subprocess
    import sys

    code = (
        "import sys, torch\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from goliath_amd import splat\n"
        "from oracle import cref\n"
        "for N in (6000, 20000):\n"
        "    g = torch.Generator().manual_seed(3 + N)\n"
        "    xys = (torch.rand(N, 2, generator=g) * 10 + 3).cuda()\n"
        "    depths = (torch.rand(N, generator=g) + 1).cuda()\n"
        "    depths[100:200] = depths[100]\n"
        "    radii = torch.ones(N, dtype=torch.int32).cuda()\n"
        "    _, ids, bins = cref.bin_and_sort(xys.cpu(), depths.cpu(), radii.cpu(), torch.ones(N, dtype=torch.int32), 64, 64, 16)\n"
        "    ws = splat._Workspace(1, N, 16, N, 'cuda')\n"
        "    splat._bin_sort(1, N, xys, depths, radii, 64, 64, ws)\n"
        "    assert torch.equal(ws.sorted_ids[0, :N].cpu(), ids), N\n"
        "print('NO_LDS_OK')\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, GOL_SORT_BIG_NO_LDS="1"))
    assert r.returncode == 0 and "NO_LDS_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


@pytest.mark.parametrize("H,W,N", [(512, 512, 10_000), (100, 77, 1_500)])
def test_rasterize_forward_backward_vs_oracle(H, W, N):
    from goliath_amd import splat
    from oracle import cref

    s = head_scene(N, H, W, seed=0)
    g, hip, _ = _project_both(s)
    (xys, depths, radii, conics, comp, nth), ids, bins = _lists(hip, s)
    opac = (s["opacity"][:, 0] * comp).contiguous()
    bg = torch.tensor([0.3, 0.1, 0.2])
    ref_img, ref_T, ref_idx = cref.rasterize_forward(ids, bins, xys, conics, s["colors"], opac, H, W, 16, bg)

    cx = hip[0].detach().clone().requires_grad_(True)
    cc = hip[3].detach().clone().requires_grad_(True)
    col = g["colors"].clone().requires_grad_(True)
    op = opac.cuda()[:, None].clone().requires_grad_(True)
    img, alpha = splat.rasterize_gaussians(cx, hip[1], hip[2], cc, hip[5], col, op, H, W, 16, bg.cuda(),
                                           return_alpha=True)
    assert rel_l2(img, ref_img) < TIGHT
    assert rel_l2(1 - alpha, ref_T) < TIGHT
    assert float(alpha.detach().max()) > 0.5

    gen = torch.Generator().manual_seed(9)
    v_out = torch.randn(H, W, 3, generator=gen)
    v_alpha = torch.randn(H, W, generator=gen)
    (img * v_out.cuda()).sum().add((alpha * v_alpha.cuda()).sum()).backward()
    r_xy, r_conic, r_col, r_op = cref.rasterize_backward(ids, bins, xys, conics, s["colors"], opac, H, W, 16, bg,
                                                         ref_T, ref_idx, v_out, v_alpha)
    assert rel_l2(col.grad, r_col) < TIGHT
    assert rel_l2(op.grad, r_op) < TIGHT
    assert rel_l2(cx.grad, r_xy) < TIGHT  # (sums of signed terms, float32 accumulation order differs: measured 2.9e-7)
    assert rel_l2(cc.grad, r_conic) < TIGHT  # measured 3.7e-7


def test_rasterize_zero_intersections_quirk():
    from goliath_amd import splat

    N = 8
    z = torch.zeros(N, device="cuda")
    img, alpha = splat.rasterize_gaussians(torch.zeros(N, 2, device="cuda"), z, z.int(), torch.zeros(N, 3, device="cuda"),
                                           z.int(), torch.rand(N, 3, device="cuda"), z[:, None], 32, 48, 16,
                                           torch.tensor([0.2, 0.4, 0.6], device="cuda"), return_alpha=True)
    assert img.shape == (32, 48, 3) and torch.allclose(img[0, 0].cpu(), torch.tensor([0.2, 0.4, 0.6]))
    assert float(alpha.min()) == 1.0  # gsplat quirk: final_T = 0 when nothing intersects


def test_project_backward_vs_oracle():
    from goliath_amd import splat
    from oracle import cref

    s = head_scene(5_000, 256, 256, seed=2)
    g = _cuda(s)
    m = g["means"].clone().requires_grad_(True)
    sc = g["scales"].clone().requires_grad_(True)
    q = g["quats"].clone().requires_grad_(True)
    out = splat.project_gaussians(m, sc, 1.0, q, g["viewmat"], s["fx"], s["fy"], s["cx"], s["cy"], s["H"], s["W"],
                                  16, 0.1)
    gen = torch.Generator().manual_seed(5)
    v_xy, v_d = torch.randn(out[0].shape, generator=gen), torch.randn(out[1].shape, generator=gen)
    v_con, v_cmp = torch.randn(out[3].shape, generator=gen), torch.randn(out[4].shape, generator=gen)
    ((out[0] * v_xy.cuda()).sum() + (out[1] * v_d.cuda()).sum() + (out[3] * v_con.cuda()).sum()
     + (out[4] * v_cmp.cuda()).sum()).backward()
    fw = [t.detach().cpu() for t in out]
    _, _, r_mean, r_scale, r_quat = cref.project_gaussians_backward(
        s["means"], s["scales"], 1.0, s["quats"], s["viewmat"], s["fx"], s["fy"], fw[6], fw[2], fw[3], fw[4],
        v_xy, v_d, v_con, v_cmp)
    assert rel_l2(m.grad, r_mean) < TIGHT
    assert rel_l2(sc.grad, r_scale) < TIGHT
    assert rel_l2(q.grad, r_quat) < 1e-5   # measured 8.9e-7


def test_fused_render_matches_compat_chain_and_reference_wrapper_semantics():
    """render() (ONE fused colour+depth pass) == the reference wrapper's chain of
    project -> rasterize(colour) -> rasterize(depth) (render_gsplat.py:49-104), forward and grads."""
    from goliath_amd import render_gs, splat

    H, W, N = 200, 136, 4000
    s = head_scene(N, H, W, seed=4)
    g = _cuda(s)

    def leafs():
        return [g[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacity", "colors")]

    m, q, sc, op, col = leafs()
    out = render_gs.render(W, H, s["fx"], s["fy"], s["cx"], s["cy"], g["viewmat"], m, q, sc, op, col)
    m2, q2, sc2, op2, col2 = leafs()
    xys, depths, radii, conics, comp, nth, _ = splat.project_gaussians(
        m2, sc2, 1.0, q2, g["viewmat"], s["fx"], s["fy"], s["cx"], s["cy"], H, W, 16, 0.1)
    bg = torch.zeros(3, device="cuda")
    img, alpha = splat.rasterize_gaussians(xys, depths, radii, conics, nth, col2, op2 * comp[:, None], H, W, 16, bg,
                                           return_alpha=True)
    dimg = splat.rasterize_gaussians(xys, depths, radii, conics, nth, depths[:, None].expand(-1, 3).contiguous(),
                                     op2 * comp[:, None], H, W, 16, bg, return_alpha=True)[0][..., 0]
    assert rel_l2(out["render"], img.permute(2, 0, 1)) < 1e-6
    assert rel_l2(out["alpha"][0], alpha) < 1e-6
    assert rel_l2(out["depth"][0], dimg) < 1e-6
    assert torch.equal(out["radii"], radii)
    gen = torch.Generator().manual_seed(1)
    w_img, w_d = torch.randn(3, H, W, generator=gen).cuda(), torch.randn(H, W, generator=gen).cuda()
    ((out["render"] * w_img).sum() + (out["depth"][0] * w_d).sum() + out["alpha"].sum()).backward()
    ((img.permute(2, 0, 1) * w_img).sum() + (dimg * w_d).sum() + alpha.sum()).backward()
    for a, b, n in ((m, m2, "means"), (q, q2, "quats"), (sc, sc2, "scales"), (op, op2, "opacity"), (col, col2, "colors")):
        assert rel_l2(a.grad, b.grad) < TIGHT, (n, rel_l2(a.grad, b.grad))   # measured 1.9e-7


def test_config2_full_size_properties():
    """BASELINE config 2 size (250k Gaussians, 2048x1334), one view: oracle parity on the full image
    plus size-independent properties."""
    from goliath_amd import render_gs, splat
    from oracle import cref

    H, W, N = 2048, 1334, 250_000
    s = head_scene(N, H, W, seed=1234)
    g = _cuda(s)
    out = render_gs.render(W, H, s["fx"], s["fy"], s["cx"], s["cy"], g["viewmat"], g["means"], g["quats"],
                           g["scales"], g["opacity"], g["colors"])
    img, alpha = out["render"], out["alpha"]
    assert torch.isfinite(img).all() and float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0
    assert float(alpha.max()) > 0.99 and float((alpha > 0.5).float().mean()) > 0.1
    # determinism of the forward (sort ties are broken by id)
    out2 = render_gs.render(W, H, s["fx"], s["fy"], s["cx"], s["cy"], g["viewmat"], g["means"], g["quats"],
                            g["scales"], g["opacity"], g["colors"])
    assert torch.equal(out2["render"], img)
    # zero-opacity Gaussians contribute nothing; permuting the Gaussians changes nothing
    op0 = g["opacity"].clone()
    op0[::2] = 0
    keep = torch.arange(1, N, 2, device="cuda")
    a = render_gs.render(W, H, s["fx"], s["fy"], s["cx"], s["cy"], g["viewmat"], g["means"], g["quats"],
                         g["scales"], op0, g["colors"])["render"]
    b = render_gs.render(W, H, s["fx"], s["fy"], s["cx"], s["cy"], g["viewmat"], g["means"][keep], g["quats"][keep],
                         g["scales"][keep], g["opacity"][keep], g["colors"][keep])["render"]
    assert rel_l2(a, b) < 1e-6
    # oracle on the full image, fed with the HIP projection
    proj = splat.project_gaussians(g["means"], g["scales"], 1.0, g["quats"], g["viewmat"], s["fx"], s["fy"],
                                   s["cx"], s["cy"], H, W, 16, 0.1)
    (xys, depths, radii, conics, comp, nth), ids, bins = _lists(proj, s)
    opac = (s["opacity"][:, 0] * comp).contiguous()
    ref_img, ref_T, _ = cref.rasterize_forward(ids, bins, xys, conics, s["colors"], opac, H, W, 16, torch.zeros(3))
    assert rel_l2(img.permute(1, 2, 0), ref_img) < 4e-5   # measured 3.2e-6
    assert rel_l2(1 - alpha[0], ref_T) < TIGHT


def test_render_batch_matches_per_view_loop():
    """R0: one batched launch == the reference's per-view loop (rgca.py:119-145)."""
    from goliath_amd import render_gs

    H, W, N, B = 160, 120, 3000, 3
    views = [head_scene(N, H, W, seed=10 + b, cam_angle=0.4 * b) for b in range(B)]
    preds = {
        "primpos": torch.stack([v["means"] for v in views]).cuda(),
        "primqvec": torch.stack([v["quats"] for v in views]).cuda(),
        "primscale": torch.stack([v["scales"] for v in views]).cuda(),
        "opacity": torch.stack([v["opacity"] for v in views]).cuda(),
        "color": torch.stack([v["colors"] for v in views]).cuda(),
    }
    K = torch.zeros(B, 3, 3)
    for b, v in enumerate(views):
        K[b, 0, 0], K[b, 1, 1], K[b, 0, 2], K[b, 1, 2], K[b, 2, 2] = v["fx"], v["fy"], v["cx"], v["cy"], 1.0
    Rt = torch.stack([v["viewmat"] for v in views])
    rgb, alpha, depth = render_gs.render_batch(K.cuda(), Rt.cuda(), preds, H, W)
    assert rgb.shape == (B, 3, H, W) and alpha.shape == (B, 1, H, W) and depth.shape == (B, 1, H, W)
    for b, v in enumerate(views):
        o = render_gs.render(W, H, v["fx"], v["fy"], v["cx"], v["cy"], Rt[b].cuda(), preds["primpos"][b],
                             preds["primqvec"][b], preds["primscale"][b], preds["opacity"][b], preds["color"][b])
        a = 1.0 - o["final_T"]
        assert rel_l2(rgb[b], o["render"]) < 1e-6
        assert rel_l2(alpha[b], a) < 1e-6
        assert rel_l2(depth[b], o["depth"] / a.clamp(0.05, 1.0)) < 1e-6


@pytest.mark.parametrize("with_l1", [False, True])
@pytest.mark.parametrize("fused", [False, True])
def test_instrumented_pass_equals_the_single_call(fused, with_l1):
    """bench.py's per-call numbers come from the instrumented pass (_lib.TIMING set: one ABI call per stage).  It must
    compute what the single-call path computes -- identical tile lists and images, leaf gradients up to the order of the
    float atomics -- and make the calls bench.py keys on, in this order.  Unfused: render_views of the attributes; fused: the
    shading kernel projects (shading_tail(..., views=...)) and the render starts at the tile count."""
    import bench
    from goliath_amd import _lib, render_gs, shade, splat

    B, S, H, W = 2, 48, 160, 112
    N, cap = S * S, 1 << 18
    g = torch.Generator().manual_seed(21)
    target, mask = torch.rand(B, 3, H, W, generator=g).cuda(), (torch.rand(B, 1, H, W, generator=g) > 0.3).float().cuda()
    kw = dict(with_depth=True, capacity=cap, **(dict(l1_target=target, l1_mask=mask) if with_l1 else {}))
    if fused:
        cfg = dict(bench.CFG, gaussians=N, slab=S, height=H, width=W, views_per_gpu=B, focal=3000.0 * W / 1334.0, seed=5)
        t = bench.make_inputs(cfg, torch.device("cuda"))
        leaves = [t[k] for k in ("f_vn", "f_vc", "postex", "tn", "albedo")]
        vs = render_gs.view_set(t["K"], t["Rt"], H, W)
        lights = dict(light_intensity=(0.5 + torch.rand(B, 3, 1, generator=g)).cuda(),
                      headrel_light_pos=(400.0 * torch.randn(B, 3, 3, generator=g)).cuda(),
                      n_lights=torch.tensor([3, 2], dtype=torch.int32).cuda())

        def render():
            preds = shade.shading_tail(*leaves, t["light_sh"], t["campos"], views=vs, **lights)
            return splat.render_views(None, None, None, None, None, None, None, H, W, raw_depth=False,
                                      projected=preds["projected"], **kw)
        calls = ["gol_bin_sort", "gol_rasterize_fwd", "gol_rasterize_bwd"]
    else:
        views = [head_scene(N, H, W, seed=30 + b, cam_angle=0.4 * b) for b in range(B)]
        leaves = [torch.stack([v[k] for v in views]).cuda().requires_grad_(True)
                  for k in ("means", "scales", "quats", "opacity", "colors")]
        viewmats = torch.stack([v["viewmat"] for v in views]).cuda()
        intrins = torch.tensor([[v["fx"], v["fy"], v["cx"], v["cy"]] for v in views]).cuda()

        def render():
            return splat.render_views(*leaves, viewmats, intrins, H, W, **kw)
        calls = ["gol_project_fwd", "gol_bin_sort", "gol_rasterize_fwd", "gol_rasterize_bwd", "gol_project_bwd"]
    w = [torch.randn(B, c, H, W, generator=g).cuda() for c in (3, 1, 1)]

    def run(timing):
        for x in leaves:
            x.grad = None
        _lib.TIMING = [] if timing else None
        try:
            out = render()
            loss = (out["render"] * w[0]).sum() + (out["alpha"] * w[1]).sum() + (out["depth_norm"] * w[2]).sum()
            (loss + out["l1_loss"] if with_l1 else loss).backward()
            names = [n for n, _, _ in _lib.TIMING] if timing else None
        finally:
            _lib.TIMING = None
        return out, [x.grad.clone() for x in leaves], names

    plain, g0, _ = run(False)
    inst, g1, names = run(True)
    assert [n for n in names if not n.startswith("gol_shade_")] == calls
    n_isect = plain["n_isect"]
    assert torch.equal(inst["n_isect"], n_isect) and 0 < int(n_isect.min()) and int(n_isect.max()) <= cap
    assert torch.equal(inst["tile_bins"], plain["tile_bins"])
    for b in range(B):
        # only what the tiles list (pruned lists leave unwritten slots between them), and final_idx only on the pixels of
        # tiles with entries (the planar raster writes it for those alone: the backward skips empty tiles)
        bins = plain["tile_bins"][b]
        listed = torch.cat([torch.arange(s, e) for s, e in bins.tolist()]).cuda()
        assert torch.equal(inst["sorted_ids"][b, listed], plain["sorted_ids"][b, listed])
        busy = (bins[:, 1] > bins[:, 0]).reshape((H + 15) // 16, (W + 15) // 16)
        busy = busy.repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W]
        assert torch.equal(inst["final_idx"][b][busy], plain["final_idx"][b][busy])
    for k in ("radii", "render", "alpha", "depth_norm") + (("l1_loss",) if with_l1 else ()):
        assert torch.equal(inst[k], plain[k]), k
    assert float(plain["alpha"].max()) > 0.5 and int((plain["radii"] > 0).sum()) > N
    for i, (a, b) in enumerate(zip(g1, g0)):
        assert float(b.abs().max()) > 0 and rel_l2(a, b) < TIGHT, (i, rel_l2(a, b))
