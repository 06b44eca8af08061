"""GPU: every tile of the image is rendered by exactly one workgroup, whatever the number of tile rows.

The raster launches hand groups of 8 tile rows (one row per die) to their workgroups in an order that is not top to bottom
(csrc/gol_raster.h: tile_of_block / row_order deals the groups out from the three thirds of the image in turn).  Any
bijection is correct; one that is not a bijection renders a tile twice and another not at all.  Here: images 40 pixels wide
(3 tiles, the last one partial) whose heights give 1, 2, 3, 5 and 9 row groups -- and one height that is no multiple of 16
-- rendered into memory that held NaNs, against the CPU oracle fed with the same projection.  A tile no workgroup wrote
stays NaN.

Bars: TIGHT = 5e-6, what tests/test_gpu_splat.py holds the same kernels to against the same oracle (identical inputs, a few
hundred Gaussians: rounding noise only, measured there 3e-8 ... 4e-7).
"""
import pytest
import torch

from scenes import head_scene, rel_l2

pytestmark = pytest.mark.gpu
TIGHT = 5e-6
W = 40
# height -> tile rows -> groups of 8 rows:  16 -> 1 -> 1;  144 -> 9 -> 2;  150 -> 10 -> 2 (last tile row 6 pixels high);
# 272 -> 17 -> 3;  528 -> 33 -> 5;  1040 -> 65 -> 9
HEIGHTS = [16, 144, 150, 272, 528, 1040]


def _scene(H):
    """A few hundred Gaussians of 1-4 pixels over the whole 40 x H image, seen from far away (nearly orthographic)."""
    N = 200 + H // 2
    s = head_scene(N, H, W, seed=H, cam_angle=0.0, focal=1000.0, cam_dist=7000.0, radii=(150.0, 3.6 * H, 50.0),
                   scale_range=(5.0, 30.0))
    return s, {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in s.items()}


def _oracle_lists(s, g):
    from goliath_amd import splat
    from oracle import cref

    H = s["H"]
    hip = splat.project_gaussians(g["means"], g["scales"], 1.0, g["quats"], g["viewmat"], s["fx"], s["fy"], s["cx"],
                                  s["cy"], H, W, 16, 0.1)
    xys, depths, radii, conics, comp, nth, _ = (t.detach().cpu() for t in hip)
    _, ids, bins = cref.bin_and_sort(xys, depths, radii, nth, H, W, 16)
    opac = (s["opacity"][:, 0] * comp).contiguous()
    return hip, (xys, depths, radii, conics, nth), ids, bins, opac


def _poison(*sizes):
    """Leave NaNs in the blocks the caching allocator hands to the next allocations of these sizes (in floats)."""
    ts = [torch.full((n,), float("nan"), device="cuda") for n in sizes]
    del ts


@pytest.mark.parametrize("H", HEIGHTS)
def test_every_tile_is_rendered_once_forward(H):
    from goliath_amd import render_gs, splat
    from oracle import cref

    s, g = _scene(H)
    _, (xys, depths, radii, conics, nth), ids, bins, opac = _oracle_lists(s, g)
    tiles_y = (H + 15) // 16
    per_row = (bins[:, 1] - bins[:, 0]).reshape(tiles_y, 3).sum(1)
    assert int((per_row > 0).sum()) >= (3 * tiles_y + 3) // 4, "the scene leaves too many tile rows empty"
    bg = torch.tensor([0.3, 0.1, 0.2])
    ref_img, ref_T, _ = cref.rasterize_forward(ids, bins, xys, conics, s["colors"], opac, H, W, 16, bg)
    ref_d, _, _ = cref.rasterize_forward(ids, bins, xys, conics, depths[:, None].expand(-1, 3).contiguous(), opac, H, W,
                                         16, torch.zeros(3))
    # the outputs (rgb, alpha, depth, depth_norm) and the workspace (final_T, final_idx) come out of NaN-filled blocks
    ws_floats = splat._layout(1, s["means"].shape[0], H, W, splat.PLANNER.initial(s["means"].shape[0], tiles_y * 3), 0).total // 4
    _poison(3 * H * W, H * W, H * W, H * W, ws_floats)
    out = render_gs.render(W, H, s["fx"], s["fy"], s["cx"], s["cy"], g["viewmat"], g["means"], g["quats"], g["scales"],
                           g["opacity"], g["colors"], bg_color=bg.cuda())
    for k in ("render", "alpha", "depth", "final_T"):
        assert torch.isfinite(out[k]).all(), (k, "a tile was left unwritten")
    e = {"rgb": rel_l2(out["render"].permute(1, 2, 0), ref_img), "final_T": rel_l2(out["final_T"][0], ref_T),
         "alpha": rel_l2(out["alpha"][0], 1 - ref_T), "depth": rel_l2(out["depth"][0], ref_d[..., 0])}
    print(f"H={H}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert float(out["alpha"].max()) > 0.5
    assert all(v < TIGHT for v in e.values()), e


@pytest.mark.parametrize("H", HEIGHTS)
def test_every_tile_is_rendered_once_backward(H):
    """The backward takes its tiles from the same function: gradients of the gsplat-layout operator against the oracle's
    (a tile visited twice doubles the gradients of its Gaussians, one never visited leaves them out)."""
    from goliath_amd import splat
    from oracle import cref

    s, g = _scene(H)
    hip, (xys, depths, radii, conics, nth), ids, bins, opac = _oracle_lists(s, g)
    bg = torch.tensor([0.3, 0.1, 0.2])
    _, ref_T, ref_idx = cref.rasterize_forward(ids, bins, xys, conics, s["colors"], opac, H, W, 16, bg)
    cx = hip[0].detach().clone().requires_grad_(True)
    cc = hip[3].detach().clone().requires_grad_(True)
    col = g["colors"].clone().requires_grad_(True)
    op = opac.cuda()[:, None].clone().requires_grad_(True)
    _poison(3 * H * W, H * W)
    img, alpha = splat.rasterize_gaussians(cx, hip[1], hip[2], cc, hip[5], col, op, H, W, 16, bg.cuda(), return_alpha=True)
    assert torch.isfinite(img).all() and torch.isfinite(alpha).all()
    gen = torch.Generator().manual_seed(9)
    v_out, v_alpha = torch.randn(H, W, 3, generator=gen), torch.randn(H, W, generator=gen)
    (img * v_out.cuda()).sum().add((alpha * v_alpha.cuda()).sum()).backward()
    r_xy, r_conic, r_col, r_op = cref.rasterize_backward(ids, bins, xys, conics, s["colors"], opac, H, W, 16, bg, ref_T,
                                                         ref_idx, v_out, v_alpha)
    e = {"colors": rel_l2(col.grad, r_col), "opacity": rel_l2(op.grad, r_op), "xy": rel_l2(cx.grad, r_xy),
         "conic": rel_l2(cc.grad, r_conic)}
    print(f"H={H}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v < TIGHT for v in e.values()), e
