"""GPU parity of the N-channel rasterizer (gol_rasterize_nd_fwd / _bwd, csrc/raster_nd.hip) -- gsplat 0.1.11's
rasterize_gaussians with colors[N, C], C != 3 -- against the C-generic CPU oracle (oracle/gsplat_oracle.c), against the
3-channel kernels, and through the gsplat drop-in.

Lists: the oracle bins the HIP projection (cref.bin_and_sort), as in test_gpu_splat.py; the HIP side bins with its own
(pruned, output-preserving) lists.  Bars as in test_gpu_splat.py: TIGHT relative L2 on small scenes with identical inputs.
"""
import sys

import pytest
import torch

from scenes import head_scene, rel_l2

pytestmark = pytest.mark.gpu
TIGHT = 5e-6    # test_gpu_splat.py's bar for the 3-channel rasterizer on the same scenes (measured there 3e-8 ... 4e-7)
SIZES = [(100, 77, 1_500), (512, 512, 10_000)]


def _setup(H, W, N, seed=0):
    from goliath_amd import splat
    from oracle import cref

    s = head_scene(N, H, W, seed=seed)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in s.items()}
    hip = splat.project_gaussians(g["means"], g["scales"], 1.0, g["quats"], g["viewmat"], s["fx"], s["fy"], s["cx"],
                                  s["cy"], H, W, 16, 0.1)
    hip = tuple(t.detach() for t in hip)
    xys, depths, radii, conics, comp, nth, _ = (t.cpu() for t in hip)
    _, ids, bins = cref.bin_and_sort(xys, depths, radii, nth, H, W, 16)
    opac = (s["opacity"][:, 0] * comp).contiguous()
    return hip, xys, conics, opac, ids, bins


def _inputs(H, W, N, C, seed=0):
    gen = torch.Generator().manual_seed(100 + C)
    colors = torch.rand(N, C, generator=gen)
    bg = torch.rand(C, generator=gen)
    v_out = torch.randn(H, W, C, generator=gen)
    v_alpha = torch.randn(H, W, generator=gen)
    return colors, bg, v_out, v_alpha


def _hip(hip, colors, opac, H, W, bg, v_out=None, v_alpha=None, retain=False):
    """rasterize_gaussians forward (+ backward of <img, v_out> + <alpha, v_alpha>) on the GPU."""
    from goliath_amd import splat

    cx = hip[0].clone().requires_grad_(True)
    cc = hip[3].clone().requires_grad_(True)
    col = colors.cuda().clone().requires_grad_(True)
    op = opac.cuda()[:, None].clone().requires_grad_(True)
    img, alpha = splat.rasterize_gaussians(cx, hip[1], hip[2], cc, hip[5], col, op, H, W, 16,
                                           None if bg is None else bg.cuda(), return_alpha=True)
    out = dict(img=img.detach().cpu(), alpha=alpha.detach().cpu())
    if v_out is not None:
        loss = (img * v_out.cuda()).sum() + (alpha * v_alpha.cuda()).sum()
        loss.backward(retain_graph=retain)
        out.update(xy=cx.grad.cpu(), conic=cc.grad.cpu(), col=col.grad.cpu(), op=op.grad.cpu())
        if retain:
            grads1 = [t.grad.clone() for t in (cx, cc, col, op)]
            for t in (cx, cc, col, op):
                t.grad = None
            loss.backward()
            out["second"] = (grads1, [t.grad.clone() for t in (cx, cc, col, op)])
    return out


def _oracle(xys, conics, colors, opac, ids, bins, H, W, bg, v_out, v_alpha):
    from oracle import cref

    img, T, idx = cref.rasterize_forward(ids, bins, xys, conics, colors, opac, H, W, 16, bg)
    r_xy, r_conic, r_col, r_op = cref.rasterize_backward(ids, bins, xys, conics, colors, opac, H, W, 16, bg, T, idx,
                                                         v_out, v_alpha)
    return dict(img=img, T=T, xy=r_xy, conic=r_conic, col=r_col, op=r_op)


@pytest.mark.parametrize("C", [1, 2, 4, 5, 8, 9, 12, 16])   # 9, 12: a masked 16-wide chunk
@pytest.mark.parametrize("H,W,N", SIZES)
def test_nd_forward_backward_vs_oracle(H, W, N, C):
    hip, xys, conics, opac, ids, bins = _setup(H, W, N)
    colors, bg, v_out, v_alpha = _inputs(H, W, N, C)
    h = _hip(hip, colors, opac, H, W, bg, v_out, v_alpha)
    r = _oracle(xys, conics, colors, opac, ids, bins, H, W, bg, v_out, v_alpha)
    assert h["img"].shape == (H, W, C)
    assert float(h["alpha"].max()) > 0.5
    assert rel_l2(h["img"], r["img"]) < TIGHT
    assert rel_l2(1 - h["alpha"], r["T"]) < TIGHT
    for k in ("col", "op", "xy", "conic"):
        assert rel_l2(h[k], r[k]) < TIGHT, (k, rel_l2(h[k], r[k]))


@pytest.mark.parametrize("C", [17, 25, 28, 32, 48])   # 25, 28: the last 16-wide chunk is masked
def test_nd_several_chunks_vs_oracle_slices(C):
    """C > 16 runs several 16-channel chunks (and a masked remainder chunk): the oracle applied to 16-channel slices gives
    the image and v_colors slice by slice, one final_T, and v_xy / v_conic / v_opacity as the sum over the slices with
    v_out_alpha given to one slice only (all of them are linear in the upstream gradient)."""
    H, W, N = 100, 77, 1_500
    hip, xys, conics, opac, ids, bins = _setup(H, W, N)
    colors, bg, v_out, v_alpha = _inputs(H, W, N, C)
    h = _hip(hip, colors, opac, H, W, bg, v_out, v_alpha)
    geo = {k: 0 for k in ("xy", "conic", "op")}
    T0 = None
    for a in range(0, C, 16):
        b = min(C, a + 16)
        r = _oracle(xys, conics, colors[:, a:b].contiguous(), opac, ids, bins, H, W, bg[a:b].contiguous(),
                    v_out[..., a:b].contiguous(), v_alpha if a == 0 else None)
        assert rel_l2(h["img"][..., a:b], r["img"]) < TIGHT, (a, b)
        assert rel_l2(h["col"][:, a:b], r["col"]) < TIGHT, (a, b)
        T0 = r["T"] if T0 is None else T0
        assert torch.equal(r["T"], T0)
        for k in geo:
            geo[k] = geo[k] + r[k]
    assert rel_l2(1 - h["alpha"], T0) < TIGHT
    for k in geo:
        assert rel_l2(h[k], geo[k]) < TIGHT, (k, rel_l2(h[k], geo[k]))


def test_nd_kernel_with_three_channels_equals_the_three_channel_kernel():
    """C = 3 forced through gol_rasterize_nd_* (the marshallers) == gol_rasterize_fwd / _bwd on the same lists."""
    from goliath_amd import splat

    H, W, N = 200, 136, 4_000
    hip, xys, conics, opac, ids, bins = _setup(H, W, N, seed=3)
    colors, bg, v_out, v_alpha = (t.cuda() for t in _inputs(H, W, N, 3))
    o = opac.cuda()
    ws = splat._Workspace(1, N, splat._tiles(H, W), int(hip[5].sum()), "cuda")
    splat._bin_sort(1, N, hip[0], hip[1], hip[2], H, W, ws, hip[3], o)
    rec3 = splat._pack_records(1, N, hip[0], hip[3], colors, None, o)
    recn = splat._pack_records(1, N, hip[0], hip[3], None, None, o)
    assert float(recn[..., 6:9].abs().max()) == 0.0   # colors = NULL: r = g = b = 0
    lists = dict(B=1, N=N, img_h=H, img_w=W, tile_bins=ws.tile_bins, sorted_ids=ws.sorted_ids, capacity=ws.capacity)
    f = lambda *s, **k: torch.empty(*s, device="cuda", **k)
    img3, T3, idx3 = f(1, H, W, 3), f(1, H, W), f(1, H, W, dtype=torch.int32)
    imgn, Tn, idxn = f(1, H, W, 3), f(1, H, W), f(1, H, W, dtype=torch.int32)
    splat._abi_rasterize_fwd(**lists, planar=0, records=rec3, with_extra=0, background=bg, out_img=img3, final_Ts=T3,
                             final_idx=idx3)
    splat._abi_rasterize_nd_fwd(**lists, C=3, records=recn, colors=colors, background=bg, out_img=imgn, final_Ts=Tn,
                                final_idx=idxn)
    assert rel_l2(imgn, img3) < TIGHT
    assert rel_l2(Tn, T3) < TIGHT
    assert float((idxn != idx3).float().mean()) < 1e-4
    g3 = [torch.zeros(N, k, device="cuda") for k in (2, 3, 3, 1)]
    gn = [torch.zeros(N, k, device="cuda") for k in (2, 3, 3, 1)]
    vo, va = v_out.contiguous(), v_alpha.contiguous()
    splat._abi_rasterize_bwd(**lists, planar=0, records=rec3, with_extra=0, background=bg, final_Ts=T3, final_idx=idx3,
                             v_out_img=vo, v_out_alpha=va, v_xy=g3[0], v_conic=g3[1], v_colors=g3[2], v_opacity=g3[3])
    splat._abi_rasterize_nd_bwd(**lists, C=3, records=recn, colors=colors, background=bg, final_Ts=Tn, final_idx=idxn,
                                v_out_img=vo, v_out_alpha=va, v_xy=gn[0], v_conic=gn[1], v_colors=gn[2], v_opacity=gn[3])
    for name, a, b in zip(("xy", "conic", "colors", "opacity"), gn, g3):
        assert float(b.abs().max()) > 0 and rel_l2(a, b) < TIGHT, (name, rel_l2(a, b))


def test_nd_rgb_plus_depth_equals_two_three_channel_calls():
    """C = 4 colours = (rgb, depth): channels 0-2 are the 3-channel image of rgb, channel 3 the one of depth."""
    H, W, N = 200, 136, 4_000
    hip, xys, conics, opac, ids, bins = _setup(H, W, N, seed=4)
    rgb = torch.rand(N, 3, generator=torch.Generator().manual_seed(1))
    depth = hip[1].cpu()[:, None]
    bg = torch.tensor([0.2, 0.4, 0.6, 0.0])
    h4 = _hip(hip, torch.cat([rgb, depth], 1), opac, H, W, bg)
    h3 = _hip(hip, rgb, opac, H, W, bg[:3])
    hd = _hip(hip, depth.expand(-1, 3).contiguous(), opac, H, W, bg[3:].expand(3).contiguous())
    assert rel_l2(h4["img"][..., :3], h3["img"]) < TIGHT
    assert rel_l2(h4["img"][..., 3], hd["img"][..., 0]) < TIGHT
    assert rel_l2(h4["alpha"], h3["alpha"]) < TIGHT


def test_nd_zero_intersections_quirk():
    """I < 1 (gsplat): the background image and alpha = 1, for any C."""
    from goliath_amd import splat

    N, C = 8, 5
    z = torch.zeros(N, device="cuda")
    bg = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5], device="cuda")
    img, alpha = splat.rasterize_gaussians(torch.zeros(N, 2, device="cuda"), z, z.int(), torch.zeros(N, 3, device="cuda"),
                                           z.int(), torch.rand(N, C, device="cuda"), z[:, None], 32, 48, 16, bg,
                                           return_alpha=True)
    assert img.shape == (32, 48, C) and torch.equal(img[5, 7].cpu(), bg.cpu())
    assert float(alpha.min()) == 1.0


def test_nd_uint8_colours_background_none_and_retain_graph():
    from goliath_amd import splat

    H, W, N, C = 100, 77, 1_500, 4
    hip, xys, conics, opac, ids, bins = _setup(H, W, N, seed=5)
    colors, bg, v_out, v_alpha = _inputs(H, W, N, C)
    # uint8 colours are divided by 255
    c8 = (colors * 255).to(torch.uint8)
    a = splat.rasterize_gaussians(hip[0], hip[1], hip[2], hip[3], hip[5], c8.cuda(), opac.cuda()[:, None], H, W, 16,
                                  bg.cuda())
    b = splat.rasterize_gaussians(hip[0], hip[1], hip[2], hip[3], hip[5], c8.float().cuda() / 255, opac.cuda()[:, None],
                                  H, W, 16, bg.cuda())
    assert a.shape == (H, W, C) and torch.equal(a, b)
    # background None: ones(C)
    hn = _hip(hip, colors, opac, H, W, None)
    h1 = _hip(hip, colors, opac, H, W, torch.ones(C))
    assert torch.equal(hn["img"], h1["img"])
    with pytest.raises(AssertionError):
        splat.rasterize_gaussians(hip[0], hip[1], hip[2], hip[3], hip[5], colors.cuda(), opac.cuda()[:, None], H, W, 16,
                                  torch.ones(3, device="cuda"))
    # a second backward through the same graph (the tile lists stay alive on the node): the same gradients
    h = _hip(hip, colors, opac, H, W, bg, v_out, v_alpha, retain=True)
    first, second = h["second"]
    for g1, g2 in zip(first, second):
        assert float(g1.abs().max()) > 0 and rel_l2(g2, g1) < TIGHT


def test_nd_through_the_gsplat_dropin(monkeypatch):
    """dropin.install() -> gsplat.rasterize_gaussians(..., colors[N, 8], ...) runs and matches the oracle."""
    from goliath_amd import dropin

    H, W, N, C = 100, 77, 1_500, 8
    hip, xys, conics, opac, ids, bins = _setup(H, W, N, seed=6)
    colors, bg, v_out, v_alpha = _inputs(H, W, N, C)
    # every module name install() registers is restored (or removed again) when the test ends
    for name in ("gsplat", "sgutilslib", "mvpraymarchlib", "utilslib"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    registered = dropin.install()
    assert set(registered) <= {"gsplat", "sgutilslib", "mvpraymarchlib", "utilslib"}
    import gsplat

    img = gsplat.rasterize_gaussians(hip[0], hip[1], hip[2], hip[3], hip[5], colors.cuda(), opac.cuda()[:, None], H, W, 16,
                                     bg.cuda())
    r = _oracle(xys, conics, colors, opac, ids, bins, H, W, bg, v_out, v_alpha)
    assert img.shape == (H, W, C)
    assert rel_l2(img, r["img"]) < TIGHT
