"""GPU parity of the raster backward's per-batch merge: the gradient slots of a 64-entry batch are summed over the waves
and weighted once per entry, then added to the 64-byte gradient records by 16 lanes per record (raster.hip, PACKED).

Small hand-built views (B = 2, a few hundred Gaussians of 1-3 px) at the smallest shapes at which the merge can go wrong:
tile lists with a short last batch and with three batches, entries that reach only one 16x8 half of a tile (one wave's
slot row stays untouched), partial tiles at both image edges, both wave layouts (pixels_per_lane 1 and 2: 4 and 2 slot
rows per entry), with and without the extra channel's gradient (component 9).  The packed output is compared with the
dense path (grad_stride = 0: thread per entry, separate arrays) on identical inputs and both with the CPU oracle.
"""
import functools
import math

import pytest
import torch

from scenes import rel_l2

pytestmark = pytest.mark.gpu
TIGHT = 5e-6    # the bar of tests/test_gpu_splat.py for these gradients at small sizes (measured 3e-8 ... 4e-7 there)
B, N = 2, 600
BG = (0.3, 0.1, 0.2)


def _view(g, H, W):
    """One view's projected attributes: centres over the image and a pixel beyond it, sigma 0.3-1 px along rotated axes."""
    xys = torch.rand(N, 2, generator=g) * torch.tensor([W + 2.0, H + 2.0]) - 1.0
    s1, s2 = (0.3 + 0.7 * torch.rand(N, generator=g) for _ in range(2))
    th = math.pi * torch.rand(N, generator=g)
    c, s = torch.cos(th), torch.sin(th)
    xx, xy, yy = c * c * s1 * s1 + s * s * s2 * s2, c * s * (s1 * s1 - s2 * s2), s * s * s1 * s1 + c * c * s2 * s2
    det = xx * yy - xy * xy
    conics = torch.stack([yy / det, -xy / det, xx / det], 1)
    radii = torch.ceil(3.0 * torch.maximum(s1, s2)).to(torch.int32)     # gsplat: 3 sigma of the major axis
    depths = 1.0 + torch.rand(N, generator=g)
    opac = 0.2 + 0.7 * torch.rand(N, generator=g)
    colors = torch.rand(N, 3, generator=g)
    # gsplat's tile rectangle of a Gaussian (get_tile_bbox)
    tiles = torch.tensor([(W + 15) // 16, (H + 15) // 16])
    tc, tr = xys / 16.0, radii[:, None].float() / 16.0
    tmin = torch.minimum((tc - tr).int().clamp(min=0), tiles)
    tmax = torch.minimum((tc + tr + 1).int().clamp(min=0), tiles)
    nth = ((tmax[:, 0] - tmin[:, 0]) * (tmax[:, 1] - tmin[:, 1])).to(torch.int32)
    return dict(xys=xys, conics=conics.contiguous(), radii=radii, depths=depths, opac=opac, colors=colors, nth=nth)


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """Scene, upstream gradients and the oracle's gradients (with and without the extra channel's) of one image size:
    computed once, shared by the variants and left unchanged."""
    from oracle import cref

    g = torch.Generator().manual_seed(100 * H + W)
    views = [_view(g, H, W) for _ in range(B)]
    v_out = torch.randn(B, H, W, 4, generator=g)      # rgb + extra
    v_alpha = torch.randn(B, H, W, generator=g)
    bg4 = torch.tensor(BG + (0.0,))                   # the extra channel composites over 0
    ref = {False: [], True: []}
    for b, v in enumerate(views):
        _, ids, bins = cref.bin_and_sort(v["xys"], v["depths"], v["radii"], v["nth"], H, W, 16)
        col4 = torch.cat([v["colors"], v["depths"][:, None]], 1).contiguous()
        _, Ts, idx = cref.rasterize_forward(ids, bins, v["xys"], v["conics"], col4, v["opac"], H, W, 16, bg4)
        for extra in (False, True):
            vo = v_out[b].clone()
            if not extra:
                vo[..., 3] = 0.0
            r_xy, r_conic, r_col, r_op = cref.rasterize_backward(ids, bins, v["xys"], v["conics"], col4, v["opac"], H, W,
                                                                 16, bg4, Ts, idx, vo, v_alpha[b])
            ref[extra].append(dict(v_colors=r_col[:, :3], v_opacity=r_op, v_xy=r_xy, v_conic=r_conic, v_extra=r_col[:, 3:4]))
    ref = {e: {k: torch.stack([r[k] for r in rs]) for k in rs[0]} for e, rs in ref.items()}
    stack = lambda k: torch.stack([v[k] for v in views]).contiguous()
    return dict(v_out=v_out, v_alpha=v_alpha, ref=ref, **{k: stack(k) for k in views[0]})


def _one_half_entries(c, H, W):
    """Gaussians whose alpha >= 1/255 ellipse lies within the pixel rows of ONE 16x8 half of a tile: |dy| of the ellipse
    sigma <= ln(255 opacity) is at most sqrt(2 tau a / (a c - b^2)); centre inside the image."""
    a, b, cc = c["conics"].unbind(-1)
    tau = torch.log(255.0 * c["opac"])
    dy = torch.sqrt(2.0 * tau * a / (a * cc - b * b))
    x, y = c["xys"].unbind(-1)
    lo, hi = torch.floor((y - dy - 0.5) / 8.0), torch.floor((y + dy - 0.5) / 8.0)
    return (lo == hi) & (y - dy > 0.5) & (y + dy < H - 0.5) & (x > 0.5) & (x < W - 0.5)


@pytest.mark.parametrize("extra", [False, True], ids=["rgb", "extra"])
@pytest.mark.parametrize("ppl", [1, 2])
@pytest.mark.parametrize("H,W", [(32, 32), (24, 40)])     # 2 x 2 full tiles; 40 wide x 24 high: partial tiles at both edges
def test_packed_merge_vs_dense_and_oracle(H, W, ppl, extra):
    from goliath_amd import splat

    c = _case(H, W)
    dev = torch.device("cuda")
    d = {k: c[k].to(dev) for k in ("xys", "conics", "radii", "depths", "opac", "colors")}
    T = splat._tiles(H, W)
    cap = int(c["nth"].sum(1).max()) + 64
    ws = splat._Workspace(B, N, T, cap, dev)
    splat._bin_sort(B, N, d["xys"], d["depths"], d["radii"], H, W, ws, d["conics"], d["opac"])
    # the lists the kernel walks: a short last batch, three batches, entries that reach one half of a tile only
    n = (ws.tile_bins[..., 1] - ws.tile_bins[..., 0]).cpu().flatten()
    assert int(ws.n_isect.max()) <= cap
    assert bool(((n > 64) & (n % 64 != 0)).any()), n.tolist()
    assert int(n.max()) >= 129, n.tolist()
    assert int(_one_half_entries(c, H, W).sum()) >= 8

    records = splat._pack_records(B, N, d["xys"], d["conics"], d["colors"], d["depths"], d["opac"])
    bg = torch.tensor(BG, device=dev)
    out_img = torch.empty(B, 3, H, W, device=dev)
    out_extra = torch.empty(B, H, W, device=dev)
    fT = torch.empty(B, H, W, device=dev)
    fidx = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    lists = dict(B=B, N=N, img_h=H, img_w=W, planar=1, tile_bins=ws.tile_bins, sorted_ids=ws.sorted_ids, capacity=cap,
                 records=records, background=bg, final_Ts=fT, final_idx=fidx, pixels_per_lane=ppl)
    splat._abi_rasterize_fwd(**lists, with_extra=1, out_img=out_img, out_extra=out_extra)
    # ... and the backward walks them: some pixel's last entry lies three batches behind its tile's first
    bins_h, fidx_h, tiles_x = ws.tile_bins.cpu(), fidx.cpu(), (W + 15) // 16
    depth = [int(fidx_h[b, 16 * (t // tiles_x):16 * (t // tiles_x) + 16, 16 * (t % tiles_x):16 * (t % tiles_x) + 16].max())
             - int(bins_h[b, t, 0]) for b in range(B) for t in range(T) if bins_h[b, t, 1] > bins_h[b, t, 0]]
    assert max(depth) >= 128, depth

    v_img = c["v_out"][..., :3].permute(0, 3, 1, 2).contiguous().to(dev)
    up = dict(v_out_img=v_img, v_out_alpha=c["v_alpha"].to(dev), with_extra=int(extra),
              v_out_extra=c["v_out"][..., 3].contiguous().to(dev) if extra else None)
    rec = torch.zeros(B, N, splat.GRAD_RECORD, device=dev)
    field = lambda k: rec.data_ptr() + 4 * k
    splat._abi_rasterize_bwd(**lists, **up, v_xy=field(4), v_conic=field(6), v_colors=field(0), v_opacity=field(3),
                             v_extra=field(9) if extra else None, grad_stride=splat.GRAD_RECORD)
    dense = dict(v_colors=torch.zeros(B, N, 3, device=dev), v_opacity=torch.zeros(B, N, 1, device=dev),
                 v_xy=torch.zeros(B, N, 2, device=dev), v_conic=torch.zeros(B, N, 3, device=dev),
                 v_extra=torch.zeros(B, N, 1, device=dev))
    splat._abi_rasterize_bwd(**lists, **up, v_xy=dense["v_xy"], v_conic=dense["v_conic"], v_colors=dense["v_colors"],
                             v_opacity=dense["v_opacity"], v_extra=dense["v_extra"] if extra else None, grad_stride=0)
    torch.cuda.synchronize()

    packed = dict(v_colors=rec[..., 0:3], v_opacity=rec[..., 3:4], v_xy=rec[..., 4:6], v_conic=rec[..., 6:9],
                  v_extra=rec[..., 9:10])
    ref = c["ref"][extra]
    names = ["v_colors", "v_opacity", "v_xy", "v_conic"] + (["v_extra"] if extra else [])
    errs = {k: (rel_l2(packed[k], dense[k]), rel_l2(packed[k], ref[k]), rel_l2(dense[k], ref[k])) for k in names}
    print({k: tuple("%.1e" % e for e in v) for k, v in errs.items()})
    for k, (pd, po, do) in errs.items():
        assert float(ref[k].abs().max()) > 0, k
        assert pd < TIGHT, (k, "packed vs dense", pd)
        assert po < TIGHT, (k, "packed vs oracle", po)
        assert do < TIGHT, (k, "dense vs oracle", do)
    # fields the merge does not own stay exactly zero: the pad floats, and component 9 without an extra gradient
    assert not bool(rec[..., 10:].any())
    if not extra:
        assert not bool(rec[..., 9].any())
