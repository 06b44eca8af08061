"""GPU parity of the raster backward's two savings (raster.hip, gol_raster.h):

  * stage_mask: the forward stores the wave mask of every list entry it stages (one byte beside sorted_ids), the backward
    of the same render takes it back instead of running the ellipse-vs-footprint test again.  With the buffer, without it
    and with GOL_RASTER_STAGE_MASK=0 the forward's outputs must be bit-identical and the gradients equal up to the order of
    the float atomics (the packed-versus-dense bar of tests/test_gpu_raster_merge.py); where the forward's footprint is not
    the backward's (one pixel per lane: launches of one or two views, or forced) the backward must compute the masks itself;
  * composite form: v_alpha = T (w - R) with one running composite R instead of T w + ra (tail - q).  Gradients against the
    CPU oracle stay inside the 5e-6 of tests/test_gpu_raster_merge.py, with a non-zero background, v_out_alpha set, pixels
    whose alpha reaches the backward's 0.99 cap and pixels that stopped with the smallest transmittance the forward can
    leave (it never leaves T <= 1e-4: the entry that would take a pixel there is not composited; the walls below bring
    every pixel of their tile to 1.1e-4 .. 1.4e-4).

The tile lists are built by hand (tile_bins / sorted_ids are inputs of the low-level entries, the oracle takes the same
lists), so that each image holds exactly the lists the kernels can go wrong at -- 32 x 32: four full tiles; 24 high x 40
wide: partial tiles at both edges and an empty tile:
  "long"   300 entries: crosses the forward's batch of 256 and four of the backward's 64; three blobs of opacity 1 centred
           on a pixel in front, so that pixel and its neighbours reach the alpha cap and stop at once while the rest of the
           tile walks the whole list
  "even"   256 entries: the list ends exactly on a batch boundary of both directions
  "wall"   four near-uniform layers of alpha ~0.9, 0.9, 0.9, 0.89 and a fifth in front of 300 more entries: every pixel of
           the tile stops at the fifth -- the forward never stages the list's second batch (its mask bytes stay unwritten)
           and the backward starts four entries into a list of 305
  "short"  130 / 70 entries, "none": no entries.
Measured maxima of rel-L2 on MI355X are in the docstrings of the tests.
"""
import functools
import math
import os

import pytest
import torch

from scenes import rel_l2

pytestmark = pytest.mark.gpu
TIGHT = 5e-6     # tests/test_gpu_raster_merge.py: packed versus dense, and either against the oracle
NV = 4           # views of a scene; the one-view launches take the first
BG = (0.3, 0.1, 0.2)
SIZES = [(32, 32), (24, 40)]
LAYOUT = {(32, 32): ["long", "even", "wall", "short130"],
          (24, 40): ["short70", "none", "wall", "even", "short130", "long"]}   # tile order: row-major
SENT = 0xAB


def _small(g, n, x0, x1, y0, y1):
    """n Gaussians of 0.3-1 px along rotated axes, centres over the rectangle and a pixel beyond it."""
    xys = torch.rand(n, 2, generator=g) * torch.tensor([x1 - x0 + 2.0, y1 - y0 + 2.0]) + torch.tensor([x0 - 1.0, y0 - 1.0])
    s1, s2 = (0.3 + 0.7 * torch.rand(n, generator=g) for _ in range(2))
    th = math.pi * torch.rand(n, generator=g)
    c, s = torch.cos(th), torch.sin(th)
    xx, xy, yy = c * c * s1 * s1 + s * s * s2 * s2, c * s * (s1 * s1 - s2 * s2), s * s * s1 * s1 + c * c * s2 * s2
    det = xx * yy - xy * xy
    return xys, torch.stack([yy / det, -xy / det, xx / det], 1), 0.2 + 0.7 * torch.rand(n, generator=g)


def _round(n, cx, cy, sigma, opac):
    """n isotropic Gaussians of `sigma` px at (cx, cy) with the opacities `opac`."""
    return (torch.tensor([[cx, cy]] * n), torch.tensor([[1.0 / sigma ** 2, 0.0, 1.0 / sigma ** 2]] * n),
            torch.tensor(opac, dtype=torch.float32))


def _view(g, H, W):
    """One view: attributes of all Gaussians, the concatenated tile lists and their [start, end) ranges."""
    tiles_x = (W + 15) // 16
    parts, ids, bins, n0 = [], [], [], 0
    for t, kind in enumerate(LAYOUT[(H, W)]):
        x0, y0 = 16 * (t % tiles_x), 16 * (t // tiles_x)
        x1, y1 = min(x0 + 16, W), min(y0 + 16, H)
        front = None
        if kind == "long":
            front, n = _round(3, 0.5 * (x0 + x1) + 0.5, 0.5 * (y0 + y1) + 0.5, 8.0, [1.0, 1.0, 1.0]), 297
        elif kind == "wall":
            front, n = _round(5, 0.5 * (x0 + x1), 0.5 * (y0 + y1), 200.0, [0.9, 0.9, 0.9, 0.89, 0.9]), 300
        else:
            n = {"even": 256, "short130": 130, "short70": 70, "none": 0}[kind]
        small = _small(g, n, x0, x1, y0, y1)
        order = torch.argsort(torch.rand(n, generator=g))          # "depth" order of the tile's small Gaussians
        start = sum(len(i) for i in ids)
        if front is not None:
            parts.append(front)
            ids.append(torch.arange(n0, n0 + len(front[0])))
            n0 += len(front[0])
        parts.append(small)
        ids.append(n0 + order)
        n0 += n
        bins.append((start, sum(len(i) for i in ids)))
    xys, conics, opac = (torch.cat([p[k] for p in parts]).contiguous() for k in range(3))
    return dict(xys=xys, conics=conics, opac=opac, colors=torch.rand(n0, 3, generator=g), depths=1.0 + torch.rand(n0, generator=g),
                ids=torch.cat(ids).to(torch.int32), bins=torch.tensor(bins, dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """Scene, upstream gradients, the oracle's forward state and gradients (with and without the extra channel's) of one
    image size: computed once, shared by the variants and left unchanged."""
    from oracle import cref

    g = torch.Generator().manual_seed(100 * H + W)
    views = [_view(g, H, W) for _ in range(NV)]
    v_out = torch.randn(NV, H, W, 4, generator=g)      # rgb + extra
    v_alpha = torch.randn(NV, H, W, generator=g)
    bg4 = torch.tensor(BG + (0.0,))
    ref, fT = {False: [], True: []}, []
    for b, v in enumerate(views):
        col4 = torch.cat([v["colors"], v["depths"][:, None]], 1).contiguous()
        _, Ts, idx = cref.rasterize_forward(v["ids"], v["bins"], v["xys"], v["conics"], col4, v["opac"], H, W, 16, bg4)
        fT.append(Ts)
        for extra in (False, True):
            vo = v_out[b].clone()
            if not extra:
                vo[..., 3] = 0.0
            r_xy, r_conic, r_col, r_op = cref.rasterize_backward(v["ids"], v["bins"], v["xys"], v["conics"], col4, v["opac"],
                                                                 H, W, 16, bg4, Ts, idx, vo, v_alpha[b])
            ref[extra].append(dict(v_colors=r_col[:, :3], v_opacity=r_op, v_xy=r_xy, v_conic=r_conic, v_extra=r_col[:, 3:4]))
    ref = {e: {k: torch.stack([r[k] for r in rs]) for k in rs[0]} for e, rs in ref.items()}
    stack = lambda k: torch.stack([v[k] for v in views]).contiguous()
    return dict(v_out=v_out, v_alpha=v_alpha, ref=ref, ref_T=torch.stack(fT), N=len(views[0]["opac"]),
                **{k: stack(k) for k in views[0]})


def _guarded(n, dev, guard=256):
    buf = torch.full((n + 2 * guard,), SENT, dtype=torch.uint8, device=dev)
    return buf, buf[guard:guard + n]


def _render(c, H, W, nb, extra, *, mask, fwd_ppl=0, bwd_ppl=0, mask_ppl=None, env=None, dense=False, skip_fwd=None):
    """Forward + backward of the first nb views through the low-level entries.  mask: hand a stage_mask buffer to both;
    mask_ppl: what the backward is told the forward ran with (default: what it did run with); skip_fwd: take this forward
    state (and its mask buffer as it is) instead of running one.  -> dict of outputs (gradients as [nb, N, k])."""
    from goliath_amd import splat

    dev = torch.device("cuda")
    N, cap = c["N"], c["ids"].shape[1]
    old = os.environ.pop("GOL_RASTER_STAGE_MASK", None)
    if env is not None:
        os.environ["GOL_RASTER_STAGE_MASK"] = env
    try:
        d = {k: c[k][:nb].contiguous().to(dev) for k in ("xys", "conics", "depths", "opac", "colors", "ids", "bins")}
        records = splat._pack_records(nb, N, d["xys"], d["conics"], d["colors"], d["depths"], d["opac"])
        bg = torch.tensor(BG, device=dev)
        o = skip_fwd or dict(out_img=torch.empty(nb, 3, H, W, device=dev), out_extra=torch.empty(nb, H, W, device=dev),
                             out_alpha=torch.empty(nb, H, W, device=dev), final_Ts=torch.empty(nb, H, W, device=dev),
                             final_idx=torch.full((nb, H, W), -7777, dtype=torch.int32, device=dev),
                             mask_buf=_guarded(nb * cap, dev) if mask else None)
        sm = o["mask_buf"][1] if mask else None
        lists = dict(B=nb, N=N, img_h=H, img_w=W, planar=1, tile_bins=d["bins"], sorted_ids=d["ids"], capacity=cap,
                     records=records, background=bg, final_Ts=o["final_Ts"], final_idx=o["final_idx"], stage_mask=sm)
        if skip_fwd is None:
            splat._abi_rasterize_fwd(**lists, with_extra=1, out_img=o["out_img"], out_extra=o["out_extra"],
                                     out_alpha=o["out_alpha"], pixels_per_lane=fwd_ppl)
        ran = fwd_ppl or splat._fwd_ppl(nb)
        up = dict(v_out_img=c["v_out"][:nb, ..., :3].permute(0, 3, 1, 2).contiguous().to(dev),
                  v_out_alpha=c["v_alpha"][:nb].contiguous().to(dev), with_extra=int(extra),
                  v_out_extra=c["v_out"][:nb, ..., 3].contiguous().to(dev) if extra else None,
                  stage_mask_ppl=(ran if mask_ppl is None else mask_ppl) if mask else 0, pixels_per_lane=bwd_ppl)
        if dense:
            gr = dict(v_colors=torch.zeros(nb, N, 3, device=dev), v_opacity=torch.zeros(nb, N, 1, device=dev),
                      v_xy=torch.zeros(nb, N, 2, device=dev), v_conic=torch.zeros(nb, N, 3, device=dev),
                      v_extra=torch.zeros(nb, N, 1, device=dev))
            splat._abi_rasterize_bwd(**lists, **up, v_xy=gr["v_xy"], v_conic=gr["v_conic"], v_colors=gr["v_colors"],
                                     v_opacity=gr["v_opacity"], v_extra=gr["v_extra"] if extra else None, grad_stride=0)
        else:
            rec = torch.zeros(nb, N, splat.GRAD_RECORD, device=dev)
            field = lambda k: rec.data_ptr() + 4 * k
            splat._abi_rasterize_bwd(**lists, **up, v_xy=field(4), v_conic=field(6), v_colors=field(0), v_opacity=field(3),
                                     v_extra=field(9) if extra else None, grad_stride=splat.GRAD_RECORD)
            gr = dict(v_colors=rec[..., 0:3], v_opacity=rec[..., 3:4], v_xy=rec[..., 4:6], v_conic=rec[..., 6:9],
                      v_extra=rec[..., 9:10])
        torch.cuda.synchronize()
    finally:
        os.environ.pop("GOL_RASTER_STAGE_MASK", None)
        if old is not None:
            os.environ["GOL_RASTER_STAGE_MASK"] = old
    return dict(o, grads=gr, ran=ran)


def _names(extra):
    return ["v_colors", "v_opacity", "v_xy", "v_conic"] + (["v_extra"] if extra else [])


def _tile_px(c, H, W, b, kind):
    t = LAYOUT[(H, W)].index(kind)
    tiles_x = (W + 15) // 16
    return slice(16 * (t // tiles_x), min(16 * (t // tiles_x) + 16, H)), slice(16 * (t % tiles_x), min(16 * (t % tiles_x) + 16, W)), t


def _assert_structure(c, H, W, nb, o):
    """The lists and pixels the case is meant to contain, read back from what the forward left."""
    fidx, fT, bins = o["final_idx"].cpu(), o["final_Ts"].cpu(), c["bins"]
    for b in range(nb):
        n = (bins[b, :, 1] - bins[b, :, 0]).tolist()
        assert sorted(n) == sorted({"long": 300, "even": 256, "wall": 305, "short130": 130, "short70": 70, "none": 0}[k]
                                   for k in LAYOUT[(H, W)])
        ys, xs, t = _tile_px(c, H, W, b, "long")       # some pixels stop at once, others walk to the end of 300 entries
        assert int(fidx[b, ys, xs].max()) == int(bins[b, t, 1]) - 1 and int(fidx[b, ys, xs].min()) <= int(bins[b, t, 0]) + 1
        ys, xs, t = _tile_px(c, H, W, b, "even")       # the backward's first batch ends with the list: 4 x 64
        assert int(fidx[b, ys, xs].max()) == int(bins[b, t, 1]) - 1 and int(bins[b, t, 1] - bins[b, t, 0]) % 256 == 0
        ys, xs, t = _tile_px(c, H, W, b, "wall")       # every pixel stopped at the fifth entry: the backward starts inside
        assert bool((fidx[b, ys, xs] == int(bins[b, t, 0]) + 3).all())
        assert 1e-4 < float(fT[b, ys, xs].min()) and float(fT[b, ys, xs].max()) < 2e-4
    # the blobs: opacity 1, centred on a pixel centre inside the image -> opacity * exp(-sigma) = 1 there, the cap binds
    ys, xs, t = _tile_px(c, H, W, 0, "long")
    blob = int(c["ids"][0, int(bins[0, t, 0])])
    cx, cy = c["xys"][0, blob].tolist()
    assert cx % 1 == 0.5 and cy % 1 == 0.5 and cx < W and cy < H and float(c["opac"][0, blob]) == 1.0


@pytest.mark.parametrize("extra", [False, True], ids=["rgb", "depth"])
@pytest.mark.parametrize("nb", [1, NV], ids=["1view_4waves", "4views_2waves"])
@pytest.mark.parametrize("H,W", SIZES)
def test_stage_mask_on_equals_off(H, W, nb, extra):
    """Forward outputs bit for bit, gradients up to atomic order: buffer handed over vs GOL_RASTER_STAGE_MASK=0 vs no buffer.
    One view: the forward takes the four-wave layout, writes no masks and the backward must not read any.
    Measured (MI355X): gradients bit-identical between the three variants at every shape -- each Gaussian of these scenes is
    in one tile's list, so every gradient component is one atomic."""
    c = _case(H, W)
    on = _render(c, H, W, nb, extra, mask=True)
    off = _render(c, H, W, nb, extra, mask=True, env="0")
    none = _render(c, H, W, nb, extra, mask=False)
    assert on["ran"] == (1 if nb <= 2 else 2)
    _assert_structure(c, H, W, nb, on)
    busy = torch.zeros(nb, H, W, dtype=torch.bool)
    for b in range(nb):
        for kind in LAYOUT[(H, W)]:
            ys, xs, _ = _tile_px(c, H, W, b, kind)
            busy[b, ys, xs] = kind != "none"
    busy = busy.cuda()
    for other in (off, none):
        for k in ("out_img", "out_extra", "out_alpha", "final_Ts"):
            assert torch.equal(on[k].view(torch.int32), other[k].view(torch.int32)), k
        assert torch.equal(on["final_idx"][busy], other["final_idx"][busy])      # (tiles without entries: not written)
    # the buffer: sentinels around it survive; written only by the two-pixel layout, only inside the lists, only up to the
    # batch of 256 that holds the tile's last final_idx; untouched with the switch off
    cap = c["ids"].shape[1]
    for r, touched in ((on, nb > 2), (off, False)):
        buf, body = r["mask_buf"]
        assert bool((buf[:256] == SENT).all()) and bool((buf[-256:] == SENT).all())
        body = body.view(nb, cap).cpu()
        if not touched:
            assert bool((body == SENT).all())
            continue
        fidx = r["final_idx"].cpu()
        for b in range(nb):
            for kind in LAYOUT[(H, W)]:
                ys, xs, t = _tile_px(c, H, W, b, kind)
                s, e = c["bins"][b, t].tolist()
                if e == s:
                    continue
                last = int(fidx[b, ys, xs].max())
                assert bool((body[b, s:last + 1] < 4).all()), (kind, "unwritten or wide mask inside the walked range")
                staged_end = min(e, s + 256 * ((last - s) // 256 + 1))
                assert bool((body[b, staged_end:e] == SENT).all()), (kind, "byte written past the staged batches")
    errs = {k: (rel_l2(on["grads"][k], off["grads"][k]), rel_l2(on["grads"][k], none["grads"][k])) for k in _names(extra)}
    print({k: tuple("%.1e" % e for e in v) for k, v in errs.items()})
    for k, es in errs.items():
        assert float(off["grads"][k].abs().max()) > 0, k
        assert max(es) < TIGHT, (k, es)
    if not extra:
        assert not bool(on["grads"]["v_extra"].any())


@pytest.mark.parametrize("fwd_ppl,bwd_ppl", [(2, 1), (1, 2), (1, 1)], ids=["fwd2_bwd1", "fwd1_bwd2", "fwd1_bwd1"])
@pytest.mark.parametrize("H,W", SIZES)
def test_differing_layouts_fall_back_to_the_reach_test(H, W, fwd_ppl, bwd_ppl):
    """Four views with the footprints forced apart (and both to one pixel per lane, which the forward does not write
    masks for): the backward is handed the buffer and the forward's layout, must ignore it and match the run without.
    Measured (MI355X): bit-identical."""
    c = _case(H, W)
    on = _render(c, H, W, NV, True, mask=True, fwd_ppl=fwd_ppl, bwd_ppl=bwd_ppl)
    none = _render(c, H, W, NV, True, mask=False, fwd_ppl=fwd_ppl, bwd_ppl=bwd_ppl)
    errs = {k: rel_l2(on["grads"][k], none["grads"][k]) for k in _names(True)}
    print({k: "%.1e" % e for k, e in errs.items()})
    for k, e in errs.items():
        assert float(none["grads"][k].abs().max()) > 0 and e < TIGHT, (k, e)


def test_backward_reads_the_masks_it_is_handed():
    """The reuse path is really taken: with a buffer of zeros in place of the forward's masks (every entry culled for every
    wave) the backward adds nothing, with the switch off the same call computes the gradients."""
    H, W = SIZES[1]
    c = _case(H, W)
    fwd = _render(c, H, W, NV, True, mask=True)
    fwd["mask_buf"][0].zero_()
    zero = _render(c, H, W, NV, True, mask=True, mask_ppl=2, skip_fwd=fwd)
    off = _render(c, H, W, NV, True, mask=True, mask_ppl=2, skip_fwd=fwd, env="0")
    for k in _names(True):
        assert not bool(zero["grads"][k].any()), k
        assert rel_l2(off["grads"][k], c["ref"][True][k]) < TIGHT, k


@pytest.mark.parametrize("extra", [False, True], ids=["rgb", "depth"])
@pytest.mark.parametrize("nb,bwd_ppl", [(1, 0), (NV, 0), (NV, 1)], ids=["1view", "4views", "4views_bwd_4waves"])
@pytest.mark.parametrize("H,W", SIZES)
def test_composite_form_vs_oracle(H, W, nb, bwd_ppl, extra):
    """Packed (masks reused where the layouts allow) and dense gradients against the CPU oracle: non-zero background,
    v_out_alpha set, alpha at the 0.99 cap, pixels stopped at T = 1.1e-4 .. 1.4e-4 (see the module docstring).
    Measured maxima over all parameters (MI355X): packed vs oracle 5.3e-7 (v_extra; v_conic 5.2e-7, v_colors 4.1e-7,
    v_opacity 3.8e-7, v_xy 2.4e-7), dense vs oracle the same, packed vs dense 7.8e-8 (v_xy; 0 elsewhere); final_T against the
    oracle's forward 9.3e-8."""
    c = _case(H, W)
    packed = _render(c, H, W, nb, extra, mask=True, bwd_ppl=bwd_ppl)
    dense = _render(c, H, W, nb, extra, mask=True, bwd_ppl=bwd_ppl, dense=True)
    _assert_structure(c, H, W, nb, packed)
    eT = rel_l2(packed["final_Ts"], c["ref_T"][:nb])
    ref = c["ref"][extra]
    errs = {k: (rel_l2(packed["grads"][k], dense["grads"][k]), rel_l2(packed["grads"][k], ref[k][:nb]),
                rel_l2(dense["grads"][k], ref[k][:nb])) for k in _names(extra)}
    print("final_T %.1e" % eT, {k: tuple("%.1e" % e for e in v) for k, v in errs.items()})
    assert eT < TIGHT
    for k, (pd, po, do) in errs.items():
        assert float(ref[k][:nb].abs().max()) > 0, k
        assert pd < TIGHT, (k, "packed vs dense", pd)
        assert po < TIGHT, (k, "packed vs oracle", po)
        assert do < TIGHT, (k, "dense vs oracle", do)


def test_render_views_fused_staged_and_switched_off_agree():
    """The whole render (gol_render_fwd / _bwd out of one workspace, four views: masks reused), the instrumented pass (one
    ABI call per stage: must reuse them the same way) and GOL_RASTER_STAGE_MASK=0: identical images, leaf gradients up to
    atomic order.  Measured (MI355X): gradients bit-identical."""
    from goliath_amd import _lib, splat
    from scenes import head_scene

    H, W, N = 40, 24, 1500
    views = [head_scene(N, H, W, seed=60 + b, cam_angle=0.4 * b) for b in range(NV)]
    leaves = [torch.stack([v[k] for v in views]).cuda().requires_grad_(True)
              for k in ("means", "scales", "quats", "opacity", "colors")]
    viewmats = torch.stack([v["viewmat"] for v in views]).cuda()
    intrins = torch.tensor([[v["fx"], v["fy"], v["cx"], v["cy"]] for v in views]).cuda()
    g = torch.Generator().manual_seed(3)
    w = [torch.randn(NV, ch, H, W, generator=g).cuda() for ch in (3, 1, 1)]

    def run(timing=False, env=None):
        for x in leaves:
            x.grad = None
        old = os.environ.pop("GOL_RASTER_STAGE_MASK", None)
        if env is not None:
            os.environ["GOL_RASTER_STAGE_MASK"] = env
        _lib.TIMING = [] if timing else None
        try:
            out = splat.render_views(*leaves, viewmats, intrins, H, W, with_depth=True, capacity=1 << 16)
            ((out["render"] * w[0]).sum() + (out["alpha"] * w[1]).sum() + (out["depth_norm"] * w[2]).sum()).backward()
            torch.cuda.synchronize()
        finally:
            _lib.TIMING = None
            os.environ.pop("GOL_RASTER_STAGE_MASK", None)
            if old is not None:
                os.environ["GOL_RASTER_STAGE_MASK"] = old
        return out, [x.grad.clone() for x in leaves]

    base, g0 = run(env="0")
    n = (base["tile_bins"][..., 1] - base["tile_bins"][..., 0])
    assert int(n.max()) > 64 and int(base["n_isect"].max()) <= 1 << 16, n.tolist()
    for kw in (dict(), dict(timing=True)):
        out, g1 = run(**kw)
        for k in ("render", "alpha", "depth_norm"):
            assert torch.equal(out[k], base[k]), (kw, k)
        errs = [rel_l2(a, b) for a, b in zip(g1, g0)]
        print(kw, ["%.1e" % e for e in errs])
        for i, (e, b) in enumerate(zip(errs, g0)):
            assert float(b.abs().max()) > 0 and e < TIGHT, (kw, i, e)
