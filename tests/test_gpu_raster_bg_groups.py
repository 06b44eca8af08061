"""GPU parity of the raster forward's empty-run path: a group of G consecutive tiles of one tile row whose lists are all
empty is written by ONE workgroup as whole rows (raster.hip, fill_group), the other workgroups of the group return.

Every output of the grouped path (GOL_RASTER_BG_GROUP = 2, 4, 8) must equal the per-tile path (= 0) BIT for bit on
identical inputs: image, final_T, alpha, raw and normalised depth (0 / 0 = NaN at norm_lo = 0: compared as int32), the
per-tile L1 sums and the loss; final_idx and the sign bytes inside non-empty tiles (elsewhere neither path writes them).
Every output is an interior view of a sentinel-filled buffer and the sentinels must survive.

Small hand-built views (B = 2, 300 Gaussians of 0.3-1 px, at least 4 px inside chosen full tiles, another pattern per
view) at the smallest shapes at which the path can go wrong: a last tile column of 6 px (W % 4 == 2: 8-byte stores), the
16-byte store path, a last tile row of 8 px, 9 tile rows (the tile-row-to-die mapping wraps), partial groups at the right
edge, an odd width (the per-tile path must be taken).  Both wave layouts run every variant: with one pixel per lane (four
waves per tile) the library keeps the per-tile path whatever the variable says, and the equality must hold there too.  The
tile ranges binning produced are read back and the group
structure the case is meant to contain is asserted before anything is compared.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
B, N = 2, 300
BG = (0.3, 0.1, 0.2)
GUARD = 64                      # sentinel elements on either side of every output (keeps 16-byte alignment)
SENT = {torch.float32: -12345.0, torch.int32: -7777, torch.uint8: 0xAB}
GROUPS = (2, 4, 8)

# populated tiles (tx, ty) per view: full 16x16 tiles only
PATTERNS = {
    (40, 70): [[(1, 0), (0, 1)], [(0, 0), (3, 0), (2, 1)]],
    (40, 72): [[(1, 0), (0, 1)], [(0, 0), (3, 0), (2, 1)]],
    (136, 150): [[(1, 0), (4, 1), (8, 3)], [(5, 2), (0, 7), (2, 4), (6, 4)]],
    (24, 69): [[(1, 0)], [(0, 0), (3, 0)]],
}
SIZES = list(PATTERNS)


def _view(g, tiles):
    """Projected attributes of one view: the Gaussians are dealt to `tiles`, centres 4 px inside (3 sigma <= 3 px stays in
    the tile); no tiles: radius 0 everywhere, binning drops every Gaussian."""
    t = torch.tensor(tiles if tiles else [(0, 0)], dtype=torch.float32)[torch.randint(0, max(len(tiles), 1), (N,), generator=g)]
    xys = 16.0 * t + 4.0 + 8.0 * torch.rand(N, 2, generator=g)
    s1, s2 = (0.3 + 0.7 * torch.rand(N, generator=g) for _ in range(2))
    th = math.pi * torch.rand(N, generator=g)
    c, s = torch.cos(th), torch.sin(th)
    xx, xy, yy = c * c * s1 * s1 + s * s * s2 * s2, c * s * (s1 * s1 - s2 * s2), s * s * s1 * s1 + c * c * s2 * s2
    det = xx * yy - xy * xy
    conics = torch.stack([yy / det, -xy / det, xx / det], 1).contiguous()
    radii = torch.ceil(3.0 * torch.maximum(s1, s2)).to(torch.int32)
    if not tiles:
        radii = torch.zeros_like(radii)
    return dict(xys=xys, conics=conics, radii=radii, depths=1.0 + torch.rand(N, generator=g),
                opac=0.2 + 0.7 * torch.rand(N, generator=g), colors=torch.rand(N, 3, generator=g))


@functools.lru_cache(maxsize=None)
def _case(H, W, scene):
    """Lists, records, target and masks of one image size on the GPU: built once, shared by the variants, left unchanged.
    scene "two": both views populated; "void": view 0 has no entries at all."""
    from goliath_amd import splat

    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1000 * H + W + (7 if scene == "void" else 0))
    pats = PATTERNS[(H, W)] if scene == "two" else [[], PATTERNS[(H, W)][1]]
    views = [_view(g, p) for p in pats]
    d = {k: torch.stack([v[k] for v in views]).contiguous().to(dev) for k in views[0]}
    T = splat._tiles(H, W)
    cap = B * N + 64
    ws = splat._Workspace(B, N, T, cap, dev)
    splat._bin_sort(B, N, d["xys"], d["depths"], d["radii"], H, W, ws, d["conics"], d["opac"])
    assert int(ws.n_isect.max()) <= cap
    records = splat._pack_records(B, N, d["xys"], d["conics"], d["colors"], d["depths"], d["opac"])
    target = torch.rand(B, 3, H, W, generator=g)
    target[:, :, ::3, ::2] = torch.tensor(BG)[None, :, None, None]      # exact zeros of the difference over the background
    mask3 = (torch.rand(B, 3, H, W, generator=g) > 0.3).float() * torch.rand(B, 3, H, W, generator=g)
    bins = ws.tile_bins.cpu()
    tx, ty = (W + 15) // 16, (H + 15) // 16
    filled = (bins[..., 1] > bins[..., 0]).view(B, ty, tx)
    tile_px = filled.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W].to(dev)
    return dict(ws=ws, cap=cap, records=records, target=target.to(dev), mask3=mask3.to(dev),
                mask1=mask3[:, :1].contiguous().to(dev), filled=filled, tile_px=tile_px, T=T)


def _groups(filled, G):
    """(view, tile row, list of per-tile 'has entries') of every group; len < G: a partial group at the right edge."""
    Bv, ty, tx = filled.shape
    return [(b, r, filled[b, r, c:c + G].tolist()) for b in range(Bv) for r in range(ty) for c in range(0, tx, G)]


def _assert_structure(c, G, scene):
    tx = c["filled"].shape[2]
    gr = _groups(c["filled"], G)
    has = lambda f: any(f(m) for _, _, m in gr)
    if tx >= G:
        assert has(lambda m: len(m) == G and not any(m)), "no all-empty full group"
    if tx % G:
        assert has(lambda m: len(m) < G and not any(m)), "no all-empty partial group at the right edge"
    assert has(lambda m: not m[0] and any(m[1:])), "no mixed group with an empty leader"
    assert has(lambda m: m[0]), "no group with a non-empty leader"
    per_view = c["filled"].flatten(1).any(1).tolist()
    assert per_view == ([True, True] if scene == "two" else [False, True]), per_view


def _guarded(shape, dtype, dev, guard=GUARD):
    n = math.prod(shape)
    buf = torch.full((n + 2 * guard,), SENT[dtype], dtype=dtype, device=dev)
    return buf, buf[guard:guard + n].view(shape)


def _run(c, H, W, *, l1, extra, norm_lo, ppl, bg=BG, guard=GUARD, graph=False):
    """One forward through the low-level entry into fresh sentinel-filled buffers -> {name: (buffer, view)}."""
    from goliath_amd import splat

    dev = torch.device("cuda")
    o = dict(out_img=_guarded((B, 3, H, W), torch.float32, dev, guard), final_Ts=_guarded((B, H, W), torch.float32, dev, guard),
             final_idx=_guarded((B, H, W), torch.int32, dev), out_alpha=_guarded((B, H, W), torch.float32, dev, guard))
    if extra:
        o["out_extra"] = _guarded((B, H, W), torch.float32, dev, guard)
        o["out_extra_norm"] = _guarded((B, H, W), torch.float32, dev, guard)
    kw = {}
    if l1 != "none":
        o["l1_sign"] = _guarded((B, H, W), torch.uint8, dev)
        o["l1_partial"] = _guarded((B, c["T"]), torch.float32, dev)
        o["l1_out"] = _guarded((1,), torch.float32, dev)
        kw = dict(l1_target=c["target"], l1_scale=1.0 / (B * 3 * H * W))
        if l1 != "target":
            kw.update(l1_mask=c["mask1"] if l1 == "mask1" else c["mask3"], l1_mask_c=1 if l1 == "mask1" else 3)
    ws, bgt = c["ws"], torch.tensor(bg, device=dev)
    call = lambda: splat._abi_rasterize_fwd(
        B=B, N=N, img_h=H, img_w=W, planar=1, tile_bins=ws.tile_bins, sorted_ids=ws.sorted_ids, capacity=c["cap"],
        records=c["records"], with_extra=int(extra), background=bgt, norm_lo=norm_lo, pixels_per_lane=ppl,
        **{k: v[1] for k, v in o.items()}, **kw)
    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            call()
        for buf, _ in o.values():           # the replay alone must produce the outputs
            buf.fill_(SENT[buf.dtype])
        gr.replay()
    else:
        call()
    torch.cuda.synchronize()
    return o


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(c, base, got, tag, guard=GUARD):
    for k, (buf, v) in got.items():
        gd = guard if k in ("out_img", "final_Ts", "out_alpha", "out_extra", "out_extra_norm") else GUARD
        s = SENT[buf.dtype]
        assert bool((buf[:gd] == s).all()) and bool((buf[gd + v.numel():] == s).all()), (tag, k, "sentinel overwritten")
        a, b = _bits(base[k][1]), _bits(v)
        if k in ("final_idx", "l1_sign"):
            a, b = a[c["tile_px"]], b[c["tile_px"]]
        assert torch.equal(a, b), (tag, k, int((a != b).sum()))


L1 = ["none", "target", "mask1", "mask3"]
VARIANTS = [(l1, extra, lo, ppl) for l1 in L1 for extra, lo in ((False, 0.05), (True, 0.05), (True, 0.0)) for ppl in (1, 2)]


@pytest.mark.parametrize("scene", ["two", "void"])
@pytest.mark.parametrize("l1,extra,norm_lo,ppl", VARIANTS,
                         ids=["%s-%s-lo%g-ppl%d" % (l, "extra" if e else "rgb", lo, p) for l, e, lo, p in VARIANTS])
@pytest.mark.parametrize("H,W", SIZES)
def test_grouped_equals_per_tile(monkeypatch, H, W, l1, extra, norm_lo, ppl, scene):
    c = _case(H, W, scene)
    for G in GROUPS:
        if W % 2 == 0:
            _assert_structure(c, G, scene)
    v = dict(l1=l1, extra=extra, norm_lo=norm_lo, ppl=ppl)
    monkeypatch.setenv("GOL_RASTER_BG_GROUP", "0")
    base = _run(c, H, W, **v)
    _assert_same(c, base, base, "G=0")          # the per-tile path keeps the sentinels too
    if extra and norm_lo == 0.0:
        assert bool(torch.isnan(base["out_extra_norm"][1]).any())       # the 0 / 0 of empty pixels is really there
    for G in GROUPS:
        monkeypatch.setenv("GOL_RASTER_BG_GROUP", str(G))
        _assert_same(c, base, _run(c, H, W, **v), "G=%d" % G)


@pytest.mark.parametrize("bg", [BG, (0.0, 0.0, 0.0)], ids=["bg", "black"])
@pytest.mark.parametrize("H,W", SIZES)
def test_empty_groups_closed_form(monkeypatch, H, W, bg):
    """Default group size (variable unset): in all-empty groups the image is the background exactly, alpha 0, final_T 1."""
    c = _case(H, W, "two")
    monkeypatch.delenv("GOL_RASTER_BG_GROUP", raising=False)
    o = _run(c, H, W, l1="mask1", extra=True, norm_lo=0.05, ppl=2, bg=bg)
    _assert_same(c, o, o, "default")
    G, seen = 4, 0
    tx = c["filled"].shape[2]
    for b in range(B):
        for r in range(c["filled"].shape[1]):
            for c0 in range(0, tx, G):
                if bool(c["filled"][b, r, c0:c0 + G].any()):
                    continue
                ys, xs = slice(16 * r, min(16 * r + 16, H)), slice(16 * c0, min(16 * (c0 + G), W))
                seen += 1
                for ch in range(3):
                    assert bool((o["out_img"][1][b, ch, ys, xs] == torch.tensor(bg[ch]).float().item()).all())
                assert bool((o["out_alpha"][1][b, ys, xs] == 0).all())
                assert bool((o["final_Ts"][1][b, ys, xs] == 1).all())
                assert bool((o["out_extra"][1][b, ys, xs] == 0).all()) and bool((o["out_extra_norm"][1][b, ys, xs] == 0).all())
    assert seen >= 2


@pytest.mark.parametrize("guard", [66, 65], ids=["8-byte-base", "4-byte-base"])
def test_unaligned_planes(monkeypatch, guard):
    """Planes that start 8 bytes off a 16-byte boundary take the 8-byte stores at W % 4 == 0; 4 bytes off, the per-tile path."""
    H, W = 40, 72
    c = _case(H, W, "two")
    v = dict(l1="mask3", extra=True, norm_lo=0.0, ppl=2, guard=guard)
    monkeypatch.setenv("GOL_RASTER_BG_GROUP", "0")
    base = _run(c, H, W, **v)
    monkeypatch.setenv("GOL_RASTER_BG_GROUP", "4")
    _assert_same(c, base, _run(c, H, W, **v), "guard=%d" % guard, guard)


@pytest.mark.parametrize("H,W", [(40, 70), (136, 150)])
def test_graph_replay(monkeypatch, H, W):
    c = _case(H, W, "two")
    v = dict(l1="mask1", extra=True, norm_lo=0.0, ppl=2)
    monkeypatch.setenv("GOL_RASTER_BG_GROUP", "0")
    base = _run(c, H, W, **v)
    monkeypatch.setenv("GOL_RASTER_BG_GROUP", "4")
    _assert_same(c, base, _run(c, H, W, graph=True, **v), "graph")
