"""GPU parity of the raster backward after two changes to its visit loop (raster.hip, gol_raster.h, raster_nd.hip):

  * two pixels per lane: the nine cross-lane sums of a visit go through gol_wave_colsum -- only the six plain sums cross the
    rows of 16 lanes, the three x-moments (Mx, Mxx, Mxy) are formed on the column sums of m0 and my, because dx is constant
    down a column of lanes; results in lanes 8 k + 7 and lane 19, one LDS slot write per result lane;
  * one mask per visit: the take decision zeroes raw = opacity e once, alpha = min(cap, raw) and gop = raw v_alpha follow
    without a second select; the moments carry the opacity, the three merges (packed, dense, raster_nd's) negate them instead
    of multiplying by -opacity, and v_opacity is the zeroth moment divided by the opacity.

The scenes, hand-built tile lists and oracle results are those of tests/test_gpu_raster_stage_mask.py (32 x 32 and 24 x 40
images; lists of 300, 256, 130, 70 and 0 entries and the "wall"), imported as tests/test_gpu_raster_sum8.py does and shared
with both.  Gradients are held against the CPU oracle with that file's bar, TIGHT = 5e-6 rel-L2, packed against dense alike.
The forward is not touched: its outputs must hash to tests/golden/raster_sum8_forward.json.

test_column_and_row_takers adds one 16 x 16 tile, one view, lists of at most 8 entries, built to show what a blob that is
symmetric about a pixel hides from a reduction that treats columns and rows differently:
  "vertical"    a thin vertical Gaussian whose takers sit in ONE column (dx is the same in every taker: Mx = dx M0, Mxx =
                dx^2 M0, Mxy = dx My hold exactly, and only one lane column feeds the column sums);
  "horizontal"  a thin horizontal one whose takers sit in ONE pixel row, row 11, of wave 1 (one row of lanes, every column);
  "rotated"     conic b != 0, centred 20 px left of the tile, reaching both waves: large dx of one sign, Mxy far from 0;
  "faint_cap"   one entry of opacity 0.02 (the moments now carry the opacity: v_opacity is a quotient by 0.02) in front of one
                whose opacity e exceeds the cap at its centre (alpha = 0.99 there while gop keeps the uncapped product);
  "all"         the five of them in one list.
For each case the CPU oracle's gradients (oracle.cref.rasterize_backward) are first asserted to be non-zero in every
component that is compared.
"""
import functools
import json
import math

import pytest
import torch

import test_gpu_raster_stage_mask as sm
import test_gpu_raster_sum8 as s8
from scenes import rel_l2

pytestmark = pytest.mark.gpu
TIGHT = sm.TIGHT


@pytest.mark.parametrize("extra", [False, True], ids=["rgb", "depth"])
@pytest.mark.parametrize("ppl", [1, 2], ids=["4waves", "2waves"])
@pytest.mark.parametrize("nb", [1, sm.NV], ids=["1view", "4views"])
@pytest.mark.parametrize("H,W", sm.SIZES)
def test_gradients_vs_oracle_forward_vs_golden(H, W, nb, ppl, extra):
    """Packed and dense backward with the wave layout forced to `ppl`, against the CPU oracle and each other; the forward's
    outputs against the digests of tests/golden/raster_sum8_forward.json.
    Measured maxima over all parameters (MI355X): packed vs oracle 5.3e-7 (v_extra; v_colors 4.8e-7, v_conic 3.9e-7,
    v_opacity 3.5e-7, v_xy 2.4e-7), dense vs oracle the same, packed vs dense 3.8e-8 (v_xy; 0 elsewhere); all digests equal."""
    c = sm._case(H, W)
    packed = sm._render(c, H, W, nb, extra, mask=True, bwd_ppl=ppl)
    dense = sm._render(c, H, W, nb, extra, mask=True, bwd_ppl=ppl, dense=True)
    sm._assert_structure(c, H, W, nb, packed)
    want = json.load(open(s8.GOLDEN))[s8.golden_key(H, W, nb)]
    busy = s8._busy(c, H, W, nb)
    assert s8.forward_digest(packed, busy) == want
    assert s8.forward_digest(dense, busy) == want
    ref = c["ref"][extra]
    errs = {k: (rel_l2(packed["grads"][k], dense["grads"][k]), rel_l2(packed["grads"][k], ref[k][:nb]),
                rel_l2(dense["grads"][k], ref[k][:nb])) for k in sm._names(extra)}
    print({k: tuple("%.1e" % e for e in v) for k, v in errs.items()})
    for k, (pd, po, do) in errs.items():
        assert float(ref[k][:nb].abs().max()) > 0, k
        assert pd < TIGHT, (k, "packed vs dense", pd)
        assert po < TIGHT, (k, "packed vs oracle", po)
        assert do < TIGHT, (k, "dense vs oracle", do)
    if not extra:
        assert not bool(packed["grads"]["v_extra"].any()) and not bool(dense["grads"]["v_extra"].any())


def _axes(s1, s2, theta):
    """Conic (a, b, c) of a Gaussian with standard deviations s1 along (cos theta, sin theta) and s2 across it."""
    c, s = math.cos(theta), math.sin(theta)
    xx, xy, yy = c * c * s1 * s1 + s * s * s2 * s2, c * s * (s1 * s1 - s2 * s2), s * s * s1 * s1 + c * c * s2 * s2
    det = xx * yy - xy * xy
    return [yy / det, -xy / det, xx / det]


#            x      y     conic                      opacity
ENTRIES = {
    "vertical":   (5.3, 7.0, _axes(0.15, 6.0, 0.0), 0.8),        # column 5 (dx = -0.2); a pixel further sigma > 14
    "horizontal": (8.0, 11.7, _axes(6.0, 0.15, 0.0), 0.8),       # row 11 (dy = -0.2), wave 1 of the two-wave layout
    "rotated":    (-20.0, 4.0, _axes(12.0, 3.0, 0.2), 0.9),      # 20 px left of the tile, long axis rising into it
    "faint":      (8.2, 6.4, _axes(3.0, 3.0, 0.0), 0.02),
    "capped":     (10.5, 9.5, _axes(2.0, 2.0, 0.0), 1.0),        # on a pixel centre: opacity e = 1 > 0.99 there
}
CASES = {"vertical": ["vertical"], "horizontal": ["horizontal"], "rotated": ["rotated"], "faint_cap": ["faint", "capped"],
         "all": ["faint", "vertical", "rotated", "horizontal", "capped"]}


def _alpha_map(name):
    x, y, (a, b, c), op = ENTRIES[name]
    pc = torch.arange(16, dtype=torch.float64) + 0.5
    dx, dy = x - pc[None, :], y - pc[:, None]
    return op * torch.exp(-(0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy))


@functools.lru_cache(maxsize=None)
def _tile_case(case):
    """One view, one 16 x 16 tile, the entries of CASES[case] as the tile's list, front to back.  Computed once per case,
    shared by the variants and left unchanged."""
    from oracle import cref

    H = W = 16
    names = CASES[case]
    n = len(names)
    assert n <= 8
    g = torch.Generator().manual_seed(1900 + sorted(CASES).index(case))
    xys = torch.tensor([[ENTRIES[k][0], ENTRIES[k][1]] for k in names], dtype=torch.float32)
    conics = torch.tensor([ENTRIES[k][2] for k in names], dtype=torch.float32)
    opac = torch.tensor([ENTRIES[k][3] for k in names], dtype=torch.float32)
    colors, depths = 0.1 + 0.9 * torch.rand(n, 3, generator=g), 1.0 + torch.rand(n, generator=g)
    ids = torch.arange(n, dtype=torch.int32)
    bins = torch.tensor([[0, n]], dtype=torch.int32)
    v_out = torch.randn(1, H, W, 4, generator=g)
    v_alpha = torch.randn(1, H, W, generator=g)
    bg4 = torch.tensor(sm.BG + (0.0,))
    col4 = torch.cat([colors, depths[:, None]], 1).contiguous()
    _, Ts, idx = cref.rasterize_forward(ids, bins, xys, conics, col4, opac, H, W, 16, bg4)
    ref = {}
    for extra in (False, True):
        vo = v_out[0].clone()
        if not extra:
            vo[..., 3] = 0.0
        r_xy, r_conic, r_col, r_op = cref.rasterize_backward(ids, bins, xys, conics, col4, opac, H, W, 16, bg4, Ts, idx, vo,
                                                             v_alpha[0])
        ref[extra] = dict(v_colors=r_col[None, :, :3], v_opacity=r_op[None], v_xy=r_xy[None], v_conic=r_conic[None],
                          v_extra=r_col[None, :, 3:4])
    one = lambda t: t[None].contiguous()
    return dict(xys=one(xys), conics=one(conics), opac=one(opac), colors=one(colors), depths=one(depths), ids=one(ids),
                bins=one(bins), v_out=v_out, v_alpha=v_alpha, N=n, ref=ref, names=names)


def test_tile_entries_are_what_they_are_meant_to_be():
    """CPU only arithmetic on the entries (no kernel): where alpha >= 1/255 for each of them."""
    reach = {k: _alpha_map(k) >= 1.0 / 255.0 for k in ENTRIES}
    rows = lambda m: sorted(set(torch.nonzero(m)[:, 0].tolist()))
    cols = lambda m: sorted(set(torch.nonzero(m)[:, 1].tolist()))
    assert cols(reach["vertical"]) == [5] and len(rows(reach["vertical"])) == 16           # one column, both waves
    assert rows(reach["horizontal"]) == [11] and len(cols(reach["horizontal"])) == 16      # one row of wave 1, every column
    r = rows(reach["rotated"])
    assert min(r) < 8 <= max(r) and int(reach["rotated"].sum()) >= 32 and ENTRIES["rotated"][2][1] != 0.0
    assert ENTRIES["rotated"][0] == -20.0
    assert int(reach["faint"].sum()) >= 16 and float(_alpha_map("faint").max()) < 0.02
    assert float(_alpha_map("capped")[9, 10]) == 1.0 and int((_alpha_map("capped") > 0.99).sum()) == 1


@pytest.mark.parametrize("extra", [False, True], ids=["rgb", "depth"])
@pytest.mark.parametrize("dense", [False, True], ids=["packed", "dense"])
@pytest.mark.parametrize("ppl", [1, 2], ids=["4waves", "2waves"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_column_and_row_takers(case, ppl, dense, extra):
    """Every entry of every case within TIGHT of the oracle, entry by entry and component group by component group.
    Measured maxima (MI355X): "all" 3.5e-6 (v_opacity; v_xy 1.9e-6, v_conic 8.8e-7, v_colors 5.8e-7), the four other cases
    at most 9.2e-7 (v_conic of "horizontal"); v_extra at most 4.7e-7."""
    c = _tile_case(case)
    ref = c["ref"][extra]
    for k in sm._names(extra):      # on the CPU, before any kernel runs: nothing compared below is a zero of the oracle
        assert bool((ref[k] != 0).all()), (case, k, ref[k])
    o = sm._render(c, 16, 16, 1, extra, mask=True, fwd_ppl=ppl, bwd_ppl=ppl, dense=dense)
    errs = {}
    for k in sm._names(extra):
        got = o["grads"][k].cpu()
        errs[k] = max(rel_l2(got[:, i], ref[k][:, i]) for i in range(c["N"]))
    print(case, {k: "%.1e" % e for k, e in errs.items()})
    for k, e in errs.items():
        assert e < TIGHT, (case, k, e)
    if not extra:
        assert not bool(o["grads"]["v_extra"].any())
