"""GPU parity of the raster backward after two changes to its visit loop (raster.hip):

  * the first eight of a visit's cross-lane sums go through one 8-way reduction (gol_wave_sum8: results in lanes 8 k + 7,
    one LDS slot write per result lane) instead of two 4-way ones;
  * the "this wave reduced entry t" flags are collected as a wave-uniform 64-bit mask and stored once per batch, zeros
    included, into a row that is no longer cleared per batch.

The scenes, hand-built tile lists and oracle results are those of tests/test_gpu_raster_stage_mask.py (32 x 32 and 24 x 40
images; lists of 300, 256, 130, 70 and 0 entries and the "wall"), imported from there and shared with it.  Gradients are held
against the CPU oracle with that file's bar, TIGHT = 5e-6 rel-L2 (the bar of tests/test_gpu_raster_merge.py).  The forward
is not touched: its outputs must hash to what the commit before the change wrote (tests/golden/raster_sum8_forward.json:
sha256 over the pixels of the tiles that have entries).

test_touched_mask_last_bit builds one 16 x 16 tile with a list of 128 entries, two batches of exactly 64: the list's first
entry (slot 63 of the second batch) reaches only the pixels of wave 1, its last entry (slot 0 of the first batch) only those
of wave 0, the 126 between them lie far outside the tile.  Wave 1's mask of the second batch is bit 63 alone and wave 0's is
empty while its row still holds the first batch's flag of slot 0: a flag that is lost, or one that survives its batch, puts a
gradient on the wrong Gaussian.
"""
import functools
import hashlib
import json
import os

import pytest
import torch

import test_gpu_raster_stage_mask as sm
from scenes import rel_l2

pytestmark = pytest.mark.gpu
TIGHT = sm.TIGHT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_sum8_forward.json")
FWD_OUTPUTS = ("out_img", "out_extra", "out_alpha", "final_Ts", "final_idx")


def _busy(c, H, W, nb):
    busy = torch.zeros(nb, H, W, dtype=torch.bool)
    for b in range(nb):
        for kind in sm.LAYOUT[(H, W)]:
            ys, xs, _ = sm._tile_px(c, H, W, b, kind)
            busy[b, ys, xs] = kind != "none"
    return busy


def forward_digest(o, busy):
    """sha256 over the forward's outputs at the pixels of tiles with entries (the others are not all written)."""
    h = hashlib.sha256()
    for k in FWD_OUTPUTS:
        t = o[k].cpu()
        m = busy[:, None].expand_as(t) if t.dim() == 4 else busy
        h.update(t[m].contiguous().numpy().tobytes())
    return h.hexdigest()


def golden_key(H, W, nb):
    return "%dx%d_%dviews" % (H, W, nb)


@pytest.mark.parametrize("extra", [False, True], ids=["rgb", "depth"])
@pytest.mark.parametrize("ppl", [1, 2], ids=["4waves", "2waves"])
@pytest.mark.parametrize("nb", [1, sm.NV], ids=["1view", "4views"])
@pytest.mark.parametrize("H,W", sm.SIZES)
def test_gradients_vs_oracle_forward_vs_parent(H, W, nb, ppl, extra):
    """Packed and dense backward with the wave layout forced to `ppl`, against the CPU oracle and each other; the forward's
    outputs against the digests taken before the change.
    Measured maxima over all parameters (MI355X): packed vs oracle 5.3e-7 (v_extra; v_conic 5.0e-7, v_colors 4.1e-7,
    v_opacity 3.9e-7, v_xy 2.4e-7), dense vs oracle the same, packed vs dense 8.1e-8 (v_xy; 0 elsewhere); all digests equal."""
    c = sm._case(H, W)
    packed = sm._render(c, H, W, nb, extra, mask=True, bwd_ppl=ppl)
    dense = sm._render(c, H, W, nb, extra, mask=True, bwd_ppl=ppl, dense=True)
    sm._assert_structure(c, H, W, nb, packed)
    want = json.load(open(GOLDEN))[golden_key(H, W, nb)]
    busy = _busy(c, H, W, nb)
    assert forward_digest(packed, busy) == want
    assert forward_digest(dense, busy) == want
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


@functools.lru_cache(maxsize=None)
def _two_batch_case(ppl):
    """One view, one 16 x 16 tile, 128 list entries (see the module docstring).  Wave 1 owns pixel rows 8-15 with two pixels
    per lane and columns 8-15 of rows 0-7 with one; wave 0 owns rows 0-7 / columns 0-7 of rows 0-7.  Computed once per
    layout, shared by the variants and left unchanged."""
    from oracle import cref

    H = W = 16
    n = 128
    first_xy, last_xy = ((8.0, 12.0), (8.0, 4.0)) if ppl == 2 else ((12.0, 4.0), (4.0, 4.0))
    g = torch.Generator().manual_seed(640 + ppl)
    xys = torch.tensor([[300.0, 300.0]] * n)
    xys[0], xys[n - 1] = torch.tensor(first_xy), torch.tensor(last_xy)
    conics = torch.tensor([[4.0, 0.0, 4.0]] * n)       # isotropic, 0.5 px: alpha >= 1/255 within 1.7 px of the centre
    opac = torch.full((n,), 0.8)
    colors, depths = torch.rand(n, 3, generator=g), 1.0 + torch.rand(n, generator=g)
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
                bins=one(bins), v_out=v_out, v_alpha=v_alpha, N=n, ref=ref, idx=idx)


@pytest.mark.parametrize("extra", [False, True], ids=["rgb", "depth"])
@pytest.mark.parametrize("dense", [False, True], ids=["packed", "dense"])
@pytest.mark.parametrize("ppl", [1, 2], ids=["4waves", "2waves"])
def test_touched_mask_last_bit(ppl, dense, extra):
    """Measured (MI355X): the two taken Gaussians within 2.6e-7 of the oracle (v_opacity; v_conic 2.0e-7, v_xy 1.4e-7,
    v_extra 1.1e-7, v_colors 9.4e-8), the 126 others exactly zero."""
    c = _two_batch_case(ppl)
    n = c["N"]
    # the case is what it is meant to be: the last entry is some pixel's final one (the first batch ends on it), taken by
    # wave 0's pixels only; the first entry is final for pixels of wave 1 only
    wave = torch.zeros(16, 16, dtype=torch.int64)
    if ppl == 2:
        wave[8:] = 1
    else:
        wave[:8, 8:], wave[8:, :8], wave[8:, 8:] = 1, 2, 3
    pc = torch.arange(16, dtype=torch.float32) + 0.5
    for i, w in ((0, 1), (n - 1, 0)):
        cx, cy = c["xys"][0, i].tolist()
        alpha = 0.8 * torch.exp(-2.0 * ((pc[None, :] - cx) ** 2 + (pc[:, None] - cy) ** 2))
        reach = alpha >= 1.0 / 255.0
        assert int(reach.sum()) >= 4 and bool((wave[reach] == w).all()), (i, w)
    idx = c["idx"].view(16, 16)
    assert int(idx.max()) == n - 1 and bool((wave[idx == n - 1] == 0).all())
    o = sm._render(c, 16, 16, 1, extra, mask=True, fwd_ppl=ppl, bwd_ppl=ppl, dense=dense)
    ref = c["ref"][extra]
    taken = [0, n - 1]
    errs = {}
    for k in sm._names(extra):
        got = o["grads"][k].cpu()
        assert not bool(got[:, 1:n - 1].any()), (k, "gradient on a Gaussian that no pixel takes")
        assert float(ref[k][:, 0].abs().max()) > 0 and float(ref[k][:, n - 1].abs().max()) > 0, k
        errs[k] = max(rel_l2(got[:, i], ref[k][:, i]) for i in taken)
    print({k: "%.1e" % e for k, e in errs.items()})
    for k, e in errs.items():
        assert e < TIGHT, (k, e)
