"""GPU: gol_ssim_fwd/bwd (goliath_amd.losses.ssim_image / rgb_ssim) vs the reference-generated golden vectors and,
at the bench's image size, vs the oracle (rel-L2 <= 1e-4 on the gradient, 1e-5 absolute on the value).

The cases of tests/ssim_cases.py (strip walk, uneven strips, padded XCD bands, images under the window, every mask kind,
near-flat bright images) are judged per pixel against the oracle in float64, by a bar RELATIVE to the distance of the
oracle's own float32 run from float64 on the same inputs: the kernel may be 4x as far (another rounding chain of the same
length: separable 11 + 11 taps against 121, a 1-ulp rcp against a division, a block reduction against a linear one), not
more.  tests/test_ssim_cases.py checks on the CPU that the cases reach those branches and that the pair is usable."""
import math

import pytest
import torch

import ssim_cases as sc
from scenes import rel_l2
from test_oracle_ssim import load_cases

pytestmark = pytest.mark.gpu


def test_ssim_matches_reference_golden():
    from goliath_amd import losses

    for tag, c in load_cases().items():
        pred = c["pred"].cuda().requires_grad_(True)
        mask = c["mask"].cuda() if "mask" in c else None
        val = losses.ssim_image(pred, c["target"].cuda(), mask)
        (grad,) = torch.autograd.grad(val, pred)
        assert abs(float(val) - float(c["value"])) < 1e-5, tag
        assert rel_l2(grad, c["grad"]) < 1e-5, tag   # measured 1.0e-6


def test_rgb_ssim_full_size_vs_oracle():
    from goliath_amd import losses
    from oracle import ssim_ref

    torch.manual_seed(0)
    B, C, H, W = 1, 3, 2048, 1334
    target = torch.rand(B, C, H, W)
    pred = (target + 0.1 * torch.randn(B, C, H, W)).requires_grad_(True)
    mask = (torch.rand(B, 1, H, W) > 0.2).float()
    ref = ssim_ref.rgb_ssim(pred, target, mask)
    (g_ref,) = torch.autograd.grad(ref, pred)
    p = pred.detach().cuda().requires_grad_(True)
    got = losses.rgb_ssim({"rendered_rgb": p}, {"image": target.cuda(), "image_mask": mask.cuda()})
    (g_got,) = torch.autograd.grad(got, p)
    assert abs(float(got) - float(ref)) < 1e-5
    assert rel_l2(g_got, g_ref) < 2e-5   # measured 1.8e-6
    # normalize_mask=False route and the unmasked mean
    got2 = losses.rgb_ssim({"rendered_rgb": p}, {"image": target.cuda(), "image_mask": mask.cuda()}, normalize_mask=False)
    assert abs(float(got2) - float(ssim_ref.rgb_ssim(pred, target, mask, normalize_mask=False))) < 1e-5
    got3 = losses.rgb_ssim({"rendered_rgb": p}, {"image": target.cuda()})
    assert abs(float(got3) - float(ssim_ref.rgb_ssim(pred, target))) < 1e-5


def test_ssim_identical_images_and_no_grad():
    from goliath_amd import losses

    x = torch.rand(2, 3, 50, 37, device="cuda")
    assert abs(float(losses.ssim_image(x, x)) - 1.0) < 1e-6
    with torch.no_grad():
        assert float(losses.ssim_image(x, x.flip(-1))) < 1.0


def _hip(tag, grad=True):
    """g * ssim_image of a case on the GPU and its gradient (both moved to the CPU)."""
    from goliath_amd import losses

    pred, target, mask, g = sc.make(tag)
    p = pred.cuda().requires_grad_(grad)
    val = g * losses.ssim_image(p, target.cuda(), None if mask is None else mask.cuda())
    if not grad:
        return val.detach().cpu(), None
    (G,) = torch.autograd.grad(val, p)
    return val.detach().cpu(), G.cpu()


@pytest.mark.parametrize("tag", sc.TAGS)
def test_ssim_cases_per_pixel_vs_float64(tag):
    """Value and per-pixel gradient of every case against the float64 oracle, by the 4x rule (module docstring).

    Measured on the MI355X, e_hip / e_ref: noise cases 0.39 ... 1.09 (worst: 5x7_bc; 1x1: 1.00, the same error as the
    oracle's float32 run), flat cases 0.31 ... 0.46 (worst: 260x390_flat) -- where float32 cancels (flat: e_ref 4e-4 ...
    5e-4 of max |grad|) the kernel is closer to float64 than the oracle's float32 run, in value too (|v - v64| 3e-6 ... 7e-6
    against 3e-5 ... 7e-5).

    [1x1] failed this bar (e_hip 3.93e-07 against e_ref 4.73e-08, ratio 8.3) until make_window() of csrc/ssim.hip
    normalised by the correctly rounded float32 sum, as the reference's gauss.sum() does: its serial float32 sum was 1 ulp
    low, 8 of the 11 weights 1 ulp high.  The other cases passed with that window, but carried its error: rel-L2 of the
    gradient 8.2e-07 -> 6.4e-07 at 260x390, 2.3e-04 -> 1.2e-04 at 260x390_flat.  (A one-pixel maximum remains a single
    draw of each chain: over 4000 random 1 x 1 images the kernel is more than 4x the oracle's float32 run in 14 % and the
    oracle more than 4x the kernel in 16 %; at this case's draw the two now give the same gradient.)"""
    v_hip, G_hip = _hip(tag)
    v32, G32 = sc.oracle(tag, torch.float32)
    v64, G64 = sc.oracle(tag, torch.float64)
    assert bool(torch.isfinite(v_hip)) and bool(torch.isfinite(G_hip).all()), tag
    if sc.BY_TAG[tag][5] == "zero":        # clamp(min=1) denominator: exactly 0, value and gradient (the oracle's are, too)
        assert float(v_hip) == 0.0 and not G_hip.any() and v64 == 0.0 and not G64.any()
        return
    e_ref, e_hip = sc.max_err(G32, G64), sc.max_err(G_hip, G64)
    d_ref, d_hip = abs(v32 - v64), abs(float(v_hip) - v64)
    r = rel_l2(G_hip, G64)
    print(f"{tag}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {e_hip / e_ref:.3f} | value: hip {d_hip:.3e} ref {d_ref:.3e} "
          f"allowed {4 * d_ref + 2.0 ** -23 * abs(v64):.3e} | rel_l2 {r:.3e}")
    assert math.isfinite(r)
    # measured worst e_hip / e_ref: noise 1.09 (5x7_bc), flat 0.46 (260x390_flat)
    assert e_hip <= 4 * e_ref, (tag, e_hip, e_ref)
    assert d_hip <= 4 * d_ref + 2.0 ** -23 * abs(v64), (tag, d_hip, d_ref)


def test_ssim_forward_localised_per_tile():
    """The scalar value cannot say where a forward error is: at 260 x 390 (9 x 13 tiles, every strip length, the padded
    band) each tile in turn is the mask, and the masked mean is held against the float64 oracle's map over the same pixels,
    by the 4x rule against the float32 oracle's map."""
    from goliath_amd import losses

    tag = "260x390"
    pred, target, _, _ = sc.make(tag)
    m32, m64 = sc.oracle_map(tag, torch.float32), sc.oracle_map(tag, torch.float64)
    part = sc.partition(260, 390)
    p, t = pred.cuda(), target.cuda()
    mask = torch.zeros(1, 1, 260, 390, device="cuda")
    got = []
    with torch.no_grad():
        for ty in range(part["tiles_y"]):
            for tx in range(part["tiles_x"]):
                mask.zero_()
                mask[..., ty * sc.TILE:(ty + 1) * sc.TILE, tx * sc.TILE:(tx + 1) * sc.TILE] = 1.0
                got.append(losses.ssim_image(p, t, mask))
    got = torch.stack(got).cpu().double().reshape(part["tiles_y"], part["tiles_x"])
    assert bool(torch.isfinite(got).all())
    over = []                                        # (|hip - f64| / allowed, tile row, tile column)
    for ty in range(part["tiles_y"]):
        for tx in range(part["tiles_x"]):
            sl = (0, 0, slice(ty * sc.TILE, (ty + 1) * sc.TILE), slice(tx * sc.TILE, (tx + 1) * sc.TILE))
            n = m64[sl].numel()
            w64 = float(m64[sl].sum() / n)
            w32 = float(m32[sl].sum() / n)          # float32 sum and division, as the oracle's masked mean
            d_ref, d_hip = abs(w32 - w64), abs(float(got[ty, tx]) - w64)
            over.append((d_hip / (4 * d_ref + 2.0 ** -23 * abs(w64)), ty, tx))
    bad = [o for o in over if not o[0] <= 1.0]
    print(f"forward localisation: worst |hip - f64| / allowed = {max(over)[0]:.3f} at tile {max(over)[1:]}; "
          f"{len(bad)} of {len(over)} tiles over the bar: {[(ty, tx) for _, ty, tx in bad][:20]}")
    assert not bad, sorted(bad, reverse=True)[:8]    # measured: worst 0.44 of the allowance


def test_ssim_no_grad_value_is_the_grad_value_bitwise():
    """dmap == nullptr (no gradient wanted) must not change the value."""
    for tag in ("260x390", "260x390_flat"):
        v_grad, _ = _hip(tag, grad=True)
        v_nograd, _ = _hip(tag, grad=False)
        assert torch.equal(v_grad, v_nograd), (tag, float(v_grad), float(v_nograd))


def test_ssim_non_contiguous_pred():
    """pred is a crop of a larger leaf: the gradient on the leaf is that of the contiguous run inside the crop, 0 outside."""
    from goliath_amd import losses

    pred, target, mask, g = sc.make("40x200_bc")
    big = torch.rand(2, 3, 50, 215, generator=torch.Generator().manual_seed(5))
    big[:, :, 3:43, 5:205] = pred
    leaf = big.cuda().requires_grad_(True)
    crop = leaf[:, :, 3:43, 5:205]
    assert not crop.is_contiguous()
    val = g * losses.ssim_image(crop, target.cuda(), mask.cuda())
    (G,) = torch.autograd.grad(val, leaf)
    v_c, G_c = _hip("40x200_bc")
    assert torch.equal(val.detach().cpu(), v_c)
    assert torch.equal(G[:, :, 3:43, 5:205].cpu(), G_c) and bool(G_c.any())
    G[:, :, 3:43, 5:205] = 0
    assert not G.any()                                            # nothing outside the crop


def test_ssim_is_deterministic():
    """Per-workgroup partial sums added by the caller, no atomics: two runs are bitwise equal (forward and backward)."""
    for tag in ("260x390", "40x200_bc"):
        v0, G0 = _hip(tag)
        v1, G1 = _hip(tag)
        assert torch.equal(v0, v1) and torch.equal(G0, G1), tag
