"""GPU parity: fused masked L1 image loss vs the reference expression (ca_code/loss/__init__.py:411)."""
import math

import pytest
import torch

from scenes import rel_l2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,mask_c", [((2, 3, 64, 52), 1), ((1, 3, 33, 17), 3), ((2, 3, 40, 40), 0)])
def test_l1_image_matches_torch(shape, mask_c):
    from goliath_amd import losses

    g = torch.Generator().manual_seed(0)
    pred = torch.rand(shape, generator=g).cuda().requires_grad_(True)
    tgt = torch.rand(shape, generator=g).cuda()
    mask = None if mask_c == 0 else (torch.rand(shape[0], mask_c, *shape[2:], generator=g) > 0.3).float().cuda()
    ref_in = pred.detach().clone().requires_grad_(True)
    ref = ((ref_in - tgt) * (mask if mask is not None else 1.0)).abs().mean()
    out = losses.l1_image(pred, tgt, mask)
    assert abs(float(out) - float(ref)) < 1e-6 * max(1.0, abs(float(ref)))
    (2.5 * ref).backward()
    (2.5 * out).backward()
    assert rel_l2(pred.grad, ref_in.grad) < 1e-6
    d = {"rendered_rgb": pred.detach()}
    t = {"image": tgt}
    if mask is not None:
        t["image_mask"] = mask
    assert abs(float(losses.rgb_l1(d, t)) - float(ref)) < 1e-6


def _l1_case(shape, mask_kind, seed):
    """pred, target, mask (CPU float32): ~1 % of the pixels of pred equal target (the kink: gradient exactly 0 there)."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    pred, tgt = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    same = torch.rand(shape, generator=g) < 0.01
    pred = torch.where(same, tgt, pred)
    if mask_kind == "none":
        mask = None
    elif mask_kind == "zero":
        mask = torch.zeros(B, 1, H, W)
    elif mask_kind == "frac1":
        mask = (torch.rand(B, 1, H, W, generator=g) > 0.3).float() * torch.rand(B, 1, H, W, generator=g)
    else:
        assert mask_kind == "bc"
        mask = (torch.rand(B, C, H, W, generator=g) > 0.3).float()
    return pred, tgt, mask, same


# gol_l1_blocks caps the grid at 64 workgroups x 1024 elements x 4: a plane of more than 262144 elements takes a second
# grid-stride trip.  512 x 516 = 264192 (HW % 4 == 0: vector path); 513 x 513 = 263169 (odd: the scalar path in every
# workgroup, and the second plane starts at an odd element offset).
L1_CASES = [((1, 1, 512, 516), "none"), ((1, 1, 512, 516), "frac1"), ((1, 2, 513, 513), "none"),
            ((1, 2, 513, 513), "frac1"), ((1, 2, 513, 513), "zero"), ((2, 3, 33, 17), "bc")]


@pytest.mark.parametrize("shape,mask_kind", L1_CASES, ids=[f"{'x'.join(map(str, s))}-{m}" for s, m in L1_CASES])
def test_l1_image_vs_float64(shape, mask_kind):
    from goliath_amd import _lib, losses

    HW = shape[2] * shape[3]
    if HW > 2048:
        assert HW > _lib.load().gol_l1_blocks(HW) * 4096 and _lib.load().gol_l1_blocks(HW) == 64      # second trip
    pred, tgt, mask, same = _l1_case(shape, mask_kind, seed=sum(shape) + len(mask_kind))
    assert 0 < int(same.sum()) and float(same.float().mean()) < 0.02

    def ref(dtype):
        p = pred.to(dtype).requires_grad_(True)
        v = 2.5 * ((p - tgt.to(dtype)) * (1.0 if mask is None else mask.to(dtype))).abs().mean()
        (gr,) = torch.autograd.grad(v, p)
        return float(v.detach()), gr

    v64, G64 = ref(torch.float64)
    v32, _ = ref(torch.float32)
    p = pred.cuda().requires_grad_(True)
    out = 2.5 * losses.l1_image(p, tgt.cuda(), None if mask is None else mask.cuda())
    (G,) = torch.autograd.grad(out, p)
    G, v_hip = G.cpu(), float(out.detach())
    assert bool(torch.isfinite(G).all()) and math.isfinite(v_hip)
    # gradient sign * m * g / n: no rounding beyond the multiplies -> within 2 ulp of the float64 result rounded to
    # float32, the same sign (and zero) pattern
    want = G64.float()
    nz = want != 0
    ulps = (G[nz].view(torch.int32).long() - want[nz].view(torch.int32).long()).abs()
    d_ref, d_hip = abs(v32 - v64), abs(v_hip - v64)
    print(f"l1 {shape} {mask_kind}: max ulp {int(ulps.max()) if ulps.numel() else 0} | value: hip {d_hip:.3e} ref "
          f"{d_ref:.3e} allowed {4 * d_ref + 2.0 ** -23 * abs(v64):.3e} | signs differ at "
          f"{int((torch.sign(G) != torch.sign(want)).sum())} of {G.numel()}")
    assert torch.equal(torch.sign(G), torch.sign(want))
    assert not G[same].any()
    if mask_kind == "zero":
        assert not G.any() and v_hip == 0.0 and v64 == 0.0
    assert ulps.numel() == 0 or int(ulps.max()) <= 2       # measured: 0 without a mask, 1 with fractional weights
    assert d_hip <= 4 * d_ref + 2.0 ** -23 * abs(v64), (d_hip, d_ref)


@pytest.mark.parametrize("mask_c", [0, 1, 3])
def test_l1_fused_into_the_raster_equals_the_standalone_loss(mask_c):
    """render_views(l1_target=...) -- the loss in the raster epilogue, its gradient carried by the raster backward -- is the
    same function as losses.l1_image on the rendered image: value and every input gradient, alone and next to a second
    consumer of the image."""
    from goliath_amd import losses, splat
    from scenes import head_scene

    H, W, N, B = 150, 130, 3000, 2
    views = [head_scene(N, H, W, seed=30 + b, cam_angle=0.3 * b) for b in range(B)]
    g = torch.Generator().manual_seed(mask_c)
    target = torch.rand(B, 3, H, W, generator=g).cuda()
    mask = (torch.rand(B, mask_c, H, W, generator=g) > 0.3).float().cuda() if mask_c else None

    def leaves():
        d = {k: torch.stack([v[k] for v in views]).cuda().requires_grad_(True) for k in
             ("means", "scales", "quats", "opacity", "colors")}
        d["viewmats"] = torch.stack([v["viewmat"] for v in views]).cuda()
        d["intrins"] = torch.tensor([[v["fx"], v["fy"], v["cx"], v["cy"]] for v in views]).cuda()
        return d

    for extra in (False, True):
        a, b_ = leaves(), leaves()
        out = splat.render_views(**a, img_h=H, img_w=W, l1_target=target, l1_mask=mask)
        ref = splat.render_views(**b_, img_h=H, img_w=W)
        l_ref = losses.l1_image(ref["render"], target, mask)
        assert abs(float(out["l1_loss"]) - float(l_ref)) < 1e-6 * max(1.0, abs(float(l_ref)))
        assert torch.equal(out["render"], ref["render"])
        la, lb = 3.0 * out["l1_loss"], 3.0 * l_ref
        if extra:  # the image also feeds another term: both gradients must add up
            la, lb = la + (out["render"] ** 2).mean(), lb + (ref["render"] ** 2).mean()
        la.backward()
        lb.backward()
        for k in ("means", "scales", "quats", "opacity", "colors"):
            assert rel_l2(a[k].grad, b_[k].grad) < 1e-5, (k, extra, rel_l2(a[k].grad, b_[k].grad))
