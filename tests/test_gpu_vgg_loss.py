"""GPU: the masked VGG loss of goliath_amd.perceptual (reduced widths, tests/vgg_cases.py:loss_case) against its float64 twin,
with every layer forced onto the fused operator and with the committed dispatch table, through the drop-in, and with a
target that requires grad.

Bound: 3 x the fp32 CPU twin's own relative deviation from float64 on the same inputs, plus 1e-6 -- two fp32 summation
orders differ from float64 independently, and the tap losses add five such terms.  The seed keeps the fp32 paths on the
float64 twin's side of every ReLU and pool decision (asserted on the CPU in tests/test_vgg_cases.py)."""
import functools
import types

import pytest
import torch

import vgg_cases as vc
from scenes import rel_l2

pytestmark = pytest.mark.gpu


def _twin(dtype, target_grad=False):
    from goliath_amd import perceptual

    feats, x, y, mask = vc.loss_case(vc.LOSS_SEED)
    x = x.to(dtype).requires_grad_(True)
    y = y.to(dtype).requires_grad_(target_grad)
    loss = perceptual.vgg_loss_torch(feats, x, y, mask.to(dtype))
    grads = torch.autograd.grad(loss, [x, y] if target_grad else [x])
    return loss.detach(), grads


@functools.lru_cache(maxsize=None)
def _reference(target_grad=False):
    """float64 loss and gradients, and the bounds 3 x (fp32 CPU twin's deviation) + 1e-6 for the loss and each gradient."""
    l64, g64 = _twin(torch.float64, target_grad)
    l32, g32 = _twin(torch.float32, target_grad)
    dev = [abs(float(l32) - float(l64)) / abs(float(l64))] + [rel_l2(a, b) for a, b in zip(g32, g64)]
    print("fp32 CPU twin against float64:", dev)
    return l64, g64, [3.0 * d + 1e-6 for d in dev]


def _gpu_case():
    feats, x, y, mask = vc.loss_case(vc.LOSS_SEED)
    return feats.cuda(), x.cuda(), y.cuda(), mask.cuda()


def _count_calls(monkeypatch):
    from goliath_amd import perceptual

    taken, op = [], perceptual.conv3_relu
    monkeypatch.setattr(perceptual, "conv3_relu", lambda *a: (taken.append(tuple(a[0].shape)), op(*a))[1])
    return taken


@pytest.mark.parametrize("forced", [True, False], ids=["all-fused", "committed-dispatch"])
def test_loss_and_image_gradient_match_float64(forced, monkeypatch):
    from goliath_amd import perceptual

    l64, (g64,), bound = _reference()
    monkeypatch.setenv("GOLIATH_FUSED_VGG_ALL", "1" if forced else "0")
    taken = _count_calls(monkeypatch)
    feats, x, y, mask = _gpu_case()
    x.requires_grad_(True)
    loss = perceptual.VGGLossMasked(feats)(x, y, mask)
    g, = torch.autograd.grad(loss, x)
    err = [abs(float(loss.detach()) - float(l64)) / abs(float(l64)), rel_l2(g, g64)]
    print("forced" if forced else "dispatch", "HIP against float64:", err, "bound", bound, "operator calls", len(taken))
    admitted, hw = 0, tuple(x.shape[2:])
    for _, weight, _, pool, _, _ in feats.layers():
        admitted += bool(perceptual.DISPATCH.get((weight.shape[1], weight.shape[0], *hw, pool), False))
        hw = (hw[0] // 2, hw[1] // 2) if pool else hw
    assert len(taken) == (26 if forced else 2 * admitted)       # prediction and target
    assert float(l64) > 0 and float(g64.abs().max()) > 0
    assert err[0] <= bound[0] and err[1] <= bound[1]


def test_target_branch_saves_nothing(monkeypatch):
    """The target runs under no_grad: the loss's graph holds no node of the target's layers, and a plain factor for a mask
    scales the unmasked loss."""
    from goliath_amd import perceptual

    monkeypatch.setenv("GOLIATH_FUSED_VGG_ALL", "1")
    feats, x, y, mask = _gpu_case()
    net = perceptual.VGGLossMasked(feats)
    x.requires_grad_(True)
    seen = []
    fwd = perceptual._Conv3.forward

    def spy(ctx, xx, *rest):
        out = fwd(ctx, xx, *rest)
        seen.append(bool(ctx.needs_input_grad[0]))
        return out

    monkeypatch.setattr(perceptual._Conv3, "forward", staticmethod(spy))
    net(x, y, mask)
    assert seen == [True] * 13 + [False] * 13
    monkeypatch.undo()
    monkeypatch.setenv("GOLIATH_FUSED_VGG_ALL", "1")
    one, half = net(x, y, 1.0), net(x, y, 0.5)
    assert float(one) > 0 and abs(float(half) / float(one) - 0.5) <= 1e-6


def test_through_patch_losses(monkeypatch):
    """dropin.patch_losses(perceptual=features) on a stand-in registry: the `vgg` entry, built and called the way
    ModularLoss does, returns the number VGGLossMasked returns; with mask_erode the mask goes through imageops.erode."""
    from goliath_amd import dropin, imageops, perceptual

    monkeypatch.setenv("GOLIATH_FUSED_VGG_ALL", "1")
    feats, x, y, mask = _gpu_case()
    reg = types.SimpleNamespace(loss_registry={"vgg": "untouched", "effnet": "untouched"}, FnLoss=None)
    assert dropin.patch_losses(reg, perceptual=feats) is reg and reg.loss_registry["effnet"] == "untouched"
    direct = perceptual.VGGLossMasked(feats)(x, y, mask)
    mod = reg.loss_registry["vgg"](None)
    got = mod({"rendered_rgb": x}, {"image": y, "image_mask": mask})
    assert torch.equal(got, direct)
    got = reg.loss_registry["vgg"](None, dst_key="other", mask_key="alpha")({"rendered_rgb": x, "other": y, "alpha": mask}, {})
    assert torch.equal(got, direct)
    hard = (mask > 0.5).float()
    eroded = reg.loss_registry["vgg"](None, mask_erode=3)({"rendered_rgb": x}, {"image": y, "image_mask": hard})
    assert torch.equal(eroded, perceptual.VGGLossMasked(feats)(x, y, imageops.erode(hard, 3)))
    assert float(eroded) != float(perceptual.VGGLossMasked(feats)(x, y, hard))


def test_target_that_requires_grad(monkeypatch):
    """The `dst_key` case: a target that requires grad takes the twin's elementwise tap lines; loss, g_image and g_target
    match float64 within the same kind of bound."""
    from goliath_amd import perceptual

    l64, g64, bound = _reference(True)
    monkeypatch.setenv("GOLIATH_FUSED_VGG_ALL", "1")
    taken = _count_calls(monkeypatch)
    feats, x, y, mask = _gpu_case()
    x.requires_grad_(True)
    y.requires_grad_(True)
    loss = perceptual.VGGLossMasked(feats)(x, y, mask)
    g = torch.autograd.grad(loss, [x, y])
    err = [abs(float(loss.detach()) - float(l64)) / abs(float(l64))] + [rel_l2(a, b) for a, b in zip(g, g64)]
    print("HIP against float64:", err, "bound", bound)
    assert len(taken) == 26 and float(g64[1].abs().max()) > 0
    for e, b in zip(err, bound):
        assert e <= b
