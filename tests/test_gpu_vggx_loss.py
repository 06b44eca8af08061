"""GPU: the masked VGG loss of goliath_amd.perceptual at precision="bf16x3" (reduced widths, tests/vgg_cases.py:loss_case at
tests/vggx_cases.py:LOSS_SEED) against the float64-accumulated split twin, the mixed dispatch, the packed-weight cache and
the drop-in.

Bound (the rule of tests/test_gpu_vgg_loss.py): 3 x the fp32-accumulated CPU split twin's own relative distance from the
float64-accumulated one, plus 1e-6.  The seed keeps both on one side of every ReLU and pool decision, and only the 32 -> 32
layers run split (both asserted on the CPU in tests/test_vggx_cases.py)."""
import types

import pytest
import torch

import vgg_cases as vc
import vggx_cases as vx
from scenes import rel_l2

pytestmark = pytest.mark.gpu


def _gpu_case(precision="bf16x3"):
    feats, x, y, mask = vc.loss_case(vx.LOSS_SEED)
    feats.precision = precision
    return feats.cuda(), x.cuda(), y.cuda(), mask.cuda()


def _count_split_calls(monkeypatch):
    from goliath_amd import perceptual

    taken, fwd = [], perceptual._Conv3x.forward
    monkeypatch.setattr(perceptual._Conv3x, "forward",
                        staticmethod(lambda ctx, x, *rest: (taken.append(tuple(x.shape)), fwd(ctx, x, *rest))[1]))
    return taken


def test_loss_and_image_gradient_match_the_split_twin(monkeypatch):
    from goliath_amd import perceptual

    l64, g64, dist = vx.loss_reference()
    bound = [3.0 * d + 1e-6 for d in dist]
    monkeypatch.setenv("GOLIATH_FUSED_VGG_ALL", "1")
    taken = _count_split_calls(monkeypatch)
    feats, x, y, mask = _gpu_case()
    x.requires_grad_(True)
    loss = perceptual.VGGLossMasked(feats)(x, y, mask)
    g, = torch.autograd.grad(loss, x)
    err = [abs(float(loss.detach()) - float(l64)) / abs(float(l64)), rel_l2(g, g64)]
    print("HIP bf16x3 against the float64-accumulated split twin:", err, "bound", bound, "split calls", len(taken))
    assert len(taken) == 16 and all(s[1] == 32 for s in taken)      # the eight 32 -> 32 layers, prediction and target
    assert float(l64) > 0 and float(g64.abs().max()) > 0
    assert err[0] <= bound[0] and err[1] <= bound[1]


def test_mixed_dispatch_leaves_the_other_layers_bitwise_alone(monkeypatch):
    """With one shape in DISPATCH_BF16X3 a layer of that shape runs split (and differs from fp32 by the split's 4.5e-6), every
    other layer does, on the same input, bit for bit what precision="fp32" does."""
    from goliath_amd import perceptual

    monkeypatch.setenv("GOLIATH_FUSED_VGG_ALL", "0")
    one = (32, 32, 6, 10, False)
    monkeypatch.setattr(perceptual, "DISPATCH_BF16X3", {one: True})
    taken = _count_split_calls(monkeypatch)
    feats, x, _, _ = _gpu_case()
    split, inp = 0, x
    with torch.no_grad():
        for i, weight, bias, pool, image_in, _ in feats.layers():
            want = perceptual._layer(inp, weight, bias, pool, image_in)
            got = perceptual._layer(inp, weight, bias, pool, image_in, "bf16x3", lambda i=i: feats.packed(i))
            if (weight.shape[1], weight.shape[0], *inp.shape[2:], pool) == one:
                split += 1
                assert not torch.equal(got, want) and rel_l2(got, want) <= 2 * vc.BAR
            else:
                assert torch.equal(got, want), i
            inp = want
        assert split == 3 and len(taken) == 3
        feats(x)
        assert len(taken) == 6
        feats.precision = "fp32"
        feats(x)
        assert len(taken) == 6


def test_packed_cache_follows_the_weights(monkeypatch):
    """pack() fills the cache for the supported layers; a forward then packs nothing; an in-place change of a weight (a new
    version) and load_state_dict make the next forward pack again, and the output follows the new weights."""
    from goliath_amd import perceptual

    monkeypatch.setenv("GOLIATH_FUSED_VGG_ALL", "1")
    feats, x, _, _ = _gpu_case()
    packs, op = [], perceptual.pack_bf16x3
    monkeypatch.setattr(perceptual, "pack_bf16x3", lambda w: (packs.append(tuple(w.shape)), op(w))[1])
    assert feats.pack() is feats and len(packs) == 8 and sorted(feats._packed) == [12, 14, 16, 19, 21, 23, 25, 28]
    with torch.no_grad():
        before = feats(x)[-1]
        assert len(packs) == 8
        getattr(feats.features, "28").weight.mul_(2.0)
        after = feats(x)[-1]
        assert len(packs) == 9 and not torch.equal(after, before)
        state = {k: v.clone() for k, v in feats.state_dict().items()}
        feats.load_state_dict(state)
        assert feats._packed == {}
        assert torch.equal(feats(x)[-1], after) and len(packs) == 17
        feats.load_torchvision_state_dict(state)
        assert feats._packed == {}


def test_through_patch_losses(monkeypatch):
    """dropin.patch_losses(perceptual=features, perceptual_precision="bf16x3"): the `vgg` entry runs the split operator and
    returns the number VGGLossMasked returns; without the keyword it stays fp32."""
    from goliath_amd import dropin, perceptual

    monkeypatch.setenv("GOLIATH_FUSED_VGG_ALL", "1")
    feats, x, y, mask = _gpu_case("fp32")
    reg = types.SimpleNamespace(loss_registry={"vgg": "untouched"}, FnLoss=None)
    dropin.patch_losses(reg, perceptual=feats)
    assert feats.precision == "fp32"
    plain = reg.loss_registry["vgg"](None)({"rendered_rgb": x}, {"image": y, "image_mask": mask})
    dropin.patch_losses(reg, perceptual=feats, perceptual_precision="bf16x3")
    assert feats.precision == "bf16x3"
    taken = _count_split_calls(monkeypatch)
    got = reg.loss_registry["vgg"](None)({"rendered_rgb": x}, {"image": y, "image_mask": mask})
    assert len(taken) == 16
    assert torch.equal(got, perceptual.VGGLossMasked(feats)(x, y, mask))
    assert abs(float(got) / float(plain) - 1.0) <= 1e-5     # the split loss is 1.6e-8 off the plain one at this seed (CPU)
