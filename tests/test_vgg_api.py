"""CPU: goliath_amd.perceptual's twin against the reference's own VGGLossMasked (tests/golden/vgg_golden.npz, made by
tests/golden/make_vgg_golden.py), state-dict loading, the frozen parameters and the drop-in keyword."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden():
    gold = np.load(os.path.join(HERE, "golden", "vgg_golden.npz"))
    sd = {k: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("features.")}
    return gold, sd


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def test_twin_reproduces_the_reference_loss():
    """vgg_loss_torch on the fixture's network and inputs: float64 against the reference run in float64 (<= 1e-12: the same
    operations in the same order), float32 against the reference run in float32 (<= 1e-6), loss and image gradient, with the
    soft mask and with a plain factor for a mask."""
    from goliath_amd import perceptual

    gold, sd = _golden()
    feats = perceptual.Vgg19Features(tuple(int(w) for w in gold["widths"])).load_torchvision_state_dict(sd)
    assert len(sd) == 26
    for tag, dtype, bar in (("64", torch.float64, 1e-12), ("32", torch.float32, 1e-6)):
        x = torch.from_numpy(gold["x"]).to(dtype).requires_grad_(True)
        y, mask = torch.from_numpy(gold["y"]).to(dtype), torch.from_numpy(gold["mask"]).to(dtype)
        loss = perceptual.vgg_loss_torch(feats, x, y, mask)
        g, = torch.autograd.grad(loss, x)
        assert loss.dtype == dtype and float(gold[f"loss{tag}"]) > 0
        e = (_rel(loss.detach(), gold[f"loss{tag}"]), _rel(g, gold[f"g_x{tag}"]))
        f = _rel(perceptual.vgg_loss_torch(feats, x.detach(), y, 0.5), gold[f"loss_factor{tag}"])
        print(tag, e, f)
        assert max(e) <= bar and f <= bar
    taps = feats.forward_torch(torch.from_numpy(gold["x"]))
    assert [tuple(t.shape[1:]) for t in taps] == [(16, 34, 45), (16, 17, 22), (16, 8, 11), (16, 4, 5), (32, 2, 2)]


def test_layout_and_frozen_parameters():
    from goliath_amd import perceptual

    feats = perceptual.Vgg19Features()
    names = [n for n, _ in feats.named_parameters()]
    assert names == [f"features.{i}.{n}" for i in (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28) for n in ("weight", "bias")]
    shapes = [tuple(p.shape) for n, p in feats.named_parameters() if n.endswith("weight")]
    assert shapes == [(64, 3, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3), (128, 128, 3, 3), (256, 128, 3, 3)] + \
        [(256, 256, 3, 3)] * 3 + [(512, 256, 3, 3)] + [(512, 512, 3, 3)] * 4
    assert not any(p.requires_grad for p in feats.parameters())
    assert [(i, pool, img, tap) for i, _, _, pool, img, tap in feats.layers() if pool or img or tap] == \
        [(0, False, True, True), (2, True, False, False), (5, False, False, True), (7, True, False, False),
         (10, False, False, True), (16, True, False, False), (19, False, False, True), (25, True, False, False),
         (28, False, False, True)]
    with pytest.raises(ValueError):
        perceptual.Vgg19Features((16, 16, 24, 32, 32))
    assert inspect.signature(perceptual.VGGLossMasked.forward).parameters.keys() >= {"x_rgb", "y_rgb", "mask"}
    assert perceptual.VGGLossMasked(perceptual.Vgg19Features((16,) * 5)).weights == [20.0, 5.0, 0.9, 0.5, 0.5]


def test_weight_gradient_raises():
    from goliath_amd import _lib, perceptual

    x = torch.randn(1, 8, 4, 4, requires_grad=True)
    w, b = torch.randn(16, 8, 3, 3), torch.zeros(16)
    for ww, bb in ((w.clone().requires_grad_(True), b), (w, b.clone().requires_grad_(True))):
        with pytest.raises(_lib.GoliathHipError, match="frozen"):
            perceptual.conv3_relu(x, ww, bb)
    with pytest.raises(_lib.GoliathHipError, match="CUDA"):     # no CPU path, no quiet fall-back
        perceptual.conv3_relu(x, w, b)
    feats = perceptual.Vgg19Features((16,) * 5)
    with pytest.raises(_lib.GoliathHipError, match="CUDA"):
        perceptual.VGGLossMasked(feats)(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), 1.0)
    y = perceptual.conv3_relu_torch(x, w, b, pool=True)
    assert tuple(y.shape) == (1, 16, 2, 2) and y.requires_grad


def test_state_dict_loading(tmp_path):
    from goliath_amd import perceptual

    gold, sd = _golden()
    widths = tuple(int(w) for w in gold["widths"])
    ref = perceptual.Vgg19Features(widths).load_torchvision_state_dict(sd)
    # without the prefix, with classifier and later feature entries: ignored
    bare = {k[len("features."):]: v for k, v in sd.items()}
    bare.update({"30.weight": torch.zeros(3), "classifier.0.weight": torch.zeros(5, 5), "classifier.0.bias": torch.zeros(5)})
    other = perceptual.Vgg19Features(widths).load_torchvision_state_dict(bare)
    for (n, a), (_, b) in zip(ref.named_parameters(), other.named_parameters()):
        assert torch.equal(a, b) and torch.equal(a, sd[n]) and not b.requires_grad
    # a file
    path = tmp_path / "vgg19_small.pth"
    torch.save(sd, path)
    third = perceptual.as_features(perceptual.Vgg19Features(widths).load_torchvision_state_dict(str(path)))
    assert torch.equal(third.features.get_submodule("28").weight, sd["features.28.weight"])
    # errors name what is expected
    with pytest.raises(FileNotFoundError, match="vgg19 state dict"):
        perceptual.Vgg19Features(widths).load_torchvision_state_dict(str(tmp_path / "absent.pth"))
    missing = {k: v for k, v in sd.items() if k != "features.19.bias"}
    with pytest.raises(KeyError, match=r"features\.19\.bias"):
        perceptual.Vgg19Features(widths).load_torchvision_state_dict(missing)
    with pytest.raises(ValueError, match=r"features\.0\.weight.*expected \(64, 3, 3, 3\)"):
        perceptual.Vgg19Features().load_torchvision_state_dict(sd)
    with pytest.raises(TypeError):
        perceptual.Vgg19Features(widths).load_torchvision_state_dict(3)


def _registry():
    entries = dict(rgb_l1="reference", rgb_ssim="reference", vgg="untouched", effnet="untouched", effnet_phys="untouched")
    return types.SimpleNamespace(loss_registry=entries, FnLoss=lambda fn, args: (fn, args))


def test_patch_losses_keyword():
    from goliath_amd import dropin, perceptual

    assert inspect.signature(dropin.patch_losses).parameters["perceptual"].default is None
    reg = dropin.patch_losses(_registry())
    assert reg.loss_registry["vgg"] == "untouched" and reg.loss_registry["effnet"] == "untouched"
    _, sd = _golden()
    feats = perceptual.Vgg19Features((16, 16, 16, 16, 32)).load_torchvision_state_dict(sd)
    reg = dropin.patch_losses(_registry(), perceptual=feats)
    assert reg.loss_registry["effnet"] == "untouched" and reg.loss_registry["effnet_phys"] == "untouched"
    mod = reg.loss_registry["vgg"](None, mask_erode=3, dst_key="rgb2")
    assert isinstance(mod, perceptual.VGGLoss) and mod.net.vgg is feats
    assert (mod.src_key, mod.tgt_key, mod.dst_key, mod.mask_key, mod.mask_erode) == \
        ("rendered_rgb", "image", "rgb2", "image_mask", 3)
    with pytest.raises(ValueError, match=r"expected \(64, 3, 3, 3\)"):     # a state dict means the full-width network
        dropin.patch_losses(_registry(), perceptual=sd)
    with pytest.raises(FileNotFoundError):
        dropin.patch_losses(_registry(), perceptual="/nonexistent/vgg19.pth")
