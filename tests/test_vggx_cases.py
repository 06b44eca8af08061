"""CPU: precision="bf16x3" of goliath_amd.perceptual judged without a GPU -- the split arithmetic's deviation from float64 on
the cases of tests/vggx_cases.py, the share of gradients the cases zero near their kinks, the seed of the whole-loss case,
and the API."""
import inspect
import json
import os
import types

import pytest
import torch

import vgg_cases as vc
import vggx_cases as vx
from scenes import rel_l2


def test_split_is_round_to_nearest_even_and_exact_to_two_to_the_minus_16():
    from goliath_amd import perceptual

    g = torch.Generator().manual_seed(5)
    v = torch.cat([torch.randn(4096, generator=g) * 3.0, torch.zeros(3),
                   torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8])])   # ties: to even
    hi, lo = perceptual.split_bf16(v)
    assert hi.dtype == torch.bfloat16 and lo.dtype == torch.bfloat16
    assert torch.equal(hi.float()[-3:], torch.tensor([1.0, 1.0 + 2.0 ** -6, -1.0]))
    assert torch.equal(hi[4096:4099].float(), torch.zeros(3)) and torch.equal(lo[4096:4099].float(), torch.zeros(3))
    rest = (v.double() - hi.double() - lo.double()).abs()
    assert float((rest / v.double().abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
    assert torch.equal(lo, (v - hi.float()).to(torch.bfloat16)) and float(lo.float().abs().max()) > 0


@pytest.mark.parametrize("i", range(len(vx.CASES)), ids=vx.IDS)
def test_split_arithmetic_stays_within_the_bar_of_float64(i):
    """Pre-activation of the float64-accumulated split twin against the plain float64 layer: rel-L2 <= BAR and every
    element within 3.1 2^-16 sum |x||w|; the twin's g_x within BAR of float64's under the same masked upstream gradient.
    Measured: pre 4.1e-6 ... 4.5e-6, g_x 4.3e-6 ... 4.5e-6, largest element error 2.4e-6 of sum |x||w| (the bound is
    4.7e-5)."""
    from goliath_amd import perceptual

    _, pool = vx.CASES[i]
    ref, inp = vx.reference(i), vx.inputs(i)
    err = (ref["pre"] - ref["pre64"]).abs()
    ratio = float((err / ref["mass"]).max())
    e_pre, e_g = rel_l2(ref["pre"], ref["pre64"]), rel_l2(ref["g_x"], ref["g_x64"])
    print(vx.IDS[i], "pre", e_pre, "element ratio", ratio, "of", vx.ELEMENT_BOUND, "g_x", e_g)
    assert e_pre <= vc.BAR
    assert bool((err <= vx.ELEMENT_BOUND * ref["mass"]).all())
    assert e_g <= vc.BAR and float(ref["g_x64"].abs().max()) > 0
    # the twin is that arithmetic: relu (and pool) of the written-out pre-activation, bitwise
    y = torch.relu(ref["pre"])
    assert torch.equal(ref["out"], torch.nn.functional.max_pool2d(y, 2) if pool else y)
    # ... and it is not plain bf16, nor plain fp32: dropping the cross terms lands far above the bar
    hh = vx.split_pre(inp["x"], inp["weight"], inp["bias"], torch.float64) \
        - torch.nn.functional.conv2d(perceptual.split_bf16(inp["x"])[1].double(),
                                     perceptual.split_bf16(inp["weight"])[0].double(), None, 1, 1)
    assert rel_l2(hh, ref["pre64"]) > 10 * vc.BAR


@pytest.mark.parametrize("i", range(len(vx.CASES)), ids=vx.IDS)
def test_zeroed_share_stays_under_the_cap(i):
    """At most 0.2 % of a case's output elements lose their upstream gradient to a kink of the split twin (KINK = 1e-4)."""
    ref = vx.reference(i)
    print(vx.IDS[i], "zeroed", ref["zeroed"])
    assert ref["zeroed"] <= vc.ZEROED_CAP
    assert float(ref["g_x"].abs().max()) > 0 and float(ref["out"].abs().max()) > 0
    (_, _, _, H, W), pool = vx.CASES[i]
    assert tuple(ref["out"].shape[2:]) == ((H // 2, W // 2) if pool else (H, W))


def test_loss_seed_keeps_both_accumulations_on_one_side():
    """At the committed seed the fp32- and the float64-accumulated split twin have identical ReLU masks and pool positions,
    for prediction and target; only the 32 -> 32 layers of LOSS_WIDTHS run split (the mix the real network has).  Their
    distance, which sets the GPU test's bound, is asserted under the largest measured over such seeds (loss 1.7e-7, g_image
    5.1e-6); at this seed it is loss 3.2e-8, g_image 2.9e-6, and the split loss is 1.6e-8, its g_image 3.8e-6 off the plain
    float64 loss (no ReLU decides differently at this seed)."""
    from goliath_amd import perceptual

    feats, x, y, mask = vc.loss_case(vx.LOSS_SEED)
    assert vc.LOSS_WIDTHS == (16, 16, 32, 32, 32) and vc.LOSS_IMAGE == (2, 3, 50, 83)
    hw, split = tuple(x.shape[2:]), []
    for _, weight, _, pool, image_in, _ in feats.layers():
        split.append(perceptual.supported(weight.shape[1], weight.shape[0], *hw, pool, image_in, "bf16x3"))
        hw = (hw[0] // 2, hw[1] // 2) if pool else hw
    assert split == [False] * 5 + [True] * 8
    for img in (x, y):
        taps32, _, relu32, pool32 = vx.trace(feats, img, torch.float32)
        taps64, _, relu64, pool64 = vx.trace(feats, img, torch.float64)
        assert len(relu32) == 13 and len(pool32) == 4
        for a, b in zip(relu32 + pool32, relu64 + pool64):
            assert torch.equal(a, b)
        for a, b in zip(perceptual.Vgg19Features.forward_torch(feats, img.double(), "bf16x3"), taps64):
            assert torch.equal(a, b)     # forward_torch routes the same layers to the split twin
    l64, g64, dist = vx.loss_reference()
    l_plain, g_plain = vx.loss_twin(torch.float64, "fp32")
    print("fp32- against float64-accumulated split twin [loss, g_image]:", dist)
    print("split against plain float64 (for the record): loss", abs(float(l64) - float(l_plain)) / float(l_plain),
          "g_image", rel_l2(g64, g_plain))
    assert float(l64) > 0 and float(g64.abs().max()) > 0
    assert dist[0] <= 1.7e-7 and dist[1] <= 5.1e-6
    assert abs(float(l64) - float(l_plain)) / float(l_plain) <= 1e-5


def test_precision_defaults_are_fp32_everywhere():
    from goliath_amd import dropin, perceptual

    for fn in (perceptual.conv3_relu, perceptual.supported, perceptual.Vgg19Features.__init__,
               perceptual.Vgg19Features.forward_torch, perceptual.vgg_loss_torch, perceptual.as_features):
        assert inspect.signature(fn).parameters["precision"].default == "fp32", fn
    params = inspect.signature(dropin.patch_losses).parameters
    assert list(params)[-1] == "perceptual_precision" and params["perceptual_precision"].default == "fp32"
    assert inspect.signature(perceptual.conv3_relu_split_torch).parameters["acc_dtype"].default is torch.float64
    feats = perceptual.Vgg19Features(vc.LOSS_WIDTHS)
    assert feats.precision == "fp32" and perceptual.Vgg19Features(vc.LOSS_WIDTHS, precision="bf16x3").precision == "bf16x3"
    assert perceptual.as_features(feats) is feats and feats.precision == "fp32"
    assert perceptual.as_features(feats, "bf16x3").precision == "bf16x3"
    # the table of admitted shapes holds what the probe admitted (shapes the split operator supports), and nothing else
    for (Ci, Co, H, W, pool), won in perceptual.DISPATCH_BF16X3.items():
        assert won is True and perceptual.supported(Ci, Co, H, W, pool, False, "bf16x3")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "vggx_probe.json")) as f:
        probe = json.load(f)
    assert sorted(map(tuple, probe["dispatch"])) == sorted(perceptual.DISPATCH_BF16X3)
    for row in probe["layers"]:
        t, h = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
        assert row["admitted"] == (h["median"] < t["median"] - t["spread"])


def test_supported_shapes():
    from goliath_amd import perceptual

    sup = perceptual.supported
    assert sup(32, 32, 1, 1, precision="bf16x3") and sup(512, 64, 7, 5, True, precision="bf16x3")
    assert not sup(48, 32, 8, 8, precision="bf16x3") and not sup(32, 16, 8, 8, precision="bf16x3")
    assert not sup(32, 48, 8, 8, precision="bf16x3") and not sup(32, 32, 1, 8, True, precision="bf16x3")
    assert not sup(3, 64, 8, 8, False, True, precision="bf16x3")      # no image layer
    assert sup(48, 16, 8, 8) and sup(3, 64, 8, 8, False, True)        # "fp32" is what it was


def test_unknown_precision_raises():
    from goliath_amd import dropin, perceptual

    feats, x, y, mask = vc.loss_case(vx.LOSS_SEED)
    w, b = vc.draw_layer(1, 32, 32)
    xx = torch.randn(1, 32, 4, 4)
    for call in (lambda: perceptual.conv3_relu(xx, w, b, precision="bf16"),
                 lambda: perceptual.supported(32, 32, 4, 4, precision="fp16"),
                 lambda: perceptual.Vgg19Features(precision="tf32"),
                 lambda: feats.forward_torch(x, "bf16x2"),
                 lambda: perceptual.vgg_loss_torch(feats, x, y, mask, precision=None),
                 lambda: perceptual.as_features(feats, "fp8"),
                 lambda: dropin.patch_losses(types.SimpleNamespace(loss_registry={}, FnLoss=None), perceptual=feats,
                                             perceptual_precision="fp8")):
        with pytest.raises(ValueError, match="precision"):
            call()


def test_cpu_tensors_raise_from_the_operator_and_run_in_the_twins():
    from goliath_amd import _lib, perceptual

    w, b = vc.draw_layer(2, 32, 64)
    x = torch.randn(2, 32, 6, 7, requires_grad=True)
    with pytest.raises(_lib.GoliathHipError, match="CUDA"):
        perceptual.conv3_relu(x, w, b, precision="bf16x3")
    with pytest.raises(_lib.GoliathHipError, match="frozen"):
        perceptual.conv3_relu(x, w.clone().requires_grad_(True), b, precision="bf16x3")
    p = perceptual.conv3_relu_split_torch(x, w, b, pool=True)
    assert p.dtype == torch.float64 and tuple(p.shape) == (2, 64, 3, 3)
    g, = torch.autograd.grad(p.sum(), x)
    assert g.dtype == x.dtype and g.shape == x.shape and float(g.abs().max()) > 0
    y32 = perceptual.conv3_relu_split_torch(x, w, b, acc_dtype=torch.float32)
    assert y32.dtype == torch.float32
    assert rel_l2(y32, perceptual.conv3_relu_split_torch(x, w, b)) <= 1e-6
    # a weight that requires grad gets none from the twin either: the layer is frozen
    wg = w.clone().requires_grad_(True)
    out = perceptual.conv3_relu_split_torch(x, wg, b)
    assert torch.autograd.grad(out.sum(), [x, wg], allow_unused=True)[1] is None
