"""GPU: the fused hidden decoder layer (goliath_amd.trunk: gol_trunk_conv_fwd/bwd) against its float64 torch twin, the
whole trunk and the model drop-in with the switch on against the switch off."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

from scenes import rel_l2

pytestmark = pytest.mark.gpu

# (B, Ci, Co, h, w)
SHAPES = [
    (2, 16, 16, 1, 1),     # every quad is a border quad
    (3, 24, 16, 5, 7),     # Ci not a multiple of 16; odd sizes; partial pixel tiles that wrap rows; odd batch
    (2, 32, 48, 9, 4),     # Co not a multiple of 32; h != w
    (1, 136, 32, 6, 6),    # more than one K stage with a ragged last channel tile
    (2, 264, 32, 4, 4),    # the vcond first-layer Ci
    (2, 64, 32, 17, 33),   # several workgroups in both directions; split-K with a ragged tail
    (9, 16, 16, 3, 2),     # batch larger than a tile of views
]
KINK = 1e-4   # upstream gradients are zeroed where the float64 pre-activation is closer to the LeakyReLU kink than this


@functools.lru_cache(maxsize=None)
def _case(i, leak=0.2):
    """Inputs (CPU, float32) and the float64 reference of shape i: y, the masked upstream gradient and the three gradients."""
    from goliath_amd import trunk

    B, Ci, Co, h, w = SHAPES[i]
    torch.manual_seed(100 + i)
    x = torch.randn(B, Ci, h, w)
    weight_v = torch.randn(Ci, Co, 4, 4)
    weight_g = torch.rand(1, Co, 1, 1) + 0.5
    bias = 0.5 * torch.randn(Co, 2 * h, 2 * w)
    weight = (weight_v.double() * (weight_g.double() / weight_v.double().norm())).float()   # layers.py:157-244
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, weight, bias))
    pre64 = torch.nn.functional.conv_transpose2d(x64, w64, None, 2, 1) + b64[None]
    y64 = trunk.convt_ub_lrelu_torch(x64, w64, b64, leak)
    keep = pre64.detach().abs() >= KINK
    up = torch.randn(y64.shape) * keep
    zeroed = 1.0 - float(keep.double().mean())
    g64 = torch.autograd.grad((y64 * up.double()).sum(), [x64, w64, b64])
    return dict(x=x, weight=weight, bias=bias, y=y64.detach(), up=up, zeroed=zeroed, grads=g64)


def _run(case, leak, need=(True, True, True)):
    from goliath_amd import trunk

    leaves = [case[k].cuda().requires_grad_(n) for k, n in zip(("x", "weight", "bias"), need)]
    y = trunk.convt_ub_lrelu(*leaves, leak)
    wanted = [t for t, n in zip(leaves, need) if n]
    grads = iter(torch.autograd.grad((y * case["up"].cuda()).sum(), wanted))
    return y, [next(grads) if n else None for n in need]


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernels_match_float64(i):
    """Forward and the three gradients <= 1e-5 rel-L2 against the float64 torch composition on the same inputs (the bar of
    test_tail_conv_kernels_match_torch; the fp32 torch composition itself sits at <= 1.6e-7 / <= 1.2e-6)."""
    case = _case(i)
    assert case["zeroed"] <= 1e-3
    y, grads = _run(case, 0.2)
    err = {"y": rel_l2(y, case["y"])}
    for n, a, b in zip(("g_x", "g_weight", "g_bias"), grads, case["grads"]):
        err[n] = rel_l2(a, b)
    print(SHAPES[i], err)
    for n, v in err.items():
        assert v <= 1e-5, (n, v)


@pytest.mark.parametrize("i,leak", [(1, 1.0), (5, 0.01)])
def test_gradient_subsets(i, leak):
    """leak = 1 (pure conv + bias, every mask 1) and a small leak, with x or the bias not requiring a gradient: the NULL
    outputs are skipped and the remaining gradients are unchanged."""
    case = _case(i, leak)
    assert case["zeroed"] <= 1e-3
    for need in ((False, True, True), (True, True, False), (False, False, True)):
        y, grads = _run(case, leak, need)
        assert rel_l2(y, case["y"]) <= 1e-5
        for n, a, b in zip(("g_x", "g_weight", "g_bias"), grads, case["grads"]):
            if a is not None:
                assert rel_l2(a, b) <= 1e-5, (n, need)


def test_backward_is_bitwise_reproducible():
    case = _case(5)
    _, g1 = _run(case, 0.2)
    _, g2 = _run(case, 0.2)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


TRUNK_SEED = 52


def _trunk_case():
    from goliath_amd import decoder

    torch.manual_seed(TRUNK_SEED)
    dec = decoder.PrimDecoderConvs(base=1)
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, decoder.ConvTranspose2dWNUB):
                m.bias.normal_(0, 0.3)
    return dec, torch.randn(1, 256), torch.randn(1, 3)


def _kink_margin(dec, embs, campos):
    """Smallest |pre-activation| of the twelve hidden layers in a float64 copy of the trunk."""
    d64 = copy.deepcopy(dec).double()
    margin = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: margin.append(float(out.abs().min())))
             for stack in (d64.vnocond_mod[:-1], d64.vcond_mod[:-1]) for m in stack if not isinstance(m, nn.LeakyReLU)]
    with torch.no_grad():
        d64.trunk(embs.double(), campos.double())
    for hk in hooks:
        hk.remove()
    assert len(margin) == 12
    return min(margin)


def test_whole_trunk_switch_on_equals_off(monkeypatch):
    """`PrimDecoderConvs(base=1).trunk`, B = 1, all twelve hidden layers on the HIP operator against the torch modules:
    outputs <= 1e-5, every trunk parameter's gradient <= 1e-4 and non-zero.  Seed 52 was picked on the CPU among 0..79 for
    the widest kink margin: the float64 trunk's smallest hidden |pre-activation| is 1.53e-5 (asserted > 1e-6 below), so no
    activation mask can differ between the two fp32 paths."""
    dec, embs, campos = _trunk_case()
    assert _kink_margin(dec, embs, campos) > 1e-6
    dec, embs, campos = dec.cuda(), embs.cuda(), campos.cuda()
    names, params = zip(*[(n, q) for n, q in dec.named_parameters()
                          if not n.startswith(("vnocond_mod.12.", "vcond_mod.12."))])
    assert len(params) == 3 + 3 + 2 * 6 * 3
    ups = None

    def run():
        nonlocal ups
        out = dec.trunk(embs, campos)
        if ups is None:
            torch.manual_seed(0)
            ups = [torch.randn_like(o) for o in out]
        return out, torch.autograd.grad(sum((o * u).sum() for o, u in zip(out, ups)), params)

    monkeypatch.delenv("GOLIATH_FUSED_TRUNK", raising=False)
    out0, g0 = run()
    monkeypatch.setenv("GOLIATH_FUSED_TRUNK", "1")
    monkeypatch.setenv("GOLIATH_FUSED_TRUNK_ALL", "1")
    from goliath_amd import trunk

    taken = []
    hip = trunk.convt_ub_lrelu
    monkeypatch.setattr(trunk, "convt_ub_lrelu", lambda *a: (taken.append(1), hip(*a))[1])
    out1, g1 = run()
    assert len(taken) == 12
    for a, b in zip(out1, out0):
        assert rel_l2(a, b) <= 1e-5
    for n, a, b in zip(names, g1, g0):
        assert float(b.norm()) > 0 and float(a.norm()) > 0, n
        assert rel_l2(a, b) <= 1e-4, n


def test_prim_decoder_forward_with_fused_trunk(monkeypatch):
    """The model-level drop-in with GOLIATH_FUSED_TRUNK=1 gives the predictions of the default path (setup of
    test_prim_decoder_forward_fuses_the_tail: reference-native slab, B = 1, no_grad)."""
    from goliath_amd import decoder, rgca, trunk

    torch.manual_seed(3)
    dec = decoder.PrimDecoderConvs().cuda()
    S = dec.slabsize
    with torch.no_grad():
        dec.vnocond_mod[-1].bias.normal_(0, 0.2)

    class Geo:
        def to_uv(self, x):
            return x

        def vn(self, x):
            return torch.roll(x, 1, 1)

    dec.geo_fn, dec.albedo = Geo(), torch.nn.Parameter(torch.rand(1, S * S, 3, device="cuda"))
    dec.color_sh_degree, dec.diff_sh_degree = 3, 8
    dec.eval()
    geom = 50 * torch.randn(1, 3, S, S, device="cuda")
    args = (torch.randn(1, 256, device="cuda"), geom, torch.tensor([[0.0, 0, -700]], device="cuda"),
            torch.rand(1, 2, 1, device="cuda"), 1000 * torch.randn(1, 2, 3, device="cuda"), 0.3 * torch.randn(1, 3, 81, device="cuda"),
            torch.full((1,), 2, dtype=torch.int32, device="cuda"))
    monkeypatch.delenv("GOLIATH_FUSED_TRUNK", raising=False)
    taken = []
    hip = trunk.convt_ub_lrelu
    monkeypatch.setattr(trunk, "convt_ub_lrelu", lambda *a: (taken.append(1), hip(*a))[1])
    with torch.no_grad():
        plain = rgca.prim_decoder_forward(dec, *args)
        assert not taken
        monkeypatch.setenv("GOLIATH_FUSED_TRUNK", "1")
        monkeypatch.setenv("GOLIATH_FUSED_TRUNK_ALL", "1")
        fused = rgca.prim_decoder_forward(dec, *args)
    assert len(taken) == 12
    assert set(fused) == set(plain)
    for k in plain:
        assert rel_l2(fused[k], plain[k]) <= 1e-4, k
