"""GPU: the fused texture-decoder layer (goliath_amd.texdec: gol_upconv_fwd/bwd) against its float64 torch twins, a stack of
layers through `texture_branches` against the library lines, and the model drop-in."""
import functools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from scenes import rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# (B, Ci, Co, Hi, Wi)
SHAPES = [
    (2, 8, 16, 1, 1),       # output 2x2: every tap overhangs; the degenerate axis has H - 1 = 1 and frac = 0
    (3, 16, 4, 3, 5),       # the Co = 4 path; odd batch
    (2, 24, 16, 5, 7),      # Ci not a multiple of 16; odd sizes
    (1, 136, 32, 6, 6),     # several K stages with a ragged last one
    (2, 64, 32, 17, 33),    # several workgroups both ways; rows that wrap tiles; split-K with a tail
    (2, 16, 4, 32, 40),     # the last layer's channel pair over many tiles
    (9, 8, 16, 3, 2),       # batch larger than a tile of views; width 2
    (2, 32, 48, 9, 4),      # Co not a multiple of 32; H != W
]
IDS = ["x".join(map(str, s)) for s in SHAPES]
KINK = 1e-4   # mode 0: upstream gradients are zeroed where the float64 pre-activation is closer to the kink than this
BAR = 1e-5


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """The draws of shape i (CPU, float32), in the order x, weight_v, weight_g, bias, gate, gb, upstream gradients."""
    B, Ci, Co, Hi, Wi = SHAPES[i]
    torch.manual_seed(300 + i)
    x = torch.randn(B, Ci, Hi, Wi)
    weight_v = torch.randn(Co, Ci, 3, 3)
    weight_g = torch.rand(Co, 1, 1, 1) + 0.5
    bias = 0.5 * torch.randn(Co, 2 * Hi, 2 * Wi)
    gate = torch.randn(B, Co, 2 * Hi, 2 * Wi)
    gb = torch.randn(B, Co, 2 * Hi, 2 * Wi)
    up0 = torch.randn(B, Co, 2 * Hi, 2 * Wi)
    up1 = torch.randn(B, Co, 2 * Hi, 2 * Wi)
    weight = (weight_v.double() * (weight_g.double() / weight_v.double().norm())).float()   # layers.py:157-244
    return dict(x=x, weight=weight, bias=bias, gate=gate, gb=gb, up0=up0, up1=up1)


@functools.lru_cache(maxsize=None)
def _case0(i, leak=0.2):
    """Mode 0: float64 reference of shape i: y, the masked upstream gradient and the gradients of x, weight, bias."""
    from goliath_amd import texdec

    inp = _inputs(i)
    x64, w64, b64 = (inp[k].double().requires_grad_(True) for k in ("x", "weight", "bias"))
    pre64 = torch.nn.functional.conv2d(texdec._up2(x64), w64, None, 1, 1) + b64[None]
    y64 = texdec.upconv_lrelu_torch(x64, w64, b64, leak)
    keep = pre64.detach().abs() >= KINK
    up = inp["up0"] * keep
    zeroed = 1.0 - float(keep.double().mean())
    g64 = torch.autograd.grad((y64 * up.double()).sum(), [x64, w64, b64])
    return dict(leaves=(inp["x"], inp["weight"], inp["bias"]), y=y64.detach(), up=up, zeroed=zeroed, grads=g64,
                names=("g_x", "g_w", "g_bias"))


@functools.lru_cache(maxsize=None)
def _case1(i, with_gb):
    """Mode 1: with gb and scale 0.707107, or gb = None and scale 1: gradients of x, weight, gate (, gb)."""
    from goliath_amd import texdec

    inp = _inputs(i)
    keys = ("x", "weight", "gate") + (("gb",) if with_gb else ())
    l64 = [inp[k].double().requires_grad_(True) for k in keys]
    scale = 0.707107 if with_gb else 1.0
    y64 = texdec.upconv_gated_torch(l64[0], l64[1], l64[2], l64[3] if with_gb else None, scale)
    g64 = torch.autograd.grad((y64 * inp["up1"].double()).sum(), l64)
    return dict(leaves=tuple(inp[k] for k in keys), y=y64.detach(), up=inp["up1"], grads=g64, scale=scale,
                names=("g_x", "g_w", "g_gate", "g_gb")[:len(keys)])


def _run0(case, leak, need=(True, True, True)):
    from goliath_amd import texdec

    leaves = [t.cuda().requires_grad_(n) for t, n in zip(case["leaves"], need)]
    y = texdec.upconv_lrelu(*leaves, leak)
    return y, _grads(y, case, leaves, need)


def _run1(case, need=None):
    from goliath_amd import texdec

    need = need or (True,) * len(case["leaves"])
    leaves = [t.cuda().requires_grad_(n) for t, n in zip(case["leaves"], need)]
    y = texdec.upconv_gated(leaves[0], leaves[1], leaves[2], leaves[3] if len(leaves) > 3 else None, case["scale"])
    return y, _grads(y, case, leaves, need)


def _grads(y, case, leaves, need):
    wanted = [t for t, n in zip(leaves, need) if n]
    grads = iter(torch.autograd.grad((y * case["up"].cuda()).sum(), wanted))
    return [next(grads) if n else None for n in need]


def _check(tag, case, y, grads):
    err = {"y": rel_l2(y, case["y"])}
    for n, a, b in zip(case["names"], grads, case["grads"]):
        if a is not None:
            err[n] = rel_l2(a, b)
    print(tag, err)
    for n, v in err.items():
        assert v <= BAR, (tag, n, v)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_mode0_matches_float64(i):
    """y, g_x, g_w and g_bias <= 1e-5 rel-L2 against the float64 twin on the same inputs (the bar of test_gpu_trunk.py and
    test_gpu_encoder.py; the fp32 torch composition itself sits at <= 6.8e-7 (y) and <= 1.5e-6 (gradients) on these shapes)."""
    case = _case0(i)
    print("zeroed", case["zeroed"])
    assert case["zeroed"] <= 1e-3
    _check((SHAPES[i], "mode 0"), case, *_run0(case, 0.2))


@pytest.mark.parametrize("with_gb", [True, False], ids=["gb", "nogb"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_mode1_matches_float64(i, with_gb):
    """y, g_x, g_w, g_gate and g_gb <= 1e-5, once with gb and scale 0.707107 and once with gb = None and scale 1 (the fp32
    composition's floor is <= 1.4e-6)."""
    case = _case1(i, with_gb)
    _check((SHAPES[i], "mode 1", with_gb), case, *_run1(case))


@pytest.mark.parametrize("i,leak", [(1, 1.0), (4, 0.01)])
def test_gradient_subsets_mode0(i, leak):
    """leak = 1 (pure conv + bias, every mask 1) and a small leak, with x, the bias or x and the weight not requiring a
    gradient: the NULL outputs are skipped and the remaining gradients are unchanged."""
    case = _case0(i, leak)
    assert case["zeroed"] <= 1e-3
    _, full = _run0(case, leak)
    for need in ((False, True, True), (True, True, False), (False, False, True)):
        y, grads = _run0(case, leak, need)
        assert [g is not None for g in grads] == list(need)
        _check((SHAPES[i], leak, need), case, y, grads)
        for a, b in zip(grads, full):
            assert a is None or torch.equal(a, b)


def test_gradient_subsets_mode1():
    """Mode 1 with the gate (and others) not requiring a gradient."""
    case = _case1(2, True)
    _, full = _run1(case)
    for need in ((True, True, False, True), (False, True, False, False), (True, False, True, False),
                 (False, False, False, True)):
        y, grads = _run1(case, need)
        assert [g is not None for g in grads] == list(need)
        _check((SHAPES[2], need), case, y, grads)
        for a, b in zip(grads, full):
            assert a is None or torch.equal(a, b)


def test_backward_is_bitwise_reproducible():
    for run, case in ((lambda c: _run0(c, 0.2), _case0(4)), (_run1, _case1(4, True))):
        y1, g1 = run(case)
        y2, g2 = run(case)
        assert torch.equal(y1, y2)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)


# ---- a stack of layers through texture_branches ------------------------------------------------------------------------
STACK_SEED = 83   # widest kink margin among 0..119 on the CPU: 3.77e-4
STACK_CHANNELS = (16, 32, 16, 4)


class _Stack(nn.Module):
    def __init__(self):
        from goliath_amd import texdec

        super().__init__()
        c, s = STACK_CHANNELS, 8
        self.n_layers_tex = 3
        self.texmod0 = nn.ModuleList([texdec.Conv3WNUB(c[i], c[i + 1], s << i, s << i) for i in range(3)])
        self.texmod1 = nn.ModuleList([texdec.Conv3WN(c[i], c[i + 1]) for i in range(3)])
        with torch.no_grad():
            for m in self.texmod0:
                m.bias.normal_(0, 0.3)


def _stack_case(seed):
    torch.manual_seed(seed)
    model = _Stack()
    joint_feat, z = torch.randn(2, 16, 4, 4), torch.randn(2, 16, 4, 4)
    gainbias = [torch.randn(2, 32, 8, 8), torch.randn(2, 16, 16, 16)]
    return model, joint_feat, z, gainbias


def _stack_kink_margin(model, joint_feat):
    """Smallest |pre-activation| in front of the three LeakyReLUs of a float64 copy of the non-linear branch."""
    import copy

    from goliath_amd import texdec

    m64, x, margin = copy.deepcopy(model).double(), joint_feat.double(), []
    with torch.no_grad():
        for layer in m64.texmod0:
            pre = layer(texdec._up2(x))
            margin.append(float(pre.abs().min()))
            x = torch.nn.functional.leaky_relu(pre, 0.2)
    return min(margin)



def test_stack_operator_equals_library_lines(monkeypatch):
    """`texture_branches` on 16 -> 32 -> 16 -> 4 twin layers (4x4 inputs, outputs 8, 16 and 32 squared, gainbias for the
    first two layers, B = 2), every layer forced onto the operator against DISPATCH = {} without the override: outputs
    <= 1e-5, every parameter's gradient <= 1e-4 and non-zero, 6 operator calls against 0.  The seed was picked on the CPU
    among 0..119 for the widest kink margin of the float64 stack (asserted > 1e-6 below), so no activation mask can differ
    between the two fp32 paths."""
    from goliath_amd import texdec

    model, joint_feat, z, gainbias = _stack_case(STACK_SEED)
    margin = _stack_kink_margin(model, joint_feat)
    print("kink margin", margin)
    assert margin > 1e-6
    model, joint_feat, z = model.cuda(), joint_feat.cuda(), z.cuda()
    gainbias = [g.cuda() for g in gainbias]
    names, params = zip(*model.named_parameters())
    assert len(params) == 3 * 3 + 3 * 2
    torch.manual_seed(0)
    up = torch.randn(2, 4, 32, 32, device="cuda")
    taken = []
    lrelu, gated = texdec.upconv_lrelu, texdec.upconv_gated
    monkeypatch.setattr(texdec, "upconv_lrelu", lambda *a: (taken.append(0), lrelu(*a))[1])
    monkeypatch.setattr(texdec, "upconv_gated", lambda *a: (taken.append(1), gated(*a))[1])

    def run():
        out = texdec.texture_branches(model, joint_feat, z, gainbias, first_size=8)
        return out, torch.autograd.grad((out * up).sum(), params)

    monkeypatch.delenv("GOLIATH_FUSED_TEXDEC_ALL", raising=False)
    monkeypatch.setattr(texdec, "DISPATCH", {})
    out0, g0 = run()
    assert not taken
    monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")
    out1, g1 = run()
    assert taken == [0, 0, 0, 1, 1, 1]
    assert tuple(out1.shape) == (2, 4, 32, 32)
    e = rel_l2(out1, out0)
    print("stack out", e)
    assert e <= 1e-5
    for n, a, b in zip(names, g1, g0):
        assert float(b.norm()) > 0 and float(a.norm()) > 0, n
        e = rel_l2(a, b)
        print("stack grad", n, e)
        assert e <= 1e-4, n


# ---- through the drop-in ---------------------------------------------------------------------------------------------------
def test_patch_urhand_texture_decoder_drop_in(monkeypatch):
    """dropin.patch_urhand(texture_decoder=True) on the shaped decoder with twin layers at supported sizes (8 -> 16 at
    32^2 -> 64^2 and 16 -> 4 at 64^2 -> 128^2 in both branches): the patched forward reproduces the unpatched predictions,
    with the dispatch table as committed and with every layer forced."""
    import urhand_shaped as shaped
    from goliath_amd import dropin, texdec, urhand

    class Twin(shaped.ShapedConvTeacherDecoder):
        def __init__(self):
            super().__init__(seed=0)
            torch.manual_seed(11)
            self.init_uv_size = 32
            self.joint_conv_block_tex = nn.Conv2d(5 + 3, 8, 3, padding=1)
            self.featenc.z, self.featenc.gb = nn.Conv2d(4, 8, 3, padding=1), nn.Conv2d(4, 16, 3, padding=1)
            self.texmod0 = nn.ModuleList([texdec.Conv3WNUB(8, 16, 64, 64), texdec.Conv3WNUB(16, 4, 128, 128)])
            self.texmod1 = nn.ModuleList([texdec.Conv3WN(8, 16), texdec.Conv3WN(16, 4)])
            with torch.no_grad():
                for m in self.texmod0:
                    m.bias.normal_(0, 0.3)

    Twin.__module__ = shaped.__name__   # the forward looks its geometry helpers up in the module that defines the class
    gold = np.load(os.path.join(HERE, "golden", "urhand_model_golden.npz"))
    dec = Twin().cuda().eval()
    depths = [torch.from_numpy(gold[f"urhand_eval_depth{i}"]) for i in range(2)]
    dec.rl = shaped.ReplayRenderLayer(512, 512, depths * 3)     # three forwards, two shadow passes each
    inp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in shaped.urhand_inputs(B=1, L=2).items()}
    module = types.SimpleNamespace(ConvTeacherDecoder=Twin, get_shadow_map=None)
    taken = []
    lrelu, gated = texdec.upconv_lrelu, texdec.upconv_gated
    monkeypatch.setattr(texdec, "upconv_lrelu", lambda *a: (taken.append(0), lrelu(*a))[1])
    monkeypatch.setattr(texdec, "upconv_gated", lambda *a: (taken.append(1), gated(*a))[1])
    monkeypatch.delenv("GOLIATH_FUSED_TEXDEC_ALL", raising=False)
    try:
        with torch.no_grad():
            dropin.patch_urhand(module)
            assert Twin.forward is urhand.conv_teacher_decoder_forward and not getattr(Twin, texdec.TEXTURE_DECODER_FLAG)
            plain = dec(**inp)
            assert not taken
            assert dropin.patch_urhand(module, texture_decoder=True) is module
            assert getattr(Twin, texdec.TEXTURE_DECODER_FLAG) is True
            committed = dec(**inp)
            n_committed = len(taken)
            monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")
            forced = dec(**inp)
    finally:
        del Twin.forward
    assert n_committed <= 4 and len(taken) == n_committed + 4
    assert float(plain["tex"].abs().max()) > 0
    for out in (committed, forced):
        assert set(out) == set(plain)
        e = rel_l2(out["tex"], plain["tex"])
        print("drop-in tex", e)
        assert e <= 1e-5
