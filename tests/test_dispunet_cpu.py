"""CPU: the fused DisplacementUNet decoder level (goliath_amd.dispunet) -- the twin module and `forward` against the float64
golden of the reference's own DisplacementUNet (tests/golden/make_dispunet_golden.py), on the torch twin of the operator
and on the library lines; the leaky's adjoint at zero; the drop-in flag; the shape predicate."""
import functools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from scenes import rel_l2

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIG = dict(uv_size=64, init_uv_size=2, output_scale=3.0, pose_feat_dim=4, n_enc_dims=[8] * 6)
BAR64 = 1e-10   # float64 rounding over ~10^3-term sums, with a wide margin


@functools.lru_cache(maxsize=None)
def golden():
    g = {}
    for i in range(2):
        with np.load(os.path.join(HERE, "golden", "dispunet_golden.part%02d.npz" % i)) as f:
            g.update({k: f[k] for k in f.files})
    return g


def golden_unet(dtype=torch.float64):
    from goliath_amd import dispunet

    unet = dispunet.DisplacementUNet(**CONFIG)
    state = {k[len("state."):]: torch.from_numpy(v) for k, v in golden().items() if k.startswith("state.")}
    unet.load_state_dict(state, strict=True)
    assert sum(p.numel() for p in unet.parameters()) == 88082 and unet.sizes == [2, 4, 8, 16, 32, 64]
    return unet.to(dtype)


def _run_against_golden(unet, op):
    from goliath_amd import dispunet

    g = golden()
    t = lambda k: torch.from_numpy(g[k]).double()
    disp, rough, interm = dispunet.forward(unet, t("feat_uv"), t("pose_cond"), op=op)
    names, params = zip(*unet.named_parameters())
    grads = torch.autograd.grad((disp * t("g_disp")).sum() + (rough * t("g_roughness")).sum(), params)
    for name, got in (("disp", disp), ("roughness", rough), ("interm_feat", interm)):
        assert got.shape == g[name].shape and rel_l2(got, torch.from_numpy(g[name])) <= BAR64, name
    assert len(names) == 18 * 3
    for n, got in zip(names, grads):
        want = torch.from_numpy(g["grad." + n])
        assert float(want.norm()) > 0 and rel_l2(got, want) <= BAR64, n


def test_forward_on_the_torch_twin_equals_the_reference_golden(monkeypatch):
    from goliath_amd import dispunet

    monkeypatch.setenv("GOLIATH_FUSED_DISPUNET_ALL", "1")
    taken = []

    def op(xa, xb, w, b, leak, act):
        taken.append((tuple(xa.shape[1:]), xb.shape[1], w.shape[0], act))
        return dispunet.upcat_conv_torch(xa, xb, w, b, leak, act)

    _run_against_golden(golden_unet(), op)
    levels = [((8, 2 << i, 2 << i), 8, 8, None) for i in range(4)]
    assert taken == (levels + [((8, 32, 32), 8, 1, ("tanh", 3.0, 0.0))]
                     + levels + [((8, 32, 32), 8, 1, ("tanh", 0.25, 0.55))])


def test_forward_on_the_library_lines_equals_the_reference_golden(monkeypatch):
    from goliath_amd import dispunet

    monkeypatch.delenv("GOLIATH_FUSED_DISPUNET_ALL", raising=False)
    monkeypatch.setattr(dispunet, "DISPATCH", {})
    _run_against_golden(golden_unet(), lambda *a: pytest.fail("nothing is admitted"))
    # the twin module's own forward is the same composition
    g = golden()
    with torch.no_grad():
        disp, rough, _ = golden_unet()(torch.from_numpy(g["feat_uv"]).double(), torch.from_numpy(g["pose_cond"]).double())
    assert rel_l2(disp, torch.from_numpy(g["disp"])) <= BAR64 and rel_l2(rough, torch.from_numpy(g["roughness"])) <= BAR64


@pytest.mark.parametrize("Hi,Wi", [(1, 1), (3, 5), (17, 33)])
def test_integer_ratio_resize_is_align_corners_bilinear(Hi, Wi):
    from goliath_amd import dispunet

    torch.manual_seed(2)
    x = torch.randn(2, 3, Hi, Wi, dtype=torch.float64)
    want = torch.nn.functional.interpolate(x, (2 * Hi, 2 * Wi), mode="bilinear", align_corners=True)
    assert rel_l2(dispunet.up2_integer(x), want) <= 1e-12


def test_a_zero_in_xa_takes_leak_times_the_incoming_gradient():
    from goliath_amd import dispunet

    torch.manual_seed(5)
    xa = torch.randn(2, 8, 3, 4, dtype=torch.float64)
    xa[0, 1, 2, 3] = xa[1, 7, 0, 0] = xa[1, 0, 1, 2] = 0.0
    zero = xa == 0
    xb, w = torch.randn(2, 8, 6, 8, dtype=torch.float64), torch.randn(4, 16, 3, 3, dtype=torch.float64)
    bias, up = torch.randn(4, 6, 8, dtype=torch.float64), torch.randn(2, 4, 6, 8, dtype=torch.float64)
    xa.requires_grad_(True)
    g_xa, = torch.autograd.grad((dispunet.upcat_conv_torch(xa, xb, w, bias, 0.2, ("tanh", 0.25, 0.55)) * up).sum(), xa)
    # the gradient that arrives at L = lrelu(xa): the same composition from L on
    L = torch.nn.functional.leaky_relu(xa.detach(), 0.2).requires_grad_(True)
    y = torch.nn.functional.conv2d(torch.cat([dispunet.up2_integer(L), xb], 1), w, None, 1, 1) + bias[None]
    g_L, = torch.autograd.grad(((torch.tanh(y) * 0.25 + 0.55) * up).sum(), L)
    assert int(zero.sum()) == 3 and float(g_L[zero].abs().min()) > 0
    assert torch.allclose(g_xa[zero], 0.2 * g_L[zero], rtol=1e-13, atol=0)
    pos = xa.detach() > 0
    assert torch.allclose(g_xa[pos], g_L[pos], rtol=1e-13, atol=0)


def _decoder_calls(monkeypatch, refiner, **flags):
    """How often `dispunet.forward` / the refiner module run when the patched decoder forward reaches the refiner."""
    from goliath_amd import dispunet, dropin

    class Stop(Exception):
        pass

    calls = {"forward": 0, "module": 0}

    def fake_forward(unet, feat_uv, pose_cond):
        assert unet is refiner
        calls["forward"] += 1
        raise Stop

    def module_forward(feat_uv, pose_cond):
        calls["module"] += 1
        raise Stop

    monkeypatch.setattr(dispunet, "forward", fake_forward)
    refiner.forward = module_forward
    import urhand_shaped as shaped

    class Dec(shaped.ShapedConvTeacherDecoder):
        pass

    Dec.__module__ = shaped.__name__
    dec = Dec(seed=0).eval()
    dec.shadow = False
    dec.geo_refiner = refiner
    module = types.SimpleNamespace(ConvTeacherDecoder=Dec, get_shadow_map=None)
    dropin.patch_urhand(module, **flags)
    assert getattr(Dec, dispunet.DISPLACEMENT_UNET_FLAG) is bool(flags.get("displacement_unet", False))
    try:
        with torch.no_grad(), pytest.raises(Stop):
            dec(**shaped.urhand_inputs(B=1, L=2))
    finally:
        del Dec.forward
    return calls


def _uvlight_on_cpu(monkeypatch):
    """The stretch in front of the refiner call runs the Phong light loop on a HIP kernel: stand in for it on the CPU."""
    from goliath_amd import uvlight

    monkeypatch.setattr(uvlight, "phong_features", lambda p_uv, *a, **k: (p_uv[:, :1], p_uv[:, :1]))


def test_patch_urhand_displacement_unet_flag_routes_the_refiner(monkeypatch):
    from goliath_amd import dispunet

    _uvlight_on_cpu(monkeypatch)
    twin = dispunet.DisplacementUNet(**CONFIG)
    assert _decoder_calls(monkeypatch, twin, displacement_unet=True) == {"forward": 1, "module": 0}
    assert _decoder_calls(monkeypatch, twin) == {"forward": 0, "module": 1}
    other = nn.Module()                                  # a refiner without dec_layers_roughness is called as a module
    other.enc_layers, other.dec_layers = twin.enc_layers, twin.dec_layers
    assert _decoder_calls(monkeypatch, other, displacement_unet=True) == {"forward": 0, "module": 1}


@pytest.mark.parametrize("Ca,Cb,Co", [(12, 8, 16), (8, 0, 16), (8, 8, 5)])
def test_upcat_conv_refuses_unsupported_shapes_before_any_launch(monkeypatch, Ca, Cb, Co):
    from goliath_amd import _lib, dispunet

    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a launch"))
    assert not dispunet.supported(Ca, Cb, Co, 2, 2)
    with pytest.raises(_lib.GoliathHipError, match="unsupported"):
        dispunet.upcat_conv(torch.zeros(1, Ca, 2, 2), torch.zeros(1, Cb, 4, 4), torch.zeros(Co, Ca + Cb, 3, 3),
                            torch.zeros(Co, 4, 4))


def test_supported_shapes_and_the_dispatch_table():
    from goliath_amd import _lib, dispunet

    for hi in (32, 64, 128, 256):                        # the model's levels (urhand_mesh_example.yml: 64 channels)
        assert dispunet.supported(64, 64, 64, hi, hi)
    assert dispunet.supported(64, 64, 1, 512, 512) and dispunet.supported(8, 8, 8, 1, 1)
    assert not dispunet.supported(0, 8, 16, 4, 4) and not dispunet.supported(8, 8, 16, 0, 4)
    assert all(len(k) == 5 and v is True and dispunet.supported(*k) for k, v in dispunet.DISPATCH.items())
    with pytest.raises(_lib.GoliathHipError, match="no CPU path"):
        dispunet.upcat_conv(torch.zeros(1, 8, 2, 2), torch.zeros(1, 8, 4, 4), torch.zeros(16, 16, 3, 3), torch.zeros(16, 4, 4))


def test_header_declares_and_binding_exports_the_entries():
    import re

    from goliath_amd import _lib

    root = os.path.dirname(HERE)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "goliath_hip.h")).read(), flags=re.S)
    for name in ("gol_upcat_conv_fwd", "gol_upcat_conv_bwd_scratch_floats", "gol_upcat_conv_bwd"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.exported_symbols(), name
