"""mvptail without a GPU: the PyTorch twin against the reference's lines written out, argument validation, the ABI."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import mvptail_cases as C

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "goliath_hip.h")


def _literal(i, mask, compact, one_channel):
    """hand_mvp.py:338-340 (+ the untied bias), :434, :472, :172-185 and render_raymarcher.py:41-47, line by line"""
    B, TD, TH, TW, ny, nx = C.SHAPES[i]
    d = C.draws(i)
    uv_y, uv_x = ny * TH, nx * TW
    alpha = (F.conv_transpose2d(d["x_alpha"], d["w_alpha"], None, 2, 1) + d["bias_alpha"][None]).view(B, TD, 1, uv_y, uv_x)
    alpha = F.relu(alpha)
    if one_channel:
        primrgba = alpha.view(B, TD, ny, TH, nx, TW).permute(0, 2, 4, 1, 3, 5).reshape(B, ny * nx, TD, TH, TW)
    else:
        rgb = (F.conv_transpose2d(d["x_rgb"], d["w_rgb"], None, 2, 1) + d["bias_rgb"][None]).view(B, TD, 3, uv_y, uv_x)
        rgb = F.relu(25.0 * rgb + 100.0)
        primrgba = torch.cat([rgb, alpha], 2).view(B, TD, 4, ny, TH, nx, TW)
        primrgba = primrgba.permute(0, 3, 5, 1, 4, 6, 2)
        primrgba = primrgba.reshape(B, ny * nx, TD, TH, TW, 4)
    if mask is None:
        return primrgba
    if compact:
        return primrgba[:, mask].contiguous()
    out = primrgba.clone()
    out[:, ~mask] = 0
    return out


@pytest.mark.parametrize("one_channel", [False, True])
@pytest.mark.parametrize("mask,compact", [(None, True), ("ends", True), ("ends", False), ("none", True)])
@pytest.mark.parametrize("i", [2, C.MASK_SHAPE])
def test_twin_is_the_references_composition(i, mask, compact, one_channel):
    from goliath_amd import mvptail

    B, TD, TH, TW, ny, nx = C.SHAPES[i]
    d = C.draws(i)
    m = None if mask is None else C.mask_of(mask, ny * nx)
    args = [None if one_channel and k.endswith("rgb") else d[k] for k in C.LEAVES]
    got = mvptail.decode_template_torch(*args, C.primsize(C.SHAPES[i]), valid_prims=m, compact=compact)
    want = _literal(i, m, compact, one_channel)
    assert got.dtype == torch.float64 and got.shape == want.shape and torch.equal(got, want)
    Kv = ny * nx if m is None or not compact else int(m.sum())
    assert got.shape[:2] == (B, Kv) and got.shape[2:5] == (TD, TH, TW)


@pytest.mark.parametrize("i", range(len(C.SHAPES)))
def test_draws_exercise_both_sides_of_both_kinks(i):
    ref = C.reference(i)
    zero = ref["out"] == 0
    assert 0.2 < float(zero[..., :3].double().mean()) < 0.8 and 0.2 < float(zero[..., 3].double().mean()) < 0.8
    assert float((~ref["keep"]).double().mean()) <= 1e-3


def _cpu_args(i=1):
    d = C.draws(i)
    return {k: d[k].float() for k in C.LEAVES}


def test_argument_validation():
    from goliath_amd import _lib, mvptail

    bad = (ValueError, _lib.GoliathHipError)
    for fn in (mvptail.decode_template, mvptail.decode_template_torch):
        a = _cpu_args(2)                                             # (3,3,3,5,2,2): h = 3, w = 5
        ps = C.primsize(C.SHAPES[2])
        with pytest.raises(bad):                                     # wrong Ci
            fn(**dict(a, x_alpha=torch.zeros(3, 8, 3, 5), x_rgb=torch.zeros(3, 8, 3, 5)), primsize=ps)
        with pytest.raises(bad):                                     # odd Sy
            fn(**dict(a, bias_alpha=torch.zeros(3, 5, 10), bias_rgb=torch.zeros(9, 5, 10)), primsize=(5, 5, 3))
        with pytest.raises(bad):                                     # TD = 11
            fn(torch.zeros(1, 16, 1, 1), torch.zeros(16, 33, 4, 4), torch.zeros(33, 2, 2), torch.zeros(1, 16, 1, 1),
               torch.zeros(16, 11, 4, 4), torch.zeros(11, 2, 2), (2, 2, 11))
        with pytest.raises(bad):                                     # a bias of the wrong size
            fn(**dict(a, bias_rgb=torch.zeros(9, 6, 9)), primsize=ps)
        with pytest.raises(bad):                                     # a mask of the wrong length
            fn(**a, primsize=ps, valid_prims=torch.ones(5, dtype=torch.bool))
        with pytest.raises(bad):
            fn(**a, primsize=ps, rgb_affine=(25.0,))
    with pytest.raises(_lib.GoliathHipError):                        # no CPU path
        mvptail.decode_template(**_cpu_args(2), primsize=C.primsize(C.SHAPES[2]))


def test_twin_runs_in_any_float_dtype():
    from goliath_amd import mvptail

    a = {k: v.to(torch.bfloat16) for k, v in _cpu_args(2).items()}
    out = mvptail.decode_template_torch(**a, primsize=C.primsize(C.SHAPES[2]))
    assert out.dtype == torch.bfloat16 and out.shape == (3, 4, 3, 3, 5, 4)


def test_header_declares_the_entries_and_the_binding_lists_them():
    from goliath_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("gol_mvp_tail_fwd", "gol_mvp_tail_bwd"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.exported_symbols()
    assert re.search(r"\blong long\s+gol_mvp_tail_bwd_scratch_floats\s*\(", hdr)
    assert "gol_mvp_tail_bwd_scratch_floats" in _lib.exported_symbols()


def test_marshallers_follow_the_header(monkeypatch):
    """the two marshallers pass exactly the parameters the header declares, in its order"""
    import inspect

    from goliath_amd import _lib, mvptail

    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for entry in ("gol_mvp_tail_fwd", "gol_mvp_tail_bwd"):
        decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", hdr).group(1)
        names = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).group(2) for p in decl.split(",")]
        fn = getattr(mvptail, "_abi_" + entry[len("gol_"):])
        assert set(inspect.signature(fn).parameters) == set(names) - {"stream"}
        calls = []
        monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
        monkeypatch.setattr(mvptail, "stream_ptr", lambda: "stream")
        monkeypatch.setattr(mvptail, "fptr", lambda t, name=None: ("p", t))
        monkeypatch.setattr(mvptail, "iptr", lambda t, name=None: ("p", t))
        fn(**{n: k for k, n in enumerate(names) if n != "stream"})
        (name, args), = calls
        assert name == entry and len(args) == len(names)
        for k, (n, a) in enumerate(zip(names, args)):
            if n == "stream":
                assert a == "stream"
            elif isinstance(a, tuple):
                assert a == ("p", k), n
            else:
                assert a.value == k, n


def test_patch_hand_mvp_fused_tail_installs_and_restores():
    import types

    from goliath_amd import dropin, mvpprims, mvptail

    class AutoEncoder:
        def render(self, K, Rt, preds, with_shadow=False):
            return "reference"

    class GeomDecoder:
        def forward(self, pose, joint, iteration=-1):
            return "reference"

    class RGBSlabDecoder:
        def forward(self, view_cos_uv, joint, ambient_occlusion):
            return "reference"

    own = RGBSlabDecoder.forward
    mod = types.SimpleNamespace(AutoEncoder=AutoEncoder, GeomDecoder=GeomDecoder, RGBSlabDecoder=RGBSlabDecoder)
    dropin.patch_hand_mvp(mod)
    assert RGBSlabDecoder.forward is own and not getattr(GeomDecoder, mvptail.FUSED_TAIL_FLAG, False)
    dropin.patch_hand_mvp(mod, fused_tail=True)
    assert RGBSlabDecoder.forward is mvptail.rgb_decoder_forward and getattr(GeomDecoder(), mvptail.FUSED_TAIL_FLAG) is True
    assert AutoEncoder.render is mvpprims.hand_mvp_render
    dropin.patch_hand_mvp(mod)
    assert RGBSlabDecoder.forward is own and getattr(GeomDecoder(), mvptail.FUSED_TAIL_FLAG) is False
