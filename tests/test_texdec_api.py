"""CPU: the fused texture-decoder layer (goliath_amd.texdec) -- ABI declaration, the torch twins against the layers they
replace, the coordinate rule, the shape predicate, what `texture_branches` recognises and the drop-in flag."""
import os
import re
import sys
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from scenes import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
ENTRIES = ("gol_upconv_fwd", "gol_upconv_bwd_scratch_floats", "gol_upconv_bwd")
GPU_SHAPES = [(2, 8, 16, 1, 1), (3, 16, 4, 3, 5), (2, 24, 16, 5, 7), (1, 136, 32, 6, 6), (2, 64, 32, 17, 33),
              (2, 16, 4, 32, 40), (9, 8, 16, 3, 2), (2, 32, 48, 9, 4)]       # tests/test_gpu_texdec.py


def _ref_layers():
    sys.path.insert(0, REF)
    try:
        import ca_code.nn.layers as la
    finally:
        sys.path.remove(REF)
    return la


def _randomise(layer):
    with torch.no_grad():
        layer.weight_v.normal_()
        layer.weight_g.uniform_(0.5, 1.5)
        if layer.bias is not None:
            layer.bias.normal_(0, 0.5)
    return layer


def _up(x, hh, ww):
    return F.interpolate(x, (hh, ww), mode="bilinear", align_corners=True)


def test_header_declares_and_binding_exports_the_entries():
    from goliath_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goliath_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.exported_symbols(), name


def test_torch_twins_equal_the_twin_layers():
    from goliath_amd import tail, texdec

    torch.manual_seed(0)
    ub, wn = _randomise(texdec.Conv3WNUB(24, 16, 10, 14)), _randomise(texdec.Conv3WN(24, 16))
    x, gate, gb = torch.randn(3, 24, 5, 7), torch.randn(3, 16, 10, 14), torch.randn(3, 16, 10, 14)
    ref = F.leaky_relu(ub(_up(x, 10, 14)), 0.2)
    got = texdec.upconv_lrelu_torch(x, tail.wn_weight(ub), ub.bias, 0.2)
    assert got.shape == ref.shape == (3, 16, 10, 14)
    assert rel_l2(got, ref) <= 1e-6
    ref = (wn(_up(x, 10, 14)) * gate + gb) * 0.707107
    assert rel_l2(texdec.upconv_gated_torch(x, tail.wn_weight(wn), gate, gb), ref) <= 1e-6
    ref = wn(_up(x, 10, 14)) * gate
    assert rel_l2(texdec.upconv_gated_torch(x, tail.wn_weight(wn), gate, None, 1.0), ref) <= 1e-6
    assert [k for k, _ in wn.named_parameters()] == ["weight_v", "weight_g"] and wn.bias is None


@needs_ref
def test_torch_twins_equal_the_reference_layers():
    from goliath_amd import tail, texdec

    la = _ref_layers()
    torch.manual_seed(1)
    ub = _randomise(la.Conv2dWNUB(24, 16, 10, 14, 3, 1, 1))
    wn = _randomise(la.Conv2dWN(24, 16, 3, 1, 1, bias=False))
    x, gate, gb = torch.randn(3, 24, 5, 7), torch.randn(3, 16, 10, 14), torch.randn(3, 16, 10, 14)
    ref = F.leaky_relu(ub(_up(x, 10, 14)), 0.2)                                  # urhand.py:592-597
    assert rel_l2(texdec.upconv_lrelu_torch(x, tail.wn_weight(ub), ub.bias, 0.2), ref) <= 1e-6
    ref = (wn(_up(x, 10, 14)) * gate + gb) * 0.707107                            # urhand.py:600-606
    assert rel_l2(texdec.upconv_gated_torch(x, tail.wn_weight(wn), gate, gb), ref) <= 1e-6
    # state dicts load both ways
    twin_ub, twin_wn = texdec.Conv3WNUB(24, 16, 10, 14), texdec.Conv3WN(24, 16)
    twin_ub.load_state_dict(ub.state_dict())
    twin_wn.load_state_dict(wn.state_dict())
    up = _up(x, 10, 14)
    assert rel_l2(twin_ub(up), ub(up)) <= 1e-6 and rel_l2(twin_wn(up), wn(up)) <= 1e-6
    back_ub, back_wn = la.Conv2dWNUB(24, 16, 10, 14, 3, 1, 1), la.Conv2dWN(24, 16, 3, 1, 1, bias=False)
    back_ub.load_state_dict(_randomise(twin_ub).state_dict())
    back_wn.load_state_dict(_randomise(twin_wn).state_dict())
    assert rel_l2(back_ub(up), twin_ub(up)) <= 1e-6 and rel_l2(back_wn(up), twin_wn(up)) <= 1e-6
    assert texdec._is_conv3_wn(ub, True) and texdec._is_conv3_wn(wn, False)
    assert not texdec._is_conv3_wn(ub, False) and not texdec._is_conv3_wn(wn, True)
    assert not texdec._is_conv3_wn(la.Conv2dWNUB(24, 16, 5, 7, 4, 2, 1), True)   # 4x4 stride 2
    assert not texdec._is_conv3_wn(la.Conv2dWN(24, 16, 3, 1, 1), True)           # tied bias


def _integer_rule_up2(x):
    """The integer-ratio rule of include/goliath_hip.h stated in float64 torch."""
    Hi, Wi = x.shape[2:]

    def axis(n):
        no = 2 * n
        r = torch.arange(no)
        nr = r * (n - 1)
        a = nr // (no - 1)
        f = (nr - a * (no - 1)).double() / float(no - 1)
        return a, torch.clamp(a + 1, max=n - 1), f

    ra, rb, rf = axis(Hi)
    ca, cb, cf = axis(Wi)
    rows = x[:, :, ra] * (1 - rf)[:, None] + x[:, :, rb] * rf[:, None]
    return rows[:, :, :, ca] * (1 - cf) + rows[:, :, :, cb] * cf


@pytest.mark.parametrize("Hi,Wi", [(1, 1), (2, 3), (3, 2), (17, 33)] + [s[3:] for s in GPU_SHAPES])
def test_integer_ratio_rule_is_align_corners_bilinear(Hi, Wi):
    torch.manual_seed(2)
    x = torch.randn(2, 3, Hi, Wi, dtype=torch.float64)
    want = _up(x, 2 * Hi, 2 * Wi)
    assert float((_integer_rule_up2(x) - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert rel_l2(_integer_rule_up2(x), want) <= 1e-12


def _first_row(i, nsrc, nout):
    """csrc/upconv.hip: up_first_row -- the first row of U that can reach source row i."""
    return 0 if (i <= 0 or nsrc <= 1) else ((i - 1) * (nout - 1)) // (nsrc - 1) + 1


@pytest.mark.parametrize("tile,region", [(4, 12), (16, 36)])
def test_input_gradient_region_holds_every_contributing_row(tile, region):
    """The input gradient gathers, per source row i, from the 5 rows of U starting at up_first_row(i), inside a region of
    12 rows (36 columns) per tile of 4 (16) source rows (columns) starting at up_first_row(tile origin): every row of U
    that the coordinate rule blends into row i lies inside both, for every tile of every size."""
    for n in list(range(1, 201)) + [1024, 2048, 2049, 4095, 4096]:
        nout = 2 * n
        reach = {}
        for r in range(nout):
            nr, d = r * (n - 1), nout - 1
            a = nr // d
            if nr - a * d < d:                  # weight 1 - frac > 0
                reach.setdefault(a, []).append(r)
            if nr - a * d > 0:                  # weight frac > 0
                reach.setdefault(min(a + 1, n - 1), []).append(r)
        for i0 in range(0, n, tile):
            lo0 = _first_row(i0, n, nout)
            for i in range(i0, min(i0 + tile, n)):
                lo = _first_row(i, n, nout)
                assert lo >= lo0
                for r in reach[i]:
                    assert lo <= r < lo + 5 and lo0 <= r < lo0 + region, (n, i0, i, r)


def test_supported_shapes():
    from goliath_amd import texdec

    size = 32
    for ci, co in texdec.CHANNELS:
        assert texdec.supported(ci, co, size, size), (ci, co)
        size *= 2
    assert size == 4096 and texdec.CHANNELS[0] == (128, 256) and texdec.CHANNELS[-1] == (16, 4)
    for _, ci, co, hi, wi in GPU_SHAPES:
        assert texdec.supported(ci, co, hi, wi), (ci, co, hi, wi)
    assert not texdec.supported(12, 16, 8, 8)
    assert not texdec.supported(16, 8, 8, 8)
    assert not texdec.supported(16, 16, 0, 8)
    assert all(len(k) == 5 and v is True for k, v in texdec.DISPATCH.items())


def test_hip_operators_refuse_cpu_tensors_and_bad_shapes():
    from goliath_amd import _lib, texdec

    x, w = torch.zeros(1, 16, 4, 4), torch.zeros(16, 16, 3, 3)
    with pytest.raises(_lib.GoliathHipError):
        texdec.upconv_lrelu(x, w, torch.zeros(16, 8, 8))
    with pytest.raises(_lib.GoliathHipError):
        texdec.upconv_gated(x, w, torch.zeros(1, 16, 8, 8))
    with pytest.raises(_lib.GoliathHipError):
        texdec.upconv_gated(x, w, torch.zeros(1, 16, 8, 8), torch.zeros(1, 16, 8, 8))


def _stack(plain=False):
    from goliath_amd import texdec

    dec = nn.Module()
    dec.n_layers_tex = 3
    if plain:
        dec.texmod0 = nn.ModuleList([nn.Conv2d(16, 32, 3, padding=1), nn.Conv2d(32, 16, 3, padding=1), nn.Conv2d(16, 4, 3, padding=1)])
        dec.texmod1 = nn.ModuleList([nn.Conv2d(16, 32, 3, padding=1, bias=False), nn.Conv2d(32, 16, 3, padding=1, bias=False),
                                     nn.Conv2d(16, 4, 3, padding=1, bias=False)])
    else:
        dec.texmod0 = nn.ModuleList([_randomise(texdec.Conv3WNUB(16, 32, 8, 8)), _randomise(texdec.Conv3WNUB(32, 16, 16, 16)),
                                     _randomise(texdec.Conv3WNUB(16, 4, 32, 32))])
        dec.texmod1 = nn.ModuleList([_randomise(texdec.Conv3WN(16, 32)), _randomise(texdec.Conv3WN(32, 16)),
                                     _randomise(texdec.Conv3WN(16, 4))])
    return dec


def _library_lines(dec, joint_feat, z, gainbias, first_size):
    """goliath_amd/urhand.py's two loops (the reference's urhand.py:583-608) with the first output size as a parameter."""
    acts, x, hh = [], joint_feat, first_size
    for i in range(dec.n_layers_tex):
        x = F.interpolate(x, (hh, hh), mode="bilinear", align_corners=True)
        x = F.leaky_relu(dec.texmod0[i](x), 0.2)
        acts.append(x)
        hh *= 2
    x, hh = z, first_size
    for i in range(dec.n_layers_tex):
        x = F.interpolate(x, (hh, hh), mode="bilinear", align_corners=True)
        x = dec.texmod1[i](x) * acts[i]
        hh *= 2
        if i < len(gainbias):
            x = (x + gainbias[i]) * 0.707107
    return x


def test_texture_branches_on_cpu_is_the_library_lines(monkeypatch):
    from goliath_amd import texdec

    monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")     # even when forced: CPU tensors take the library lines
    torch.manual_seed(3)
    dec = _stack()
    joint_feat, z = torch.randn(2, 16, 4, 4), torch.randn(2, 16, 4, 4)
    gainbias = [torch.randn(2, 32, 8, 8), torch.randn(2, 16, 16, 16)]
    with torch.no_grad():
        assert torch.equal(texdec.texture_branches(dec, joint_feat, z, gainbias, first_size=8),
                           _library_lines(dec, joint_feat, z, gainbias, 8))
        # the model's first size: 64 (the inputs are then resized by 16x, not 2x)
        dec.texmod0[0].bias = nn.Parameter(torch.randn(32, 64, 64))
        dec.texmod0[1].bias = nn.Parameter(torch.randn(16, 128, 128))
        dec.texmod0[2].bias = nn.Parameter(torch.randn(4, 256, 256))
        assert torch.equal(texdec.texture_branches(dec, joint_feat, z, []), _library_lines(dec, joint_feat, z, [], 64))


def _record(monkeypatch, texdec):
    """Which layers would go to the HIP operators: pretend the tensors are on the GPU, record the calls instead of
    launching."""
    taken = []
    monkeypatch.setattr(texdec, "_on_gpu", lambda *tensors: True)

    def lrelu(x, w, b, leak=0.2):
        taken.append((0, tuple(w.shape), tuple(x.shape[2:]), leak))
        return texdec.upconv_lrelu_torch(x, w, b, leak)

    def gated(x, w, gate, gb=None, scale=texdec.GAIN_SCALE):
        taken.append((1, tuple(w.shape), tuple(x.shape[2:]), gb is not None, scale))
        return texdec.upconv_gated_torch(x, w, gate, gb, scale)

    monkeypatch.setattr(texdec, "upconv_lrelu", lrelu)
    monkeypatch.setattr(texdec, "upconv_gated", gated)
    return taken


def test_texture_branches_takes_exactly_the_wn_3x3_layers_with_half_size_inputs(monkeypatch):
    from goliath_amd import encoder, texdec

    torch.manual_seed(4)
    monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")
    taken = _record(monkeypatch, texdec)
    dec = _stack()
    joint_feat, z = torch.randn(2, 16, 4, 4), torch.randn(2, 16, 4, 4)
    gainbias = [torch.randn(2, 32, 8, 8), torch.randn(2, 16, 16, 16)]
    with torch.no_grad():
        got, ref = texdec.texture_branches(dec, joint_feat, z, gainbias, first_size=8), _library_lines(dec, joint_feat, z, gainbias, 8)
    assert taken == [(0, (32, 16, 3, 3), (4, 4), 0.2), (0, (16, 32, 3, 3), (8, 8), 0.2), (0, (4, 16, 3, 3), (16, 16), 0.2),
                     (1, (32, 16, 3, 3), (4, 4), True, 0.707107), (1, (16, 32, 3, 3), (8, 8), True, 0.707107),
                     (1, (4, 16, 3, 3), (16, 16), False, 1.0)]
    assert rel_l2(got, ref) <= 1e-6
    # not taken: an input that is not hh/2 (the first layer of either branch here), a plain nn.Conv2d (second layer of
    # texmod0), a tied bias in texmod0 (third layer: a bias-free WN layer where an untied bias belongs)
    del taken[:]
    dec.texmod0[1] = nn.Conv2d(32, 16, 3, padding=1)
    dec.texmod0[2] = _randomise(texdec.Conv3WN(16, 4))
    tied = _randomise(texdec.Conv3WN(16, 4))
    tied.bias = nn.Parameter(torch.randn(4))           # a tied, 1-D bias: neither an untied 3-D one nor none
    assert not texdec._is_conv3_wn(tied, True) and not texdec._is_conv3_wn(tied, False)
    assert not texdec._is_conv3_wn(dec.texmod0[2], True)
    jf2, z2 = torch.randn(2, 16, 2, 2), torch.randn(2, 16, 2, 2)
    with torch.no_grad():
        got, ref = texdec.texture_branches(dec, jf2, z2, gainbias, first_size=8), _library_lines(dec, jf2, z2, gainbias, 8)
    assert taken == [(1, (16, 32, 3, 3), (8, 8), True, 0.707107), (1, (4, 16, 3, 3), (16, 16), False, 1.0)]
    assert torch.equal(got, ref) or rel_l2(got, ref) <= 1e-6
    # a 4x4 / stride 2 Conv2dWNUB is not this operator's layer; plain layers are never taken
    assert not texdec._is_conv3_wn(encoder.Conv2dWNUB(16, 16, 4, 4), True)
    del taken[:]
    plain = _stack(plain=True)
    with torch.no_grad():
        assert torch.equal(texdec.texture_branches(plain, joint_feat, z, gainbias, first_size=8),
                           _library_lines(plain, joint_feat, z, gainbias, 8))
    assert not taken
    # without the override only DISPATCH admits
    monkeypatch.delenv("GOLIATH_FUSED_TEXDEC_ALL")
    monkeypatch.setattr(texdec, "DISPATCH", {(1, 32, 16, 8, 8): True})
    dec = _stack()
    with torch.no_grad():
        texdec.texture_branches(dec, joint_feat, z, gainbias, first_size=8)
    assert taken == [(1, (16, 32, 3, 3), (8, 8), True, 0.707107)]


def test_patch_urhand_flag_is_idempotent_and_default_is_unchanged():
    import inspect

    from goliath_amd import dropin, texdec, urhand

    class ConvTeacherDecoder:
        pass

    stand_in = types.SimpleNamespace(ConvTeacherDecoder=ConvTeacherDecoder, get_shadow_map=None)
    assert inspect.signature(dropin.patch_urhand).parameters["texture_decoder"].default is False
    assert dropin.patch_urhand(stand_in, texture_decoder=True) is stand_in
    assert dropin.patch_urhand(stand_in, texture_decoder=True) is stand_in
    assert getattr(ConvTeacherDecoder, texdec.TEXTURE_DECODER_FLAG) is True
    assert ConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward
    dropin.patch_urhand(stand_in, uv_frames=True, texture_decoder=True)
    assert ConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward_uv_frames
    assert getattr(ConvTeacherDecoder, texdec.TEXTURE_DECODER_FLAG) is True
    dropin.patch_urhand(stand_in)                                   # and back: the default binding clears the flag
    assert getattr(ConvTeacherDecoder, texdec.TEXTURE_DECODER_FLAG) is False
    assert ConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward


def test_shaped_decoder_texture_lines_are_bitwise_unchanged_by_the_flag(monkeypatch):
    """The tail of the decoder forward on the shaped decoder's plain nn.Conv2d layers (CPU): with the flag set, with the
    override, `texture_branches` returns what the forward's own lines return, bit for bit."""
    import urhand_shaped as shaped
    from goliath_amd import texdec

    monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")
    dec = shaped.ShapedConvTeacherDecoder(seed=0).eval()
    torch.manual_seed(5)
    joint_feat = dec.joint_conv_block_tex(torch.randn(1, 8, 8, 8))
    z, gainbias = dec.featenc(torch.randn(1, 4, 64, 64))
    with torch.no_grad():
        assert torch.equal(texdec.texture_branches(dec, joint_feat, z, gainbias), _library_lines(dec, joint_feat, z, gainbias, 64))
