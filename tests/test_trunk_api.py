"""CPU: the fused hidden-decoder-layer operator (goliath_amd.trunk) -- ABI declaration, the torch twin against the layer it
replaces, the shape predicate, the opt-in switch of `PrimDecoderConvs.trunk` and what `run_stack` recognises."""
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

from scenes import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
ENTRIES = ("gol_trunk_conv_fwd", "gol_trunk_conv_bwd_scratch_floats", "gol_trunk_conv_bwd")
REFERENCE_PAIRS = [(256, 256), (264, 256), (256, 128), (128, 128), (128, 64), (64, 32), (32, 16)]  # rgca.py:408-454


def test_header_declares_and_binding_exports_the_entries():
    from goliath_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goliath_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.exported_symbols(), name


def test_torch_twin_equals_layer_then_leaky_relu():
    from goliath_amd import decoder, tail, trunk

    torch.manual_seed(0)
    layer = decoder.ConvTranspose2dWNUB(24, 16, 10, 14)
    with torch.no_grad():
        layer.weight_v.normal_()
        layer.weight_g.uniform_(0.5, 1.5)
        layer.bias.normal_(0, 0.5)
    x = torch.randn(3, 24, 5, 7)
    ref = nn.LeakyReLU(0.2)(layer(x))
    got = trunk.convt_ub_lrelu_torch(x, tail.wn_weight(layer), layer.bias, 0.2)
    assert got.shape == ref.shape == (3, 16, 10, 14)
    assert rel_l2(got, ref) <= 1e-6


def test_hip_operator_refuses_cpu_tensors():
    from goliath_amd import _lib, trunk

    with pytest.raises(_lib.GoliathHipError):
        trunk.convt_ub_lrelu(torch.zeros(1, 16, 2, 2), torch.zeros(16, 16, 4, 4), torch.zeros(16, 4, 4))


def test_supported_shapes():
    from goliath_amd import trunk

    for ci, co in REFERENCE_PAIRS:
        assert trunk.supported(ci, co), (ci, co)
    assert not trunk.supported(12, 16)
    assert not trunk.supported(16, 8)


def test_switch_leaves_the_cpu_trunk_unchanged(monkeypatch):
    from goliath_amd import decoder

    torch.manual_seed(1)
    dec = decoder.PrimDecoderConvs(base=1)
    with torch.no_grad():
        for m in dec.modules():
            if isinstance(m, decoder.ConvTranspose2dWNUB):
                m.bias.normal_(0, 0.3)
    embs, campos = torch.randn(2, 256), torch.randn(2, 3)
    monkeypatch.delenv("GOLIATH_FUSED_TRUNK", raising=False)
    with torch.no_grad():
        off = dec.trunk(embs, campos)
        monkeypatch.setenv("GOLIATH_FUSED_TRUNK", "1")
        monkeypatch.setenv("GOLIATH_FUSED_TRUNK_ALL", "1")   # even when forced: CPU tensors take the module path
        on = dec.trunk(embs, campos)
    for a, b in zip(on, off):
        assert a.shape == b.shape and torch.equal(a, b)


def test_run_stack_calls_other_modules_unchanged(monkeypatch):
    from goliath_amd import trunk

    monkeypatch.setenv("GOLIATH_FUSED_TRUNK_ALL", "1")
    torch.manual_seed(2)
    calls = []

    class Probe(nn.Identity):
        def forward(self, x):
            calls.append(tuple(x.shape))
            return x

    conv3 = nn.ConvTranspose2d(16, 16, 3, 1, 1)   # a transposed conv, but 3x3 / stride 1 and no weight norm
    seq = nn.Sequential(Probe(), conv3, nn.LeakyReLU(0.2), nn.Conv2d(16, 8, 3, 1, 1), Probe())
    x = torch.randn(2, 16, 5, 6)
    with torch.no_grad():
        assert torch.equal(trunk.run_stack(seq, x), seq(x))
    assert calls == [(2, 16, 5, 6), (2, 8, 5, 6)] * 2
    assert not trunk._is_convt_wnub(conv3) and not trunk._is_convt_wnub(seq[0])


@needs_ref
def test_run_stack_recognises_the_reference_layers(monkeypatch):
    from goliath_amd import decoder, trunk

    sys.path.insert(0, REF)
    try:
        import ca_code.nn.layers as la
    finally:
        sys.path.remove(REF)
    torch.manual_seed(3)
    seq = nn.Sequential(*la.make_conv_trans(24, 16, 4, 2, 1, "wn", nn.LeakyReLU(0.2, inplace=True), ub=(10, 14)),
                        *la.make_conv_trans(16, 16, 4, 2, 1, "wn", ub=(20, 28)))
    assert trunk._is_convt_wnub(seq[0]) and isinstance(seq[1], nn.LeakyReLU) and trunk._is_convt_wnub(seq[2])
    assert trunk._is_convt_wnub(decoder.ConvTranspose2dWNUB(8, 16, 4, 4))
    # the non-transposed sibling has the same parameter names and a 4x4 / stride 2 kernel: it is not taken
    assert not trunk._is_convt_wnub(la.Conv2dWNUB(16, 16, 5, 7, 4, 2, 1))
    # which pairs would go to the HIP operator: record the calls instead of launching
    taken = []
    monkeypatch.setenv("GOLIATH_FUSED_TRUNK_ALL", "1")
    monkeypatch.setattr(trunk, "_takes_hip", lambda layer, x: True)
    monkeypatch.setattr(trunk, "convt_ub_lrelu", lambda x, w, b, leak: (taken.append((tuple(w.shape), leak)),
                                                                         trunk.convt_ub_lrelu_torch(x, w, b, leak))[1])
    x = torch.randn(2, 24, 5, 7)
    with torch.no_grad():
        got, ref = trunk.run_stack(seq, x), seq(x)
    assert taken == [((24, 16, 4, 4), 0.2)]          # the last layer has no activation behind it: a module call
    assert rel_l2(got, ref) <= 1e-6
