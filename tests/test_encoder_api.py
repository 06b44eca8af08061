"""CPU: the fused encoder-layer operator (goliath_amd.encoder) -- ABI declaration, the torch twin against the layer it
replaces, the shape predicate, what `run_stack` recognises, the `Encoder` twin against the reference's and the drop-in."""
import copy
import os
import re
import sys
import types

import pytest
import torch
import torch.nn as nn

from scenes import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
ENTRIES = ("gol_enc_conv_fwd", "gol_enc_conv_bwd_scratch_floats", "gol_enc_conv_bwd")
REFERENCE_PAIRS = [(3, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256)]  # rgca.py:281-298


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
        layer.bias.normal_(0, 0.5)
    return layer


def test_header_declares_and_binding_exports_the_entries():
    from goliath_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goliath_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.exported_symbols(), name


def test_torch_twin_equals_layer_then_leaky_relu():
    from goliath_amd import encoder, tail

    torch.manual_seed(0)
    layer = _randomise(encoder.Conv2dWNUB(24, 16, 5, 7))
    x = torch.randn(3, 24, 10, 14)
    ref = nn.LeakyReLU(0.2)(layer(x))
    got = encoder.conv_ub_lrelu_torch(x, tail.wn_weight(layer), layer.bias, 0.2)
    assert got.shape == ref.shape == (3, 16, 5, 7)
    assert rel_l2(got, ref) <= 1e-6


@needs_ref
def test_torch_twin_equals_the_reference_layer():
    from goliath_amd import encoder, tail

    la = _ref_layers()
    torch.manual_seed(1)
    layer = _randomise(la.Conv2dWNUB(24, 16, 5, 7, 4, 2, 1))
    x = torch.randn(3, 24, 10, 14)
    ref = nn.LeakyReLU(0.2)(layer(x))
    assert rel_l2(encoder.conv_ub_lrelu_torch(x, tail.wn_weight(layer), layer.bias, 0.2), ref) <= 1e-6
    color = 255.0 * torch.rand(3, 24, 10, 14)
    ref = nn.LeakyReLU(0.2)(layer(color / 255.0 - 0.5))          # rgca.py:314
    got = encoder.conv_ub_lrelu_torch(color, tail.wn_weight(layer), layer.bias, 0.2, 1.0 / 255.0, -0.5)
    assert rel_l2(got, ref) <= 1e-6
    twin = encoder.Conv2dWNUB(24, 16, 5, 7)
    twin.load_state_dict(layer.state_dict())                      # same keys, same shapes
    assert rel_l2(twin(x), layer(x)) <= 1e-6


def test_supported_shapes():
    from goliath_amd import encoder

    size = 1024
    for ci, co in REFERENCE_PAIRS:
        assert encoder.supported(ci, co, size, size), (ci, co)
        size //= 2
    assert encoder.supported(1, 16, 2, 2) and encoder.supported(4, 16, 6, 4) and encoder.supported(136, 32, 12, 12)
    assert not encoder.supported(12, 16, 8, 8)
    assert not encoder.supported(5, 16, 8, 8)
    assert not encoder.supported(16, 8, 8, 8)
    assert not encoder.supported(16, 16, 7, 8)
    assert not encoder.supported(16, 16, 8, 9)


def test_hip_operator_refuses_cpu_tensors():
    from goliath_amd import _lib, encoder

    with pytest.raises(_lib.GoliathHipError):
        encoder.conv_ub_lrelu(torch.zeros(1, 16, 4, 4), torch.zeros(16, 16, 4, 4), torch.zeros(16, 2, 2))


def test_run_stack_on_cpu_is_the_sequential(monkeypatch):
    from goliath_amd import encoder

    monkeypatch.setenv("GOLIATH_FUSED_ENCODER_ALL", "1")     # even when forced: CPU tensors take the module path
    torch.manual_seed(2)
    seq = nn.Sequential(_randomise(encoder.Conv2dWNUB(3, 16, 6, 4)), nn.LeakyReLU(0.2, inplace=True),
                        _randomise(encoder.Conv2dWNUB(16, 16, 3, 2)), nn.LeakyReLU(0.2, inplace=True))
    x = torch.randn(2, 3, 12, 8)
    with torch.no_grad():
        assert torch.equal(encoder.run_stack(seq, x), seq(x))
        assert torch.equal(encoder.run_stack(seq, x, 0.5, -0.25), seq(x * 0.5 - 0.25))


def _record(monkeypatch, encoder):
    """Which pairs would go to the HIP operator: record the calls instead of launching."""
    taken = []
    monkeypatch.setattr(encoder, "_takes_hip", lambda layer, x: True)

    def fake(x, w, b, leak=0.2, in_scale=1.0, in_shift=0.0):
        taken.append((tuple(w.shape), leak, in_scale, in_shift))
        return encoder.conv_ub_lrelu_torch(x, w, b, leak, in_scale, in_shift)

    monkeypatch.setattr(encoder, "conv_ub_lrelu", fake)
    return taken


def test_run_stack_takes_exactly_the_conv_lrelu_pairs(monkeypatch):
    from goliath_amd import decoder, encoder

    torch.manual_seed(3)
    taken = _record(monkeypatch, encoder)

    class Conv3WNUB(nn.Module):   # a weight-normalised conv with an untied bias, but 3x3 / stride 1
        def __init__(self, n_in, n_out, height, width):
            super().__init__()
            self.weight_v = nn.Parameter(torch.randn(n_out, n_in, 3, 3))
            self.weight_g = nn.Parameter(torch.rand(n_out, 1, 1, 1) + 0.5)
            self.bias = nn.Parameter(torch.randn(n_out, height, width))

        def forward(self, x):
            w = self.weight_v * (self.weight_g / self.weight_v.norm())
            return torch.nn.functional.conv2d(x, w, None, 1, 1) + self.bias[None]

    seq = nn.Sequential(
        _randomise(encoder.Conv2dWNUB(3, 16, 8, 12)), nn.LeakyReLU(0.2),            # taken (with the affine)
        Conv3WNUB(16, 16, 8, 12), nn.LeakyReLU(0.2),                                # 3x3: not taken
        nn.Conv2d(16, 8, 4, 2, 1), nn.LeakyReLU(0.2),                               # no weight norm: not taken
        _randomise(decoder.ConvTranspose2dWNUB(8, 16, 8, 12)), nn.LeakyReLU(0.2),   # transposed: not taken
        _randomise(encoder.Conv2dWNUB(16, 32, 4, 6)), nn.LeakyReLU(0.1),            # taken (no affine any more)
        _randomise(encoder.Conv2dWNUB(32, 16, 2, 3)), nn.Tanh(),                    # no LeakyReLU behind it
        _randomise(encoder.Conv2dWNUB(16, 16, 1, 1)),                               # last layer, nothing behind it
    )
    for i in (2, 4, 6):
        assert not encoder._is_conv_wnub(seq[i]), i
    x = 255.0 * torch.rand(2, 3, 16, 24)
    with torch.no_grad():
        got, ref = encoder.run_stack(seq, x, 1.0 / 255.0, -0.5), seq(x / 255.0 - 0.5)
    assert taken == [((16, 3, 4, 4), 0.2, 1.0 / 255.0, -0.5), ((32, 16, 4, 4), 0.1, 1.0, 0.0)]
    assert rel_l2(got, ref) <= 1e-6
    # a first layer that is not taken: the affine is applied in torch in front of the stack, no operator call sees it
    del taken[:]
    with torch.no_grad():
        got, ref = encoder.run_stack(seq[2:], torch.rand(2, 16, 8, 12), 2.0, 0.5), None
    assert taken == [((32, 16, 4, 4), 0.1, 1.0, 0.0)]


@needs_ref
def test_run_stack_recognises_the_reference_layers(monkeypatch):
    from goliath_amd import encoder

    la = _ref_layers()
    torch.manual_seed(4)
    seq = nn.Sequential(_randomise(la.Conv2dWNUB(24, 16, 5, 7, 4, 2, 1)), nn.LeakyReLU(0.2, inplace=True),
                        _randomise(la.Conv2dWNUB(16, 16, 5, 7, 3, 1, 1)), nn.LeakyReLU(0.2, inplace=True),
                        _randomise(la.ConvTranspose2dWNUB(16, 16, 10, 14, 4, 2, 1)), nn.LeakyReLU(0.2, inplace=True),
                        _randomise(la.Conv2dWNUB(16, 16, 5, 7, 4, 2, 1)))
    assert encoder._is_conv_wnub(seq[0]) and encoder._is_conv_wnub(seq[6])
    assert not encoder._is_conv_wnub(seq[2]) and not encoder._is_conv_wnub(seq[4])
    assert not encoder._is_conv_wnub(la.Conv2dWN(16, 16, 4, 2, 1))          # tied bias
    taken = _record(monkeypatch, encoder)
    x = torch.randn(2, 24, 10, 14)
    with torch.no_grad():
        got, ref = encoder.run_stack(seq, x), seq(x)
    assert taken == [((16, 24, 4, 4), 0.2, 1.0, 0.0)]   # the last layer has no activation behind it: a module call
    assert rel_l2(got, ref) <= 1e-6


@needs_ref
def test_encoder_state_dict_matches_reference_encoder():
    from goliath_amd import encoder

    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_shade_golden as g

    g.install_stubs()
    sys.path.insert(0, REF)
    try:
        import ca_code.models.rgca as R

        ref = R.Encoder(256, 77)
    finally:
        sys.path.remove(REF)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    del ref
    got = {k: tuple(v.shape) for k, v in encoder.Encoder(256, 77).state_dict().items()}
    assert got == want


@needs_ref
def test_small_encoder_equals_reference_layers():
    """`Encoder(base=1).eval()` against a module assembled from the reference's la.* layers (the constructor lines of
    rgca.py:277-304 at a 256^2 texture) with the same weights and the reference's forward lines."""
    from goliath_amd import encoder

    la = _ref_layers()
    torch.manual_seed(5)
    n_verts, lrelu = 50, lambda: nn.LeakyReLU(0.2, inplace=True)
    mine = encoder.Encoder(256, n_verts, base=1).eval()
    with torch.no_grad():
        for m in mine.texmod:
            if isinstance(m, encoder.Conv2dWNUB):
                m.bias.normal_(0, 0.3)
    ref = nn.Module()
    ref.geommod = nn.Sequential(la.LinearWN(n_verts * 3, 256), lrelu())
    layers, c, s = [], 3, 256
    for co in encoder.CHANNELS:
        s //= 2
        layers += [la.Conv2dWNUB(c, co, s, s, 4, 2, 1), lrelu()]
        c = co
    ref.texmod = nn.Sequential(*layers)
    ref.jointmod = nn.Sequential(la.LinearWN(256 + 256, 512), lrelu())
    ref.mean, ref.logvar = la.LinearWN(512, 256), la.LinearWN(512, 256)
    ref.load_state_dict(mine.state_dict())
    geom, color = torch.randn(2, n_verts, 3), 255.0 * torch.rand(2, 3, 256, 256)
    with torch.no_grad():
        out = mine(geom, color)
        geomout = ref.geommod(geom.view(geom.shape[0], -1))                     # rgca.py:313-317
        texout = ref.texmod(color / 255.0 - 0.5).view(-1, 256)
        encout = ref.jointmod(torch.cat([geomout, texout], dim=1))
        mu, logvar = ref.mean(encout) * 0.1, ref.logvar(encout) * 0.01
    assert set(out) == {"embs", "embs_mu", "embs_logvar"}
    assert rel_l2(out["embs_mu"], mu) <= 1e-6 and rel_l2(out["embs_logvar"], logvar) <= 1e-6
    assert torch.equal(out["embs"], out["embs_mu"])


def test_patch_encoder_is_idempotent_and_leaves_the_cpu_forward_unchanged(monkeypatch):
    from goliath_amd import dropin, encoder

    class Plain(encoder.Encoder):   # the unpatched forward: the reference's lines (rgca.py:310-332)
        def forward(self, geom, color):
            geomout = self.geommod(geom.view(geom.shape[0], -1))
            texout = self.texmod(color / 255.0 - 0.5).view(-1, 256 * self.base * self.base)
            encout = self.jointmod(torch.cat([geomout, texout], dim=1))
            embs_mu = self.mean(encout) * self.mean_scale
            embs_logvar = self.logvar(encout) * self.logvar_scale
            if self.training:
                embs = embs_mu + torch.exp(embs_logvar) * torch.randn_like(embs_mu) * self.noise_std
            else:
                embs = embs_mu.clone()
            return dict(embs=embs, embs_mu=embs_mu, embs_logvar=embs_logvar)

    torch.manual_seed(6)
    model = Plain(64, 30, base=1)
    geom, color = torch.randn(2, 30, 3), 255.0 * torch.rand(2, 3, 256, 256)

    def run():
        torch.manual_seed(7)           # the training-mode noise draw
        with torch.no_grad():
            return model(geom, color)

    before = run()
    stand_in = types.SimpleNamespace(Encoder=Plain)
    monkeypatch.setenv("GOLIATH_FUSED_ENCODER_ALL", "1")
    assert dropin.patch_encoder(stand_in) is stand_in and Plain.forward is encoder.encoder_forward
    assert dropin.patch_encoder(stand_in) is stand_in and Plain.forward is encoder.encoder_forward
    after = run()
    assert set(after) == set(before)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    assert not torch.equal(after["embs"], after["embs_mu"])     # training mode: the noise was drawn, and identically
