"""CPU: the fused front of URHand's FeatEncoderUNet (goliath_amd.featenc) -- the torch twin against the float64 golden of the
reference's own layers (tests/golden/make_featenc_golden.py), `forward` on the library lines and on the injected twin, the
module twin against the reference class, the shape predicate, the marshallers against the header, the drop-in flag."""
import ctypes
import functools
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from scenes import rel_l2

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
BAR64 = 1e-10   # float64 rounding over ~10^3-term sums, with a wide margin (test_dispunet_cpu.BAR64)
ENTRIES = ("gol_featenc_front_fwd", "gol_featenc_front_bwd")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, "golden", "featenc_golden.npz")) as f:
        return {k: f[k] for k in f.files}


def golden_layers(dtype=torch.float64):
    """(proj, feat): twin layers carrying the golden's parameters."""
    from goliath_amd import featenc

    g = golden()
    proj, feat = featenc.ConvWN(4, 16, 7, 1, 3, bias=False), featenc.ConvWN(16, 32, 4, 2, 1, bias=False)
    for name, layer in (("proj", proj), ("feat", feat)):
        layer.load_state_dict({k: torch.from_numpy(g[name + "." + k]) for k in ("weight_g", "weight_v")}, strict=True)
    return proj.to(dtype), feat.to(dtype)


def golden_grad_names():
    return [n + "." + k for n in ("proj", "feat") for k in ("weight_v", "weight_g")]


def test_front_torch_equals_the_reference_golden():
    from goliath_amd import featenc, tail

    g = golden()
    proj, feat = golden_layers()
    y = featenc.front_torch(torch.from_numpy(g["x"]).double(), tail.wn_weight(proj), tail.wn_weight(feat))
    assert y.shape == g["y"].shape and rel_l2(y, torch.from_numpy(g["y"])) <= BAR64
    params = [proj.weight_v, proj.weight_g, feat.weight_v, feat.weight_g]
    grads = torch.autograd.grad((y * torch.from_numpy(g["g_y"]).double()).sum(), params)
    for n, got in zip(golden_grad_names(), grads):
        want = torch.from_numpy(g["grad." + n])
        assert float(want.norm()) > 0 and rel_l2(got, want) <= BAR64, n


def _small_encoder(dtype=torch.float64, seed=3):
    from goliath_amd import featenc

    torch.manual_seed(seed)
    fe = featenc.FeatEncoderUNet(1, 3, 8, base=16)
    with torch.no_grad():
        for m in fe.modules():
            if isinstance(m, featenc.ConvWN):
                m.weight_g.mul_(torch.rand_like(m.weight_g) + 0.5)
        fe.enc.bias.normal_(0, 0.3)
    return fe.to(dtype)


def test_forward_with_an_empty_table_is_the_plain_module_bitwise(monkeypatch):
    from goliath_amd import featenc

    monkeypatch.delenv("GOLIATH_FUSED_FEATENC_ALL", raising=False)
    monkeypatch.setattr(featenc, "DISPATCH", {})
    fe = _small_encoder()
    x = torch.randn(2, 4, 32, 32, dtype=torch.float64)
    z, gb = featenc.forward(fe, x, op=lambda *a: pytest.fail("nothing is admitted"))
    z0, gb0 = fe(x)
    assert torch.equal(z, z0) and len(gb) == len(gb0) == 4 and all(torch.equal(a, b) for a, b in zip(gb, gb0))
    assert z.shape == (2, 8, 1, 1) and [t.shape[1] for t in gb] == [64, 32, 32, 16]


def test_forward_routes_the_front_to_the_injected_operator(monkeypatch):
    from goliath_amd import featenc

    monkeypatch.setenv("GOLIATH_FUSED_FEATENC_ALL", "1")
    fe = _small_encoder()
    x = torch.randn(2, 4, 32, 32, dtype=torch.float64)
    taken = []

    def op(x_, w_p, w_f):
        taken.append((tuple(x_.shape), tuple(w_p.shape), tuple(w_f.shape)))
        return featenc.front_torch(x_, w_p, w_f)

    z, gb = featenc.forward(fe, x, op=op)
    assert taken == [((2, 4, 32, 32), (16, 4, 7, 7), (48, 16, 4, 4))]
    z0, gb0 = fe(x)
    assert rel_l2(z, z0) <= BAR64 and len(gb) == len(gb0)
    for a, b in zip(gb, gb0):
        assert a.shape == b.shape and rel_l2(a, b) <= BAR64
    # an input that asks for a gradient, a layer with a bias, another geometry: the reference's lines
    for spoil in ("grad", "bias", "stride"):
        fe2, x2 = _small_encoder(), x.clone()
        if spoil == "grad":
            x2.requires_grad_(True)
        elif spoil == "bias":
            fe2.proj.bias = torch.nn.Parameter(torch.zeros(16, dtype=torch.float64))
        else:
            fe2.feat_mod[0].pad = 2
        featenc.forward(fe2, x2, op=lambda *a: pytest.fail(spoil))


def _ref_urhand():
    for p in (ROOT, HERE, os.path.join(HERE, "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ref_stubs

    ref_stubs.install()
    import ca_code.models.urhand as U

    return U


@needs_ref
def test_twin_loads_the_reference_state_dict_and_matches_it():
    from goliath_amd import featenc

    U = _ref_urhand()
    torch.manual_seed(0)
    ref = U.FeatEncoderUNet(1, 3, 128)
    with torch.no_grad():
        for q in ref.parameters():
            if q.dim() == 4 and q.shape[1:] == (1, 1, 1):
                q.mul_(torch.rand_like(q) + 0.5)
        ref.enc.bias.normal_(0, 0.3)
    twin = featenc.FeatEncoderUNet(1, 3, 128)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in twin.state_dict().items()} == want
    assert set(want) >= {"proj.weight_g", "proj.weight_v", "feat_mod.0.weight_v", "gb_mod.3.weight_g", "enc.bias"}
    twin.load_state_dict(ref.state_dict(), strict=True)
    ref, twin = ref.double(), twin.double()
    x = torch.randn(1, 4, 32, 32, dtype=torch.float64)
    with torch.no_grad():
        z0, gb0 = ref(x)
        z1, gb1 = twin(x)
    assert rel_l2(z1, z0) <= BAR64 and len(gb1) == len(gb0) == 4
    for a, b in zip(gb1, gb0):
        assert a.shape == b.shape and rel_l2(a, b) <= BAR64
    # the reference's own layers are recognised by `forward`
    assert featenc._is_conv_wn(ref.proj, 7, 1, 3) and featenc._is_conv_wn(ref.feat_mod[0], 4, 2, 1)
    assert not featenc._is_conv_wn(ref.enc, 4, 2, 1) and not featenc._is_conv_wn(ref.feat_mod[0], 7, 1, 3)


def test_supported_truth_table():
    from goliath_amd import featenc

    ok = lambda **k: featenc.supported(**{**dict(Cx=4, Cm=64, Co=192, H=1024, W=1024), **k})
    assert ok()
    assert [ok(Cx=c) for c in (0, 1, 8, 9)] == [False, True, True, False]
    assert [ok(Cm=c) for c in (8, 16, 24)] == [False, True, False]
    assert [ok(Co=c) for c in (8, 16, 24)] == [False, True, False]
    assert not ok(H=7) and not ok(W=9) and not ok(H=0) and not ok(W=0) and ok(H=2, W=2)
    assert all(len(k) == 5 and v is True and featenc.supported(*k) for k, v in featenc.DISPATCH.items())


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goliath_hip.h")).read(), flags=re.S)


def test_header_declares_and_binding_exports_the_entries():
    from goliath_amd import _lib

    for name in ENTRIES + ("gol_featenc_front_bwd_scratch_floats",):
        assert re.search(r"\b" + name + r"\s*\(", _header()), name
        assert name in _lib.exported_symbols(), name


@pytest.mark.parametrize("entry", ENTRIES)
def test_marshallers_follow_the_header(entry, monkeypatch):
    """Each marshaller passes exactly the parameters goliath_hip.h declares, in its order and with its C types (the
    library sets no argtypes: a miscounted or swapped list would reach a kernel as a garbage pointer)."""
    from goliath_amd import _lib, featenc

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(featenc, "_abi_" + entry[len("gol_"):])
    sig = inspect.signature(fn).parameters
    assert set(sig) == {n for _, n in params} - {"stream"}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in sig.values())
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1)}[ctype]
        v = {"stream": 0xBEEF}.get(name, v)
        if name != "stream":
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(featenc, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


def test_scratch_query_follows_the_header(monkeypatch):
    from goliath_amd import _lib, featenc

    decl = re.search(r"\blong long\s+gol_featenc_front_bwd_scratch_floats\s*\(([^)]*)\)", _header()).group(1)
    assert [" ".join(p.split()) for p in decl.split(",")] == ["int B", "int Cx", "int Cm", "int Co", "int H", "int W"]
    seen = []

    def fake(*args):
        seen.append(args)
        return 7

    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(gol_featenc_front_bwd_scratch_floats=fake))
    assert featenc.bwd_scratch_floats(1, 2, 3, 4, 5, 6) == 7
    assert [(type(a), a.value) for a in seen[0]] == [(ctypes.c_int, v) for v in (1, 2, 3, 4, 5, 6)]
    assert fake.restype is ctypes.c_longlong


def test_patch_urhand_sets_and_clears_the_flag():
    from goliath_amd import dropin, featenc

    class Dec:
        pass

    module = types.SimpleNamespace(ConvTeacherDecoder=Dec, get_shadow_map=None)
    assert featenc.FEATENC_FLAG == "_gol_feat_encoder"
    try:
        dropin.patch_urhand(module)
        assert getattr(Dec, featenc.FEATENC_FLAG) is False
        assert dropin.patch_urhand(module, feat_encoder=True) is module
        assert getattr(Dec, featenc.FEATENC_FLAG) is True
        dropin.patch_urhand(module)
        assert getattr(Dec, featenc.FEATENC_FLAG) is False
    finally:
        del Dec.forward


def test_front_refuses_cpu_tensors_an_input_gradient_and_wrong_shapes(monkeypatch):
    from goliath_amd import _lib, featenc

    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a launch"))
    x, w_p, w_f = torch.zeros(1, 4, 8, 8), torch.zeros(16, 4, 7, 7), torch.zeros(32, 16, 4, 4)
    with pytest.raises(_lib.GoliathHipError, match="no CPU path"):
        featenc.front(x, w_p, w_f)
    with pytest.raises(_lib.GoliathHipError, match="no input gradient"):
        featenc.front(x.clone().requires_grad_(True), w_p, w_f)
    with pytest.raises(_lib.GoliathHipError, match="w_proj"):
        featenc.front(x, torch.zeros(16, 3, 7, 7), w_f)
    with pytest.raises(_lib.GoliathHipError, match="w_feat"):
        featenc.front(x, w_p, torch.zeros(32, 16, 3, 3))
    with pytest.raises(_lib.GoliathHipError, match="unsupported"):
        featenc.front(torch.zeros(1, 4, 7, 8), w_p, w_f)
    with pytest.raises(_lib.GoliathHipError, match="unsupported"):
        featenc.front(torch.zeros(1, 9, 8, 8), torch.zeros(16, 9, 7, 7), w_f)
