"""CPU: the interface of the fused textured mesh render (meshraster.render_textured / FusedRenderLayer, csrc/meshrender.hip)
-- RenderLayer's signatures, the drop-in binding, the C-ABI marshallers against include/goliath_hip.h, no CPU path."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gol_mesh_render_fwd", "gol_mesh_render_bwd", "gol_mesh_render_edge_bwd"]


def _header():
    return open(os.path.join(ROOT, "include", "goliath_hip.h")).read()


def _params(fn):
    return [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]


def test_fused_layer_has_render_layers_signatures():
    from goliath_amd import meshraster

    assert issubclass(meshraster.FusedRenderLayer, meshraster.RenderLayer)
    assert _params(meshraster.FusedRenderLayer.__init__) == _params(meshraster.RenderLayer.__init__)
    assert _params(meshraster.FusedRenderLayer.forward) == _params(meshraster.RenderLayer.forward)
    vi = torch.tensor([[0, 1, 2]])
    layer = meshraster.FusedRenderLayer(8, 6, vi, torch.tensor([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]), vi, flip_uvs=True)
    assert (layer.h, layer.w) == (8, 6) and torch.allclose(layer.vt[:, 1], torch.tensor([0.8, 0.6, 0.4]))


def test_patch_urhand_binds_the_fused_layer_on_request():
    from goliath_amd import dropin, meshraster, urhand

    class ConvTeacherDecoder:
        def forward(self):
            pass

    def module():
        return types.SimpleNamespace(get_shadow_map="reference", RenderLayer="drtk", ConvTeacherDecoder=ConvTeacherDecoder)

    with pytest.warns(RuntimeWarning, match="UNVERIFIED"):
        assert dropin.patch_urhand(module(), mesh_render_layer="fused").RenderLayer is meshraster.FusedRenderLayer
    with pytest.warns(RuntimeWarning, match="UNVERIFIED"):
        assert dropin.patch_urhand(module(), mesh_render_layer=True).RenderLayer is meshraster.RenderLayer
    ur = dropin.patch_urhand(module())
    assert ur.RenderLayer == "drtk" and ConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward


def test_library_list_names_the_new_entries():
    from goliath_amd import _lib

    for name in ENTRIES:
        assert name in _lib.exported_symbols()
        assert re.search(r"\bint\s+" + name + r"\s*\(", _header()), name


@pytest.mark.parametrize("entry", ENTRIES)
def test_mesh_render_marshallers_follow_the_header(entry, monkeypatch):
    """Each marshaller passes exactly the parameters goliath_hip.h declares, in its order and with its C types (the
    library sets no argtypes: a miscounted or swapped list would reach a kernel as a garbage pointer)."""
    from goliath_amd import _lib, meshraster

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(meshraster, "_abi_" + entry[len("gol_"):])
    assert set(inspect.signature(fn).parameters) == {n for _, n in params} - {"stream"}
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "int64_t": (ctypes.c_int64, (1 << 40) + i),
                      "float": (ctypes.c_float, i + 0.5)}[ctype]
        v = {"stream": 0xBEEF}.get(name, v)
        if name != "stream":
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(meshraster, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


def test_cpu_tensors_raise():
    from goliath_amd import _lib, meshraster

    B, H, W = 1, 4, 5
    vi = torch.tensor([[0, 1, 2]])
    args = dict(v_pix=torch.rand(B, 3, 3), vi=vi, vt=torch.rand(3, 2), vti=vi, tex=torch.rand(B, 3, 8, 8),
                index_img=torch.zeros(B, H, W, dtype=torch.int32), depth_img=torch.ones(B, H, W),
                bary_img=torch.full((B, 3, H, W), 1 / 3))
    with pytest.raises(_lib.GoliathHipError):
        meshraster.render_textured(**args, edge_grad=True)
    layer = meshraster.FusedRenderLayer(H, W, vi, torch.rand(3, 2), vi)
    K = torch.eye(3)[None]
    Rt = torch.cat([torch.eye(3), torch.tensor([[0.0], [0.0], [3.0]])], 1)[None]
    with pytest.raises(_lib.GoliathHipError):
        layer(torch.rand(B, 3, 3), torch.rand(B, 3, 8, 8), K, Rt)
