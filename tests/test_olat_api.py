"""CPU: the public surface of the fused OLAT path -- drop-in bindings, the CPU fall-back of the fused forward_rgb, the error
messages of goliath_amd.olat and the C ABI's declarations.  The kernels themselves are tested in test_gpu_olat.py."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

import olat_cases as C
import urhand_shaped as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gol_olat_features_fwd", "gol_olat_combine_fwd", "gol_olat_combine_bwd")


def _header():
    hdr = open(os.path.join(ROOT, "include", "goliath_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_patch_hand_teacher_binds_default_fused_and_restores():
    from goliath_amd import dropin, urhand

    tm = types.SimpleNamespace(OLATRGBDecoder=type("OLATRGBDecoder", (), {}))
    assert dropin.patch_hand_teacher(tm) is tm
    assert tm.OLATRGBDecoder.forward_rgb is urhand.olat_rgb_decoder_forward_rgb
    assert dropin.patch_hand_teacher(tm, olat_fused=True) is tm
    assert tm.OLATRGBDecoder.forward_rgb is urhand.olat_rgb_decoder_forward_rgb_fused
    dropin.patch_hand_teacher(tm, olat_fused=False)
    assert tm.OLATRGBDecoder.forward_rgb is urhand.olat_rgb_decoder_forward_rgb
    want = list(inspect.signature(urhand.olat_rgb_decoder_forward_rgb).parameters)
    assert list(inspect.signature(urhand.olat_rgb_decoder_forward_rgb_fused).parameters) == want


@pytest.mark.parametrize("training,iteration", [(False, None), (True, 0), (True, 5000)])
def test_fused_forward_falls_back_on_cpu_tensors(monkeypatch, training, iteration):
    from goliath_amd import olat, urhand

    B, L = 2, 2
    g = torch.Generator().manual_seed(3)
    volume = torch.rand(B, L, 4, 4, 1, 2, 4, 4, generator=g)
    monkeypatch.setattr(urhand, "deep_shadow", lambda *a, **k: volume)

    def no_kernel(*a, **k):
        raise AssertionError("the fused operators were called with CPU tensors")

    monkeypatch.setattr(olat, "features", no_kernel)
    monkeypatch.setattr(olat, "combine", no_kernel)
    dec = S.ShapedOLATRGBDecoder(None, 200.0, seed=0).train(training)
    inp = S.teacher_inputs(B=B, L=L)
    want = urhand.olat_rgb_decoder_forward_rgb(dec, **inp, iteration=iteration)
    got = urhand.olat_rgb_decoder_forward_rgb_fused(dec, **inp, iteration=iteration)
    assert set(got) == set(want) == ({"primrgb", "primshadow", "texolat"} if training else {"primrgb", "primshadow"})
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_error_messages_name_the_argument():
    from goliath_amd import _lib, olat

    case = C.standin_case(1, 2)
    geom = [case[k] for k in C.GEOM_KEYS]
    tail = (case["primsize"], case["npx"], case["npy"], case["volradius"])
    with pytest.raises(_lib.GoliathHipError, match=r"shadow must be \[2, 16, 2, 4, 4\], got \[2, 16, 4, 4, 2\]"):
        olat.features(*geom, case["shadow"].permute(0, 1, 3, 4, 2).contiguous(), *tail)
    with pytest.raises(_lib.GoliathHipError, match=r"primrot must be \[1, 16, 3, 3\]"):
        olat.features(geom[0], geom[1][:, :, :2], *geom[2:], case["shadow"], *tail)
    with pytest.raises(_lib.GoliathHipError, match="shadow must be a CUDA tensor"):     # everything right but the device
        olat.features(*geom, case["shadow"], *tail)
    cc = C.combine_case(1, 2)
    args = (cc["light_intensity"], cc["shadow"], cc["primsize"], cc["npx"], cc["npy"], False, True)
    with pytest.raises(_lib.GoliathHipError, match=r"tex is 8 x 8.*16 x 16 map \(uv_size\)"):
        olat.combine(cc["tex"][:, :, :8, :8].contiguous(), *args)
    with pytest.raises(_lib.GoliathHipError, match="tex must be contiguous"):
        olat.combine(cc["tex"].transpose(2, 3), *args)
    with pytest.raises(_lib.GoliathHipError, match="tex must have dtype torch.float32"):
        olat.combine(cc["tex"].double(), *args)
    with pytest.raises(_lib.GoliathHipError, match="tex must be a CUDA tensor"):
        olat.combine(cc["tex"], *args)


def test_fused_forward_rejects_a_uv_size_the_primitives_do_not_tile(monkeypatch):
    """The check sits behind the CPU fall-back, so the tensors only claim to be on the GPU; it raises before any launch."""
    from goliath_amd import _lib, urhand

    dec = S.ShapedOLATRGBDecoder(None, 200.0, seed=0).eval()
    dec.uv_size = 20
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(_lib.GoliathHipError, match="uv_size 20 is not 4 x 4 primitives of 4 x 4 texels"):
        urhand.olat_rgb_decoder_forward_rgb_fused(dec, **S.teacher_inputs(B=1, L=2))


def test_symbols_are_declared_and_listed():
    from goliath_amd import _lib

    declared = set(re.findall(r"\b(gol_[a-z0-9_]+)\s*\(", _header()))
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.exported_symbols(), name


@pytest.mark.parametrize("entry", ENTRIES)
def test_marshallers_follow_the_header(entry, monkeypatch):
    """olat's marshaller of an entry passes exactly the parameters goliath_hip.h declares, in its order and with its C
    types (the library sets no argtypes: a swapped pair would reach a kernel as a wrong pointer)."""
    from goliath_amd import _lib, olat

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(olat, "_abi_" + entry[len("gol_"):])
    assert set(inspect.signature(fn).parameters) == {n for _, n in params} - {"stream"}
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "float": (ctypes.c_float, i + 0.5)}[ctype]
        if name == "stream":
            v = 0xBEEF
        else:
            kw[name] = ctypes.c_void_p(v) if cls is ctypes.c_void_p else v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(olat, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)
