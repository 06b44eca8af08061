"""CPU: the oracle of tests/viewtex_cases.py pinned to the reference's own geom.py, the committed golden file, and the host
side of goliath_amd/viewtex.py and dropin.patch_view_texture.

The reference's unmodified compute_face_visibility, compute_uv_visiblity_face and compute_view_texture reproduce the
oracle on the same inputs: in float64 identically on every texel; in float32 identically outside the oracle's band, and
inside it a texel equals the oracle under one of the rounding choices per axis.  Those tests need /root/reference; the
others run everywhere."""
import importlib.util
import inspect
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import viewtex_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
GOLDEN = os.path.join(HERE, "golden", "viewtex_golden.npz")
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference tree (build container only)")
ENTRIES = ("gol_face_visibility", "gol_view_texture", "gol_texmean_finalize")


def _maker():
    spec = importlib.util.spec_from_file_location("make_viewtex_golden", os.path.join(HERE, "golden", "make_viewtex_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def maker():
    return _maker()


@pytest.fixture(scope="module")
def geom(maker):
    return maker.reference_geom()


def _t(a):
    return torch.from_numpy(np.array(a))


# ---- the fixtures and the oracle by themselves ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_fixtures_hold_what_they_claim(name):
    share = C.check_fixture(name)
    print(f"[viewtex cpu] {name}: band = {100 * share:.2f} % of the texels")


def test_oracle_rounds_half_to_even_and_clamps():
    """One texel, one face, an orthographic-like camera: pix = (x, y) straight from the vertex."""
    idx = np.zeros((1, 1, 3), np.int64)
    bary = np.array([[[1.0, 0.0, 0.0]]], np.float32)
    face = np.zeros((1, 1), np.int64)
    image = np.arange(3 * 4 * 6, dtype=np.float32).reshape(1, 3, 4, 6)
    K = np.eye(3, dtype=np.float32)[None]
    Rt = np.eye(4, dtype=np.float32)[None, :3]
    index_img = np.zeros((1, 4, 6), np.int64)
    for (x, y), (col, row) in {(1.0, 1.0): (0, 0), (2.0, 3.0): (2, 2), (3.0, 2.0): (2, 2), (-5.0, 9.0): (0, 3),
                               (2.2, 0.1): (2, 0), (100.0, -1.0): (5, 0)}.items():
        verts = np.array([[[x, y, 1.0]]], np.float32)
        o = C.compute(verts, image, index_img, K, Rt, idx, bary, face, 1)
        assert o.tex[0, :, 0, 0].tolist() == image[0, :, row, col].tolist(), (x, y)
    o = C.compute(np.array([[[1.0, 1.0, 0.0]]], np.float32), image, index_img, K, Rt, idx, bary, face, 1)
    assert (o.tex == 0).all() and o.mask.all()                       # p.z == 0: the value 0, still visible


# ---- the oracle against the reference's own code ----------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", C.NAMES)
def test_reference_visibility_reproduces_the_oracle(geom, name):
    c, o = C.case(name), C.oracle(name)
    fv = geom.compute_face_visibility(_t(c.index_img), _t(c.faces))
    assert fv.dtype == torch.bool and tuple(fv.shape) == (C.B, c.F) and np.array_equal(fv.numpy(), o.face_vis)
    uv = geom.compute_uv_visiblity_face(_t(c.index_img), _t(c.faces), _t(c.face_index_uv))
    assert uv.dtype == torch.bool and tuple(uv.shape) == (C.B, c.S, c.S) and np.array_equal(uv.numpy(), o.mask[:, 0])


@needs_ref
@pytest.mark.parametrize("threshold", [None, C.THRESHOLD])
@pytest.mark.parametrize("name", C.NAMES)
def test_reference_view_texture_reproduces_the_oracle(geom, maker, name, threshold):
    c, o = C.case(name), C.oracle(name, threshold)
    tex64, mask64 = maker.reference_outputs(geom, c, threshold, torch.float64)
    assert tex64.dtype == torch.float64 and tuple(tex64.shape) == (C.B, 3, c.S, c.S)
    assert mask64.dtype == torch.bool and tuple(mask64.shape) == (C.B, 1, c.S, c.S)
    d64 = np.abs(tex64.numpy() - o.tex).max()
    print(f"[viewtex cpu] {name} thr={threshold}: float64 reference - oracle = {d64}")
    assert d64 == 0.0 and np.array_equal(mask64.numpy(), o.mask)     # identical on every texel
    tex32, mask32 = maker.reference_outputs(geom, c, threshold, torch.float32)
    assert tex32.dtype == torch.float32 and mask32.dtype == torch.bool and np.array_equal(mask32.numpy(), o.mask)
    tex32 = tex32.numpy()
    out = ~o.band
    differ = int((tex32 != o.tex).any(1).any(0)[o.band].sum())
    print(f"[viewtex cpu] {name}: band {int(o.band.sum())} texels, float32 reference differs on {differ} of them")
    assert np.array_equal(tex32[..., out], o.tex[..., out])          # identical outside the band
    assert C.in_alts(tex32, o, o.band).all()                         # inside: one of the rounding choices per axis


@needs_ref
def test_committed_golden_is_what_the_script_produces(maker):
    fresh = maker.build()
    with np.load(GOLDEN) as z:
        assert sorted(z.files) == sorted(fresh)
        for k, v in fresh.items():
            assert z[k].dtype == v.dtype and np.array_equal(z[k], v), k
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_golden_holds_the_cases_inputs():
    with np.load(GOLDEN) as z:
        for name in C.NAMES:
            c = C.case(name)
            for k in ("verts", "image", "index_img", "K", "Rt", "index_image_uv", "bary_image_uv", "face_index_uv", "faces"):
                assert np.array_equal(z[f"{name}/{k}"], getattr(c, k)), (name, k)
            o = C.oracle(name)
            assert np.array_equal(z[f"{name}/mask"], o.mask) and np.array_equal(z[f"{name}/face_vis"], o.face_vis)
            assert np.array_equal(z[f"{name}/tex"][..., ~o.band], o.tex[..., ~o.band])


# ---- host side, no reference needed -----------------------------------------------------------------------------------------
@needs_ref
def test_parameter_lists_equal_the_references(geom):
    from goliath_amd import viewtex

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    assert params(viewtex.compute_view_texture) == params(geom.compute_view_texture)
    src = open(os.path.join(REF, "ca_code", "utils", "tex.py")).read()
    want = re.search(r"def get_tex_rl\((.*?)\):", src, re.S).group(1)
    assert [p.split(":")[0].strip() for p in re.split(r",(?![^\[]*\])", want)] == \
        [p for p in inspect.signature(viewtex.get_tex_rl).parameters]


def test_cpu_tensors_raise():
    from goliath_amd import _lib, viewtex

    c = C.case("b")
    idx, bary, face = _t(c.index_image_uv), _t(c.bary_image_uv), _t(c.face_index_uv)
    with pytest.raises(_lib.GoliathHipError):
        viewtex.ViewTexTopology(idx, bary, face)
    with pytest.raises(_lib.GoliathHipError):
        viewtex.face_visibility(_t(c.index_img), c.F)
    with pytest.raises(_lib.GoliathHipError):
        viewtex.uv_visibility(_t(c.index_img), c.F, face)
    with pytest.raises(_lib.GoliathHipError):
        viewtex.compute_view_texture(_t(c.verts), _t(c.faces), _t(c.image), _t(c.index_img), None, _t(c.K), _t(c.Rt), idx,
                                     bary, face)
    with pytest.raises(_lib.GoliathHipError):
        viewtex.get_tex_rl(None, _t(c.image), (_t(c.verts), _t(c.faces)), _t(c.Rt), _t(c.K), face, idx, bary)


def test_topology_raises_on_shape_mismatches(monkeypatch):
    from goliath_amd import viewtex

    monkeypatch.setattr(viewtex, "_need_gpu", lambda *a: None)       # the shape checks come before any device work
    idx, bary, face = torch.zeros(8, 6, 3, dtype=torch.int64), torch.zeros(8, 6, 3), torch.zeros(8, 6, dtype=torch.int64)
    topo = viewtex.ViewTexTopology(idx, bary, face)
    assert (topo.S_h, topo.S_w) == (8, 6) and topo.index_image_uv.dtype == torch.int32
    assert topo.face_index_uv.dtype == torch.int32 and topo.index_image_uv.is_contiguous()
    for bad in ((idx[:, :5], bary, face), (idx, bary[:7], face), (idx, bary, face[:, :5]), (idx[..., :2], bary[..., :2], face),
                (idx, bary, face[None]), (idx.float(), bary, face)):
        with pytest.raises(ValueError):
            viewtex.ViewTexTopology(*bad)


def _stand_in():
    calls = []
    m = types.ModuleType("stand_in_geom")

    def compute_face_visibility(index_img, faces):
        calls.append("face")
        return "face-ref"

    def compute_uv_visiblity_face(face_index_image, faces, face_index_uv):
        calls.append("uv")
        return "uv-ref"

    def compute_view_texture(verts, faces, image, face_index_image, normal_image, K, Rt, index_image_uv, bary_image_uv,
                             face_index_uv, intensity_threshold=None, normal_threshold=None):
        calls.append(("tex", intensity_threshold, normal_threshold))
        return "tex-ref"

    m.compute_face_visibility, m.compute_uv_visiblity_face = compute_face_visibility, compute_uv_visiblity_face
    m.compute_view_texture = compute_view_texture
    return m, calls


def test_patch_view_texture_on_a_stand_in_module():
    from goliath_amd import dropin

    m, calls = _stand_in()
    originals = m.compute_face_visibility, m.compute_uv_visiblity_face, m.compute_view_texture
    t = types.ModuleType("stand_in_tex")
    t.compute_view_texture = m.compute_view_texture
    t.get_tex_rl = lambda rl, image, ply, extrin, intrin, face_index, index_image, bary_image: "rl-ref"
    rl_original = t.get_tex_rl
    had_tex = "ca_code.utils.tex" in sys.modules
    assert dropin.patch_view_texture(m, t) is m
    once = m.compute_face_visibility, m.compute_uv_visiblity_face, m.compute_view_texture, t.get_tex_rl
    assert all(a is not b for a, b in zip(once, originals + (rl_original,)))
    assert [f.reference for f in once] == list(originals) + [rl_original]
    assert t.compute_view_texture is m.compute_view_texture
    assert dropin.patch_view_texture(m, t) is m                      # idempotent: nothing is wrapped twice
    assert (m.compute_face_visibility, m.compute_uv_visiblity_face, m.compute_view_texture, t.get_tex_rl) == once
    assert [f.reference for f in once] == list(originals) + [rl_original]
    assert [p.name for p in inspect.signature(m.compute_view_texture).parameters.values()] == \
        [p.name for p in inspect.signature(originals[2]).parameters.values()]
    # non-CUDA inputs go to the reference
    c = C.case("b")
    cpu = [_t(a) for a in (c.verts, c.faces, c.image, c.index_img)]
    assert m.compute_face_visibility(cpu[3], cpu[1]) == "face-ref"
    assert m.compute_uv_visiblity_face(cpu[3], cpu[1], _t(c.face_index_uv)) == "uv-ref"
    assert m.compute_view_texture(cpu[0], cpu[1], cpu[2], cpu[3], None, _t(c.K), _t(c.Rt), _t(c.index_image_uv),
                                  _t(c.bary_image_uv), _t(c.face_index_uv), intensity_threshold=7.0) == "tex-ref"
    assert t.get_tex_rl(None, cpu[2], (cpu[0], cpu[1]), _t(c.Rt), _t(c.K), _t(c.face_index_uv), _t(c.index_image_uv),
                        _t(c.bary_image_uv)) == "rl-ref"
    assert calls == ["face", "uv", ("tex", 7.0, None)]
    assert ("ca_code.utils.tex" in sys.modules) == had_tex


def test_patch_view_texture_does_not_import_the_tex_module():
    code = ("import sys, types; sys.path.insert(0, %r)\n"
            "from goliath_amd import dropin\n"
            "pkg = types.ModuleType('ca_code'); pkg.__path__ = []\n"
            "utils = types.ModuleType('ca_code.utils'); utils.__path__ = []\n"
            "g = types.ModuleType('ca_code.utils.geom')\n"
            "g.compute_face_visibility = g.compute_uv_visiblity_face = g.compute_view_texture = lambda *a, **k: None\n"
            "sys.modules.update({'ca_code': pkg, 'ca_code.utils': utils, 'ca_code.utils.geom': g}); utils.geom = g\n"
            "assert dropin.patch_view_texture() is g and g.compute_view_texture._goliath_viewtex\n"
            "assert 'ca_code.utils.tex' not in sys.modules and 'cv2' not in sys.modules and 'drtk' not in sys.modules\n"
            "print('no tex import')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "no tex import" in r.stdout, r.stdout + r.stderr


def test_entries_are_declared_bound_and_exported():
    from goliath_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goliath_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in goliath_hip.h"
        assert name in _lib.exported_symbols() and hasattr(lib, name)


@pytest.mark.parametrize("entry", ENTRIES)
def test_marshallers_follow_the_header(entry, monkeypatch):
    """Each marshaller passes exactly the parameters goliath_hip.h declares, in its order and with its C types."""
    import ctypes

    from goliath_amd import _lib, viewtex

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goliath_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", hdr).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(viewtex, "_abi_" + entry[len("gol_"):])
    assert set(inspect.signature(fn).parameters) == {n for _, n in params} - {"stream"}
    kw, want = {}, []
    for i, (ctype, pname) in enumerate(params):
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "int64_t": (ctypes.c_int64, (1 << 40) + i),
                      "float": (ctypes.c_float, i + 0.5)}[ctype]
        if pname == "stream":
            v = 0xBEEF
        else:
            kw[pname] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(viewtex, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry and len(calls[0][1]) == len(params)
    for (ctype, pname), (cls, v), a in zip(params, want, calls[0][1]):
        assert type(a) is cls and a.value == v, (pname, ctype, a)
