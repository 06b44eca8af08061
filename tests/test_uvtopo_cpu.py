"""CPU: the oracle of tests/uvtopo_cases.py pinned to the reference's own geom.py, and the host side of
goliath_amd/uvtopo.py and of the two drop-in calls that go with it.

With `geom.make_uv_face_index` replaced by the oracle's face image (a function of the arguments the reference passes: the
vt it has already flipped, flip_uv=False), the reference's unmodified make_uv_vert_index, make_uv_barys and bary_coords
reproduce the oracle's index_image exactly and its bary_image to fp32 rounding, and every covered texel has all three
reference barycentrics >= -1e-6: the face stored at texel (r, c) contains uv = ((c + 0.5) / W, (r + 0.5) / H) -- the
texel-centre pin.  The reference's index_image_impaint (scikit-learn KD-tree) agrees with the oracle's source map wherever
the nearest valid texel is unique, and in distance and validity where it is tied.  Those tests need /root/reference and
scikit-learn; the others run everywhere."""
import importlib.util
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import uvtopo_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
EPS = float(np.finfo(np.float32).eps)
needs_ref = pytest.mark.skipif(not os.path.isdir(REF) or importlib.util.find_spec("sklearn") is None,
                               reason="needs the reference tree (build container only) and scikit-learn")


@pytest.fixture(scope="module")
def geom():
    from goliath_amd import dropin

    dropin.install_pytorch3d_shim()      # (a no-op where another test module's stand-ins are registered already)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import ca_code.utils.geom as geom

    return geom


def _oracle_face_index(vt, vti, uv_shape, flip_uv=True, device=None):
    H, W = (uv_shape, uv_shape) if isinstance(uv_shape, int) else uv_shape
    return torch.from_numpy(U.face_image(vt.cpu().numpy(), vti.cpu().numpy(), H, W, flip_uv)[0].copy())


def _oracle_impaint(index_image, bary_image=None, distance_threshold=100.0, device=None):
    idx = index_image.cpu().numpy()
    valid = (idx != -1).any(-1) if idx.ndim == 3 else idx != -1
    src = U.nearest_valid(valid, distance_threshold).src
    out = torch.from_numpy(U.impaint(idx, src).copy())
    if bary_image is None:
        return out
    return out, torch.from_numpy(U.impaint(bary_image.cpu().numpy(), src).copy())


def _tensors(c):
    return torch.from_numpy(np.asarray(c.vi)), torch.from_numpy(np.asarray(c.vt)), torch.from_numpy(np.asarray(c.vti))


# ---- the oracle against the reference's own code ----------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", list(U.CASES))
def test_reference_functions_reproduce_the_oracle(geom, monkeypatch, name):
    c, o = U.CASES[name], U.oracle(name)
    vi, vt, vti = _tensors(c)
    monkeypatch.setattr(geom, "make_uv_face_index", _oracle_face_index)
    index_image = geom.make_uv_vert_index(vt, vi, vti, uv_shape=c.S, flip_uv=c.flip_uv)
    face, bary = geom.make_uv_barys(vt, vti, uv_shape=c.S, flip_uv=c.flip_uv)
    assert index_image.dtype == torch.int64 and np.array_equal(index_image.numpy(), o.index_image)
    assert np.array_equal(face.numpy(), o.face)
    bary = bary.numpy()
    assert bary.dtype == np.float32
    d32 = np.abs(bary.astype(np.float64) - o.bary32).max()
    d64, own = np.abs(bary - o.bary64).max(), np.abs(o.bary32.astype(np.float64) - o.bary64).max()
    print(f"[uvtopo cpu] {name}: reference - oracle fp32 = {d32:.3e}, reference - fp64 = {d64:.3e}, oracle fp32's own = {own:.3e}")
    assert d32 <= 4.0 * EPS                      # fp32 rounding of the same formula
    assert d64 <= 2.0 * own + 4.0 * EPS
    # the texel-centre pin: the reference's own barycentrics say the sample lies in the stored face
    assert o.valid.any() and bary[o.valid].min() >= -1e-6
    assert (bary[~o.valid] == 0).all()


@needs_ref
@pytest.mark.parametrize("name,threshold", U.IMPAINT)
def test_reference_impaint_agrees_with_the_oracle(geom, name, threshold):
    o, n = U.oracle(name), U.oracle_nearest(name, threshold)
    S = o.valid.shape[0]
    ids = np.where(o.valid, np.arange(S * S).reshape(S, S), -1)           # every valid texel carries its own id
    got = geom.index_image_impaint(torch.from_numpy(ids), distance_threshold=threshold).numpy()
    inv = ~o.valid
    assert np.array_equal(got[o.valid], ids[o.valid])
    assert np.array_equal(got[inv] >= 0, n.src[inv] >= 0)                 # validity, tied or not
    filled = inv & (n.src >= 0)
    rr, cc = np.nonzero(filled)
    d2 = (got[filled] // S - rr) ** 2 + (got[filled] % S - cc) ** 2
    assert np.array_equal(d2, n.d2[filled])                               # distance, tied or not
    uniq = filled & n.unique
    assert uniq.any() and np.array_equal(got[uniq], n.src[uniq])
    # with barycentrics, the 3-D form: the same sources
    idx3 = np.repeat(ids[..., None], 3, -1)
    bary = np.random.default_rng(0).random((S, S, 3)).astype(np.float32)
    got3, gotb = geom.index_image_impaint(torch.from_numpy(idx3), torch.from_numpy(bary), threshold)
    assert np.array_equal(got3.numpy()[..., 0], got)
    assert np.array_equal(gotb.numpy()[uniq], U.impaint(bary, n.src)[uniq])


@needs_ref
def test_reference_impaint_single_texel_maps(geom):
    for which in ("corner", "inner"):
        valid = U.masks_e()[which]
        ids = np.where(valid, 7, -1)
        for threshold in (100.0, 5.0):
            got = geom.index_image_impaint(torch.from_numpy(ids), distance_threshold=threshold).numpy()
            assert np.array_equal(got, U.impaint(ids, U.nearest_valid(valid, threshold).src))


@needs_ref
@pytest.mark.parametrize("name,flip_uv", [("b", False), ("b", True)])
def test_geometry_module_through_patch_geometry_ctor(geom, monkeypatch, name, flip_uv):
    """The real GeometryModule(...) under patch_geometry_ctor, with the two HIP functions replaced by the oracle: the
    rebinding reaches the constructor and render_index_images, and the buffers have the reference's dtypes and shapes."""
    from goliath_amd import dropin, uvtopo

    c = U.CASES[name]
    vi, vt, vti = _tensors(c)
    for k in ("make_uv_face_index", "index_image_impaint"):
        monkeypatch.setattr(geom, k, getattr(geom, k))                    # restored after the test
    before = geom.make_uv_face_index, geom.index_image_impaint
    calls = []
    monkeypatch.setattr(uvtopo, "uv_face_index", lambda *a, **k: (calls.append(("face", k.get("device"))),
                                                                  _oracle_face_index(*a, **k))[1])
    monkeypatch.setattr(uvtopo, "impaint", lambda *a, **k: (calls.append(("impaint", k.get("device"))),
                                                            _oracle_impaint(*a, **k))[1])
    assert dropin.patch_geometry_ctor(geom) is geom
    assert geom.make_uv_face_index is not before[0] and geom.index_image_impaint is not before[1]
    assert [p.name for p in inspect.signature(geom.make_uv_face_index).parameters.values()] == \
        [p.name for p in inspect.signature(before[0]).parameters.values()]
    assert [(p.name, p.default) for p in inspect.signature(geom.index_image_impaint).parameters.values()] == \
        [(p.name, p.default) for p in inspect.signature(before[1]).parameters.values()]
    S = c.S
    face, band = U.face_image(c.vt, c.vti, S, S, flip_uv)
    index_image = np.asarray(c.vi)[np.clip(face, 0, None)]
    index_image[face < 0] = -1
    bary32 = U.bary_image(face, c.vt, c.vti, flip_uv, np.float32)
    src = U.nearest_valid(face >= 0, 3.0).src
    for imp in (False, True):
        calls.clear()
        gm = geom.GeometryModule(vi, vt, vti, None, S, flip_uv=flip_uv, impaint=imp, impaint_threshold=3.0)
        assert [k for k, _ in calls] == ["face", "face"] + (["impaint", "impaint"] if imp else [])
        assert all(dev == "cuda" for _, dev in calls)                     # CPU buffers: the work is sent to the GPU
        assert gm.index_image.dtype == torch.int64 and tuple(gm.index_image.shape) == (S, S, 3)
        assert gm.face_index_image.dtype == torch.int64 and tuple(gm.face_index_image.shape) == (S, S)
        assert gm.bary_image.dtype == torch.float32 and tuple(gm.bary_image.shape) == (S, S, 3)
        assert gm.valid_mask.dtype == torch.bool and tuple(gm.valid_mask.shape) == (S, S, 1)
        assert np.array_equal(gm.valid_mask.numpy()[..., 0], face >= 0)   # before the impaint
        s = src if imp else np.full_like(src, -1)
        assert np.array_equal(gm.index_image.numpy(), U.impaint(index_image, s))
        assert np.array_equal(gm.face_index_image.numpy(), U.impaint(face, s))
        assert np.abs(gm.bary_image.numpy() - U.impaint(bary32, s)).max() <= 4.0 * EPS
    idx, fimg, bimg = gm.render_index_images(S, flip_uv=flip_uv, impaint=True)
    assert tuple(idx.shape) == (S, S, 3) and tuple(fimg.shape) == (S, S) and tuple(bimg.shape) == (S, S, 3)
    assert np.array_equal(idx.numpy(), U.impaint(index_image, U.nearest_valid(face >= 0, 100.0).src))


@needs_ref
def test_shim_lets_geom_import_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from goliath_amd import dropin\n"
            "names = dropin.install_pytorch3d_shim()\n"
            "if not names:\n"
            "    print('shim ok: the real pytorch3d is installed, nothing registered'); raise SystemExit(0)\n"
            "assert 'pytorch3d.transforms' in names and dropin.install_pytorch3d_shim() == []\n"
            "import ca_code.utils.geom as geom\n"
            "assert geom.GeometryModule is not None\n"
            "try:\n"
            "    geom.Meshes(1)\n"
            "except RuntimeError as e:\n"
            "    assert 'patch_geometry_ctor' in str(e)\n"
            "else:\n"
            "    raise SystemExit('placeholder did not raise')\n"
            "from pytorch3d.renderer.mesh.textures import TexturesUV\n"
            "from pytorch3d.renderer import MeshRasterizer, RasterizationSettings\n"
            "from pytorch3d.utils import cameras_from_opencv_projection\n"
            "from pytorch3d.io import load_ply\n"
            "from pytorch3d.transforms import axis_angle_to_matrix, euler_angles_to_matrix, matrix_to_axis_angle\n"
            "print('shim ok')\n") % (REF, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shim ok" in r.stdout, r.stdout + r.stderr


# ---- host side, no reference needed ---------------------------------------------------------------------------------------
def test_case_f_seed_keeps_the_edge_band_small():
    assert int(U.oracle("f").band.sum()) <= 2
    assert all(not U.oracle(n).band.any() for n in U.EXACT)


def test_oracle_nearest_is_the_lexicographic_minimum():
    valid = np.zeros((5, 7), bool)
    valid[0, 3] = valid[2, 1] = valid[2, 5] = valid[4, 3] = True
    n = U.nearest_valid(valid, 100.0)
    assert n.src[2, 3] == 0 * 7 + 3 and not n.unique[2, 3] and n.d2[2, 3] == 4      # four at distance 2: the upper one
    assert n.src[2, 2] == 2 * 7 + 1 and n.unique[2, 2]
    assert n.src[1, 2] == 0 * 7 + 3 and not n.unique[1, 2]                          # (0,3) and (2,1) at d2 = 2: upper row
    assert (U.nearest_valid(valid, 1.0).src == -1).all() and (U.nearest_valid(valid, 1.5).src >= 0).sum() == 22


def test_max_d2_is_the_strict_threshold():
    from goliath_amd import uvtopo

    for t in (0.5, 1.0, 2.5, 3.0, math.sqrt(8.0), 7.3, 100.0, 1e9, float("inf")):
        k = uvtopo.max_d2_of(t, 300, 200)
        cap = 299 ** 2 + 199 ** 2
        assert k == cap or (math.sqrt(k) < t and not math.sqrt(k + 1) < t), t
    assert uvtopo.max_d2_of(2.5, 24, 24) == 6 and uvtopo.max_d2_of(3.0, 24, 24) == 8
    assert uvtopo.max_d2_of(0.0, 24, 24) == -1 and uvtopo.max_d2_of(float("nan"), 24, 24) == -1
    assert uvtopo.max_d2_of(-1.0, 24, 24) == -1


def test_cpu_tensors_raise():
    from goliath_amd import _lib, uvtopo

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    vi, vt, vti = _tensors(U.CASES["a"])
    with pytest.raises(_lib.GoliathHipError):
        uvtopo.uv_face_index(vt, vti, 16)
    with pytest.raises(_lib.GoliathHipError):
        uvtopo.index_images(vi, vt, vti, 16)
    with pytest.raises(_lib.GoliathHipError):
        uvtopo.impaint(torch.full((4, 4), -1))
    with pytest.raises(_lib.GoliathHipError):
        uvtopo.nearest_valid(torch.zeros(4, 4, dtype=torch.bool))
    with pytest.raises(_lib.GoliathHipError):
        uvtopo.uv_topology(vi, vt, vti, 16)


@pytest.mark.parametrize("entry", ["gol_uv_face_index", "gol_uv_topology", "gol_nearest_valid", "gol_impaint_gather"])
def test_marshallers_follow_the_header(entry, monkeypatch):
    """Each marshaller passes exactly the parameters goliath_hip.h declares, in its order and with its C types."""
    import ctypes

    from goliath_amd import _lib, uvtopo

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goliath_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", hdr).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(uvtopo, "_abi_" + entry[len("gol_"):])
    assert set(inspect.signature(fn).parameters) == {n for _, n in params} - {"stream"}
    kw, want = {}, []
    for i, (ctype, pname) in enumerate(params):
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "int64_t": (ctypes.c_int64, (1 << 40) + i)}[ctype]
        if pname == "stream":
            v = 0xBEEF
        else:
            kw[pname] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(uvtopo, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry and len(calls[0][1]) == len(params)
    for (ctype, pname), (cls, v), a in zip(params, want, calls[0][1]):
        assert type(a) is cls and a.value == v, (pname, ctype, a)


def test_placeholders_name_the_patch():
    from goliath_amd import dropin

    f = dropin._pytorch3d_placeholder("structures.Meshes")
    assert f.__name__ == "Meshes"
    with pytest.raises(RuntimeError, match="patch_geometry_ctor"):
        f([1], faces=None)


def _rot(axis, t):
    c, s = math.cos(t), math.sin(t)
    return {"X": [[1, 0, 0], [0, c, -s], [0, s, c]], "Y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
            "Z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]


def test_transform_restatements_against_closed_form_rotations():
    from goliath_amd import dropin

    dt = torch.float64
    angles = [0.0, 1e-7, 0.3, -1.1, math.pi / 2, 2.5, math.pi - 1e-3]
    unit = {"X": [1.0, 0, 0], "Y": [0, 1.0, 0], "Z": [0, 0, 1.0]}
    for ax in "XYZ":
        for t in angles:
            want = torch.tensor(_rot(ax, t), dtype=dt)
            aa = torch.tensor(unit[ax], dtype=dt) * t
            assert torch.allclose(dropin.axis_angle_to_matrix(aa), want, atol=1e-12)
            back = dropin.matrix_to_axis_angle(want)
            assert torch.allclose(back, aa, atol=1e-9), (ax, t, back)
    # a rotation by 2 pi / 3 about (1, 1, 1) / sqrt 3 permutes the axes: x -> y -> z -> x
    aa = torch.full((3,), 2 * math.pi / 3 / math.sqrt(3), dtype=dt)
    perm = torch.tensor([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=dt)
    assert torch.allclose(dropin.axis_angle_to_matrix(aa), perm, atol=1e-12)
    assert torch.allclose(dropin.matrix_to_axis_angle(perm), aa, atol=1e-12)
    # a half turn (the pivot is not w): about z, and about (1, 1, 0) / sqrt 2
    half = torch.tensor([[-1.0, 0, 0], [0, -1, 0], [0, 0, 1]], dtype=dt)
    assert torch.allclose(dropin.matrix_to_axis_angle(half).abs(), torch.tensor([0, 0, math.pi], dtype=dt), atol=1e-9)
    half2 = torch.tensor([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]], dtype=dt)
    assert torch.allclose(dropin.matrix_to_axis_angle(half2).abs(),
                          torch.tensor([math.pi / math.sqrt(2), math.pi / math.sqrt(2), 0], dtype=dt), atol=1e-9)
    # Euler: the product of the elementary rotations in the convention's order, batched, fp32 and fp64
    e = torch.tensor([[0.3, -0.7, 1.9], [2.0, 0.1, -0.4]], dtype=dt)
    for conv in ("XYZ", "ZYX", "ZXZ", "YXZ"):
        got = dropin.euler_angles_to_matrix(e, conv)
        for b in range(2):
            want = torch.eye(3, dtype=dt)
            for ax, t in zip(conv, e[b].tolist()):
                want = want @ torch.tensor(_rot(ax, t), dtype=dt)
            assert torch.allclose(got[b], want, atol=1e-12), conv
        assert torch.allclose(dropin.euler_angles_to_matrix(e.float(), conv), got.float(), atol=1e-6)
    with pytest.raises(ValueError):
        dropin.euler_angles_to_matrix(e, "XXY")
    # batched round trip through both maps, generic rotations
    g = torch.Generator().manual_seed(0)
    aa = torch.randn(4, 5, 3, generator=g, dtype=dt)
    aa = aa / aa.norm(dim=-1, keepdim=True) * (torch.rand(4, 5, 1, generator=g, dtype=dt) * 3.0 + 0.05)
    R = dropin.axis_angle_to_matrix(aa)
    assert R.shape == (4, 5, 3, 3) and torch.allclose(R @ R.transpose(-1, -2), torch.eye(3, dtype=dt).expand(4, 5, 3, 3), atol=1e-12)
    assert torch.allclose(torch.linalg.det(R), torch.ones(4, 5, dtype=dt), atol=1e-12)
    assert torch.allclose(dropin.matrix_to_axis_angle(R), aa, atol=1e-9)
