"""CPU: the interface of the uvframes operator (goliath_amd/uvframes.py, csrc/uvframes.hip) -- the packed constants against
the reference's float32 values (tests/golden/uvframes_golden.partNN.npz), the second triple and the extra CSR tables against
brute force, the C-ABI marshallers against include/goliath_hip.h, argument validation, the drop-in's keyword."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import npz_parts
import uvframes_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gol_uvframes_fwd", "gol_uvframes_bwd"]


@pytest.fixture(scope="module")
def G():
    return npz_parts.load(os.path.join(ROOT, "tests", "golden", "uvframes_golden.npz"))


def _header():
    return open(os.path.join(ROOT, "include", "goliath_hip.h")).read()


def test_library_lists_and_exports_the_new_entries():
    from goliath_amd import _lib, build

    lib = ctypes.CDLL(build.build())
    for name in ENTRIES + ["gol_uvframes_bwd_scratch_floats"]:
        assert name in _lib.exported_symbols()
        assert re.search(r"\b" + name + r"\s*\(", _header()), name
        assert hasattr(lib, name), name
    fn = lib.gol_uvframes_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    P, nblk = 64 * 64, 16
    # doubles for the camera partials, the per-texel planes, the item / triple sums, mode 0's normal path
    assert fn(2, 81, 64, 128, 130, 0, 1) == 2 * 2 * nblk * 3 + 2 * 3 * P + 2 * 6 * P + 2 * 130 * 3 + 2 * 128 * 9
    assert fn(2, 81, 64, 128, 130, 140, 0) == (2 * 2 * nblk * 3 + 2 * 3 * P + 2 * 3 * P + 2 * 130 * 3 + 2 * 128 * 9
                                               + 2 * 140 * 9 + 2 * (2 * 81 * 3 + 2))
    assert fn(0, 81, 64, 128, 130, 0, 1) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_uvframes_marshallers_follow_the_header(entry, monkeypatch):
    """Each marshaller passes exactly the parameters goliath_hip.h declares, in its order and with its C types (the
    library sets no argtypes: a miscounted or swapped list would reach a kernel as a garbage pointer)."""
    from goliath_amd import _lib, uvframes

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(uvframes, "_abi_" + entry[len("gol_"):])
    sig = inspect.signature(fn).parameters
    assert set(sig) == {n for _, n in params} - {"stream"}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in sig.values())
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "float": (ctypes.c_float, i + 0.5)}[ctype]
        v = {"stream": 0xBEEF}.get(name, v)
        if name != "stream":
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(uvframes, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


@pytest.mark.parametrize("name", cases.CASES)
def test_packed_constants_equal_the_references_float32_values(G, name):
    from goliath_amd import uvframes

    geo = cases.geometry(name)
    topo = uvframes.UVFramesTopology(geo)
    n = lambda t: t.numpy()
    mask = n((geo.index_image != -1).any(-1)).reshape(-1)
    tid = n(topo.geo.texel_rec)[:, 0]
    assert ((tid >= 0) == mask).all()
    want = G[f"consts/{name}"]                                     # per covered texel, row-major: (f, vt01.y, vt02.y)
    got = n(topo.tri_const)[tid[mask]]
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got[:, :3].view(np.int32), want.view(np.int32))       # bit for bit
    assert (got[:, 3] == 0).all()
    if name == "seam":   # the negative tiny fin became +1e-8: f = 1 / 1e-8 in float32
        assert (got[:, 0] == np.float32(1.0) / np.float32(1e-8)).sum() > 0
    # the second triple: vi[face_index_image] per covered texel; the same object where the two images agree everywhere
    flat_idx = n(geo.index_image).reshape(-1, 3)
    second = n(geo.vi)[n(geo.face_index_image).reshape(-1)]
    same = (second[mask] == flat_idx[mask]).all()
    assert (topo.nrm is topo.geo) == bool(same)
    assert same == (name != "impaint")
    ntid = n(topo.nrm.texel_rec)[:, 0]
    assert ((ntid >= 0) == mask).all()
    assert np.array_equal(n(topo.nrm.triples)[ntid[mask]], second[mask])
    assert np.array_equal(n(topo.geo.triples)[tid[mask]], flat_idx[mask])
    # a triple's items are item_tid's run; vertex -> (triple, corner) slots invert the triple table
    itid, start = n(topo.geo.item_tid), n(topo.tri_item_start)
    assert start[0] == 0 and start[-1] == topo.geo.I and len(start) == topo.T + 1
    for t in range(topo.T):
        assert start[t + 1] > start[t] and (itid[start[t]:start[t + 1]] == t).all()
    if name == "coarse":
        assert int((start[1:] - start[:-1]).min()) > 1           # every triple spans several 64-texel items
    table, vs, slot = n(topo.geo.triples).reshape(-1), n(topo.vq_start), n(topo.vq_slot)
    assert len(vs) == topo.V + 1 and vs[0] == 0 and vs[-1] == len(table) == len(slot)
    assert sorted(slot.tolist()) == list(range(len(table)))
    for v in range(topo.V):
        seg = slot[vs[v]:vs[v + 1]]
        assert (table[seg] == v).all() and (np.diff(seg) > 0).all()
    assert topo.tri_item_start.dtype == topo.vq_start.dtype == topo.vq_slot.dtype == torch.int32
    assert topo.to("cpu") is topo


def test_topology_rejects_bad_input():
    from goliath_amd import uvframes

    geo = cases.geometry("dome")
    del geo.v2uv
    with pytest.raises(ValueError, match="v2uv"):
        uvframes.UVFramesTopology(geo)
    geo = cases.geometry("dome")
    geo.index_image[10, 10, 1] = -1                               # a covered texel with one id of -1
    with pytest.raises(ValueError, match="-1"):
        uvframes.UVFramesTopology(geo)
    geo = cases.geometry("dome")
    geo.face_index_image[10, 10] = geo.vi.shape[0]                # a face that does not exist, on a covered texel
    with pytest.raises(ValueError, match="face_index_image"):
        uvframes.UVFramesTopology(geo)
    geo = cases.geometry("dome")
    geo.v2uv[40, 0] = geo.vt.shape[0]                             # a uv slot that does not exist
    with pytest.raises(ValueError, match="v2uv"):
        uvframes.UVFramesTopology(geo)
    geo = cases.geometry("dome")
    geo.face_index_image = geo.face_index_image[:32]
    with pytest.raises(ValueError):
        uvframes.UVFramesTopology(geo)


def test_arguments_are_validated_and_there_is_no_cpu_path():
    from goliath_amd import _lib, uvframes, uvgeom

    geo = cases.geometry("coarse")
    topo = uvframes.UVFramesTopology(geo)
    x = torch.rand(1, 9, 3)
    with pytest.raises(_lib.GoliathHipError, match="no CPU path"):
        uvframes.uv_frames(x, topo)
    with pytest.raises(TypeError):
        uvframes.uv_frames(x, uvgeom.UVTopology(geo.vi, geo.index_image, geo.bary_image))
    with pytest.raises(TypeError):
        uvframes.uv_frames(x, topo, None)                         # posmap and the rest are keyword-only


def test_patch_urhand_keyword_leaves_the_default_binding_untouched():
    from goliath_amd import dropin, shadowmap, urhand

    class ConvTeacherDecoder:
        pass

    module = types.SimpleNamespace(ConvTeacherDecoder=ConvTeacherDecoder, get_shadow_map=None, RenderLayer="theirs")
    assert inspect.signature(dropin.patch_urhand).parameters["uv_frames"].default is False
    assert dropin.patch_urhand(module) is module
    assert ConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward
    assert module.get_shadow_map is shadowmap.get_shadow_map and module.RenderLayer == "theirs"
    dropin.patch_urhand(module, uv_frames=False)
    assert ConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward
    dropin.patch_urhand(module, uv_frames=True)
    assert ConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward_uv_frames
    assert module.RenderLayer == "theirs"
    dropin.patch_urhand(module)                                   # and back
    assert ConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward
    # the two forwards take the reference's parameter list
    a = inspect.signature(urhand.conv_teacher_decoder_forward)
    b = inspect.signature(urhand.conv_teacher_decoder_forward_uv_frames)
    assert list(a.parameters) == list(b.parameters)
    assert [p.default for p in a.parameters.values()] == [p.default for p in b.parameters.values()]


def test_topology_is_cached_on_the_decoder_and_follows_its_buffers():
    from goliath_amd import uvframes

    dec = types.SimpleNamespace(geo_fn=cases.geometry("coarse"))
    topo = uvframes.topology_of(dec)
    assert isinstance(topo, uvframes.UVFramesTopology) and uvframes.topology_of(dec) is topo
    dec.geo_fn = cases.geometry("dome")
    assert uvframes.topology_of(dec).V == 81
