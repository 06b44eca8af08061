"""CPU: the interface of the uvgeom operators (goliath_amd/uvgeom.py, csrc/uvgeom.hip) -- the C-ABI marshallers against
include/goliath_hip.h, the packed topology against a brute-force regrouping, the drop-in binding, no CPU path."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from urhand_shaped import FakeGeo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gol_vert_normals_fwd", "gol_vert_normals_bwd", "gol_values_to_uv_fwd", "gol_values_to_uv_bwd",
           "gol_uvgeom_fwd", "gol_uvgeom_bwd"]


def _header():
    return open(os.path.join(ROOT, "include", "goliath_hip.h")).read()


def test_library_lists_and_exports_the_new_entries():
    from goliath_amd import _lib, build

    lib = ctypes.CDLL(build.build())
    for name in ENTRIES:
        assert name in _lib.exported_symbols()
        assert re.search(r"\bint\s+" + name + r"\s*\(", _header()), name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("entry", ENTRIES)
def test_uvgeom_marshallers_follow_the_header(entry, monkeypatch):
    """Each marshaller passes exactly the parameters goliath_hip.h declares, in its order and with its C types (the
    library sets no argtypes: a miscounted or swapped list would reach a kernel as a garbage pointer)."""
    from goliath_amd import _lib, uvgeom

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(uvgeom, "_abi_" + entry[len("gol_"):])
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
    monkeypatch.setattr(uvgeom, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


def _impainted(geo):
    """FakeGeo's images with the empty texels below row 2 reusing one triple (barycentrics that do not sum to 1) and one
    texel with a single invalid id."""
    idx, bary = geo.index_image.clone(), geo.bary_image.clone()
    empty = (idx == -1).all(-1)
    empty[:2] = False
    idx[empty], bary[empty] = geo.vi[3], torch.tensor([0.5, 0.4, 0.3])
    idx[0, 1] = torch.tensor([2, -1, 5])
    return idx, bary


@pytest.mark.parametrize("impainted", [False, True])
def test_topology_packing_against_brute_force(impainted):
    from goliath_amd import uvgeom

    geo = FakeGeo(48, 5)
    idx, bary = _impainted(geo) if impainted else (geo.index_image, geo.bary_image)
    topo = uvgeom.UVTopology(geo.vi, idx, bary)
    n = lambda t: t.numpy()
    S, V = 48, 36
    assert (topo.S, topo.V, topo.F) == (S, V, geo.vi.shape[0])
    flat = n(idx).reshape(-1, 3)
    covered = np.flatnonzero((flat != -1).all(-1))
    assert topo.M == len(covered) and np.array_equal(n(topo.covered_mask()).reshape(-1).nonzero()[0], covered)
    # per texel: its triple and its barycentrics exactly as given
    rec, triples = n(topo.texel_rec), n(topo.triples)
    assert len({tuple(t) for t in triples}) == topo.T == len({tuple(flat[t]) for t in covered})
    assert (rec[:, 0] >= 0).sum() == topo.M and ((rec[:, 0] < 0) == ~np.isin(np.arange(S * S), covered)).all()
    for t in covered:
        assert tuple(triples[rec[t, 0]]) == tuple(flat[t])
    assert np.array_equal(rec[:, 1:].copy().view(np.float32), n(bary).reshape(-1, 3).astype(np.float32))
    # every covered texel once in the CSR; members of a segment / an item share their triple
    texel_of, ts, it, itid = n(topo.texel_of), n(topo.triple_start), n(topo.item_start), n(topo.item_tid)
    assert sorted(texel_of.tolist()) == covered.tolist()
    assert ts[0] == 0 and ts[-1] == topo.M and len(ts) == topo.T + 1
    for k in range(topo.T):
        assert ts[k + 1] > ts[k] and (rec[texel_of[ts[k]:ts[k + 1]], 0] == k).all()
    assert it[0] == 0 and it[-1] == topo.M and len(it) == topo.I + 1 and len(itid) == topo.I
    for i in range(topo.I):
        assert 0 < it[i + 1] - it[i] <= uvgeom.ITEM_TEXELS and (rec[texel_of[it[i]:it[i + 1]], 0] == itid[i]).all()
    if impainted:
        assert int((ts[1:] - ts[:-1]).max()) > uvgeom.ITEM_TEXELS and topo.I > topo.T
    # vertex -> (face, corner) slots: the inverse of vi; vertex -> (item, corner) slots: the inverse of the items' triples
    for start, slot, table in ((n(topo.vf_start), n(topo.vf_slot), n(geo.vi).reshape(-1)),
                               (n(topo.vt_start), n(topo.vt_slot), triples[itid].reshape(-1))):
        assert len(start) == V + 1 and start[0] == 0 and start[-1] == len(table) == len(slot)
        assert sorted(slot.tolist()) == list(range(len(table)))
        for v in range(V):
            seg = slot[start[v]:start[v + 1]]
            assert (table[seg] == v).all() and (np.diff(seg) > 0).all()
            assert len(seg) == (table == v).sum()
    assert all(getattr(topo, k).dtype == torch.int32 for k in topo._TENSORS)


def test_topology_rejects_bad_input_and_follows_to():
    from goliath_amd import uvgeom

    geo = FakeGeo(16, 2)
    with pytest.raises(ValueError):
        uvgeom.UVTopology(geo.vi, geo.index_image, geo.bary_image, n_verts=5)          # ids beyond the vertex count
    with pytest.raises(ValueError):
        uvgeom.UVTopology(geo.vi, geo.index_image[:, :8], geo.bary_image[:, :8])       # not square
    topo = uvgeom.UVTopology(geo.vi, geo.index_image, geo.bary_image, n_verts=12)
    assert topo.V == 12 and topo.vf_start.numel() == 13 and topo.to("cpu") is topo


def test_cpu_tensors_raise():
    from goliath_amd import _lib, uvgeom

    geo = FakeGeo(16, 2)
    topo = uvgeom.UVTopology(geo.vi, geo.index_image, geo.bary_image)
    x = torch.rand(1, 9, 3)
    for fn in (uvgeom.vert_normals, uvgeom.values_to_uv, uvgeom.uv_geometry):
        with pytest.raises(_lib.GoliathHipError):
            fn(x, topo)
    with pytest.raises(TypeError):
        uvgeom.values_to_uv(x, geo)


def test_patch_geometry_binds_and_is_idempotent():
    from goliath_amd import dropin, uvgeom

    class GeometryModule:
        def to_uv(self, values):
            return "reference"

        def vn(self, verts):
            return "reference"

    module = types.SimpleNamespace(GeometryModule=GeometryModule)
    for _ in range(2):
        assert dropin.patch_geometry(module) is module
        assert GeometryModule.to_uv is uvgeom.geometry_to_uv and GeometryModule.vn is uvgeom.geometry_vn
    # the topology is built lazily from the module's own buffers, cached, and rebuilt when they change
    gm, geo = GeometryModule(), FakeGeo(16, 2)
    assert uvgeom.fused_topology(gm, 9) is None                                  # no buffers: nothing to pack
    gm.vi, gm.index_image, gm.bary_image = geo.vi, geo.index_image, geo.bary_image
    topo = uvgeom.fused_topology(gm, 9)
    assert isinstance(topo, uvgeom.UVTopology) and uvgeom.fused_topology(gm, 9) is topo
    gm.index_image = FakeGeo(24, 2).index_image
    gm.bary_image = FakeGeo(24, 2).bary_image
    assert uvgeom.fused_topology(gm, 9).S == 24


def test_prim_decoder_forward_keeps_the_old_lines_without_index_images(monkeypatch):
    """A geo_fn that was neither patched nor given a topology (tests/rgca_shaped.py:GridGeo) takes the three geo_fn calls."""
    from goliath_amd import rgca, uvgeom
    from rgca_shaped import GridGeo

    assert uvgeom.fused_topology(GridGeo(), 81) is None
    assert uvgeom.fused_topology(FakeGeo(16, 2), 9) is None      # index images, but its class is not patched
    calls = []

    class Stop(Exception):
        pass

    class Geo(GridGeo):
        def to_uv(self, values):
            calls.append("to_uv")
            return super().to_uv(values)

        def vn(self, verts):
            calls.append("vn")
            return super().vn(verts)

    def stop(*a, **k):
        raise Stop

    monkeypatch.setattr(rgca, "uv_geometry", lambda *a, **k: calls.append("uv_geometry"))
    dec = types.SimpleNamespace(geo_fn=Geo(), encmod=stop)
    with pytest.raises(Stop):
        rgca.prim_decoder_forward(dec, torch.zeros(1, 256), torch.rand(1, 81, 3), None, None, None, None, None)
    assert calls == ["to_uv", "vn", "to_uv"]
    # ... and one uv_geometry call once the geo_fn carries a packed topology
    geo = FakeGeo(16, 2)
    geo.uv_topology = uvgeom.UVTopology(geo.vi, geo.index_image, geo.bary_image)
    calls.clear()
    monkeypatch.setattr(rgca, "uv_geometry", lambda *a, **k: (calls.append("uv_geometry"), (None, None))[1])
    with pytest.raises(Stop):
        rgca.prim_decoder_forward(types.SimpleNamespace(geo_fn=geo, encmod=stop), torch.zeros(1, 256), torch.rand(1, 9, 3),
                                  None, None, None, None, None)
    assert calls == ["uv_geometry"]
