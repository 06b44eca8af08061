"""GPU: the uvgeom operators (goliath_amd/uvgeom.py, csrc/uvgeom.hip) against the reference's own float64 results
(tests/golden/uvgeom_golden.partNN.npz, written by tests/golden/make_uvgeom_golden.py from ca_code/utils/geom.py).

The bound of every comparison: |HIP - fp64| <= 2 x |the reference's fp32 - fp64| (same fixture, same views / channels)
+ a floor of 4 eps32 x the magnitude of the quantity (max |verts| for positions, 1 for unit normals, max |g_fp64| for a
gradient).  The factor 2 covers another summation order of the same fp32 terms.  Nothing is excluded: all texels, all
vertices.  Measured ratios (error / bound) are printed before each assertion and recorded in DESIGN.md section 8."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import npz_parts
from urhand_shaped import FakeGeo

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def G():
    return npz_parts.load(os.path.join(HERE, "golden", "uvgeom_golden.npz"))


def _t(a, dev="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _topo(G, dev="cuda"):
    from goliath_amd import uvgeom

    return uvgeom.UVTopology(_t(G["vi"], dev), _t(G["index_image"], dev), _t(G["bary_image"], dev))


def _check(name, got, ref32, ref64, scale):
    """|got - ref64| <= 2 |ref32 - ref64| + 4 eps32 scale (max norms over everything passed: nothing left out)."""
    got, ref32, ref64 = (np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64)
                         for x in (got, ref32, ref64))
    err, ref_err = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max()
    bound = 2.0 * ref_err + 4.0 * EPS * scale
    print(f"[uvgeom] {name}: |hip - fp64| = {err:.3e}, reference fp32's own = {ref_err:.3e}, bound = {bound:.3e}, "
          f"ratio = {err / bound:.3f}")
    assert np.isfinite(got).all(), name
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("B", [1, 3])
def test_vert_normals_parity(G, B):
    from goliath_amd import uvgeom

    topo = _topo(G)
    verts = _t(G["verts"][:B]).requires_grad_(True)
    vn = uvgeom.vert_normals(verts, topo)
    (vn * _t(G["g_vn"][:B])).sum().backward()
    _check(f"vn B={B}", vn, G["ref32/vn"][:B], G["ref64/vn"][:B], 1.0)
    g64 = G["ref64/g_verts_vn"][:B]
    _check(f"g_verts(vn) B={B}", verts.grad, G["ref32/g_verts_vn"][:B], g64, np.abs(g64).max())


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("B", [1, 3])
def test_values_to_uv_parity(G, B, C):
    from goliath_amd import uvgeom

    topo = _topo(G)
    values = _t(G["values"][:B, :, :C]).requires_grad_(True)
    uv = uvgeom.values_to_uv(values, topo)
    assert uv.shape == (B, C, topo.S, topo.S)
    (uv * _t(G["g_uv"][:B, :C])).sum().backward()
    _check(f"uv B={B} C={C}", uv, G["ref32/uv"][:B, :C], G["ref64/uv"][:B, :C], np.abs(G["values"]).max())
    g64 = G["ref64/g_values"][:B, :, :C]
    _check(f"g_values B={B} C={C}", values.grad, G["ref32/g_values"][:B, :, :C], g64, np.abs(g64).max())
    assert (uv[:, :, ~topo.covered_mask()] == 0).all()


@pytest.mark.parametrize("B", [1, 3])
def test_uv_geometry_parity(G, B):
    from goliath_amd import uvgeom

    topo = _topo(G)
    verts = _t(G["verts"][:B]).requires_grad_(True)
    postex, tn = uvgeom.uv_geometry(verts, topo)
    ((postex * _t(G["g_postex"][:B])).sum() + (tn * _t(G["g_tn"][:B])).sum()).backward()
    _check(f"postex B={B}", postex, G["ref32/postex"][:B], G["ref64/postex"][:B], np.abs(G["verts"]).max())
    _check(f"tn B={B}", tn, G["ref32/tn"][:B], G["ref64/tn"][:B], 1.0)
    g64 = G["ref64/g_verts_geo"][:B]
    _check(f"g_verts(postex, tn) B={B}", verts.grad, G["ref32/g_verts_geo"][:B], g64, np.abs(g64).max())
    un = ~topo.covered_mask()
    assert (postex[:, :, un] == 0).all() and (tn[:, :, un] == 0).all()


def test_fused_equals_the_separate_operators(G):
    from goliath_amd import uvgeom

    topo = _topo(G)
    w_p, w_n = _t(G["g_postex"]), _t(G["g_tn"])
    a = _t(G["verts"]).requires_grad_(True)
    postex, tn = uvgeom.uv_geometry(a, topo)
    ((postex * w_p).sum() + (tn * w_n).sum()).backward()
    b = _t(G["verts"]).requires_grad_(True)
    postex2 = uvgeom.values_to_uv(b, topo)
    tn2 = F.normalize(uvgeom.values_to_uv(uvgeom.vert_normals(b, topo), topo), dim=1)
    ((postex2 * w_p).sum() + (tn2 * w_n).sum()).backward()
    for name, x, y, r32, r64, scale in (
            ("postex", postex, postex2, G["ref32/postex"], G["ref64/postex"], np.abs(G["verts"]).max()),
            ("tn", tn, tn2, G["ref32/tn"], G["ref64/tn"], 1.0),
            ("g_verts", a.grad, b.grad, G["ref32/g_verts_geo"], G["ref64/g_verts_geo"], np.abs(G["ref64/g_verts_geo"]).max())):
        bound = 2.0 * np.abs(np.float64(r32) - r64).max() + 4.0 * EPS * scale
        d = float((x.detach().double() - y.detach().double()).abs().max())
        print(f"[uvgeom] fused - composed {name}: {d:.3e} (bound {bound:.3e}, ratio {d / bound:.3f})")
        assert d <= bound, (name, d, bound)


def test_poisoned_buffers_come_back_fully_written(G):
    """Through the ABI marshallers: every output (and every gradient) element is written, uncovered texels with exact 0."""
    from goliath_amd import uvgeom

    topo = _topo(G)
    B, V, S, C = 2, topo.V, topo.S, 4
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    verts, values = _t(G["verts"][:B]), _t(G["values"][:B])
    kw = dict(vi=topo.vi, vf_start=topo.vf_start, vf_slot=topo.vf_slot)
    tex = dict(texel_rec=topo.texel_rec, triples=topo.triples)
    bwd = dict(item_start=topo.item_start, texel_of=topo.texel_of, vt_start=topo.vt_start, vt_slot=topo.vt_slot)
    vn, out, postex, tn = nan(B, V, 3), nan(B, C, S, S), nan(B, 3, S, S), nan(B, 3, S, S)
    uvgeom._abi_vert_normals_fwd(B=B, V=V, F=topo.F, verts=verts, eps=1e-5, vn=vn, **kw)
    uvgeom._abi_values_to_uv_fwd(B=B, V=V, C=C, S=S, T=topo.T, values=values, out=out, **tex)
    vn2 = nan(B, V, 3)
    uvgeom._abi_uvgeom_fwd(B=B, V=V, F=topo.F, S=S, T=topo.T, verts=verts, vn_eps=1e-5, norm_eps=1e-12, vn=vn2,
                           postex=postex, tn=tn, **kw, **tex)
    g_s, g_verts, g_values, g_verts2 = nan(B, V, 3), nan(B, V, 3), nan(B, V, C), nan(B, V, 3)
    uvgeom._abi_vert_normals_bwd(B=B, V=V, F=topo.F, verts=verts, eps=1e-5, g_vn=_t(G["g_vn"][:B]), g_s=g_s,
                                 g_verts=g_verts, **kw)
    uvgeom._abi_values_to_uv_bwd(B=B, V=V, C=C, S=S, T=topo.T, I=topo.I, texel_rec=topo.texel_rec, g_out=_t(G["g_uv"][:B]),
                                 item_sums=nan(B, topo.I, 3, C), g_values=g_values, **bwd)
    uvgeom._abi_uvgeom_bwd(B=B, V=V, F=topo.F, S=S, T=topo.T, I=topo.I, verts=verts, vn_eps=1e-5, norm_eps=1e-12, vn=vn2,
                           g_postex=_t(G["g_postex"][:B]), g_tn=_t(G["g_tn"][:B]), item_sums=nan(B, topo.I, 18),
                           g_s=nan(B, V, 3), g_verts=g_verts2, item_tid=topo.item_tid, **kw, **tex, **bwd)
    for name, t in dict(vn=vn, out=out, vn2=vn2, postex=postex, tn=tn, g_verts=g_verts, g_values=g_values,
                        g_verts2=g_verts2).items():
        assert torch.isfinite(t).all(), name
    un = ~topo.covered_mask()
    assert un.any() and (out[:, :, un] == 0).all() and (postex[:, :, un] == 0).all() and (tn[:, :, un] == 0).all()
    assert torch.equal(vn, vn2)
    _check("abi g_verts", g_verts2, G["ref32/g_verts_geo"][:B], G["ref64/g_verts_geo"][:B],
           np.abs(G["ref64/g_verts_geo"][:B]).max())


# ---- edge cases against a float64 composition written from the stated semantics -------------------------------------------
def _compose(verts, vi, index_image, bary_image, norm_eps, eps=1e-5):
    """Vertex normals, position map and unit normal map in verts' dtype.  Face normal: cross product of the two edges
    leaving corner 0, divided by its length clamped at 1e-5; every face adds it to its three vertices; the sum is divided by
    its length clamped at eps.  A texel with three valid ids holds the bary-weighted sum of its three vertices' values,
    any other texel 0.  The normal map is divided by its per-texel length clamped at norm_eps."""
    dt = verts.dtype
    B, V = verts.shape[:2]
    c0, c1, c2 = (verts[:, vi[:, k]] for k in range(3))
    cr = torch.linalg.cross(c1 - c0, c2 - c0)
    fn = cr / cr.norm(dim=-1, keepdim=True).clamp(min=1e-5)
    s = torch.zeros_like(verts)
    for k in range(3):
        s = s.index_add(1, vi[:, k], fn)
    vn = s / s.norm(dim=-1, keepdim=True).clamp(min=eps)
    ok = (index_image != -1).all(-1)
    ids = index_image.clamp(min=0)
    w = (bary_image.to(torch.float32).to(dt) * ok[..., None].to(dt))

    def to_uv(x):
        return sum(x[:, ids[..., k]] * w[None, ..., k, None] for k in range(3)).permute(0, 3, 1, 2)

    raw = to_uv(vn)
    return vn, to_uv(verts), raw / raw.norm(dim=1, keepdim=True).clamp(min=norm_eps)


def _edge_scene():
    """FakeGeo(128, 4) (25 vertices) plus: vertex 25 without a face; 26-28 a zero-area face; 29-31 and 32-34 two unit
    triangles facing +z and -z exactly.  Index image: every texel the mesh leaves empty (but row 0) reuses the triple of
    face 5 with barycentrics that do not sum to 1 -- an impainted-style map, and one triple of > 4096 texels; texel (0, 0)
    interpolates the vertex normals (0,0,1) and (0,0,-1) to exactly zero; texel (0, 1) sits on the zero-area face (its
    vertex normals are zero); texel (0, 2) has one invalid id (uncovered); the rest of row 0 is empty."""
    geo = FakeGeo(128, 4)
    g = torch.Generator().manual_seed(7)
    t = torch.linspace(-1.0, 1.0, 5)
    v, u = torch.meshgrid(t, t, indexing="ij")
    base = torch.stack([80.0 * u, 100.0 * v, -60.0 * (1.0 - 0.5 * (u * u + v * v))], -1).reshape(-1, 3)
    base = base + 1.5 * torch.randn(base.shape, generator=g)
    extra = torch.tensor([[3.0, 4.0, 5.0],                                         # 25: no face
                          [0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 4.0, 6.0],       # 26-28: collinear
                          [0.0, 0.0, 7.0], [1.0, 0.0, 7.0], [0.0, 1.0, 7.0],       # 29-31: normal (0,0,1)
                          [0.0, 0.0, 9.0], [0.0, 1.0, 9.0], [1.0, 0.0, 9.0]])      # 32-34: normal (0,0,-1)
    verts = torch.cat([base, extra])[None].repeat(2, 1, 1)
    verts[1, :25] += 0.5 * torch.randn(25, 3, generator=g)
    vi = torch.cat([geo.vi, torch.tensor([[26, 27, 28], [29, 30, 31], [32, 33, 34]])])
    idx, bary = geo.index_image.clone(), geo.bary_image.clone()
    empty = (idx == -1).all(-1)
    empty[0] = False
    idx[empty] = geo.vi[5]
    bary[empty] = torch.tensor([0.5, 0.4, 0.3])
    idx[0], bary[0] = -1, 0.0
    idx[0, 0], bary[0, 0] = torch.tensor([29, 32, 25]), torch.tensor([0.5, 0.5, 0.0])
    idx[0, 1], bary[0, 1] = torch.tensor([26, 27, 28]), torch.tensor([0.2, 0.3, 0.5])
    idx[0, 2], bary[0, 2] = torch.tensor([3, -1, 4]), torch.tensor([0.2, 0.3, 0.5])
    return verts, vi, idx, bary


def test_edge_cases_against_a_float64_composition():
    from goliath_amd import uvgeom

    verts, vi, idx, bary = _edge_scene()
    topo = uvgeom.UVTopology(vi.cuda(), idx.cuda(), bary.cuda())
    assert int((topo.triple_start[1:] - topo.triple_start[:-1]).max()) > 4096      # the long-segment path
    assert topo.I > topo.T and int((topo.item_start[1:] - topo.item_start[:-1]).max()) <= 64
    g = torch.Generator().manual_seed(11)
    S = idx.shape[0]
    w_vn, w_p, w_n = (torch.randn(s, generator=g) for s in ((2, 35, 3), (2, 3, S, S), (2, 3, S, S)))
    ref = {}
    for dt in (torch.float32, torch.float64):
        x = verts.to(dt).clone().requires_grad_(True)
        vn, postex, tn = _compose(x, vi, idx, bary, 1e-12)
        (g_vn,) = torch.autograd.grad((vn * w_vn.to(dt)).sum(), x, retain_graph=True)
        (g_geo,) = torch.autograd.grad((postex * w_p.to(dt)).sum() + (tn * w_n.to(dt)).sum(), x)
        ref[dt] = dict(vn=vn.detach(), postex=postex.detach(), tn=tn.detach(), g_vn=g_vn, g_geo=g_geo)
    r32, r64 = ref[torch.float32], ref[torch.float64]
    # the scene holds what it claims
    assert (r64["vn"][:, 25:29] == 0).all() and (r64["tn"][:, :, 0, 0] == 0).all() and (r64["tn"][:, :, 0, 1] == 0).all()
    assert float(r64["g_geo"][:, 29:].abs().max()) > 1e10 and float(r64["g_vn"][:, 26:29].abs().max()) > 1e3
    x = verts.cuda().requires_grad_(True)
    vn = uvgeom.vert_normals(x, topo)
    (g_vn,) = torch.autograd.grad((vn * w_vn.cuda()).sum(), x)
    postex, tn = uvgeom.uv_geometry(x, topo)
    (g_geo,) = torch.autograd.grad((postex * w_p.cuda()).sum() + (tn * w_n.cuda()).sum(), x)
    assert (vn[:, 25:29] == 0).all() and (g_vn[:, 25] == 0).all()                   # no face: zero normal, zero gradient
    assert (tn[:, :, 0, :2] == 0).all() and (postex[:, :, 0, 2:] == 0).all() and (tn[:, :, 0, 2:] == 0).all()
    _check("edge vn", vn, r32["vn"], r64["vn"], 1.0)
    _check("edge postex", postex, r32["postex"], r64["postex"], float(verts.abs().max()))
    _check("edge tn", tn, r32["tn"], r64["tn"], 1.0)
    # gradients in three groups of vertices, each with its own scale: the 1 / 1e-12 texel (vertices 29-34), the 1 / 1e-5
    # face (26-28), everything else
    for name, rows in (("norm_eps clamp", slice(29, 35)), ("face clamp", slice(26, 29)), ("regular", slice(0, 26))):
        for key, got in (("g_vn", g_vn), ("g_geo", g_geo)):
            _check(f"edge {key} [{name}]", got[:, rows], r32[key][:, rows], r64[key][:, rows],
                   float(r64[key][:, rows].abs().max()))


def test_training_step_captures_as_a_graph(G):
    """uv_geometry -> weighted sum -> backward on one stream, captured once and replayed with changed vertices."""
    from goliath_amd import uvgeom

    topo = _topo(G)
    w_p, w_n = _t(G["g_postex"]), _t(G["g_tn"])
    static = _t(G["verts"]).clone().requires_grad_(True)

    def step():
        postex, tn = uvgeom.uv_geometry(static, topo)
        loss = (postex * w_p).sum() + (tn * w_n).sum()
        (g,) = torch.autograd.grad(loss, static)
        return loss, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, grad_g = step()
    gen = torch.Generator().manual_seed(3)
    for i in range(3):
        with torch.no_grad():
            static.copy_(_t(G["verts"]) + (0.3 * (i + 1) * torch.randn(static.shape, generator=gen)).cuda())
        graph.replay()
        torch.cuda.synchronize()
        got_loss, got_grad = loss_g.clone(), grad_g.clone()
        loss_e, grad_e = step()
        assert torch.equal(got_loss, loss_e) and torch.equal(got_grad, grad_e), i   # bitwise: every sum has a fixed order


# ---- through the drop-in ---------------------------------------------------------------------------------------------------
class GeometryModule(torch.nn.Module):
    """GeometryModule-shaped: the buffers of FakeGeo(64, 8) and the two methods as the parent path runs them (boolean-mask
    gather / scatter_add_ composition, in this file's own words)."""

    def __init__(self):
        super().__init__()
        geo = FakeGeo(64, 8)
        for k in ("vi", "index_image", "bary_image"):
            self.register_buffer(k, getattr(geo, k))

    def vn(self, verts):
        from urhand_shaped import vert_normals

        return vert_normals(verts, self.vi)

    def to_uv(self, values):
        S = self.index_image.shape[0]
        mask = (self.index_image != -1).all(-1)
        flat = (values[:, self.index_image[mask]].permute(0, 3, 1, 2) * self.bary_image[mask].float()).sum(-1)
        out = torch.zeros(values.shape[0], values.shape[-1], S, S, dtype=values.dtype, device=values.device)
        out[:, :, mask] = flat
        return out


def _decoder_step(dec, geom, w_p, w_n):
    from goliath_amd import rgca
    from rgca_shaped import cameras

    B = geom.shape[0]
    g = torch.Generator().manual_seed(5)
    embs = torch.randn(B, 256, generator=g).cuda()
    campos = cameras(B)[2].cuda()
    light_pos = (1100.0 * F.normalize(torch.randn(B, 2, 3, generator=g), dim=-1)).cuda()
    preds = rgca.prim_decoder_forward(dec, embs, geom, campos, torch.ones(B, 2, 3).cuda(), light_pos,
                                      (0.1 * torch.randn(B, 3, 81, generator=g)).cuda(), torch.tensor([2] * B).cuda())
    (grad,) = torch.autograd.grad((preds["primpos"] * w_p).sum() + (preds["primnmlbase"] * w_n).sum(), geom)
    return preds["primpos"].detach(), preds["primnmlbase"].detach(), grad


def test_rgca_decoder_through_patch_geometry(G):
    from goliath_amd import dropin, uvgeom
    from rgca_shaped import ShapedPrimDecoder

    B, N = 2, 64 * 64
    dec = ShapedPrimDecoder(seed=0).cuda().eval()
    dec.geo_fn = GeometryModule().cuda()
    gen = torch.Generator().manual_seed(9)
    w_p, w_n = torch.randn(B, N, 3, generator=gen).cuda(), torch.randn(B, N, 3, generator=gen).cuda()
    verts = _t(G["verts"][:B])
    module = types.SimpleNamespace(GeometryModule=GeometryModule)
    old = GeometryModule.to_uv, GeometryModule.vn
    assert uvgeom.fused_topology(dec.geo_fn, 81) is None
    calls = []
    GeometryModule.to_uv = lambda self, v: (calls.append("to_uv"), old[0](self, v))[1]
    GeometryModule.vn = lambda self, v: (calls.append("vn"), old[1](self, v))[1]
    try:   # unpatched: the parent's three calls, nothing else
        pos0, nml0, g0 = _decoder_step(dec, verts.clone().requires_grad_(True), w_p, w_n)
    finally:
        GeometryModule.to_uv, GeometryModule.vn = old
    assert calls == ["to_uv", "vn", "to_uv"], calls
    pos0b, nml0b, g0b = _decoder_step(dec, verts.clone().requires_grad_(True), w_p, w_n)
    try:
        dropin.patch_geometry(module)
        assert uvgeom.fused_topology(dec.geo_fn, 81) is not None
        pos1, nml1, g1 = _decoder_step(dec, verts.clone().requires_grad_(True), w_p, w_n)
    finally:
        GeometryModule.to_uv, GeometryModule.vn = old
    geo = dec.geo_fn
    # (primnmlbase depends on the geometry lines alone; primpos also carries the decoder's convolutions, whose sums are not
    # ordered from run to run)
    assert torch.equal(nml0, nml0b)
    # yardstick: the float64 composition of the geometry lines; primpos = postex + a term that does not depend on geom
    cpu = {k: getattr(geo, k).cpu() for k in ("vi", "index_image", "bary_image")}
    lay = lambda t: t.reshape(B, 64, 64, 3).permute(0, 3, 1, 2).cpu()
    x = verts.cpu().double().requires_grad_(True)
    _, postex64, tn64 = _compose(x, cpu["vi"], cpu["index_image"], cpu["bary_image"], 1e-12)
    (g64,) = torch.autograd.grad((postex64 * lay(w_p).double()).sum() + (tn64 * lay(w_n).double()).sum(), x)
    x32 = verts.cpu().requires_grad_(True)
    _, postex32, tn32 = _compose(x32, cpu["vi"], cpu["index_image"], cpu["bary_image"], 1e-12)
    _check("drop-in primnmlbase", lay(nml1), tn32, tn64.detach(), 1.0)
    offset = lay(pos0).double() - postex32.detach().double()          # the decoder's own position term (unpatched run)
    _check("drop-in primpos", lay(pos1).double() - offset, postex32, postex64.detach(), float(verts.abs().max()))
    _check("drop-in g_geom", g1, g0, g64, float(g64.abs().max()))


def test_second_backward_raises(G):
    from goliath_amd import uvgeom

    topo = _topo(G)
    for fn, key in ((uvgeom.vert_normals, "verts"), (uvgeom.values_to_uv, "values"),
                    (lambda x, t: uvgeom.uv_geometry(x, t)[1], "verts")):
        x = _t(G[key]).requires_grad_(True)
        loss = fn(x, topo).sum()
        loss.backward()
        with pytest.raises(RuntimeError):
            loss.backward()
