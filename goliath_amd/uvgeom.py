"""Tracked mesh -> UV position / normal maps on the HIP kernels of csrc/uvgeom.hip, with gradients.

    UVTopology(vi, index_image, bary_image)     the constant topology, packed once (the only place that syncs the host)
    vert_normals(verts, topo, eps=1e-5)         ca_code/utils/geom.py:337-346
    values_to_uv(values, topo)                  ca_code/utils/geom.py:308-324 (GeometryModule.to_uv, make_postex, ...)
    uv_geometry(verts, topo, norm_eps=1e-12)    postex, tn of PrimDecoder.forward (ca_code/models/rgca.py:483-491) in one call

The reference runs these lines as boolean-mask gathers (a host sync each), `scatter_add_` and an accumulating index_put in
the backward.  Here each direction is one pass with nothing but the output written, on the current stream, without host
sync: a training step through them captures as a graph.  Every tensor must be on the GPU: there is no CPU path.
"""
import ctypes

import torch

from . import _lib
from ._lib import c_float, c_int, stream_ptr

_F32, _I32 = torch.float32, torch.int32
ITEM_TEXELS = 64   # a triple's texels are reduced in work items of at most this many (csrc/uvgeom.hip)


class UVTopology:
    """The constant part of `values_to_uv` / `vert_normals`, packed for the kernels (int32 / float32 on one device).

    vi[F,3]: faces; index_image[S,S,3]: vertex ids per texel (-1 = none); bary_image[S,S,3]: barycentrics, used exactly as
    given (an impainted map's need not sum to 1).  n_verts: the vertex count of the tensors that will be passed (default:
    the largest id + 1).  Attributes (see include/goliath_hip.h): vi, vf_start, vf_slot, texel_rec, triples, triple_start,
    item_start, item_tid, texel_of, vt_start, vt_slot; sizes S, V, F, T (distinct triples), M (covered texels), I (items).
    A texel is covered when all three of its ids are valid (geom.py:310); texels are grouped by vertex TRIPLE, not by face
    index, so impainted index images group correctly."""

    _TENSORS = ("vi", "vf_start", "vf_slot", "texel_rec", "triples", "triple_start", "item_start", "item_tid", "texel_of",
                "vt_start", "vt_slot")

    def __init__(self, vi, index_image, bary_image, n_verts=None):
        if index_image.dim() != 3 or index_image.shape[0] != index_image.shape[1] or index_image.shape[2] != 3:
            raise ValueError(f"index_image must be [S,S,3], got {tuple(index_image.shape)}")
        if tuple(bary_image.shape) != tuple(index_image.shape):
            raise ValueError("bary_image must have index_image's shape")
        if vi.dim() != 2 or vi.shape[1] != 3:
            raise ValueError(f"vi must be [F,3], got {tuple(vi.shape)}")
        dev = index_image.device
        S = index_image.shape[0]
        P = S * S
        vi = vi.to(dev).long()
        idx = index_image.reshape(P, 3).long()
        mask = (idx != -1).all(-1)
        top = max(int(vi.max()) if vi.numel() else -1, int(idx.max()) if P else -1)
        V = int(n_verts) if n_verts is not None else top + 1
        if top >= V or (vi.numel() and int(vi.min()) < 0) or bool((idx[mask] < 0).any()):
            raise ValueError(f"vertex ids must lie in [0, {V})")
        covered = mask.nonzero().flatten()                                   # ascending texel ids
        triples, inv = torch.unique(idx[covered], dim=0, return_inverse=True)
        T, M = triples.shape[0], covered.numel()
        tid = torch.full((P,), -1, dtype=torch.long, device=dev)
        tid[covered] = inv
        rec = torch.empty(P, 4, dtype=_I32, device=dev)
        rec[:, 0] = tid.to(_I32)
        rec[:, 1:] = bary_image.reshape(P, 3).to(_F32).contiguous().view(_I32)
        counts = torch.bincount(inv, minlength=T)
        triple_start = torch.zeros(T + 1, dtype=torch.long, device=dev)
        triple_start[1:] = counts.cumsum(0)
        texel_of = covered[torch.argsort(inv, stable=True)]
        # work items: every triple's run in pieces of at most ITEM_TEXELS texels
        n_items = (counts + ITEM_TEXELS - 1) // ITEM_TEXELS
        item_tid = torch.repeat_interleave(torch.arange(T, device=dev), n_items)
        I = item_tid.numel()
        first = torch.zeros(T + 1, dtype=torch.long, device=dev)
        first[1:] = n_items.cumsum(0)
        local = torch.arange(I, device=dev) - first[item_tid]
        item_start = torch.empty(I + 1, dtype=torch.long, device=dev)
        item_start[:I] = triple_start[item_tid] + ITEM_TEXELS * local
        item_start[I] = M
        # vertex -> (item, corner) and vertex -> (face, corner): stable sorts keep the slots of a vertex ascending
        corner_vertex = triples[item_tid].reshape(-1)
        self.S, self.V, self.F, self.T, self.M, self.I = S, V, vi.shape[0], T, M, I
        self.vi = vi.to(_I32).contiguous()
        self.vf_start, self.vf_slot = self._csr(vi.reshape(-1), V)
        self.vt_start, self.vt_slot = self._csr(corner_vertex, V)
        self.texel_rec, self.triples = rec, triples.to(_I32).contiguous()
        self.triple_start, self.texel_of = triple_start.to(_I32), texel_of.to(_I32)
        self.item_start, self.item_tid = item_start.to(_I32), item_tid.to(_I32)
        self.device = dev

    @staticmethod
    def _csr(keys, n):
        start = torch.zeros(n + 1, dtype=torch.long, device=keys.device)
        start[1:] = torch.bincount(keys, minlength=n).cumsum(0)
        return start.to(_I32), torch.argsort(keys, stable=True).to(_I32)

    def to(self, device):
        device = torch.device(device)
        if device == self.device:
            return self
        new = object.__new__(UVTopology)
        new.__dict__.update(self.__dict__)
        for name in self._TENSORS:
            setattr(new, name, getattr(self, name).to(device))
        new.device = new.vi.device
        return new

    def covered_mask(self):
        """[S,S] bool: the texels `values_to_uv` writes."""
        return (self.texel_rec[:, 0] >= 0).reshape(self.S, self.S)


# ---- one marshaller per C-ABI entry: keywords = the header's parameter names; a pointer is a GPU tensor (checked), a
# device address or None; stream = the current one ------------------------------------------------------------------------
def _p(x, dtype=_F32, name="tensor"):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else _lib.ptr(x, dtype, name)


def _abi_vert_normals_fwd(*, B, V, F, verts, vi, vf_start, vf_slot, eps, vn):
    _lib.call("gol_vert_normals_fwd", c_int(B), c_int(V), c_int(F), _p(verts), _p(vi, _I32), _p(vf_start, _I32),
              _p(vf_slot, _I32), c_float(eps), _p(vn), stream_ptr())


def _abi_vert_normals_bwd(*, B, V, F, verts, vi, vf_start, vf_slot, eps, g_vn, g_s, g_verts):
    _lib.call("gol_vert_normals_bwd", c_int(B), c_int(V), c_int(F), _p(verts), _p(vi, _I32), _p(vf_start, _I32),
              _p(vf_slot, _I32), c_float(eps), _p(g_vn), _p(g_s), _p(g_verts), stream_ptr())


def _abi_values_to_uv_fwd(*, B, V, C, S, T, values, texel_rec, triples, out):
    _lib.call("gol_values_to_uv_fwd", c_int(B), c_int(V), c_int(C), c_int(S), c_int(T), _p(values), _p(texel_rec, _I32),
              _p(triples, _I32), _p(out), stream_ptr())


def _abi_values_to_uv_bwd(*, B, V, C, S, T, I, texel_rec, item_start, texel_of, vt_start, vt_slot, g_out, item_sums,
                          g_values):
    _lib.call("gol_values_to_uv_bwd", c_int(B), c_int(V), c_int(C), c_int(S), c_int(T), c_int(I), _p(texel_rec, _I32),
              _p(item_start, _I32), _p(texel_of, _I32), _p(vt_start, _I32), _p(vt_slot, _I32), _p(g_out), _p(item_sums),
              _p(g_values), stream_ptr())


def _abi_uvgeom_fwd(*, B, V, F, S, T, verts, vi, vf_start, vf_slot, texel_rec, triples, vn_eps, norm_eps, vn, postex, tn):
    _lib.call("gol_uvgeom_fwd", c_int(B), c_int(V), c_int(F), c_int(S), c_int(T), _p(verts), _p(vi, _I32),
              _p(vf_start, _I32), _p(vf_slot, _I32), _p(texel_rec, _I32), _p(triples, _I32), c_float(vn_eps),
              c_float(norm_eps), _p(vn), _p(postex), _p(tn), stream_ptr())


def _abi_uvgeom_bwd(*, B, V, F, S, T, I, verts, vi, vf_start, vf_slot, texel_rec, triples, item_start, item_tid, texel_of,
                    vt_start, vt_slot, vn_eps, norm_eps, vn, g_postex, g_tn, item_sums, g_s, g_verts):
    _lib.call("gol_uvgeom_bwd", c_int(B), c_int(V), c_int(F), c_int(S), c_int(T), c_int(I), _p(verts), _p(vi, _I32),
              _p(vf_start, _I32), _p(vf_slot, _I32), _p(texel_rec, _I32), _p(triples, _I32), _p(item_start, _I32),
              _p(item_tid, _I32), _p(texel_of, _I32), _p(vt_start, _I32), _p(vt_slot, _I32), c_float(vn_eps),
              c_float(norm_eps), _p(vn), _p(g_postex), _p(g_tn), _p(item_sums), _p(g_s), _p(g_verts), stream_ptr())


def _f32(t):
    return None if t is None else t.detach().to(_F32).contiguous()


def _check(name, x, topo, last=None):
    if not isinstance(topo, UVTopology):
        raise TypeError(f"{name}: topo must be a UVTopology")
    if not x.is_cuda:
        raise _lib.GoliathHipError(f"{name} needs CUDA(HIP) tensors; there is no CPU path")
    if topo.device != x.device:
        raise _lib.GoliathHipError(f"{name}: the topology is on {topo.device}, the tensor on {x.device} (use topo.to())")
    if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] != topo.V or (last is not None and x.shape[2] != last) or x.shape[2] < 1:
        raise _lib.GoliathHipError(f"{name}: expected [B, {topo.V}, {last or 'C'}], got {tuple(x.shape)}")


def _saved(ctx):
    """The saved tensors; a second backward (buffers freed) raises RuntimeError, as for any autograd node."""
    return ctx.saved_tensors


class _VertNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, topo, eps):
        v = _f32(verts)
        B, V = v.shape[:2]
        vn = torch.empty_like(v)
        with _lib.device_guard(v.device):
            _abi_vert_normals_fwd(B=B, V=V, F=topo.F, verts=v, vi=topo.vi, vf_start=topo.vf_start, vf_slot=topo.vf_slot,
                                  eps=eps, vn=vn)
        ctx.save_for_backward(v)
        ctx.topo, ctx.eps, ctx.dtype = topo, eps, verts.dtype
        return vn.to(verts.dtype)

    @staticmethod
    def backward(ctx, g_vn):
        (v,) = _saved(ctx)
        topo = ctx.topo
        B, V = v.shape[:2]
        g_s, g_verts = torch.empty_like(v), torch.empty_like(v)
        with _lib.device_guard(v.device):
            _abi_vert_normals_bwd(B=B, V=V, F=topo.F, verts=v, vi=topo.vi, vf_start=topo.vf_start, vf_slot=topo.vf_slot,
                                  eps=ctx.eps, g_vn=_f32(g_vn), g_s=g_s, g_verts=g_verts)
        return g_verts.to(ctx.dtype), None, None


class _ValuesToUV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, topo):
        v = _f32(values)
        B, V, C = v.shape
        out = torch.empty(B, C, topo.S, topo.S, device=v.device)
        with _lib.device_guard(v.device):
            _abi_values_to_uv_fwd(B=B, V=V, C=C, S=topo.S, T=topo.T, values=v, texel_rec=topo.texel_rec,
                                  triples=topo.triples, out=out)
        ctx.topo, ctx.shape, ctx.dtype = topo, (B, V, C), values.dtype
        ctx.save_for_backward(out.new_empty(0))   # nothing of the forward is needed; kept so that a second backward raises
        return out.to(values.dtype)

    @staticmethod
    def backward(ctx, g_out):
        _saved(ctx)
        topo, (B, V, C) = ctx.topo, ctx.shape
        g_out = _f32(g_out)
        item_sums = torch.empty(B, max(topo.I, 1), 3, C, device=g_out.device)
        g_values = torch.empty(B, V, C, device=g_out.device)
        with _lib.device_guard(g_out.device):
            _abi_values_to_uv_bwd(B=B, V=V, C=C, S=topo.S, T=topo.T, I=topo.I, texel_rec=topo.texel_rec,
                                  item_start=topo.item_start, texel_of=topo.texel_of, vt_start=topo.vt_start,
                                  vt_slot=topo.vt_slot, g_out=g_out, item_sums=item_sums, g_values=g_values)
        return g_values.to(ctx.dtype), None


class _UVGeometry(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, topo, vn_eps, norm_eps):
        v = _f32(verts)
        B, V = v.shape[:2]
        vn = torch.empty_like(v)                                   # the scratch the backward reuses
        postex = torch.empty(B, 3, topo.S, topo.S, device=v.device)
        tn = torch.empty_like(postex)
        with _lib.device_guard(v.device):
            _abi_uvgeom_fwd(B=B, V=V, F=topo.F, S=topo.S, T=topo.T, verts=v, vi=topo.vi, vf_start=topo.vf_start,
                            vf_slot=topo.vf_slot, texel_rec=topo.texel_rec, triples=topo.triples, vn_eps=vn_eps,
                            norm_eps=norm_eps, vn=vn, postex=postex, tn=tn)
        ctx.save_for_backward(v, vn)
        ctx.topo, ctx.eps, ctx.dtype = topo, (vn_eps, norm_eps), verts.dtype
        return postex.to(verts.dtype), tn.to(verts.dtype)

    @staticmethod
    def backward(ctx, g_postex, g_tn):
        v, vn = _saved(ctx)
        topo = ctx.topo
        B, V = v.shape[:2]
        item_sums = torch.empty(B, max(topo.I, 1), 18, device=v.device)
        g_s, g_verts = torch.empty_like(v), torch.empty_like(v)
        with _lib.device_guard(v.device):
            _abi_uvgeom_bwd(B=B, V=V, F=topo.F, S=topo.S, T=topo.T, I=topo.I, verts=v, vi=topo.vi, vf_start=topo.vf_start,
                            vf_slot=topo.vf_slot, texel_rec=topo.texel_rec, triples=topo.triples,
                            item_start=topo.item_start, item_tid=topo.item_tid, texel_of=topo.texel_of,
                            vt_start=topo.vt_start, vt_slot=topo.vt_slot, vn_eps=ctx.eps[0], norm_eps=ctx.eps[1], vn=vn,
                            g_postex=_f32(g_postex), g_tn=_f32(g_tn), item_sums=item_sums, g_s=g_s, g_verts=g_verts)
        return g_verts.to(ctx.dtype), None, None, None


def vert_normals(verts, topo, eps=1e-5):
    """verts[B,V,3] -> unit vertex normals [B,V,3]: the reference's vert_normals(verts, vi, eps) (geom.py:337-346)."""
    _check("vert_normals", verts, topo, last=3)
    return _VertNormals.apply(verts, topo, float(eps))


def values_to_uv(values, topo):
    """values[B,V,C] -> [B,C,S,S]: the reference's values_to_uv (geom.py:308-324); zero where uncovered."""
    _check("values_to_uv", values, topo)
    return _ValuesToUV.apply(values, topo)


def uv_geometry(verts, topo, norm_eps=1e-12, vn_eps=1e-5):
    """verts[B,V,3] -> (postex[B,3,S,S], tn[B,3,S,S]) = (to_uv(verts), normalize(to_uv(vn(verts)), dim=1)), the first lines
    of PrimDecoder.forward (rgca.py:483-491).  norm_eps: F.normalize's 1e-12; URHand's interpolated normal uses 1e-5."""
    _check("uv_geometry", verts, topo, last=3)
    return _UVGeometry.apply(verts, topo, float(vn_eps), float(norm_eps))


# ---- binding to a GeometryModule-shaped object (buffers vi, index_image, bary_image) ---------------------------------------
def topology_of(geo_fn, n_verts):
    """The packed topology of a module that owns `vi`, `index_image` and `bary_image`, built on first use, cached on the
    module, rebuilt when a buffer's device, shape or storage (or the vertex count) changes.  None if a buffer is missing."""
    bufs = tuple(getattr(geo_fn, k, None) for k in ("vi", "index_image", "bary_image"))
    if not all(torch.is_tensor(b) for b in bufs):
        return None
    key = (int(n_verts),) + tuple((b.device, tuple(b.shape), b.data_ptr(), b._version) for b in bufs)
    cached = geo_fn.__dict__.get("_gol_uv_topology")
    if cached is None or cached[0] != key:
        cached = (key, UVTopology(*bufs, n_verts=n_verts))
        geo_fn.__dict__["_gol_uv_topology"] = cached
    return cached[1]


def geometry_to_uv(self, values):
    """GeometryModule.to_uv (geom.py:270-271) on gol_values_to_uv."""
    return values_to_uv(values, topology_of(self, values.shape[1]))


def geometry_vn(self, verts):
    """GeometryModule.vn (geom.py:267-268) on gol_vert_normals."""
    return vert_normals(verts, topology_of(self, verts.shape[1]))


def fused_topology(geo_fn, n_verts):
    """The topology `prim_decoder_forward` may use for ONE uv_geometry call: only for a geo_fn whose class was patched by
    dropin.patch_geometry() or that carries a packed topology (`geo_fn.uv_topology`, a UVTopology).  None otherwise: the
    caller keeps the reference's three calls."""
    own = getattr(geo_fn, "uv_topology", None)
    if isinstance(own, UVTopology):
        return own
    if getattr(type(geo_fn), "to_uv", None) is geometry_to_uv and getattr(type(geo_fn), "vn", None) is geometry_vn:
        return topology_of(geo_fn, n_verts)
    return None
