"""URHand's per-texel tangent frames, normal map and view conditioning on the HIP kernels of csrc/uvframes.hip.

    UVFramesTopology(geo_fn)          the constant topology of a GeometryModule-shaped object, packed once
    uv_frames(verts, topo, *, posmap=None, flip_normal=False, cam_pos=None, want_frames=False) -> nml, viewout, frames

replaces, in ConvTeacherDecoder.forward, ca_code/models/urhand.py:366-392 (posmap=None: normals interpolated from the vertex
normals), :467-486 (posmap given: xyz2normals(posmap)) and :573-578 (cam_pos given: the frame applied to the normalised view
vector), i.e. compute_tbn_uv_given_normal / xyz2normals / vert_normals of ca_code/utils/geom.py.  The numerics are stated
line by line in include/goliath_hip.h.  One forward and one backward pass over the map on the current stream, no host
sync, no atomics, bitwise reproducible.  Every tensor must be on the GPU: there is no CPU path.
"""
import ctypes

import torch

from . import _lib
from ._lib import c_int, stream_ptr
from .uvgeom import UVTopology

_F32, _I32 = torch.float32, torch.int32
_BUFFERS = ("vi", "vt", "v2uv", "index_image", "face_index_image", "bary_image")


class UVFramesTopology:
    """The constant part of URHand's frames, packed for the kernels.

    geo_fn: an object with the buffers of ca_code.utils.geom.GeometryModule: vi[F,3], vt[Vt,2], v2uv[V,n] (its FIRST column
    is used, urhand.py:369), index_image[S,S,3], face_index_image[S,S], bary_image[S,S,3].  A texel is covered when
    `(index_image != -1).any(-1)` (urhand.py:367); a covered texel with an id of -1 is rejected (the reference would read
    the last vertex for it).  Attributes: geo (the UVTopology of index_image), nrm (the UVTopology of
    vi[face_index_image], the triple the normals are interpolated over; `geo` itself where the two images agree
    everywhere), tri_const[T,4] = (f, vt01.y, vt02.y, 0) in float32 by the reference's own operations (geom.py:448-454),
    tri_item_start[T+1], vq_start[V+1], vq_slot[3T] (vertex -> (triple, corner) slots, ascending)."""

    def __init__(self, geo_fn, n_verts=None):
        bufs = {k: getattr(geo_fn, k, None) for k in _BUFFERS}
        missing = [k for k, v in bufs.items() if not torch.is_tensor(v)]
        if missing:
            raise ValueError(f"geo_fn lacks the buffers {missing}")
        idx = bufs["index_image"]
        dev = idx.device
        vi, vt, v2uv = bufs["vi"].to(dev).long(), bufs["vt"].to(dev).to(_F32), bufs["v2uv"].to(dev).long()
        face = bufs["face_index_image"].to(dev).long()
        if vt.dim() != 2 or vt.shape[1] != 2:
            raise ValueError(f"vt must be [Vt,2], got {tuple(vt.shape)}")
        if v2uv.dim() != 2 or v2uv.shape[1] < 1:
            raise ValueError(f"v2uv must be [V,n], got {tuple(v2uv.shape)}")
        if idx.dim() != 3 or tuple(face.shape) != tuple(idx.shape[:2]):
            raise ValueError("face_index_image must be [S,S] for an index_image [S,S,3]")
        mask = (idx != -1).any(-1)
        if not torch.equal(mask, (idx != -1).all(-1)):
            raise ValueError("a covered texel of index_image has an id of -1")
        self.geo = UVTopology(vi, idx, bufs["bary_image"].to(dev), n_verts=n_verts)
        V, T = self.geo.V, self.geo.T
        if v2uv.shape[0] < V:
            raise ValueError(f"v2uv has {v2uv.shape[0]} rows for {V} vertices")
        if bool(((face[mask] < 0) | (face[mask] >= vi.shape[0])).any()):
            raise ValueError(f"face_index_image must lie in [0, {vi.shape[0]}) on the covered texels")
        nidx = torch.full_like(idx.long(), -1)
        nidx[mask] = vi[face[mask]]
        self.nrm = self.geo if torch.equal(nidx, idx.long()) else UVTopology(vi, nidx, bufs["bary_image"].to(dev), n_verts=V)
        triples = self.geo.triples.long()
        slot0 = v2uv[triples, 0]
        if T and (int(slot0.min()) < 0 or int(slot0.max()) >= vt.shape[0]):
            raise ValueError(f"v2uv[:, 0] must lie in [0, {vt.shape[0]}) for the vertices of the covered texels")
        tri_uv = vt[slot0]                                                       # [T,3,2], urhand.py:369
        vt01, vt02 = tri_uv[:, 1] - tri_uv[:, 0], tri_uv[:, 2] - tri_uv[:, 0]   # geom.py:448-454, float32
        fin = vt01[..., 0] * vt02[..., 1] - vt01[..., 1] * vt02[..., 0]
        fin[torch.abs(fin) < 1.0e-8] = 1.0e-8
        f = 1.0 / fin
        self.tri_const = torch.stack([f, vt01[..., 1], vt02[..., 1], torch.zeros_like(f)], -1).contiguous()
        self.tri_item_start = torch.searchsorted(self.geo.item_tid.long().contiguous(),
                                                 torch.arange(T + 1, device=dev)).to(_I32)
        self.vq_start, self.vq_slot = UVTopology._csr(triples.reshape(-1), V)
        self.S, self.V, self.T, self.device = self.geo.S, V, T, dev

    def to(self, device):
        device = torch.device(device)
        if device == self.device:
            return self
        new = object.__new__(UVFramesTopology)
        new.__dict__.update(self.__dict__)
        new.geo = self.geo.to(device)
        new.nrm = new.geo if self.nrm is self.geo else self.nrm.to(device)
        for name in ("tri_const", "tri_item_start", "vq_start", "vq_slot"):
            setattr(new, name, getattr(self, name).to(device))
        new.device = new.tri_const.device
        return new

    def covered_mask(self):
        """[S,S] bool: the texels that receive a frame."""
        return self.geo.covered_mask()


# ---- one marshaller per C-ABI entry: keywords = the header's parameter names ----------------------------------------------
def _p(x, dtype=_F32, name="tensor"):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else _lib.ptr(x, dtype, name)


def _abi_uvframes_bwd_scratch_floats(*, B, V, S, T, I, In, mode):
    fn = _lib.load().gol_uvframes_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    return int(fn(c_int(B), c_int(V), c_int(S), c_int(T), c_int(I), c_int(In), c_int(mode)))


def _abi_uvframes_fwd(*, B, V, F, S, T, Tn, mode, flip_normal, verts, vi, vf_start, vf_slot, texel_rec, triples, tri_const,
                      ntexel_rec, ntriples, posmap, cam_pos, vn, t0, nml, viewout, frames):
    _lib.call("gol_uvframes_fwd", c_int(B), c_int(V), c_int(F), c_int(S), c_int(T), c_int(Tn), c_int(mode),
              c_int(flip_normal), _p(verts), _p(vi, _I32), _p(vf_start, _I32), _p(vf_slot, _I32), _p(texel_rec, _I32),
              _p(triples, _I32), _p(tri_const), _p(ntexel_rec, _I32), _p(ntriples, _I32), _p(posmap), _p(cam_pos), _p(vn),
              _p(t0), _p(nml), _p(viewout), _p(frames), stream_ptr())


def _abi_uvframes_bwd(*, B, V, F, S, T, Tn, I, In, mode, flip_normal, verts, vi, vf_start, vf_slot, texel_rec, triples,
                      tri_const, item_start, texel_of, tri_item_start, vq_start, vq_slot, ntexel_rec, ntriples, nitem_start,
                      ntexel_of, nvt_start, nvt_slot, posmap, cam_pos, vn, t0, g_nml, g_viewout, g_frames, scratch, g_verts,
                      g_posmap, g_cam_pos):
    _lib.call("gol_uvframes_bwd", c_int(B), c_int(V), c_int(F), c_int(S), c_int(T), c_int(Tn), c_int(I), c_int(In),
              c_int(mode), c_int(flip_normal), _p(verts), _p(vi, _I32), _p(vf_start, _I32), _p(vf_slot, _I32),
              _p(texel_rec, _I32), _p(triples, _I32), _p(tri_const), _p(item_start, _I32), _p(texel_of, _I32),
              _p(tri_item_start, _I32), _p(vq_start, _I32), _p(vq_slot, _I32), _p(ntexel_rec, _I32), _p(ntriples, _I32),
              _p(nitem_start, _I32), _p(ntexel_of, _I32), _p(nvt_start, _I32), _p(nvt_slot, _I32), _p(posmap), _p(cam_pos),
              _p(vn), _p(t0), _p(g_nml), _p(g_viewout), _p(g_frames), _p(scratch), _p(g_verts), _p(g_posmap),
              _p(g_cam_pos), stream_ptr())


def _f32(t):
    return None if t is None else t.detach().to(_F32).contiguous()


def _topology_args(topo):
    g, n = topo.geo, topo.nrm
    return dict(vi=g.vi, vf_start=g.vf_start, vf_slot=g.vf_slot, texel_rec=g.texel_rec, triples=g.triples,
                tri_const=topo.tri_const, ntexel_rec=n.texel_rec, ntriples=n.triples)


class _UVFrames(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, posmap, cam_pos, topo, mode, flip_normal, want_frames):
        v, pm, cam = _f32(verts), _f32(posmap), _f32(cam_pos)
        g, n = topo.geo, topo.nrm
        B, V, S = v.shape[0], topo.V, topo.S
        vn = torch.empty_like(v) if mode == 0 else None            # kept for the backward, like t0
        t0 = torch.empty(B, max(topo.T, 1), 3, device=v.device)
        nml = torch.empty(B, 3, S, S, device=v.device)
        viewout = torch.empty_like(nml) if cam is not None else None
        frames = torch.empty(B, S, S, 3, 3, device=v.device) if want_frames else None
        with _lib.device_guard(v.device):
            _abi_uvframes_fwd(B=B, V=V, F=g.F, S=S, T=g.T, Tn=n.T, mode=mode, flip_normal=int(flip_normal), verts=v,
                              posmap=pm, cam_pos=cam, vn=vn, t0=t0, nml=nml, viewout=viewout, frames=frames,
                              **_topology_args(topo))
        none = v.new_empty(0)
        ctx.save_for_backward(v, none if pm is None else pm, none if cam is None else cam, none if vn is None else vn, t0)
        ctx.topo, ctx.mode, ctx.flip = topo, mode, int(flip_normal)
        ctx.have = (pm is not None, cam is not None)
        ctx.dtypes = (verts.dtype, None if posmap is None else posmap.dtype, None if cam_pos is None else cam_pos.dtype)
        cast = lambda t: None if t is None else t.to(verts.dtype)
        return cast(nml), cast(viewout), cast(frames)

    @staticmethod
    def backward(ctx, g_nml, g_viewout, g_frames):
        v, pm, cam, vn, t0 = ctx.saved_tensors       # a second backward (buffers freed) raises, as for any autograd node
        topo, mode = ctx.topo, ctx.mode
        g, n = topo.geo, topo.nrm
        have_pm, have_cam = ctx.have
        pm, cam, vn = (pm if have_pm else None), (cam if have_cam else None), (vn if mode == 0 else None)
        B, V, S = v.shape[0], topo.V, topo.S
        want_cam = have_cam and ctx.needs_input_grad[2]
        g_verts = torch.empty_like(v)
        g_posmap = torch.empty_like(pm) if have_pm and (mode == 1 or have_cam) else None
        g_cam = torch.empty_like(cam) if want_cam else None
        with _lib.device_guard(v.device):
            scratch = torch.empty(_abi_uvframes_bwd_scratch_floats(B=B, V=V, S=S, T=g.T, I=g.I, In=n.I, mode=mode),
                                  device=v.device)
            _abi_uvframes_bwd(B=B, V=V, F=g.F, S=S, T=g.T, Tn=n.T, I=g.I, In=n.I, mode=mode, flip_normal=ctx.flip, verts=v,
                              item_start=g.item_start, texel_of=g.texel_of, tri_item_start=topo.tri_item_start,
                              vq_start=topo.vq_start, vq_slot=topo.vq_slot, nitem_start=n.item_start, ntexel_of=n.texel_of,
                              nvt_start=n.vt_start, nvt_slot=n.vt_slot, posmap=pm, cam_pos=cam, vn=vn, t0=t0,
                              g_nml=_f32(g_nml), g_viewout=_f32(g_viewout) if have_cam else None, g_frames=_f32(g_frames),
                              scratch=scratch, g_verts=g_verts, g_posmap=g_posmap, g_cam_pos=g_cam,
                              **_topology_args(topo))
        dv, dp, dc = ctx.dtypes
        return (g_verts.to(dv), None if g_posmap is None else g_posmap.to(dp), None if g_cam is None else g_cam.to(dc),
                None, None, None, None)


def uv_frames(verts, topo, *, posmap=None, flip_normal=False, cam_pos=None, want_frames=False, normals_from_posmap=None):
    """verts[B,V,3] -> (nml[B,3,S,S], viewout[B,3,S,S] or None, frames[B,S,S,3,3] or None); zeros where uncovered.

    posmap=None: the normals are the vertex normals of `verts` interpolated over vi[face_index_image] (urhand.py:375-383).
    posmap[B,3,S,S]: the normals are xyz2normals(posmap) (urhand.py:467-468); normals_from_posmap=False keeps the
    interpolated ones and uses posmap for the view vector only.  flip_normal: rows (t, -b, -n) instead of (t, -b, n).
    cam_pos[B,3] (needs posmap): viewout = frame . normalize(cam_pos - posmap) (urhand.py:573-578).  nml is the frame's
    third row as the planar map the light kernels read; frames only with want_frames (the decoder never needs it).
    Gradients reach verts, posmap and cam_pos."""
    if not isinstance(topo, UVFramesTopology):
        raise TypeError("uv_frames: topo must be a UVFramesTopology")
    if not verts.is_cuda:
        raise _lib.GoliathHipError("uv_frames needs CUDA(HIP) tensors; there is no CPU path")
    if topo.device != verts.device:
        raise _lib.GoliathHipError(f"uv_frames: the topology is on {topo.device}, verts on {verts.device} (use topo.to())")
    if verts.dim() != 3 or verts.shape[0] < 1 or tuple(verts.shape[1:]) != (topo.V, 3):
        raise _lib.GoliathHipError(f"uv_frames: verts must be [B, {topo.V}, 3], got {tuple(verts.shape)}")
    B, S = verts.shape[0], topo.S
    if posmap is not None and (tuple(posmap.shape) != (B, 3, S, S) or posmap.device != verts.device):
        raise _lib.GoliathHipError(f"uv_frames: posmap must be [{B}, 3, {S}, {S}] on {verts.device}")
    if cam_pos is not None:
        if posmap is None:
            raise _lib.GoliathHipError("uv_frames: cam_pos needs posmap (the view vector is cam_pos - posmap)")
        if tuple(cam_pos.shape) != (B, 3) or cam_pos.device != verts.device:
            raise _lib.GoliathHipError(f"uv_frames: cam_pos must be [{B}, 3] on {verts.device}")
    if normals_from_posmap is None:
        normals_from_posmap = posmap is not None
    if normals_from_posmap and posmap is None:
        raise _lib.GoliathHipError("uv_frames: normals_from_posmap needs posmap")
    return _UVFrames.apply(verts, posmap, cam_pos, topo, 1 if normals_from_posmap else 0, bool(flip_normal),
                           bool(want_frames))


def topology_of(decoder):
    """The packed topology of a decoder's `geo_fn`, built on first use and cached on the decoder; rebuilt when a buffer's
    device, shape or storage changes."""
    gf = decoder.geo_fn
    bufs = tuple(getattr(gf, k, None) for k in _BUFFERS)
    key = tuple((b.device, tuple(b.shape), b.data_ptr(), b._version) if torch.is_tensor(b) else None for b in bufs)
    cached = decoder.__dict__.get("_gol_uv_frames_topology")
    if cached is None or cached[0] != key:
        cached = (key, UVFramesTopology(gf))
        decoder.__dict__["_gol_uv_frames_topology"] = cached
    return cached[1]
