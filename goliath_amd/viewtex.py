"""Camera images unwrapped into UV space, and their mean over many views, on the HIP kernels of csrc/viewtex.hip: the
per-camera body of the reference's ca_code/scripts/run_gen_texmean.py:83-108 (through ca_code/utils/tex.py:21-63 and
ca_code/utils/geom.py:834-910), which gives the URHand / RGCA models the `tex_mean` of a new capture.

    ViewTexTopology(index_image_uv, bary_image_uv, face_index_uv)   the three UV images packed once (int32, contiguous)
    face_visibility(index_img, n_faces)                             compute_face_visibility (geom.py:834-845), bool [B,F]
    uv_visibility(index_img, n_faces, face_index_uv)                compute_uv_visiblity_face (geom.py:847-859), bool [B,S,S]
    compute_view_texture(verts, faces, image, face_index_image,     compute_view_texture (geom.py:862-910): (tex, mask)
                         normal_image, K, Rt, index_image_uv,
                         bary_image_uv, face_index_uv, ...)
    TexMean(topology, n_faces, device)                              the script's two accumulators: .add(...) per batch of
                                                                    cameras, .mean(...) at the end
    get_tex_rl(rl, image, ply, extrin, intrin, face_index,          tex.py:21-63, any B, no dummy texture render
               index_image, bary_image)

Per view and texel, in fp32 in the reference's order: xyz = sum_k verts[idx_k] bary_k; p = K (R xyz + t) with the full
3x3 K; pix = p.xy / p.z; grid_sample(nearest, align_corners=False, border padding) of the image at 2 pix / (W, H) - 1;
times the texel's visibility (its face appears in the view's face index image); times all_c(value_c <= threshold) when
an intensity threshold is given.

STATED behaviour:
  * only the face index image matters for visibility: a sample behind the camera (p.z < 0) is taken like any other -- the
    reference has no depth test;
  * p.z == 0 or a non-finite pixel coordinate gives the texel the value 0 for that view (the reference's result there is
    unspecified);
  * a texel that is not visible gives exactly 0 even if the image holds NaN there (the reference gives NaN * 0 = NaN);
  * a face index outside [-1, F) in the camera's index image is ignored (the reference would raise);
  * `normal_image` and `normal_threshold` are accepted and unused, as in the reference;
  * `intensity_threshold` of None or 0 means no filter: the reference's truthiness test.

Every tensor must be on the GPU: there is no CPU path.  Nothing here syncs the host, so a frame's cameras go through as
one batch and the accumulate mode writes no [B,3,S,S] tensor at all.
"""
import ctypes

import torch

from . import _lib
from ._lib import c_float, c_i64, c_int, stream_ptr

_F32, _I32, _I64, _U8 = torch.float32, torch.int32, torch.int64, torch.uint8


# ---- one marshaller per C-ABI entry: keywords = the header's parameter names; a pointer is a GPU tensor (checked), a
# device address or None; stream = the current one ------------------------------------------------------------------------
def _p(x, dtype=_F32, name="tensor"):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else _lib.ptr(x, dtype, name)


def _abi_face_visibility(*, B, F, H, W, index_img, face_vis):
    _lib.call("gol_face_visibility", c_int(B), c_int(F), c_int(H), c_int(W), _p(index_img, _I32), _p(face_vis, None),
              stream_ptr())


def _abi_view_texture(*, B, V, F, H, W, S_h, S_w, verts, verts_bstride, image, K, Rt, index_image_uv, bary_image_uv,
                      face_index_uv, face_vis, has_threshold=0, intensity_threshold=0.0, tex=None, mask=None, total=None,
                      cnt=None):
    _lib.call("gol_view_texture", c_int(B), c_int(V), c_int(F), c_int(H), c_int(W), c_int(S_h), c_int(S_w), _p(verts),
              c_i64(verts_bstride), _p(image), _p(K), _p(Rt), _p(index_image_uv, _I32), _p(bary_image_uv),
              _p(face_index_uv, _I32), _p(face_vis, None), c_int(has_threshold), c_float(intensity_threshold), _p(tex),
              _p(mask, None), _p(total), _p(cnt), stream_ptr())


def _abi_texmean_finalize(*, S_h, S_w, total, cnt, eps, flip_rows, bgr, out):
    _lib.call("gol_texmean_finalize", c_int(S_h), c_int(S_w), _p(total), _p(cnt), c_float(eps), c_int(flip_rows),
              c_int(bgr), _p(out), stream_ptr())


def _need_gpu(name, *tensors):
    for t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.GoliathHipError(f"{name} needs CUDA(HIP) tensors; there is no CPU path")


class ViewTexTopology:
    """index_image_uv[S_h,S_w,3] (int64 or int32, -1 = empty), bary_image_uv[S_h,S_w,3] float, face_index_uv[S_h,S_w]
    (int64 or int32) -- the outputs of uvtopo.index_images(...) or a GeometryModule's buffers -- as the contiguous int32 /
    float32 device arrays the kernels read."""

    def __init__(self, index_image_uv, bary_image_uv, face_index_uv):
        _need_gpu("ViewTexTopology", index_image_uv, bary_image_uv, face_index_uv)
        if index_image_uv.dim() != 3 or index_image_uv.shape[2] != 3:
            raise ValueError(f"index_image_uv must be [S_h,S_w,3], got {tuple(index_image_uv.shape)}")
        if tuple(bary_image_uv.shape) != tuple(index_image_uv.shape):
            raise ValueError(f"bary_image_uv must have index_image_uv's shape, got {tuple(bary_image_uv.shape)}")
        if tuple(face_index_uv.shape) != tuple(index_image_uv.shape[:2]):
            raise ValueError(f"face_index_uv must be [S_h,S_w] = {tuple(index_image_uv.shape[:2])}, "
                             f"got {tuple(face_index_uv.shape)}")
        if index_image_uv.dtype not in (_I32, _I64) or face_index_uv.dtype not in (_I32, _I64):
            raise ValueError("index_image_uv and face_index_uv must be int32 or int64")
        dev = index_image_uv.device
        self.S_h, self.S_w = int(index_image_uv.shape[0]), int(index_image_uv.shape[1])
        self.device = dev
        self.index_image_uv = index_image_uv.detach().to(_I32).contiguous()
        self.bary_image_uv = bary_image_uv.detach().to(device=dev, dtype=_F32).contiguous()
        self.face_index_uv = face_index_uv.detach().to(device=dev, dtype=_I32).contiguous()


def _index_img(name, index_img):
    _need_gpu(name, index_img)
    if index_img.dim() != 3:
        raise ValueError(f"the face index image must be [B,H,W], got {tuple(index_img.shape)}")
    if index_img.dtype not in (_I32, _I64):
        raise ValueError("the face index image must be int32 or int64")
    return index_img.detach().to(_I32).contiguous()


def _face_vis(index_img32, n_faces):
    """index_img32[B,H,W] int32 -> uint8 [B,F]; the caller holds the device guard."""
    B, H, W = index_img32.shape
    face_vis = torch.empty(B, int(n_faces), dtype=_U8, device=index_img32.device)   # (the entry zeroes it)
    _abi_face_visibility(B=B, F=int(n_faces), H=H, W=W, index_img=index_img32, face_vis=face_vis)
    return face_vis


def face_visibility(index_img, n_faces):
    """compute_face_visibility (geom.py:834-845) with `faces.shape[0]` passed as a number: index_img[B,H,W] int32 / int64
    (-1 = empty) -> bool [B,F]."""
    index_img = _index_img("face_visibility", index_img)
    with _lib.device_guard(index_img.device):
        return _face_vis(index_img, n_faces).view(torch.bool)


def _launch(topo, n_faces, verts, image, K, Rt, face_vis, intensity_threshold, tex=None, mask=None, total=None, cnt=None):
    B, _, H, W = image.shape
    _abi_view_texture(B=B, V=verts.shape[1], F=int(n_faces), H=H, W=W, S_h=topo.S_h, S_w=topo.S_w, verts=verts,
                      verts_bstride=0 if verts.shape[0] == 1 else verts.shape[1] * 3, image=image, K=K, Rt=Rt,
                      index_image_uv=topo.index_image_uv, bary_image_uv=topo.bary_image_uv,
                      face_index_uv=topo.face_index_uv, face_vis=face_vis, has_threshold=int(bool(intensity_threshold)),
                      intensity_threshold=float(intensity_threshold) if intensity_threshold else 0.0, tex=tex, mask=mask,
                      total=total, cnt=cnt)


def _views(name, verts, image, K, Rt):
    """The per-view inputs as contiguous float32: verts[B or 1,V,3], image[B,3,H,W], K[B,3,3], Rt[B,3,4]."""
    _need_gpu(name, verts, image, K, Rt)
    if image.dim() != 4 or image.shape[1] != 3:
        raise ValueError(f"image must be [B,3,H,W], got {tuple(image.shape)}")
    if image.dtype != _F32:
        raise ValueError(f"image must be float32, got {image.dtype}")
    B = image.shape[0]
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[0] not in (1, B):
        raise ValueError(f"verts must be [B,V,3] or [1,V,3] with B = {B}, got {tuple(verts.shape)}")
    if tuple(K.shape) != (B, 3, 3) or Rt.dim() != 3 or Rt.shape[0] != B or Rt.shape[1] < 3 or Rt.shape[2] != 4:
        raise ValueError(f"K must be [B,3,3] and Rt [B,3,4] with B = {B}, got {tuple(K.shape)} and {tuple(Rt.shape)}")
    f32 = lambda t: t.detach().to(_F32).contiguous()   # noqa: E731
    return f32(verts), image.detach().contiguous(), f32(K), f32(Rt[:, :3])


def uv_visibility(index_img, n_faces, face_index_uv):
    """compute_uv_visiblity_face (geom.py:847-859): bool [B,S_h,S_w], a texel's face appears in view b's index image."""
    index_img = _index_img("uv_visibility", index_img)
    _need_gpu("uv_visibility", face_index_uv)
    if face_index_uv.dim() != 2:
        raise ValueError(f"face_index_uv must be [S_h,S_w], got {tuple(face_index_uv.shape)}")
    S_h, S_w = face_index_uv.shape
    dev = index_img.device
    B, H, W = index_img.shape
    face32 = face_index_uv.detach().to(device=dev, dtype=_I32).contiguous()
    mask = torch.empty(B, S_h, S_w, dtype=torch.bool, device=dev)
    with _lib.device_guard(dev):
        face_vis = _face_vis(index_img, n_faces)
        # (the mask alone needs neither the mesh nor the images)
        _abi_view_texture(B=B, V=0, F=int(n_faces), H=H, W=W, S_h=S_h, S_w=S_w, verts=None, verts_bstride=0, image=None,
                          K=None, Rt=None, index_image_uv=None, bary_image_uv=None, face_index_uv=face32,
                          face_vis=face_vis, mask=mask)
    return mask


_TOPOLOGIES = {}   # (address, version, shape) of the three UV images -> ViewTexTopology; a handful of entries at most


def _cached_topology(index_image_uv, bary_image_uv, face_index_uv):
    key = tuple((t.data_ptr(), t._version, tuple(t.shape), t.dtype) for t in (index_image_uv, bary_image_uv, face_index_uv))
    topo = _TOPOLOGIES.get(key)
    if topo is None:
        if len(_TOPOLOGIES) >= 8:
            _TOPOLOGIES.clear()
        topo = _TOPOLOGIES[key] = ViewTexTopology(index_image_uv, bary_image_uv, face_index_uv)
        topo._sources = (index_image_uv, bary_image_uv, face_index_uv)   # keeps the addresses of the key alive
    return topo


def view_texture(topology, n_faces, verts, image, K, Rt, index_img, intensity_threshold=None):
    """compute_view_texture on a packed topology: (tex[B,3,S_h,S_w] float32, mask[B,1,S_h,S_w] bool)."""
    verts, image, K, Rt = _views("view_texture", verts, image, K, Rt)
    index_img = _index_img("view_texture", index_img)
    if tuple(index_img.shape) != (image.shape[0],) + tuple(image.shape[2:]):
        raise ValueError(f"the face index image must be [B,H,W] of image, got {tuple(index_img.shape)}")
    B, dev = image.shape[0], image.device
    tex = torch.empty(B, 3, topology.S_h, topology.S_w, dtype=_F32, device=dev)
    mask = torch.empty(B, 1, topology.S_h, topology.S_w, dtype=torch.bool, device=dev)
    with _lib.device_guard(dev):
        face_vis = _face_vis(index_img, n_faces)
        _launch(topology, n_faces, verts, image, K, Rt, face_vis, intensity_threshold, tex=tex, mask=mask)
    return tex, mask


def compute_view_texture(verts, faces, image, face_index_image, normal_image, K, Rt, index_image_uv, bary_image_uv,
                         face_index_uv, intensity_threshold=None, normal_threshold=None):
    """compute_view_texture (geom.py:862-910), its parameter list, shapes and dtypes: verts[B,V,3] (or [1,V,3]),
    faces[F,3], image[B,3,H,W] float32, face_index_image[B,H,W] int32 / int64, K[B,3,3], Rt[B,3,4], the three UV images
    -> (tex[B,3,S,S] float32, mask[B,1,S,S] bool).  normal_image and normal_threshold are unused, as in the reference.
    The UV images are packed on first use and kept, keyed by their addresses and versions."""
    _need_gpu("compute_view_texture", verts, image, face_index_image, K, Rt, index_image_uv, bary_image_uv, face_index_uv)
    topo = _cached_topology(index_image_uv, bary_image_uv, face_index_uv)
    return view_texture(topo, faces.shape[0], verts, image, K, Rt, face_index_image, intensity_threshold)


def _rasterized_index(verts, vi, K, Rt, H, W):
    from . import meshraster

    B = K.shape[0]
    v_pix = meshraster.transform(verts.expand(B, -1, -1), K, Rt)
    return meshraster.rasterize(v_pix, vi, H, W, with_bary=False)[0]


class TexMean:
    """The accumulators of run_gen_texmean.py:83-105: `.add(...)` per batch of cameras, `.mean(...)` at the end.

        tm = TexMean(ViewTexTopology(index_image, bary_image, face_index), n_faces=vi.shape[0], device="cuda")
        tm.add(mesh_world, images, K, Rt, vi=vi)        # all cameras of a frame in one call
        tex_mean = tm.mean(flip_rows=True, bgr=True)    # [S,S,3], what the script hands to cv2.imwrite
    """

    def __init__(self, topology, n_faces, device=None):
        if not isinstance(topology, ViewTexTopology):
            raise TypeError("topology must be a ViewTexTopology")
        device = topology.device if device is None else torch.device(device)
        if device.type != "cuda":
            raise _lib.GoliathHipError("TexMean needs a CUDA(HIP) device; there is no CPU path")
        if device.index is not None and device.index != topology.device.index:
            raise ValueError("the topology lives on another device")
        self.topology = topology
        self.n_faces = int(n_faces)
        self.total = torch.zeros(3, topology.S_h, topology.S_w, dtype=_F32, device=topology.device)
        self.count = torch.zeros(topology.S_h, topology.S_w, dtype=_F32, device=topology.device)

    def reset(self):
        self.total.zero_()
        self.count.zero_()

    def add(self, verts, image, K, Rt, index_img=None, vi=None, intensity_threshold=None):
        """verts[B,V,3] or [1,V,3] (one posed mesh seen by B cameras), image[B,3,H,W] float32, K[B,3,3], Rt[B,3,4].
        index_img[B,H,W]: the cameras' face index images; None = rasterise them here from `vi`[F,3] (meshraster).
        total += sum_b tex_b and count += sum_b mask_b in view order, without writing a [B,3,S,S] tensor."""
        verts, image, K, Rt = _views("TexMean.add", verts, image, K, Rt)
        B, _, H, W = image.shape
        if index_img is None:
            if vi is None:
                raise ValueError("TexMean.add needs index_img, or vi to rasterise it")
            index_img = _rasterized_index(verts, vi, K, Rt, H, W)
        index_img = _index_img("TexMean.add", index_img)
        if tuple(index_img.shape) != (B, H, W):
            raise ValueError(f"index_img must be [B,H,W] of image, got {tuple(index_img.shape)}")
        with _lib.device_guard(image.device):
            face_vis = _face_vis(index_img, self.n_faces)
            _launch(self.topology, self.n_faces, verts, image, K, Rt, face_vis, intensity_threshold, total=self.total,
                    cnt=self.count)
        return self

    def mean(self, eps=1e-5, flip_rows=False, bgr=False):
        """total / (count + eps) as [S_h,S_w,3] (run_gen_texmean.py:105-106); flip_rows and bgr: the script's th.flip and
        its channel swap for cv2.imwrite (:106-108)."""
        t = self.topology
        out = torch.empty(t.S_h, t.S_w, 3, dtype=_F32, device=self.total.device)
        with _lib.device_guard(self.total.device):
            _abi_texmean_finalize(S_h=t.S_h, S_w=t.S_w, total=self.total, cnt=self.count, eps=float(eps),
                                  flip_rows=int(bool(flip_rows)), bgr=int(bool(bgr)), out=out)
        return out


def get_tex_rl(rl, image, ply, extrin, intrin, face_index, index_image, bary_image):
    """ca_code/utils/tex.py:21-63 for any B: image[B,3,H,W], ply = (verts[B or 1,V,3], faces[F,3]), extrin[B,3,4],
    intrin[B,3,3], face_index[S,S], index_image[S,S,3], bary_image[S,S,3] -> (tex[B,3,S,S], mask[B,1,S,S]).  The camera's
    face index image comes from rl(...)["index_img"] when a render layer is given -- it has to be handed some texture: an
    8x8 one, not the reference's zero 1024^2 dummy --, otherwise from meshraster with no texture work at all."""
    geom, faces = ply
    _need_gpu("get_tex_rl", geom, image, extrin, intrin, face_index, index_image, bary_image)
    B, _, H, W = image.shape
    if rl is not None:
        tex_tmp = torch.zeros(B, 3, 8, 8, dtype=geom.dtype, device=geom.device)
        index_img = rl(geom.expand(B, -1, -1), tex_tmp, K=intrin, Rt=extrin)["index_img"]
    else:
        index_img = _rasterized_index(geom.detach().float(), faces, intrin.float(), extrin.float()[:, :3], H, W)
    return compute_view_texture(geom, faces, image, index_img, None, intrin, extrin, index_image, bary_image, face_index,
                                intensity_threshold=None, normal_threshold=0.1)
