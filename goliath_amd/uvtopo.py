"""The constant UV topology images of a mesh on the HIP kernels of csrc/uvtopo.hip: what `GeometryModule.__init__`
(ca_code/utils/geom.py:197-249) gets from pytorch3d's CUDA `rasterize_meshes` and a scikit-learn KD-tree.

    uv_face_index(vt, vti, uv_shape, flip_uv=True)          make_uv_face_index (geom.py:31-66), after its `1 - vt`
    index_images(vi, vt, vti, uv_size, flip_uv=False,       the four buffers the constructor registers (geom.py:225-249)
                 impaint=False, impaint_threshold=100.0)
    impaint(index_image, bary_image=None,                   index_image_impaint (geom.py:145-194)
            distance_threshold=100.0)
    nearest_valid(valid, distance_threshold)                its source map alone: int32 [H,W] linear texel ids, -1 = none
    uv_topology(vi, vt, vti, uv_size, ...)                  index_images handed straight to uvgeom.UVTopology

PINNED by the reference's own code (tests/test_uvtopo_cpu.py runs it): texel (r, c) is sampled at
uv = ((c + 0.5) / W, (r + 0.5) / H), v mirrored first when flip_uv -- the grid make_uv_barys evaluates on, so the face
stored at a texel has to contain that point; the barycentrics are bary_coords' fp32 arithmetic; the impaint takes the
nearest valid texel by Euclidean distance over integer (row, col), strictly nearer than the threshold, and `valid_mask`
is taken before it.  STATED (pytorch3d is third-party and absent from the reference tree; believed strict-interior with
the lowest face index winning, not verifiable here): a texel centre exactly on an edge IS covered (gol_mesh_raster's
`>= 0` on un-normalised anchored edge functions, either winding), zero-area faces are skipped, the lowest face index wins
where faces overlap (gol_mesh_raster_flat: the rasteriser's kernel without its depth test -- all UV faces lie at z = 1), and among equidistant impaint sources the lexicographically smallest (row, col) is taken (the
KD-tree's choice is unspecified).  One source map serves the three images; the reference queries the tree twice.

Every tensor must be on the GPU: there is no CPU path.  Nothing here syncs the host.
"""
import collections
import ctypes
import math

import torch

from . import _lib
from ._lib import c_i64, c_int, stream_ptr

_F32, _I32, _I64 = torch.float32, torch.int32, torch.int64

IndexImages = collections.namedtuple("IndexImages", ["index_image", "bary_image", "face_index_image", "valid_mask"])


# ---- one marshaller per C-ABI entry: keywords = the header's parameter names; a pointer is a GPU tensor (checked), a
# device address or None; stream = the current one ------------------------------------------------------------------------
def _p(x, dtype=_F32, name="tensor"):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else _lib.ptr(x, dtype, name)


def _abi_uv_face_index(*, Vt, F, H, W, flip_uv, vt, vti, face_img, workspace):
    _lib.call("gol_uv_face_index", c_int(Vt), c_int(F), c_int(H), c_int(W), c_int(flip_uv), _p(vt), _p(vti, _I32),
              _p(face_img, _I32), _p(workspace, torch.uint8), stream_ptr())


def _abi_uv_topology(*, F, Vt, H, W, flip_uv, face_img, vi, vti, vt, index_image, face_index_image, bary_image,
                     valid_mask):
    _lib.call("gol_uv_topology", c_int(F), c_int(Vt), c_int(H), c_int(W), c_int(flip_uv), _p(face_img, _I32),
              _p(vi, _I32), _p(vti, _I32), _p(vt), _p(index_image, _I64), _p(face_index_image, _I64), _p(bary_image),
              _p(valid_mask, torch.bool), stream_ptr())


def _abi_nearest_valid(*, H, W, max_d2, valid, col_near, src):
    _lib.call("gol_nearest_valid", c_int(H), c_int(W), c_i64(max_d2), _p(valid, torch.bool), _p(col_near, _I32),
              _p(src, _I32), stream_ptr())


def _abi_impaint_gather(*, P, src, w0=0, in0=None, out0=None, w1=0, in1=None, out1=None, w2=0, in2=None, out2=None):
    _lib.call("gol_impaint_gather", c_i64(P), _p(src, _I32), c_int(w0), _p(in0, None), _p(out0, None), c_int(w1),
              _p(in1, None), _p(out1, None), c_int(w2), _p(in2, None), _p(out2, None), stream_ptr())


def _need_gpu(name, *tensors):
    for t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.GoliathHipError(f"{name} needs CUDA(HIP) tensors; there is no CPU path")


def _shape2(uv_shape):
    H, W = (uv_shape, uv_shape) if isinstance(uv_shape, int) else uv_shape
    return int(H), int(W)


def max_d2_of(distance_threshold, H, W):
    """The largest integer d2 with sqrt(d2) < distance_threshold -- the reference's `dists < distance_threshold` on the
    KD-tree's float64 distances (geom.py:172), as an integer bound on the squared distance; -1 = nothing is accepted.
    Capped at the image's squared diagonal."""
    t = float(distance_threshold)
    cap = (H - 1) ** 2 + (W - 1) ** 2
    if not t > 0.0:          # (NaN compares false with everything: nothing accepted, as in the reference)
        return -1
    if math.isinf(t) or t * t > cap + 1:
        return cap
    k = min(int(t * t), cap)
    while k < cap and math.sqrt(k + 1) < t:
        k += 1
    while k >= 0 and not math.sqrt(k) < t:
        k -= 1
    return k


def _face_image(vt32, vti32, H, W, flip_uv):
    dev = vt32.device
    face = torch.empty(H, W, dtype=_I32, device=dev)
    fn = _lib.load().gol_uv_face_index_workspace_bytes
    fn.restype = ctypes.c_int64
    ws = torch.empty(max(int(fn(c_int(vt32.shape[0]), c_int(vti32.shape[0]), c_int(H), c_int(W))), 16),
                     dtype=torch.uint8, device=dev)
    _abi_uv_face_index(Vt=vt32.shape[0], F=vti32.shape[0], H=H, W=W, flip_uv=int(bool(flip_uv)), vt=vt32, vti=vti32,
                       face_img=face, workspace=ws)
    return face


def _mesh(name, vt, vti, vi=None):
    _need_gpu(name, vt)
    if vt.dim() != 2 or vt.shape[1] != 2:
        raise ValueError(f"vt must be [Vt,2], got {tuple(vt.shape)}")
    if vti.dim() != 2 or vti.shape[1] != 3:
        raise ValueError(f"vti must be [F,3], got {tuple(vti.shape)}")
    dev = vt.device
    vt32 = vt.detach().to(_F32).contiguous()
    vti32 = vti.to(device=dev, dtype=_I32).contiguous()
    if vi is None:
        return vt32, vti32
    if tuple(vi.shape) != tuple(vti.shape):
        raise ValueError("vi must have vti's shape")
    return vt32, vti32, vi.to(device=dev, dtype=_I32).contiguous()


def uv_face_index(vt, vti, uv_shape, flip_uv=True, device=None):
    """make_uv_face_index (geom.py:31-66): int64 [H,W], the UV triangle that holds texel (r, c)'s sample
    uv = ((c + 0.5) / W, (r + 0.5) / H) -- in the uv with v mirrored when flip_uv --, -1 where none."""
    if device is not None:   # (the reference moves vt to `device`, default "cuda": geom.py:44-58)
        vt = vt.to(device)
    vt32, vti32 = _mesh("uv_face_index", vt, vti)
    H, W = _shape2(uv_shape)
    with _lib.device_guard(vt32.device):
        return _face_image(vt32, vti32, H, W, flip_uv).long()


def nearest_valid(valid, distance_threshold=100.0):
    """valid[H,W] bool -> int32 [H,W]: for every texel that is not valid the linear id (row * W + col) of the nearest valid
    texel -- squared Euclidean distance over integer (row, col), ties to the lexicographically smallest (row, col) --
    if it is strictly nearer than distance_threshold; -1 otherwise and on valid texels."""
    _need_gpu("nearest_valid", valid)
    if valid.dim() != 2:
        raise ValueError(f"valid must be [H,W], got {tuple(valid.shape)}")
    valid = valid.to(torch.bool).contiguous()
    H, W = valid.shape
    src = torch.empty(H, W, dtype=_I32, device=valid.device)
    col_near = torch.empty(H, W, dtype=_I32, device=valid.device)
    with _lib.device_guard(valid.device):
        _abi_nearest_valid(H=H, W=W, max_d2=max_d2_of(distance_threshold, H, W), valid=valid, col_near=col_near, src=src)
    return src


def _words(t):
    """(words per texel, contiguous tensor) of an [H,W] or [H,W,C] image with 4- or 8-byte elements."""
    t = t.contiguous()
    if t.element_size() not in (4, 8):
        raise ValueError(f"impaint: unsupported dtype {t.dtype}")
    per = 1 if t.dim() == 2 else int(t.shape[2])
    return per * t.element_size() // 4, t


def _gather(src, images):
    """images: up to three [H,W(,C)] tensors -> their impainted copies, one launch."""
    outs, kw = [], {}
    for k, img in enumerate(images):
        w, img = _words(img)
        out = torch.empty_like(img)
        outs.append(out)
        kw.update({f"w{k}": w, f"in{k}": img, f"out{k}": out})
    _abi_impaint_gather(P=src.numel(), src=src, **kw)
    return outs


def impaint(index_image, bary_image=None, distance_threshold=100.0, device=None):
    """index_image_impaint (geom.py:145-194): index_image [H,W] or [H,W,C] (a texel is valid when any of its entries is not
    -1, geom.py:151-154); every other texel takes the entries -- and bary_image's, when given -- of the nearest valid
    texel strictly nearer than distance_threshold.  Returns the impainted index image, or the pair with bary_image.
    device: a GPU to compute on when the images live elsewhere (GeometryModule.__init__ passes CPU buffers); the results
    come back on the images' own devices, as the reference returns them."""
    if device is not None:
        home = (index_image.device, None if bary_image is None else bary_image.device)
        out = impaint(index_image.to(device), None if bary_image is None else bary_image.to(device), distance_threshold)
        return out.to(home[0]) if bary_image is None else (out[0].to(home[0]), out[1].to(home[1]))
    _need_gpu("impaint", index_image, bary_image)
    if index_image.dim() == 3:
        valid = (index_image != -1).any(dim=-1)
    elif index_image.dim() == 2:
        valid = index_image != -1
    else:
        raise ValueError("`index_image` should be a [H,W] or [H,W,C] image")
    if bary_image is not None and tuple(bary_image.shape[:2]) != tuple(index_image.shape[:2]):
        raise ValueError("bary_image must have index_image's height and width")
    with _lib.device_guard(index_image.device):
        src = nearest_valid(valid, distance_threshold)
        outs = _gather(src, [index_image] if bary_image is None else [index_image, bary_image])
    return outs[0] if bary_image is None else (outs[0], outs[1])


def index_images(vi, vt, vti, uv_size, flip_uv=False, impaint=False, impaint_threshold=100.0):
    """The buffers GeometryModule.__init__ registers (geom.py:225-249), as device tensors:
    index_image[S,S,3] int64 (-1 = empty), bary_image[S,S,3] float32 (0 = empty), face_index_image[S,S] int64,
    valid_mask[S,S,1] bool -- the latter taken BEFORE the impaint, as the reference does."""
    vt32, vti32, vi32 = _mesh("index_images", vt, vti, vi)
    S = int(uv_size)
    dev = vt32.device
    index_image = torch.empty(S, S, 3, dtype=_I64, device=dev)
    face_index_image = torch.empty(S, S, dtype=_I64, device=dev)
    bary_image = torch.empty(S, S, 3, dtype=_F32, device=dev)
    valid_mask = torch.empty(S, S, 1, dtype=torch.bool, device=dev)
    with _lib.device_guard(dev):
        face = _face_image(vt32, vti32, S, S, flip_uv)
        _abi_uv_topology(F=vti32.shape[0], Vt=vt32.shape[0], H=S, W=S, flip_uv=int(bool(flip_uv)), face_img=face, vi=vi32,
                         vti=vti32, vt=vt32, index_image=index_image, face_index_image=face_index_image,
                         bary_image=bary_image, valid_mask=valid_mask)
        if impaint:
            # (the reference's validity, (index_image != -1).any(-1), of a freshly built image is the coverage itself)
            src = nearest_valid(valid_mask[..., 0], impaint_threshold)
            index_image, bary_image, face_index_image = _gather(src, [index_image, bary_image, face_index_image])
    return IndexImages(index_image, bary_image, face_index_image, valid_mask)


def uv_topology(vi, vt, vti, uv_size, flip_uv=False, impaint=False, impaint_threshold=100.0, n_verts=None):
    """index_images(...) packed for the uvgeom kernels: a uvgeom.UVTopology (its constructor is the one place that syncs)."""
    from . import uvgeom

    img = index_images(vi, vt, vti, uv_size, flip_uv=flip_uv, impaint=impaint, impaint_threshold=impaint_threshold)
    return uvgeom.UVTopology(vi.to(img.index_image.device), img.index_image, img.bary_image, n_verts=n_verts)
