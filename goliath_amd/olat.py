"""The MVP teacher's per-light work around its UNet on the HIP kernels of csrc/olat.hip.

    features(primpos, primrot, primscale, valid_prims, light_pos, campos, shadow, primsize, n_prim_x, n_prim_y, volradius) -> x
    combine(tex, light_intensity, shadow, primsize, n_prim_x, n_prim_y, use_shadow, want_texolat) -> rgb, texolat | None, primshadow

replace, in OLATRGBDecoder.forward_rgb, ca_code/models/hand_teacher_mvp.py:371-439 (the UNet input: light and view directions
in the primitives' frames, the valid_prims mask, the UV layout, the cat with 1 - shadow) and :468-488 (sigmoid, 25 t + 100,
relu, the intensity product, the sum over the lights and primshadow).  The numerics are stated in include/goliath_hip.h.
One launch each (and one for the backward of `combine`) on the current stream, no host sync, no atomics, bitwise
reproducible.  Every tensor must be on the GPU, float32 and contiguous: there is no CPU path.
"""
import torch

from . import _lib
from ._lib import c_float, c_int, stream_ptr

_F32 = torch.float32
_LINSPACE = {}


def _linspace(n, device):
    """torch.linspace(-1, 1, n) on `device`, made once: the rounding of the voxel coordinates is torch's own."""
    key = (int(n), device)
    t = _LINSPACE.get(key)
    if t is None:
        t = _LINSPACE[key] = torch.linspace(-1.0, 1.0, int(n), device=device)
    return t


def _check(t, name, shape):
    """`t` after the host-side checks every entry makes first: shape, float32, contiguous.  That it is on the GPU is
    `_lib.ptr`'s to say, when the pointer is taken."""
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        got = list(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise _lib.GoliathHipError(f"{name} must be {list(shape)}, got {got}")
    if t.dtype != _F32:
        raise _lib.GoliathHipError(f"{name} must have dtype {_F32}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.GoliathHipError(f"{name} must be contiguous")
    return t


def _geometry(primsize, n_prim_x, n_prim_y):
    X, Y, Z = (int(v) for v in primsize)
    npx, npy = int(n_prim_x), int(n_prim_y)
    if min(X, Y, Z, npx, npy) < 1:
        raise _lib.GoliathHipError(f"primsize {tuple(primsize)} and the primitive grid {npy} x {npx} must be positive")
    return X, Y, Z, npx, npy


def _shadow_arg(shadow, BL, K, Z, Y, X):
    if torch.is_tensor(shadow) and shadow.dim() == 6 and shadow.shape[-1] == 1:
        shadow = shadow[..., 0]                      # mvp.shadow_march's trailing 1: a view, no copy
    return _check(shadow, "shadow", (BL, K, Z, Y, X))


# ---- one marshaller per C-ABI entry: keywords = the header's parameter names ----------------------------------------------
def _abi_olat_features_fwd(*, B, L, X, Y, Z, npx, npy, primpos, primrot, primscale, valid_prims, light_pos, campos, shadow,
                           volradius, lin_x, lin_y, lin_z, x):
    _lib.call("gol_olat_features_fwd", c_int(B), c_int(L), c_int(X), c_int(Y), c_int(Z), c_int(npx), c_int(npy), primpos,
              primrot, primscale, valid_prims, light_pos, campos, shadow, c_float(volradius), lin_x, lin_y, lin_z, x,
              stream_ptr())


def _abi_olat_combine_fwd(*, B, L, X, Y, Z, npx, npy, use_shadow, tex, light_intensity, shadow, rgb, texolat, primshadow):
    _lib.call("gol_olat_combine_fwd", c_int(B), c_int(L), c_int(X), c_int(Y), c_int(Z), c_int(npx), c_int(npy),
              c_int(use_shadow), tex, light_intensity, shadow, rgb, texolat, primshadow, stream_ptr())


def _abi_olat_combine_bwd(*, B, L, X, Y, Z, npx, npy, use_shadow, tex, light_intensity, shadow, g_rgb, g_texolat, g_tex):
    _lib.call("gol_olat_combine_bwd", c_int(B), c_int(L), c_int(X), c_int(Y), c_int(Z), c_int(npx), c_int(npy),
              c_int(use_shadow), tex, light_intensity, shadow, g_rgb, g_texolat, g_tex, stream_ptr())


def features(primpos, primrot, primscale, valid_prims, light_pos, campos, shadow, primsize, n_prim_x, n_prim_y, volradius):
    """The UNet input x[B L, 7 Z, n_prim_y Y, n_prim_x X]: light directions, view directions, 1 - shadow.

    primpos[B,K,3], primrot[B,K,3,3], primscale[B,K,3], valid_prims[K] (a float 0 / 1 mask), light_pos[B,L,3], campos[B,3],
    shadow[B L,K,Z,Y,X] (or with the trailing 1 `mvp.shadow_march` returns), primsize = (X, Y, Z), K = n_prim_y n_prim_x.
    The returned tensor does NOT require grad, in training either.  The reference marks its three pieces
    `requires_grad = True` there (hand_teacher_mvp.py:434-437), but they are local leaves of forward_rgb whose `.grad` nobody
    can read; leaving that out changes no gradient a caller sees and spares the first convolution its input-gradient."""
    X, Y, Z, npx, npy = _geometry(primsize, n_prim_x, n_prim_y)
    K = npx * npy
    if not torch.is_tensor(light_pos) or light_pos.dim() != 3:
        raise _lib.GoliathHipError("light_pos must be [B, L, 3]")
    B, L = int(light_pos.shape[0]), int(light_pos.shape[1])
    if L < 1:
        raise _lib.GoliathHipError("light_pos must hold at least one light")
    named = dict(shadow=_shadow_arg(shadow, B * L, K, Z, Y, X), primpos=_check(primpos, "primpos", (B, K, 3)),
                 primrot=_check(primrot, "primrot", (B, K, 3, 3)), primscale=_check(primscale, "primscale", (B, K, 3)),
                 valid_prims=_check(valid_prims, "valid_prims", (K,)), light_pos=_check(light_pos, "light_pos", (B, L, 3)),
                 campos=_check(campos, "campos", (B, 3)))
    args = {name: _lib.fptr(t, name) for name, t in named.items()}
    dev = named["shadow"].device
    for name, t in named.items():
        if t.device != dev:
            raise _lib.GoliathHipError(f"{name} is on {t.device}, shadow on {dev}")
    x = torch.empty(B * L, 7 * Z, npy * Y, npx * X, device=dev, dtype=_F32)
    with _lib.device_guard(dev):
        lin = [_linspace(n, dev) for n in (X, Y, Z)]
        _abi_olat_features_fwd(B=B, L=L, X=X, Y=Y, Z=Z, npx=npx, npy=npy, volradius=float(volradius),
                               lin_x=_lib.fptr(lin[0], "lin_x"), lin_y=_lib.fptr(lin[1], "lin_y"),
                               lin_z=_lib.fptr(lin[2], "lin_z"), x=_lib.fptr(x, "x"), **args)
    return x


class _Combine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, light_intensity, shadow, geom, use_shadow, want_texolat):
        X, Y, Z, npx, npy = geom
        B, L = light_intensity.shape[:2]
        Sy, Sx = npy * Y, npx * X
        t = tex.detach()
        rgb = torch.empty(B, Z, 3, Sy, Sx, device=t.device, dtype=_F32)
        primshadow = torch.empty_like(rgb)
        texolat = torch.empty(B, L, Z, 3, Sy, Sx, device=t.device, dtype=_F32) if want_texolat else None
        with _lib.device_guard(t.device):
            _abi_olat_combine_fwd(B=B, L=L, X=X, Y=Y, Z=Z, npx=npx, npy=npy, use_shadow=int(use_shadow),
                                  tex=_lib.fptr(t, "tex"), light_intensity=_lib.fptr(light_intensity, "light_intensity"),
                                  shadow=_lib.fptr(shadow, "shadow"), rgb=_lib.fptr(rgb, "rgb"),
                                  texolat=_lib.fptr(texolat, "texolat"), primshadow=_lib.fptr(primshadow, "primshadow"))
        ctx.save_for_backward(t, light_intensity, shadow)     # nothing but the inputs: the backward recomputes from tex
        ctx.geom, ctx.use_shadow = geom, int(use_shadow)
        ctx.mark_non_differentiable(primshadow)
        ctx.set_materialize_grads(False)                      # an unused texolat costs no zero-filled gradient
        if texolat is None:
            return rgb, primshadow
        return rgb, texolat, primshadow

    @staticmethod
    def backward(ctx, g_rgb, *rest):
        t, light_intensity, shadow = ctx.saved_tensors
        X, Y, Z, npx, npy = ctx.geom
        B, L = light_intensity.shape[:2]
        g_texolat = rest[0] if len(rest) == 2 else None
        g_rgb = torch.zeros(B, Z, 3, npy * Y, npx * X, device=t.device) if g_rgb is None else g_rgb.to(_F32).contiguous()
        if g_texolat is not None:
            g_texolat = g_texolat.to(_F32).contiguous()
        g_tex = torch.empty_like(t)
        with _lib.device_guard(t.device):
            _abi_olat_combine_bwd(B=B, L=L, X=X, Y=Y, Z=Z, npx=npx, npy=npy, use_shadow=ctx.use_shadow,
                                  tex=_lib.fptr(t, "tex"), light_intensity=_lib.fptr(light_intensity, "light_intensity"),
                                  shadow=_lib.fptr(shadow, "shadow"), g_rgb=_lib.fptr(g_rgb, "g_rgb"),
                                  g_texolat=_lib.fptr(g_texolat, "g_texolat"), g_tex=_lib.fptr(g_tex, "g_tex"))
        return g_tex, None, None, None, None, None


def combine(tex, light_intensity, shadow, primsize, n_prim_x, n_prim_y, use_shadow, want_texolat):
    """tex[B L, 4 Z, S_y, S_x] -> (rgb[B,Z,3,S_y,S_x], texolat[B,L,Z,3,S_y,S_x] or None, primshadow[B,Z,3,S_y,S_x]).

    light_intensity[B,L,3] or [B,L,1] (expanded); shadow as for `features`; use_shadow: the deep shadow itself instead of
    sigmoid(tex_0) (the reference's warm-up branch, iteration < 1000 in training).  Differentiable with respect to `tex`
    only; primshadow is marked non-differentiable, texolat is formed only with want_texolat (training)."""
    X, Y, Z, npx, npy = _geometry(primsize, n_prim_x, n_prim_y)
    K = npx * npy
    if not torch.is_tensor(light_intensity) or light_intensity.dim() != 3 or light_intensity.shape[2] not in (1, 3):
        raise _lib.GoliathHipError("light_intensity must be [B, L, 3] or [B, L, 1]")
    B, L = int(light_intensity.shape[0]), int(light_intensity.shape[1])
    if L < 1:
        raise _lib.GoliathHipError("light_intensity must hold at least one light")
    if torch.is_tensor(tex) and tex.dim() == 4 and tuple(tex.shape[2:]) != (npy * Y, npx * X):
        raise _lib.GoliathHipError(f"tex is {tex.shape[2]} x {tex.shape[3]}, but {npy} x {npx} primitives of {Y} x {X} texels "
                                   f"make a {npy * Y} x {npx * X} map (uv_size)")
    _check(tex, "tex", (B * L, 4 * Z, npy * Y, npx * X))
    shadow = _shadow_arg(shadow, B * L, K, Z, Y, X)
    if light_intensity.shape[2] == 1:
        light_intensity = light_intensity.expand(-1, -1, 3)
    light_intensity = _check(light_intensity.detach().contiguous(), "light_intensity", (B, L, 3))
    for name, t in (("tex", tex), ("light_intensity", light_intensity), ("shadow", shadow)):
        _lib.fptr(t, name)                           # on the GPU, by name, before autograd wraps the call
    for name, t in (("light_intensity", light_intensity), ("shadow", shadow)):
        if t.device != tex.device:
            raise _lib.GoliathHipError(f"{name} is on {t.device}, tex on {tex.device}")
    out = _Combine.apply(tex, light_intensity, shadow.detach(), (X, Y, Z, npx, npy), bool(use_shadow), bool(want_texolat))
    if want_texolat:
        return out
    return out[0], None, out[1]
