"""The last layer of the MVP hand model's two decoders written straight into the primitive template (csrc/mvptail.hip).

Both decoders of `ca_code/models/hand_mvp.py` end in `ConvTranspose2dWNUB(16, TD * C, 4, 2, 1)` at 512^2 -> 1024^2 with an
untied bias (:338-340, :384, :455); the colours then take `relu(25 x + 100)` (:472), alpha `relu` (:434), and `render`
rearranges the two slabs into the channels-last template (:172-185) of which the march keeps `template[:, valid_prims]`
(ca_code/utils/render_raymarcher.py:41-47).  The slabs exist only to be re-read; here they are never written.

  decode_template(x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, primsize, valid_prims=None, compact=True,
                  rgb_affine=(25.0, 100.0))
      the 16-channel activations of the two decoders -> the template, forward and backward (an autograd Function on
      gol_mvp_tail_fwd / _bwd); x_rgb=None gives the one-channel (alpha only) template
  decode_template_torch(...)
      the same composition in plain PyTorch, in the reference's order of operations: parity twin, runs on the CPU
  TailHandle, tail_handle(decoder, x, TD, C), rgb_decoder_forward
      the model binding of dropin.patch_hand_mvp(fused_tail=True): a decoder stops in front of its last layer and hands
      over (activation, layer); goliath_amd.mvpprims.hand_mvp_render gives two such handles to decode_template

The weight norm stays torch algebra on the small tensor (`tail.wn_weight`), so gradients reach weight_v / weight_g through
the ordinary graph and the kernels see the effective weight.  Everything runs on the current stream; there is no CPU path.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_float, c_int, fptr, iptr, stream_ptr
from .mvpprims import _aligned16, _f32c, _need_gpu, prim_slots
from .tail import wn_weight

FUSED_TAIL_FLAG = "_goliath_fused_tail"   # set on the decoder classes by dropin.patch_hand_mvp(fused_tail=True)
MAX_TD = 10                               # 3 TD <= 32: two row tiles of colour (the limit csrc/tail.hip has)


# ------------------------------------------------------------------------------------------------------- ABI marshallers
def _abi_mvp_tail_fwd(*, B, Ci, h, w, TD, TH, TW, ny, nx, x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, slot, live,
                      Kout, rgb_scale, rgb_shift, out):
    _lib.call("gol_mvp_tail_fwd", c_int(B), c_int(Ci), c_int(h), c_int(w), c_int(TD), c_int(TH), c_int(TW), c_int(ny),
              c_int(nx), fptr(x_rgb), fptr(w_rgb), fptr(bias_rgb), fptr(x_alpha), fptr(w_alpha), fptr(bias_alpha),
              iptr(slot), iptr(live), c_int(Kout), c_float(rgb_scale), c_float(rgb_shift), fptr(out), stream_ptr())


def _abi_mvp_tail_bwd(*, B, Ci, h, w, TD, TH, TW, ny, nx, C, x_rgb, w_rgb_t, x_alpha, w_alpha_t, slot, live, Kout, rgb_scale,
                      g_out, out, g_x_rgb, g_x_alpha, g_w_rgb, g_w_alpha, g_bias_rgb, g_bias_alpha, scratch):
    _lib.call("gol_mvp_tail_bwd", c_int(B), c_int(Ci), c_int(h), c_int(w), c_int(TD), c_int(TH), c_int(TW), c_int(ny),
              c_int(nx), c_int(C), fptr(x_rgb), fptr(w_rgb_t), fptr(x_alpha), fptr(w_alpha_t), iptr(slot), iptr(live),
              c_int(Kout), c_float(rgb_scale), fptr(g_out), fptr(out), fptr(g_x_rgb), fptr(g_x_alpha), fptr(g_w_rgb),
              fptr(g_w_alpha), fptr(g_bias_rgb), fptr(g_bias_alpha), fptr(scratch), stream_ptr())


def _scratch_floats(B, h, w, TD, C):
    fn = _lib.load().gol_mvp_tail_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    return int(fn(c_int(B), c_int(h), c_int(w), c_int(TD), c_int(C)))


# -------------------------------------------------------------------------------------------------------------- operator
def _geometry(x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, primsize):
    TW, TH, TD = (int(v) for v in primsize)      # the reference's primsize is (x, y, z)
    if min(TW, TH, TD) < 1:
        raise ValueError("primsize must be positive")
    if TD > MAX_TD:
        raise ValueError(f"decode_template supports 1 <= TD <= {MAX_TD}, got {TD}")
    if not torch.is_tensor(x_alpha) or x_alpha.dim() != 4:
        raise ValueError("x_alpha must be [B,16,h,w]")
    B, Ci, h, w = x_alpha.shape
    if Ci != 16:
        raise ValueError(f"the last decoder layers have 16 input channels, got {Ci}")
    Sy, Sx = 2 * h, 2 * w
    if Sy % TH or Sx % TW:
        raise ValueError(f"the [{Sy},{Sx}] output does not tile into primitives of size {(TW, TH, TD)}")
    branches = [("alpha", x_alpha, w_alpha, bias_alpha, TD)]
    if x_rgb is not None:
        branches.append(("rgb", x_rgb, w_rgb, bias_rgb, 3 * TD))
    elif w_rgb is not None or bias_rgb is not None:
        raise ValueError("w_rgb / bias_rgb without x_rgb")
    for name, x, wt, bias, CH in branches:
        if not all(torch.is_tensor(t) for t in (x, wt, bias)):
            raise ValueError(f"x_{name}, w_{name} and bias_{name} must be tensors")
        if tuple(x.shape) != (B, 16, h, w):
            raise ValueError(f"x_{name} must be {(B, 16, h, w)}, got {tuple(x.shape)}")
        if tuple(wt.shape) != (16, CH, 4, 4):
            raise ValueError(f"w_{name} must be {(16, CH, 4, 4)} (ConvTranspose2d layout), got {tuple(wt.shape)}")
        if tuple(bias.shape) != (CH, Sy, Sx):
            raise ValueError(f"bias_{name} must be {(CH, Sy, Sx)}, got {tuple(bias.shape)}")
        if not (x.dtype.is_floating_point and wt.dtype.is_floating_point and bias.dtype.is_floating_point):
            raise ValueError("the operands must be floating point")
    return B, h, w, TD, TH, TW, Sy // TH, Sx // TW


class _DecodeTemplate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, geom, slot, live, Kout, affine):
        B, h, w, TD, TH, TW, ny, nx = geom
        has_rgb = x_rgb is not None
        C = 4 if has_rgb else 1
        xr, wr, br = (_f32c(t.detach()) for t in (x_rgb, w_rgb, bias_rgb)) if has_rgb else (None, None, None)
        xa, wa, ba = (_f32c(t.detach()) for t in (x_alpha, w_alpha, bias_alpha))
        dev = xa.device
        shape = (TD, TH, TW, 4) if has_rgb else (TD, TH, TW)
        out = torch.empty((B, Kout, *shape), dtype=torch.float32, device=dev)
        ctx.dims = dict(B=B, Ci=16, h=h, w=w, TD=TD, TH=TH, TW=TW, ny=ny, nx=nx, slot=slot, live=live, Kout=Kout,
                        rgb_scale=float(affine[0]))
        ctx.C, ctx.dtypes = C, tuple(None if t is None else t.dtype for t in (x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha))
        if B and Kout:
            with _lib.device_guard(dev):
                _abi_mvp_tail_fwd(x_rgb=xr, w_rgb=wr, bias_rgb=br, x_alpha=xa, w_alpha=wa, bias_alpha=ba,
                                  rgb_shift=float(affine[1]), out=out, **ctx.dims)
        ctx.save_for_backward(*((xr, wr, xa, wa, out) if has_rgb else (xa, wa, out)))
        return out.to(x_alpha.dtype)

    @staticmethod
    def backward(ctx, g_out):
        d, C = ctx.dims, ctx.C
        if C == 4:
            xr, wr, xa, wa, out = ctx.saved_tensors
        else:
            (xa, wa, out), xr, wr = ctx.saved_tensors, None, None
        B, h, w, TD = d["B"], d["h"], d["w"], d["TD"]
        dev = xa.device
        need = list(ctx.needs_input_grad[:6])
        if C == 1:
            need[0] = need[1] = need[2] = False
        new = lambda flag, *shape: torch.empty(shape, dtype=torch.float32, device=dev) if flag else None
        g = dict(g_x_rgb=new(need[0], B, 16, h, w), g_w_rgb=new(need[1], 16, 3 * TD, 4, 4),
                 g_bias_rgb=new(need[2], 3 * TD, 2 * h, 2 * w), g_x_alpha=new(need[3], B, 16, h, w),
                 g_w_alpha=new(need[4], 16, TD, 4, 4), g_bias_alpha=new(need[5], TD, 2 * h, 2 * w))
        if B == 0 or d["Kout"] == 0 or g_out is None:     # nothing came back (Kv = 0): zeros without a launch
            for t in g.values():
                if t is not None:
                    t.zero_()
        elif any(need):
            g_out = _aligned16(_f32c(g_out))
            slabs = need[0] or need[1] or need[3] or need[4]
            scratch = torch.empty(_scratch_floats(B, h, w, TD, C), dtype=torch.float32, device=dev) if slabs else None
            # the weights with the input channel last: [CH,4,4,16]
            wrt = wr.permute(1, 2, 3, 0).contiguous() if need[0] else None
            wat = wa.permute(1, 2, 3, 0).contiguous() if need[3] else None
            with _lib.device_guard(dev):
                _abi_mvp_tail_bwd(C=C, x_rgb=xr, w_rgb_t=wrt, x_alpha=xa, w_alpha_t=wat, g_out=g_out, out=out,
                                  scratch=scratch, **d, **g)
        order = ("g_x_rgb", "g_w_rgb", "g_bias_rgb", "g_x_alpha", "g_w_alpha", "g_bias_alpha")
        grads = [None if g[k] is None else g[k].to(dt) for k, dt in zip(order, ctx.dtypes)]
        return (*grads, None, None, None, None, None)


def _check_mask(valid_prims, K):
    if valid_prims is not None:
        if not torch.is_tensor(valid_prims) or valid_prims.dim() != 1 or valid_prims.numel() != K:
            raise ValueError(f"valid_prims must be a mask of the {K} primitives")


def _check_affine(rgb_affine):
    if rgb_affine is None or len(rgb_affine) != 2:
        raise ValueError("rgb_affine must be (scale, shift)")
    return float(rgb_affine[0]), float(rgb_affine[1])


def decode_template(x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, primsize, valid_prims=None, compact=True,
                    rgb_affine=(25.0, 100.0)):
    """The 16-channel input of the two last decoder layers -> the channels-last primitive template, differentiable w.r.t.
    all six tensors.

    x_rgb[B,16,h,w], w_rgb[16,3TD,4,4] (the effective weight, ConvTranspose2d layout), bias_rgb[3TD,2h,2w]; x_alpha[B,16,h,w],
    w_alpha[16,TD,4,4], bias_alpha[TD,2h,2w]; primsize = (TW, TH, TD), the reference's (x, y, z) order.  Returns
    template[B,K',TD,TH,TW,4] = relu(scale convT(x_rgb) + scale bias + shift) in the colours and relu(convT(x_alpha) + bias)
    in alpha; with x_rgb = w_rgb = bias_rgb = None the one-channel [B,K',TD,TH,TW].  valid_prims=None keeps all K = ny nx
    primitives, a mask with compact=True keeps the valid ones in order (`template[:, valid_prims]`), compact=False keeps all
    K with the invalid ones zeroed.  1 <= TD <= 10.  float32 compute, the result has x_alpha's dtype."""
    geom = _geometry(x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, primsize)
    ny, nx = geom[-2:]
    affine = _check_affine(rgb_affine)
    _check_mask(valid_prims, ny * nx)
    _need_gpu("decode_template", x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, valid_prims)
    if valid_prims is None:
        slot, live, Kout = None, None, ny * nx
    else:
        slot, live, Kout = prim_slots(valid_prims, compact)
    return _DecodeTemplate.apply(x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, geom, slot, live, Kout, affine)


def decode_template_torch(x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, primsize, valid_prims=None, compact=True,
                          rgb_affine=(25.0, 100.0)):
    """`decode_template` in plain PyTorch, in the reference's order of operations (hand_mvp.py:338-340 + untied bias, :434,
    :472, :172-185, render_raymarcher.py:41-47): parity twin, runs on the CPU in any float dtype."""
    B, h, w, TD, TH, TW, ny, nx = _geometry(x_rgb, w_rgb, bias_rgb, x_alpha, w_alpha, bias_alpha, primsize)
    scale, shift = _check_affine(rgb_affine)
    _check_mask(valid_prims, ny * nx)
    Sy, Sx = 2 * h, 2 * w
    alpha = F.relu((F.conv_transpose2d(x_alpha, w_alpha, None, 2, 1) + bias_alpha[None]).view(B, TD, 1, Sy, Sx))
    if x_rgb is not None:
        rgb = (F.conv_transpose2d(x_rgb, w_rgb, None, 2, 1) + bias_rgb[None]).view(B, TD, 3, Sy, Sx)
        rgb = F.relu(scale * rgb + shift)
        template = torch.cat([rgb, alpha], 2).view(B, TD, 4, ny, TH, nx, TW).permute(0, 3, 5, 1, 4, 6, 2)
        template = template.reshape(B, ny * nx, TD, TH, TW, 4)
    else:
        template = alpha.view(B, TD, ny, TH, nx, TW).permute(0, 2, 4, 1, 3, 5).reshape(B, ny * nx, TD, TH, TW)
    if valid_prims is None:
        return template
    keep = valid_prims != 0
    if compact:
        return template[:, keep].contiguous()
    return template * keep.to(template.dtype).view(1, -1, *([1] * (template.dim() - 2)))


# --------------------------------------------------------------------------------------------------------- model binding
class TailHandle:
    """A decoder that stopped in front of its last layer: the 16-channel activation `x`, the layer, and what the decoder's
    forward does with the layer's output (`channels` = 3: view + relu(25 y + 100), hand_mvp.py:465-472; 1: view + relu,
    :427-434).  `materialize()` runs those lines for a caller that wants the slab."""
    __slots__ = ("x", "layer", "TD", "channels", "_slab")

    def __init__(self, x, layer, TD, channels):
        self.x, self.layer, self.TD, self.channels, self._slab = x, layer, int(TD), int(channels), None

    def materialize(self):
        if self._slab is None:
            y = self.layer(self.x)
            y = y.view(y.shape[0], self.TD, self.channels, y.shape[-2], y.shape[-1])
            self._slab = F.relu(25.0 * y + 100.0) if self.channels == 3 else F.relu(y)
        return self._slab


def _fusable_last(layer, x, CH):
    """The last layer is a CUDA float32 ConvTranspose2dWNUB 16 -> CH, 4/2/1, whose untied bias has the output's size."""
    from .trunk import _is_convt_wnub

    if not _is_convt_wnub(layer) or not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32):
        return False
    v, g, bias = layer.weight_v, layer.weight_g, layer.bias
    if not all(t.is_cuda and t.dtype == torch.float32 for t in (v, g, bias)):
        return False
    return (tuple(v.shape[:2]) == (16, CH) and x.shape[1] == 16
            and tuple(bias.shape) == (CH, 2 * x.shape[2], 2 * x.shape[3]))


def tail_handle(decoder, x, TD, channels):
    """`decoder.texbranch` (hand_mvp.DeconvContentDecoder, :331-341) up to its last layer -> TailHandle, or None when the
    decoder has to run its own lines.  The hidden layers go through trunk.run_stack when trunk.enabled()."""
    from . import trunk

    seq = getattr(decoder, "texbranch", None)
    if not isinstance(seq, nn.Sequential) or len(seq) < 1 or not 1 <= int(TD) <= MAX_TD:
        return None
    hidden, last = seq[:-1], seq[-1]
    if not hasattr(last, "weight_v") or last.weight_v.dim() != 4 or tuple(last.weight_v.shape[:2]) != (16, TD * channels):
        return None      # decided before any hidden layer runs
    y = trunk.run_stack(hidden, x) if trunk.enabled() else hidden(x)
    handle = TailHandle(y, last, TD, channels)
    if not _fusable_last(last, y, TD * channels):
        return handle.materialize()    # the decoder's own lines on the activation that already exists
    return handle


def rgb_decoder_forward(self, view_cos_uv, joint, ambient_occlusion):
    """Drop-in for hand_mvp.RGBSlabDecoder.forward (hand_mvp.py:457-474) under patch_hand_mvp(fused_tail=True): the same
    calls in the same order, but the texture decoder stops in front of its last layer and a TailHandle is returned in
    place of the colour slab (the slab itself where the last layer is not the fusable one)."""
    B = joint.shape[0]
    ao_ds = F.interpolate(ambient_occlusion, (64, 64), mode="bilinear")
    view_cond = torch.cat((joint, view_cos_uv, ao_ds), 1)
    res = tail_handle(self.texdecoder, view_cond, self.primsize_z, 3)
    if res is None:
        rgb = self.texdecoder(view_cond).view(B, self.primsize_z, 3, self.uv_size, self.uv_size)
        res = F.relu(25.0 * rgb + 100.0)
    return res


def handles_fit(primrgb, primalpha, primsize):
    """Two TailHandles that `decode_template` takes together for primitives of `primsize`."""
    if not (isinstance(primrgb, TailHandle) and isinstance(primalpha, TailHandle)):
        return False
    TW, TH, TD = (int(v) for v in primsize)
    xr, xa = primrgb.x, primalpha.x
    return (primrgb.channels == 3 and primalpha.channels == 1 and primrgb.TD == TD and primalpha.TD == TD
            and xr.shape == xa.shape and (2 * xa.shape[2]) % TH == 0 and (2 * xa.shape[3]) % TW == 0)


def decode_handles(primrgb, primalpha, primsize, valid_prims=None):
    """decode_template on the two handles of a student's decoders (compacted, the reference's 25 x + 100)."""
    return decode_template(primrgb.x, wn_weight(primrgb.layer), primrgb.layer.bias, primalpha.x, wn_weight(primalpha.layer),
                           primalpha.layer.bias, primsize, valid_prims=valid_prims, compact=True)


def materialized(v):
    return v.materialize() if isinstance(v, TailHandle) else v
