"""The UNet of the MVP teacher: its levels as one split-bf16 operator each, opt-in.

`OLATRGBDecoder.forward_rgb` (ca_code/models/hand_teacher_mvp.py:253-494) runs, between the UNet input and the OLAT sum, ten
levels (:444-467, built at :185-241): each nn.Sequential(la.Conv2dWNUB(Ci, Co, 3, H, W, 1, 1), nn.LeakyReLU(0.2,
inplace=True)), with a bilinear resize between levels and, in the decoder half, a th.cat with the skip (or with
`joint_feat` at the bottom).  On the library that is a concatenation, a convolution, a bias add and an activation per level,
and their four backward kernels.

`conv3_ub_lrelu(xa, xb, weight, bias, leak)` is one level as ONE operator at precision "bf16x3" (gol_conv3ub_*,
csrc/conv3ub.hip): the 3x3 / stride 1 / pad 1 convolution of cat(xa, xb) -- which is never written -- + untied bias +
LeakyReLU forward; the gradients to xa, xb, weight and bias backward, each launched only where it is required.  The product
is the split one of `perceptual`: every operand written as two bf16 values, three bf16 MFMAs summed in fp32 (4.5e-6 rel-L2
from float64).  `conv3_ub_lrelu_split_torch` is that arithmetic in plain PyTorch (any device), with its own autograd.

The weight norm stays torch algebra on the small tensors (`tail.wn_weight`), so gradients reach weight_v / weight_g through
the ordinary graph and the kernels see the effective weight.

`forward(decoder, x, joint_feat, precision)` is the UNet of hand_teacher_mvp.py:444-467.  At "fp32" (the default everywhere)
it runs exactly the reference's lines.  At "bf16x3" a level whose layer is of the expected kind goes to the operator where
its (Ca, Cb, Co, H, W) is in `DISPATCH` -- the result of tools/olatunet_probe.py, by the
rule of section 6a -- or, with GOLIATH_FUSED_OLATUNET_ALL=1, for every supported shape (tests, probes); the skip or
`joint_feat` is handed over as `xb`, so no th.cat happens.  F.interpolate stays the library's.  Anything else -- a plain
nn.Conv2d, CPU or non-fp32 tensors, other shapes -- runs the module's own lines.
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_float, c_int, stream_ptr
from .featenc import _p, _sp, _three
from .perceptual import _precision
from .tail import wn_weight
from .texdec import _is_conv3_wn

# class attribute dropin.patch_hand_teacher(unet_precision=...) sets on OLATRGBDecoder: the `precision`
# goliath_amd.urhand.olat_rgb_decoder_forward_rgb_fused passes to `forward`
UNET_PRECISION_FLAG = "_gol_olat_unet_precision"

# (Ca, Cb, Co, H, W) of a level -> True, for precision="bf16x3": shapes where gol_conv3ub_* (pack + forward + the four
# gradients) won tools/olatunet_probe.py against cat + F.conv2d + bias add + leaky_relu and their autograd backward in fp32 by
# more than both sides' spread AT B L = 5 AND AT B L = 1 (profiles/olatunet_probe.json, "dispatch"; DESIGN.md section
# 6c-quinquies), MI355X, and nothing else.  Forward + backward medians in ms at B L = 5, then at 1: split operator against the
# library (and the two spreads).  Not admitted: the first level (56, 0, 64, 1024, 1024) -- 8.964 against 9.911 at 5 but 1.956
# against 1.892 at 1 -- and every level at 128^2 and 64^2 (launch-bound, within the spreads at B L = 1).  The weight gradient
# alone is BELOW the library's at the two-source levels (49-81 TF against 58-91; a tie at enc 1); the forward and the input
# gradients carry the win.
DISPATCH = {
    (64, 0, 64, 512, 512): True,       # enc 1: 2.498 against 3.516 (0.012, 0.089); 0.549 against 0.696 (0.007, 0.012)
    (64, 64, 64, 256, 256): True,      # dec 2: 1.089 against 1.566 (0.009, 0.028); 0.268 against 0.339 (0.022, 0.018)
    (64, 64, 64, 512, 512): True,      # dec 3: 4.448 against 6.395 (0.022, 0.219); 0.929 against 1.244 (0.009, 0.008)
    (64, 64, 32, 1024, 1024): True,    # dec 4: 13.007 against 15.834 (0.035, 0.325); 2.717 against 3.129 (0.013, 0.067)
}


def supported(Ca, Cb, Co, H, W):
    """Shapes gol_conv3ub_* take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    return (Ca > 0 and Cb >= 0 and Co > 0 and Co % 32 == 0 and Ca % 8 == 0 and Cb % 8 == 0 and (Cb == 0 or Ca % 32 == 0)
            and H >= 1 and W >= 1)


# the marshallers: the parameters of include/goliath_hip.h by name (tests/test_conv3ub_cpu.py holds them to the header)
def _abi_conv3ub_pack(*, Co, Ci, weight, packed):
    _lib.call("gol_conv3ub_pack", c_int(Co), c_int(Ci), _p(weight, "weight"), _sp(packed, "packed"), stream_ptr())


def _abi_conv3ub_fwd(*, B, Ca, Cb, Co, H, W, leak, xa, xb, packed, bias, y):
    _lib.call("gol_conv3ub_fwd", c_int(B), c_int(Ca), c_int(Cb), c_int(Co), c_int(H), c_int(W), c_float(leak), _p(xa, "xa"),
              _p(xb, "xb"), _sp(packed, "packed"), _p(bias, "bias"), _p(y, "y"), stream_ptr())


def _abi_conv3ub_bwd_x(*, B, Ca, Cb, Co, H, W, leak, packed, y, g_y, g_xa, g_xb):
    _lib.call("gol_conv3ub_bwd_x", c_int(B), c_int(Ca), c_int(Cb), c_int(Co), c_int(H), c_int(W), c_float(leak),
              _sp(packed, "packed"), _p(y, "y"), _p(g_y, "g_y"), _p(g_xa), _p(g_xb), stream_ptr())


def _abi_conv3ub_bwd_w(*, B, Ca, Cb, Co, H, W, leak, xa, xb, y, g_y, g_w, scratch):
    _lib.call("gol_conv3ub_bwd_w", c_int(B), c_int(Ca), c_int(Cb), c_int(Co), c_int(H), c_int(W), c_float(leak),
              _p(xa, "xa"), _p(xb, "xb"), _p(y, "y"), _p(g_y, "g_y"), _p(g_w), _p(scratch), stream_ptr())


def _abi_conv3ub_bwd_bias(*, B, Co, H, W, leak, y, g_y, g_bias):
    _lib.call("gol_conv3ub_bwd_bias", c_int(B), c_int(Co), c_int(H), c_int(W), c_float(leak), _p(y, "y"), _p(g_y, "g_y"),
              _p(g_bias), stream_ptr())


def packed_elems(Co, Ci):
    """16-bit elements of the packed weight (a pure host call; 0 for unsupported channel counts)."""
    fn = _lib.load().gol_conv3ub_packed_elems
    fn.restype = ctypes.c_longlong
    return int(fn(c_int(Co), c_int(Ci)))


def bwd_w_scratch_floats(B, Ca, Cb, Co, H, W):
    """Floats of scratch the weight gradient needs (a pure host call; 0 for an unsupported shape)."""
    fn = _lib.load().gol_conv3ub_bwd_w_scratch_floats
    fn.restype = ctypes.c_longlong
    return int(fn(c_int(B), c_int(Ca), c_int(Cb), c_int(Co), c_int(H), c_int(W)))


class _Conv3UB(torch.autograd.Function):
    """include/goliath_hip.h: gol_conv3ub_*.  Packs in forward; saves xa, xb (for the weight gradient), y and the packed
    weight (for the input gradients)."""

    @staticmethod
    def forward(ctx, xa, xb, weight, bias, leak):
        B, Ca, H, W = xa.shape
        Cb = 0 if xb is None else xb.shape[1]
        Co = weight.shape[0]
        dims = dict(B=B, Ca=Ca, Cb=Cb, Co=Co, H=H, W=W, leak=leak)
        packed = torch.empty(packed_elems(Co, Ca + Cb), device=xa.device, dtype=torch.int16)
        y = torch.empty(B, Co, H, W, device=xa.device)
        with _lib.device_guard(xa.device):
            _abi_conv3ub_pack(Co=Co, Ci=Ca + Cb, weight=weight, packed=packed)
            _abi_conv3ub_fwd(**dims, xa=xa, xb=xb, packed=packed, bias=bias, y=y)
        need_xa, need_xb, need_w = ctx.needs_input_grad[:3]
        ctx.save_for_backward(xa if need_w else None, xb if need_w else None, y, packed if need_xa or need_xb else None)
        ctx.dims = dims
        return y

    @staticmethod
    def backward(ctx, g):
        xa, xb, y, packed = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        d = ctx.dims
        need_xa, need_xb, need_w, need_b = ctx.needs_input_grad[:4]
        g_xa = g_xb = g_w = g_b = None
        new = lambda *shape: torch.empty(*shape, device=g.device)
        with _lib.device_guard(g.device):
            if need_xa or need_xb:
                g_xa = new(d["B"], d["Ca"], d["H"], d["W"]) if need_xa else None
                g_xb = new(d["B"], d["Cb"], d["H"], d["W"]) if need_xb else None
                _abi_conv3ub_bwd_x(**d, packed=packed, y=y, g_y=g, g_xa=g_xa, g_xb=g_xb)
            if need_w:
                g_w = new(d["Co"], d["Ca"] + d["Cb"], 3, 3)
                # per-workgroup partial sums, added in a fixed order by a second kernel: no float atomics
                scratch = new(bwd_w_scratch_floats(**{k: v for k, v in d.items() if k != "leak"}))
                _abi_conv3ub_bwd_w(**d, xa=xa, xb=xb, y=y, g_y=g, g_w=g_w, scratch=scratch)
            if need_b:
                g_b = new(d["Co"], d["H"], d["W"])
                _abi_conv3ub_bwd_bias(B=d["B"], Co=d["Co"], H=d["H"], W=d["W"], leak=d["leak"], y=y, g_y=g, g_bias=g_b)
        return g_xa, g_xb, g_w, g_b, None


def _level_shapes(name, xa, xb, weight, bias):
    """(Ca, Cb, Co, H, W) of a call, or an error naming what does not fit."""
    Cb = 0 if xb is None else xb.shape[1] if xb.dim() == 4 else -1
    ok = xa.dim() == 4 and weight.dim() == 4 and bias.dim() == 3 and Cb >= 0
    ok = ok and (xb is None or (xb.shape[0], *xb.shape[2:]) == (xa.shape[0], *xa.shape[2:]))
    ok = ok and tuple(weight.shape) == (weight.shape[0], xa.shape[1] + Cb, 3, 3)
    ok = ok and tuple(bias.shape) == (weight.shape[0], *xa.shape[2:])
    if not ok:
        raise _lib.GoliathHipError(f"{name}: shapes {tuple(xa.shape)}, {None if xb is None else tuple(xb.shape)}, "
                                   f"{tuple(weight.shape)}, {tuple(bias.shape)} (xa[B,Ca,H,W], xb[B,Cb,H,W] or None, "
                                   "weight[Co,Ca+Cb,3,3], bias[Co,H,W])")
    return xa.shape[1], Cb, weight.shape[0], xa.shape[2], xa.shape[3]


def conv3_ub_lrelu(xa, xb, weight, bias, leak=0.2):
    """xa[B,Ca,H,W], xb[B,Cb,H,W] or None, weight[Co,Ca+Cb,3,3] (effective), bias[Co,H,W] ->
    leaky_relu(conv2d(cat(xa, xb), weight, None, 1, 1) + bias[None], leak)[B,Co,H,W] at precision "bf16x3", with gradients
    to xa, xb, weight and bias (whichever are required).  fp32 CUDA(HIP) tensors, a shape `supported` admits, B <= 65535,
    leak > 0: anything else raises.  HIP kernels; no CPU path."""
    dims = _level_shapes("olatunet.conv3_ub_lrelu", xa, xb, weight, bias)
    if not supported(*dims) or xa.shape[0] > 65535:
        raise _lib.GoliathHipError("olatunet.conv3_ub_lrelu: unsupported shape B = %d, (Ca, Cb, Co, H, W) = %s: Co must be "
                                   "a multiple of 32, Ca and Cb of 8, Ca of 32 where Cb > 0, B <= 65535" % (xa.shape[0], dims))
    if not leak > 0:
        raise _lib.GoliathHipError(f"olatunet.conv3_ub_lrelu: leak must be positive, got {leak}")
    tensors = [t for t in (xa, xb, weight, bias) if t is not None]
    if not all(t.is_cuda for t in tensors):
        raise _lib.GoliathHipError("olatunet.conv3_ub_lrelu needs CUDA(HIP) tensors; there is no CPU path")
    if not all(t.dtype == torch.float32 for t in tensors):
        raise _lib.GoliathHipError(f"olatunet.conv3_ub_lrelu takes float32 tensors, got {[t.dtype for t in tensors]}")
    if xa.shape[0] == 0:
        x = xa if xb is None else torch.cat([xa, xb], 1)
        return F.leaky_relu(F.conv2d(x, weight, None, 1, 1) + bias[None], leak)
    return _Conv3UB.apply(xa.contiguous(), None if xb is None else xb.contiguous(), weight.contiguous(), bias.contiguous(),
                          float(leak))


class _SplitConv3UB(torch.autograd.Function):
    """conv3_ub_lrelu_split_torch: the forward and the four gradients of gol_conv3ub_* in `acc_dtype`, every convolution a
    split product; g_pre is formed in float32 from the upstream gradient and the sign of y, THEN split."""

    @staticmethod
    def forward(ctx, xa, xb, weight, bias, leak, acc_dtype, y_sign):
        x = xa if xb is None else torch.cat([xa, xb], 1)
        pre = _three(lambda a, w: F.conv2d(a, w, None, 1, 1), x, weight, acc_dtype) + bias.to(acc_dtype)[None]
        y = torch.where(pre > 0, pre, leak * pre)
        ctx.save_for_backward(x, weight, (y > 0) if y_sign is None else y_sign)
        ctx.leak, ctx.acc_dtype, ctx.Ca = leak, acc_dtype, xa.shape[1]
        ctx.dtypes = (xa.dtype, None if xb is None else xb.dtype, weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, positive = ctx.saved_tensors
        g = g.to(torch.float32)
        g_pre = torch.where(positive, g, ctx.leak * g)       # float32, as the kernels form it
        need_xa, need_xb, need_w, need_b = ctx.needs_input_grad[:4]
        ta, tb, tw, tbias = ctx.dtypes
        g_xa = g_xb = g_w = g_b = None
        if need_xa or need_xb:
            g_x = _three(lambda a, w: F.conv_transpose2d(a, w, None, 1, 1), g_pre, weight, ctx.acc_dtype)
            g_xa = g_x[:, :ctx.Ca].to(ta) if need_xa else None
            g_xb = g_x[:, ctx.Ca:].to(tb) if need_xb else None
        if need_w:
            g_w = _three(lambda a, v: torch.nn.grad.conv2d_weight(v, weight.shape, a, 1, 1), g_pre, x, ctx.acc_dtype).to(tw)
        if need_b:
            g_b = g_pre.to(ctx.acc_dtype).sum(0).to(tbias)
        return g_xa, g_xb, g_w, g_b, None, None, None


def conv3_ub_lrelu_split_torch(xa, xb, weight, bias, leak=0.2, acc_dtype=torch.float64, *, y_sign=None):
    """`conv3_ub_lrelu` in plain PyTorch, on any device: cat(xa, xb) and weight (taken as float32) are split by
    `perceptual.split_bf16` and the three products lo hi, hi lo, hi hi are three F.conv2d accumulated in `acc_dtype`; bias and
    leak follow in `acc_dtype`.  Its backward forms g_pre = y > 0 ? g : leak g in float32, splits it, the weight and x the
    same way and forms g_x (transposed convolution), g_w (correlation of g_pre with x) as three products each and g_bias as
    the batch sum in `acc_dtype`.  y_sign (a bool tensor of y's shape) replaces y > 0 in the backward: a parity test hands
    over the operator's own sign, so that a `pre` that rounds across zero is not counted against the gradients.  Returns
    `acc_dtype`; gradients come back in the inputs' dtypes."""
    _level_shapes("olatunet.conv3_ub_lrelu_split_torch", xa, xb, weight, bias)
    return _SplitConv3UB.apply(xa, xb, weight, bias, float(leak), acc_dtype, y_sign)


def _level(layer):
    """(conv, leak) if `layer` is nn.Sequential(weight-normalised 3x3 / 1 / 1 conv with an untied bias, LeakyReLU): this
    project's texdec.Conv3WNUB or the reference's la.Conv2dWNUB (same parameter names); None otherwise."""
    if not isinstance(layer, nn.Sequential) or len(layer) != 2 or not isinstance(layer[1], nn.LeakyReLU):
        return None
    if not _is_conv3_wn(layer[0], True) or not layer[1].negative_slope > 0:
        return None
    return layer[0], float(layer[1].negative_slope)


def _takes(layer, xa, xb, op):
    """Whether `layer` on cat(xa, xb) goes to the split operator `op`: a layer `_level` recognises whose weight and full-size
    bias fit the tensors, a shape `supported` and `DISPATCH` admit (or GOLIATH_FUSED_OLATUNET_ALL=1) and, for the HIP
    operator, fp32 tensors on the GPU."""
    kind = _level(layer)
    if not op or kind is None or xa.dim() != 4 or (xb is not None and (xb.dim() != 4 or xb.shape[2:] != xa.shape[2:])):
        return False
    conv = kind[0]
    Ca, Cb = xa.shape[1], 0 if xb is None else xb.shape[1]
    Co, H, W = conv.weight_v.shape[0], xa.shape[2], xa.shape[3]
    if conv.weight_v.shape[1] != Ca + Cb or tuple(conv.bias.shape) != (Co, H, W) or not 0 < xa.shape[0] <= 65535:
        return False
    if op is conv3_ub_lrelu and not all(t.is_cuda and t.dtype == torch.float32
                                        for t in (xa, xb, conv.weight_v, conv.weight_g, conv.bias) if t is not None):
        return False
    dims = (Ca, Cb, Co, H, W)
    return supported(*dims) and (os.environ.get("GOLIATH_FUSED_OLATUNET_ALL", "0") == "1" or DISPATCH.get(dims, False))


def forward(decoder, x, joint_feat, precision="fp32", op=None):
    """The UNet of OLATRGBDecoder.forward_rgb (hand_teacher_mvp.py:444-467) on x [B L, Ci, S, S] and joint_feat (already
    expanded to B L) -> the last level's output.  precision="fp32": the reference's lines and nothing else.  "bf16x3": a level
    `_takes` admits runs as op(xa, xb, wn_weight(conv), conv.bias, leak) with the skip or joint_feat as xb (no th.cat);
    op = None is the HIP operator `conv3_ub_lrelu`, `conv3_ub_lrelu_split_torch` (or any callable of those five arguments)
    the twin; a level that is not admitted runs the reference's lines."""
    op = (conv3_ub_lrelu if op is None else op) if _precision(precision) == "bf16x3" else False

    def level(layer, xa, xb):
        if _takes(layer, xa, xb, op):
            conv, leak = _level(layer)
            return op(xa, xb, wn_weight(conv), conv.bias, leak)
        return layer(xa if xb is None else torch.cat([xa, xb], dim=1))

    enc_acts = []
    for i, layer in enumerate(decoder.enc_layers):          # UNet encoder
        x = level(layer, x, None)
        enc_acts.append(x)
        if i < len(decoder.sizes) - 1:
            x = F.interpolate(x, scale_factor=0.5, mode="bilinear", recompute_scale_factor=True, align_corners=True)
    for i, layer in enumerate(decoder.dec_layers):          # UNet decoder with skip connections
        if i == 0:
            x = level(layer, x, joint_feat)
        else:
            skip = enc_acts[-i - 1]
            x = level(layer, F.interpolate(x, size=skip.shape[2:4], mode="bilinear", align_corners=True), skip)
    return x
