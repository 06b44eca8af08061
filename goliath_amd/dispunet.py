"""URHand's DisplacementUNet: a level of its two decoder branches as one fused operator.

`DisplacementUNet.forward` (ca_code/models/urhand.py:200-242, built at :109-198) runs, per level 1..n of either decoder
branch (:217-226, :231-239), `F.leaky_relu(x, 0.2)` on the previous layer's output, an exact 2x
`F.interpolate(..., mode="bilinear", align_corners=True)`, `th.cat([x, x_prev], 1)` with the encoder's skip and a
weight-normalised 3x3 / stride 1 / pad 1 convolution with an untied bias (la.Conv2dWNUB), and after the last level tanh
and an affine (:227-228 displacement, :240-241 roughness): the activated, the upsampled and the concatenated tensor are
each written and read back, forwards and backwards.  `upcat_conv` runs such a level as ONE HIP kernel forward
(gol_upcat_conv_fwd: the leaky and the bilinear blend happen while the first half of the operand is loaded, the skip is
the second half of the same K loop, fp32-MFMA implicit GEMM, bias / tanh / affine on the accumulators, nothing but y
written) and up to five backward (gol_upcat_conv_bwd: gradient of xa as the bilinear adjoint gathered on chip times the
leaky mask, gradient of the skip as a transposed convolution with mirrored taps, weight gradient with the upsampled
operand recomputed and a fixed-order reduction, bias gradient; no float atomics).  The resize follows the integer-ratio
coordinate rule of include/goliath_hip.h; `upcat_conv_torch` is the same composition in plain PyTorch (any device, any
dtype: the float64 twin).

The weight norm stays torch algebra on the small tensor (`tail.wn_weight`), as in goliath_amd/texdec.py.

`forward` mirrors DisplacementUNet.forward and takes the operator for the decoder levels whose (Ca, Cb, Co, Hi, Wi) is
in `DISPATCH` -- the per-shape result of tools/dispunet_probe.py, by the rule of section 6a: a
shape is admitted only where the HIP operator's forward + backward beat the library composition by more than the
composition's own run-to-run spread.  GOLIATH_FUSED_DISPUNET_ALL=1 forces the operator for every supported shape (tests,
probes).  The encoder and decoder layer 0 of both branches stay on the library lines.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_float, c_int, fptr, stream_ptr
from .tail import wn_weight
from .texdec import Conv3WNUB, _is_conv3_wn

LEAK = 0.2                    # urhand.py:205,222,235
ROUGHNESS_HEAD = (0.25, 0.55)  # (tanh + 1) / 4 + 0.3 (urhand.py:240-241) as tanh * scale + shift

# class attribute dropin.patch_urhand(displacement_unet=True) sets on the decoder class: its forward calls `forward` here
DISPLACEMENT_UNET_FLAG = "_gol_displacement_unet"

# (Ca, Cb, Co, Hi, Wi) of a decoder level (Hi, Wi: the size of xa) -> True: shapes where the HIP operator won the probe
# (B = 1, MI355X).  From profiles/dispunet_probe.json ("dispatch"; forward + backward medians in ms, HIP against the library
# composition, and the composition's spread).  Shapes that are not listed stay on the library lines inside `forward`: the
# four 64 + 64 -> 64 levels lose in both branches (32^2 ... 256^2: 0.30 / 0.40 / 0.63 / 1.96 ms against 0.24 / 0.24 / 0.38 /
# 1.35; the measured table is in DESIGN.md section 6c-bis).
DISPATCH = {
    (64, 64, 1, 512, 512): True,   # both heads: 1.398 ms against 2.713 (torch spread 0.026) with the displacement head,
                                   # 1.395 against 2.733 (0.034) with the roughness head
}


def supported(Ca, Cb, Co, Hi, Wi):
    """Shapes the kernels take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    return (Ca >= 8 and Ca % 8 == 0 and Cb >= 8 and Cb % 8 == 0 and (Co % 8 == 0 or 1 <= Co <= 4) and Co > 0
            and Hi > 0 and Wi > 0)


def _act_args(act):
    """act=None -> (0, 1, 0); act=("tanh", scale, shift) -> (1, scale, shift)."""
    if act is None:
        return 0, 1.0, 0.0
    if len(act) != 3 or act[0] != "tanh":
        raise _lib.GoliathHipError(f"upcat_conv: act must be None or ('tanh', scale, shift), got {act!r}")
    return 1, float(act[1]), float(act[2])


class _UpCat(torch.autograd.Function):
    """include/goliath_hip.h: gol_upcat_conv_*."""

    @staticmethod
    def forward(ctx, xa, xb, weight, bias, leak, act, scale, shift):
        B, Ca, Hi, Wi = xa.shape
        Cb, Co = xb.shape[1], weight.shape[0]
        y = torch.empty(B, Co, 2 * Hi, 2 * Wi, device=xa.device)
        dims = (c_int(B), c_int(Ca), c_int(Cb), c_int(Co), c_int(Hi), c_int(Wi), c_int(act), c_float(leak), c_float(scale),
                c_float(shift))
        with _lib.device_guard(xa.device):
            _lib.call("gol_upcat_conv_fwd", *dims, fptr(xa, "xa"), fptr(xb, "xb"), fptr(weight, "weight"),
                      fptr(bias, "bias"), fptr(y), stream_ptr())
        ctx.save_for_backward(xa, xb, weight, y if act == 1 else None)
        ctx.dims = dims
        return y

    @staticmethod
    def backward(ctx, g):
        xa, xb, weight, y = ctx.saved_tensors
        Co, H, W = weight.shape[0], xb.shape[2], xb.shape[3]
        g = g.to(torch.float32).contiguous()
        need_xa, need_xb, need_w, need_b = ctx.needs_input_grad[:4]
        g_xa = torch.empty_like(xa) if need_xa else None
        g_xb = torch.empty_like(xb) if need_xb else None
        g_w = torch.empty_like(weight) if need_w else None
        g_b = torch.empty(Co, H, W, device=xa.device) if need_b else None
        scratch = None
        if need_w:  # per-workgroup partial sums of the weight gradient (reduced by a second kernel: no float atomics)
            fn = _lib.load().gol_upcat_conv_bwd_scratch_floats
            fn.restype = ctypes.c_longlong
            scratch = torch.empty(int(fn(*ctx.dims[:6])), device=xa.device)
        with _lib.device_guard(xa.device):
            _lib.call("gol_upcat_conv_bwd", *ctx.dims, fptr(xa, "xa"), fptr(xb, "xb"), fptr(weight, "weight"), fptr(y, "y"),
                      fptr(g, "g_y"), fptr(g_xa), fptr(g_xb), fptr(g_w), fptr(g_b), fptr(scratch), stream_ptr())
        return g_xa, g_xb, g_w, g_b, None, None, None, None


def _f32(t):
    return t.to(torch.float32).contiguous()


def _shapes(xa, xb, weight, bias):
    """(Ca, Cb, Co, Hi, Wi) of a call, or an error naming what does not fit."""
    if xa.dim() != 4 or xb.dim() != 4 or weight.dim() != 4:
        raise _lib.GoliathHipError(f"upcat_conv: shapes {tuple(xa.shape)}, {tuple(xb.shape)}, {tuple(weight.shape)}")
    B, Ca, Hi, Wi = xa.shape
    Cb, Co = xb.shape[1], weight.shape[0]
    if tuple(xb.shape) != (B, Cb, 2 * Hi, 2 * Wi):
        raise _lib.GoliathHipError(f"upcat_conv: skip {tuple(xb.shape)} is not twice the size of {tuple(xa.shape)}")
    if tuple(weight.shape) != (Co, Ca + Cb, 3, 3):
        raise _lib.GoliathHipError(f"upcat_conv: weight {tuple(weight.shape)} for {Ca} + {Cb} input channels")
    if tuple(bias.shape) != (Co, 2 * Hi, 2 * Wi):
        raise _lib.GoliathHipError(f"upcat_conv: bias {tuple(bias.shape)} for an output {(B, Co, 2 * Hi, 2 * Wi)}")
    return Ca, Cb, Co, Hi, Wi


def upcat_conv(xa, xb, weight, bias, leak=LEAK, act=None):
    """xa[B,Ca,Hi,Wi] (before its activation), xb[B,Cb,2Hi,2Wi], weight[Co,Ca+Cb,3,3] (effective), bias[Co,2Hi,2Wi] ->
    conv(cat(bilinear 2x (lrelu(xa, leak)), xb), weight, s1 p1) + bias, and with act=("tanh", scale, shift)
    tanh(.) * scale + shift.  HIP kernels; no CPU path."""
    code, scale, shift = _act_args(act)
    dims = _shapes(xa, xb, weight, bias)
    if not supported(*dims):
        raise _lib.GoliathHipError("upcat_conv: unsupported shape (Ca, Cb, Co, Hi, Wi) = %s: Ca and Cb must be positive "
                                   "multiples of 8, Co a multiple of 8 or 1..4" % (dims,))
    if xa.shape[0] > 65535:
        raise _lib.GoliathHipError(f"upcat_conv: unsupported batch {xa.shape[0]} > 65535")
    if not (xa.is_cuda and xb.is_cuda and weight.is_cuda and bias.is_cuda):
        raise _lib.GoliathHipError("upcat_conv needs CUDA(HIP) tensors; there is no CPU path")
    return _UpCat.apply(_f32(xa), _f32(xb), _f32(weight), _f32(bias), float(leak), code, scale, shift)


def _axis(n, device, dtype):
    """Source indices and fractions of the 2n rows of an exact 2x align_corners resize, by the integer-ratio rule of
    include/goliath_hip.h: r0 = (r (n-1)) div (2n-1), frac = ((r (n-1)) mod (2n-1)) / (2n-1), r1 = min(r0+1, n-1)."""
    d = 2 * n - 1
    nr = torch.arange(2 * n, device=device) * (n - 1)
    a = torch.div(nr, d, rounding_mode="floor")
    return a, torch.clamp(a + 1, max=n - 1), (nr - a * d).to(dtype) / d


def up2_integer(x):
    """Exact 2x bilinear resize, align_corners=True, by the integer-ratio rule (equal to F.interpolate in exact arithmetic)."""
    ra, rb, rf = _axis(x.shape[2], x.device, x.dtype)
    ca, cb, cf = _axis(x.shape[3], x.device, x.dtype)
    rows = x[:, :, ra] * (1 - rf)[:, None] + x[:, :, rb] * rf[:, None]
    return rows[:, :, :, ca] * (1 - cf) + rows[:, :, :, cb] * cf


def upcat_conv_torch(xa, xb, weight, bias, leak=LEAK, act=None):
    """The same composition in plain PyTorch, in the reference's order of operations (urhand.py:222-228) with the
    integer-ratio resize: parity twin, any device, any dtype."""
    code, scale, shift = _act_args(act)
    _shapes(xa, xb, weight, bias)
    x = torch.cat([up2_integer(F.leaky_relu(xa, leak)), xb], dim=1)
    y = F.conv2d(x, weight, None, 1, 1) + bias[None]
    return torch.tanh(y) * scale + shift if code else y


def _admitted(dims):
    return supported(*dims) and (os.environ.get("GOLIATH_FUSED_DISPUNET_ALL", "0") == "1" or DISPATCH.get(dims, False))


def _takes_operator(layer, xa, xb, op):
    """Whether decoder level `layer` on (xa, xb) goes to `op`: a weight-normalised 3x3 / s1 / p1 layer with an untied bias,
    a skip of exactly twice xa's size, a shape that passes `supported` and `DISPATCH` (or GOLIATH_FUSED_DISPUNET_ALL=1) and,
    for the HIP operator, fp32 tensors on the GPU."""
    if not op or not (_is_conv3_wn(layer, True) and xa.dim() == 4 and xb.dim() == 4):
        return False
    Co, Ct = layer.weight_v.shape[:2]
    B, Ca, Hi, Wi = xa.shape
    Cb = xb.shape[1]
    if tuple(xb.shape) != (B, Cb, 2 * Hi, 2 * Wi) or Ct != Ca + Cb or tuple(layer.bias.shape) != (Co, 2 * Hi, 2 * Wi):
        return False
    if op is upcat_conv and not all(t.is_cuda and t.dtype == torch.float32 for t in (xa, xb, layer.weight_v, layer.bias)):
        return False
    return B <= 65535 and _admitted((Ca, Cb, Co, Hi, Wi))


def _decode(layers, x, enc_acts, head, finish, op):
    """One decoder branch (urhand.py:217-228 / :231-241) from the input of its layer 0.  head = (scale, shift) of the tanh
    head as the operator takes it, finish = the reference's own lines after the last layer."""
    fused_head = False
    for i, layer in enumerate(layers):
        if i == 0:
            x = layer(x)
            continue
        x_prev = enc_acts[-i - 1]
        last = i == len(layers) - 1
        if _takes_operator(layer, x, x_prev, op):
            x = op(x, x_prev, wn_weight(layer), layer.bias, LEAK, ("tanh",) + tuple(head) if last else None)
            fused_head = last
        else:
            x = F.leaky_relu(x, 0.2, inplace=True)
            x = F.interpolate(x, size=x_prev.shape[2:4], mode="bilinear", align_corners=True)
            x = torch.cat([x, x_prev], dim=1)
            x = layer(x)
    return x if fused_head else finish(torch.tanh(x))


def forward(unet, feat_uv, pose_cond, op=None):
    """DisplacementUNet.forward (urhand.py:200-242) -> (disp, roughness, interm_feat).  The encoder and decoder layer 0 of
    both branches are the reference's lines; decoder levels 1..n go to `op` where `_takes_operator` admits them and run the
    reference's four lines verbatim otherwise.  op = None is the HIP operator `upcat_conv`; `upcat_conv_torch` routes the
    same levels to the torch twin (any device, float64); False admits nothing (the library composition)."""
    op = upcat_conv if op is None else op
    enc_acts = []
    x = feat_uv
    n = len(unet.enc_layers)
    for i, layer in enumerate(unet.enc_layers):          # unet enc
        x = F.leaky_relu(layer(x), 0.2, inplace=True)
        enc_acts.append(x)
        if i < n - 1:
            x = F.interpolate(x, scale_factor=0.5, mode="bilinear", recompute_scale_factor=True, align_corners=True)
    enc_x = x
    interm_feat = torch.cat([enc_x, pose_cond], dim=1)
    disp = _decode(unet.dec_layers, interm_feat, enc_acts, (float(unet.output_scale), 0.0),
                   lambda t: t * unet.output_scale, op)
    roughness = _decode(unet.dec_layers_roughness, enc_x, enc_acts, ROUGHNESS_HEAD,
                        lambda t: (t + 1) / 4. + 0.3, op)   # [-1, 1] -> [0.3, 0.8]
    return disp, roughness, interm_feat


class DisplacementUNet(nn.Module):
    """Module twin of the reference's DisplacementUNet (urhand.py:109-242) under its state-dict names
    (enc_layers.i.{bias,weight_g,weight_v}, dec_layers.*, dec_layers_roughness.*): a reference checkpoint loads.  Its own
    forward is the library composition (`forward` of this module with nothing admitted)."""

    def __init__(self, uv_size, init_uv_size, output_scale, pose_feat_dim, n_enc_dims=(64, 64, 64, 64, 64, 64)):
        super().__init__()
        self.uv_size, self.init_uv_size, self.output_scale = uv_size, init_uv_size, output_scale
        self.n_blocks = int(np.log2(uv_size // init_uv_size))
        self.sizes = [init_uv_size * 2 ** s for s in range(self.n_blocks + 1)]
        d = list(n_enc_dims)
        enc = [(2 * 3, d[0])] + [(d[i], d[i + 1]) for i in range(5)]            # id mesh & normal
        dec = [(d[5] + pose_feat_dim, d[4])] + [(d[4 - i] * 2, d[3 - i]) for i in range(4)] + [(d[0] * 2, 1)]
        rough = [(d[5], d[4])] + dec[1:]
        n = len(self.sizes)
        self.enc_layers = nn.ModuleList(Conv3WNUB(*enc[i], self.sizes[-i - 1], self.sizes[-i - 1]) for i in range(n))
        self.dec_layers, self.dec_layers_roughness = (
            nn.ModuleList(Conv3WNUB(*dims[i], s, s, alpha=1.0 if i == n - 1 else LEAK) for i, s in enumerate(self.sizes))
            for dims in (dec, rough))

    def forward(self, feat_uv, pose_cond):
        return forward(self, feat_uv, pose_cond, op=False)
