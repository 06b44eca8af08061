"""URHand's texture decoder: a layer of its two 7-layer branches as one fused operator.

`ConvTeacherDecoder.forward` (/root/reference/ca_code/models/urhand.py:583-608, layers built at :302-323) runs, per layer and
branch, an exact 2x `F.interpolate(..., mode="bilinear", align_corners=True)`, a weight-normalised 3x3 / stride 1 / pad 1
convolution and either an untied bias + LeakyReLU(0.2) (`texmod0`, la.Conv2dWNUB) or a gate by the other branch's
activation, + gainbias, * 0.707107 (`texmod1`, la.Conv2dWN without bias): the upsampled tensor is written and read back,
forwards and backwards.  `upconv_lrelu` / `upconv_gated` run such a layer as ONE HIP kernel forward (gol_upconv_fwd: the
bilinear blend happens while the operand is loaded, fp32-MFMA implicit GEMM, the epilogue on the accumulators, nothing but
y written) and up to four backward (gol_upconv_bwd: input gradient as the bilinear adjoint gathered on chip, weight
gradient with the upsampled operand recomputed, bias gradient, gate gradient with the accumulator recomputed; no float
atomics).  The resize follows the integer-ratio coordinate rule of include/goliath_hip.h, so the operator is pinned
against float64; `upconv_lrelu_torch` / `upconv_gated_torch` are the same compositions in plain PyTorch (parity twins, CPU,
float64).

The weight norm stays torch algebra on the small tensor (`tail.wn_weight`), so gradients reach weight_v / weight_g
through the ordinary graph and the kernels see the effective weight.

`texture_branches` walks the two loops and takes the operator for the layers whose (mode, Ci, Co, Hi, Wi) is in
`DISPATCH` -- the per-shape result of tools/texdec_probe.py, by the rule of section 6a: a shape is
admitted only where the HIP operator's forward + backward beat the library composition by more than the composition's
own run-to-run spread.  GOLIATH_FUSED_TEXDEC_ALL=1 forces the operator for every supported shape (tests, probes).
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_float, c_int, fptr, stream_ptr
from .decoder import LEAK, _glorot_, _wn
from .tail import wn_weight

# (Ci, Co) of the seven layers of either branch (urhand.py:302-323); layer i reads 32 * 2^i squared, writes twice that
CHANNELS = ((128, 256), (256, 128), (128, 128), (128, 64), (64, 32), (32, 16), (16, 4))
GAIN_SCALE = 0.707107   # urhand.py:588,606

# class attribute dropin.patch_urhand(texture_decoder=True) sets on the decoder class: its forward calls texture_branches
TEXTURE_DECODER_FLAG = "_gol_texture_decoder"

# (mode, Ci, Co, Hi, Wi) of the layer INPUT -> True: shapes where the HIP operator won the probe (B = 1, MI355X).
# From profiles/texdec_probe.json ("dispatch"; forward + backward medians in ms, HIP against the library composition, and
# the composition's spread); shapes that are not listed stay on the library lines inside texture_branches: the five
# smaller layers of either branch lose (128->256 at 32^2 ... 64->32 at 512^2: 0.49 ... 2.61 ms against 0.18 ... 2.03 in
# mode 0, 0.69 ... 3.04 against 0.24 ... 2.06 in mode 1; the measured table is in DESIGN.md section 6c).
DISPATCH = {
    (0, 32, 16, 1024, 1024): True,   # 2.860 ms against 3.875 (torch spread 0.030)
    (0, 16, 4, 2048, 2048): True,    # 3.937 ms against 8.134 (0.049)
    (1, 32, 16, 1024, 1024): True,   # 3.236 ms against 3.892 (0.033); no gainbias at this layer
    (1, 16, 4, 2048, 2048): True,    # 4.824 ms against 8.198 (0.059); no gainbias at this layer
}


def supported(Ci, Co, Hi, Wi):
    """Shapes the kernels take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    return Ci > 0 and Co > 0 and Hi > 0 and Wi > 0 and Ci % 8 == 0 and (Co % 16 == 0 or Co <= 4)


class _UpConv(torch.autograd.Function):
    """include/goliath_hip.h: gol_upconv_*.  mode 0: a = bias[Co,H,W], gb unused; mode 1: a = gate[B,Co,H,W], gb or None."""

    @staticmethod
    def forward(ctx, x, weight, a, gb, mode, leak, scale):
        B, Ci, Hi, Wi = x.shape
        Co = weight.shape[0]
        y = torch.empty(B, Co, 2 * Hi, 2 * Wi, device=x.device)
        dims = (c_int(B), c_int(Ci), c_int(Co), c_int(Hi), c_int(Wi), c_int(mode), c_float(leak), c_float(scale))
        with _lib.device_guard(x.device):
            _lib.call("gol_upconv_fwd", *dims, fptr(x, "x"), fptr(weight, "weight"), fptr(a if mode == 0 else None, "bias"),
                      fptr(a if mode == 1 else None, "gate"), fptr(gb, "gb"), fptr(y), stream_ptr())
        ctx.save_for_backward(x, weight, y if mode == 0 else a)
        ctx.dims = dims
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, aux = ctx.saved_tensors
        B, Ci, Hi, Wi = x.shape
        Co, mode = weight.shape[0], ctx.dims[5].value
        g = g.to(torch.float32).contiguous()
        need_x, need_w, need_a, need_gb = ctx.needs_input_grad[:4]
        g_x = torch.empty_like(x) if need_x else None
        g_w = torch.empty_like(weight) if need_w else None
        g_a = (torch.empty(Co, 2 * Hi, 2 * Wi, device=x.device) if mode == 0 else torch.empty_like(g)) if need_a else None
        g_gb = torch.empty_like(g) if (need_gb and mode == 1) else None
        scratch = None
        if need_w:  # per-workgroup partial sums of the weight gradient (reduced by a second kernel: no float atomics)
            fn = _lib.load().gol_upconv_bwd_scratch_floats
            fn.restype = ctypes.c_longlong
            scratch = torch.empty(int(fn(*ctx.dims[:5])), device=x.device)
        with _lib.device_guard(x.device):
            _lib.call("gol_upconv_bwd", *ctx.dims, fptr(x, "x"), fptr(weight, "weight"),
                      fptr(aux if mode == 0 else None, "y"), fptr(aux if mode == 1 else None, "gate"), fptr(g, "g_y"),
                      fptr(g_x), fptr(g_w), fptr(g_a if mode == 0 else None), fptr(g_a if mode == 1 else None), fptr(g_gb),
                      fptr(scratch), stream_ptr())
        return g_x, g_w, g_a, g_gb, None, None, None


def _check(name, x, weight):
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape) != (weight.shape[0], x.shape[1], 3, 3):
        raise _lib.GoliathHipError(f"{name}: shapes {tuple(x.shape)}, {tuple(weight.shape)}")
    B, _, Hi, Wi = x.shape
    return (B, weight.shape[0], 2 * Hi, 2 * Wi)


def _f32(t):
    return t.to(torch.float32).contiguous()


def upconv_lrelu(x, weight, bias, leak=0.2):
    """x[B,Ci,Hi,Wi], weight[Co,Ci,3,3] (effective), bias[Co,2Hi,2Wi] ->
    lrelu(conv(bilinear 2x (x), weight, s1 p1) + bias)[B,Co,2Hi,2Wi].  HIP kernels; no CPU path."""
    if not (x.is_cuda and weight.is_cuda and bias.is_cuda):
        raise _lib.GoliathHipError("upconv_lrelu needs CUDA(HIP) tensors; there is no CPU path")
    out = _check("upconv_lrelu", x, weight)
    if tuple(bias.shape) != out[1:]:
        raise _lib.GoliathHipError(f"upconv_lrelu: bias {tuple(bias.shape)} for an output {out}")
    return _UpConv.apply(_f32(x), _f32(weight), _f32(bias), None, 0, float(leak), 1.0)


def upconv_gated(x, weight, gate, gb=None, scale=GAIN_SCALE):
    """x[B,Ci,Hi,Wi], weight[Co,Ci,3,3] (effective), gate[B,Co,2Hi,2Wi], gb (broadcastable to the gate's shape) or None ->
    (conv(bilinear 2x (x), weight, s1 p1) * gate + gb) * scale.  HIP kernels; no CPU path."""
    if not (x.is_cuda and weight.is_cuda and gate.is_cuda and (gb is None or gb.is_cuda)):
        raise _lib.GoliathHipError("upconv_gated needs CUDA(HIP) tensors; there is no CPU path")
    out = _check("upconv_gated", x, weight)
    if tuple(gate.shape) != out:
        raise _lib.GoliathHipError(f"upconv_gated: gate {tuple(gate.shape)} for an output {out}")
    if gb is not None:
        try:
            gb = _f32(gb.expand(out))
        except RuntimeError as e:
            raise _lib.GoliathHipError(f"upconv_gated: gb {tuple(gb.shape)} for an output {out}") from e
    return _UpConv.apply(_f32(x), _f32(weight), _f32(gate), gb, 1, 1.0, float(scale))


def _up2(x):
    return F.interpolate(x, (2 * x.shape[2], 2 * x.shape[3]), mode="bilinear", align_corners=True)


def upconv_lrelu_torch(x, weight, bias, leak=0.2):
    """The same composition in plain PyTorch, in the reference's order of operations (urhand.py:592-597): parity twin,
    runs on CPU and in float64."""
    return F.leaky_relu(F.conv2d(_up2(x), weight, None, 1, 1) + bias[None], leak)


def upconv_gated_torch(x, weight, gate, gb=None, scale=GAIN_SCALE):
    """The same composition in plain PyTorch, in the reference's order of operations (urhand.py:600-606)."""
    y = F.conv2d(_up2(x), weight, None, 1, 1) * gate
    if gb is not None:
        y = y + gb
    return y * scale


class Conv3WNUB(nn.Module):
    """3x3 / stride 1 / pad 1 conv, weight-normalised, untied bias [C_out, height, width]: la.Conv2dWNUB(.., 3, 1, 1)."""

    def __init__(self, n_in, n_out, height, width, alpha=LEAK):
        super().__init__()
        self.weight_v = nn.Parameter(torch.empty(n_out, n_in, 3, 3))
        _glorot_(self.weight_v, n_in, n_out, 9, alpha)
        self.weight_g = nn.Parameter(torch.full((n_out, 1, 1, 1), float(self.weight_v.detach().norm())))
        self.bias = nn.Parameter(torch.zeros(n_out, height, width))

    def weight(self):
        return _wn(self.weight_v, self.weight_g)

    def forward(self, x):
        return F.conv2d(x, self.weight(), None, 1, 1) + self.bias[None]


class Conv3WN(nn.Module):
    """3x3 / stride 1 / pad 1 conv, weight-normalised, no bias: la.Conv2dWN(.., 3, 1, 1, bias=False)."""

    def __init__(self, n_in, n_out, alpha=1.0):
        super().__init__()
        self.weight_v = nn.Parameter(torch.empty(n_out, n_in, 3, 3))
        _glorot_(self.weight_v, n_in, n_out, 9, alpha)
        self.weight_g = nn.Parameter(torch.full((n_out, 1, 1, 1), float(self.weight_v.detach().norm())))
        self.register_parameter("bias", None)

    def weight(self):
        return _wn(self.weight_v, self.weight_g)

    def forward(self, x):
        return F.conv2d(x, self.weight(), None, 1, 1)


def _is_conv3_wn(m, untied_bias):
    """A weight-normalised 3x3 / stride 1 / pad 1 conv: this module's or the reference's layer (same parameter names), with
    an untied 3-D bias (texmod0) or without any bias (texmod1).  Not another kernel size or stride, not a tied bias, not a
    layer without weight norm."""
    if isinstance(m, nn.ConvTranspose2d) or not all(hasattr(m, a) for a in ("weight_v", "weight_g")):
        return False
    bias = getattr(m, "bias", None)
    if (bias is None or bias.dim() != 3) if untied_bias else (bias is not None):
        return False
    if m.weight_v.dim() != 4 or tuple(m.weight_v.shape[2:]) != (3, 3) or tuple(m.weight_g.shape) != (m.weight_v.shape[0], 1, 1, 1):
        return False
    if isinstance(m, (Conv3WNUB, Conv3WN)):
        return True
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    return (isinstance(m, nn.Conv2d) and pair(m.stride) == (1, 1) and pair(m.padding) == (1, 1)
            and pair(m.dilation) == (1, 1) and m.groups == 1 and m.padding_mode == "zeros")


def _on_gpu(*tensors):
    return all(t is None or t.is_cuda for t in tensors)


def _takes_hip(mode, layer, x, hh, *others):
    """Whether layer (already recognised) on input x with the target size (hh, hh) goes to the operator; `others` are the
    further tensors the call would read (the gate, the gainbias)."""
    if not (x.dim() == 4 and _on_gpu(x, layer.weight_v, layer.bias, *others)):
        return False
    Co, Ci = layer.weight_v.shape[:2]
    Hi, Wi = x.shape[2:]
    if x.shape[1] != Ci or (2 * Hi, 2 * Wi) != (hh, hh) or not supported(Ci, Co, Hi, Wi):
        return False
    if mode == 0 and tuple(layer.bias.shape) != (Co, hh, hh):
        return False
    if mode == 1 and tuple(others[0].shape) != (x.shape[0], Co, hh, hh):
        return False
    return os.environ.get("GOLIATH_FUSED_TEXDEC_ALL", "0") == "1" or DISPATCH.get((mode, Ci, Co, Hi, Wi), False)


def texture_branches(decoder, joint_feat, z, gainbias, first_size=64):
    """The two loops of `ConvTeacherDecoder.forward` (urhand.py:583-608; goliath_amd/urhand.py): the non-linear branch on
    `joint_feat`, then the linear branch on `z` gated by the first one's activations.  Returns x before the final resize to
    uv_size.  A layer goes to `upconv_lrelu` / `upconv_gated` only if it is a weight-normalised 3x3 / s1 / p1 layer (untied
    3-D bias in texmod0, no bias in texmod1), the tensors are on the GPU, its input is exactly (hh/2, hh/2) and the shape
    passes `supported` and `DISPATCH` (or GOLIATH_FUSED_TEXDEC_ALL=1); otherwise the reference's three lines run unchanged.
    `first_size` is the output size of the first layer: 64 in the model (urhand.py:591,599); tests run smaller stacks."""
    acts, x, hh = [], joint_feat, first_size
    for i in range(decoder.n_layers_tex):                # non-linear branch
        layer = decoder.texmod0[i]
        if _is_conv3_wn(layer, True) and _takes_hip(0, layer, x, hh):
            x = upconv_lrelu(x, wn_weight(layer), layer.bias, 0.2)
        else:
            x = F.interpolate(x, (hh, hh), mode="bilinear", align_corners=True)
            x = F.leaky_relu(layer(x), 0.2)
        acts.append(x)
        hh *= 2
    x, hh = z, first_size
    for i in range(decoder.n_layers_tex):                # energy-in / energy-out linear branch, gated by the activations
        layer = decoder.texmod1[i]
        gb = gainbias[i] if i < len(gainbias) else None
        if _is_conv3_wn(layer, False) and _takes_hip(1, layer, x, hh, acts[i], gb):
            x = upconv_gated(x, wn_weight(layer), acts[i], gb, GAIN_SCALE if gb is not None else 1.0)
            hh *= 2
        else:
            x = F.interpolate(x, (hh, hh), mode="bilinear", align_corners=True)
            x = layer(x) * acts[i]
            hh *= 2
            if gb is not None:
                x = (x + gb) * 0.707107
    return x
