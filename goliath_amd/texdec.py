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

precision="bf16x3" (opt-in; "fp32" is the default everywhere and runs exactly the lines above) takes the same layer through
gol_upconvx_* (csrc/upconvx.hip): the same fusion, with every product of the three convolutions the split one of
`perceptual` -- U after its fp32 blend, g_pre after it is formed and the weight written as two bf16 values each, three bf16
MFMAs summed in fp32.  `upconv_lrelu_split_torch` / `upconv_gated_split_torch` are that arithmetic in plain PyTorch (any
device), with their own autograd.  `texture_branches(..., precision="bf16x3")` takes it for the layers whose shape passes
`supported_bf16x3` and is in `DISPATCH_BF16X3` (tools/texdecx_probe.py), or for every such
shape with GOLIATH_FUSED_TEXDEC_ALL=1; any other layer takes exactly the "fp32" decision.
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_float, c_int, fptr, stream_ptr
from .decoder import LEAK, _glorot_, _wn
from .perceptual import _precision, _three
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

# stored next to TEXTURE_DECODER_FLAG by dropin.patch_urhand(texture_decoder_precision=...): the `precision`
# goliath_amd.urhand passes to texture_branches
TEXDEC_PRECISION_FLAG = "_gol_texture_decoder_precision"

# (mode, Ci, Co, Hi, Wi) of the layer INPUT -> True, for precision="bf16x3": shapes where gol_upconvx_* (pack + forward + all
# gradients) won tools/texdecx_probe.py against what precision="fp32" runs for that shape (the library lines for the five
# small layers, gol_upconv_* for 32 -> 16) by more than both sides' spread (profiles/texdecx_probe.json, "dispatch"; DESIGN.md
# section 6c-sexies), B = 1, MI355X, and nothing else.  Forward + backward medians in ms, split operator against the other side
# (and the two spreads).  Not admitted: 128->256 @ 32^2 and 256->128 @ 64^2 (launch-bound: 0.27 against 0.21, 0.42 against
# 0.41 in mode 0); 128->128 @ 128^2 (ahead on the medians, 0.584 against 0.676 and 0.668 against 0.726, but a disturbed round
# put the library's spread above 1 ms in the committed run); 64->32 @ 512^2 in mode 1 (a tie, 2.054 against 2.057); 32->16 @
# 1024^2 (3.72 against the fp32 operator's 2.88: the input and weight gradients run at 27 and 24 TF with 16 output channels).
DISPATCH_BF16X3 = {
    (0, 128, 64, 256, 256): True,    # 1.145 ms against 1.429 (0.119, 0.134)
    (0, 64, 32, 512, 512): True,     # 1.823 ms against 2.028 (0.089, 0.034)
    (1, 128, 64, 256, 256): True,    # 1.361 ms against 1.499 (0.009, 0.011)
}


def supported(Ci, Co, Hi, Wi):
    """Shapes the kernels take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    return Ci > 0 and Co > 0 and Hi > 0 and Wi > 0 and Ci % 8 == 0 and (Co % 16 == 0 or Co <= 4)


def supported_bf16x3(Ci, Co, Hi, Wi):
    """Shapes gol_upconvx_* take (the ABI answers GOL_ERR_UNSUPPORTED otherwise): six of the seven layers; not 16 -> 4."""
    return Ci > 0 and Co > 0 and Hi > 0 and Wi > 0 and Ci % 32 == 0 and Co % 16 == 0


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


def _p(t, name="tensor"):
    return ctypes.c_void_p(t) if t is None or isinstance(t, int) else fptr(t, name)


def _sp(t, name="tensor"):
    return ctypes.c_void_p(t) if t is None or isinstance(t, int) else _lib.ptr(t, torch.int16, name)


# the marshallers: the parameters of include/goliath_hip.h by name (tests/test_upconvx_cpu.py holds them to the header)
def _abi_upconvx_pack(*, Co, Ci, weight, packed):
    _lib.call("gol_upconvx_pack", c_int(Co), c_int(Ci), _p(weight, "weight"), _sp(packed, "packed"), stream_ptr())


def _abi_upconvx_fwd(*, B, Ci, Co, Hi, Wi, mode, leak, scale, x, packed, bias, gate, gb, y):
    _lib.call("gol_upconvx_fwd", c_int(B), c_int(Ci), c_int(Co), c_int(Hi), c_int(Wi), c_int(mode), c_float(leak),
              c_float(scale), _p(x, "x"), _sp(packed, "packed"), _p(bias, "bias"), _p(gate, "gate"), _p(gb, "gb"), _p(y, "y"),
              stream_ptr())


def _abi_upconvx_bwd_x(*, B, Ci, Co, Hi, Wi, mode, leak, scale, packed, y, gate, g_y, g_x):
    _lib.call("gol_upconvx_bwd_x", c_int(B), c_int(Ci), c_int(Co), c_int(Hi), c_int(Wi), c_int(mode), c_float(leak),
              c_float(scale), _sp(packed, "packed"), _p(y, "y"), _p(gate, "gate"), _p(g_y, "g_y"), _p(g_x), stream_ptr())


def _abi_upconvx_bwd_w(*, B, Ci, Co, Hi, Wi, mode, leak, scale, x, y, gate, g_y, g_w, scratch):
    _lib.call("gol_upconvx_bwd_w", c_int(B), c_int(Ci), c_int(Co), c_int(Hi), c_int(Wi), c_int(mode), c_float(leak),
              c_float(scale), _p(x, "x"), _p(y, "y"), _p(gate, "gate"), _p(g_y, "g_y"), _p(g_w), _p(scratch), stream_ptr())


def _abi_upconvx_bwd_gate(*, B, Ci, Co, Hi, Wi, scale, x, packed, g_y, g_gate, g_gb):
    _lib.call("gol_upconvx_bwd_gate", c_int(B), c_int(Ci), c_int(Co), c_int(Hi), c_int(Wi), c_float(scale), _p(x, "x"),
              _sp(packed, "packed"), _p(g_y, "g_y"), _p(g_gate), _p(g_gb), stream_ptr())


def _abi_upconv_bwd(*, B, Ci, Co, Hi, Wi, mode, leak, scale, x, w_eff, y, gate, g_y, g_x, g_w, g_bias, g_gate, g_gb,
                    scratch):
    """gol_upconv_bwd by name: the split operator calls it for the gradients that hold no product (g_bias, g_gb alone)."""
    _lib.call("gol_upconv_bwd", c_int(B), c_int(Ci), c_int(Co), c_int(Hi), c_int(Wi), c_int(mode), c_float(leak),
              c_float(scale), _p(x, "x"), _p(w_eff, "w_eff"), _p(y, "y"), _p(gate, "gate"), _p(g_y, "g_y"), _p(g_x), _p(g_w),
              _p(g_bias), _p(g_gate), _p(g_gb), _p(scratch), stream_ptr())


def packed_elems_bf16x3(Co, Ci):
    """16-bit elements of gol_upconvx_pack's packed weight (a pure host call; 0 for unsupported channel counts)."""
    fn = _lib.load().gol_upconvx_packed_elems
    fn.restype = ctypes.c_longlong
    return int(fn(c_int(Co), c_int(Ci)))


def bwd_w_scratch_floats_bf16x3(B, Ci, Co, Hi, Wi):
    """Floats of scratch gol_upconvx_bwd_w needs (a pure host call; 0 for an unsupported shape)."""
    fn = _lib.load().gol_upconvx_bwd_w_scratch_floats
    fn.restype = ctypes.c_longlong
    return int(fn(c_int(B), c_int(Ci), c_int(Co), c_int(Hi), c_int(Wi)))


class _UpConvX(torch.autograd.Function):
    """include/goliath_hip.h: gol_upconvx_*.  mode 0: a = bias[Co,H,W], gb unused; mode 1: a = gate[B,Co,H,W], gb or None.
    Packs in forward; saves x (weight and gate gradients), the packed weight (input and gate gradients) and y (mode 0) or
    the gate (mode 1); backward launches, per needs_input_grad, only the kernels required."""

    @staticmethod
    def forward(ctx, x, weight, a, gb, mode, leak, scale):
        B, Ci, Hi, Wi = x.shape
        Co = weight.shape[0]
        dims = dict(B=B, Ci=Ci, Co=Co, Hi=Hi, Wi=Wi, mode=mode, leak=leak, scale=scale)
        packed = torch.empty(packed_elems_bf16x3(Co, Ci), device=x.device, dtype=torch.int16)
        y = torch.empty(B, Co, 2 * Hi, 2 * Wi, device=x.device)
        with _lib.device_guard(x.device):
            _abi_upconvx_pack(Co=Co, Ci=Ci, weight=weight, packed=packed)
            _abi_upconvx_fwd(**dims, x=x, packed=packed, bias=a if mode == 0 else None, gate=a if mode == 1 else None,
                             gb=gb, y=y)
        need_x, need_w, need_a = ctx.needs_input_grad[:3]
        need_gate = need_a and mode == 1
        ctx.save_for_backward(x if need_w or need_gate else None, packed if need_x or need_gate else None,
                              y if mode == 0 else a)
        ctx.dims = dims
        return y

    @staticmethod
    def backward(ctx, g):
        x, packed, aux = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        d = ctx.dims
        B, Ci, Co, Hi, Wi, mode = (d[k] for k in ("B", "Ci", "Co", "Hi", "Wi", "mode"))
        need_x, need_w, need_a, need_gb = ctx.needs_input_grad[:4]
        need_gb = need_gb and mode == 1
        g_x = g_w = g_a = g_gb = None
        new = lambda *shape: torch.empty(*shape, device=g.device)
        y, gate = (aux, None) if mode == 0 else (None, aux)
        stream = dict(x=None, w_eff=None, y=y, gate=gate, g_y=g, g_x=None, g_w=None, g_bias=None, g_gate=None, g_gb=None,
                      scratch=None)
        with _lib.device_guard(g.device):
            if need_x:
                g_x = new(B, Ci, Hi, Wi)
                _abi_upconvx_bwd_x(**d, packed=packed, y=y, gate=gate, g_y=g, g_x=g_x)
            if need_w:
                g_w = new(Co, Ci, 3, 3)
                # per-workgroup partial sums, added in a fixed order by a second kernel: no float atomics
                scratch = new(bwd_w_scratch_floats_bf16x3(B, Ci, Co, Hi, Wi))
                _abi_upconvx_bwd_w(**d, x=x, y=y, gate=gate, g_y=g, g_w=g_w, scratch=scratch)
            if need_a and mode == 0:      # no product in it: the fp32 operator's streaming pass
                g_a = new(Co, 2 * Hi, 2 * Wi)
                _abi_upconv_bwd(**d, **dict(stream, g_bias=g_a))
            elif need_a:                  # the gate gradient is the forward again; g_gb rides along
                g_a = torch.empty_like(g)
                g_gb = torch.empty_like(g) if need_gb else None
                _abi_upconvx_bwd_gate(B=B, Ci=Ci, Co=Co, Hi=Hi, Wi=Wi, scale=d["scale"], x=x, packed=packed, g_y=g,
                                      g_gate=g_a, g_gb=g_gb)
            elif need_gb:
                g_gb = torch.empty_like(g)
                _abi_upconv_bwd(**d, **dict(stream, g_gb=g_gb))
        return g_x, g_w, g_a, g_gb, None, None, None


def _check_bf16x3(name, x, weight):
    Co, Ci = weight.shape[:2]
    if not supported_bf16x3(Ci, Co, x.shape[2], x.shape[3]) or x.shape[0] > 65535:
        raise _lib.GoliathHipError(f"{name}: unsupported shape at precision 'bf16x3': x {tuple(x.shape)}, weight "
                                   f"{tuple(weight.shape)}: Ci must be a multiple of 32, Co of 16, B <= 65535")


def upconv_lrelu(x, weight, bias, leak=0.2, precision="fp32"):
    """x[B,Ci,Hi,Wi], weight[Co,Ci,3,3] (effective), bias[Co,2Hi,2Wi] ->
    lrelu(conv(bilinear 2x (x), weight, s1 p1) + bias)[B,Co,2Hi,2Wi].  HIP kernels; no CPU path.  precision="bf16x3":
    the split-bf16 operator (gol_upconvx_*; a shape `supported_bf16x3` admits, leak > 0), with gradients to x, weight and
    bias, whichever are required."""
    split = _precision(precision) == "bf16x3"
    if not (x.is_cuda and weight.is_cuda and bias.is_cuda):
        raise _lib.GoliathHipError("upconv_lrelu needs CUDA(HIP) tensors; there is no CPU path")
    out = _check("upconv_lrelu", x, weight)
    if tuple(bias.shape) != out[1:]:
        raise _lib.GoliathHipError(f"upconv_lrelu: bias {tuple(bias.shape)} for an output {out}")
    if split:
        _check_bf16x3("upconv_lrelu", x, weight)
        if not leak > 0:
            raise _lib.GoliathHipError(f"upconv_lrelu: leak must be positive, got {leak}")
        return _UpConvX.apply(_f32(x), _f32(weight), _f32(bias), None, 0, float(leak), 1.0)
    return _UpConv.apply(_f32(x), _f32(weight), _f32(bias), None, 0, float(leak), 1.0)


def upconv_gated(x, weight, gate, gb=None, scale=GAIN_SCALE, precision="fp32"):
    """x[B,Ci,Hi,Wi], weight[Co,Ci,3,3] (effective), gate[B,Co,2Hi,2Wi], gb (broadcastable to the gate's shape) or None ->
    (conv(bilinear 2x (x), weight, s1 p1) * gate + gb) * scale.  HIP kernels; no CPU path.  precision="bf16x3": the
    split-bf16 operator (gol_upconvx_*; a shape `supported_bf16x3` admits), with gradients to x, weight, gate and gb,
    whichever are required."""
    split = _precision(precision) == "bf16x3"
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
    if split:
        _check_bf16x3("upconv_gated", x, weight)
        return _UpConvX.apply(_f32(x), _f32(weight), _f32(gate), gb, 1, 1.0, float(scale))
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


def _rule_axis(n, device):
    """The integer-ratio rule along one axis of n source texels: (r0, r1, frac) of the 2 n rows of U, frac in float32 as the
    kernels form it (include/goliath_hip.h: gol_upconv_*)."""
    r = torch.arange(2 * n, device=device)
    nr, d = r * (n - 1), 2 * n - 1
    q = nr // d
    return q, (q + 1).clamp(max=n - 1), (nr - q * d).to(torch.float32) / float(d)


def up2_rule(x):
    """U = bilinear 2x of x[B,C,Hi,Wi] by the integer-ratio rule, in x's dtype, by the kernels' blend expression
    (1 - fr) ((1 - fc) x00 + fc x01) + fr ((1 - fc) x10 + fc x11)."""
    r0, r1, fr = _rule_axis(x.shape[2], x.device)
    c0, c1, fc = _rule_axis(x.shape[3], x.device)
    fr, fc = fr.to(x.dtype)[:, None], fc.to(x.dtype)[None, :]
    top, bot = x[:, :, r0], x[:, :, r1]
    return (1 - fr) * ((1 - fc) * top[..., c0] + fc * top[..., c1]) + fr * ((1 - fc) * bot[..., c0] + fc * bot[..., c1])


def _rule_matrix(n, device, dtype):
    """[2 n, n]: row r holds 1 - frac at r0 and frac at r1 (formed in float32, as the gather of gol_upconvx_bwd_x)."""
    q0, q1, f = _rule_axis(n, device)
    m = torch.zeros(2 * n, n, device=device, dtype=dtype)
    rows = torch.arange(2 * n, device=device)
    m.index_put_((rows, q0), (1 - f).to(dtype), accumulate=True)
    m.index_put_((rows, q1), f.to(dtype), accumulate=True)
    return m


class _SplitUpConv(torch.autograd.Function):
    """upconv_*_split_torch: the forward and every gradient of gol_upconvx_* in `acc_dtype`, each convolution a split product.
    U is blended in float32 and THEN split; g_pre is formed in float32 from the upstream gradient and the sign of y (mode 0)
    or the gate (mode 1) and THEN split; the bilinear adjoint and the epilogues run in `acc_dtype`."""

    @staticmethod
    def forward(ctx, x, weight, a, gb, mode, leak, scale, acc_dtype, y_sign):
        U = up2_rule(x.to(torch.float32))
        acc = _three(lambda u, w: F.conv2d(u, w, None, 1, 1), U, weight, acc_dtype)
        if mode == 0:
            pre = acc + a.to(acc_dtype)[None]
            y = torch.where(pre > 0, pre, leak * pre)
            aux = (y > 0) if y_sign is None else y_sign
        else:
            y = acc * a.to(acc_dtype)
            if gb is not None:
                y = y + gb.to(acc_dtype)
            y = y * scale
            aux = a.to(torch.float32)
        ctx.save_for_backward(U, weight, aux, acc if mode == 1 else None)
        ctx.mode, ctx.leak, ctx.scale, ctx.acc_dtype = mode, leak, scale, acc_dtype
        ctx.dtypes = (x.dtype, weight.dtype, a.dtype, None if gb is None else gb.dtype)
        return y

    @staticmethod
    def backward(ctx, g):
        U, weight, aux, acc = ctx.saved_tensors
        g = g.to(torch.float32)
        # float32, as the kernels form it
        g_pre = torch.where(aux, g, ctx.leak * g) if ctx.mode == 0 else (ctx.scale * g) * aux
        need_x, need_w, need_a, need_gb = ctx.needs_input_grad[:4]
        tx, tw, ta, tgb = ctx.dtypes
        g_x = g_w = g_a = g_gb = None
        if need_x:
            g_U = _three(lambda v, w: F.conv_transpose2d(v, w, None, 1, 1), g_pre, weight, ctx.acc_dtype)
            R = _rule_matrix(U.shape[2] // 2, U.device, ctx.acc_dtype)
            C = _rule_matrix(U.shape[3] // 2, U.device, ctx.acc_dtype)
            g_x = torch.einsum("ri,bkrc,cj->bkij", R, g_U, C).to(tx)
        if need_w:
            g_w = _three(lambda v, u: torch.nn.grad.conv2d_weight(u, weight.shape, v, 1, 1), g_pre, U, ctx.acc_dtype).to(tw)
        if need_a:
            g_a = (g_pre.to(ctx.acc_dtype).sum(0) if ctx.mode == 0 else (ctx.scale * g).to(ctx.acc_dtype) * acc).to(ta)
        if need_gb and ctx.mode == 1:
            g_gb = (ctx.scale * g).to(tgb)
        return g_x, g_w, g_a, g_gb, None, None, None, None, None


def upconv_lrelu_split_torch(x, weight, bias, leak=0.2, acc_dtype=torch.float64, *, y_sign=None):
    """`upconv_lrelu(..., precision="bf16x3")` in plain PyTorch, on any device: U is formed in float32 by the integer-ratio
    rule's expression (`up2_rule`), U and weight (taken as float32) are split by `perceptual.split_bf16` and the three
    products lo hi, hi lo, hi hi are three F.conv2d accumulated in `acc_dtype`; bias and leak follow in `acc_dtype`.  Its
    backward forms g_pre = y > 0 ? g : leak g in float32, splits it the same way and forms g_U (transposed convolution) and
    g_w (correlation of g_pre with U) as three products each, g_x as the bilinear adjoint of g_U and g_bias as the batch sum,
    in `acc_dtype`.  y_sign (a bool tensor of y's shape) replaces y > 0 in the backward: a parity test hands over the
    operator's own sign, so that a `pre` that rounds across zero is not counted against the gradients.  Returns `acc_dtype`;
    gradients come back in the inputs' dtypes."""
    out = _check("upconv_lrelu_split_torch", x, weight)
    if tuple(bias.shape) != out[1:]:
        raise _lib.GoliathHipError(f"upconv_lrelu_split_torch: bias {tuple(bias.shape)} for an output {out}")
    return _SplitUpConv.apply(x, weight, bias, None, 0, float(leak), 1.0, acc_dtype, y_sign)


def upconv_gated_split_torch(x, weight, gate, gb=None, scale=GAIN_SCALE, acc_dtype=torch.float64):
    """`upconv_gated(..., precision="bf16x3")` in plain PyTorch, on any device: the split products of
    `upconv_lrelu_split_torch`, then (acc gate + gb) scale in `acc_dtype`.  Its backward forms g_pre = (scale g) gate in
    float32 and THEN splits it; g_gate = (scale g) acc and g_gb = scale g.  Returns `acc_dtype`; gradients come back in the
    inputs' dtypes."""
    out = _check("upconv_gated_split_torch", x, weight)
    if tuple(gate.shape) != out:
        raise _lib.GoliathHipError(f"upconv_gated_split_torch: gate {tuple(gate.shape)} for an output {out}")
    if gb is not None:
        gb = gb.expand(out)
    return _SplitUpConv.apply(x, weight, gate, gb, 1, 1.0, float(scale), acc_dtype, None)


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


def _takes_split(mode, layer, x, hh, *others):
    """`_takes_hip` for precision="bf16x3": the same conditions on the layer and the tensors, with `supported_bf16x3` and
    `DISPATCH_BF16X3` as the shape rule and the table."""
    if not (x.dim() == 4 and _on_gpu(x, layer.weight_v, layer.bias, *others)):
        return False
    Co, Ci = layer.weight_v.shape[:2]
    Hi, Wi = x.shape[2:]
    if x.shape[1] != Ci or (2 * Hi, 2 * Wi) != (hh, hh) or not supported_bf16x3(Ci, Co, Hi, Wi) or x.shape[0] > 65535:
        return False
    if mode == 0 and tuple(layer.bias.shape) != (Co, hh, hh):
        return False
    if mode == 1 and tuple(others[0].shape) != (x.shape[0], Co, hh, hh):
        return False
    return os.environ.get("GOLIATH_FUSED_TEXDEC_ALL", "0") == "1" or DISPATCH_BF16X3.get((mode, Ci, Co, Hi, Wi), False)


def texture_branches(decoder, joint_feat, z, gainbias, first_size=64, precision="fp32"):
    """The two loops of `ConvTeacherDecoder.forward` (urhand.py:583-608; goliath_amd/urhand.py): the non-linear branch on
    `joint_feat`, then the linear branch on `z` gated by the first one's activations.  Returns x before the final resize to
    uv_size.  A layer goes to `upconv_lrelu` / `upconv_gated` only if it is a weight-normalised 3x3 / s1 / p1 layer (untied
    3-D bias in texmod0, no bias in texmod1), the tensors are on the GPU, its input is exactly (hh/2, hh/2) and the shape
    passes `supported` and `DISPATCH` (or GOLIATH_FUSED_TEXDEC_ALL=1); otherwise the reference's three lines run unchanged.
    `first_size` is the output size of the first layer: 64 in the model (urhand.py:591,599); tests run smaller stacks.
    precision="bf16x3": a recognised layer whose shape passes `supported_bf16x3` and `DISPATCH_BF16X3` (or
    GOLIATH_FUSED_TEXDEC_ALL=1) goes to the split-bf16 operator instead; every other layer takes exactly the decision
    above.  At "fp32" (the default) nothing but the lines above runs."""
    split = _precision(precision) == "bf16x3"
    acts, x, hh = [], joint_feat, first_size
    for i in range(decoder.n_layers_tex):                # non-linear branch
        layer = decoder.texmod0[i]
        if split and _is_conv3_wn(layer, True) and _takes_split(0, layer, x, hh):
            x = upconv_lrelu(x, wn_weight(layer), layer.bias, 0.2, precision="bf16x3")
        elif _is_conv3_wn(layer, True) and _takes_hip(0, layer, x, hh):
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
        if split and _is_conv3_wn(layer, False) and _takes_split(1, layer, x, hh, acts[i], gb):
            x = upconv_gated(x, wn_weight(layer), acts[i], gb, GAIN_SCALE if gb is not None else 1.0, precision="bf16x3")
            hh *= 2
        elif _is_conv3_wn(layer, False) and _takes_hip(1, layer, x, hh, acts[i], gb):
            x = upconv_gated(x, wn_weight(layer), acts[i], gb, GAIN_SCALE if gb is not None else 1.0)
            hh *= 2
        else:
            x = F.interpolate(x, (hh, hh), mode="bilinear", align_corners=True)
            x = layer(x) * acts[i]
            hh *= 2
            if gb is not None:
                x = (x + gb) * 0.707107
    return x
