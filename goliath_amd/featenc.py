"""URHand's FeatEncoderUNet: its 7x7 projection and first 4x4 / stride 2 feature layer as one fused operator.

`FeatEncoderUNet.forward` (ca_code/models/urhand.py:98-107, built at :82-96 and :302, called at :585 on
`feat_p.detach()`) starts with `proj` = Conv2dWN(Cx -> 64, 7, 1, 3, bias=False) and `feat_mod[0]` = Conv2dWN(64 -> 192, 4,
2, 1, bias=False) with nothing between them (la.Conv2dWN, ca_code/nn/layers.py:470): at the model's size (uv 1024^2, 1
diffuse + 3 specular channels) the 64-channel tensor between the two is 268 MB per view, written, read once, kept for the
weight gradient, and its gradient is a second tensor of that size.  `front` runs the pair as ONE HIP kernel forward
(gol_featenc_front_fwd: per 8x8 output tile the 18x18 region of the intermediate is recomputed on chip in K stages of 16
channels, fp32-MFMA in both GEMMs, nothing but y written) and two weight-gradient kernels backward (gol_featenc_front_bwd:
the intermediate and its gradient recomputed per tile, fixed-order reduction, no float atomics).  There is NO input
gradient: the model feeds a detached tensor, and `front` refuses an input that requires one.  `front_torch` is the same
composition in plain PyTorch (any device, any dtype: the float64 twin).

The weight norm stays torch algebra on the small tensors (`tail.wn_weight`), so gradients reach weight_v / weight_g
through the ordinary graph and the kernels see the effective weights.

`forward` mirrors FeatEncoderUNet.forward and takes the operator where the two layers are of the expected kind and
(Cx, Cm, Co, H, W) is in `DISPATCH` -- the result of tools/featenc_probe.py, by the rule of
section 6a: a shape is admitted only where the HIP operator's forward + backward beat the library composition by more
than the composition's own run-to-run spread.  GOLIATH_FUSED_FEATENC_ALL=1 forces the operator for every supported shape
(tests, probes).  `gb_mod[0]` and every later layer run on the library, on the operator's y.

`precision="bf16x3"` (opt-in; the default everywhere is "fp32") sends the four bias-free 4x4 / stride 2 / pad 1 feature
layers `feat_mod[0..3]` (urhand.py:93, :102) to `conv4s2`: the split-bf16 product of `perceptual` (every operand written
as two bf16 values, three bf16 MFMAs summed in fp32) with ALL THREE directions, forward, input gradient and weight gradient
(gol_conv4x_pack / _fwd / _bwd_x / _bwd_w).  `conv4s2_split_torch` is that arithmetic in plain
PyTorch.  A layer goes to the operator where its (Ci, Co, H, W) is in `DISPATCH_BF16X3` -- the result of
tools/conv4x_probe.py -- or with GOLIATH_FUSED_FEATENC_ALL=1; any other layer runs the reference's line, as does every layer
at "fp32".  `proj`, `gb_mod[*]` and `enc` stay on the library.  The fused front keeps its own table and ignores `precision`.
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_int, fptr, stream_ptr
from .decoder import _glorot_, _wn
from .perceptual import _precision, split_bf16
from .tail import wn_weight

# class attribute dropin.patch_urhand(feat_encoder=True) sets on the decoder class: its forward calls `forward` here
FEATENC_FLAG = "_gol_feat_encoder"
# stored next to it by dropin.patch_urhand(feat_encoder_precision=...): the `precision` goliath_amd.urhand passes to `forward`
FEATENC_PRECISION_FLAG = "_gol_feat_encoder_precision"

# (Cx, Cm, Co, H, W) of the input -> True: shapes where the HIP operator won the probe (B = 1, MI355X).  From
# profiles/featenc_probe.json ("dispatch"; forward + backward medians in ms, HIP against the two library convolutions and
# their autograd backward, and the library's spread).  Shapes that are not listed stay on the library lines inside
# `forward`.  EMPTY as measured: the model's shape (4, 64, 192, 1024, 1024) loses, 8.551 ms against 4.067 (library spread
# 0.243) -- the forward ties (1.493 against 1.498) and a forward + backward peaks at 242 MB instead of 1210, but the two
# weight-gradient kernels take 7.1 ms against the library's 2.6 (the measured table is in DESIGN.md section 6c-ter).
DISPATCH = {
}


# (Ci, Co, H, W) of a feat_mod layer's INPUT -> True, for precision="bf16x3": shapes where gol_conv4x_* (pack + forward +
# both gradients) won tools/conv4x_probe.py against F.conv2d and its autograd backward in fp32 by more than the library's
# spread (profiles/conv4x_probe.json, "dispatch"), B = 1 on the MI355X, and nothing else.
# Forward + backward (to x and w, pack included) medians in ms, split operator against the library (and the library's spread):
DISPATCH_BF16X3 = {
    (64, 192, 1024, 1024): True,    # feat_mod[0]: 2.928 against 3.123 (0.090)
    (192, 384, 512, 512): True,     # feat_mod[1]: 3.740 against 4.265 (0.114)
    (384, 384, 256, 256): True,     # feat_mod[2]: 1.923 against 2.212 (0.051)
    (384, 768, 128, 128): True,     # feat_mod[3]: 1.113 against 1.143 (0.014)
}


def supported(Cx, Cm, Co, H, W):
    """Shapes the kernels take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    return (1 <= Cx <= 8 and Cm > 0 and Cm % 16 == 0 and Co > 0 and Co % 16 == 0 and H >= 2 and W >= 2
            and H % 2 == 0 and W % 2 == 0)


def _p(t, name="tensor"):
    return ctypes.c_void_p(t) if t is None or isinstance(t, int) else fptr(t, name)


# the marshallers: the parameters of include/goliath_hip.h by name (tests/test_featenc_cpu.py holds them to the header)
def _abi_featenc_front_fwd(*, B, Cx, Cm, Co, H, W, x, w_p, w_f, y):
    _lib.call("gol_featenc_front_fwd", c_int(B), c_int(Cx), c_int(Cm), c_int(Co), c_int(H), c_int(W), _p(x, "x"),
              _p(w_p, "w_proj"), _p(w_f, "w_feat"), _p(y, "y"), stream_ptr())


def _abi_featenc_front_bwd(*, B, Cx, Cm, Co, H, W, x, w_p, w_f, g_y, g_w_p, g_w_f, scratch):
    _lib.call("gol_featenc_front_bwd", c_int(B), c_int(Cx), c_int(Cm), c_int(Co), c_int(H), c_int(W), _p(x, "x"),
              _p(w_p, "w_proj"), _p(w_f, "w_feat"), _p(g_y, "g_y"), _p(g_w_p), _p(g_w_f), _p(scratch), stream_ptr())


def bwd_scratch_floats(B, Cx, Cm, Co, H, W):
    """Floats of scratch the backward needs (a pure host call; 0 for an unsupported shape)."""
    fn = _lib.load().gol_featenc_front_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    return int(fn(c_int(B), c_int(Cx), c_int(Cm), c_int(Co), c_int(H), c_int(W)))


class _Front(torch.autograd.Function):
    """y[B,Co,H/2,W/2] = conv4s2(conv7(x, w_proj), w_feat)  (include/goliath_hip.h: gol_featenc_front_*)."""

    @staticmethod
    def forward(ctx, x, w_proj, w_feat):
        B, Cx, H, W = x.shape
        Cm, Co = w_proj.shape[0], w_feat.shape[0]
        y = torch.empty(B, Co, H // 2, W // 2, device=x.device)
        dims = dict(B=B, Cx=Cx, Cm=Cm, Co=Co, H=H, W=W)
        with _lib.device_guard(x.device):
            _abi_featenc_front_fwd(**dims, x=x, w_p=w_proj, w_f=w_feat, y=y)
        ctx.save_for_backward(x, w_proj, w_feat)
        ctx.dims = dims
        return y

    @staticmethod
    def backward(ctx, g):
        x, w_proj, w_feat = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        _, need_p, need_f = ctx.needs_input_grad
        g_p = torch.empty_like(w_proj) if need_p else None
        g_f = torch.empty_like(w_feat) if need_f else None
        # per-workgroup partial sums of the weight gradients (reduced by a second kernel: no float atomics)
        scratch = torch.empty(bwd_scratch_floats(**ctx.dims), device=x.device)
        with _lib.device_guard(x.device):
            _abi_featenc_front_bwd(**ctx.dims, x=x, w_p=w_proj, w_f=w_feat, g_y=g, g_w_p=g_p, g_w_f=g_f, scratch=scratch)
        return None, g_p, g_f


def _f32(t):
    return t.to(torch.float32).contiguous()


def _shapes(x, w_proj, w_feat):
    """(Cx, Cm, Co, H, W) of a call, or an error naming what does not fit."""
    if x.dim() != 4 or w_proj.dim() != 4 or w_feat.dim() != 4:
        raise _lib.GoliathHipError(f"featenc.front: shapes {tuple(x.shape)}, {tuple(w_proj.shape)}, {tuple(w_feat.shape)}")
    _, Cx, H, W = x.shape
    Cm, Co = w_proj.shape[0], w_feat.shape[0]
    if tuple(w_proj.shape) != (Cm, Cx, 7, 7):
        raise _lib.GoliathHipError(f"featenc.front: w_proj {tuple(w_proj.shape)} for {Cx} input channels and a 7x7 kernel")
    if tuple(w_feat.shape) != (Co, Cm, 4, 4):
        raise _lib.GoliathHipError(f"featenc.front: w_feat {tuple(w_feat.shape)} for {Cm} channels and a 4x4 kernel")
    return Cx, Cm, Co, H, W


def front(x, w_proj, w_feat):
    """x[B,Cx,H,W] (no gradient), w_proj[Cm,Cx,7,7], w_feat[Co,Cm,4,4] (both effective) ->
    conv(conv(x, w_proj, s1 p3), w_feat, s2 p1)[B,Co,H/2,W/2].  HIP kernels; no CPU path; no input gradient."""
    if x.requires_grad:
        raise _lib.GoliathHipError("featenc.front has no input gradient: x must not require grad (the model passes "
                                   "feat_p.detach())")
    dims = _shapes(x, w_proj, w_feat)
    if not supported(*dims):
        raise _lib.GoliathHipError("featenc.front: unsupported shape (Cx, Cm, Co, H, W) = %s: Cx must be 1..8, Cm and Co "
                                   "multiples of 16, H and W even" % (dims,))
    if x.shape[0] > 65535:
        raise _lib.GoliathHipError(f"featenc.front: unsupported batch {x.shape[0]} > 65535")
    if not (x.is_cuda and w_proj.is_cuda and w_feat.is_cuda):
        raise _lib.GoliathHipError("featenc.front needs CUDA(HIP) tensors; there is no CPU path")
    return _Front.apply(_f32(x), _f32(w_proj), _f32(w_feat))


def front_torch(x, w_proj, w_feat):
    """The same composition in plain PyTorch (urhand.py:100-102 on the effective weights): parity twin, runs on the CPU and
    in float64."""
    return F.conv2d(F.conv2d(x, w_proj, None, 1, 3), w_feat, None, 2, 1)


# ---- the 4x4 / stride 2 / pad 1 layer at precision "bf16x3" ---------------------------------------------------------------
def conv4_supported(Ci, Co, H, W):
    """Shapes gol_conv4x_* take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    return Ci > 0 and Co > 0 and Ci % 32 == 0 and Co % 32 == 0 and H >= 2 and W >= 2 and H % 2 == 0 and W % 2 == 0


def _sp(t, name="tensor"):
    return ctypes.c_void_p(t) if t is None or isinstance(t, int) else _lib.ptr(t, torch.int16, name)


def _abi_conv4x_pack(*, Co, Ci, weight, packed):
    _lib.call("gol_conv4x_pack", c_int(Co), c_int(Ci), _p(weight, "weight"), _sp(packed, "packed"), stream_ptr())


def _abi_conv4x_fwd(*, B, Ci, Co, H, W, x, packed, y):
    _lib.call("gol_conv4x_fwd", c_int(B), c_int(Ci), c_int(Co), c_int(H), c_int(W), _p(x, "x"), _sp(packed, "packed"),
              _p(y, "y"), stream_ptr())


def _abi_conv4x_bwd_x(*, B, Ci, Co, H, W, packed, g_y, g_x):
    _lib.call("gol_conv4x_bwd_x", c_int(B), c_int(Ci), c_int(Co), c_int(H), c_int(W), _sp(packed, "packed"),
              _p(g_y, "g_y"), _p(g_x), stream_ptr())


def _abi_conv4x_bwd_w(*, B, Ci, Co, H, W, x, g_y, g_w, scratch):
    _lib.call("gol_conv4x_bwd_w", c_int(B), c_int(Ci), c_int(Co), c_int(H), c_int(W), _p(x, "x"), _p(g_y, "g_y"),
              _p(g_w), _p(scratch), stream_ptr())


def conv4x_packed_elems(Co, Ci):
    """16-bit elements of the packed weight (a pure host call; 0 for unsupported channel counts)."""
    fn = _lib.load().gol_conv4x_packed_elems
    fn.restype = ctypes.c_longlong
    return int(fn(c_int(Co), c_int(Ci)))


def conv4x_bwd_w_scratch_floats(B, Ci, Co, H, W):
    """Floats of scratch the weight gradient needs (a pure host call; 0 for an unsupported shape)."""
    fn = _lib.load().gol_conv4x_bwd_w_scratch_floats
    fn.restype = ctypes.c_longlong
    return int(fn(c_int(B), c_int(Ci), c_int(Co), c_int(H), c_int(W)))


class _Conv4x(torch.autograd.Function):
    """include/goliath_hip.h: gol_conv4x_pack / _fwd / _bwd_x / _bwd_w.  Packs in forward; saves x and the packed weight."""

    @staticmethod
    def forward(ctx, x, weight):
        B, Ci, H, W = x.shape
        Co = weight.shape[0]
        dims = dict(B=B, Ci=Ci, Co=Co, H=H, W=W)
        packed = torch.empty(conv4x_packed_elems(Co, Ci), device=x.device, dtype=torch.int16)
        y = torch.empty(B, Co, H // 2, W // 2, device=x.device)
        with _lib.device_guard(x.device):
            _abi_conv4x_pack(Co=Co, Ci=Ci, weight=weight, packed=packed)
            _abi_conv4x_fwd(**dims, x=x, packed=packed, y=y)
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, packed if ctx.needs_input_grad[0] else None)
        ctx.dims = dims
        return y

    @staticmethod
    def backward(ctx, g):
        x, packed = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        d = ctx.dims
        need_x, need_w = ctx.needs_input_grad
        g_x = g_w = None
        with _lib.device_guard(g.device):
            if need_x:
                g_x = torch.empty(d["B"], d["Ci"], d["H"], d["W"], device=g.device)
                _abi_conv4x_bwd_x(**d, packed=packed, g_y=g, g_x=g_x)
            if need_w:
                g_w = torch.empty(d["Co"], d["Ci"], 4, 4, device=g.device)
                # per-workgroup partial sums, added in a fixed order by a second kernel: no float atomics
                scratch = torch.empty(conv4x_bwd_w_scratch_floats(**d), device=g.device)
                _abi_conv4x_bwd_w(**d, x=x, g_y=g, g_w=g_w, scratch=scratch)
        return g_x, g_w


def _conv4_shapes(name, x, weight):
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape) != (weight.shape[0], x.shape[1], 4, 4):
        raise _lib.GoliathHipError(f"{name}: shapes {tuple(x.shape)}, {tuple(weight.shape)} (x[B,Ci,H,W], weight[Co,Ci,4,4])")
    return x.shape[1], weight.shape[0], x.shape[2], x.shape[3]


def conv4s2(x, weight, precision="bf16x3"):
    """x[B,Ci,H,W], weight[Co,Ci,4,4] (effective) -> conv2d(x, weight, None, 2, 1)[B,Co,H/2,W/2] at precision "bf16x3",
    with gradients to x and to weight (whichever is required).  fp32 CUDA(HIP) tensors, Ci and Co multiples of 32, H and W
    even, B <= 65535: anything else raises.  HIP kernels; no CPU path."""
    if _precision(precision) != "bf16x3":
        raise _lib.GoliathHipError("featenc.conv4s2 exists at precision='bf16x3' only (fp32 is F.conv2d)")
    dims = _conv4_shapes("featenc.conv4s2", x, weight)
    if not conv4_supported(*dims) or x.shape[0] > 65535:
        raise _lib.GoliathHipError("featenc.conv4s2: unsupported shape B = %d, (Ci, Co, H, W) = %s: Ci and Co must be "
                                   "multiples of 32, H and W even and >= 2, B <= 65535" % (x.shape[0], dims))
    if not (x.is_cuda and weight.is_cuda):
        raise _lib.GoliathHipError("featenc.conv4s2 needs CUDA(HIP) tensors; there is no CPU path")
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise _lib.GoliathHipError(f"featenc.conv4s2 takes float32 tensors, got {x.dtype} and {weight.dtype}")
    if x.shape[0] == 0:
        return F.conv2d(x, weight, None, 2, 1)
    return _Conv4x.apply(x.contiguous(), weight.contiguous())


def _three(op, a, b, dtype):
    """lo_a hi_b + hi_a lo_b + hi_a hi_b in `dtype` (every product of two bf16 values is exact in float32 already)."""
    (ah, al), (bh, bl) = ((h.to(dtype), l.to(dtype)) for h, l in (split_bf16(a), split_bf16(b)))
    return op(al, bh) + op(ah, bl) + op(ah, bh)


class _SplitConv4(torch.autograd.Function):
    """conv4s2_split_torch: the three directions of gol_conv4x_* in `acc_dtype`, every one a split product."""

    @staticmethod
    def forward(ctx, x, weight, acc_dtype):
        ctx.save_for_backward(x, weight)
        ctx.acc_dtype = acc_dtype
        return _three(lambda a, w: F.conv2d(a, w, None, 2, 1), x, weight, acc_dtype)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.to(torch.float32)
        g_x = g_w = None
        if ctx.needs_input_grad[0]:
            g_x = _three(lambda a, w: F.conv_transpose2d(a, w, None, 2, 1), g, weight, ctx.acc_dtype).to(x.dtype)
        if ctx.needs_input_grad[1]:
            g_w = _three(lambda a, v: torch.nn.grad.conv2d_weight(v, weight.shape, a, 2, 1), g, x,
                         ctx.acc_dtype).to(weight.dtype)
        return g_x, g_w, None


def conv4s2_split_torch(x, weight, acc_dtype=torch.float64):
    """`conv4s2` in plain PyTorch, on any device: x and weight (taken as float32) are split by `perceptual.split_bf16` and
    the three products lo hi, hi lo, hi hi are three F.conv2d accumulated in `acc_dtype`.  Its backward splits the upstream
    gradient (float32), the weight and x the same way and forms g_x (transposed convolution) and g_w (correlation of g with
    x) as three products each in `acc_dtype`.  Returns `acc_dtype`; gradients come back in the inputs' dtypes."""
    _conv4_shapes("featenc.conv4s2_split_torch", x, weight)
    return _SplitConv4.apply(x, weight, acc_dtype)


class ConvWN(nn.Module):
    """k x k conv, weight-normalised (direction normalised over the whole tensor, one magnitude per output channel), with a
    tied bias [C_out] or none: la.Conv2dWN(n_in, n_out, k, stride, pad, bias=...)."""

    def __init__(self, n_in, n_out, ksize, stride, pad, bias=True, alpha=1.0):
        super().__init__()
        self.ksize, self.stride, self.pad = ksize, stride, pad
        self.weight_v = nn.Parameter(torch.empty(n_out, n_in, ksize, ksize))
        _glorot_(self.weight_v, n_in, n_out, ksize * ksize, alpha)
        self.weight_g = nn.Parameter(torch.full((n_out, 1, 1, 1), float(self.weight_v.detach().norm())))
        if bias:
            self.bias = nn.Parameter(torch.zeros(n_out))
        else:
            self.register_parameter("bias", None)

    def weight(self):
        return _wn(self.weight_v, self.weight_g)

    def forward(self, x):
        return F.conv2d(x, self.weight(), self.bias, self.stride, self.pad)


def _is_conv_wn(m, ksize, stride, pad):
    """A weight-normalised k x k / stride / pad conv WITHOUT bias: this module's or the reference's layer (same parameter
    names).  Not a transposed conv, not another geometry, not a layer with a bias or without weight norm."""
    if isinstance(m, nn.ConvTranspose2d) or not all(hasattr(m, a) for a in ("weight_v", "weight_g")):
        return False
    if getattr(m, "bias", None) is not None:
        return False
    if m.weight_v.dim() != 4 or tuple(m.weight_v.shape[2:]) != (ksize, ksize) or \
            tuple(m.weight_g.shape) != (m.weight_v.shape[0], 1, 1, 1):
        return False
    if isinstance(m, ConvWN):
        return (m.ksize, m.stride, m.pad) == (ksize, stride, pad)
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    return (isinstance(m, nn.Conv2d) and pair(m.stride) == (stride, stride) and pair(m.padding) == (pad, pad)
            and pair(m.dilation) == (1, 1) and m.groups == 1 and m.padding_mode == "zeros")


def _admitted(dims):
    return supported(*dims) and (os.environ.get("GOLIATH_FUSED_FEATENC_ALL", "0") == "1" or DISPATCH.get(dims, False))


def _takes_operator(fe, x, op):
    """Whether `proj` + `feat_mod[0]` on x go to `op`: a 7/1/3 and a 4/2/1 weight-normalised conv without bias whose channel
    counts chain, an input that needs no gradient, a shape that passes `supported` and `DISPATCH` (or
    GOLIATH_FUSED_FEATENC_ALL=1) and, for the HIP operator, fp32 tensors on the GPU."""
    if not op or len(fe.feat_mod) < 1 or x.dim() != 4 or x.requires_grad:
        return False
    proj, feat = fe.proj, fe.feat_mod[0]
    if not (_is_conv_wn(proj, 7, 1, 3) and _is_conv_wn(feat, 4, 2, 1)):
        return False
    Cm, Cx = proj.weight_v.shape[:2]
    Co = feat.weight_v.shape[0]
    if x.shape[1] != Cx or feat.weight_v.shape[1] != Cm or x.shape[0] > 65535:
        return False
    if op is front and not all(t.is_cuda and t.dtype == torch.float32
                               for t in (x, proj.weight_v, proj.weight_g, feat.weight_v, feat.weight_g)):
        return False
    return bool(_admitted((Cx, Cm, Co, x.shape[2], x.shape[3])))


def _takes_conv4(layer, x, conv):
    """Whether `layer` on x goes to the split operator `conv`: a weight-normalised 4/2/1 conv without bias, a shape
    gol_conv4x_* supports and `DISPATCH_BF16X3` admits (or GOLIATH_FUSED_FEATENC_ALL=1) and, for the HIP operator, fp32
    tensors on the GPU."""
    if not conv or x.dim() != 4 or not _is_conv_wn(layer, 4, 2, 1):
        return False
    Co, Ci = layer.weight_v.shape[:2]
    if x.shape[1] != Ci or not 0 < x.shape[0] <= 65535:
        return False
    if conv is conv4s2 and not all(t.is_cuda and t.dtype == torch.float32 for t in (x, layer.weight_v, layer.weight_g)):
        return False
    dims = (Ci, Co, x.shape[2], x.shape[3])
    return conv4_supported(*dims) and (os.environ.get("GOLIATH_FUSED_FEATENC_ALL", "0") == "1"
                                       or DISPATCH_BF16X3.get(dims, False))


def forward(featenc, x, op=None, precision="fp32", conv=None):
    """FeatEncoderUNet.forward (urhand.py:98-107) -> (z, gb).  `proj` and `feat_mod[0]` go to `op` where `_takes_operator`
    admits them and run the reference's two lines otherwise; everything from `gb_mod[0]` on is the reference's.  op = None is
    the HIP operator `front`; `front_torch` routes the pair to the torch twin (any device, float64); False admits nothing
    (the library composition).  precision="bf16x3": every `feat_mod[i]` that `_takes_conv4` admits runs as
    conv(x, wn_weight(feat_mod[i])) -- conv = None is the HIP operator `conv4s2`, `conv4s2_split_torch` (or any callable of
    (x, weight)) the twin; a layer that is not admitted, and every layer at "fp32", runs the reference's line."""
    op = front if op is None else op
    conv = (conv4s2 if conv is None else conv) if _precision(precision) == "bf16x3" else False
    gb = []
    first = 0
    if _takes_operator(featenc, x, op):
        x = op(x, wn_weight(featenc.proj), wn_weight(featenc.feat_mod[0]))
        gb.insert(0, featenc.gb_mod[0](x))
        first = 1
    else:
        x = featenc.proj(x)
    for i in range(first, featenc.n_layers):
        if _takes_conv4(featenc.feat_mod[i], x, conv):
            x = conv(x, wn_weight(featenc.feat_mod[i]))
        else:
            x = featenc.feat_mod[i](x)
        b = featenc.gb_mod[i](x)
        gb.insert(0, b)
    z = featenc.enc(x)
    return z, gb


class FeatEncoderUNet(nn.Module):
    """Module twin of the reference's FeatEncoderUNet (urhand.py:82-107) under its state-dict names (proj.weight_{g,v},
    feat_mod.i.*, gb_mod.i.*, enc.{bias,weight_g,weight_v}): at base=64 a reference checkpoint loads.  `base` scales the
    channel list (64 in the reference; tests run a whole encoder at 16).  Its own forward is the library composition
    (`forward` of this module with the fused front not admitted); `precision` ("fp32" by default) is kept as an attribute
    and handed to `forward`: at "bf16x3" the admitted `feat_mod` layers run on `conv4s2`."""

    def __init__(self, n_diff_feat, n_spec_feat, out_ch, m=1, base=64, precision="fp32"):
        super().__init__()
        self.precision = _precision(precision)
        c = 3
        nfc = [base, base * c, 2 * base * c, 2 * base * c, 4 * base * c]
        nbc = [base, base * m, 2 * base * m, 2 * base * m, 4 * base * m]
        self.proj = ConvWN(n_diff_feat + n_spec_feat, base, 7, 1, 3, bias=False)
        self.feat_mod = nn.ModuleList(ConvWN(nfc[i], nfc[i + 1], 4, 2, 1, bias=False) for i in range(len(nfc) - 1))
        self.gb_mod = nn.ModuleList(ConvWN(nfc[i + 1], nbc[i + 1], 1, 1, 0, bias=False) for i in range(len(nfc) - 1))
        self.n_layers = len(nfc) - 1
        self.enc = ConvWN(4 * base * c, out_ch, 4, 2, 1)  # collapsed to one layer

    def forward(self, x):
        return forward(self, x, op=False, precision=self.precision)

    def forward_torch(self, x, precision=None, acc_dtype=torch.float64):
        """The twin of `forward`: at "bf16x3" the same `feat_mod` layers on `conv4s2_split_torch`, accumulated in
        `acc_dtype` and handed on in x's dtype (any device).  precision = None: the module's."""
        conv = lambda t, w: conv4s2_split_torch(t, w, acc_dtype).to(t.dtype)
        return forward(self, x, op=False, precision=self.precision if precision is None else precision, conv=conv)
