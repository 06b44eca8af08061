"""Hidden decoder layers as one fused operator (profiles/LOG.md open item 6).

Each of the twelve hidden layers of the two decoders is `ConvTranspose2dWNUB(Ci, Co, 4, 2, 1)` + an untied bias +
`LeakyReLU(0.2)` (/root/reference/ca_code/models/rgca.py:408-426,429-454; ca_code/nn/layers.py:331-397): a MIOpen
transposed convolution, an ATen add and an ATen leaky_relu forward, two MIOpen gradient convolutions, a batch
reduction and the activation's backward on the way back.  `convt_ub_lrelu` runs a layer as ONE HIP kernel forward
(gol_trunk_conv_fwd: fp32-MFMA implicit GEMM, bias and activation on the accumulators, nothing but y written) and
three backward (gol_trunk_conv_bwd: input, weight and bias gradient, the activation mask read from the sign of y,
no float atomics); `convt_ub_lrelu_torch` is the same composition in plain PyTorch (parity twin, runs on CPU).

The weight norm stays torch algebra on the small tensor (`tail.wn_weight`), so gradients reach weight_v / weight_g
through the ordinary graph and the kernels see the effective weight.

`run_stack` walks an `nn.Sequential` and takes the operator for the (layer, LeakyReLU) pairs whose shape is in
`DISPATCH` -- the per-shape result of tools/trunk_probe.py: a shape is admitted only where the
HIP operator's forward + backward beat the library composition by more than the composition's own run-to-run spread.
GOLIATH_FUSED_TRUNK_ALL=1 forces the operator for every supported shape (tests, probes).
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_float, c_int, fptr, stream_ptr
from .tail import wn_weight

# (Ci, Co, h, w) of the layer INPUT -> True: shapes where the HIP operator won the probe (B = 8, MI355X).
# From profiles/trunk_probe.json ("dispatch"); shapes that are not listed stay on the torch modules inside run_stack:
# 256->256 and 264->256 at 8^2, 256->128 at 16^2 and 128->128 at 32^2 lose (0.26-0.39 ms against 0.20-0.24 ms forward +
# backward: too few pixels for the 64-pixel row tiles of the gradient kernels).
DISPATCH = {
    (128, 64, 64, 64): True,     # 0.326 ms against 0.350 (torch spread 0.022)
    (64, 32, 128, 128): True,    # 0.343 ms against 0.416 (0.026)
    (32, 16, 256, 256): True,    # 0.448 ms against 0.631 (0.022)
}


def supported(Ci, Co):
    """Shapes the kernels take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    return Ci > 0 and Co > 0 and Ci % 8 == 0 and Co % 16 == 0


def _dims(B, Ci, Co, h, w, leak):
    return c_int(B), c_int(Ci), c_int(Co), c_int(h), c_int(w), c_float(leak)


class _TrunkConv(torch.autograd.Function):
    """y[B,Co,2h,2w] = lrelu(convT(x, weight) + bias[None])  (include/goliath_hip.h: gol_trunk_conv_*)."""

    @staticmethod
    def forward(ctx, x, weight, bias, leak):
        B, Ci, h, w = x.shape
        Co = weight.shape[1]
        y = torch.empty(B, Co, 2 * h, 2 * w, device=x.device)
        with _lib.device_guard(x.device):
            _lib.call("gol_trunk_conv_fwd", *_dims(B, Ci, Co, h, w, leak), fptr(x, "x"), fptr(weight, "weight"),
                      fptr(bias, "bias"), fptr(y), stream_ptr())
        ctx.save_for_backward(x, weight, y)
        ctx.leak = leak
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        B, Ci, h, w = x.shape
        Co = weight.shape[1]
        g = g.to(torch.float32).contiguous()
        need_x, need_w, need_b, _ = ctx.needs_input_grad
        g_x = torch.empty_like(x) if need_x else None
        g_w = torch.empty_like(weight) if need_w else None
        g_b = torch.empty(Co, 2 * h, 2 * w, device=x.device) if need_b else None
        wt = weight.permute(1, 3, 0, 2).contiguous() if need_x else None   # [Co,4 kx,Ci,4 ky]
        scratch = None
        if need_w:  # per-workgroup partial sums of the weight gradient (reduced by a second kernel: no float atomics)
            fn = _lib.load().gol_trunk_conv_bwd_scratch_floats
            fn.restype = ctypes.c_longlong
            scratch = torch.empty(int(fn(c_int(B), c_int(Ci), c_int(Co), c_int(h), c_int(w))), device=x.device)
        with _lib.device_guard(x.device):
            _lib.call("gol_trunk_conv_bwd", *_dims(B, Ci, Co, h, w, ctx.leak), fptr(x, "x"), fptr(wt, "w_eff_t"),
                      fptr(y, "y"), fptr(g, "g_y"), fptr(g_x), fptr(g_w), fptr(g_b), fptr(scratch), stream_ptr())
        return g_x, g_w, g_b, None


def convt_ub_lrelu(x, weight, bias, leak=0.2):
    """x[B,Ci,h,w], weight[Ci,Co,4,4] (effective), bias[Co,2h,2w] -> lrelu(convT(x, weight, s2 p1) + bias)[B,Co,2h,2w].
    HIP kernels; no CPU path."""
    if not (x.is_cuda and weight.is_cuda and bias.is_cuda):
        raise _lib.GoliathHipError("convt_ub_lrelu needs CUDA(HIP) tensors; there is no CPU path")
    if x.dim() != 4 or tuple(weight.shape) != (x.shape[1], weight.shape[1], 4, 4) or \
            tuple(bias.shape) != (weight.shape[1], 2 * x.shape[2], 2 * x.shape[3]):
        raise _lib.GoliathHipError(f"convt_ub_lrelu: shapes {tuple(x.shape)}, {tuple(weight.shape)}, {tuple(bias.shape)}")
    c = lambda t: t.to(torch.float32).contiguous()
    return _TrunkConv.apply(c(x), c(weight), c(bias), float(leak))


def convt_ub_lrelu_torch(x, weight, bias, leak=0.2):
    """The same composition in plain PyTorch, in the reference's order of operations: parity twin, runs on CPU."""
    return F.leaky_relu(F.conv_transpose2d(x, weight, None, 2, 1) + bias[None], leak)


def _is_convt_wnub(m):
    """A weight-normalised 4x4 / stride 2 / pad 1 transposed conv with an untied bias: goliath_amd.decoder's or the
    reference's ConvTranspose2dWNUB (same parameter names; cf. rgca._can_fuse_tail)."""
    from .decoder import ConvTranspose2dWNUB

    if not all(hasattr(m, a) for a in ("weight_v", "weight_g", "bias")) or m.bias is None or m.bias.dim() != 3:
        return False
    if m.weight_v.dim() != 4 or tuple(m.weight_v.shape[2:]) != (4, 4):
        return False
    if isinstance(m, ConvTranspose2dWNUB):
        return True
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    return (isinstance(m, nn.ConvTranspose2d) and pair(m.stride) == (2, 2) and pair(m.padding) == (1, 1)
            and pair(m.output_padding) == (0, 0) and pair(m.dilation) == (1, 1) and m.groups == 1)


def _takes_hip(layer, x):
    if not (x.is_cuda and x.dim() == 4 and layer.weight_v.is_cuda and layer.bias.is_cuda):
        return False
    Ci, Co = layer.weight_v.shape[:2]
    h, w = x.shape[2:]
    if x.shape[1] != Ci or tuple(layer.bias.shape) != (Co, 2 * h, 2 * w) or not supported(Ci, Co):
        return False
    return os.environ.get("GOLIATH_FUSED_TRUNK_ALL", "0") == "1" or DISPATCH.get((Ci, Co, h, w), False)


def run_stack(seq, x):
    """`seq(x)` for an nn.Sequential, with every (ConvTranspose2dWNUB, LeakyReLU) pair that `_takes_hip` admits run
    as one `convt_ub_lrelu`; every other module is simply called."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        act = mods[i + 1] if i + 1 < len(mods) else None
        if isinstance(act, nn.LeakyReLU) and act.negative_slope > 0 and _is_convt_wnub(m) and _takes_hip(m, x):
            x = convt_ub_lrelu(x, wn_weight(m), m.bias, act.negative_slope)
            i += 2
        else:
            x = m(x)
            i += 1
    return x


def enabled():
    """GOLIATH_FUSED_TRUNK=1: the decoders run their hidden layers through `run_stack` (default: off)."""
    return os.environ.get("GOLIATH_FUSED_TRUNK", "0") == "1"
