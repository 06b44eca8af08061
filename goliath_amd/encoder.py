"""The joint texture / geometry encoder, and its texture stack as fused operators.

Same architecture, parameter names and shapes as `Encoder` (/root/reference/ca_code/models/rgca.py:256-332): `geommod`,
`texmod`, `jointmod`, `mean`, `logvar` built from weight-normalised layers (`ca_code/nn/layers.py:276-328,472`; weight
norm: one magnitude per output channel, direction normalised over the whole tensor, `layers.py:157-244`), so a reference
state_dict loads unchanged (tests/test_encoder_api.py checks the key set against the reference class when the reference
tree is present).  `base` is the spatial size the texture stack ends at: 4 in the reference (a 1024^2 texture); base=1
keeps the architecture and shrinks the texture to 256^2 for tests.

Each of the eight `texmod` layers is `Conv2dWNUB(Ci, Co, 4, 2, 1)` + an untied bias + `LeakyReLU(0.2)`: a MIOpen
convolution, an ATen add and an ATen leaky_relu forward, two MIOpen gradient convolutions, a batch reduction and the
activation's backward on the way back -- behind `color / 255.0 - 0.5`, two more passes over the texture.
`conv_ub_lrelu` runs a layer as ONE HIP kernel forward (gol_enc_conv_fwd: fp32-MFMA implicit GEMM, the affine of the
first layer folded into the load, bias and activation on the accumulators, nothing but y written) and three backward
(gol_enc_conv_bwd: input, weight and bias gradient, the activation mask read from the sign of y, no float atomics);
`conv_ub_lrelu_torch` is the same composition in plain PyTorch (parity twin, runs on CPU).

The weight norm stays torch algebra on the small tensor (`tail.wn_weight`), so gradients reach weight_v / weight_g
through the ordinary graph and the kernels see the effective weight.

`run_stack` walks an `nn.Sequential` and takes the operator for the (layer, LeakyReLU) pairs whose shape is in
`DISPATCH` -- the per-shape result of tools/encoder_probe.py, by the rule of section 6a: a shape
is admitted only where the HIP operator's forward + backward beat the library composition by more than the
composition's own run-to-run spread.  GOLIATH_FUSED_ENCODER_ALL=1 forces the operator for every supported shape
(tests, probes).
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_float, c_int, fptr, stream_ptr
from .decoder import LEAK, ConvTranspose2dWNUB, LinearWN, _glorot_, _wn
from .tail import wn_weight

# outputs of the eight texture layers (rgca.py:281-298); the first reads the 3 colour channels
CHANNELS = (32, 32, 64, 64, 128, 128, 256, 256)

# (Ci, Co, H, W) of the layer INPUT -> True: shapes where the HIP operator won the probe (B = 8, MI355X).
# From profiles/encoder_probe.json ("dispatch"; forward + backward medians in ms, HIP against the library composition, and
# the composition's spread); shapes that are not listed stay on the torch modules inside run_stack: 128->128 at 32^2,
# 128->256 at 16^2 and 256->256 at 8^2 lose (0.173 / 0.209 / 0.280 against 0.146 / 0.135 / 0.134: too few pixels for the
# 64-pixel tiles of the three GEMM kernels).
DISPATCH = {
    (3, 32, 1024, 1024): True,   # 0.456 ms against 0.933 (torch spread 0.004); the composition includes color / 255 - 0.5
    (32, 32, 512, 512): True,    # 0.666 ms against 0.891 (0.021)
    (32, 64, 256, 256): True,    # 0.314 ms against 0.381 (0.022)
    (64, 64, 128, 128): True,    # 0.186 ms against 0.202 (0.013): by 0.003 ms beyond the spread
    (64, 128, 64, 64): True,     # 0.153 ms against 0.179 (0.010)
}


def supported(Ci, Co, H, W):
    """Shapes the kernels take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    return (Ci > 0 and Co > 0 and H > 0 and W > 0 and Co % 16 == 0 and (Ci % 8 == 0 or Ci <= 4)
            and H % 2 == 0 and W % 2 == 0)


def _dims(B, Ci, Co, H, W, leak, in_scale, in_shift):
    return c_int(B), c_int(Ci), c_int(Co), c_int(H), c_int(W), c_float(leak), c_float(in_scale), c_float(in_shift)


class _EncConv(torch.autograd.Function):
    """y[B,Co,H/2,W/2] = lrelu(conv(in_scale x + in_shift, weight) + bias[None])  (include/goliath_hip.h: gol_enc_conv_*)."""

    @staticmethod
    def forward(ctx, x, weight, bias, leak, in_scale, in_shift):
        B, Ci, H, W = x.shape
        Co = weight.shape[0]
        y = torch.empty(B, Co, H // 2, W // 2, device=x.device)
        with _lib.device_guard(x.device):
            _lib.call("gol_enc_conv_fwd", *_dims(B, Ci, Co, H, W, leak, in_scale, in_shift), fptr(x, "x"),
                      fptr(weight, "weight"), fptr(bias, "bias"), fptr(y), stream_ptr())
        ctx.save_for_backward(x, weight, y)
        ctx.consts = (leak, in_scale, in_shift)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        B, Ci, H, W = x.shape
        Co = weight.shape[0]
        g = g.to(torch.float32).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        g_x = torch.empty_like(x) if need_x else None
        g_w = torch.empty_like(weight) if need_w else None
        g_b = torch.empty(Co, H // 2, W // 2, device=x.device) if need_b else None
        scratch = None
        if need_w:  # per-workgroup partial sums of the weight gradient (reduced by a second kernel: no float atomics)
            fn = _lib.load().gol_enc_conv_bwd_scratch_floats
            fn.restype = ctypes.c_longlong
            scratch = torch.empty(int(fn(c_int(B), c_int(Ci), c_int(Co), c_int(H), c_int(W))), device=x.device)
        with _lib.device_guard(x.device):
            _lib.call("gol_enc_conv_bwd", *_dims(B, Ci, Co, H, W, *ctx.consts), fptr(x, "x"), fptr(weight, "weight"),
                      fptr(y, "y"), fptr(g, "g_y"), fptr(g_x), fptr(g_w), fptr(g_b), fptr(scratch), stream_ptr())
        return g_x, g_w, g_b, None, None, None


def conv_ub_lrelu(x, weight, bias, leak=0.2, in_scale=1.0, in_shift=0.0):
    """x[B,Ci,H,W], weight[Co,Ci,4,4] (effective), bias[Co,H/2,W/2] ->
    lrelu(conv(in_scale x + in_shift, weight, s2 p1) + bias)[B,Co,H/2,W/2]; the zero pad comes after the affine.
    HIP kernels; no CPU path."""
    if not (x.is_cuda and weight.is_cuda and bias.is_cuda):
        raise _lib.GoliathHipError("conv_ub_lrelu needs CUDA(HIP) tensors; there is no CPU path")
    if x.dim() != 4 or tuple(weight.shape) != (weight.shape[0], x.shape[1], 4, 4) or x.shape[2] % 2 or x.shape[3] % 2 or \
            tuple(bias.shape) != (weight.shape[0], x.shape[2] // 2, x.shape[3] // 2):
        raise _lib.GoliathHipError(f"conv_ub_lrelu: shapes {tuple(x.shape)}, {tuple(weight.shape)}, {tuple(bias.shape)}")
    c = lambda t: t.to(torch.float32).contiguous()
    return _EncConv.apply(c(x), c(weight), c(bias), float(leak), float(in_scale), float(in_shift))


def conv_ub_lrelu_torch(x, weight, bias, leak=0.2, in_scale=1.0, in_shift=0.0):
    """The same composition in plain PyTorch, in the reference's order of operations (the affine on x first, then the
    zero-padded convolution, the bias, the activation): parity twin, runs on CPU and in float64."""
    if in_scale != 1.0 or in_shift != 0.0:
        x = x * in_scale + in_shift
    return F.leaky_relu(F.conv2d(x, weight, None, 2, 1) + bias[None], leak)


class Conv2dWNUB(nn.Module):
    """4x4 / stride 2 / pad 1 conv, weight-normalised, untied bias [C_out, height, width] (the OUTPUT size)."""

    def __init__(self, n_in, n_out, height, width, alpha=LEAK):
        super().__init__()
        self.weight_v = nn.Parameter(torch.empty(n_out, n_in, 4, 4))
        _glorot_(self.weight_v, n_in, n_out, 16, alpha)
        self.weight_g = nn.Parameter(torch.full((n_out, 1, 1, 1), float(self.weight_v.detach().norm())))
        self.bias = nn.Parameter(torch.zeros(n_out, height, width))

    def weight(self):
        return _wn(self.weight_v, self.weight_g)

    def forward(self, x):
        return F.conv2d(x, self.weight(), None, 2, 1) + self.bias[None]


def _is_conv_wnub(m):
    """A weight-normalised 4x4 / stride 2 / pad 1 conv with an untied bias: this module's or the reference's Conv2dWNUB
    (same parameter names).  Not the transposed sibling, not another kernel size, not a layer without weight norm."""
    if isinstance(m, (ConvTranspose2dWNUB, nn.ConvTranspose2d)):
        return False
    if not all(hasattr(m, a) for a in ("weight_v", "weight_g", "bias")) or m.bias is None or m.bias.dim() != 3:
        return False
    if m.weight_v.dim() != 4 or tuple(m.weight_v.shape[2:]) != (4, 4) or tuple(m.weight_g.shape) != (m.weight_v.shape[0], 1, 1, 1):
        return False
    if isinstance(m, Conv2dWNUB):
        return True
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    return (isinstance(m, nn.Conv2d) and pair(m.stride) == (2, 2) and pair(m.padding) == (1, 1)
            and pair(m.dilation) == (1, 1) and m.groups == 1 and m.padding_mode == "zeros")


def _takes_hip(layer, x):
    if not (x.is_cuda and x.dim() == 4 and layer.weight_v.is_cuda and layer.bias.is_cuda):
        return False
    Co, Ci = layer.weight_v.shape[:2]
    H, W = x.shape[2:]
    if x.shape[1] != Ci or not supported(Ci, Co, H, W) or tuple(layer.bias.shape) != (Co, H // 2, W // 2):
        return False
    return os.environ.get("GOLIATH_FUSED_ENCODER_ALL", "0") == "1" or DISPATCH.get((Ci, Co, H, W), False)


def _pair_taken(mods, i, x):
    act = mods[i + 1] if i + 1 < len(mods) else None
    return (isinstance(act, nn.LeakyReLU) and act.negative_slope > 0 and _is_conv_wnub(mods[i])
            and bool(_takes_hip(mods[i], x)))


def first_layer_taken(seq, x):
    """Whether `run_stack(seq, x, ...)` would hand an input affine to the operator (its first pair is taken)."""
    mods = list(seq)
    return bool(mods) and _pair_taken(mods, 0, x)


def run_stack(seq, x, in_scale=1.0, in_shift=0.0):
    """`seq(in_scale * x + in_shift)` for an nn.Sequential, with every (Conv2dWNUB, LeakyReLU) pair that `_takes_hip`
    admits run as one `conv_ub_lrelu`; every other module is simply called.  The affine goes into the first layer's load
    if that layer is taken, otherwise it is applied in torch in front of the stack."""
    mods = list(seq)
    affine = in_scale != 1.0 or in_shift != 0.0
    if affine and not (mods and _pair_taken(mods, 0, x)):
        x, affine = x * in_scale + in_shift, False
    i = 0
    while i < len(mods):
        m = mods[i]
        if _pair_taken(mods, i, x):
            if affine:
                x, affine = conv_ub_lrelu(x, wn_weight(m), m.bias, mods[i + 1].negative_slope, in_scale, in_shift), False
            else:
                x = conv_ub_lrelu(x, wn_weight(m), m.bias, mods[i + 1].negative_slope)
            i += 2
        else:
            x = m(x)
            i += 1
    return x


def encoder_forward(self, geom, color):
    """`Encoder.forward` (rgca.py:310-332) with `texmod` run through `run_stack`: where the first texture layer is taken,
    `color / 255.0 - 0.5` is folded into its load; otherwise that line and the stack are the reference's.  Everything else,
    the noise draw and the output keys included, is as the reference."""
    preds = {}

    geomout = self.geommod(geom.view(geom.shape[0], -1))
    if first_layer_taken(self.texmod, color):
        texout = run_stack(self.texmod, color, 1.0 / 255.0, -0.5)
    else:
        texout = run_stack(self.texmod, color / 255.0 - 0.5)
    texout = texout.view(texout.shape[0], -1)
    encout = self.jointmod(torch.cat([geomout, texout], dim=1))
    embs_mu = self.mean(encout) * self.mean_scale
    embs_logvar = self.logvar(encout) * self.logvar_scale

    # the noise is only applied to the input-conditioned values
    if self.training:
        noise = torch.randn_like(embs_mu)
        embs = embs_mu + torch.exp(embs_logvar) * noise * self.noise_std
    else:
        embs = embs_mu.clone()

    preds.update(embs=embs, embs_mu=embs_mu, embs_logvar=embs_logvar)
    return preds


class Encoder(nn.Module):
    """geom[B,n_verts_in,3], color[B,3,256 base,256 base] (0..255) -> embs, embs_mu, embs_logvar [B,n_embs]."""

    def __init__(self, n_embs, n_verts_in, noise_std=1.0, mean_scale=0.1, logvar_scale=0.01, base=4):
        super().__init__()
        self.noise_std, self.n_embs, self.mean_scale, self.logvar_scale = noise_std, n_embs, mean_scale, logvar_scale
        self.n_verts_in, self.base = n_verts_in, base
        self.geommod = nn.Sequential(LinearWN(n_verts_in * 3, 256), nn.LeakyReLU(LEAK, inplace=True))
        layers, c, s = [], 3, 256 * base
        for co in CHANNELS:
            s //= 2
            layers += [Conv2dWNUB(c, co, s, s), nn.LeakyReLU(LEAK, inplace=True)]
            c = co
        self.texmod = nn.Sequential(*layers)
        self.jointmod = nn.Sequential(LinearWN(256 + 256 * base * base, 512), nn.LeakyReLU(LEAK, inplace=True))
        self.mean = LinearWN(512, n_embs, alpha=1.0)
        self.logvar = LinearWN(512, n_embs, alpha=1.0)

    def forward(self, geom, color):
        return encoder_forward(self, geom, color)
