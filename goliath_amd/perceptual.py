"""The masked VGG19 feature loss (`vgg` in the hand configs) on a fused HIP layer operator.

`VGGLossMasked` (ca_code/loss/vgg.py:52-88, registered at ca_code/loss/perceptual.py:55-58) normalises
prediction and target, runs both through torchvision's VGG19 up to relu5_1 and sums five masked L1 distances of the
activations relu1_1 .. relu5_1.  The network is frozen, so a layer needs its output and its INPUT gradient and nothing
else.  `conv3_relu` runs such a layer -- 3x3 / stride 1 / pad 1 convolution + bias + ReLU, optionally on the normalised
image, optionally followed by the 2x2 max-pool -- as ONE HIP kernel forward (gol_conv3_fwd: fp32-MFMA implicit GEMM, the
normalisation in the load, bias, ReLU and pool on the accumulators; with pool only the pooled tensor and one position
byte per pooled element are written) and ONE backward (gol_conv3_bwd_x: the ReLU / pool mask applied while loading, the
same GEMM with mirrored taps, the clamp / std / 255 chain of the image in the epilogue; no atomics).  `conv3_relu_torch`
is the same layer in plain PyTorch (parity twin, any dtype and device), `vgg_loss_torch` the whole loss as the twin.

`Vgg19Features` holds the 13 convolutions under torchvision's parameter names and loads a `vgg19` state dict the USER
supplies: nothing is ever downloaded, torchvision is not needed.

A layer goes to the operator where its (Ci, Co, H, W, pool) is in `DISPATCH` -- the per-shape result of
tools/vgg_probe.py, by the rule of section 6a: a shape is admitted only where the HIP operator's
forward + backward beat the library composition by more than the composition's own run-to-run spread.  Every other
shape runs F.conv2d + relu (+ max_pool2d) inside the same function.  GOLIATH_FUSED_VGG_ALL=1 forces the operator for
every supported shape (tests, probes).

`precision="bf16x3"` (opt-in; the default everywhere is "fp32") runs the layers with Ci % 32 == 0 and Co % 32 == 0 on
gol_conv3x_fwd / gol_conv3x_bwd_x: each operand is split into two bf16 values, `split_bf16`, and three bf16 MFMAs are summed
in fp32 (4.5e-6 rel-L2 against float64, under the 1e-5 bar).  `conv3_relu_split_torch` is that
arithmetic in plain PyTorch.  Such a layer goes to the split operator where its shape is in `DISPATCH_BF16X3` (or with
GOLIATH_FUSED_VGG_ALL=1); a layer the split operator does not support or admit does exactly what "fp32" does for it.
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_int, fptr, ptr, stream_ptr

MEAN = (0.485, 0.456, 0.406)    # vgg.py:63
STD = (0.229, 0.224, 0.225)     # vgg.py:64
LOSS_WEIGHTS = (20.0, 5.0, 0.9, 0.5, 0.5)   # vgg.py:58

# torchvision's vgg19().features[0:30]: index of each convolution, convolutions per width, a pool after the first four groups
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)
GROUPS = (2, 2, 4, 4, 1)
TAPPED = (0, 5, 10, 19, 28)         # relu1_1, relu2_1, relu3_1, relu4_1, relu5_1: what Vgg19.forward returns (vgg.py:42-49)
POOLED = (2, 7, 16, 25)             # conv1_2, conv2_2, conv3_4, conv4_4: followed by features[4], [9], [18], [27]

# (Ci, Co, H, W, pool) of the layer INPUT -> True: shapes where the HIP operator won the probe (B = 1, MI355X), from
# profiles/vgg_probe.json ("dispatch"; forward + input gradient medians in ms, HIP against the library composition, and the
# composition's spread) and nothing else.  Shapes that are not listed stay on the library lines: the nine shapes from
# 64->128 @ 1024x667 to 512->512 @ 128x83 lose (2.45 ... 5.27 ms against 2.16 ... 3.41; the table is in DESIGN.md section 6e).
DISPATCH = {
    (3, 64, 2048, 1334, False): True,    # the image layer: 1.134 ms against 1.977 (torch spread 0.025)
    (64, 64, 2048, 1334, True): True,    # conv1_2 + pool: 4.946 ms against 5.720 (0.068)
}


# the same for precision="bf16x3": shapes where gol_conv3x_* won tools/vggx_probe.py against the library composition by more
# than its spread (profiles/vggx_probe.json, "dispatch") and nothing else.  Forward + input gradient
# medians in ms at B = 1 on the MI355X, split operator against the library composition (and the composition's spread)
DISPATCH_BF16X3 = {
    (64, 64, 2048, 1334, True): True,     # 1.699 against 5.587 (0.080); the fp32 operator of DISPATCH: 4.946
    (64, 128, 1024, 667, False): True,    # 0.974 against 2.061 (0.023)
    (128, 128, 1024, 667, True): True,    # 1.520 against 4.139 (0.101)
    (128, 256, 512, 333, False): True,    # 0.830 against 1.861 (0.039)
    (256, 256, 512, 333, False): True,    # 1.537 against 3.547 (0.072)
    (256, 256, 512, 333, True): True,     # 1.388 against 3.795 (0.057)
    (256, 512, 256, 166, False): True,    # 0.783 against 1.639 (0.065)
    (512, 512, 256, 166, False): True,    # 1.420 against 3.003 (0.056)
    (512, 512, 256, 166, True): True,     # 1.425 against 3.149 (0.179)
    (512, 512, 128, 83, False): True,     # 0.453 against 0.996 (0.015)
}

PRECISIONS = ("fp32", "bf16x3")


def _precision(precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    return precision


def supported(Ci, Co, H, W, pool=False, image_in=False, precision="fp32"):
    """Shapes the kernels of `precision` take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    if min(Ci, Co, H, W) < 1 or Co % 16 != 0 or (pool and (H < 2 or W < 2)):
        return False
    if _precision(precision) == "bf16x3":
        return not image_in and Ci % 32 == 0 and Co % 32 == 0
    return Ci == 3 if image_in else Ci % 8 == 0


def _dims(x, weight, pool, image_in):
    B, Ci, H, W = x.shape
    return (c_int(B), c_int(Ci), c_int(weight.shape[0]), c_int(H), c_int(W), c_int(int(image_in)), c_int(int(pool)))


class _Conv3(torch.autograd.Function):
    """include/goliath_hip.h: gol_conv3_fwd / gol_conv3_bwd_x.  Saves y, or p and the position bytes; x only with image_in."""

    @staticmethod
    def forward(ctx, x, weight, bias, pool, image_in):
        B, _, H, W = x.shape
        Co = weight.shape[0]
        out = torch.empty((B, Co, H // 2, W // 2) if pool else (B, Co, H, W), device=x.device)
        pos = torch.empty(out.shape, device=x.device, dtype=torch.uint8) if pool else None
        dims = _dims(x, weight, pool, image_in)
        with _lib.device_guard(x.device):
            _lib.call("gol_conv3_fwd", *dims, fptr(x, "x"), fptr(weight, "weight"), fptr(bias, "bias"), fptr(out),
                      ptr(pos, torch.uint8), stream_ptr())
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x if image_in else None, weight, out, pos)
            ctx.dims, ctx.shape = dims, x.shape
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, out, pos = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        g_x = torch.empty(ctx.shape, device=g.device)
        with _lib.device_guard(g.device):
            _lib.call("gol_conv3_bwd_x", *ctx.dims, fptr(x, "x"), fptr(weight, "weight"), fptr(out, "y"),
                      ptr(pos, torch.uint8), fptr(g, "g_y"), fptr(g_x), stream_ptr())
        return g_x, None, None, None, None


def pack_bf16x3(weight):
    """weight[Co,Ci,3,3] (CUDA) split once into the packed hi / lo buffer of gol_conv3x_fwd / gol_conv3x_bwd_x (int16)."""
    Co, Ci = weight.shape[:2]
    fn = _lib.load().gol_conv3x_packed_elems
    fn.restype = ctypes.c_longlong
    n = fn(c_int(Co), c_int(Ci))
    if n <= 0:
        raise _lib.GoliathHipError(f"bf16x3 needs Ci and Co to be multiples of 32, got {Ci} -> {Co}")
    weight = weight.detach().to(torch.float32).contiguous()
    packed = torch.empty(n, device=weight.device, dtype=torch.int16)
    with _lib.device_guard(weight.device):
        _lib.call("gol_conv3x_pack", c_int(Co), c_int(Ci), fptr(weight, "weight"), ptr(packed, torch.int16), stream_ptr())
    return packed


class _Conv3x(torch.autograd.Function):
    """include/goliath_hip.h: gol_conv3x_fwd / gol_conv3x_bwd_x.  Saves y, or p and the position bytes, and the packed weight."""

    @staticmethod
    def forward(ctx, x, packed, bias, pool):
        B, Ci, H, W = x.shape
        Co = bias.shape[0]
        out = torch.empty((B, Co, H // 2, W // 2) if pool else (B, Co, H, W), device=x.device)
        pos = torch.empty(out.shape, device=x.device, dtype=torch.uint8) if pool else None
        dims = (c_int(B), c_int(Ci), c_int(Co), c_int(H), c_int(W), c_int(int(pool)))
        with _lib.device_guard(x.device):
            _lib.call("gol_conv3x_fwd", *dims, fptr(x, "x"), ptr(packed, torch.int16, "packed"), fptr(bias, "bias"),
                      fptr(out), ptr(pos, torch.uint8), stream_ptr())
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(packed, out, pos)
            ctx.dims, ctx.shape = dims, x.shape
        return out

    @staticmethod
    def backward(ctx, g):
        packed, out, pos = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        g_x = torch.empty(ctx.shape, device=g.device)
        with _lib.device_guard(g.device):
            _lib.call("gol_conv3x_bwd_x", *ctx.dims, ptr(packed, torch.int16, "packed"), fptr(out, "y"),
                      ptr(pos, torch.uint8), fptr(g, "g_y"), fptr(g_x), stream_ptr())
        return g_x, None, None, None


def _check(name, x, weight, bias, image_in):
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape) != (weight.shape[0], x.shape[1], 3, 3) \
            or tuple(bias.shape) != (weight.shape[0],):
        raise _lib.GoliathHipError(f"{name}: shapes {tuple(x.shape)}, {tuple(weight.shape)}, {tuple(bias.shape)}")
    if image_in and x.shape[1] != 3:
        raise _lib.GoliathHipError(f"{name}: image_in needs 3 channels, got {x.shape[1]}")
    if torch.is_grad_enabled() and (weight.requires_grad or bias.requires_grad):
        raise _lib.GoliathHipError(f"{name}: the layer is frozen: there is no weight or bias gradient "
                                   "(detach the parameters, or use conv3_relu_torch)")


def conv3_relu(x, weight, bias, pool=False, image_in=False, precision="fp32", packed=None):
    """x[B,Ci,H,W], weight[Co,Ci,3,3], bias[Co] -> relu(conv(x, weight, s1 p1) + bias)[B,Co,H,W], or its 2x2 / stride 2
    max-pool [B,Co,H/2,W/2] with pool.  image_in (Ci = 3): x is the image in 0..255 and the operand its normalisation
    (vgg.py:62-65), zero-padded in normalised space.  Gradient reaches x only; asking for a weight or bias gradient
    raises.  precision="bf16x3": the split-bf16 product (Ci and Co multiples of 32, no image_in; anything else raises);
    packed = pack_bf16x3(weight) from an earlier call spares the split of the weight.  HIP kernels; no CPU path."""
    _check("conv3_relu", x, weight, bias, image_in)
    _precision(precision)
    if not (x.is_cuda and weight.is_cuda and bias.is_cuda):
        raise _lib.GoliathHipError("conv3_relu needs CUDA(HIP) tensors; there is no CPU path")
    c = lambda t: t.detach().to(torch.float32).contiguous()
    if precision == "bf16x3":
        if image_in:
            raise _lib.GoliathHipError("conv3_relu: precision='bf16x3' has no image layer")
        if packed is None:
            packed = pack_bf16x3(weight)
        return _Conv3x.apply(x.to(torch.float32).contiguous(), packed, c(bias), bool(pool))
    return _Conv3.apply(x.to(torch.float32).contiguous(), c(weight), c(bias), bool(pool), bool(image_in))


def normalize(batch):
    """VGGLossMasked.normalize (vgg.py:62-65)."""
    mean = batch.new_tensor(MEAN).view(1, 3, 1, 1)
    std = batch.new_tensor(STD).view(1, 3, 1, 1)
    return ((batch / 255.0).clamp(0.0, 1.0) - mean) / std


def conv3_relu_torch(x, weight, bias, pool=False, image_in=False):
    """The same layer in plain PyTorch, in the reference's order of operations: parity twin, any dtype and device."""
    if image_in:
        x = normalize(x)
    y = F.relu(F.conv2d(x, weight, bias, 1, 1))
    return F.max_pool2d(y, 2) if pool else y


def split_bf16(t):
    """(hi, lo) of gol_conv3x_*: hi = bf16(t), lo = bf16(t - hi), both by round to nearest even, of t taken as float32."""
    t = t.to(torch.float32)
    hi = t.to(torch.bfloat16)
    return hi, (t - hi.to(torch.float32)).to(torch.bfloat16)


def _three(conv, a, w, dtype):
    """lo_a hi_w + hi_a lo_w + hi_a hi_w in `dtype` (every product of two bf16 values is exact in float32 already)."""
    (ah, al), (wh, wl) = ((h.to(dtype), l.to(dtype)) for h, l in (split_bf16(a), split_bf16(w)))
    return conv(al, wh) + conv(ah, wl) + conv(ah, wh)


class _SplitLayer(torch.autograd.Function):
    """conv3_relu_split_torch: the forward and the input gradient of gol_conv3x_fwd / gol_conv3x_bwd_x in `acc_dtype`."""

    @staticmethod
    def forward(ctx, x, weight, bias, pool, acc_dtype):
        pre = _three(lambda a, w: F.conv2d(a, w, None, 1, 1), x, weight, acc_dtype) + bias.to(acc_dtype).view(1, -1, 1, 1)
        y = F.relu(pre)
        out, idx = F.max_pool2d(y, 2, return_indices=True) if pool else (y, None)
        ctx.save_for_backward(weight, y > 0, idx)
        ctx.acc_dtype, ctx.x_dtype = acc_dtype, x.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        weight, live, idx = ctx.saved_tensors
        g = g.to(torch.float32)
        if idx is not None:   # the element max_pool2d chose (the first maximum of a window) receives the window's gradient
            full = torch.zeros(live.shape, dtype=g.dtype, device=g.device)
            g = full.flatten(2).scatter_(2, idx.flatten(2), g.flatten(2)).view(live.shape)
        g_pre = g * live
        g_x = _three(lambda a, w: F.conv_transpose2d(a, w, None, 1, 1), g_pre, weight, ctx.acc_dtype)
        return g_x.to(ctx.x_dtype), None, None, None, None


def conv3_relu_split_torch(x, weight, bias, pool=False, acc_dtype=torch.float64):
    """The layer at precision "bf16x3" in plain PyTorch, on any device: x and weight (taken as float32) are split by
    `split_bf16` and the three products hi hi, hi lo, lo hi are three F.conv2d accumulated in `acc_dtype`; bias, ReLU and
    pool as `conv3_relu_torch`.  Its backward forms g_pre (ReLU / pool mask on the upstream gradient, float32), splits
    g_pre and the weight the same way and runs the transposed convolution as three products in `acc_dtype`.  Returns
    `acc_dtype`; the weights are frozen (no weight or bias gradient)."""
    return _SplitLayer.apply(x, weight.detach(), bias.detach(), bool(pool), acc_dtype)


def _route(x, weight, pool, image_in, precision="fp32"):
    """Which operator a layer takes: "bf16x3", "fp32" or None (the library lines)."""
    if not (x.is_cuda and weight.is_cuda and x.dim() == 4 and x.shape[0] > 0):
        return None
    Co, Ci = weight.shape[:2]
    H, W = x.shape[2:]
    if x.shape[1] != Ci:
        return None
    forced, key = os.environ.get("GOLIATH_FUSED_VGG_ALL", "0") == "1", (Ci, Co, H, W, bool(pool))
    if precision == "bf16x3" and supported(Ci, Co, H, W, pool, image_in, "bf16x3") \
            and (forced or DISPATCH_BF16X3.get(key, False)):
        return "bf16x3"
    if supported(Ci, Co, H, W, pool, image_in) and (forced or DISPATCH.get(key, False)):
        return "fp32"
    return None


def _layer(x, weight, bias, pool, image_in, precision="fp32", packed=None):
    """One layer: the operator where the shape is admitted, the library lines everywhere else.  packed: a callable that
    returns the layer's packed weight (bf16x3 only)."""
    route = _route(x, weight, pool, image_in, precision)
    if route == "bf16x3":
        return conv3_relu(x, weight, bias, pool, precision="bf16x3", packed=packed() if packed is not None else None)
    if route == "fp32":
        return conv3_relu(x, weight, bias, pool, image_in)
    return conv3_relu_torch(x, weight.to(x.dtype), bias.to(x.dtype), pool, image_in)


def _expected_keys():
    return [f"features.{i}.{n}" for i in CONV_INDEX for n in ("weight", "bias")]


class _Slot(nn.Module):
    """Holder of one convolution's frozen weight and bias (so the parameters carry torchvision's names)."""

    def __init__(self, n_in, n_out):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(n_out, n_in, 3, 3) * (2.0 / (9 * n_in)) ** 0.5, requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(n_out), requires_grad=False)


class Vgg19Features(nn.Module):
    """The 13 convolutions of torchvision's `vgg19().features[0:30]` (2, 2, 4, 4, 1 per width; a pool after each of the
    first four groups) as frozen parameters `features.{0,2,5,...,28}.{weight,bias}`.  `forward(image)` takes the image in
    0..255 and returns the five activations relu1_1 .. relu5_1 of `Vgg19.forward` (vgg.py:42-49) on its normalisation.
    Freshly built it holds random weights: load the pretrained ones with `load_torchvision_state_dict`.  `widths` other
    than VGG19's (multiples of 16) exist for tests and fixtures.  precision="bf16x3" sends the layers the split operator
    supports and admits to it (the module docstring); their packed weights are built on first use and cached per layer,
    keyed on the parameter's storage and version; `pack()` builds them ahead (callers that capture graphs), loading a
    state dict drops them."""

    def __init__(self, widths=(64, 128, 256, 512, 512), precision="fp32"):
        super().__init__()
        widths = tuple(int(w) for w in widths)
        if len(widths) != 5 or any(w < 16 or w % 16 for w in widths):
            raise ValueError(f"Vgg19Features: widths must be five multiples of 16, got {widths}")
        self.widths = widths
        self.precision = _precision(precision)
        self._packed = {}
        self.features = nn.Module()
        n_in, it = 3, iter(CONV_INDEX)
        for width, count in zip(widths, GROUPS):
            for _ in range(count):
                self.features.add_module(str(next(it)), _Slot(n_in, width))
                n_in = width

    def layers(self):
        """(index, weight, bias, pool, image_in, tapped) per convolution, in order."""
        for i in CONV_INDEX:
            slot = getattr(self.features, str(i))
            yield i, slot.weight, slot.bias, i in POOLED, i == 0, i in TAPPED

    def packed(self, index):
        """The packed bf16x3 weight of convolution `index`, from the cache or built now."""
        weight = getattr(self.features, str(index)).weight
        key = (weight.untyped_storage().data_ptr(), weight._version, weight.device)
        hit = self._packed.get(index)
        if hit is None or hit[0] != key:
            hit = self._packed[index] = (key, pack_bf16x3(weight))
        return hit[1]

    def pack(self):
        """Build the packed weight of every layer the split operator supports now (CUDA parameters), so that no later
        forward allocates or launches for it."""
        for i, weight, _, _, image_in, _ in self.layers():
            if supported(weight.shape[1], weight.shape[0], 2, 2, False, image_in, "bf16x3"):
                self.packed(i)
        return self

    def load_state_dict(self, *args, **kwargs):
        self._packed.clear()
        return super().load_state_dict(*args, **kwargs)

    def load_torchvision_state_dict(self, path_or_dict):
        """Load the convolutions of a torchvision `vgg19` state dict (e.g. the file `vgg19-dcbb9e9d.pth`, obtained by the
        user) given as a mapping or as a path for torch.load.  Keys with or without the `features.` prefix; `classifier.*`
        and later feature entries are ignored.  A missing file, a missing key or a wrong shape is an error that names
        what is expected.  Nothing is downloaded."""
        self._packed.clear()
        sd = path_or_dict
        if isinstance(sd, (str, os.PathLike)):
            if not os.path.isfile(sd):
                raise FileNotFoundError(f"{sd}: no such file.  Expected a torchvision vgg19 state dict (torch.save of "
                                        "vgg19().state_dict(), e.g. vgg19-dcbb9e9d.pth); it is never downloaded here")
            sd = torch.load(sd, map_location="cpu")
        if not hasattr(sd, "keys"):
            raise TypeError(f"load_torchvision_state_dict: a state dict or a path is expected, got {type(sd).__name__}")
        with torch.no_grad():
            for key in _expected_keys():
                short = key[len("features."):]
                if key not in sd and short not in sd:
                    raise KeyError(f"vgg19 state dict lacks '{key}' (also looked for '{short}'); expected the keys "
                                   f"features.{{{','.join(map(str, CONV_INDEX))}}}.{{weight,bias}}")
                src = sd[key] if key in sd else sd[short]
                index, name = short.split(".")
                dst = getattr(getattr(self.features, index), name)
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError(f"vgg19 state dict: '{key}' has shape {tuple(src.shape)}, expected {tuple(dst.shape)} "
                                     f"(widths {self.widths})")
                dst.copy_(src)
        return self

    def forward(self, image):
        out, x = [], image
        for i, weight, bias, pool, image_in, tapped in self.layers():
            x = _layer(x, weight, bias, pool, image_in, self.precision, lambda i=i: self.packed(i))
            if tapped:
                out.append(x)
        return out

    def forward_torch(self, image, precision="fp32"):
        """The twin: every layer on `conv3_relu_torch`, the parameters cast to the image's dtype.  precision="bf16x3": the
        layers the split operator supports run on `conv3_relu_split_torch`, accumulated in the image's dtype."""
        _precision(precision)
        out, x = [], image
        for _, weight, bias, pool, image_in, tapped in self.layers():
            if precision == "bf16x3" and supported(weight.shape[1], weight.shape[0], *x.shape[2:], pool, image_in, "bf16x3"):
                x = conv3_relu_split_torch(x, weight, bias, pool, acc_dtype=x.dtype)
            else:
                x = conv3_relu_torch(x, weight.to(x.dtype), bias.to(x.dtype), pool, image_in)
            if tapped:
                out.append(x)
        return out


def _level_mask(mask, feat):
    """vgg.py:76-81: the mask resized to the level, detached; a non-tensor mask is a plain factor."""
    if isinstance(mask, torch.Tensor):
        return F.interpolate(mask, size=(feat.shape[-2], feat.shape[-1]), mode="bilinear").detach()
    return mask


def _tap_losses_torch(x_feats, y_feats, mask, weights):
    """vgg.py:74-88, elementwise."""
    loss = 0
    for i in range(len(x_feats)):
        m = _level_mask(mask, x_feats[i])
        loss = loss + weights[i] * (x_feats[i] * m - y_feats[i] * m).abs().mean()
    return loss


def vgg_loss_torch(features, x_rgb, y_rgb, mask, weights=None, precision="fp32"):
    """The whole loss in plain PyTorch, line by line as `VGGLossMasked.forward` (vgg.py:67-88): parity twin, any dtype and
    device (the network's parameters are cast to the images' dtype).  precision: as `Vgg19Features.forward_torch`."""
    weights = list(LOSS_WEIGHTS) if weights is None else weights
    return _tap_losses_torch(features.forward_torch(x_rgb, precision), features.forward_torch(y_rgb, precision), mask,
                             weights)


class VGGLossMasked(nn.Module):
    """`VGGLossMasked` of vgg.py:52-88 over a `Vgg19Features`: forward(x_rgb, y_rgb, mask), weights [20, 5, 0.9, 0.5, 0.5].

    The target branch runs under no_grad and saves nothing when `y_rgb` does not require grad.  The per-level mask stays the
    reference's F.interpolate(mask, size, mode="bilinear") (one channel, tiny).  Each tap's distance goes through
    losses.image_penalty (IMG_ABS with the mask): that is mean |(x - y) m|, equal to the reference's mean |x m - y m| up to
    rounding, with gradient 0 at a zero residual (torch's abs has sign(0) = 0 as well).  A non-tensor mask is a plain
    factor, as in the reference.  A target that requires grad (the `dst_key` case) takes the twin's elementwise lines
    for the tap distances, so the gradient reaches it.  CUDA(HIP) tensors only; `vgg_loss_torch` is the CPU twin."""

    def __init__(self, features, weights=None):
        super().__init__()
        if not isinstance(features, Vgg19Features):
            raise TypeError("VGGLossMasked: features must be a Vgg19Features")
        self.vgg = features
        self.weights = list(LOSS_WEIGHTS) if weights is None else weights

    def forward(self, x_rgb, y_rgb, mask):
        from . import losses

        if not (x_rgb.is_cuda and y_rgb.is_cuda):
            raise _lib.GoliathHipError("VGGLossMasked needs CUDA(HIP) tensors; vgg_loss_torch is the CPU twin")
        x_vgg = self.vgg(x_rgb)
        if torch.is_grad_enabled() and y_rgb.requires_grad:
            return _tap_losses_torch(x_vgg, self.vgg(y_rgb), mask, self.weights)
        with torch.no_grad():
            y_vgg = self.vgg(y_rgb)
        loss = 0
        for i in range(len(x_vgg)):
            m = _level_mask(mask, x_vgg[i])
            if isinstance(m, torch.Tensor):
                if m.shape[1] not in (1, x_vgg[i].shape[1]):
                    raise ValueError(f"VGGLossMasked: mask {tuple(mask.shape)} must have 1 or {x_vgg[i].shape[1]} channels")
                term = losses.image_penalty(x_vgg[i], y_vgg[i], losses.IMG_ABS, m)
            else:
                term = losses.image_penalty(x_vgg[i], y_vgg[i], losses.IMG_ABS) * abs(m)
            loss = loss + self.weights[i] * term
        return loss


class VGGLoss(nn.Module):
    """The registry entry `vgg` (perceptual.py:55-58): `BasePerceptualLoss.forward`'s lines (perceptual.py:41-52) over
    `VGGLossMasked(features)`, the erosion on imageops.erode."""

    def __init__(self, assets=None, features=None, src_key="rendered_rgb", tgt_key="image", dst_key=None,
                 mask_key="image_mask", mask_erode=None):
        super().__init__()
        if features is None:
            raise ValueError("VGGLoss: features (a Vgg19Features with the pretrained weights loaded) is required")
        self.src_key, self.tgt_key, self.dst_key = src_key, tgt_key, dst_key
        self.mask_key, self.mask_erode = mask_key, mask_erode
        self.net = VGGLossMasked(features)

    def forward(self, preds, targets):
        from . import imageops

        # NOTE: for relighting training, mask comes from rendered alpha
        fg_mask = targets[self.mask_key] if self.mask_key in targets else preds[self.mask_key]
        if self.mask_erode is not None:
            fg_mask = imageops.erode(fg_mask, self.mask_erode)
        src = preds[self.src_key]
        tgt = targets[self.tgt_key] if self.dst_key is None else preds[self.dst_key]
        return self.net(src, tgt, fg_mask)


def as_features(perceptual, precision="fp32"):
    """A `Vgg19Features` from what dropin.patch_losses(perceptual=...) accepts: the network itself, a vgg19 state dict or
    the path of one.  A network built here gets `precision`; one that is passed in keeps its own unless `precision` names
    another than the default, which is then set on it."""
    _precision(precision)
    if isinstance(perceptual, Vgg19Features):
        if precision != "fp32":
            perceptual.precision = precision
        return perceptual
    return Vgg19Features(precision=precision).load_torchvision_state_dict(perceptual)
