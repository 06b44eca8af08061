"""The EfficientNet-B0 feature loss (`effnet`, `effnet_phys` in URHand's config) on a fused HIP MBConv front.

`EfficientNetLoss` (ca_code/loss/effnet.py:16-69, registered at ca_code/loss/perceptual.py:60-69) normalises prediction and
target, runs both through torchvision's `efficientnet_b0().features[0:4]` in eval mode and sums three masked L1 distances
of the outputs of features[1], [2], [3] (weights 0.8, 0.1, 0.1).  The network is frozen, so a block needs its output and
its INPUT gradient and nothing else.  `mbconv_front` runs the front of an inverted-residual block -- expand 1x1 + BN +
SiLU, depthwise k x k / stride s + BN, and the squeeze sum of SiLU(z) -- as ONE HIP kernel forward (gol_mbconv_front_fwd:
the expanded tensor is recomputed per tile into LDS on the fp32 MFMA and never exists in memory) and ONE backward
(gol_mbconv_front_bwd_x; no atomics).  `mbconv_front_torch` is the same in plain PyTorch (parity twin, any dtype and
device), `effnet_loss_torch` the whole loss as the twin.  BatchNorm (eval, eps 1e-5) is folded into (weight, bias) in
float64, once after loading: w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps).

`EffNetB0Features` holds the six modules under torchvision's state-dict names and loads an `efficientnet_b0` state dict
the USER supplies: nothing is ever downloaded, torchvision is not needed.

The normalisation, the stem, the two tiny SE convolutions, the gate SiLU(z) s, the project convolution and the residual
add are torch operators.  A front goes to the HIP operator where its (Ci, Ce, H, W, k, stride) is in `DISPATCH` -- the
per-shape result of tools/effnet_probe.py, by the rule of section 6a: a shape is admitted only
where the operator's forward + backward beat the folded library lines by more than their own run-to-run spread.  Every
other shape runs the twin's lines inside the same function.  GOLIATH_FUSED_EFFNET_ALL=1 forces the operator for every
supported shape (tests, probes).
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import c_int, ptr, stream_ptr

MEAN = (0.485, 0.456, 0.406)    # effnet.py:27
STD = (0.229, 0.224, 0.225)     # effnet.py:31
LOSS_WEIGHTS = (0.8, 0.1, 0.1)  # effnet.py:35
BN_EPS = 1e-5

# torchvision's efficientnet_b0().features[1:4]: (name, block input, expanded, output channels, kernel, stride, residual).
# MBConv1 (features.1.0) has no expand convolution: its sub-modules are block.0 depthwise, block.1 SE, block.2 project;
# the MBConv6 blocks are block.0 expand, block.1 depthwise, block.2 SE, block.3 project.  SE squeeze = max(1, input // 4).
STEM = 32
BLOCKS = (
    ("1.0", 32, 32, 16, 3, 1, False),
    ("2.0", 16, 96, 24, 3, 2, False),
    ("2.1", 24, 144, 24, 3, 1, True),
    ("3.0", 24, 144, 40, 5, 2, False),
    ("3.1", 40, 240, 40, 5, 1, True),
)
TAPPED = ("1.0", "2.1", "3.1")      # the last block of features[1], [2], [3]: what _compute_features returns (effnet.py:45-51)

# (Ci, Ce, H, W, k, stride) of the front's INPUT -> True: shapes where the HIP operator won the probe (B = 1, MI355X), from
# profiles/effnet_probe.json ("dispatch"; forward + input gradient medians in ms, HIP against the folded library lines, and
# the lines' spread) and nothing else.  All five fronts of features[1:4] at 2048 x 1334 won; a shape that is not listed
# (any other image size) stays on the library lines.  The table is in DESIGN.md section 6f.
DISPATCH = {
    (32, 32, 1024, 667, 3, 1): True,     # 1.0 (no expand): 0.325 ms against 2.236 (torch spread 0.014)
    (16, 96, 1024, 667, 3, 2): True,     # 2.0: 0.445 ms against 2.358 (0.021)
    (24, 144, 512, 334, 3, 1): True,     # 2.1: 0.416 ms against 2.062 (0.005)
    (24, 144, 512, 334, 5, 2): True,     # 3.0: 0.318 ms against 1.071 (0.006)
    (40, 240, 256, 167, 5, 1): True,     # 3.1: 0.692 ms against 1.642 (0.007)
}


def out_size(n, k, stride):
    """floor((n + 2 p - k) / stride) + 1 with p = (k - 1) // 2."""
    return (n + 2 * ((k - 1) // 2) - k) // stride + 1


def supported(Ci, Ce, H, W, k, stride, expand=True):
    """Shapes the kernels take (the ABI answers GOL_ERR_UNSUPPORTED otherwise)."""
    if min(Ci, Ce, H, W) < 1 or k not in (3, 5) or stride not in (1, 2):
        return False
    return Ci % 8 == 0 and Ce % 16 == 0 and (expand or Ci == Ce)


def _abi_mbconv_front_tiles(*, H, W, k, stride):
    return _lib.load().gol_mbconv_front_tiles(c_int(H), c_int(W), c_int(k), c_int(stride))


def _abi_mbconv_front_fwd(*, B, Ci, Ce, H, W, k, stride, expand, x, w_e, b_e, w_d, b_d, z, partials):
    _lib.call("gol_mbconv_front_fwd", c_int(B), c_int(Ci), c_int(Ce), c_int(H), c_int(W), c_int(k), c_int(stride),
              c_int(expand), _p(x), _p(w_e), _p(b_e), _p(w_d), _p(b_d), _p(z), _p(partials), stream_ptr())


def _abi_mbconv_front_bwd_x(*, B, Ci, Ce, H, W, k, stride, expand, x, w_e, b_e, w_d, z, g_z, g_ssum, g_x):
    _lib.call("gol_mbconv_front_bwd_x", c_int(B), c_int(Ci), c_int(Ce), c_int(H), c_int(W), c_int(k), c_int(stride),
              c_int(expand), _p(x), _p(w_e), _p(b_e), _p(w_d), _p(z), _p(g_z), _p(g_ssum), _p(g_x), stream_ptr())


def _p(t):
    """A tensor's device pointer (float32, or float64 for the partials); a raw address passes through."""
    if t is None or isinstance(t, torch.Tensor):
        return ptr(t, None if t is None or t.dtype == torch.float64 else torch.float32)
    return ctypes.c_void_p(t)


class _Front(torch.autograd.Function):
    """include/goliath_hip.h: gol_mbconv_front_fwd / gol_mbconv_front_bwd_x.  Saves x, z and the folded weights."""

    @staticmethod
    def forward(ctx, x, w_e, b_e, w_d, b_d, k, stride):
        B, Ci, H, W = x.shape
        Ce = w_d.shape[0]
        Ho, Wo = out_size(H, k, stride), out_size(W, k, stride)
        z = torch.empty((B, Ce, Ho, Wo), device=x.device)
        dims = dict(B=B, Ci=Ci, Ce=Ce, H=H, W=W, k=k, stride=stride, expand=int(w_e is not None))
        if B == 0:
            ssum = torch.zeros((0, Ce), device=x.device)
        else:
            with _lib.device_guard(x.device):
                tiles = _abi_mbconv_front_tiles(H=H, W=W, k=k, stride=stride)
                partials = torch.empty((B, Ce, tiles), device=x.device, dtype=torch.float64)
                _abi_mbconv_front_fwd(**dims, x=x, w_e=w_e, b_e=b_e, w_d=w_d, b_d=b_d, z=z, partials=partials)
            ssum = partials.sum(2).to(torch.float32)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, w_e, b_e, w_d, z)
            ctx.dims = dims
        return z, ssum

    @staticmethod
    def backward(ctx, g_z, g_ssum):
        x, w_e, b_e, w_d, z = ctx.saved_tensors
        g_z = g_z.to(torch.float32).contiguous()
        g_ssum = g_ssum.to(torch.float32).contiguous()
        g_x = torch.empty_like(x)
        if ctx.dims["B"] > 0:
            with _lib.device_guard(g_z.device):
                _abi_mbconv_front_bwd_x(**ctx.dims, x=x, w_e=w_e, b_e=b_e, w_d=w_d, z=z, g_z=g_z, g_ssum=g_ssum, g_x=g_x)
        return g_x, None, None, None, None, None, None


def _check(name, x, w_e, b_e, w_d, b_d, k):
    tensors = [t for t in (w_e, b_e, w_d, b_d) if t is not None]
    if (w_e is None) != (b_e is None):
        raise _lib.GoliathHipError(f"{name}: w_e and b_e come together (both None: no expand)")
    Ce = w_d.shape[0]
    ok = x.dim() == 4 and w_d.numel() == Ce * k * k and tuple(b_d.shape) == (Ce,)
    if ok and w_e is not None:
        ok = w_e.numel() == Ce * x.shape[1] and w_e.shape[:2] == (Ce, x.shape[1]) and tuple(b_e.shape) == (Ce,)
    if not ok:
        raise _lib.GoliathHipError(f"{name}: shapes x {tuple(x.shape)}, w_e {None if w_e is None else tuple(w_e.shape)}, "
                                   f"w_d {tuple(w_d.shape)}, b_d {tuple(b_d.shape)}, k {k}")
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise _lib.GoliathHipError(f"{name}: the block is frozen: there is no weight or bias gradient "
                                   "(detach the parameters, or use mbconv_front_torch)")
    return tensors


def mbconv_front(x, w_e, b_e, w_d, b_d, k, stride):
    """x[B,Ci,H,W], w_e[Ce,Ci(,1,1)], b_e[Ce], w_d[Ce(,1),k,k], b_d[Ce] (BatchNorm folded in) -> (z, ssum):
    z[B,Ce,Ho,Wo] = depthwise_k,stride(pad0(SiLU(w_e x + b_e))) + b_d, the pre-activation, and ssum[B,Ce] = the sum of
    SiLU(z) over the plane.  w_e = b_e = None: no expand, the depthwise runs on x (Ci == Ce).  The padding is zero in
    the EXPANDED tensor.  Gradient reaches x only; asking for a weight gradient raises.  HIP kernels; no CPU path."""
    tensors = _check("mbconv_front", x, w_e, b_e, w_d, b_d, k)
    if not (x.is_cuda and all(t.is_cuda for t in tensors)):
        raise _lib.GoliathHipError("mbconv_front needs CUDA(HIP) tensors; there is no CPU path")
    c = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
    return _Front.apply(x.to(torch.float32).contiguous(), c(w_e), c(b_e), c(w_d), c(b_d), int(k), int(stride))


def mbconv_front_torch(x, w_e, b_e, w_d, b_d, k, stride):
    """The same in plain PyTorch, in the library's order of operations: parity twin, any dtype and device."""
    Ce = w_d.shape[0]
    e = x if w_e is None else F.silu(F.conv2d(x, w_e.reshape(Ce, x.shape[1], 1, 1), b_e))
    z = F.conv2d(e, w_d.reshape(Ce, 1, k, k), b_d, stride, (k - 1) // 2, 1, Ce)
    return z, F.silu(z).sum((2, 3))


def _takes_hip(x, w_d, k, stride, expand):
    if not (x.is_cuda and w_d.is_cuda and x.dim() == 4 and x.shape[0] > 0):
        return False
    Ci, H, W = x.shape[1:]
    Ce = w_d.shape[0]
    if not supported(Ci, Ce, H, W, k, stride, expand):
        return False
    return os.environ.get("GOLIATH_FUSED_EFFNET_ALL", "0") == "1" or DISPATCH.get((Ci, Ce, H, W, k, stride), False)


def _front(x, w_e, b_e, w_d, b_d, k, stride):
    """One front: the operator where the shape is admitted, the library lines everywhere else."""
    if _takes_hip(x, w_d, k, stride, w_e is not None):
        return mbconv_front(x, w_e, b_e, w_d, b_d, k, stride)
    return mbconv_front_torch(x, w_e, b_e, w_d, b_d, k, stride)


def normalize(batch, mean=None, std=None):
    """EfficientNetLoss.normalize (effnet.py:42-43).  mean, std: the constants as [1,3,1,1] tensors already on the device
    (building them here is a host-to-device copy, which a stream capture does not allow)."""
    if mean is None:
        mean = batch.new_tensor(MEAN).view(1, 3, 1, 1)
        std = batch.new_tensor(STD).view(1, 3, 1, 1)
    return ((batch / 255.0).clamp(0.0, 1.0) - mean) / std


def _block_layout(name, c_in, c_exp, c_out, k):
    """{role: (sub-module path below features.<name>, conv weight shape)} and the SE shapes of one block."""
    has_expand = c_exp != c_in
    dw, se, proj = (1, 2, 3) if has_expand else (0, 1, 2)
    convs = {"dw": (f"block.{dw}", (c_exp, 1, k, k)), "project": (f"block.{proj}", (c_out, c_exp, 1, 1))}
    if has_expand:
        convs["expand"] = ("block.0", (c_exp, c_in, 1, 1))
    return convs, f"block.{se}", max(1, c_in // 4)


def expected_entries():
    """[(key, shape)] of every tensor the network holds, in torchvision's state-dict order."""
    def conv_bn(path, shape):
        c = shape[0]
        return [(f"{path}.0.weight", shape)] + [(f"{path}.1.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var")]

    out = conv_bn("features.0", (STEM, 3, 3, 3))
    for name, c_in, c_exp, c_out, k, _, _ in BLOCKS:
        convs, se, sq = _block_layout(name, c_in, c_exp, c_out, k)
        base = f"features.{name}."
        if "expand" in convs:
            out += conv_bn(base + convs["expand"][0], convs["expand"][1])
        out += conv_bn(base + convs["dw"][0], convs["dw"][1])
        out += [(f"{base}{se}.fc1.weight", (sq, c_exp, 1, 1)), (f"{base}{se}.fc1.bias", (sq,)),
                (f"{base}{se}.fc2.weight", (c_exp, sq, 1, 1)), (f"{base}{se}.fc2.bias", (c_exp,))]
        out += conv_bn(base + convs["project"][0], convs["project"][1])
    return out


class EffNetB0Features(nn.Module):
    """The stem and the five MBConv blocks of torchvision's `efficientnet_b0().features[0:4]` as frozen tensors under the
    state-dict names of that model (convolution `.0.weight`, BatchNorm `.1.{weight,bias,running_mean,running_var}`, SE
    `fc1` / `fc2` with bias).  `forward(image)` takes the image in 0..255 and returns the outputs of features[1], [2], [3]
    (effnet.py:45-51) on its normalisation, in eval mode.  Freshly built it holds random weights: load the pretrained
    ones with `load_torchvision_state_dict`."""

    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(0)
        for key, shape in expected_entries():
            *path, leaf = key.split(".")
            mod = self
            for part in path:
                if not hasattr(mod, part):
                    mod.add_module(part, nn.Module())
                mod = getattr(mod, part)
            if leaf in ("running_mean", "running_var"):
                mod.register_buffer(leaf, torch.zeros(shape) if leaf == "running_mean" else torch.ones(shape))
            elif len(shape) == 4:
                fan_in = shape[1] * shape[2] * shape[3]
                mod.register_parameter(leaf, nn.Parameter(torch.randn(shape, generator=gen) * fan_in ** -0.5, requires_grad=False))
            else:   # BatchNorm weight 1, every bias 0
                is_bn_weight = leaf == "weight"
                mod.register_parameter(leaf, nn.Parameter(torch.ones(shape) if is_bn_weight else torch.zeros(shape),
                                                          requires_grad=False))
        self._folded = {}

    def _apply(self, fn, *args, **kwargs):
        self._folded = {}       # .to(), .cuda(), .double(): fold again from the moved tensors
        return super()._apply(fn, *args, **kwargs)

    def load_torchvision_state_dict(self, path_or_dict):
        """Load features[0:4] of a torchvision `efficientnet_b0` state dict (e.g. the file
        `efficientnet_b0_rwightman-7f5810bc.pth`, obtained by the user) given as a mapping or as a path for torch.load.
        Keys with or without the `features.` prefix; `num_batches_tracked`, later features and the classifier are ignored.
        A missing file, a missing key or a wrong shape is an error that names what is expected.  Nothing is downloaded."""
        sd = path_or_dict
        if isinstance(sd, (str, os.PathLike)):
            if not os.path.isfile(sd):
                raise FileNotFoundError(f"{sd}: no such file.  Expected a torchvision efficientnet_b0 state dict (torch.save "
                                        "of efficientnet_b0().state_dict(), e.g. efficientnet_b0_rwightman-7f5810bc.pth); "
                                        "it is never downloaded here")
            sd = torch.load(sd, map_location="cpu")
        if not hasattr(sd, "keys"):
            raise TypeError(f"load_torchvision_state_dict: a state dict or a path is expected, got {type(sd).__name__}")
        own = dict(self.state_dict(keep_vars=True))
        with torch.no_grad():
            for key, shape in expected_entries():
                short = key[len("features."):]
                if key not in sd and short not in sd:
                    stem = key.rsplit(".", 2)[0]
                    near = sorted(k for k in sd.keys() if k.startswith(stem) or k.startswith(stem[len("features."):]))[:6]
                    raise KeyError(f"efficientnet_b0 state dict lacks '{key}' (also looked for '{short}'), expected with "
                                   f"shape {tuple(shape)}; keys found under '{stem}': {near if near else 'none'}")
                src = sd[key] if key in sd else sd[short]
                if tuple(src.shape) != tuple(shape):
                    raise ValueError(f"efficientnet_b0 state dict: '{key}' has shape {tuple(src.shape)}, expected {tuple(shape)}")
                own[key].copy_(src)
        self._folded = {}
        return self

    def folded(self, dtype=torch.float32):
        """The network with BatchNorm folded in, computed in float64 and cast to `dtype`: a dict with `stem` = (w, b),
        `norm` = (mean, std) and per block name (w_e [Ce,Ci] or None, b_e, w_d [Ce,k,k], b_d, fc1 w, fc1 b, fc2 w, fc2 b, w_p, b_p)."""
        if dtype in self._folded:
            return self._folded[dtype]
        sd = {k: v.detach().double() for k, v in self.state_dict().items()}

        def fold(path):
            scale = sd[f"{path}.1.weight"] / torch.sqrt(sd[f"{path}.1.running_var"] + BN_EPS)
            w = sd[f"{path}.0.weight"] * scale.view(-1, 1, 1, 1)
            return w.to(dtype), (sd[f"{path}.1.bias"] - sd[f"{path}.1.running_mean"] * scale).to(dtype)

        device = sd["features.0.0.weight"].device
        out = {"stem": fold("features.0"),
               "norm": tuple(torch.tensor(v, dtype=dtype, device=device).view(1, 3, 1, 1) for v in (MEAN, STD))}
        for name, c_in, c_exp, c_out, k, _, _ in BLOCKS:
            convs, se, _ = _block_layout(name, c_in, c_exp, c_out, k)
            base = f"features.{name}."
            w_e = b_e = None
            if "expand" in convs:
                w_e, b_e = fold(base + convs["expand"][0])
                w_e = w_e.reshape(c_exp, c_in).contiguous()
            w_d, b_d = fold(base + convs["dw"][0])
            fcs = tuple(sd[f"{base}{se}.{n}"].to(dtype) for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"))
            out[name] = (w_e, b_e, w_d.reshape(c_exp, k, k).contiguous(), b_d) + fcs + fold(base + convs["project"][0])
        self._folded[dtype] = out
        return out

    def _run(self, image, front):
        f = self.folded(image.dtype)
        x = F.silu(F.conv2d(normalize(image, *f["norm"]), f["stem"][0], f["stem"][1], 2, 1))
        taps = []
        for name, _, _, _, k, stride, residual in BLOCKS:
            w_e, b_e, w_d, b_d, w1, b1, w2, b2, w_p, b_p = f[name]
            z, ssum = front(x, w_e, b_e, w_d, b_d, k, stride)
            s = (ssum / (z.shape[2] * z.shape[3]))[:, :, None, None]
            s = torch.sigmoid(F.conv2d(F.silu(F.conv2d(s, w1, b1)), w2, b2))
            y = F.conv2d(F.silu(z) * s, w_p, b_p)
            x = y + x if residual else y
            if name in TAPPED:
                taps.append(x)
        return taps

    def forward(self, image):
        return self._run(image, _front)

    def forward_torch(self, image):
        """The twin: every front on `mbconv_front_torch`, the folded parameters cast to the image's dtype."""
        return self._run(image, mbconv_front_torch)


def _level_mask(mask, feat):
    """effnet.py:62-67: the mask resized to the level, detached; anything that is not a tensor means no mask."""
    if isinstance(mask, torch.Tensor):
        return F.interpolate(mask, size=(feat.shape[-2], feat.shape[-1]), mode="bilinear").detach()
    return 1.0


def _tap_losses_torch(x_feats, y_feats, mask, weights):
    """effnet.py:60-69, elementwise."""
    loss = 0.0
    for i, (fx, fy) in enumerate(zip(x_feats, y_feats)):
        m = _level_mask(mask, fx)
        loss = loss + weights[i] * ((fx - fy) * m).abs().mean()
    return loss


def effnet_loss_torch(features, x, y, mask=None, weights=None):
    """The whole loss in plain PyTorch, line by line as `EfficientNetLoss.forward` (effnet.py:53-69): parity twin, any
    dtype and device (the folded parameters are cast to the images' dtype)."""
    weights = list(LOSS_WEIGHTS) if weights is None else weights
    return _tap_losses_torch(features.forward_torch(x), features.forward_torch(y), mask, weights)


class EfficientNetLoss(nn.Module):
    """`EfficientNetLoss` of effnet.py:16-69 over an `EffNetB0Features`: forward(x, y, mask=None), weights [0.8, 0.1, 0.1].

    The target branch runs under no_grad and saves nothing when `y` does not require grad.  The per-level mask stays the
    reference's F.interpolate(mask, size, mode="bilinear") (one channel, tiny).  Each tap's distance goes through
    losses.image_penalty (IMG_ABS with the mask): mean |(fx - fy) m|, the reference's expression.  A mask that is not a
    tensor means m = 1.0, as in the reference.  A target that requires grad (the `dst_key` case) takes the twin's
    elementwise lines for the tap distances, so the gradient reaches it.  CUDA(HIP) tensors only; `effnet_loss_torch` is
    the CPU twin."""

    def __init__(self, features, weights=None):
        super().__init__()
        if not isinstance(features, EffNetB0Features):
            raise TypeError("EfficientNetLoss: features must be an EffNetB0Features")
        self.ftrs_net = features
        self.weights = list(LOSS_WEIGHTS) if weights is None else weights

    def forward(self, x, y, mask=None):
        from . import losses

        if not (x.is_cuda and y.is_cuda):
            raise _lib.GoliathHipError("EfficientNetLoss needs CUDA(HIP) tensors; effnet_loss_torch is the CPU twin")
        ftrs_x = self.ftrs_net(x)
        if torch.is_grad_enabled() and y.requires_grad:
            return _tap_losses_torch(ftrs_x, self.ftrs_net(y), mask, self.weights)
        with torch.no_grad():
            ftrs_y = self.ftrs_net(y)
        loss = 0.0
        for i, (fx, fy) in enumerate(zip(ftrs_x, ftrs_y)):
            m = _level_mask(mask, fx)
            if isinstance(m, torch.Tensor):
                if m.shape[1] not in (1, fx.shape[1]):
                    raise ValueError(f"EfficientNetLoss: mask {tuple(mask.shape)} must have 1 or {fx.shape[1]} channels")
                term = losses.image_penalty(fx, fy, losses.IMG_ABS, m.to(torch.float32).contiguous())
            else:
                term = losses.image_penalty(fx, fy, losses.IMG_ABS)
            loss = loss + self.weights[i] * term
        return loss


class EffNetLoss(nn.Module):
    """The registry entries `effnet` and `effnet_phys` (perceptual.py:60-69): `BasePerceptualLoss.forward`'s lines
    (perceptual.py:41-52) over `EfficientNetLoss(features)`, the erosion on imageops.erode."""

    def __init__(self, assets=None, features=None, src_key="rendered_rgb", tgt_key="image", dst_key=None,
                 mask_key="image_mask", mask_erode=None):
        super().__init__()
        if features is None:
            raise ValueError("EffNetLoss: features (an EffNetB0Features with the pretrained weights loaded) is required")
        self.src_key, self.tgt_key, self.dst_key = src_key, tgt_key, dst_key
        self.mask_key, self.mask_erode = mask_key, mask_erode
        self.net = EfficientNetLoss(features)

    def forward(self, preds, targets):
        from . import imageops

        # NOTE: for relighting training, mask comes from rendered alpha
        fg_mask = targets[self.mask_key] if self.mask_key in targets else preds[self.mask_key]
        if self.mask_erode is not None:
            fg_mask = imageops.erode(fg_mask, self.mask_erode)
        src = preds[self.src_key]
        tgt = targets[self.tgt_key] if self.dst_key is None else preds[self.dst_key]
        return self.net(src, tgt, fg_mask)


def as_features(effnet):
    """An `EffNetB0Features` from what dropin.patch_losses(effnet=...) accepts: the network itself, an efficientnet_b0
    state dict or the path of one."""
    if isinstance(effnet, EffNetB0Features):
        return effnet
    return EffNetB0Features().load_torchvision_state_dict(effnet)
