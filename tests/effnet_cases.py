"""Case table and float64 references of the fused MBConv front (goliath_amd.effnet: gol_mbconv_front_fwd / _bwd_x) and of the
EfficientNet feature loss, shared by tests/test_effnet_cases.py (CPU), tests/test_gpu_mbconv_front.py and
tests/test_gpu_effnet_loss.py.  All draws are made on the CPU from fixed seeds: x randn, w_e randn / sqrt(Ci), w_d randn / k,
BOTH biases 0.5 randn (so that the zero padding of the expanded tensor is visible: SiLU(b_e) is far from 0), upstream g_z
and g_ssum randn; images uniform in [-40, 290] so that both clamp branches occur.

The kernels' tiles: forward 8 x 32 output pixels at stride 1 and 8 x 16 at stride 2, backward 8 x 32 input pixels, chunks of
16 expanded channels (Ce is a multiple of 16, so no chunk is ragged), groups of 48 input channels in the backward (one
accumulator set of 16 / 32 / 48 rows for Ci <= 16 / 32 / 48, several workgroups beyond)."""
import functools

import torch
import torch.nn as nn

KINK = 1e-4         # upstream gradients are zeroed where an image value is closer to a clamp kink than this (vgg_cases.KINK)
BAR = 1e-5          # rel-L2 against float64 (tests/vgg_cases.py, test_gpu_texdec.py)
ZEROED_CAP = 2e-3

# (B, Ci, Ce, H, W, k, stride, expand)
CASES = [
    (2, 32, 32, 9, 33, 3, 1, 0),      # block 1.0's form, no expand; tiles both ways
    (2, 16, 96, 9, 35, 3, 2, 1),      # stride 2 with odd H and W (out 5 x 18): two forward tiles across
    (1, 24, 144, 18, 37, 3, 1, 1),    # several tiles both ways, odd W, nine channel chunks of 16
    (2, 24, 144, 17, 34, 5, 2, 1),    # k5 s2, odd H even W: both parities of the transposed taps
    (1, 40, 240, 7, 5, 5, 1, 1),      # image smaller than a tile, Ci = 40 (not a multiple of 16): 48-row accumulators
    (3, 8, 16, 2, 2, 5, 2, 1),        # image smaller than the filter, one output pixel, odd batch
    (2, 16, 48, 1, 1, 3, 2, 1),       # a single pixel
    (1, 8, 16, 40, 70, 5, 2, 1),      # tiles both ways (forward 3 x 3, backward 5 x 3) with a halo crossing every tile edge
    (1, 56, 16, 9, 34, 3, 1, 1),      # Ci > 48: two input-channel groups in the backward, the second ragged (8 of 48)
    (1, 16, 16, 17, 40, 5, 1, 0),     # k5 s1 without expand, tiles both ways
]
IDS = ["x".join(map(str, c[:5])) + f"k{c[5]}s{c[6]}" + ("" if c[7] else "n") for c in CASES]
EXPAND = [i for i, c in enumerate(CASES) if c[7]]


def out_size(n, k, s):
    return (n + 2 * ((k - 1) // 2) - k) // s + 1


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The draws of case i (CPU, float32)."""
    B, Ci, Ce, H, W, k, s, expand = CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    x = torch.randn(B, Ci, H, W, generator=g)
    w_e = torch.randn(Ce, Ci, generator=g) / Ci ** 0.5
    b_e = 0.5 * torch.randn(Ce, generator=g)
    w_d = torch.randn(Ce, k, k, generator=g) / k
    b_d = 0.5 * torch.randn(Ce, generator=g)
    g_z = torch.randn(B, Ce, out_size(H, k, s), out_size(W, k, s), generator=g)
    g_ssum = torch.randn(B, Ce, generator=g)
    if not expand:
        w_e = b_e = None
    return dict(x=x, w_e=w_e, b_e=b_e, w_d=w_d, b_d=b_d, g_z=g_z, g_ssum=g_ssum, k=k, stride=s)


def run_twin(i, dtype, front=None, g_z=True, g_ssum=True):
    """(z, ssum, g_x) of case i from `front` (default: effnet.mbconv_front_torch) in `dtype` on the CPU."""
    from goliath_amd import effnet

    front = effnet.mbconv_front_torch if front is None else front
    inp = inputs(i)
    c = lambda t: None if t is None else t.to(dtype)
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    z, ssum = front(x, c(inp["w_e"]), c(inp["b_e"]), c(inp["w_d"]), c(inp["b_d"]), inp["k"], inp["stride"])
    up = (z * c(inp["g_z"])).sum() * float(g_z) + (ssum * c(inp["g_ssum"])).sum() * float(g_ssum)
    g_x, = torch.autograd.grad(up, x)
    return z.detach(), ssum.detach(), g_x


@functools.lru_cache(maxsize=None)
def reference(i, g_z=True, g_ssum=True):
    """The float64 twin of case i."""
    return run_twin(i, torch.float64, None, g_z, g_ssum)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the whole network and the loss ------------------------------------------------------------------------------------------
LOSS_IMAGE = (2, 3, 37, 50)     # taps 16 x 19 x 25, 24 x 10 x 13, 40 x 5 x 7


def conv_bn(c_in, c_out, k, stride, groups=1, act=True):
    layers = [nn.Conv2d(c_in, c_out, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(c_out)]
    return nn.Sequential(*layers, nn.SiLU()) if act else nn.Sequential(*layers)


class SqueezeExcite(nn.Module):
    def __init__(self, channels, squeeze):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, channels, 1)

    def forward(self, x):
        s = torch.sigmoid(self.fc2(nn.functional.silu(self.fc1(x.mean((2, 3), keepdim=True)))))
        return s * x


class MBConv(nn.Module):
    """An inverted-residual block written from the issue's table out of plain library modules."""

    def __init__(self, c_in, c_exp, c_out, k, stride, residual):
        super().__init__()
        layers = [conv_bn(c_in, c_exp, 1, 1)] if c_exp != c_in else []
        layers += [conv_bn(c_exp, c_exp, k, stride, groups=c_exp), SqueezeExcite(c_exp, max(1, c_in // 4)),
                   conv_bn(c_exp, c_out, 1, 1, act=False)]
        self.block = nn.Sequential(*layers)
        self.residual = residual

    def forward(self, x):
        return self.block(x) + x if self.residual else self.block(x)


def module_network(seed):
    """features[0:4] as plain nn modules (eval mode) with random weights and running statistics (var in [0.5, 2]); its
    state dict carries the table's keys plus num_batches_tracked."""
    from goliath_amd import effnet

    torch.manual_seed(seed)
    stages = {}
    for name, c_in, c_exp, c_out, k, stride, residual in effnet.BLOCKS:
        stages.setdefault(name.split(".")[0], []).append(MBConv(c_in, c_exp, c_out, k, stride, residual))
    net = nn.Module()
    net.features = nn.Sequential(conv_bn(3, effnet.STEM, 3, 2), *(nn.Sequential(*stages[s]) for s in ("1", "2", "3")))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(m.bias.shape, generator=g))
            elif isinstance(m, nn.Conv2d) and m.bias is not None:
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
    return net.eval()


def module_taps(net, image):
    from goliath_amd import effnet

    out, x = [], effnet.normalize(image)
    for i, stage in enumerate(net.features):
        x = stage(x)
        if i > 0:
            out.append(x)
    return out


def draw_image(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 330.0 - 40.0


@functools.lru_cache(maxsize=None)
def loss_case(seed=7):
    """The network (real widths, random weights), prediction, target and a soft mask with an all-zero region."""
    from goliath_amd import effnet

    feats = effnet.EffNetB0Features().load_torchvision_state_dict(module_network(seed).state_dict())
    x, y = draw_image(10 * seed + 1, LOSS_IMAGE), draw_image(10 * seed + 2, LOSS_IMAGE)
    g = torch.Generator().manual_seed(10 * seed + 3)
    mask = torch.rand(LOSS_IMAGE[0], 1, *LOSS_IMAGE[2:], generator=g)
    mask[:, :, :, :12] = 0.0
    return feats, x, y, mask


def kink_mask(*images):
    """1 where every image value is farther than KINK from 0 and 255 (the clamp's kinks), else 0; per pixel."""
    near = torch.zeros(images[0].shape, dtype=torch.bool)
    for im in images:
        near |= (im.double().abs() < KINK) | ((im.double() - 255.0).abs() < KINK)
    return ~near


def reference_transcription(taps_x, taps_y, mask, weights=(0.8, 0.1, 0.1)):
    """The loss lines of the reference (the loop over the taps, the bilinear mask, the weighted masked mean absolute
    difference) written out on given taps."""
    loss = 0.0
    for i, (fx, fy) in enumerate(zip(taps_x, taps_y)):
        if isinstance(mask, torch.Tensor):
            m = nn.functional.interpolate(mask, size=(fx.shape[-2], fx.shape[-1]), mode="bilinear").detach()
        else:
            m = 1.0
        loss += weights[i] * ((fx - fy) * m).abs().mean()
    return loss
