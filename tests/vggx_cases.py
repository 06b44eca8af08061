"""Case tables and references of the split-bf16 VGG layer (goliath_amd.perceptual, precision="bf16x3": gol_conv3x_fwd /
gol_conv3x_bwd_x) and of the masked VGG loss at that precision, shared by tests/test_vggx_cases.py (CPU),
tests/test_gpu_vggconvx.py and tests/test_gpu_vggx_loss.py.  Draws, KINK, BAR and ZEROED_CAP are those of tests/vgg_cases.py.

The reference of the GPU tests is the split twin accumulated in float64 ON THE SAME float32 INPUTS: the splits of identical
inputs are bit-identical, so the operator differs from it by its fp32 summation order alone (about 1e-7), while a kernel
that truncates instead of rounding, or drops a cross term, lands above BAR."""
import functools

import torch
import torch.nn.functional as F

import vgg_cases as vc

# (B, Ci, Co, H, W), pool.  The kernel's tile is 8 x 32 pixels x 64 channels (32 where there are only 32), its K stage 32
# channels; the channels WRITTEN are Co forward and Ci backward.  The cases of the issue, unchanged: each does for this
# tile what its note says -- 96 = 64 + a ragged 32 forward, 160 = 64 + 64 + a ragged 32 backward and five K stages forward.
CASES = [
    ((2, 32, 32, 8, 32), False),     # exactly one tile, one K stage
    ((2, 32, 96, 18, 37), False),    # tiles both ways, odd W, a ragged channel tile
    ((3, 64, 32, 7, 5), False),      # smaller than a tile, odd batch, two K stages
    ((1, 160, 64, 17, 34), False),   # five K stages; backward: three channel tiles, the last ragged
    ((2, 32, 32, 18, 37), True),     # pooled: odd W drops a column
    ((2, 32, 64, 7, 5), True),       # pooled: odd H and W drop a row and a column
    ((2, 64, 32, 2, 2), True),       # pooled: one window
]
IDS = ["x".join(map(str, s)) + ("p" if pool else "") for s, pool in CASES]
POOLED = [i for i, c in enumerate(CASES) if c[1]]

ELEMENT_BOUND = 3.1 * 2.0 ** -16    # |split - exact| <= this x sum |x||w|: 2^-16 per operand, 2^-16 (1 + 2^-7) for lo lo


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The draws of case i (CPU, float32), as vgg_cases.inputs makes them: x, weight, bias and the upstream gradient."""
    (B, Ci, Co, H, W), pool = CASES[i]
    weight, bias = vc.draw_layer(1700 + i, Ci, Co)
    g = torch.Generator().manual_seed(1800 + i)
    x = torch.randn(B, Ci, H, W, generator=g)
    up = torch.randn((B, Co, H // 2, W // 2) if pool else (B, Co, H, W), generator=g)
    return dict(x=x, weight=weight, bias=bias, up=up)


def split_pre(x, weight, bias, dtype):
    """The pre-activation of the split arithmetic written out: lo_x hi_w + hi_x lo_w + hi_x hi_w + bias in `dtype`."""
    from goliath_amd import perceptual

    (xh, xl), (wh, wl) = ((h.to(dtype), l.to(dtype)) for h, l in (perceptual.split_bf16(x), perceptual.split_bf16(weight)))
    conv = lambda a, w: F.conv2d(a, w, None, 1, 1)
    return conv(xl, wh) + conv(xh, wl) + conv(xh, wh) + bias.to(dtype).view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def reference(i):
    """Case i on the float64-accumulated split twin: its pre-activation, output, window argmax, the upstream gradient
    zeroed at the twin's kinks, g_x and the zeroed share; and the plain float64 layer (pre-activation, g_x under the same
    upstream gradient) with sum |x||w| for the element bound."""
    from goliath_amd import perceptual

    _, pool = CASES[i]
    inp = inputs(i)
    x = inp["x"].clone().requires_grad_(True)
    pre = split_pre(inp["x"], inp["weight"], inp["bias"], torch.float64)
    out = perceptual.conv3_relu_split_torch(x, inp["weight"], inp["bias"], pool, acc_dtype=torch.float64)
    unsafe = vc.layer_kinks(inp["x"].double(), pre, pool, False)
    up = inp["up"] * ~unsafe
    g_x, = torch.autograd.grad((out * up.double()).sum(), x)
    argmax = vc.windows(F.relu(pre)).argmax(-1) if pool else None
    x64 = inp["x"].double().requires_grad_(True)
    w64, b64 = inp["weight"].double(), inp["bias"].double()
    out64 = perceptual.conv3_relu_torch(x64, w64, b64, pool)
    g_x64, = torch.autograd.grad((out64 * up.double()).sum(), x64)
    return dict(pre=pre, out=out.detach(), up=up, g_x=g_x, argmax=argmax, unsafe=unsafe,
                zeroed=float(unsafe.double().mean()), pre64=F.conv2d(x64.detach(), w64, b64, 1, 1), g_x64=g_x64,
                mass=F.conv2d(x64.detach().abs(), w64.abs(), None, 1, 1))


# ---- the whole loss -----------------------------------------------------------------------------------------------------
LOSS_SEED = 48    # the fp32- and the float64-accumulated split twin agree on every ReLU mask and pool position (so does 7;
                  # seed 90 has one disagreement): asserted in test_vggx_cases.py


def trace(feats, image, dtype):
    """vgg_cases.trace at precision "bf16x3": the layers the split operator supports on the split arithmetic accumulated in
    `dtype`, the others as they are.  (taps, pre-activations, ReLU masks, pool positions)."""
    from goliath_amd import perceptual

    taps, pres, relus, pools = [], [], [], []
    x = image.to(dtype)
    with torch.no_grad():
        for _, weight, bias, pool, image_in, tapped in feats.layers():
            if perceptual.supported(weight.shape[1], weight.shape[0], *x.shape[2:], pool, image_in, "bf16x3"):
                pre = split_pre(x, weight, bias, dtype)
            else:
                pre = F.conv2d(perceptual.normalize(x) if image_in else x, weight.to(dtype), bias.to(dtype), 1, 1)
            pres.append(pre)
            relus.append(pre > 0)
            x = F.relu(pre)
            if pool:
                pools.append(vc.windows(x).argmax(-1))
                x = F.max_pool2d(x, 2)
            if tapped:
                taps.append(x)
    return taps, pres, relus, pools


def loss_twin(dtype, precision="bf16x3"):
    """Loss and image gradient of the loss case on the twin of `precision`, accumulated in `dtype`."""
    from goliath_amd import perceptual

    feats, x, y, mask = vc.loss_case(LOSS_SEED)
    x = x.to(dtype).requires_grad_(True)
    loss = perceptual.vgg_loss_torch(feats, x, y.to(dtype), mask.to(dtype), precision=precision)
    g, = torch.autograd.grad(loss, x)
    return loss.detach(), g


@functools.lru_cache(maxsize=None)
def loss_reference():
    """The float64-accumulated split twin's loss and g_image, and the fp32-accumulated split twin's relative distance from
    them: [loss, g_image]."""
    from scenes import rel_l2

    l64, g64 = loss_twin(torch.float64)
    l32, g32 = loss_twin(torch.float32)
    return l64, g64, [abs(float(l32) - float(l64)) / abs(float(l64)), rel_l2(g32, g64)]
