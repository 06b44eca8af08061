"""Case tables and float64 references of the fused VGG layer (goliath_amd.perceptual: gol_conv3_fwd / gol_conv3_bwd_x) and of
the masked VGG loss, shared by tests/test_vgg_cases.py (CPU), tests/test_gpu_vggconv.py and tests/test_gpu_vgg_loss.py.
All draws are made on the CPU from fixed seeds: weights randn * sqrt(2 / (9 Ci)), bias 0.1 * randn, images uniform in
[-40, 290] so that both clamp branches occur."""
import functools

import torch
import torch.nn.functional as F

KINK = 1e-4    # upstream gradients are zeroed where the float64 twin is closer to a kink than this
BAR = 1e-5     # rel-L2 against float64 (the bar of test_gpu_texdec.py)
ZEROED_CAP = 2e-3

# (B, Ci, Co, H, W), pool, image_in.  The kernel's tile is 8 x 32 pixels x 16 / 32 / 64 channels, K stages of 8 channels.
CASES = [
    ((2, 3, 16, 9, 33), False, True),      # image input: tiles both ways, both clamp branches
    ((2, 8, 16, 8, 32), False, False),     # exactly one tile
    ((2, 16, 48, 18, 37), False, False),   # tiles both ways, odd W, Co not a multiple of 32
    ((3, 24, 32, 7, 5), False, False),     # smaller than a tile, odd batch, Ci not a multiple of 16
    ((1, 72, 64, 17, 34), False, False),   # several K stages with a ragged last one (of 16; nine stages of 8 here)
    ((2, 16, 16, 18, 37), True, False),    # pooled: odd W drops a column
    ((2, 8, 16, 7, 5), True, False),       # pooled: odd H and W drop a row and a column
    ((2, 16, 32, 2, 2), True, False),      # pooled: one window
    ((2, 3, 32, 10, 35), True, True),      # image input with pool (no layer of VGG19; the ABI takes the combination)
]
IDS = ["x".join(map(str, s)) + ("p" if pool else "") + ("i" if img else "") for s, pool, img in CASES]
POOLED = [i for i, c in enumerate(CASES) if c[1]]


def draw_layer(seed, Ci, Co):
    g = torch.Generator().manual_seed(seed)
    weight = torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (9 * Ci)) ** 0.5
    bias = 0.1 * torch.randn(Co, generator=g)
    return weight, bias


def draw_image(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 330.0 - 40.0


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The draws of case i (CPU, float32): x, weight, bias and the upstream gradient of the output."""
    (B, Ci, Co, H, W), pool, image_in = CASES[i]
    weight, bias = draw_layer(700 + i, Ci, Co)
    g = torch.Generator().manual_seed(800 + i)
    x = draw_image(900 + i, (B, Ci, H, W)) if image_in else torch.randn(B, Ci, H, W, generator=g)
    up = torch.randn((B, Co, H // 2, W // 2) if pool else (B, Co, H, W), generator=g)
    return dict(x=x, weight=weight, bias=bias, up=up)


def windows(t):
    """[B,C,H,W] -> [B,C,H/2,W/2,4]: the 2x2 windows of the floor pool, positions row-major."""
    B, C, H, W = t.shape
    Hp, Wp = H // 2, W // 2
    return t[:, :, :2 * Hp, :2 * Wp].reshape(B, C, Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Hp, Wp, 4)


def layer_kinks(x64, pre64, pool, image_in):
    """Boolean mask over the layer's OUTPUT elements whose upstream gradient is zeroed: a pre-activation within KINK of
    0 (with pool: anywhere in the window), the top two values of a live pool window within KINK, an image value within
    KINK of 0 or 255 anywhere under the element's 3x3 taps (with pool: under the window's)."""
    near = pre64.abs() < KINK
    if image_in:
        edge = ((x64.abs() < KINK) | ((x64 - 255.0).abs() < KINK)).any(1, keepdim=True).double()
        near = near | (F.max_pool2d(edge, 3, 1, 1) > 0)
    if not pool:
        return near
    top = windows(F.relu(pre64)).topk(2, -1).values
    close = (top[..., 0] > 0) & (top[..., 0] - top[..., 1] < KINK)
    return close | windows(near).any(-1)


@functools.lru_cache(maxsize=None)
def reference(i):
    """Float64 twin of case i: the output, the position of each window's maximum, the masked upstream gradient, g_x, and
    the share of the output elements whose upstream gradient was zeroed."""
    from goliath_amd import perceptual

    _, pool, image_in = CASES[i]
    inp = inputs(i)
    x64 = inp["x"].double().requires_grad_(True)
    w64, b64 = inp["weight"].double(), inp["bias"].double()
    pre64 = F.conv2d(perceptual.normalize(x64) if image_in else x64, w64, b64, 1, 1)
    out64 = perceptual.conv3_relu_torch(x64, w64, b64, pool, image_in)
    unsafe = layer_kinks(x64.detach(), pre64.detach(), pool, image_in)
    up = inp["up"] * ~unsafe
    g_x, = torch.autograd.grad((out64 * up.double()).sum(), x64)
    argmax = windows(F.relu(pre64.detach())).argmax(-1) if pool else None
    return dict(out=out64.detach(), up=up, g_x=g_x, argmax=argmax, unsafe=unsafe, zeroed=float(unsafe.double().mean()))


# ---- the whole loss -----------------------------------------------------------------------------------------------------
LOSS_WIDTHS = (16, 16, 32, 32, 32)
LOSS_IMAGE = (2, 3, 50, 83)     # 25 x 41, 12 x 20, 6 x 10 and 3 x 5 after the pools
LOSS_SEED = 48                  # chosen among 0..119 for the widest float64 margin (loss_margin), see test_vgg_cases.py


def loss_case(seed):
    """The network (reduced widths), prediction, target and a soft mask with an all-zero region, drawn from `seed`."""
    from goliath_amd import perceptual

    feats = perceptual.Vgg19Features(LOSS_WIDTHS)
    with torch.no_grad():
        for k, (_, weight, bias, _, _, _) in enumerate(feats.layers()):
            w, b = draw_layer(1000 * seed + k, weight.shape[1], weight.shape[0])
            weight.copy_(w)
            bias.copy_(b)
    x = draw_image(1000 * seed + 100, LOSS_IMAGE)
    y = draw_image(1000 * seed + 101, LOSS_IMAGE)
    g = torch.Generator().manual_seed(1000 * seed + 102)
    mask = torch.rand(LOSS_IMAGE[0], 1, *LOSS_IMAGE[2:], generator=g)
    mask[:, :, :, :24] = 0.0
    return feats, x, y, mask


def trace(feats, image, dtype):
    """The network on `image` in `dtype`, layer by layer: (taps, pre-activations, ReLU masks, pool positions)."""
    from goliath_amd import perceptual

    taps, pres, relus, pools = [], [], [], []
    x = image.to(dtype)
    with torch.no_grad():
        for _, weight, bias, pool, image_in, tapped in feats.layers():
            pre = F.conv2d(perceptual.normalize(x) if image_in else x, weight.to(dtype), bias.to(dtype), 1, 1)
            pres.append(pre)
            relus.append(pre > 0)
            x = F.relu(pre)
            if pool:
                pools.append(windows(x).argmax(-1))
                x = F.max_pool2d(x, 2)
            if tapped:
                taps.append(x)
    return taps, pres, relus, pools


def loss_margin(feats, x, y, mask):
    """Smallest distance to a kink of the float64 loss: |pre-activation|, the gap of a live pool window's top two, an image
    value's distance to 0 and 255, and the non-zero masked tap residuals |(vx - vy) m|."""
    margin = []
    traces = [trace(feats, img, torch.float64) for img in (x, y)]
    for img, (taps, pres, _, _) in zip((x, y), traces):
        margin.append(float(img.double().abs().min()))
        margin.append(float((img.double() - 255.0).abs().min()))
        for (_, _, _, pool, _, _), pre in zip(feats.layers(), pres):
            margin.append(float(pre.abs().min()))
            if pool:
                top = windows(F.relu(pre)).topk(2, -1).values
                live = top[..., 0] > 0
                if live.any():
                    margin.append(float((top[..., 0] - top[..., 1])[live].min()))
    for vx, vy in zip(traces[0][0], traces[1][0]):
        m = F.interpolate(mask.double(), size=vx.shape[-2:], mode="bilinear")
        res = ((vx - vy) * m).abs()
        if (res > 0).any():
            margin.append(float(res[res > 0].min()))
    return min(margin)
