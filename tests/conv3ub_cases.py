"""Case table, draws and references of the split-bf16 3x3 convolution of two sources + untied bias + LeakyReLU
(goliath_amd.olatunet.conv3_ub_lrelu, precision "bf16x3": gol_conv3ub_*), shared by tests/test_conv3ub_cpu.py and
tests/test_gpu_conv3ub.py.

The reference of the GPU tests is the split twin accumulated in float64 ON THE SAME float32 INPUTS: the splits of identical
inputs are bit-identical, so the operator differs from it by its fp32 summation order alone (about 1e-7), while a kernel that
truncates instead of rounding, or drops a cross term, lands above BAR.

The gradients go through the activation's sign.  Two computations of `pre` that differ in the last bits disagree about the
sign of an element that lies within rounding of zero, and ONE such element moves a gradient by (1 - leak) g there: 2e-3
rel-L2 in g_bias at these sizes.  That is a property of the activation, not of either computation, so every comparison of
gradients is made under ONE sign mask handed to both sides (`gradients(i, positive)`): the operator's own on the GPU, the
float64 reference's on the CPU; how far two masks may differ is a test of its own (`NEAR_ZERO`, `SIGN_CAP`)."""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

BAR = 1e-5                          # the project's bar (tests/vgg_cases.py, tests/conv4x_cases.py)
ELEMENT_BOUND = 3.1 * 2.0 ** -16    # tests/vggx_cases.py: |split - exact| <= this x sum |a||b| for two split operands
LEAK = 0.2
NEAR_ZERO = 1e-5                    # signs may differ only where |pre64| < NEAR_ZERO x rms(pre64) ...
SIGN_CAP = 1e-3                     # ... and at no more than this share of a case's elements

# (B, Ca, Cb, Co, H, W).  The kernels' tiles are the ones the issue assumed: fwd and bwd_x own 8 x 32 pixels x 64 channels
# written (32 where only 32 are written), K stage 32 channels read from ONE source; bwd_w walks chunks of 32 pixels of one
# row, 64 co x 32 ci per workgroup, and splits the chunks over K blocks.  So the issue's table covers them as it stands.
CASES = [
    (2, 32, 0, 32, 1, 1),       # one pixel, 8 of 9 taps on the padding
    (3, 56, 0, 64, 7, 5),       # ragged K stage 32 + 24; smaller than a tile; odd batch; bwd_x writes 56 rows
    (2, 64, 64, 32, 18, 37),    # two sources; tiles both ways; odd width; the Co = 32 path
    (1, 32, 32, 96, 9, 33),     # tile + 1 both ways; Co = 64 + a ragged 32; bwd_x's one group holds rows of xa AND of xb
    (1, 64, 0, 64, 8, 32),      # exactly one tile
    (1, 160, 0, 64, 10, 34),    # five K stages; bwd_x writes 64 + 64 + 32 rows; five ci groups in bwd_w
    (1, 32, 24, 32, 6, 40),     # ragged second source
    (3, 64, 64, 64, 67, 10),    # the bwd_w K split: 3 x 67 x 1 = 201 chunks over 4 channel-tile pairs -> 101 blocks of 2, the
                                # last holds 1
]
IDS = ["x".join(map(str, c)) for c in CASES]
KSPLIT = 7
KSPLIT_BLOCKS = 101


def bwd_w_blocks(B, Ca, Cb, Co, H, W):
    """The K blocks of gol_conv3ub_bwd_w by its documented formula: chunks of 32 pixels of a row, aimed at 512 workgroups
    over the (Cip / 32) x ceil(Co / 64) channel-tile pairs, no empty block."""
    cdiv = lambda a, b: -(-a // b)
    nchunks = B * H * cdiv(W, 32)
    pairs = cdiv(Ca + Cb, 32) * cdiv(Co, 64)
    nblk = max(1, min(cdiv(512, pairs), nchunks))
    return cdiv(nchunks, cdiv(nchunks, nblk))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The draws of case i (CPU, float32): xa, xb (None where Cb = 0), up ~ randn, w ~ randn / sqrt(9 Ci),
    bias ~ 0.3 randn, fixed seeds."""
    B, Ca, Cb, Co, H, W = CASES[i]
    g = torch.Generator().manual_seed(5100 + i)
    xa = torch.randn(B, Ca, H, W, generator=g)
    xb = torch.randn(B, Cb, H, W, generator=g) if Cb else None
    w = torch.randn(Co, Ca + Cb, 3, 3, generator=g) / (9 * (Ca + Cb)) ** 0.5
    bias = 0.3 * torch.randn(Co, H, W, generator=g)
    up = torch.randn(B, Co, H, W, generator=g)
    return dict(xa=xa, xb=xb, w=w, bias=bias, up=up)


def xcat(inp):
    return inp["xa"] if inp["xb"] is None else torch.cat([inp["xa"], inp["xb"]], 1)


def parts(t, which):
    """The parts of t ('h' = hi, 'l' = lo of perceptual.split_bf16) named by the string `which`, in float64."""
    from goliath_amd import perceptual

    hi, lo = (v.double() for v in perceptual.split_bf16(t))
    return [{"h": hi, "l": lo}[k] for k in which]


def g_pre32(up, positive):
    """g_pre as the kernels form it: float32, y > 0 ? g : leak g."""
    return torch.where(positive, up, LEAK * up)


def products(xs, ws, gs):
    """The three convolutions as sums over terms in float64: xs, ws, gs are the lists of the operands' parts, aligned per
    term.  -> pre - bias = x * w, g_x = g * w, g_w = g * x."""
    conv = sum(F.conv2d(a, b, None, 1, 1) for a, b in zip(xs, ws))
    g_x = sum(F.conv_transpose2d(a, b, None, 1, 1) for a, b in zip(gs, ws))
    g_w = sum(torch.nn.grad.conv2d_weight(b, ws[0].shape, a, 1, 1) for a, b in zip(gs, xs))
    return conv, g_x, g_w


def _finish(inp, conv, g_x, g_w, g_pre):
    Ca = inp["xa"].shape[1]
    pre = conv + inp["bias"].double()[None]
    return dict(pre=pre, y=torch.where(pre > 0, pre, LEAK * pre), g_xa=g_x[:, :Ca], g_xb=g_x[:, Ca:], g_w=g_w,
                g_bias=g_pre.double().sum(0))


def written_out(i, positive, first="lhh", second="hlh"):
    """The split products of case i written out in float64 in the twin's order of terms, lo hi + hi lo + hi hi with the
    operand pairs (x, w), (g_pre, w), (g_pre, x); other `first` / `second` strings drop or change terms."""
    inp = inputs(i)
    x, g_pre = xcat(inp), g_pre32(inp["up"], positive)
    x1, g1 = parts(x, first), parts(g_pre, first)
    w2, x2 = parts(inp["w"], second), parts(x, second)
    conv, g_x, _ = products(x1, w2, g1)
    _, _, g_w = products(x2, w2, g1)
    return _finish(inp, conv, g_x, g_w, g_pre)


def truncated(i, positive):
    """The split with both conversions TRUNCATED to bf16 (round toward zero) instead of rounded: what a kernel that takes the
    upper 16 bits of a float would compute.  The remainder v - hi - lo then has v's sign for every operand (about
    (0.72 x 2^-8)^2 = 8e-6 |v| on average), so the errors of a sum's terms add up instead of cancelling."""
    def split(t):
        chop = lambda v: (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
        hi = chop(t)
        return [hi.double(), chop(t - hi).double()]

    inp = inputs(i)
    x, g_pre = xcat(inp), g_pre32(inp["up"], positive)
    (xh, xl), (wh, wl), (gh, gl) = split(x), split(inp["w"]), split(g_pre)
    conv, g_x, _ = products([xl, xh, xh], [wh, wl, wh], [gl, gh, gh])
    _, _, g_w = products([xh, xl, xh], [wh, wl, wh], [gl, gh, gh])
    return _finish(inp, conv, g_x, g_w, g_pre)


KEYS = ("y", "g_xa", "g_xb", "g_w", "g_bias")


@functools.lru_cache(maxsize=None)
def forward64(i):
    """Plain float64 of case i: pre and y."""
    inp = inputs(i)
    pre = F.conv2d(xcat(inp).double(), inp["w"].double(), None, 1, 1) + inp["bias"].double()[None]
    return dict(pre=pre, y=torch.where(pre > 0, pre, LEAK * pre))


def gradients(i, positive):
    """Case i under the sign mask `positive` (bool [B,Co,H,W], CPU): the float64-accumulated split twin through its autograd
    (y, g_xa, g_xb, g_w, g_bias), plain float64 (the same keys + "64") and sum |a||b| of each convolution (m_*)."""
    from goliath_amd import olatunet

    inp = inputs(i)
    # float64 copies of the float32 draws: the twin splits the same bits and hands the gradients back in float64
    leaves = {k: inp[k].double().requires_grad_(True) for k in ("xa", "xb", "w", "bias") if inp[k] is not None}
    y = olatunet.conv3_ub_lrelu_split_torch(leaves["xa"], leaves.get("xb"), leaves["w"], leaves["bias"], LEAK,
                                            acc_dtype=torch.float64, y_sign=positive)
    grads = dict(zip(leaves, torch.autograd.grad((y * inp["up"].double()).sum(), list(leaves.values()))))
    out = dict(y=y.detach(), g_xa=grads["xa"], g_xb=grads.get("xb"), g_w=grads["w"], g_bias=grads["bias"])
    x64, w64 = xcat(inp).double(), inp["w"].double()
    g64 = torch.where(positive, inp["up"].double(), LEAK * inp["up"].double())
    plain = _finish(inp, *products([x64], [w64], [g64]), g64)
    mass = products([x64.abs()], [w64.abs()], [g64.abs()])
    Ca = inp["xa"].shape[1]
    out.update({k + "64": plain[k] for k in KEYS})
    out.update(m_y=mass[0], m_g_xa=mass[1][:, :Ca], m_g_xb=mass[1][:, Ca:], m_g_w=mass[2])
    if inp["xb"] is None:
        out["g_xb64"] = None
    return out


@functools.lru_cache(maxsize=None)
def reference(i):
    """`gradients` of case i under the float64 reference's own sign (the CPU tests' reference; its y and y64 are what the
    GPU tests compare the forward against)."""
    return gradients(i, forward64(i)["pre"] > 0)


def near_zero(i):
    """The elements of case i whose float64 pre lies within NEAR_ZERO x rms(pre) of zero: where a sign may differ."""
    pre = forward64(i)["pre"]
    return pre.abs() < NEAR_ZERO * pre.pow(2).mean().sqrt()


# ---- the whole UNet -------------------------------------------------------------------------------------------------------
class SmallOLATUNet(nn.Module):
    """The UNet attributes of OLATRGBDecoder (hand_teacher_mvp.py:185-241) at three levels of 32^2 / 16^2 / 8^2: encoder
    56 -> 32 -> 32 -> 32, decoder (32 + 32) -> 32 three times; joint_feat has 32 channels at 8^2."""

    def __init__(self, seed=21):
        from goliath_amd import texdec

        super().__init__()
        torch.manual_seed(seed)
        self.sizes = [32, 16, 8]
        level = lambda ci, co, s: nn.Sequential(texdec.Conv3WNUB(ci, co, s, s), nn.LeakyReLU(0.2, inplace=True))
        self.enc_layers = nn.ModuleList([level(56, 32, 32), level(32, 32, 16), level(32, 32, 8)])
        self.dec_layers = nn.ModuleList([level(64, 32, 8), level(64, 32, 16), level(64, 32, 32)])
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, texdec.Conv3WNUB):
                    m.weight_g.mul_(torch.rand_like(m.weight_g) + 0.5)
                    m.bias.normal_(0, 0.3)


UNET_SHAPES = [(56, 0, 32, 32, 32), (32, 0, 32, 16, 16), (32, 0, 32, 8, 8), (32, 32, 32, 8, 8), (32, 32, 32, 16, 16),
               (32, 32, 32, 32, 32)]


def unet(dtype=torch.float32):
    return SmallOLATUNet().to(dtype)


def unet_inputs(B=2):
    g = torch.Generator().manual_seed(5200)
    return torch.randn(B, 56, 32, 32, generator=g), torch.randn(B, 32, 8, 8, generator=g)


def module_loop(dec, x, joint_feat):
    """hand_teacher_mvp.py:444-467 as the parent commit runs it (goliath_amd.urhand.olat_rgb_decoder_forward_rgb)."""
    enc_acts = []
    for i, layer in enumerate(dec.enc_layers):
        x = layer(x)
        enc_acts.append(x)
        if i < len(dec.sizes) - 1:
            x = F.interpolate(x, scale_factor=0.5, mode="bilinear", recompute_scale_factor=True, align_corners=True)
    for i, layer in enumerate(dec.dec_layers):
        if i == 0:
            x = torch.cat([x, joint_feat], dim=1)
        else:
            skip = enc_acts[-i - 1]
            x = torch.cat([F.interpolate(x, size=skip.shape[2:4], mode="bilinear", align_corners=True), skip], dim=1)
        x = layer(x)
    return x


def unet_run(dec, x, joint_feat, run):
    """(output, joint_feat gradient, parameter gradients by name) of run(dec, x, joint_feat) under a fixed random upstream
    gradient."""
    joint_feat = joint_feat.clone().requires_grad_(True)
    out = run(dec, x, joint_feat)
    up = torch.randn(out.shape, generator=torch.Generator().manual_seed(5201)).to(out)
    names, params = zip(*dec.named_parameters())
    grads = torch.autograd.grad((out * up).sum(), (joint_feat,) + params)
    return out.detach(), grads[0], dict(zip(names, grads[1:]))
