"""Case table, draws and references of the split-bf16 4x4 / stride 2 / pad 1 convolution (goliath_amd.featenc.conv4s2,
precision "bf16x3": gol_conv4x_pack / _fwd / _bwd_x / _bwd_w), shared by tests/test_conv4x_cpu.py and tests/test_gpu_conv4x.py.

The reference of the GPU tests is the split twin accumulated in float64 ON THE SAME float32 INPUTS: the splits of identical
inputs are bit-identical, so the operator differs from it by its fp32 summation order alone (about 1e-7), while a kernel that
truncates instead of rounding, or drops a cross term, lands above BAR."""
import functools

import torch
import torch.nn.functional as F

BAR = 1e-5                          # the project's bar (tests/vgg_cases.py, tests/test_gpu_featenc.py)
ELEMENT_BOUND = 3.1 * 2.0 ** -16    # tests/vggx_cases.py: |split - exact| <= this x sum |a||b| for two split operands

# (B, Ci, Co, H, W).  The kernels' tiles: fwd and bwd_x own 8 x 16 OUTPUT pixels (16 x 32 input pixels) x 128 channels written
# (64 where Co <= 64 forward; always 64 in bwd_x, which writes Ci), K stage 32 channels read; bwd_w walks chunks of 32 output
# pixels of one output row, 64 co x 32 ci per workgroup, and splits the chunks over K blocks.  The first five and the K-split
# case are the issue's; the tile here is 8 x 16 where the issue assumed 8 x 32, so the "exactly one tile", "tile + 1" and
# "half-empty channel group" cases are added.
CASES = [
    (2, 32, 32, 2, 2),        # one output pixel, 12 of its 16 taps on the padding, one K stage
    (3, 64, 32, 14, 10),      # output 7 x 5, smaller than any tile, odd batch, two K stages
    (2, 32, 96, 36, 74),      # output 18 x 37: tiles both ways, odd width, 96 = 64 + a ragged 32 forward; bwd_w: 2 chunks a row
    (1, 160, 64, 34, 68),     # five K stages forward; 160 channels written by bwd_x (64 + 64 + a ragged 32); 5 ci groups in bwd_w
    (1, 32, 32, 4, 130),      # output 2 x 65: one column past a tile edge (4 x 16 + 1) and past a chunk (2 x 32 + 1), two rows
    (3, 64, 128, 134, 10),    # bwd_w K split: 3 x 67 x 1 = 201 chunks over 4 channel-tile groups -> 101 blocks of 2, the last
                              # holds 1 (gol_conv4x_bwd_w_scratch_floats = 101 x 16 Co Ci); output 67 rows = 8 tiles + 3
    (1, 32, 32, 16, 32),      # exactly one 8 x 16 tile
    (1, 32, 64, 18, 34),      # tile + 1 both ways: output 9 x 17
    (1, 32, 192, 8, 8),       # Co = 128 + 64: the second channel group's upper two waves own no channel
]
IDS = ["x".join(map(str, c)) for c in CASES]
KSPLIT = 5
KSPLIT_BLOCKS = 101


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The draws of case i (CPU, float32): x, up ~ randn, w ~ randn / sqrt(16 Ci), fixed seeds."""
    B, Ci, Co, H, W = CASES[i]
    g = torch.Generator().manual_seed(4100 + i)
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 4, 4, generator=g) / (16 * Ci) ** 0.5
    up = torch.randn(B, Co, H // 2, W // 2, generator=g)
    return dict(x=x, w=w, up=up)


def products(xs, ws, ups):
    """The three directions as sums over terms in float64: xs, ws, ups are the lists of the operands' parts, aligned per
    term.  -> y = x * w, g_x = up * w, g_w = up * x."""
    y = sum(F.conv2d(a, b, None, 2, 1) for a, b in zip(xs, ws))
    g_x = sum(F.conv_transpose2d(a, b, None, 2, 1) for a, b in zip(ups, ws))
    g_w = sum(torch.nn.grad.conv2d_weight(b, ws[0].shape, a, 2, 1) for a, b in zip(ups, xs))
    return y, g_x, g_w


def parts(t, which):
    """The parts of t ('h' = hi, 'l' = lo of perceptual.split_bf16) named by the string `which`, in float64."""
    from goliath_amd import perceptual

    hi, lo = (v.double() for v in perceptual.split_bf16(t))
    return [{"h": hi, "l": lo}[k] for k in which]


def written_out(i, first="lhh", second="hlh"):
    """The split products of case i written out in float64 in the twin's order of terms, lo hi + hi lo + hi hi with the
    operand pairs (x, w), (up, w), (up, x); other `first` / `second` strings drop or change terms."""
    inp = inputs(i)
    x1, up1 = parts(inp["x"], first), parts(inp["up"], first)
    w2, x2 = parts(inp["w"], second), parts(inp["x"], second)
    y, g_x, _ = products(x1, w2, up1)
    _, _, g_w = products(x2, w2, up1)
    return dict(y=y, g_x=g_x, g_w=g_w)


@functools.lru_cache(maxsize=None)
def reference(i):
    """Case i: the float64-accumulated split twin (y, g_x, g_w through its autograd), plain float64 (y64, g_x64, g_w64) and
    sum |a||b| of each direction for the element bound (m_y, m_g_x, m_g_w)."""
    from goliath_amd import featenc

    inp = inputs(i)
    x, w, up = inp["x"], inp["w"], inp["up"]
    # float64 copies of the float32 draws: the twin splits the same bits and hands the gradients back in float64
    xt, wt = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = featenc.conv4s2_split_torch(xt, wt, acc_dtype=torch.float64)
    g_x, g_w = torch.autograd.grad((y * up.double()).sum(), (xt, wt))
    x64, w64, u64 = x.double(), w.double(), up.double()
    y64, g_x64, g_w64 = products([x64], [w64], [u64])
    m_y, m_g_x, m_g_w = products([x64.abs()], [w64.abs()], [u64.abs()])
    return dict(y=y.detach(), g_x=g_x, g_w=g_w, y64=y64, g_x64=g_x64, g_w64=g_w64, m_y=m_y, m_g_x=m_g_x, m_g_w=m_g_w)


# ---- the whole encoder ----------------------------------------------------------------------------------------------------
def encoder(dtype=torch.float32, seed=11):
    """FeatEncoderUNet(1, 3, 16, base=32): channels 32 / 96 / 192 / 192 / 384, all multiples of 32, for a 64 x 64 input."""
    from goliath_amd import featenc

    torch.manual_seed(seed)
    fe = featenc.FeatEncoderUNet(1, 3, 16, base=32)
    with torch.no_grad():
        for m in fe.modules():
            if isinstance(m, featenc.ConvWN):
                m.weight_g.mul_(torch.rand_like(m.weight_g) + 0.5)
        fe.enc.bias.normal_(0, 0.3)
    return fe.to(dtype)


def encoder_input(B=2):
    return torch.randn(B, 4, 64, 64, generator=torch.Generator().manual_seed(4200))


def encoder_run(fe, x, run):
    """(z, gb, parameter gradients by name) of run(fe, x) under fixed random upstream gradients (z first, then gb in order)."""
    z, gb = run(fe, x)
    outs = [z] + list(gb)
    g = torch.Generator().manual_seed(4201)
    loss = sum((o * torch.randn(o.shape, generator=g).to(o)).sum() for o in outs)
    names, params = zip(*fe.named_parameters())
    grads = torch.autograd.grad(loss, params)
    return z.detach(), [t.detach() for t in gb], dict(zip(names, grads))


def worst(got, want):
    """The largest rel-L2 of a list or dict of tensors against its counterpart."""
    if isinstance(got, dict):
        return max(rel_l2(got[k], want[k]) for k in want)
    return max(rel_l2(a, b) for a, b in zip(got, want))
