"""Case table, draws and references of the split-bf16 texture-decoder layer (goliath_amd.texdec.upconv_lrelu / upconv_gated at
precision "bf16x3": gol_upconvx_*), shared by tests/test_upconvx_cpu.py and tests/test_gpu_upconvx.py.

The reference of the GPU tests is the split twin accumulated in float64 ON THE SAME float32 INPUTS: U is blended in float32 by
the same expression and the splits of identical values are bit-identical, so the operator differs from it by its fp32
summation order (and the contraction of the blend into fused multiply-adds) alone, about 1e-7, while a kernel that truncates
instead of rounding, or drops a cross term, lands above BAR.  Plain float64 is U (F.interpolate, align_corners=True) and the
convolution in float64: texdec.upconv_lrelu_torch / upconv_gated_torch.

Mode 0's gradients go through the activation's sign; tests/conv3ub_cases.py explains why every comparison of them is made
under ONE sign mask handed to both sides (`gradients(i, variant, positive)`): the operator's own on the GPU, the float64
reference's on the CPU; how far two masks may differ is a test of its own (`NEAR_ZERO`, `SIGN_CAP`)."""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

from conv3ub_cases import BAR, ELEMENT_BOUND, LEAK, NEAR_ZERO, SIGN_CAP, parts, rel_l2  # the project's values: 1e-5,
#                                                                   3.1 x 2^-16, 0.2, 1e-5, 1e-3

SCALE = 0.707107

# (B, Ci, Co, Hi, Wi) of the layer INPUT; the output is 2 Hi x 2 Wi.  The tiles this table assumes: fwd owns 8 x 32 output
# pixels x 16 CT channels (CT = 1 for Co = 16, 2 for 32, else 4 in groups of 64), K stage 32 channels; bwd_x owns 2 x 14
# TEXELS of x (its region of g_U is one 8 x 32 tile) x 32 or 64 input channels; bwd_w walks chunks of 32 pixels of one output
# row, 64 co x 32 ci per workgroup, and splits the chunks over K blocks.
CASES = [
    (2, 32, 16, 1, 1),       # output 2 x 2; every tap on the padding; Hi - 1 = 0: frac 0, r1 = r0; the CT = 1 path
    (3, 64, 32, 3, 5),       # smaller than a tile; odd batch; two K stages; CT = 2; one texel row past bwd_x's tile
    (1, 32, 64, 4, 16),      # exactly one 8 x 32 output tile; CT = 4
    (1, 32, 48, 5, 17),      # output 10 x 34: one row pair and one column pair past a tile; rows past Co in a 64-row group
    (2, 128, 64, 9, 18),     # four K stages; tiles both ways; bwd_x writes 128 rows
    (1, 256, 128, 2, 3),     # the deepest channel pair: eight K stages, two output-channel groups
    (1, 32, 16, 33, 20),     # output 66 x 40: nine tile rows with a ragged last; H != W; the last row and column clamp r1
    (1, 32, 16, 3, 15),      # bwd_x: one texel past its 2 x 14 tile in each direction
    (2, 64, 128, 67, 10),    # the bwd_w K split: 2 x 134 x 1 = 268 chunks over 4 channel-tile pairs -> 90 blocks of 3, the
                             # last holds 1
]
IDS = ["x".join(map(str, c)) for c in CASES]
KSPLIT = 8
KSPLIT_BLOCKS = 90
VARIANTS = ("lrelu", "gated_gb", "gated")     # mode 0; mode 1 with and without gainbias
PARAMS = [(i, v) for i in range(len(CASES)) for v in VARIANTS]
PARAM_IDS = [IDS[i] + "-" + v for i, v in PARAMS]


def bwd_w_blocks(B, Ci, Co, Hi, Wi):
    """The K blocks of gol_upconvx_bwd_w by its documented formula: chunks of 32 pixels of an output row, aimed at 512
    workgroups over the (Ci / 32) x ceil(Co / 64) channel-tile pairs, no empty block."""
    cdiv = lambda a, b: -(-a // b)
    nchunks = B * 2 * Hi * cdiv(2 * Wi, 32)
    pairs = (Ci // 32) * cdiv(Co, 64)
    nblk = max(1, min(cdiv(512, pairs), nchunks))
    return cdiv(nchunks, cdiv(nchunks, nblk))


@functools.lru_cache(maxsize=None)
def inputs(i):
    """The draws of case i (CPU, float32): x, gate, gb, up ~ randn, w ~ randn / sqrt(9 Ci), bias ~ 0.3 randn, fixed seeds."""
    B, Ci, Co, Hi, Wi = CASES[i]
    g = torch.Generator().manual_seed(5300 + i)
    x = torch.randn(B, Ci, Hi, Wi, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5
    bias = 0.3 * torch.randn(Co, 2 * Hi, 2 * Wi, generator=g)
    gate = torch.randn(B, Co, 2 * Hi, 2 * Wi, generator=g)
    gb = torch.randn(B, Co, 2 * Hi, 2 * Wi, generator=g)
    up = torch.randn(B, Co, 2 * Hi, 2 * Wi, generator=g)
    return dict(x=x, w=w, bias=bias, gate=gate, gb=gb, up=up)


def names(variant):
    """The differentiable inputs of a variant, in the operator's argument order."""
    return {"lrelu": ("x", "w", "bias"), "gated_gb": ("x", "w", "gate", "gb"), "gated": ("x", "w", "gate")}[variant]


def keys(variant):
    return ("y",) + tuple("g_" + n for n in names(variant))


def call(variant, op_lrelu, op_gated, t, **kw):
    """The variant's operator on the tensors t (a dict by `names`)."""
    if variant == "lrelu":
        return op_lrelu(t["x"], t["w"], t["bias"], LEAK, **kw)
    return op_gated(t["x"], t["w"], t["gate"], t.get("gb") if variant == "gated_gb" else None, SCALE, **kw)


def up64(x):
    return F.interpolate(x, (2 * x.shape[2], 2 * x.shape[3]), mode="bilinear", align_corners=True)


def g_pre32(inp, variant, positive):
    """g_pre as the kernels form it, in float32: y > 0 ? g : leak g (mode 0), (scale g) gate (mode 1)."""
    if variant == "lrelu":
        return torch.where(positive, inp["up"], LEAK * inp["up"])
    return (SCALE * inp["up"]) * inp["gate"]


def products(us, ws, gs, u_for_w=None):
    """The three convolutions as sums over terms in float64: us, ws, gs are the lists of the operands' parts, aligned per
    term.  -> acc = U * w, g_U = g * w, g_w = g * U (u_for_w: U's parts in g_w's order of terms)."""
    acc = sum(F.conv2d(a, b, None, 1, 1) for a, b in zip(us, ws))
    g_U = sum(F.conv_transpose2d(a, b, None, 1, 1) for a, b in zip(gs, ws))
    g_w = sum(torch.nn.grad.conv2d_weight(b, ws[0].shape, a, 1, 1) for a, b in zip(gs, us if u_for_w is None else u_for_w))
    return acc, g_U, g_w


def adjoint64(x_shape, g_U):
    """The bilinear adjoint in float64 through the library's own autograd."""
    leaf = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(up64(leaf), leaf, g_U)[0]


def finish(inp, variant, acc, g_U, g_w, g_pre, adjoint=None):
    """y and the gradients of a variant from its three convolutions (float64 epilogues)."""
    up = inp["up"].double()
    out = dict(acc=acc, g_w=g_w, g_x=(adjoint or (lambda g: adjoint64(inp["x"].shape, g)))(g_U))
    if variant == "lrelu":
        pre = acc + inp["bias"].double()[None]
        out.update(pre=pre, y=torch.where(pre > 0, pre, LEAK * pre), g_bias=g_pre.double().sum(0))
    else:
        y = acc * inp["gate"].double()
        if variant == "gated_gb":
            y = y + inp["gb"].double()
            out["g_gb"] = (SCALE * inp["up"]).double()
        out.update(y=y * SCALE, g_gate=(SCALE * inp["up"]).double() * acc)
    return out


def rule_adjoint(inp):
    """The twin's own adjoint (texdec._rule_matrix in float64)."""
    from goliath_amd import texdec

    Hi, Wi = inp["x"].shape[2:]
    R, C = texdec._rule_matrix(Hi, "cpu", torch.float64), texdec._rule_matrix(Wi, "cpu", torch.float64)
    return lambda g_U: torch.einsum("ri,bkrc,cj->bkij", R, g_U, C)


def written_out(i, variant, positive, first="lhh", second="hlh"):
    """The split products of case i written out in float64 in the twin's order of terms, lo hi + hi lo + hi hi with the operand
    pairs (U, w), (g_pre, w), (g_pre, U), U blended in float32 by the rule; other `first` / `second` strings drop or change
    terms."""
    from goliath_amd import texdec

    inp = inputs(i)
    U, g_pre = texdec.up2_rule(inp["x"]), g_pre32(inp, variant, positive)
    u1, g1 = parts(U, first), parts(g_pre, first)
    w2, u2 = parts(inp["w"], second), parts(U, second)
    return finish(inp, variant, *products(u1, w2, g1, u2), g_pre, rule_adjoint(inp))


def truncated(i, variant, positive):
    """The split with both conversions TRUNCATED to bf16 (round toward zero) instead of rounded (tests/conv3ub_cases.py)."""
    from goliath_amd import texdec

    def split(t):
        chop = lambda v: (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
        hi = chop(t)
        return [hi.double(), chop(t - hi).double()]

    inp = inputs(i)
    U, g_pre = texdec.up2_rule(inp["x"]), g_pre32(inp, variant, positive)
    (uh, ul), (wh, wl), (gh, gl) = split(U), split(inp["w"]), split(g_pre)
    return finish(inp, variant, *products([ul, uh, uh], [wh, wl, wh], [gl, gh, gh], [uh, ul, uh]), g_pre, rule_adjoint(inp))


@functools.lru_cache(maxsize=None)
def forward64(i, variant):
    """Plain float64 of case i: y (and pre in mode 0) of texdec.upconv_*_torch on float64 copies."""
    from goliath_amd import texdec

    inp = inputs(i)
    t = {k: inp[k].double() for k in names(variant)}
    y = call(variant, texdec.upconv_lrelu_torch, texdec.upconv_gated_torch, t)
    out = dict(y=y)
    if variant == "lrelu":
        out["pre"] = F.conv2d(up64(t["x"]), t["w"], None, 1, 1) + t["bias"][None]
    return out


def gradients(i, variant, positive=None):
    """Case i under the sign mask `positive` (mode 0: bool [B,Co,H,W], CPU): the float64-accumulated split twin through its
    autograd (`keys(variant)`), plain float64 (the same keys + "64") and sum |a||b| of each convolution (m_*)."""
    from goliath_amd import texdec

    inp = inputs(i)
    # float64 copies of the float32 draws: the twin splits the same bits and hands the gradients back in float64
    leaves = {k: inp[k].double().requires_grad_(True) for k in names(variant)}
    kw = dict(acc_dtype=torch.float64)
    if variant == "lrelu":
        kw["y_sign"] = positive
    y = call(variant, texdec.upconv_lrelu_split_torch, texdec.upconv_gated_split_torch, leaves, **kw)
    grads = torch.autograd.grad((y * inp["up"].double()).sum(), list(leaves.values()))
    out = dict(y=y.detach(), **{"g_" + k: g for k, g in zip(leaves, grads)})
    U64, w64 = up64(inp["x"].double()), inp["w"].double()
    g64 = g_pre32(inp, variant, positive).double() if variant == "lrelu" else (SCALE * inp["up"].double()) * inp["gate"].double()
    plain = finish(inp, variant, *products([U64], [w64], [g64]), g64)
    m_acc, m_gU, m_gw = products([U64.abs()], [w64.abs()], [g64.abs()])
    out.update({k + "64": plain[k] for k in keys(variant)})
    out.update(m_y=m_acc * (1.0 if variant == "lrelu" else SCALE * inp["gate"].double().abs()),
               m_g_x=adjoint64(inp["x"].shape, m_gU), m_g_w=m_gw)
    if variant != "lrelu":
        out["m_g_gate"] = (SCALE * inp["up"].double()).abs() * m_acc
    return out


@functools.lru_cache(maxsize=None)
def reference(i, variant):
    """`gradients` of case i under the float64 reference's own sign (the CPU tests' reference; its y and y64 are what the
    GPU tests compare the forward against)."""
    return gradients(i, variant, forward64(i, variant)["pre"] > 0 if variant == "lrelu" else None)


def near_zero(i):
    """The elements of case i (mode 0) whose float64 pre lies within NEAR_ZERO x rms(pre) of zero: where a sign may differ."""
    pre = forward64(i, "lrelu")["pre"]
    return pre.abs() < NEAR_ZERO * pre.pow(2).mean().sqrt()


# ---- a small stack -----------------------------------------------------------------------------------------------------
STACK_CHANNELS = (32, 64, 32, 16)
STACK_SHAPES = [(32, 64, 4, 4), (64, 32, 8, 8), (32, 16, 16, 16)]     # (Ci, Co, Hi, Wi) of the three layers of a branch


class SmallTexDecoder(nn.Module):
    """The texture-branch attributes of ConvTeacherDecoder (urhand.py:302-323) at three layers from 4^2: channels
    (32, 64, 32, 16) in both branches, built from texdec.Conv3WNUB / Conv3WN."""

    def __init__(self, seed=23):
        from goliath_amd import texdec

        super().__init__()
        torch.manual_seed(seed)
        ch = STACK_CHANNELS
        self.n_layers_tex = len(ch) - 1
        self.texmod0 = nn.ModuleList([texdec.Conv3WNUB(ch[k], ch[k + 1], 8 << k, 8 << k) for k in range(self.n_layers_tex)])
        self.texmod1 = nn.ModuleList([texdec.Conv3WN(ch[k], ch[k + 1]) for k in range(self.n_layers_tex)])
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, (texdec.Conv3WNUB, texdec.Conv3WN)):
                    m.weight_g.mul_(torch.rand_like(m.weight_g) + 0.5)
                if isinstance(m, texdec.Conv3WNUB):
                    m.bias.normal_(0, 0.3)


def stack(dtype=torch.float32):
    return SmallTexDecoder().to(dtype)


def stack_inputs(B=2):
    """joint_feat, z and the gainbias of the first two layers."""
    g = torch.Generator().manual_seed(5400)
    ch = STACK_CHANNELS
    return (torch.randn(B, ch[0], 4, 4, generator=g), torch.randn(B, ch[0], 4, 4, generator=g),
            [torch.randn(B, ch[k + 1], 8 << k, 8 << k, generator=g) for k in range(2)])


def library_loops(dec, joint_feat, z, gainbias, first_size=8):
    """urhand.py:583-608 as the parent commit runs it where no layer is dispatched."""
    acts, x, hh = [], joint_feat, first_size
    for i in range(dec.n_layers_tex):
        x = F.interpolate(x, (hh, hh), mode="bilinear", align_corners=True)
        x = F.leaky_relu(dec.texmod0[i](x), 0.2)
        acts.append(x)
        hh *= 2
    x, hh = z, first_size
    for i in range(dec.n_layers_tex):
        x = F.interpolate(x, (hh, hh), mode="bilinear", align_corners=True)
        x = dec.texmod1[i](x) * acts[i]
        hh *= 2
        if i < len(gainbias):
            x = (x + gainbias[i]) * 0.707107
    return x


def twin_loops(dec, joint_feat, z, gainbias, first_size=8, acc_dtype=torch.float64):
    """The same two loops with every layer on the split twins accumulated in `acc_dtype` (the effective weight through
    tail.wn_weight, as texture_branches forms it)."""
    from goliath_amd import texdec
    from goliath_amd.tail import wn_weight

    acts, x = [], joint_feat
    for i in range(dec.n_layers_tex):
        layer = dec.texmod0[i]
        x = texdec.upconv_lrelu_split_torch(x, wn_weight(layer), layer.bias, 0.2, acc_dtype).to(joint_feat.dtype)
        acts.append(x)
    x = z
    for i in range(dec.n_layers_tex):
        gb = gainbias[i] if i < len(gainbias) else None
        x = texdec.upconv_gated_split_torch(x, wn_weight(dec.texmod1[i]), acts[i], gb,
                                            texdec.GAIN_SCALE if gb is not None else 1.0, acc_dtype).to(z.dtype)
    return x


def stack_run(dec, joint_feat, z, gainbias, run):
    """(output, input gradients by name, parameter gradients by name) of run(dec, joint_feat, z, gainbias) under a fixed
    random upstream gradient."""
    ins = dict(joint_feat=joint_feat.clone().requires_grad_(True), z=z.clone().requires_grad_(True),
               **{"gainbias%d" % k: g.clone().requires_grad_(True) for k, g in enumerate(gainbias)})
    out = run(dec, ins["joint_feat"], ins["z"], [ins["gainbias%d" % k] for k in range(len(gainbias))])
    up = torch.randn(out.shape, generator=torch.Generator().manual_seed(5401)).to(out)
    pnames, params = zip(*dec.named_parameters())
    grads = torch.autograd.grad((out * up).sum(), tuple(ins.values()) + params)
    return out.detach(), dict(zip(ins, grads[:len(ins)])), dict(zip(pnames, grads[len(ins):]))
