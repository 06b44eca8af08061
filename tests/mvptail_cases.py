"""Shapes, draws and the float64 reference of the mvptail tests (no tests in here)."""
import functools

import torch

# (B, TD, TH, TW, ny, nx)
SHAPES = [
    (2, 8, 16, 16, 2, 2),    # the model's primitive; h = w = 16: 17 quads per row, one over a tile of 16
    (1, 1, 2, 2, 1, 1),      # h = w = 1: every tap overhangs; CH = 3 / 1
    (3, 3, 3, 5, 2, 2),      # odd TH and TW: primitive boundaries on both quad parities; CH = 9; odd batch
    (2, 8, 4, 8, 5, 9),      # h = 10, w = 36: three ragged quad tiles per row; 45 primitives for the masks
    (1, 5, 16, 16, 1, 3),    # CH = 15, one short of a row tile
    (9, 2, 2, 4, 3, 2),      # a batch above any per-pass view count
    (2, 10, 4, 4, 2, 2),     # 3 TD = 30, the top of the range
]
MASK_SHAPE = 3               # index of the 45-primitive shape
MASKS = ("all", "ends", "one", "none")
AFFINE = (25.0, 100.0)
SCREEN_RGB, SCREEN_ALPHA = 1e-3, 1e-4


def primsize(shape):
    _, TD, TH, TW, _, _ = shape
    return (TW, TH, TD)


def mask_of(kind, K):
    """all valid / first, last and three interior primitives dropped / only one kept / none kept"""
    m = torch.ones(K, dtype=torch.bool)
    if kind == "ends":
        m[[0, K - 1, K // 4, K // 2, K // 2 + 1]] = False
    elif kind == "one":
        m[:] = False
        m[K // 3] = True
    elif kind == "none":
        m[:] = False
    return m


def _wn(v, g):
    """the effective weight of a weight-normalised layer: one magnitude per output channel, direction normalised over the
    whole tensor"""
    return v * (g / v.norm())


@functools.lru_cache(maxsize=None)
def draws(i):
    """float64 leaves of shape i, drawn in float32 in a fixed order: x_rgb, x_alpha, (v, g) of rgb, (v, g) of alpha, the two
    biases, the upstream gradient (full K, four channels).  Shared by the tests: never written."""
    B, TD, TH, TW, ny, nx = SHAPES[i]
    h, w = ny * TH // 2, nx * TW // 2
    torch.manual_seed(500 + i)
    x_rgb, x_alpha = torch.randn(B, 16, h, w), torch.randn(B, 16, h, w)
    ws = []
    for CH in (3 * TD, TD):
        v, g = torch.randn(16, CH, 4, 4), 0.5 + torch.rand(1, CH, 1, 1)
        ws.append(8.0 * _wn(v, g))
    bias_rgb = -4.0 + 0.05 * torch.randn(3 * TD, 2 * h, 2 * w)
    bias_alpha = 0.3 * torch.randn(TD, 2 * h, 2 * w)
    g_out = torch.randn(B, ny * nx, TD, TH, TW, 4)
    d = dict(x_rgb=x_rgb, w_rgb=ws[0], bias_rgb=bias_rgb, x_alpha=x_alpha, w_alpha=ws[1], bias_alpha=bias_alpha, g_out=g_out)
    return {k: v.double() for k, v in d.items()}


LEAVES = ("x_rgb", "w_rgb", "bias_rgb", "x_alpha", "w_alpha", "bias_alpha")


def to_template(slab, shape):
    """[B,TD,C,Sy,Sx] -> [B,K,TD,TH,TW,C], the reference's view / permute(0,3,5,1,4,6,2) / reshape"""
    B, TD, TH, TW, ny, nx = shape
    C = slab.shape[2]
    return slab.view(B, TD, C, ny, TH, nx, TW).permute(0, 3, 5, 1, 4, 6, 2).reshape(B, ny * nx, TD, TH, TW, C)


@functools.lru_cache(maxsize=None)
def reference(i):
    """float64: the pre-activations in template layout, the kink screen (1 = keep) and the upstream gradient with the
    screened elements zeroed.  All full K, four channels."""
    import torch.nn.functional as F

    shape = SHAPES[i]
    B, TD, TH, TW, ny, nx = shape
    d = draws(i)
    Sy, Sx = ny * TH, nx * TW
    pre_rgb = (F.conv_transpose2d(d["x_rgb"], d["w_rgb"], None, 2, 1) + d["bias_rgb"][None]).view(B, TD, 3, Sy, Sx)
    pre_alpha = (F.conv_transpose2d(d["x_alpha"], d["w_alpha"], None, 2, 1) + d["bias_alpha"][None]).view(B, TD, 1, Sy, Sx)
    aff = AFFINE[0] * pre_rgb + AFFINE[1]
    keep = to_template(torch.cat([aff.abs() >= SCREEN_RGB, pre_alpha.abs() >= SCREEN_ALPHA], 2), shape)
    out = to_template(torch.cat([torch.relu(aff), torch.relu(pre_alpha)], 2), shape)
    return dict(out=out, keep=keep, g_out=d["g_out"] * keep)


def select(t, mask, compact):
    """what the operator keeps of a full-K tensor [B,K,...]"""
    if mask is None:
        return t
    if compact:
        return t[:, mask].contiguous()
    return t * mask.to(t.dtype).view(1, -1, *([1] * (t.dim() - 2)))


def twin_grads(i, mask=None, compact=True, one_channel=False):
    """float64 output and the six (two) gradients of decode_template_torch under the screened upstream gradient"""
    from goliath_amd import mvptail

    d = draws(i)
    names = LEAVES[3:] if one_channel else LEAVES
    leaf = {k: d[k].clone().requires_grad_(True) for k in names}
    args = [leaf.get(k) for k in LEAVES]
    out = mvptail.decode_template_torch(*args, primsize(SHAPES[i]), valid_prims=mask, compact=compact, rgb_affine=AFFINE)
    g = reference(i)["g_out"]
    g = g[..., 3] if one_channel else g
    if mask is not None and compact:
        g = g[:, mask].contiguous()
    if out.numel():
        out.backward(g)
    return out.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
