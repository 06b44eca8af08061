"""Deterministic inputs for the SSIM parity tests (tests/test_ssim_cases.py guards them on the CPU,
tests/test_gpu_ssim.py feeds them to gol_ssim_fwd / gol_ssim_bwd), a pure-Python replica of the kernel's workgroup
partition (csrc/ssim.hip: strip_of_block, grid_x) and the float32 / float64 oracle results the GPU tests are judged by.

Plain helper module: no fixtures, no GPU.  Every builder returns CPU float32 tensors; the oracle results are computed
once per case and dtype and shared (callers must not modify them).
"""
import functools
import zlib

import torch

TILE, STRIPS, XCDS = 32, 6, 8     # kTile, kStrips and the XCD count of csrc/ssim.hip

MASK_KINDS = ("none", "b1", "bc", "frac1", "zero")
#   none   no mask                           b1     [B,1] of 0 / 1            bc    [B,C] of 0 / 1
#   frac1  [B,1] uniform(0,1) x (0 / 1)      zero   [B,1] of 0 (the clamp(min=1) denominator)
INPUT_KINDS = ("noise", "flat")
#   noise  target ~ U(0,1), pred = target + 0.1 N(0,1)                      (as in tests/golden/ssim_golden.npz)
#   flat   target = 0.9 with 2 % of the pixels at 0.1, pred = target + 0.01 N(0,1): E[x^2] - mu^2 cancels in float32

# (tag, B, C, H, W, mask kind, input kind, g)   g = the upstream gradient: the loss is g * ssim
CASES = [
    # image smaller than / equal to the window: one tile, every halo read clamp-indexed
    ("1x1", 1, 1, 1, 1, "none", "noise", 1.0),
    ("5x7_bc", 2, 3, 5, 7, "bc", "noise", -1.0),            # mask_c = C with B = 2 at a small shape
    ("11x10_frac", 1, 3, 11, 10, "frac1", "noise", 0.37),
    # exact tile; 1-row and 1-column last tiles, strips [2,2,2,2,0,0]
    ("32x32", 1, 2, 32, 32, "b1", "noise", 0.37),
    ("33x225", 1, 2, 33, 225, "none", "noise", -1.0),
    ("33x225_flat", 1, 2, 33, 225, "b1", "flat", 1.0),
    # strips [2,2,2,1,0,0]: a short last strip and empty strips; mask_c = C = 3 with B = 2
    ("40x200_bc", 2, 3, 40, 200, "bc", "noise", 0.37),
    ("40x200_flat", 2, 3, 40, 200, "frac1", "flat", -1.0),
    # strips [3,3,3,3,1,0], 9 tile rows: rows_per_xcd = 2 with 7 padding slots; last tile row 4 px, last tile 6 px wide
    ("260x390", 1, 1, 260, 390, "none", "noise", 1.0),
    ("260x390_flat", 1, 1, 260, 390, "frac1", "flat", 0.37),
    # 10 tile rows of 3 single-tile strips
    ("290x65", 1, 2, 290, 65, "b1", "noise", -1.0),
    ("290x65_zero", 1, 2, 290, 65, "zero", "noise", 1.0),
]
TAGS = [c[0] for c in CASES]
BY_TAG = {c[0]: c for c in CASES}


def cdiv(a, b):
    return (a + b - 1) // b


def partition(H, W):
    """What strip_of_block / grid_x of csrc/ssim.hip give for an H x W plane: the grid is XCDS bands of `rows_per_xcd`
    tile-row slots, each slot `strips` workgroups; strip s walks tiles [s * per, min(tiles_x, (s + 1) * per))."""
    tiles_y, tiles_x = cdiv(H, TILE), cdiv(W, TILE)
    strips = min(tiles_x, STRIPS)
    per = cdiv(tiles_x, strips)
    rows_per_xcd = cdiv(tiles_y, XCDS)
    lens = [max(0, min(tiles_x, (s + 1) * per) - s * per) for s in range(strips)]
    # slot (xcd, j) holds tile row xcd * rows_per_xcd + j; a slot whose row is >= tiles_y is padding
    rows = [x * rows_per_xcd + j for x in range(XCDS) for j in range(rows_per_xcd)]
    assert sorted(r for r in rows if r < tiles_y) == list(range(tiles_y))      # every tile row in exactly one slot
    assert sum(lens) == tiles_x
    return {"tiles_x": tiles_x, "tiles_y": tiles_y, "strip_lens": lens, "rows_per_xcd": rows_per_xcd,
            "padding_slots": sum(1 for r in rows if r >= tiles_y), "grid": XCDS * rows_per_xcd * strips}


def make_inputs(kind, B, C, H, W, gen):
    if kind == "noise":
        target = torch.rand(B, C, H, W, generator=gen)
        return target + 0.1 * torch.randn(B, C, H, W, generator=gen), target
    assert kind == "flat"
    dots = torch.rand(B, C, H, W, generator=gen) < 0.02
    target = torch.where(dots, torch.tensor(0.1), torch.tensor(0.9))
    return target + 0.01 * torch.randn(B, C, H, W, generator=gen), target


def make_mask(kind, B, C, H, W, gen):
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(B, 1, H, W)
    mc = C if kind == "bc" else 1
    m = (torch.rand(B, mc, H, W, generator=gen) > 0.3).float()
    if kind == "frac1":
        m = m * torch.rand(B, 1, H, W, generator=gen)
    return m


@functools.lru_cache(maxsize=None)
def make(tag):
    """(pred, target, mask or None, g) of a case: CPU float32, seeded by the tag."""
    _, B, C, H, W, mk, ik, g = BY_TAG[tag]
    gen = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    pred, target = make_inputs(ik, B, C, H, W, gen)
    return pred, target, make_mask(mk, B, C, H, W, gen), g


@functools.lru_cache(maxsize=None)
def oracle(tag, dtype):
    """(value, gradient) of g * ssim(target, pred, mask) by oracle/ssim_ref.py in `dtype` (value: a Python float of the
    dtype's result; gradient: a CPU tensor of `dtype`)."""
    from oracle import ssim_ref

    pred, target, mask, g = make(tag)
    p = pred.to(dtype, copy=True).requires_grad_(True)         # a leaf of its own: the shared inputs stay as they are
    val = g * ssim_ref.ssim(target.to(dtype), p, None if mask is None else mask.to(dtype))
    (grad,) = torch.autograd.grad(val, p)
    return float(val.detach()), grad


@functools.lru_cache(maxsize=None)
def oracle_map(tag, dtype):
    """The oracle's per-pixel SSIM map of a case in `dtype` (no mask, no g)."""
    from oracle import ssim_ref

    pred, target, _, _ = make(tag)
    with torch.no_grad():
        return ssim_ref.ssim_map(target.to(dtype), pred.to(dtype))


def max_err(a, ref):
    """max |a - ref| / max |ref| (0 / 0 = 0): a per-pixel maximum, not a norm."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    num, den = float((a - ref).abs().max()), float(ref.abs().max())
    return 0.0 if num == 0.0 else num / den if den > 0 else float("inf")
