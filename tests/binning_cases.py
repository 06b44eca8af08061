"""Deterministic inputs for the tile-binning parity tests (tests/test_binning_cases.py guards them on the CPU,
tests/test_gpu_binning.py feeds them to gol_bin_sort) and a brute-force float64 reference of what pruning may drop.

Plain helper module: no fixtures, no GPU.  Every builder returns CPU tensors (xys[N,2] f32, depths[N] f32, radii[N] i32
[, conics[N,3] f32, opacities[N] f32], H, W); the tile width is 16 (goliath_amd.splat.BLOCK).  Image sizes are written
W x H in the scenario tables, tile t is (t % tiles_x, t // tiles_x).
"""
import math

import numpy as np
import torch

BLOCK = 16
ALPHA_MIN = 1.0 / 255.0     # the rasterizer's cut, in float64
ALPHA_CAP = 0.999

# ---- the list-length plans of the scenarios (tile -> length) -------------------------------------------------------
# (a) 64 x 64, T = 16: every size class of the per-tile sort at once, MID and BIG queues both populated (cap 7 each)
PLAN_A = (64, 64, {0: 1, 1: 2, 2: 63, 3: 64, 4: 65, 5: 256, 6: 257, 7: 1025, 8: 2048, 9: 2049, 10: 3000, 11: 4096,
                   12: 4097, 13: 9000, 14: 16385, 15: 0})
# (b) 64 x 32, T = 8, cap 3: four MID and four BIG lists compete for three slots each
PLAN_B = (32, 64, {0: 2049, 1: 2100, 2: 3000, 3: 4096, 4: 4097, 5: 5000, 6: 9000, 7: 17000})
# (c) T = 1, 2, 3: cap 0 (every long list sorted in place); T = 4, 5: cap 1
PLANS_C = {
    1: (16, 16, {0: 3000}),
    2: (16, 32, {0: 3000, 1: 5000}),
    3: (16, 48, {0: 3000, 1: 5000, 2: 2500}),
    4: (32, 32, {0: 3000, 1: 5000, 2: 2500, 3: 4500}),
    5: (16, 80, {0: 3000, 1: 5000, 2: 2500, 3: 4500, 4: 70}),
}


def tiles_of(H, W):
    return (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def one_tile_gaussians(tile_xy, n, gen):
    """n Gaussians of radius 1 with centres at 16 t + U(3, 13): each hits exactly tile `tile_xy` = (tx, ty).
    `gen` is a numpy Generator.  Depths uniform in [1, 2)."""
    xy = np.asarray(tile_xy, np.float64) * BLOCK + gen.uniform(3.0, 13.0, size=(n, 2))
    return xy.astype(np.float32), gen.uniform(1.0, 2.0, size=n).astype(np.float32), np.ones(n, np.int32)


def planned_lists(H, W, plan, seed=0):
    """Gaussians that give tile t a list of exactly plan[t] entries, concatenated in a shuffled id order.
    Returns (xys, depths, radii, H, W, plan); the oracle's bins must reproduce `plan` (tests assert it first)."""
    gen = np.random.default_rng(seed)
    tx, ty = tiles_of(H, W)
    assert all(0 <= t < tx * ty for t in plan)
    parts = [one_tile_gaussians((t % tx, t // tx), n, gen) for t, n in sorted(plan.items()) if n > 0]
    xys, depths, radii = (np.concatenate([p[k] for p in parts]) for k in range(3))
    perm = gen.permutation(xys.shape[0])
    return _t(xys[perm], np.float32), _t(depths[perm], np.float32), _t(radii[perm], np.int32), H, W, dict(plan)


def pad_to(xys, depths, radii, N):
    """Pad a scenario to N Gaussians with radius-0 entries (they hit nothing)."""
    n = xys.shape[0]
    assert N >= n
    return (torch.cat([xys, torch.zeros(N - n, 2)]), torch.cat([depths, torch.ones(N - n)]),
            torch.cat([radii, torch.zeros(N - n, dtype=torch.int32)]))


def two_tile_chunk_scene():
    """32 x 16 image (T = 2).  Ids 0 .. 4095 cover BOTH tiles (radius 12 at the shared border), ids 4096 .. 9095 sit on
    tile 1: with 4096 Gaussians per scatter workgroup the first workgroup counts 4096 in both halves of one packed
    counter word and uses all of its per-lane mask registers."""
    gen = np.random.default_rng(77)
    n0, n1 = 4096, 5000
    xy0 = np.stack([gen.uniform(15.0, 17.0, n0), gen.uniform(6.0, 10.0, n0)], 1)
    xy1, d1, r1 = one_tile_gaussians((1, 0), n1, gen)
    xys = np.concatenate([xy0.astype(np.float32), xy1])
    depths = np.concatenate([gen.uniform(1.0, 2.0, n0).astype(np.float32), d1])
    radii = np.concatenate([np.full(n0, 12, np.int32), r1])
    return _t(xys, np.float32), _t(depths, np.float32), _t(radii, np.int32), 16, 32, {0: n0, 1: n0 + n1}


# ---- depth sets of the single-tile sort cases -----------------------------------------------------------------------
DEPTH_SETS = ("tie_groups", "all_equal", "two_ulp", "clustered_outliers", "subnormal", "specials")


def depth_case(n, kind):
    """A single-tile list (64 x 64 image, tile 0) of n entries with the depth set `kind`.  The expected order is by the
    depth's bit pattern as an unsigned 32-bit number, then by id."""
    gen = np.random.default_rng(1000 + n + 7 * DEPTH_SETS.index(kind))
    xys, depths, radii = one_tile_gaussians((0, 0), n, gen)
    if kind == "tie_groups":       # small groups of equal depths inside a uniform list: the bucket sort accepts them
        perm = gen.permutation(n)
        pos = 0
        for size in (2, 8, 40, 2, 8, 40):
            depths[perm[pos:pos + size]] = depths[perm[pos]]
            pos += size
    elif kind == "all_equal":
        depths[:] = np.float32(1.5)
    elif kind == "two_ulp":
        depths[:] = np.where(gen.random(n) < 0.5, np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)))
    elif kind == "clustered_outliers":
        depths[:] = (1.0 + gen.uniform(0.0, 1e-6, n)).astype(np.float32)
        far = gen.permutation(n)[:max(2, n // 100)]
        depths[far[0::2]] = np.float32(50.0)
        depths[far[1::2]] = np.float32(1e4)
    elif kind == "subnormal":      # float32 subnormals and tiny normals: the span is too small for a finite bucket scale
        depths[:] = np.exp(gen.uniform(math.log(1e-44), math.log(1e-37), n)).astype(np.float32)
    elif kind == "specials":
        at = gen.permutation(n)[:5]
        depths[at] = np.array([0.0, -0.0, -1.0, np.inf, np.nan], np.float32)
    else:
        raise ValueError(kind)
    return _t(xys, np.float32), _t(depths, np.float32), _t(radii, np.int32), 64, 64


def in_list_order(depths, ids):
    """True iff the list `ids` is strictly increasing in (depth bits as an unsigned 32-bit number, id): the order every
    tile list is kept in."""
    bits = (depths.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF)[ids.long()]
    i = ids.to(torch.int64)
    return bool(((bits[1:] > bits[:-1]) | ((bits[1:] == bits[:-1]) & (i[1:] > i[:-1]))).all())


# ---- anisotropic Gaussians with consistent (radius, conic) ---------------------------------------------------------
def _conic_and_radius(smax, ratio, theta):
    """Covariance R diag(smax^2, (smax / ratio)^2) R^T -> (conic (a, b, c), radius) as gsplat derives them
    (radius = ceil(3 sqrt(larger eigenvalue)))."""
    l1, l2 = smax ** 2, (smax / ratio) ** 2
    c, s = np.cos(theta), np.sin(theta)
    sxx, syy, sxy = c * c * l1 + s * s * l2, s * s * l1 + c * c * l2, c * s * (l1 - l2)
    det = sxx * syy - sxy * sxy
    conic = np.stack([syy / det, -sxy / det, sxx / det], 1)
    bb = 0.5 * (sxx + syy)
    v1 = bb + np.sqrt(np.maximum(0.1, bb * bb - det))
    return conic, np.ceil(3.0 * np.sqrt(v1)).astype(np.int32)


def _log_uniform(gen, lo, hi, n):
    return np.exp(gen.uniform(math.log(lo), math.log(hi), n))


def aniso_gaussians(n, gen, H, W, smax_lo, smax_hi, margin=0.0):
    xy = np.stack([gen.uniform(-margin, W + margin, n), gen.uniform(-margin, H + margin, n)], 1)
    conic, radii = _conic_and_radius(_log_uniform(gen, smax_lo, smax_hi, n), _log_uniform(gen, 1.0, 30.0, n),
                                     gen.uniform(0.0, math.pi, n))
    return xy, conic, radii, _log_uniform(gen, 0.5 / 255.0, 1.0, n)


def _pack(xy, depths, radii, conic, opac, H, W):
    return (_t(xy, np.float32), _t(depths, np.float32), _t(radii, np.int32), _t(conic, np.float32),
            _t(opac, np.float32), H, W)


def radius_set_scene(H=96, W=96, N=12000, seed=5):
    """(e) mixed footprints: radii drawn from {1, 9, 20, 40}, conics with 3 sigma_max = radius - 0.5."""
    gen = np.random.default_rng(seed)
    radii = gen.choice(np.array([1, 9, 20, 40], np.int32), N)
    smax = (radii - 0.5) / 3.0
    # (the radii are the drawn ones: gsplat's eigenvalue floor would turn the conic of a radius-1 splat into radius 2)
    conic, _ = _conic_and_radius(smax, _log_uniform(gen, 1.0, 30.0, N), gen.uniform(0.0, math.pi, N))
    xy = np.stack([gen.uniform(0, W, N), gen.uniform(0, H, N)], 1)
    return _pack(xy, gen.uniform(1.0, 10.0, N), radii, conic, _log_uniform(gen, 0.5 / 255.0, 1.0, N), H, W)


def many_tile_scene(H, W, N=4000, seed=11):
    """(g) uniform centres, radii 1 ... 40; Gaussian 0 sits in the last tile and Gaussian 1 in the first one."""
    gen = np.random.default_rng(seed)
    xy, conic, radii, opac = aniso_gaussians(N, gen, H, W, 0.2, 13.3)
    tx, ty = tiles_of(H, W)
    # (round, sigma = 3 px, centred on a pixel centre: visible in their tile whatever the random draw)
    xy[0] = [(tx - 1) * BLOCK + 2.5, (ty - 1) * BLOCK + 2.5]
    xy[1] = [8.5, 8.5]
    conic[:2], radii[:2], opac[:2] = [1.0 / 9.0, 0.0, 1.0 / 9.0], 9, 0.9
    return _pack(xy, gen.uniform(1.0, 10.0, N), radii, conic, opac, H, W)


PRUNE_H, PRUNE_W, PRUNE_N = 112, 160, 1500
OP_CUT = np.float32(1.0) / np.float32(255.0)                 # "exactly 1/255" as the kernels see it
OP_CUT_NEXT = np.nextafter(OP_CUT, np.float32(1.0))


def prune_scene(seed):
    """160 x 112 image (10 x 7 tiles), 1500 rotated anisotropic Gaussians (axis ratio 1 ... 30, opacity log-uniform over
    [0.5/255, 1]) for the pruning contract, with the special classes that prune_scene_classes() counts."""
    gen = np.random.default_rng(seed)
    H, W, N = PRUNE_H, PRUNE_W, PRUNE_N
    n_hand, n_big, n_deg, n_narrow, n_out = 32, 60, 24, 60, 100
    n_gen = N - (n_hand + n_big + n_deg + n_narrow + n_out)
    xy, conic, radii, opac = [], [], [], []

    def add(x, c, r, o):
        xy.append(x); conic.append(c); radii.append(r); opac.append(o)

    # hand-placed: centres exactly on the pixel centres either side of a tile border, opacity at the cut
    kx, ky = gen.integers(1, W // BLOCK, n_hand), gen.integers(1, H // BLOCK, n_hand)
    sx, sy = np.where(gen.random(n_hand) < 0.5, -0.5, 0.5), np.where(gen.random(n_hand) < 0.5, -0.5, 0.5)
    c, r = _conic_and_radius(1.0 + (np.arange(n_hand) % 5), 1.0 + 0.5 * (np.arange(n_hand) % 3), gen.uniform(0, math.pi, n_hand))
    add(np.stack([BLOCK * kx + sx, BLOCK * ky + sy], 1), c, r,
        np.array([OP_CUT, OP_CUT_NEXT, np.float32(1.0)], np.float64)[np.arange(n_hand) % 3])
    # boxes of more than 64 tiles (all 70): long thin streaks through the middle of the image
    # (along a diagonal, so that the alpha >= 1/255 ellipse itself spans every tile column and row)
    th = gen.uniform(0.5, 0.7, n_big)
    th = np.where(gen.random(n_big) < 0.5, th, math.pi - th)
    c, r = _conic_and_radius(gen.uniform(40.0, 50.0, n_big), gen.uniform(8.0, 30.0, n_big), th)
    add(np.stack([gen.uniform(72, 88, n_big), gen.uniform(48, 64, n_big)], 1), c, r, gen.uniform(0.5, 1.0, n_big))
    # conics that are no ellipse: det <= 0 or a <= 0 (the kernel must keep their whole box)
    x, c, r, o = aniso_gaussians(n_deg, gen, H, W, 3.0, 10.0)
    kind = np.arange(n_deg) % 3
    s = gen.uniform(0.5, 2.0, n_deg)
    c = np.where(kind[:, None] == 0, np.stack([0.02 * s, 0.05 * s, 0.02 * s], 1),
                 np.where(kind[:, None] == 1, np.stack([-0.01 * s, 0 * s, 0.02 * s], 1),
                          np.stack([0 * s, 0 * s, 0.02 * s], 1)))
    add(x, c, r, o)
    # so narrow that whole tile rows (or columns) of the box see no pixel centre of the alpha >= 1/255 region
    th = np.where(gen.random(n_narrow) < 0.5, 0.0, 0.5 * math.pi) + gen.uniform(-0.15, 0.15, n_narrow)
    c, r = _conic_and_radius(gen.uniform(12.0, 25.0, n_narrow), gen.uniform(20.0, 30.0, n_narrow), th)
    add(np.stack([gen.uniform(0, W, n_narrow), gen.uniform(0, H, n_narrow)], 1), c, r, gen.uniform(0.2, 1.0, n_narrow))
    # centres up to 3 radii outside the image
    x, c, r, o = aniso_gaussians(n_out, gen, H, W, 2.0, 15.0)
    off = gen.uniform(0.0, 3.0, n_out) * r
    side = gen.integers(0, 4, n_out)
    x[:, 0] = np.where(side == 0, -off, np.where(side == 1, W + off, x[:, 0]))
    x[:, 1] = np.where(side == 2, -off, np.where(side == 3, H + off, x[:, 1]))
    add(x, c, r, o)
    # the rest
    add(*aniso_gaussians(n_gen, gen, H, W, 0.4, 16.0))
    xy, conic, radii, opac = (np.concatenate(v) for v in (xy, conic, radii, opac))
    return _pack(xy, gen.uniform(1.0, 10.0, N), radii, conic, opac, H, W)


# ---- float64 reference of the pruning contract ----------------------------------------------------------------------
def oracle_lists(xys, depths, radii, H, W):
    """gsplat's sorted tile lists from the CPU oracle: (ids[I] i32, bins[T,2] i32)."""
    import ctypes

    from oracle import cref

    xys, depths, radii = xys.float().contiguous(), depths.float().contiguous(), radii.to(torch.int32).contiguous()
    tx, ty = tiles_of(H, W)
    # a first call with no room only counts the pairs (the oracle counts past its capacity)
    scratch_k, scratch_i = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    scratch_b = torch.zeros(tx * ty, 2, dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    n = cref.lib().orc_bin_sort(ctypes.c_int(xys.shape[0]), p(xys), p(depths), p(radii), ctypes.c_int(H), ctypes.c_int(W),
                                ctypes.c_int(BLOCK), ctypes.c_int64(0), p(scratch_k), p(scratch_i), p(scratch_b))
    _, ids, bins = cref.bin_and_sort(xys, depths, radii, torch.tensor([n], dtype=torch.int64), H, W, BLOCK)
    return ids, bins


def prune_reference(xys, radii, conics, opac, H, W, lists=None):
    """Which pairs of gsplat's lists can be seen at all, by brute force in float64.

    For every entry of the oracle's lists (`lists` = (ids, bins) of oracle_lists(); None: lists taken at equal depths,
    i.e. ordered by id) evaluate sigma = (a dx^2 + c dy^2) / 2 + b dx dy at all 256 pixel centres of the entry's tile --
    the full 16 x 16 block, also where it sticks out of the image: the superset a kernel may use.  An entry is `live` iff
    at some centre sigma >= 0 and min(0.999, opacity exp(-sigma)) >= 1/255.  Returns live[I] bool (numpy),
    aligned with ids."""
    if lists is None:
        lists = oracle_lists(xys, torch.ones(xys.shape[0]), radii, H, W)
    ids, bins = lists
    tx, ty = tiles_of(H, W)
    lens = (bins[:, 1] - bins[:, 0]).numpy().astype(np.int64)
    assert int(lens.sum()) == ids.numel() and bool((bins[1:, 0][lens[1:] > 0] >= 0).all())
    tile = np.repeat(np.arange(tx * ty), lens)
    # (the lists are contiguous in tile order: position p of ids belongs to tile[p])
    g = ids.numpy().astype(np.int64)
    xy, con, op = xys.numpy().astype(np.float64), conics.numpy().astype(np.float64), opac.numpy().astype(np.float64)
    px = np.arange(BLOCK) + 0.5
    live = np.zeros(g.shape[0], bool)
    for s in range(0, g.shape[0], 32768):
        gi, ti = g[s:s + 32768], tile[s:s + 32768]
        dx = ((ti % tx) * BLOCK)[:, None] + px[None, :] - xy[gi, 0][:, None]       # [P, 16]
        dy = ((ti // tx) * BLOCK)[:, None] + px[None, :] - xy[gi, 1][:, None]
        a, b, c = (con[gi, k][:, None, None] for k in range(3))
        sigma = 0.5 * (a * dx[:, None, :] ** 2 + c * dy[:, :, None] ** 2) + b * dx[:, None, :] * dy[:, :, None]
        with np.errstate(over="ignore"):
            alpha = np.minimum(ALPHA_CAP, op[gi][:, None, None] * np.exp(-sigma))
        live[s:s + 32768] = ((sigma >= 0) & (alpha >= ALPHA_MIN)).any(axis=(1, 2))
    return live


def prune_scene_classes(scene, lists, live):
    """Counts of the special classes of a prune_scene, recomputed from its tensors (not from labels the builder kept)."""
    xys, depths, radii, conics, opac, H, W = scene
    xy, con, op, r = xys.numpy(), conics.numpy().astype(np.float64), opac.numpy(), radii.numpy()
    ids, bins = lists
    tx, ty = tiles_of(H, W)
    lens = (bins[:, 1] - bins[:, 0]).numpy().astype(np.int64)
    tile = np.repeat(np.arange(tx * ty), lens)
    g = ids.numpy().astype(np.int64)
    N = xy.shape[0]
    on_border = np.ones(N, bool)
    for k in range(2):
        f = np.abs(xy[:, k].astype(np.float64) - np.round(xy[:, k] / BLOCK) * BLOCK)
        on_border &= (f == 0.5) & (np.round(xy[:, k] / BLOCK) > 0)
    box = np.bincount(g, minlength=N)
    det = con[:, 0] * con[:, 2] - con[:, 1] ** 2
    ellipse = (det > 0) & (con[:, 0] > 0) & (con[:, 2] > 0)
    # the alpha >= 1/255 ellipse itself spans every tile column and row (so the kernel's own box stays above 64 tiles)
    with np.errstate(invalid="ignore", divide="ignore"):
        tau2 = 2.0 * np.log(np.maximum(255.0 * op.astype(np.float64), 1e-300))
        hx, hy = np.sqrt(tau2 * con[:, 2] / det), np.sqrt(tau2 * con[:, 0] / det)
    spans = ellipse & (tau2 > 0) & (xy[:, 0] - hx < 15.5) & (xy[:, 0] + hx > W - 15.5) & (xy[:, 1] - hy < 15.5) \
        & (xy[:, 1] + hy > H - 15.5)
    # tile rows of the box: rows with / without a live pair
    rows_all = np.zeros((N, ty), bool)
    rows_live = np.zeros((N, ty), bool)
    rows_all[g, tile // tx] = True
    rows_live[g[live], tile[live] // tx] = True
    outside = (xy[:, 0] < 0) | (xy[:, 0] > W) | (xy[:, 1] < 0) | (xy[:, 1] > H)
    return {
        "op_cut_on_border": int((on_border & (op == OP_CUT)).sum()),
        "op_next_on_border": int((on_border & (op == OP_CUT_NEXT)).sum()),
        "op_one_on_border": int((on_border & (op == 1.0)).sum()),
        "outside_with_pairs": int((outside & (box > 0)).sum()),
        "outside_beyond_radius": int((outside & (box == 0) & (r > 0)).sum()),
        "box_over_64": int((box > 64).sum()),
        "box_over_64_ellipse_spans_image": int(((box > 64) & spans).sum()),
        "not_an_ellipse": int((~ellipse & (box > 0)).sum()),
        "row_without_pixel": int((ellipse & rows_live.any(1) & (rows_all & ~rows_live).any(1)).sum()),
    }
