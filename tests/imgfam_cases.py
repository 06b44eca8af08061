"""TEST INFRASTRUCTURE: the shapes and scenes of the imgfam fixtures (tests/golden/make_imgfam_golden.py builds them, the
imgfam tests name them) and the float case's decision rule.  numpy only."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)

# ---- the penalty kernel's cases -------------------------------------------------------------------------------------------
KINDS = ("abs", "sq", "expw")                       # GOL_IMGLOSS_ABS, _SQ, _EXPW in this order
HWS = (1, 3, 4, 4095, 4096, 4097, 2 * 4096 + 5)     # the chunk is 4096 floats
BCS = ((1, 1), (2, 3))
MASKS = ("none", "one", "full")                     # no mask, [B,1,HW], [B,C,HW]
VETOS = ("none", "veto")
PALETTE = 509                                        # prime: a value meets every lane, float4 slot and chunk offset


def shape_tag(B, C, HW):
    return f"b{B}c{C}hw{HW}"


# ---- the mask operators' cases --------------------------------------------------------------------------------------------
TILE_W, TILE_H = 64, 16                              # the output tile of gol_depth_disc_mask / gol_mask_erode
SIZES = ((1, 1), (1, 7), (7, 1), (3, 3), (33, 35), (17, 250),
         (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (2 * TILE_H + 1, 2 * TILE_W + 1))
STEP_SIZE = (2 * TILE_H + 1, 2 * TILE_W + 1)         # the step edges at offsets 0 .. tile + 1 live at this size
POOLS = (1, 3, 5)
ERODE_KS = (1, 3, 5, 31)
# sqrt(n) > t decides as n > 1600 at t = 40: 1600 = 40^2 + 0^2 fires just below 40 only; the next reachable n is
# 1602 = 39^2 + 9^2 (gx and gy of integer depths have one parity), which sqrt(1601) lets fire and sqrt(1602) does not.
THRESHOLDS = tuple(float(v) for v in (np.nextafter(np.float32(40.0), np.float32(0.0)), np.float32(40.0),
                                      np.sqrt(np.float32(1601.0)), np.sqrt(np.float32(1602.0))))


def size_tag(H, W):
    return f"{H}x{W}"


def seams(n, tile):
    """Both sides of every tile seam inside [0, n)."""
    return [v for s in range(tile, n, tile) for v in (s - 1, s) if 0 <= v < n]


def marks(H, W):
    """Corners and border mid-points, then both sides of every tile seam (each on a row / column of its own where the
    image has room)."""
    a = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    b = [((5 * i + 2) % H, x) for i, x in enumerate(seams(W, TILE_W))] + \
        [(y, (7 * i + 3) % W) for i, y in enumerate(seams(H, TILE_H))]
    return sorted(set(a)), sorted(set(b))


def sobel_norm64(depth):
    """float64 Sobel norm of every centre of depth [S,H,W] (zero padding), from the stored float32 values, and the largest
    |depth| of each centre's 3x3 window."""
    d = np.pad(depth.astype(np.float64), ((0, 0), (1, 1), (1, 1)))
    H, W = depth.shape[1:]
    w = lambda dy, dx: d[:, dy:dy + H, dx:dx + W]
    gx = (w(0, 2) - w(0, 0)) + 2.0 * (w(1, 2) - w(1, 0)) + (w(2, 2) - w(2, 0))
    gy = (w(2, 0) - w(0, 0)) + 2.0 * (w(2, 1) - w(0, 1)) + (w(2, 2) - w(0, 2))
    big = np.max(np.stack([np.abs(w(dy, dx)) for dy in range(3) for dx in range(3)]), axis=0)
    return np.sqrt(gx * gx + gy * gy), big


def window_any(flags, pool):
    """OR of boolean flags [S,H,W] over each pixel's pool x pool window (outside the image: False)."""
    r = pool // 2
    f = np.pad(flags, ((0, 0), (r, r), (r, r)))
    H, W = flags.shape[1:]
    out = np.zeros_like(flags)
    for dy in range(pool):
        for dx in range(pool):
            out |= f[:, dy:dy + H, dx:dx + W]
    return out


def decide(depth, pool, threshold=40.0):
    """(decided_true, decided_false) of the float case: tau = 64 eps32 max(40, 8 max|d| over the window) per centre; a pixel
    is decided true if a centre of its window has s > t + tau, decided false if every one has s < t - tau."""
    s, big = sobel_norm64(depth)
    tau = 64.0 * EPS32 * np.maximum(40.0, 8.0 * big)
    sure_fire, sure_quiet = s > threshold + tau, s < threshold - tau
    return window_any(sure_fire, pool), ~window_any(~sure_quiet, pool)


FLAGGED_CAP = 1e-3    # flagged (undecided) pixels / pixels of the float scene
