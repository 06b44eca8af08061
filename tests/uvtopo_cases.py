"""Cases and the numpy float64 oracle of the UV topology images (goliath_amd/uvtopo.py, csrc/uvtopo.hip), shared by
tests/test_uvtopo_cpu.py (which pins this oracle to the reference's own geom.py) and tests/test_gpu_uvtopo.py.

Oracle, from the stated semantics:
  * coverage: texel (r, c) is sampled at pixel (c + 0.5, r + 0.5) of the UV triangles scaled to pixels, (u W, v' H) with
    v' = 1 - v (in fp32) when flip_uv; float64 edge functions of the fp32 vt, anchored at the face's first vertex and
    oriented by the sign of the area; inside is >= 0; zero-area faces are skipped; the lowest face index wins;
  * barycentrics: the reference's bary_coords formula (anchored at the third vertex, denom clamped away from 0 by 1e-6
    keeping its sign, b2 = 1 - b0 - b1) in float64 on the fp32 vt, and in fp32 (its own rounding error: the tests' bound);
  * impaint source: brute force, the valid texel at the smallest squared distance over integer (row, col), ties to the
    lexicographically smallest (row, col), accepted when sqrt(d2) < threshold; -1 on valid texels and where none is.
Edge band of a case: texels where some face that (nearly) covers the sample -- all three normalised edge functions
>= -1e-5 -- has one with 0 < |E| / |area| < 1e-5: there fp32 and float64 may decide differently.  Every case but "f" is
built from dyadic coordinates whose products are exact in fp32: their band is empty and on-edge samples are exact zeros.
"""
import collections
import functools

import numpy as np

BAND = 1e-5
Case = collections.namedtuple("Case", ["name", "S", "vi", "vt", "vti", "flip_uv"])
Oracle = collections.namedtuple("Oracle", ["face", "index_image", "bary64", "bary32", "valid", "band"])
Nearest = collections.namedtuple("Nearest", ["src", "d2", "unique"])


# ---- oracle -----------------------------------------------------------------------------------------------------------------
def effective_vt(vt, flip_uv):
    vt = np.asarray(vt, np.float32).copy()
    if flip_uv:
        vt[:, 1] = np.float32(1.0) - vt[:, 1]
    return vt


def face_image(vt, vti, H, W, flip_uv):
    """-> (face[H,W] int64, band[H,W] bool)."""
    P = effective_vt(vt, flip_uv).astype(np.float64) * np.array([W, H], np.float64)
    face = np.full((H, W), -1, np.int64)
    band = np.zeros((H, W), bool)
    for f, (i0, i1, i2) in enumerate(np.asarray(vti)):
        a, b, c = P[i0], P[i1], P[i2]
        ux, uy, wx, wy = b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1]
        area = ux * wy - uy * wx
        if area == 0.0:
            continue
        sg = 1.0 if area > 0 else -1.0
        xs, ys = (a[0], b[0], c[0]), (a[1], b[1], c[1])
        j0, j1 = max(0, int(np.ceil(min(xs) - 0.5)) - 1), min(W - 1, int(np.floor(max(xs) - 0.5)) + 1)
        k0, k1 = max(0, int(np.ceil(min(ys) - 0.5)) - 1), min(H - 1, int(np.floor(max(ys) - 0.5)) + 1)
        if j0 > j1 or k0 > k1:
            continue
        dx = (np.arange(j0, j1 + 1) + 0.5 - a[0])[None, :]
        dy = (np.arange(k0, k1 + 1) + 0.5 - a[1])[:, None]
        E1 = sg * (wy * dx - wx * dy)
        E2 = sg * (-uy * dx + ux * dy)
        E0 = abs(area) - E1 - E2
        E = np.stack([E0, E1, E2]) / abs(area)
        inside = (E >= 0).all(0)
        sub = face[k0:k1 + 1, j0:j1 + 1]
        sub[inside & (sub < 0)] = f
        band[k0:k1 + 1, j0:j1 + 1] |= (E >= -BAND).all(0) & ((np.abs(E) < BAND) & (E != 0)).any(0)
    return face, band


def bary_coords(points, tri, dtype):
    """The reference's formula (ca_code/utils/geom.py:86-106) in `dtype`: points[N,2], tri[3,N,2] -> [N,3]."""
    points, tri = points.astype(dtype), tri.astype(dtype)
    eps, one = dtype(1.0e-6), dtype(1.0)
    x, x1, x2 = points[:, 0] - tri[2, :, 0], tri[0, :, 0] - tri[2, :, 0], tri[1, :, 0] - tri[2, :, 0]
    y, y1, y2 = points[:, 1] - tri[2, :, 1], tri[0, :, 1] - tri[2, :, 1], tri[1, :, 1] - tri[2, :, 1]
    denom = y2 * x1 - y1 * x2
    n0 = y2 * x - x2 * y
    n1 = x1 * y - y1 * x
    denom = np.where(denom >= 0, np.maximum(denom, eps), np.minimum(denom, -eps))
    b0, b1 = n0 / denom, n1 / denom
    return np.stack([b0, b1, one - b0 - b1], -1).astype(dtype)


def bary_image(face, vt, vti, flip_uv, dtype):
    H, W = face.shape
    vt_e = effective_vt(vt, flip_uv)
    tri = vt_e[np.asarray(vti)[np.clip(face, 0, None).reshape(-1)]].transpose(1, 0, 2)        # [3,N,2]
    if dtype is np.float32:   # the reference's grid: fp32 (k + 0.5) / n
        gx = (np.arange(W, dtype=np.float32) + np.float32(0.5)) / np.float32(W)
        gy = (np.arange(H, dtype=np.float32) + np.float32(0.5)) / np.float32(H)
    else:
        gx, gy = (np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H
    pts = np.stack(np.broadcast_arrays(gx[None, :], gy[:, None]), -1).reshape(-1, 2)
    out = bary_coords(pts, tri, dtype).reshape(H, W, 3)
    out[face < 0] = 0
    return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = CASES[name]
    face, band = face_image(c.vt, c.vti, c.S, c.S, c.flip_uv)
    index_image = np.asarray(c.vi, np.int64)[np.clip(face, 0, None)]
    index_image[face < 0] = -1
    out = Oracle(face, index_image, bary_image(face, c.vt, c.vti, c.flip_uv, np.float64),
                 bary_image(face, c.vt, c.vti, c.flip_uv, np.float32), face >= 0, band)
    for a in out:
        a.setflags(write=False)
    return out


def nearest_valid(valid, threshold):
    """Brute force -> Nearest(src[H,W] int32, d2[H,W] int64 (-1 where no valid texel exists or the texel is valid),
    unique[H,W] bool: exactly one valid texel at the smallest distance)."""
    valid = np.asarray(valid, bool)
    H, W = valid.shape
    src = np.full(H * W, -1, np.int32)
    d2o = np.full(H * W, -1, np.int64)
    uniq = np.zeros(H * W, bool)
    vr, vc = np.nonzero(valid)
    ir, ic = np.nonzero(~valid)
    if len(vr) and len(ir):
        vlin = vr.astype(np.int64) * W + vc
        for s in range(0, len(ir), 4096):
            rr, cc = ir[s:s + 4096, None].astype(np.int64), ic[s:s + 4096, None].astype(np.int64)
            d2 = (rr - vr[None, :]) ** 2 + (cc - vc[None, :]) ** 2
            best = np.argmin(d2 * (H * W) + vlin[None, :], axis=1)      # (d2, row, col) lexicographic
            dmin = d2[np.arange(len(best)), best]
            dst = (rr * W + cc)[:, 0]
            ok = np.sqrt(dmin.astype(np.float64)) < float(threshold)
            src[dst[ok]] = vlin[best[ok]]
            d2o[dst] = dmin
            uniq[dst] = (d2 == dmin[:, None]).sum(1) == 1
    return Nearest(src.reshape(H, W), d2o.reshape(H, W), uniq.reshape(H, W))


@functools.lru_cache(maxsize=None)
def oracle_nearest(name, threshold):
    out = nearest_valid(oracle(name).valid, threshold)
    for a in out:
        a.setflags(write=False)
    return out


def impaint(img, src):
    """img[H,W(,C)] with the source map applied."""
    H, W = src.shape
    flat = img.reshape(H * W, -1)
    s = src.reshape(-1)
    take = np.where(s >= 0, s, np.arange(H * W))
    return flat[take].reshape(img.shape)


# ---- meshes -----------------------------------------------------------------------------------------------------------------
def grid_mesh(us, vs, first_vertex=0):
    """Vertices on the grid vs x us (row-major), two triangles per cell -> (vt[n,2] float32, faces[m,3] int64)."""
    nu, nv = len(us), len(vs)
    vt = np.array([[u, v] for v in vs for u in us], np.float32)
    faces = []
    for j in range(nv - 1):
        for i in range(nu - 1):
            p = first_vertex + j * nu + i
            faces += [[p, p + 1, p + nu + 1], [p, p + nu + 1, p + nu]]
    return vt, np.array(faces, np.int64)


def _case_a(flip_uv):
    # S = 16: a 3x3-cell grid whose vertices sit on texel centres: on-edge, on-diagonal and on-vertex samples, exact in fp32
    k = (np.array([2, 5, 9, 13]) + 0.5) / 16.0
    vt, f = grid_mesh(k, k)
    return Case("a_flip" if flip_uv else "a", 16, f, vt, f, flip_uv)


def _mesh_b():
    # S = 24 (no multiple of the 16-texel tile); coordinates in 1/64 (0.375 texels: every product is exact in fp32)
    q = 1.0 / 64.0
    vtA, fA = grid_mesh(np.array([4, 14, 24]) * q, np.array([4, 16, 28]) * q, 0)              # texels c <= 8
    vtB, fB = grid_mesh(np.array([38, 50, 62]) * q, np.array([4, 20, 36]) * q, 9)             # texels c >= 14: a 5-texel gutter
    extra = np.array([[40, 8], [60, 8], [48, 30],          # 18-20: overlaps island B, listed BEFORE B's faces (wins)
                      [6, 6], [22, 8], [10, 26],           # 21-23: overlaps island A, listed last (loses)
                      [20, 50], [40, 50], [30, 80]],       # 24-26: reaches v = 1.25, partly outside the image
                     np.float32) * np.float32(q)
    vt = np.concatenate([vtA, vtB, extra]).astype(np.float32)
    vti = np.concatenate([[[0, 4, 8]],                     # face 0: zero area (the diagonal of island A), must not cover
                          [[18, 19, 20]], fA, fB, [[21, 22, 23]], [[24, 25, 26]]]).astype(np.int64)
    # seam: island B's left column (uv ids 9, 12, 15) are the mesh vertices of island A's right column (2, 5, 8)
    v_of_vt = np.arange(27)
    v_of_vt[[9, 12, 15]] = [2, 5, 8]
    vi = v_of_vt[vti]
    assert (vi != vti).any()
    return vi, vt, vti


def _case_d():
    # S = 272 = 17 x 16: coordinates in 1/256 (17 / 16 texels).  Three square islands; the texels of column 76 between the
    # first two (columns 34..50 and 102..118) are equidistant from both, rows between islands 1 and 3 likewise; the far
    # right and bottom are more than 100 texels from everything
    q = 1.0 / 256.0
    parts, faces, n = [], [], 0
    for (u0, v0) in ((32, 32), (96, 32), (32, 192)):
        vt, f = grid_mesh(np.array([u0, u0 + 16]) * q, np.array([v0, v0 + 16]) * q, n)
        parts.append(vt)
        faces.append(f)
        n += 4
    vt, f = np.concatenate(parts).astype(np.float32), np.concatenate(faces)
    return Case("d", 272, f, vt, f, False)


def jittered_grid(seed, S=64, n=8):
    """An n x n-cell grid over most of the image with every vertex moved by up to 0.3 of a cell: non-dyadic coordinates."""
    rng = np.random.default_rng(seed)
    k = np.linspace(0.06, 0.94, n + 1)
    vt, f = grid_mesh(k, k)
    vt = (vt + (rng.random(vt.shape) - 0.5) * 0.6 * (k[1] - k[0])).astype(np.float32)
    return Case("f", S, f, vt, f, False)


F_SEED = 0   # chosen on the CPU (tests/test_uvtopo_cpu.py asserts it): the edge band of case "f" holds at most 2 texels


def _cases():
    vi, vt, vti = _mesh_b()
    out = [_case_a(False), _case_a(True), Case("b", 24, vi, vt, vti, False), Case("b_flip", 24, vi, vt, vti, True),
           _case_d(), jittered_grid(F_SEED)]
    return collections.OrderedDict((c.name, c) for c in out)


CASES = _cases()
EXACT = ("a", "a_flip", "b", "b_flip", "d")           # (a)-(d): identical on every texel
IMPAINT = (("b", 100.0), ("b", 3.0), ("b", 2.5), ("b_flip", 100.0), ("d", 100.0))   # (c), (d)


def masks_e():
    """(e): an all-empty map and maps with a single valid texel (a corner and an inner texel), S = 20."""
    empty = np.zeros((20, 20), bool)
    corner, inner = empty.copy(), empty.copy()
    corner[19, 0] = True
    inner[7, 12] = True
    return {"empty": empty, "corner": corner, "inner": inner}
