"""oracle/mesh_ref.py -- TEST INFRASTRUCTURE ONLY (CPU oracle, never shipped).

Plain numpy z-buffer rasterizer with the conventions of goliath_amd/csrc/meshraster.hip (sample at pixel centres, all
edge functions >= 0, nearest positive depth, ties to the lower face index, perspective-correct depth / barycentrics).
It checks the HIP kernel's bookkeeping (tile binning, compaction order, z-test); it is NOT a restatement of the
reference: the index / depth / barycentric images come from the third-party drtk in the reference
(/root/reference/ca_code/utils/render_drtk.py:44-46), whose source is absent -- PARITY UNPINNED for this stand-in.

A face is skipped, as the kernel skips it, when one of its vertex indices is outside [0, V) (numpy alone would wrap a
negative one), one of its x / y is not finite, one of its z is not > 0 (NaN included), or its area is 0.
"""
import numpy as np


def faces_over_pixels(v, vi, H, W):
    """The faces of one view that survive the skip rules and touch the image, in face order, in v's dtype.

    v[V,3], vi[F,3] -> yields (f, (k0, k1, j0, j1), px, py, (a, b, c), area, (b0, b1, b2)): inclusive pixel bounds, the pixel
    centres of that box (meshgrid), the three vertices, the signed area and the three barycentrics over the box."""
    V = v.shape[0]
    half, one = v.dtype.type(0.5), v.dtype.type(1.0)
    fin = np.isfinite(v[:, :2]).all(1)
    for f, (i0, i1, i2) in enumerate(np.asarray(vi, dtype=np.int64).tolist()):
        if not (0 <= i0 < V and 0 <= i1 < V and 0 <= i2 < V):
            continue
        if not (fin[i0] and fin[i1] and fin[i2]):
            continue
        a, b, c = v[i0], v[i1], v[i2]
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = a, b, c
        if not (az > 0 and bz > 0 and cz > 0):
            continue
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if area == 0:
            continue
        j0, j1 = max(0, int(np.ceil(min(ax, bx, cx) - half))), min(W - 1, int(np.floor(max(ax, bx, cx) - half)))
        k0, k1 = max(0, int(np.ceil(min(ay, by, cy) - half))), min(H - 1, int(np.floor(max(ay, by, cy) - half)))
        if j0 > j1 or k0 > k1:
            continue
        px, py = np.meshgrid(np.arange(j0, j1 + 1).astype(v.dtype) + half, np.arange(k0, k1 + 1).astype(v.dtype) + half)
        if v.dtype == np.float64:
            b0 = ((by - cy) * px + (cx - bx) * py + (bx * cy - cx * by)) / area
            b1 = ((cy - ay) * px + (ax - cx) * py + (cx * ay - ax * cy)) / area
            b2 = ((ay - by) * px + (bx - ax) * py + (ax * by - bx * ay)) / area
        else:
            # the same three functions arranged around vertex a.  In absolute pixel coordinates the float32 products
            # (~1e4 in a 1024^2 image) cancel down to an area of ~50: 1e-4 of a barycentric is lost, which is why the
            # kernel anchors too.  A float32 yardstick that throws that away would license the same loss in the kernel
            dx, dy = px - ax, py - ay
            b1 = ((cy - ay) * dx + (ax - cx) * dy) / area
            b2 = ((ay - by) * dx + (bx - ax) * dy) / area
            b0 = one - b1 - b2
        yield f, (k0, k1, j0, j1), px, py, (a, b, c), area, (b0, b1, b2)


def rasterize(v_pix, vi, H, W, dtype=np.float64):
    """v_pix[B,V,3] float, vi[F,3] int -> index[B,H,W] int32, depth[B,H,W], bary[B,3,H,W].

    float64 arithmetic by default: the oracle.  dtype=np.float32 evaluates the same functions in float32 numpy (barycentrics
    anchored at the face's first vertex, see faces_over_pixels): the reference's own fp32 distance from its fp64 self, the
    yardstick of the depth / barycentric bounds."""
    v_pix = np.asarray(v_pix, dtype=dtype)
    B = v_pix.shape[0]
    index = -np.ones((B, H, W), np.int32)
    best_iz = np.zeros((B, H, W), dtype)
    bary = np.zeros((B, 3, H, W), dtype)
    one = dtype(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for b in range(B):
            for f, (k0, k1, j0, j1), _, _, (va, vb, vc), _, (b0, b1, b2) in faces_over_pixels(v_pix[b], vi, H, W):
                w0, w1, w2 = b0 / va[2], b1 / vb[2], b2 / vc[2]
                iz = w0 + w1 + w2
                sl = (b, slice(k0, k1 + 1), slice(j0, j1 + 1))
                win = (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & (iz > best_iz[sl])
                best_iz[sl] = np.where(win, iz, best_iz[sl])
                index[sl] = np.where(win, f, index[sl])
                for c, w in enumerate((w0, w1, w2)):
                    s = (b, c, slice(k0, k1 + 1), slice(j0, j1 + 1))
                    bary[s] = np.where(win, w / np.where(iz != 0, iz, one), bary[s])
    depth = np.where(index >= 0, one / np.where(best_iz != 0, best_iz, one), dtype(0.0))
    return index, depth, bary
