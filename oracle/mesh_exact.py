"""oracle/mesh_exact.py -- TEST INFRASTRUCTURE ONLY: the judges of the mesh rasterizer (csrc/meshraster.hip).

Three pieces, all CPU, all decided BEFORE the output under test is looked at:

  classify()        dyadic scenes (x, y multiples of 2^-8, |x|, |y| < 4096): exact integer edge functions, per pixel the
                    closed acceptance set, split into strictly-inside / shared-edge / outline hits, with the exact 1 / z
                    of every hit as a fractions.Fraction.  The fill rule, without rounding.
  generic_reference()  any scene: oracle/mesh_ref.py in float64 and in float32, plus two a-priori flags per pixel
                    (edge proximity, depth near-tie) that say where an fp32 implementation may legitimately differ.
  judge()           ONE comparison for both kinds of scene; takes (index, depth, bary) arrays from anywhere and returns
                    a Report (counts, measured ratios, failures with the first offenders spelled out).

Edge-proximity flag, derivation.  The kernel evaluates b1 = e3 dx + e4 dy, b2 = e6 dx + e7 dy, b0 = 1 - b1 - b2 with
e = (vertex difference) / area rounded once, dx = px - ax exact or rounded once.  Each of b1, b2 is two rounded products
of a rounded quotient plus one rounded sum: every term carries <= ~1.5 eps32 of ITS OWN magnitude, so the absolute error
is <= ~4 eps32 M with M = max(1, |e3 dx|, |e4 dy|, |e6 dx|, |e7 dy|), with or without FMA contraction (contraction only
removes roundings); b0 adds two more subtractions of numbers <= M.  An un-normalised evaluation (edge function, then
one multiplication by 1 / area) is inside the same bound.  tau = 32 eps32 M leaves 8x head-room.  A pixel is flagged
when ANY face whose pixel bounds contain it has some |b_k| <= tau there: only at such a pixel can the sign of a
barycentric, hence coverage, depend on rounding.  The depth flag marks pixels whose two nearest covering faces differ
by less than 32 eps32 in 1 / z, relative: there the z-test may depend on rounding.
"""
from fractions import Fraction

import numpy as np

from . import mesh_ref

EPS32 = float(np.finfo(np.float32).eps)
TAU = 32.0 * EPS32          # edge proximity, in units of M
TIE = 32.0 * EPS32          # depth near-tie, relative
DEPTH_FLAGGED = 64.0 * EPS32  # a flagged pixel's face must lie this close (relative) to the oracle's depth
FLAGGED_SHARE = 1e-3        # condition on a generic scene: flagged pixels <= 0.1 % of the covered ones, per view
Q = 256                     # dyadic grid: 2^-8


# ---- dyadic scenes: the exact classifier ------------------------------------------------------------------------------------
STRICT, SHARED, OUTLINE = 0, 1, 2


def classify(v_pix, vi, H, W):
    """Exact closed acceptance sets of a dyadic scene.

    Returns one dict per view: (i, j) -> list of hits (f, kind, iz) in face order, f a face whose three exact edge
    functions are >= 0 at the pixel centre (either winding), kind STRICT (all three > 0), SHARED (on an edge or vertex,
    every edge it lies on belongs to >= 2 distinct faces) or OUTLINE (it lies on an edge owned by ONE face, or on a vertex
    that such an edge ends in: the sample is on the outline of the mesh although this face's own two edges there are shared), iz the exact
    1 / z of the face's plane at the sample.  Two faces with the same three vertices are one owner."""
    v = np.asarray(v_pix, dtype=np.float64)
    vi = np.asarray(vi, dtype=np.int64)
    B, V = v.shape[:2]
    owners = {}
    valid = [(0 <= vi[f]).all() and (vi[f] < V).all() for f in range(len(vi))]
    for f, (i0, i1, i2) in enumerate(vi.tolist()):
        if valid[f]:
            tri = tuple(sorted((i0, i1, i2)))
            for e in ((i0, i1), (i1, i2), (i2, i0)):
                owners.setdefault(tuple(sorted(e)), set()).add(tri)
    rim = {i for e, tris in owners.items() if len(tris) == 1 for i in e}   # vertices on the outline of the mesh
    views = []
    for b in range(B):
        used = np.unique(vi[valid])
        xy = v[b, used, :2]
        assert np.isfinite(xy).all() and (np.abs(xy) < 4096).all() and (xy * Q == np.round(xy * Q)).all(), \
            "classify() needs dyadic x, y: multiples of 2^-8 below 4096 (then every edge function below is exact)"
        X = np.round(v[b, :, :2] * Q).astype(np.int64)   # units of 2^-8; products < 2^42: exact in int64
        zf = [Fraction(float(z)) if np.isfinite(z) else None for z in v[b, :, 2]]
        hits = {}
        for f, (i0, i1, i2) in enumerate(vi.tolist()):
            if not valid[f] or not (v[b, [i0, i1, i2], 2] > 0).all():
                continue
            (ax, ay), (bx, by), (cx, cy) = X[i0].tolist(), X[i1].tolist(), X[i2].tolist()
            area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            if area == 0:
                continue
            s = 1 if area > 0 else -1
            # pixel j has its centre at (2 j + 1) * Q / 2
            j0, j1 = max(0, -((Q // 2 - min(ax, bx, cx)) // Q)), min(W - 1, (max(ax, bx, cx) - Q // 2) // Q)
            k0, k1 = max(0, -((Q // 2 - min(ay, by, cy)) // Q)), min(H - 1, (max(ay, by, cy) - Q // 2) // Q)
            if j0 > j1 or k0 > k1:
                continue
            px, py = np.meshgrid(np.arange(j0, j1 + 1, dtype=np.int64) * Q + Q // 2,
                                 np.arange(k0, k1 + 1, dtype=np.int64) * Q + Q // 2)
            E0 = s * ((bx - px) * (cy - py) - (by - py) * (cx - px))   # |area(p, b, c)| signed: vertex a's weight
            E1 = s * ((cx - px) * (ay - py) - (cy - py) * (ax - px))
            E2 = s * ((ax - px) * (by - py) - (ay - py) * (bx - px))
            kk, jj = np.nonzero((E0 >= 0) & (E1 >= 0) & (E2 >= 0))
            edges = (tuple(sorted((i1, i2))), tuple(sorted((i2, i0))), tuple(sorted((i0, i1))))   # where E0 / E1 / E2 = 0
            for k, j in zip(kk.tolist(), jj.tolist()):
                e = (int(E0[k, j]), int(E1[k, j]), int(E2[k, j]))
                on = [edges[n] for n in range(3) if e[n] == 0]
                at_vertex = set(on[0]) & set(on[1]) if len(on) == 2 else set()
                kind = STRICT if not on else OUTLINE if any(len(owners[x]) == 1 for x in on) or at_vertex & rim else SHARED
                iz = (Fraction(e[0]) / zf[i0] + Fraction(e[1]) / zf[i1] + Fraction(e[2]) / zf[i2]) / (s * area)
                hits.setdefault((k0 + k, j0 + j), []).append((f, kind, iz))
        views.append(hits)
    return views


class ExactReference:
    """A dyadic scene with its classification."""

    def __init__(self, v_pix, vi, H, W):
        self.kind = "exact"
        self.v_pix, self.vi, self.H, self.W = np.asarray(v_pix, np.float64), np.asarray(vi, np.int64), H, W
        self.views = classify(v_pix, vi, H, W)
        self.ref64 = mesh_ref.rasterize(v_pix, vi, H, W)
        self.ref32 = mesh_ref.rasterize(v_pix, vi, H, W, dtype=np.float32)

    def pixel_kind(self, b, p):
        return min(k for _, k, _ in self.views[b][p])   # STRICT < SHARED < OUTLINE: the strongest claim on the pixel

    def pixels(self, kind):
        return [(b, p) for b, hits in enumerate(self.views) for p in hits if self.pixel_kind(b, p) == kind]


# ---- generic scenes: float64 oracle + a-priori flags ------------------------------------------------------------------------
def _tau(a, b, c, area, px, py):
    dx, dy = px - a[0], py - a[1]
    e3, e4, e6, e7 = (c[1] - a[1]) / area, (a[0] - c[0]) / area, (a[1] - b[1]) / area, (b[0] - a[0]) / area
    M = np.maximum(1.0, np.maximum(np.maximum(np.abs(e3 * dx), np.abs(e4 * dy)),
                                   np.maximum(np.abs(e6 * dx), np.abs(e7 * dy))))
    return TAU * M


def flags(v_pix, vi, H, W):
    """float64, from the oracle's data alone -> edge[B,H,W] bool (some face whose bounds contain the pixel has a
    barycentric within tau of 0), tie[B,H,W] bool (the two nearest covering faces within 32 eps32 in 1 / z), solid[B,H,W]
    int32 (number of faces that cover the pixel with every barycentric > tau: a pixel with solid > 0 is inside the mesh
    beyond rounding and cannot be empty)."""
    v_pix = np.asarray(v_pix, dtype=np.float64)
    B = v_pix.shape[0]
    edge = np.zeros((B, H, W), bool)
    solid = np.zeros((B, H, W), np.int32)
    iz1, iz2 = np.zeros((B, H, W)), np.zeros((B, H, W))
    for b in range(B):
        for f, (k0, k1, j0, j1), px, py, (va, vb, vc), area, (b0, b1, b2) in mesh_ref.faces_over_pixels(v_pix[b], vi, H, W):
            sl = (b, slice(k0, k1 + 1), slice(j0, j1 + 1))
            tau = _tau(va, vb, vc, area, px, py)
            bmin = np.minimum(np.minimum(b0, b1), b2)
            edge[sl] |= np.minimum(np.minimum(np.abs(b0), np.abs(b1)), np.abs(b2)) <= tau
            solid[sl] += bmin > tau
            iz = np.where(bmin >= 0, b0 / va[2] + b1 / vb[2] + b2 / vc[2], 0.0)
            iz2[sl] = np.maximum(iz2[sl], np.minimum(iz1[sl], iz))
            iz1[sl] = np.maximum(iz1[sl], iz)
    tie = (iz2 > 0) & (iz1 - iz2 < TIE * iz1)
    return edge, tie, solid


def bary_at(v_pix, vi, b, f, i, j):
    """float64 barycentrics (mesh_ref's formula), 1 / z, tau and perspective-correct barycentrics of faces f at the centres
    of pixels (i, j) of views b (equal-length integer arrays).  A face the skip rules drop gets NaN."""
    v = np.asarray(v_pix, dtype=np.float64)
    vi = np.asarray(vi, dtype=np.int64)
    V, F = v.shape[1], len(vi)
    b, f, i, j = (np.asarray(x, dtype=np.int64) for x in (b, f, i, j))
    ok = (f >= 0) & (f < F)
    tri = vi[np.where(ok, f, 0)]
    ok &= ((tri >= 0) & (tri < V)).all(1)
    tri = np.where(ok[:, None], tri, 0)
    A, Bv, C = (v[b, tri[:, n]] for n in range(3))
    px, py = j + 0.5, i + 0.5
    with np.errstate(all="ignore"):
        area = (Bv[:, 0] - A[:, 0]) * (C[:, 1] - A[:, 1]) - (Bv[:, 1] - A[:, 1]) * (C[:, 0] - A[:, 0])
        ok &= np.isfinite(A[:, :2]).all(1) & np.isfinite(Bv[:, :2]).all(1) & np.isfinite(C[:, :2]).all(1)
        ok &= (A[:, 2] > 0) & (Bv[:, 2] > 0) & (C[:, 2] > 0) & (area != 0)
        area = np.where(ok, area, 1.0)
        b0 = ((Bv[:, 1] - C[:, 1]) * px + (C[:, 0] - Bv[:, 0]) * py + (Bv[:, 0] * C[:, 1] - C[:, 0] * Bv[:, 1])) / area
        b1 = ((C[:, 1] - A[:, 1]) * px + (A[:, 0] - C[:, 0]) * py + (C[:, 0] * A[:, 1] - A[:, 0] * C[:, 1])) / area
        b2 = ((A[:, 1] - Bv[:, 1]) * px + (Bv[:, 0] - A[:, 0]) * py + (A[:, 0] * Bv[:, 1] - Bv[:, 0] * A[:, 1])) / area
        iz = b0 / A[:, 2] + b1 / Bv[:, 2] + b2 / C[:, 2]
        tau = _tau(A.T, Bv.T, C.T, area, px, py)
        persp = np.stack([b0 / A[:, 2], b1 / Bv[:, 2], b2 / C[:, 2]]) / iz
    nan = np.where(ok, 0.0, np.nan)
    return np.stack([b0, b1, b2]) + nan, iz + nan, tau, persp + nan


class GenericReference:
    """flagged_share: the condition on the scene (flagged <= this share of covered, per view); a scene BUILT to put samples
    on edges states its own.  numeric: False leaves the depth / barycentric bounds out, for a scene whose float32 yardstick
    overflows (then its own error, hence the bound, means nothing)."""

    def __init__(self, v_pix, vi, H, W, flagged_share=FLAGGED_SHARE, numeric=True):
        self.kind = "generic"
        self.flagged_share, self.numeric = flagged_share, numeric
        self.v_pix, self.vi, self.H, self.W = np.asarray(v_pix, np.float64), np.asarray(vi, np.int64), H, W
        self.ref64 = mesh_ref.rasterize(v_pix, vi, H, W)
        self.ref32 = mesh_ref.rasterize(v_pix, vi, H, W, dtype=np.float32)
        self.edge, self.tie, self.solid = flags(v_pix, vi, H, W)
        self.flagged = self.edge | self.tie


# ---- the judge --------------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self, name):
        self.name, self.failures, self.lines, self.ratios = name, [], [], {}

    def fail(self, what, offenders=()):
        self.failures.append(what + "".join("\n      " + o for o in list(offenders)[:6]))

    @property
    def ok(self):
        return not self.failures

    def __str__(self):
        return "\n".join(self.lines + ["  FAIL " + f for f in self.failures])


def _numeric(rep, tag, ref, index, depth, bary, where):
    """Depth / barycentrics over the pixels `where` (index agrees with the oracle there), max norm, nothing left out:
    |got - fp64| <= 2 |ref32 - fp64| + 4 eps32 scale, and |sum(bary) - 1| <= 4 eps32 on every covered pixel of `got`."""
    (ri, rd, rb), (_, d32, b32) = ref.ref64, ref.ref32
    depth, bary = np.asarray(depth, np.float64), np.asarray(bary, np.float64)
    if not (np.isfinite(depth).all() and np.isfinite(bary).all()):
        rep.fail(f"{tag}: non-finite depth / barycentrics")
        return
    empty = index < 0
    if (depth[empty] != 0).any() or (bary[np.broadcast_to(empty[:, None], bary.shape)] != 0).any():
        rep.fail(f"{tag}: an empty pixel holds a depth / barycentric other than 0")
    w3 = np.broadcast_to(where[:, None], bary.shape)
    for what, got, r32, r64, sel, scale in (("depth", depth, d32, rd, where, float(rd.max()) if rd.size else 1.0),
                                            ("bary", bary, b32, rb, w3, 1.0)):
        if not sel.any():
            continue
        err, ref_err = np.abs(got - r64)[sel].max(), np.abs(np.asarray(r32, np.float64) - r64)[sel].max()
        bound = 2.0 * ref_err + 4.0 * EPS32 * scale
        rep.ratios[what] = err / bound
        rep.lines.append(f"[meshraster] {tag} {what}: |got - fp64| = {err:.3e}, reference fp32's own = {ref_err:.3e}, "
                         f"bound = {bound:.3e}, ratio = {err / bound:.3f}")
        if not err <= bound:
            k = int(np.argmax(np.where(sel, np.abs(got - r64), -1.0)))
            rep.fail(f"{tag}: {what} error {err:.3e} > bound {bound:.3e}",
                     [f"at flat index {k} {np.unravel_index(k, got.shape)}: got {got.flat[k]!r}, fp64 {r64.flat[k]!r}"])
    cov = index >= 0
    if cov.any():
        s = np.abs(bary.sum(1) - 1.0)[cov].max()
        rep.ratios["bary_sum"] = s / (4.0 * EPS32)
        rep.lines.append(f"[meshraster] {tag} |sum(bary) - 1| = {s:.3e} (bound {4.0 * EPS32:.3e}, ratio {s / (4.0 * EPS32):.3f})")
        if not s <= 4.0 * EPS32:
            rep.fail(f"{tag}: |sum(bary) - 1| = {s:.3e} > 4 eps32")


def _judge_exact(ref, index, depth, bary, rep):
    F = len(ref.vi)
    counts = {STRICT: 0, SHARED: 0, OUTLINE: 0}
    bad = {"strict": [], "hole": [], "shared": [], "outline": [], "stray": []}
    numeric_ok = np.zeros(index.shape, bool)
    for b, hits in enumerate(ref.views):
        stray = np.argwhere(index[b] >= 0)
        for i, j in stray.tolist():
            if (i, j) not in hits:
                bad["stray"].append(f"view {b} pixel ({i}, {j}): face {index[b, i, j]} where no face's closed set contains the sample")
        for (i, j), hs in hits.items():
            h = int(index[b, i, j])
            kind = min(k for _, k, _ in hs)
            counts[kind] += 1
            top = max(iz for _, _, iz in hs)
            nearest = [f for f, _, iz in hs if iz == top]
            desc = (f"view {b} pixel ({i}, {j}): got face {h}, accepted set "
                    + ", ".join(f"{f}:{'SIO'[k]}:1/z={float(iz):.9g}" for f, k, iz in hs))
            if kind == STRICT and all(k == STRICT for _, k, _ in hs):
                if h != min(nearest):      # exact nearest, exact ties to the lower index.  No cap, no exceptions
                    bad["strict"].append(desc)
                else:
                    numeric_ok[b, i, j] = True
                continue
            allowed = set(nearest)
            if h == -1 and -1 not in allowed:
                bad["outline" if kind == OUTLINE else "hole"].append(desc)
            elif h not in allowed:
                bad["shared" if kind != OUTLINE else "outline"].append(desc)
    rep.lines.append(f"[meshraster] {rep.name}: samples strictly inside {counts[STRICT]}, on a shared edge / vertex "
                     f"{counts[SHARED]}, on an outline edge {counts[OUTLINE]}; wrong: strict {len(bad['strict'])}, holes on "
                     f"interior edges {len(bad['hole'])}, shared-edge {len(bad['shared'])}, outline {len(bad['outline'])}, "
                     f"stray {len(bad['stray'])}")
    rep.counts = dict(strict=counts[STRICT], shared=counts[SHARED], outline=counts[OUTLINE], **{"bad_" + k: len(x) for k, x in bad.items()})
    for k, what in (("strict", "a strictly-inside sample does not hold the exact nearest face"),
                    ("hole", "HOLE: a sample on an interior edge / vertex is empty"),
                    ("shared", "an on-edge sample holds a face that is not an exactly-nearest member of its closed set"),
                    ("outline", "an outline sample is not covered as the stated rule demands"),
                    ("stray", "a face where none may be")):
        if bad[k]:
            rep.fail(f"{len(bad[k])} x {what}", bad[k])
    if ((index < -1) | (index >= F)).any():
        rep.fail("face index out of range")
    _numeric(rep, rep.name, ref, index, depth, bary, numeric_ok)


def _judge_generic(ref, index, depth, bary, rep):
    ri, rd, _ = ref.ref64
    F = len(ref.vi)
    if ((index < -1) | (index >= F)).any():
        rep.fail("face index out of range")
        return
    rep.views = []
    for b in range(index.shape[0]):
        covered, flagged = int((ri[b] >= 0).sum()), int(ref.flagged[b].sum())
        diff = index[b] != ri[b]
        n_flag_diff = int((diff & ref.flagged[b]).sum())
        rep.views.append(dict(covered=covered, flagged=flagged, mismatch_flagged=n_flag_diff,
                              mismatch_unflagged=int((diff & ~ref.flagged[b]).sum())))
        rep.lines.append(f"[meshraster] {rep.name} view {b}: covered {covered}, flagged {flagged} "
                         f"({100.0 * flagged / max(covered, 1):.4f} %), mismatches among flagged {n_flag_diff}, "
                         f"among un-flagged {rep.views[-1]['mismatch_unflagged']}")
        if flagged > ref.flagged_share * covered:
            rep.fail(f"view {b}: the scene does not meet the condition flagged <= {100.0 * ref.flagged_share:g} % of covered "
                     f"({flagged} of {covered})")
    diff = index != ri
    # un-flagged: equal.  No cap on top of the flag
    ub, ui, uj = np.nonzero(diff & ~ref.flagged)
    if len(ub):
        hb, _, _, _ = bary_at(ref.v_pix, ref.vi, ub[:6], index[ub[:6], ui[:6], uj[:6]], ui[:6], uj[:6])
        rep.fail(f"{len(ub)} un-flagged pixels differ from the oracle",
                 [f"view {b} pixel ({i}, {j}): got face {index[b, i, j]}, oracle {ri[b, i, j]}, solid covering faces "
                  f"{ref.solid[b, i, j]}, fp64 barycentrics of the face got {hb[:, n]}" for n, (b, i, j) in
                  enumerate(zip(ub[:6].tolist(), ui[:6].tolist(), uj[:6].tolist()))])
    # flagged and different: the face got must contain the sample within tau and lie at the oracle's depth; empty only at
    # a true silhouette sample (no face covers it beyond rounding)
    fb, fi, fj = np.nonzero(diff & ref.flagged)
    if len(fb):
        h = index[fb, fi, fj]
        hb, hiz, tau, hpb = bary_at(ref.v_pix, ref.vi, fb, np.maximum(h, 0), fi, fj)
        with np.errstate(all="ignore"):
            inside = hb.min(0) >= -tau
            near = np.abs(1.0 / hiz - rd[fb, fi, fj]) <= DEPTH_FLAGGED * rd[fb, fi, fj]
            # ... and what was WRITTEN there must be that face's depth and barycentrics: 64 eps32 relative for the depth
            # (as above), tau (the barycentric error the flag was derived from) + 64 eps32 for the barycentrics
            wrote = (np.abs(depth[fb, fi, fj] - 1.0 / hiz) <= DEPTH_FLAGGED / hiz) & \
                    (np.abs(bary[fb, :, fi, fj].T - hpb).max(0) <= tau + DEPTH_FLAGGED)
        has_ref = ri[fb, fi, fj] >= 0
        okay = np.where(h < 0, ref.solid[fb, fi, fj] == 0, inside & (near | ~has_ref) & wrote)
        if not okay.all():
            w = np.nonzero(~okay)[0]
            rep.fail(f"{len(w)} flagged pixels hold a face (or a hole) that rounding does not explain",
                     [f"view {fb[n]} pixel ({fi[n]}, {fj[n]}): got face {h[n]}, oracle {ri[fb[n], fi[n], fj[n]]}, solid covering "
                      f"faces {ref.solid[fb[n], fi[n], fj[n]]}, fp64 barycentrics of the face got {hb[:, n]}, tau {tau[n]:.3e}, "
                      f"its depth {1.0 / hiz[n]:.9g} vs oracle {rd[fb[n], fi[n], fj[n]]:.9g}, written depth "
                      f"{depth[fb[n], fi[n], fj[n]]:.9g}, written barycentrics {bary[fb[n], :, fi[n], fj[n]]} vs {hpb[:, n]}" for n in w[:6]])
    if ref.numeric:
        _numeric(rep, rep.name, ref, index, depth, bary, ~diff & ~ref.flagged & (ri >= 0))


def judge(ref, index, depth, bary, name="scene"):
    """The comparison of the mesh rasterizer's three images with a reference (ExactReference or GenericReference).

    Exact (dyadic) scenes, per sample: strictly inside -> the exact nearest face, exact ties to the lower index; on a
    shared edge / vertex -> an exactly-nearest member of the closed acceptance set, never empty; on an outline edge ->
    covered; nowhere a face whose closed set does not contain the sample.
    Generic scenes, per view: flagged <= 0.1 % of covered (a condition on the scene); un-flagged pixels equal; a flagged
    pixel that differs holds a face with fp64 min_k b_k >= -tau within 64 eps32 of the oracle's depth, and that face's own
    depth and barycentrics, or is empty only if no face covers it beyond tau.  Both: depth / barycentrics within 2 x the reference's own fp32 distance + 4 eps32
    on every agreeing (un-flagged / strictly inside) covered pixel, |sum(bary) - 1| <= 4 eps32, empty pixels exactly 0."""
    rep = Report(name)
    index = np.asarray(index)
    B = ref.v_pix.shape[0]
    if index.shape != (B, ref.H, ref.W) or np.shape(depth) != index.shape or np.shape(bary) != (B, 3, ref.H, ref.W):
        rep.fail("wrong output shape")
        return rep
    (_judge_exact if ref.kind == "exact" else _judge_generic)(ref, index, np.asarray(depth), np.asarray(bary), rep)
    return rep
