"""CPU: the yardsticks of the mesh-rasterizer tests are proven before a GPU is involved (oracle/mesh_ref.py with the
kernel's skip rules, oracle/mesh_exact.py: exact classifier, a-priori flags, the judge).

"The judge has teeth": mesh_ref's own output with ONE seeded defect is rejected, every defect; mesh_ref's formulas
evaluated in float32 numpy are accepted on every generic scene -- the caps are reachable by a correct implementation --
and every generic scene meets the condition flagged <= 0.1 % of covered."""
import numpy as np
import pytest
import torch

import mesh_scenes
from oracle import mesh_exact, mesh_ref
from scenes import icosphere, look_at_viewmat


def _mesh_ref_before(v_pix, vi, H, W):
    """oracle/mesh_ref.rasterize as it was before it learnt the kernel's skip rules (kept verbatim as the yardstick of
    'equals its old self')."""
    v_pix = np.asarray(v_pix, dtype=np.float64)
    vi = np.asarray(vi, dtype=np.int64)
    B = v_pix.shape[0]
    index = -np.ones((B, H, W), np.int32)
    best_iz = np.zeros((B, H, W))
    bary = np.zeros((B, 3, H, W))
    for b in range(B):
        for f, (i0, i1, i2) in enumerate(vi):
            (ax, ay, az), (bx, by, bz), (cx, cy, cz) = v_pix[b, i0], v_pix[b, i1], v_pix[b, i2]
            area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            if not (az > 0 and bz > 0 and cz > 0) or area == 0:
                continue
            j0, j1 = max(0, int(np.ceil(min(ax, bx, cx) - 0.5))), min(W - 1, int(np.floor(max(ax, bx, cx) - 0.5)))
            k0, k1 = max(0, int(np.ceil(min(ay, by, cy) - 0.5))), min(H - 1, int(np.floor(max(ay, by, cy) - 0.5)))
            if j0 > j1 or k0 > k1:
                continue
            px, py = np.meshgrid(np.arange(j0, j1 + 1) + 0.5, np.arange(k0, k1 + 1) + 0.5)
            b0 = ((by - cy) * px + (cx - bx) * py + (bx * cy - cx * by)) / area
            b1 = ((cy - ay) * px + (ax - cx) * py + (cx * ay - ax * cy)) / area
            b2 = ((ay - by) * px + (bx - ax) * py + (ax * by - bx * ay)) / area
            w0, w1, w2 = b0 / az, b1 / bz, b2 / cz
            iz = w0 + w1 + w2
            sl = (b, slice(k0, k1 + 1), slice(j0, j1 + 1))
            win = (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & (iz > best_iz[sl])
            best_iz[sl] = np.where(win, iz, best_iz[sl])
            index[sl] = np.where(win, f, index[sl])
            for c, w in enumerate((w0, w1, w2)):
                s = (b, c, slice(k0, k1 + 1), slice(j0, j1 + 1))
                bary[s] = np.where(win, w / np.where(iz != 0, iz, 1.0), bary[s])
    depth = np.where(index >= 0, 1.0 / np.where(best_iz != 0, best_iz, 1.0), 0.0)
    return index, depth, bary


@pytest.mark.parametrize("H,W,subdiv", [(96, 80, 2), (130, 67, 3), (16, 16, 0)])
def test_extended_mesh_ref_equals_its_old_self(H, W, subdiv):
    """The three scenes of tests/test_gpu_meshraster.py::test_mesh_raster_matches_numpy_oracle, bit for bit."""
    import math

    from goliath_amd import meshraster

    B = 2
    verts, faces = icosphere(subdiv)
    g = torch.Generator().manual_seed(subdiv)
    verts = verts[None].repeat(B, 1, 1) * (1.0 + 0.15 * torch.rand(B, verts.shape[0], 1, generator=g))
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = 0.9 * W
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W / 2.0, H / 2.0, 1.0
    Rt = torch.stack([look_at_viewmat((3.0 * math.sin(0.7 * b), 0.3 * b, -3.0 * math.cos(0.7 * b))) for b in range(B)])
    v_pix = meshraster.transform(verts, K, Rt).numpy()
    old, new = _mesh_ref_before(v_pix, faces.numpy(), H, W), mesh_ref.rasterize(v_pix, faces.numpy(), H, W)
    assert (old[0] >= 0).mean() > 0.15
    for o, n in zip(old, new):
        assert o.dtype == n.dtype and np.array_equal(o, n)


def test_mesh_ref_skips_what_the_kernel_skips():
    v, f, H, W = mesh_scenes.hostile_scene(huge=True)
    index, depth, bary = mesh_ref.rasterize(v, f, H, W)
    P = mesh_scenes.HOSTILE
    assert f[26, 1] == v.shape[1] and v.shape[0] == 2            # a vertex index of exactly V, two views
    assert not (set(np.unique(index).tolist()) & set(P["skipped"]))
    assert np.isfinite(depth).all() and np.isfinite(bary).all()
    assert (index >= 0).all()                                    # the huge faces cover the whole image
    assert {P["z_inf"], P["column"], P["row"], P["corner"]} <= set(np.unique(index).tolist())
    assert (index[0, :, W - 1] == P["column"]).sum() >= 1 and (index[0, H - 1, :] == P["row"]).sum() >= 1
    assert index[0, H - 1, W - 1] == P["corner"] and (index[0] == P["corner"]).sum() == 1
    # a range check that let V through would draw the face at V from the next view's first vertex, in front of everything
    wrong = f.copy()
    wrong[26, 1] = 0
    assert (mesh_ref.rasterize(v, wrong, H, W)[0] == 26).any()
    # without the skip rules numpy would have wrapped vi = -1 to the last vertex
    index2, _, _ = mesh_ref.rasterize(*mesh_scenes.hostile_scene(huge=False))
    front = index < len(f) - 2
    assert (index2 == -1).any() and np.array_equal(index2[0][front[0]], index[0][front[0]])
    assert set(np.unique(index[0][index2[0] < 0]).tolist()) == {len(f) - 2} and set(np.unique(index[1][index2[0] < 0]).tolist()) == {len(f) - 1}


# ---- the dyadic classifier ------------------------------------------------------------------------------------------------------
DYADIC = [("3x5", 0, 0), ("7x3", 1, 1), ("3.5x2.5s", 0, 2), ("3.5x2.5s", 1, 0), ("5x5", 1, 2), ("1x1", 0, 1),
          ("2.5x6s", 1, 1), ("11x13", 0, 2)]


def _exact_refs():
    for cell, far, winding in DYADIC:
        yield f"lattice {cell} far={far} winding={winding}", mesh_exact.ExactReference(*mesh_scenes.lattice_scene(cell, far, winding))
    yield "fan and slivers", mesh_exact.ExactReference(*mesh_scenes.fan_and_slivers())


def test_classifier_agrees_with_mesh_ref_strictly_inside_and_finds_the_edge_samples():
    total = {mesh_exact.STRICT: 0, mesh_exact.SHARED: 0, mesh_exact.OUTLINE: 0}
    for name, ref in _exact_refs():
        ri = ref.ref64[0]
        for kind in total:
            total[kind] += len(ref.pixels(kind))
        for b, hits in enumerate(ref.views):
            assert np.array_equal(ri[b] >= 0, _mask(hits, ri[b].shape)), name   # closed rule: mesh_ref covers the closed set
            for (i, j), hs in hits.items():
                if all(k == mesh_exact.STRICT for _, k, _ in hs):
                    top = max(iz for _, _, iz in hs)
                    assert ri[b, i, j] == min(f for f, _, iz in hs if iz == top), (name, b, i, j)
                else:       # on an edge mesh_ref's float64 answer is one of the exactly-nearest members
                    top = max(iz for _, _, iz in hs)
                    assert ri[b, i, j] in [f for f, _, iz in hs if iz == top], (name, b, i, j)
        rep = mesh_exact.judge(ref, *ref.ref64, name=name)
        assert rep.ok, str(rep)
    print("samples strictly inside / on shared edges / on outline edges:", total)
    assert total[mesh_exact.SHARED] > 2000 and total[mesh_exact.OUTLINE] > 300 and total[mesh_exact.STRICT] > 20000


def _mask(hits, shape):
    m = np.zeros(shape, bool)
    for i, j in hits:
        m[i, j] = True
    return m


def test_fan_and_slivers_hold_the_samples_they_were_built_for():
    ref = mesh_exact.ExactReference(*mesh_scenes.fan_and_slivers())
    hits = ref.views[0]
    for ox, oy in ((0, 0), (880, 690)):
        centre = hits[(oy + 30, ox + 20)]
        assert len(centre) == 7 and all(k == mesh_exact.SHARED for _, k, _ in centre)
        for n in range(12):
            (f, k, _), = hits[(oy + 10, ox + 24 + 4 * n)]
            assert k == mesh_exact.OUTLINE


def test_classifier_refuses_non_dyadic_input():
    v, f, H, W = mesh_scenes.fan_and_slivers()
    v = v.copy()
    v[0, 3, 0] += 1e-3
    with pytest.raises(AssertionError):
        mesh_exact.classify(v, f, H, W)


# ---- the judge has teeth: exact scenes ------------------------------------------------------------------------------------------
def _copy(ref):
    return tuple(np.array(x, copy=True) for x in ref.ref64)


def _rejects(ref, index, depth, bary, needle):
    rep = mesh_exact.judge(ref, index, depth, bary)
    assert not rep.ok and needle in "\n".join(rep.failures), (needle, str(rep))


def test_judge_rejects_defects_on_edges_and_ties():
    ref = mesh_exact.ExactReference(*mesh_scenes.lattice_scene("3x5", 0, 0))
    assert mesh_exact.judge(ref, *ref.ref64).ok
    # one shared-edge sample left empty: a hole on an interior edge
    (b, (i, j)) = ref.pixels(mesh_exact.SHARED)[7]
    index, depth, bary = _copy(ref)
    index[b, i, j], depth[b, i, j], bary[b, :, i, j] = -1, 0.0, 0.0
    _rejects(ref, index, depth, bary, "HOLE")
    # one shared-edge sample given a face that does not contain it
    index, depth, bary = _copy(ref)
    inside = {f for f, _, _ in ref.views[b][(i, j)]}
    index[b, i, j] = next(f for f in range(len(ref.vi)) if f not in inside)
    _rejects(ref, index, depth, bary, "not an exactly-nearest member")
    # one outline sample left empty (the stated rule covers it)
    (b, (i, j)) = ref.pixels(mesh_exact.OUTLINE)[3]
    index, depth, bary = _copy(ref)
    index[b, i, j], depth[b, i, j], bary[b, :, i, j] = -1, 0.0, 0.0
    _rejects(ref, index, depth, bary, "outline sample")
    # a face where none may be
    index, depth, bary = _copy(ref)
    i, j = np.argwhere(index[0] < 0)[0]
    index[0, i, j], depth[0, i, j], bary[0, :, i, j] = 0, 2.5, (1.0, 0.0, 0.0)
    _rejects(ref, index, depth, bary, "a face where none may be")
    # an exact tie resolved to the higher face index
    v, table, single, H, W = mesh_scenes.tie_scene()
    tie = mesh_exact.ExactReference(v, table, H, W)
    assert mesh_exact.judge(tie, *tie.ref64).ok
    assert np.array_equal(tie.ref64[0], mesh_ref.rasterize(v, single, H, W)[0])      # the copies never win
    index, depth, bary = _copy(tie)
    strict = [(b, p) for b, p in tie.pixels(mesh_exact.STRICT) if tie.ref64[0][b][p] < 64]
    b, (i, j) = strict[5]
    index[b, i, j] += 1024
    _rejects(tie, index, depth, bary, "exact nearest face")
    index[b, i, j] += 1024
    _rejects(tie, index, depth, bary, "exact nearest face")
    b, (i, j) = next((b, p) for b, p in tie.pixels(mesh_exact.STRICT) if 64 <= tie.ref64[0][b][p] < 192)
    index, depth, bary = _copy(tie)
    assert (table[index[b, i, j]] == table[index[b, i, j] + 1]).all()
    index[b, i, j] += 1
    _rejects(tie, index, depth, bary, "exact nearest face")


# ---- the judge has teeth: generic scenes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mesh_scenes.GENERIC)
def test_generic_scene_meets_the_condition_and_float32_numpy_passes(name):
    ref = mesh_scenes.generic_reference(name)
    for b in range(ref.flagged.shape[0]):
        covered, flagged = int((ref.ref64[0][b] >= 0).sum()), int(ref.flagged[b].sum())
        print(f"{name} view {b}: covered {covered}, flagged {flagged} ({100.0 * flagged / covered:.4f} %)")
        assert covered > 0.05 * ref.H * ref.W and flagged <= mesh_exact.FLAGGED_SHARE * covered
    assert mesh_exact.judge(ref, *ref.ref64, name=name).ok
    rep = mesh_exact.judge(ref, *ref.ref32, name=name + " float32 numpy")
    print(rep)
    assert rep.ok, str(rep)


def _interior(ref, b=0):
    """An un-flagged pixel covered beyond rounding by a front and a back face, away from every flagged pixel."""
    ok = (ref.solid[b] >= 2) & ~ref.flagged[b]
    ii, jj = np.nonzero(ok)
    k = len(ii) // 2
    return b, int(ii[k]), int(jj[k])


def test_judge_rejects_every_seeded_defect_on_a_generic_scene():
    ref = mesh_scenes.generic_reference("spheres512")
    F = len(ref.vi)
    assert F > 2048
    b, i, j = _interior(ref)
    # a single interior pixel set to -1
    index, depth, bary = _copy(ref)
    index[b, i, j], depth[b, i, j], bary[b, :, i, j] = -1, 0.0, 0.0
    _rejects(ref, index, depth, bary, "un-flagged pixels differ")
    # a single interior pixel given the back face of the closed mesh
    n = np.arange(F)
    bb, iz, tau, _ = mesh_exact.bary_at(ref.v_pix, ref.vi, np.full(F, b), n, np.full(F, i), np.full(F, j))
    covering = n[np.nan_to_num(bb.min(0), nan=-1.0) > tau]
    assert len(covering) >= 2 and ref.ref64[0][b, i, j] == covering[np.argmax(iz[covering])]
    back = covering[np.argmin(iz[covering])]
    index, depth, bary = _copy(ref)
    index[b, i, j] = back
    _rejects(ref, index, depth, bary, "un-flagged pixels differ")
    # ... and the same at a FLAGGED pixel inside the silhouette: the flag is no licence for a face at another depth, or a hole
    fb, fi, fj = (x[0] for x in np.nonzero(ref.flagged & (ref.solid >= 1) & (ref.ref64[0] >= 0)))
    bb, iz, tau, _ = mesh_exact.bary_at(ref.v_pix, ref.vi, np.full(F, fb), n, np.full(F, fi), np.full(F, fj))
    covering = n[np.nan_to_num(bb.min(0), nan=-1.0) >= 0]
    back = covering[np.argmin(iz[covering])]
    assert 1.0 / iz[back] > 1.01 * ref.ref64[1][fb, fi, fj]
    index, depth, bary = _copy(ref)
    index[fb, fi, fj] = back
    _rejects(ref, index, depth, bary, "rounding does not explain")
    index[fb, fi, fj] = -1
    _rejects(ref, index, depth, bary, "rounding does not explain")
    # one tile (16 x 16) of one view left at "no face"
    index, depth, bary = _copy(ref)
    ti, tj = 16 * (i // 16), 16 * (j // 16)
    index[b, ti:ti + 16, tj:tj + 16], depth[b, ti:ti + 16, tj:tj + 16], bary[b, :, ti:ti + 16, tj:tj + 16] = -1, 0.0, 0.0
    _rejects(ref, index, depth, bary, "un-flagged pixels differ")
    # the faces 1024.. (second compaction round) dropped
    dropped = mesh_ref.rasterize(ref.v_pix, ref.vi[:1024], ref.H, ref.W)
    assert (dropped[0] != ref.ref64[0]).any()
    _rejects(ref, *dropped, "un-flagged pixels differ")
    # one pixel's depth off by 1e-4 relative
    index, depth, bary = _copy(ref)
    depth[b, i, j] *= 1.0 + 1e-4
    _rejects(ref, index, depth, bary, "depth error")
    # barycentrics permuted at one pixel
    index, depth, bary = _copy(ref)
    assert np.abs(bary[b, 0, i, j] - bary[b, 1, i, j]) > 1e-3
    bary[b, :, i, j] = bary[b, [1, 0, 2], i, j]
    _rejects(ref, index, depth, bary, "bary error")
    # barycentrics that do not sum to 1; garbage in an empty pixel; NaN
    index, depth, bary = _copy(ref)
    bary[b, :, i, j] *= 1.0 + 1e-6
    _rejects(ref, index, depth, bary, "sum(bary)")
    index, depth, bary = _copy(ref)
    ei, ej = np.argwhere(index[b] < 0)[0]
    depth[b, ei, ej] = 1e-30
    _rejects(ref, index, depth, bary, "empty pixel")
    depth[b, ei, ej] = np.nan
    _rejects(ref, index, depth, bary, "non-finite")


def test_judge_checks_what_is_written_next_to_a_legitimately_different_face():
    """At a flagged pixel the neighbour across the edge is as good an answer as the oracle's face -- with ITS depth and
    barycentrics.  The same face with a depth off by 1e-4, or with the oracle face's barycentrics, is rejected."""
    ref = mesh_scenes.generic_reference("light1024")
    F, n = len(ref.vi), np.arange(len(ref.vi))
    found = 0
    for b, i, j in np.argwhere(ref.flagged & (ref.ref64[0] >= 0)).tolist():
        hb, hiz, tau, hpb = mesh_exact.bary_at(ref.v_pix, ref.vi, np.full(F, b), n, np.full(F, i), np.full(F, j))
        with np.errstate(all="ignore"):
            alt = (hb.min(0) >= -tau) & (np.abs(1.0 / hiz - ref.ref64[1][b, i, j]) <= mesh_exact.DEPTH_FLAGGED * ref.ref64[1][b, i, j])
        alt[ref.ref64[0][b, i, j]] = False
        if not alt.any():
            continue
        h = int(n[alt][0])
        if np.abs(hpb[:, h] - ref.ref64[2][b, :, i, j]).max() < 0.1:   # (duplicate geometry: nothing to tell apart)
            continue
        found += 1
        index, depth, bary = _copy(ref)
        index[b, i, j], depth[b, i, j], bary[b, :, i, j] = h, 1.0 / hiz[h], hpb[:, h]
        rep = mesh_exact.judge(ref, index, depth, bary)
        assert rep.ok, str(rep)
        depth[b, i, j] *= 1.0 + 1e-4
        _rejects(ref, index, depth, bary, "rounding does not explain")
        depth[b, i, j], bary[b, :, i, j] = 1.0 / hiz[h], ref.ref64[2][b, :, i, j]
        _rejects(ref, index, depth, bary, "rounding does not explain")
        if found == 3:
            break
    assert found >= 1


def test_soup_scenes_raise_no_flag():
    """The bookkeeping scenes of the GPU test are un-flagged by construction: there the index image must be EQUAL."""
    for v, f, H, W in (mesh_scenes.stack_scene(False), mesh_scenes.stack_scene(True), mesh_scenes.many_views(12, 16, 16),
                       mesh_scenes.many_views(12, 24, 40), mesh_scenes.hostile_scene(False), mesh_scenes.hostile_scene(True),
                       mesh_scenes.soup(3, 1, 1, 1, Lmax=3, margin=1), mesh_scenes.soup(40, 35, 33, 2),
                       mesh_scenes.soup(300, 250, 17, 3), mesh_scenes.soup(600, 16, 1024, 4)):
        edge, tie, solid = mesh_exact.flags(v, f, H, W)
        assert not edge.any() and not tie.any()
        assert (solid > 0).any()
    v, f, H, W = mesh_scenes.stack_scene(False)
    index = mesh_ref.rasterize(v, f, H, W)[0]
    assert (index[0, 48:64, 32:48] >= 0).sum() > 100 and (index >= 0).sum() == (index[0, 48:64, 32:48] >= 0).sum()
