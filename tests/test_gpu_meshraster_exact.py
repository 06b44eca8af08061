"""GPU: gol_mesh_raster (csrc/meshraster.hip) held to its own stated conventions by references that are exact.

Dyadic scenes (lattices with vertices on pixel centres, a fan, slivers, duplicated faces): oracle/mesh_exact.classify
decides coverage with integer arithmetic -- the fill rule, watertightness and tie-breaking without any tolerance.
Generic closed meshes at the sizes the product runs: oracle/mesh_ref.py in float64, equality on every pixel that the
a-priori flags (computed from the oracle's data alone) do not mark, a containment + depth condition on the marked ones,
depth / barycentrics within 2 x the reference's own float32 distance.  Bookkeeping paths (compaction rounds, many views,
odd sizes, hostile input, poisoned outputs, graph replay): index images EQUAL to mesh_ref's on scenes without any flag.
The judge itself is tested on the CPU (tests/test_mesh_exact.py).  Measured figures: DESIGN.md section 2."""
import numpy as np
import pytest
import torch

import mesh_scenes
from oracle import mesh_exact, mesh_ref

pytestmark = pytest.mark.gpu


def _hip(v_pix, vi, H, W, with_bary=True):
    from goliath_amd import meshraster

    out = meshraster.rasterize(torch.from_numpy(np.ascontiguousarray(v_pix)).cuda(), torch.from_numpy(vi).cuda(), H, W,
                               with_bary=with_bary)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _judged(ref, name, out):
    rep = mesh_exact.judge(ref, *out, name=name)
    print(rep)
    assert rep.ok, str(rep)
    return rep


# ---- dyadic scenes: the fill rule, exactly --------------------------------------------------------------------------------------
@pytest.mark.parametrize("winding", [0, 1, 2])
@pytest.mark.parametrize("far", [0, 1])
@pytest.mark.parametrize("cell", list(mesh_scenes.LATTICE_CELLS))
def test_lattice_fill_rule_is_exact_and_watertight(cell, far, winding):
    """Strictly inside: the exact nearest face.  On a shared edge / vertex: an exactly-nearest member of the closed set,
    never empty.  On an outline edge: covered, as the stated rule (all three edge functions >= 0) says."""
    v, f, H, W = mesh_scenes.lattice_scene(cell, far, winding)
    ref = mesh_exact.ExactReference(v, f, H, W)
    rep = _judged(ref, f"lattice {cell} far={far} winding={winding}", _hip(v, f, H, W))
    assert rep.counts["shared"] > 50 and rep.counts["outline"] > 10


def test_fan_and_slivers():
    v, f, H, W = mesh_scenes.fan_and_slivers()
    rep = _judged(mesh_exact.ExactReference(v, f, H, W), "fan and slivers", _hip(v, f, H, W))
    assert rep.counts["outline"] >= 24 and rep.counts["shared"] >= 2


def test_exact_ties_go_to_the_lowest_index_in_every_round_and_every_run():
    """Copies of a block of faces 1024 and 2048 entries later (other compaction rounds) and right next to the original
    (same round, free order in the compacted list): the images are those of the table without the copies, every time."""
    v, table, single, H, W = mesh_scenes.tie_scene()
    ref = mesh_exact.ExactReference(v, table, H, W)
    runs = [_hip(v, table, H, W) for _ in range(3)]
    _judged(ref, "ties", runs[0])
    alone = _hip(v, single, H, W)
    assert (runs[0][0] >= 0).sum() > 1400
    for r in runs:
        for got, want in zip(r, alone):
            assert np.array_equal(got, want)


def test_fine_grid_large_faces_outside_the_exact_range():
    """Dyadic input on the full 2^-8 grid with faces ~100 px across: more bits than fp32 edge functions hold, so the kernel
    promises here what it promises on any mesh -- the generic judge: un-flagged pixels equal to the oracle, a sample within
    rounding of an edge held by a face that contains it within tau, at that face's depth, empty only if NO face covers it
    beyond tau.  A sample exactly on a shared edge may therefore be rejected by both neighbours: the exact classifier
    counts these, the count is printed and recorded -- measured, not asserted to be 0: outside the exact
    range shared edges are NOT watertight on-edge.  (The scene is built to put samples on edges: its flagged share is what
    it is; every other condition holds as on the closed meshes.)"""
    v, f, H, W = mesh_scenes.fine_grid_pairs()
    out = _hip(v, f, H, W)
    _judged(mesh_exact.GenericReference(v, f, H, W, flagged_share=1.0), "fine grid pairs", out)
    hits = mesh_exact.classify(v, f, H, W)[0]
    shared = [p for p, hs in hits.items() if min(k for _, k, _ in hs) == mesh_exact.SHARED]
    strict = [p for p, hs in hits.items() if all(k == mesh_exact.STRICT for _, k, _ in hs)]
    holes = sum(out[0][0][p] < 0 for p in shared)
    foreign = sum(out[0][0][p] not in [g for g, _, _ in hits[p]] for p in shared) - holes
    wrong = sum(out[0][0][p] != hits[p][0][0] for p in strict if len(hits[p]) == 1)
    print(f"[meshraster] fine grid pairs: samples on shared edges {len(shared)}, empty {holes}, held by a face outside their "
          f"closed set {foreign}; strictly inside one face {len(strict)}, of which not that face {wrong}")
    assert len(shared) > 800 and foreign == 0


# ---- generic closed meshes at the sizes the product runs ------------------------------------------------------------------------
@pytest.mark.parametrize("name", mesh_scenes.GENERIC)
def test_closed_mesh_at_product_size(name):
    """Un-flagged pixels equal; flagged ones explained by rounding (no crack inside the silhouette); flagged <= 0.1 % of
    covered; depth / barycentrics within 2 x the float32 reference's own error + 4 eps32, |sum(bary) - 1| <= 4 eps32."""
    v, f, H, W = mesh_scenes.generic_scene(name)
    ref = mesh_scenes.generic_reference(name)
    rep = _judged(ref, name, _hip(v, f, H, W))
    assert all(r["covered"] > 0.05 * H * W for r in rep.views)


# ---- bookkeeping paths ----------------------------------------------------------------------------------------------------------
def _equal_to_mesh_ref(name, v, f, H, W, numeric=True):
    ref = mesh_exact.GenericReference(v, f, H, W, numeric=numeric)
    assert not ref.flagged.any()                 # by construction: nothing for rounding to decide
    out = _hip(v, f, H, W)
    assert np.array_equal(out[0], ref.ref64[0]), (name, np.argwhere(out[0] != ref.ref64[0])[:8])
    _judged(ref, name, out)
    return out


@pytest.mark.parametrize("spread", [False, True])
def test_three_compaction_rounds_on_one_tile(spread):
    """3000 faces at distinct depths inside one tile (a full round of 1024 hits, several 256-record batches); spread:
    tiles with exactly 1024, 1025 and 257 hits."""
    v, f, H, W = mesh_scenes.stack_scene(spread)
    index = _equal_to_mesh_ref(f"stack spread={spread}", v, f, H, W)[0]
    assert len(np.unique(index[index >= 0])) > (40 if spread else 10)


@pytest.mark.parametrize("H,W", [(16, 16), (24, 40)])
def test_300_views_with_empty_and_off_screen_ones(H, W):
    v, f, _, _ = mesh_scenes.many_views(300, H, W)
    index = _equal_to_mesh_ref(f"300 views {H}x{W}", v, f, H, W)[0]
    seen = (index >= 0).reshape(300, -1).any(1)
    assert seen[0::6].all() and not seen[np.arange(300) % 6 != 0].any()


def test_no_faces_and_no_views():
    from goliath_amd import meshraster

    v, f, H, W = mesh_scenes.soup(5, 20, 24, 1)
    index, depth, bary = _hip(v, f[:0], H, W)
    assert (index == -1).all() and (depth == 0).all() and (bary == 0).all()
    out = meshraster.rasterize(torch.zeros(0, 15, 3, device="cuda"), torch.from_numpy(f).cuda(), H, W)
    assert out[0].shape == (0, H, W) and out[1].shape == (0, H, W) and out[2].shape == (0, 3, H, W)


@pytest.mark.parametrize("H,W,n,seed", [(1, 1, 3, 1), (35, 33, 40, 2), (250, 17, 300, 3), (16, 1024, 600, 4)])
def test_odd_sizes(H, W, n, seed):
    """1 x 1; 33 x 35 with one view (pixel count not a multiple of 4: the scalar clear path); 17 x 250; 1024 x 16."""
    v, f, _, _ = mesh_scenes.soup(n, H, W, seed, Lmax=3 if H == 1 else 12, margin=1 if H == 1 else 4)
    index = _equal_to_mesh_ref(f"{W}x{H}", v, f, H, W)[0]
    assert (index >= 0).any()


@pytest.mark.parametrize("huge", [False, True])
def test_hostile_faces_are_skipped_and_the_others_unaffected(huge):
    """vi = -1 and vi >= V, NaN / inf in x, y and z, z = 0, z < 0, zero area; faces touching only the last column, the last
    row and the corner sample; huge: faces with vertices at +-1e6 and +-1e30 pixels covering the whole image, two views (the
    face with vi = V would find the second view's first vertex).  huge: index, coverage and exact zeros only -- the float32
    yardstick overflows on the 1e30 face, its own error is no bound; the other faces' numbers are judged without it."""
    v, f, H, W = mesh_scenes.hostile_scene(huge)
    P = mesh_scenes.HOSTILE
    assert f[26, 1] == v.shape[1]
    index, depth, bary = _equal_to_mesh_ref(f"hostile huge={huge}", v, f, H, W, numeric=not huge)
    assert not set(np.unique(index).tolist()) & set(P["skipped"])
    assert index[0, H - 1, W - 1] == P["corner"] and (index[0, :, W - 1] == P["column"]).any() and (index[0, H - 1, :] == P["row"]).any()
    if huge:
        assert (index >= 0).all() and (index[0] == P["huge_1e6"]).any() and (index[1] == P["huge_1e30"]).any()
        assert np.isfinite(depth).all() and np.isfinite(bary).all()
        # a face of constant depth z: the image holds z wherever a huge face shows.  Each barycentric carries <= 4 eps32 M
        # (derivation in oracle/mesh_exact.py; M ~ 1 for these faces), 12 eps32 on their sum, plus the roundings of the
        # sum and the reciprocal: 16 eps32
        for face, z in ((P["huge_1e6"], 5.0), (P["huge_1e30"], 6.0)):
            assert np.abs(depth[0][index[0] == face] - z).max(initial=0.0) <= 16 * mesh_exact.EPS32 * z
            assert np.abs(depth[1][index[1] == face] - (11.0 - z)).max(initial=0.0) <= 16 * mesh_exact.EPS32 * z


def test_poisoned_outputs_come_back_fully_written_and_bary_is_optional():
    """Through the ABI call itself: outputs pre-filled with NaN / garbage are fully written; bary_img = NULL gives the same
    index and depth."""
    import ctypes

    from goliath_amd import _lib
    from goliath_amd._lib import c_int, fptr, iptr, stream_ptr

    v, f, H, W = mesh_scenes.soup(40, 35, 33, 2)
    ref = mesh_ref.rasterize(v, f, H, W)
    v_pix, vi = torch.from_numpy(v).cuda(), torch.from_numpy(f).int().cuda()
    fn = _lib.load().gol_mesh_raster_workspace_bytes
    fn.restype = ctypes.c_int64
    ws = torch.full((int(fn(c_int(1), c_int(len(f)))) // 4,), -7, dtype=torch.int32, device="cuda")
    outs = []
    for with_bary in (True, False):
        index = torch.full((1, H, W), 123456, dtype=torch.int32, device="cuda")
        depth = torch.full((1, H, W), float("nan"), device="cuda")
        bary = torch.full((1, 3, H, W), float("nan"), device="cuda") if with_bary else None
        _lib.call("gol_mesh_raster", c_int(1), c_int(v.shape[1]), c_int(len(f)), c_int(H), c_int(W), fptr(v_pix), iptr(vi),
                  iptr(index), fptr(depth), fptr(bary), iptr(ws), stream_ptr())
        torch.cuda.synchronize()
        outs.append((index.cpu().numpy(), depth.cpu().numpy(), None if bary is None else bary.cpu().numpy()))
    (i0, d0, b0), (i1, d1, _) = outs
    assert np.array_equal(i0, ref[0]) and np.isfinite(d0).all() and np.isfinite(b0).all()
    assert (d0[i0 < 0] == 0).all() and (b0[np.broadcast_to((i0 < 0)[:, None], b0.shape)] == 0).all()
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)


def test_graph_replay_on_changed_vertices_equals_eager():
    from goliath_amd import graphs, meshraster

    v, f, H, W = mesh_scenes.generic_scene("spheres512")
    v_pix, vi = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    moved = torch.from_numpy(np.ascontiguousarray(v[::-1])).cuda() + torch.tensor([3.25, -2.5, 0.1], device="cuda")
    cap = graphs.CapturedStep(lambda: meshraster.rasterize(v_pix, vi, H, W))
    v_pix.copy_(moved)
    replayed = [t.clone() for t in cap.replay()]
    eager = meshraster.rasterize(moved, vi, H, W)
    first = meshraster.rasterize(torch.from_numpy(v).cuda(), vi, H, W)
    assert not torch.equal(first[0], eager[0])
    for r, e in zip(replayed, eager):
        assert torch.equal(r, e)
