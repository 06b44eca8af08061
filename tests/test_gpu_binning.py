"""GPU parity of gol_bin_sort (csrc/binning.hip) with the CPU oracle (oracle/gsplat_oracle.c: orc_bin_sort), integer-exact,
on the control flow the single-tile tests of test_gpu_splat.py do not reach: both long-list queues at once and overflowing,
queue capacity 0 and 1, views b > 0, images with more tiles than the staged scan / the LDS count and scatter hold, the
pruned mode's contract against a brute-force float64 reference, capacity overflow, depth edge cases, and the library's
process-wide statics.  Inputs: tests/binning_cases.py (guarded on the CPU by tests/test_binning_cases.py).

Which branch each test reaches:
  (a) both_queues           sort_kernel's queue push, MID from the front and BIG from the back of one view's queue, both
                            drained by sort_mid_kernel / sort_big_kernel; every size class of the tile kernel beside them
  (b) queues_overflow       slot >= cap: the in-place bitonic_sort branch of sort_kernel next to queued lists
  (c) degenerate_queues     queue_cap(T) / 2 == 0 (T <= 3: no atomic at all) and == 1 (T = 4, 5)
  (d) multi_view            queue + b T, keys + b capacity, bins + b T 2, an empty view between two busy ones
  (e) mixed_footprints      ids repeated across lists, lengths where they fall; row_span / wrapped masks with conics
  (f) depth_edges           bucket_sort_tile accepting ties, scale = 0, scale = inf, the decline test, in all three kernels
  (g) many_tiles            scan_kernel's last staged size and its unstaged loop; count_lds / scatter_lds at their last size;
                            count_kernel / scatter_kernel (global atomics, tile_reached) beyond it
  (h) prune_contract        tile_box(tight), row_span, hm == false re-test, !rc.exact, tau < 0; the render over pruned lists
  (i) capacity_overflow     slot < capacity guards, tile_range's clamp, sorting a truncated list
  (j) library_statics       GOL_SORT_BIG_NO_LDS, GOL_BIN_WGS, GOL_BIN_WGS2 (chunk 4096: mask registers k = 0..3, 16-bit
                            packed counters at 4096) in one fresh child process
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import binning_cases as bc

pytestmark = pytest.mark.gpu


# ---- helpers ---------------------------------------------------------------------------------------------------------
def run_hip(views, H, W, capacity, pruned=False):
    """One gol_bin_sort call over `views` (a list of scene tuples of one N).  Returns the workspace."""
    from goliath_amd import splat

    B, N = len(views), views[0][0].shape[0]
    stack = lambda k: torch.stack([v[k] for v in views]).cuda().contiguous()
    tx, ty = bc.tiles_of(H, W)
    ws = splat._Workspace(B, N, tx * ty, capacity, "cuda")
    ws.sorted_ids.fill_(-1)
    args = (stack(3), stack(4)) if pruned else ()
    splat._bin_sort(B, N, stack(0), stack(1), stack(2), H, W, ws, *args)
    torch.cuda.synchronize()
    return ws


def assert_exact(ws, b, ids, bins):
    """View b of the workspace holds exactly the oracle's lists."""
    I = ids.numel()
    assert int(ws.n_isect[b]) == I
    hb = ws.tile_bins[b].cpu()
    assert torch.equal(hb[:, 1] - hb[:, 0], bins[:, 1] - bins[:, 0])
    busy = bins[:, 1] > bins[:, 0]
    assert torch.equal(hb[busy], bins[busy])          # (the oracle leaves the bins of empty tiles at 0)
    got = ws.sorted_ids[b, :I].cpu()
    if not torch.equal(got, ids):
        bad = (got != ids).nonzero()[:, 0]
        tile = int((bins[:, 1] > int(bad[0])).nonzero()[0, 0])
        raise AssertionError(f"view {b}: {bad.numel()} of {I} list entries differ, first at {int(bad[0])} "
                             f"(tile {tile}, list of {int(bins[tile, 1] - bins[tile, 0])})")


def hip_pairs(ws, b, N):
    """(tile, id) of every entry of view b's lists, concatenated in tile order."""
    hb = ws.tile_bins[b].cpu().numpy().astype(np.int64)
    lens = hb[:, 1] - hb[:, 0]
    assert (lens >= 0).all()
    tile = np.repeat(np.arange(hb.shape[0]), lens)
    at = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens) + np.repeat(hb[:, 0], lens)
    ids = ws.sorted_ids[b].cpu().numpy().astype(np.int64)[at]
    assert ((ids >= 0) & (ids < N)).all()
    return tile, ids, hb


def check_pruned(ws, b, N, ids, bins, live, capacity):
    """The pruning contract of one view (every tile): order-preserving subsequence of the oracle's list, every live pair
    kept, segments inside their reservations.  Returns kept[I] bool over the oracle's pairs."""
    T = bins.shape[0]
    tile_h, ids_h, hb = hip_pairs(ws, b, N)
    lens_o = (bins[:, 1] - bins[:, 0]).numpy().astype(np.int64)
    key_o = np.repeat(np.arange(T), lens_o) * N + ids.numpy().astype(np.int64)
    order = np.argsort(key_o, kind="stable")
    key_h = tile_h * N + ids_h
    at = np.minimum(np.searchsorted(key_o[order], key_h), key_o.size - 1)
    assert (key_o[order][at] == key_h).all(), "a pruned list holds a Gaussian that gsplat's list of the tile does not"
    pos = order[at]
    assert (np.diff(pos) > 0).all(), "a pruned list is not an order-preserving subsequence of gsplat's list"
    kept = np.zeros(key_o.size, bool)
    kept[pos] = True
    lost = live & ~kept
    assert not lost.any(), (f"{int(lost.sum())} visible (Gaussian, tile) pairs were pruned, e.g. Gaussian "
                            f"{int(ids[int(lost.nonzero()[0][0])])} in tile {int(key_o[lost.nonzero()[0][0]] // N)}")
    n_isect = int(ws.n_isect[b])
    assert int((hb[:, 1] - hb[:, 0]).sum()) <= n_isect <= capacity
    assert (hb[:-1, 1] <= hb[1:, 0]).all() and (hb[:, 0] <= hb[:, 1]).all() and hb[0, 0] == 0 and hb[-1, 1] <= n_isect
    return kept


@functools.lru_cache(maxsize=None)
def planned(name):
    spec = {"a": bc.PLAN_A, "b": bc.PLAN_B, **{f"c{T}": p for T, p in bc.PLANS_C.items()}}[name]
    scene = bc.planned_lists(*spec)
    xys, depths, radii, H, W, plan = scene
    ids, bins = bc.oracle_lists(xys, depths, radii, H, W)
    assert (bins[:, 1] - bins[:, 0]).tolist() == [plan.get(t, 0) for t in range(bins.shape[0])]
    return scene, ids, bins


@functools.lru_cache(maxsize=None)
def prune_case(seed):
    scene = bc.prune_scene(seed)
    xys, depths, radii, conics, opac, H, W = scene
    lists = bc.oracle_lists(xys, depths, radii, H, W)
    return scene, lists, bc.prune_reference(xys, radii, conics, opac, H, W, lists)


# ---- (a) (b) (c): the two long-list queues -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c1", "c2", "c3", "c4", "c5"])
def test_queues(name):
    """(a) both queues populated, no overflow; (b) both overflowing into the in-place network (which list overflows is up
    to the atomics: the ids must be exact regardless); (c) queue capacity 0 and 1."""
    scene, ids, bins = planned(name)
    H, W = scene[3], scene[4]
    ws = run_hip([scene], H, W, ids.numel())
    assert_exact(ws, 0, ids, bins)


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def test_multi_view():
    """Three views in one call on the 64 x 64 image: (b)'s Gaussians, nothing, (a)'s Gaussians."""
    (sa, _, _), (sb, _, _) = planned("a"), planned("b")
    H, W = 64, 64
    N = max(sa[0].shape[0], sb[0].shape[0])
    v0, v2 = bc.pad_to(*sb[:3], N), bc.pad_to(*sa[:3], N)
    v1 = (v0[0], v0[1], torch.zeros(N, dtype=torch.int32))
    views = [v0, v1, v2]
    refs = [bc.oracle_lists(*v, H, W) for v in views]
    assert refs[1][0].numel() == 0 and refs[0][0].numel() == sb[0].shape[0] and refs[2][0].numel() == sa[0].shape[0]
    assert int((refs[0][1][:, 1] - refs[0][1][:, 0]).max()) == 17000      # (b)'s tiles 0..7 are tiles 0..7 here too
    ws = run_hip(views, H, W, N)
    for b, (ids, bins) in enumerate(refs):
        assert_exact(ws, b, ids, bins)
    assert int(ws.tile_bins[1].max()) == 0


# ---- (e) ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_case():
    scene = bc.radius_set_scene()
    xys, depths, radii, conics, opac, H, W = scene
    lists = bc.oracle_lists(xys, depths, radii, H, W)
    return scene, lists


@pytest.mark.parametrize("pruned", [False, True])
def test_mixed_footprints(pruned):
    scene, (ids, bins) = mixed_case()
    xys, depths, radii, conics, opac, H, W = scene
    lens = bins[:, 1] - bins[:, 0]
    assert int((lens > 2048).sum()) > 0 and int((lens <= 2048).sum()) > 0     # tile kernel and queued lists together
    assert sorted(torch.unique(radii).tolist()) == [1, 9, 20, 40]
    ws = run_hip([scene], H, W, ids.numel(), pruned)
    if not pruned:
        assert_exact(ws, 0, ids, bins)
    else:
        live = bc.prune_reference(xys, radii, conics, opac, H, W, (ids, bins))
        kept = check_pruned(ws, 0, xys.shape[0], ids, bins, live, ids.numel())
        assert 0.1 < live.mean() < 0.95 and kept.sum() < kept.size


# ---- (f) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bc.DEPTH_SETS)
@pytest.mark.parametrize("n", [300, 3000, 6000])
def test_depth_edges(n, kind):
    """Tile kernel (300), MID kernel (3000), BIG kernel (6000).  Expected: the oracle's order, i.e. by the depth's bit
    pattern as an unsigned 32-bit number, then by id."""
    scene = bc.depth_case(n, kind)
    xys, depths, radii, H, W = scene
    ids, bins = bc.oracle_lists(xys, depths, radii, H, W)
    assert bins[0].tolist() == [0, n]
    ws = run_hip([scene], H, W, n)
    assert_exact(ws, 0, ids, bins)


# ---- (g) ---------------------------------------------------------------------------------------------------------------
MANY = [(2048, 1536, 12288), (2048, 1552, 12416), (2048, 2048, 16384), (2048, 2064, 16512), (2041, 2070, 16640)]


@pytest.mark.parametrize("pruned", [False, True])
@pytest.mark.parametrize("W,H,T", MANY)
def test_many_tiles(W, H, T, pruned):
    scene = bc.many_tile_scene(H, W)
    xys, depths, radii, conics, opac, H, W = scene
    tx, ty = bc.tiles_of(H, W)
    assert tx * ty == T
    ids, bins = bc.oracle_lists(xys, depths, radii, H, W)
    lens = bins[:, 1] - bins[:, 0]
    assert int(lens[T - 1]) > 0 and int(lens[0]) > 0
    assert T == 12288 or int(lens[12288:T - 1].sum()) > 0          # tiles past the staged scan's size, beside the last
    assert 1 <= int(radii.min()) and int(radii.max()) <= 40
    ws = run_hip([scene], H, W, ids.numel(), pruned)
    if not pruned:
        assert_exact(ws, 0, ids, bins)
    else:
        live = bc.prune_reference(xys, radii, conics, opac, H, W, (ids, bins))
        kept = check_pruned(ws, 0, xys.shape[0], ids, bins, live, ids.numel())
        last = np.repeat(np.arange(T), lens.numpy()) == T - 1
        assert (live & last).any() and (kept & last).any()        # the last tile keeps its visible Gaussian
        assert 0.1 < live.mean() < 0.95 and kept.sum() < kept.size


# ---- (h) ---------------------------------------------------------------------------------------------------------------
def _render(ws, records, N, H, W, bg):
    from goliath_amd import splat

    out = torch.full((1, H, W, 3), float("nan"), device="cuda")
    Ts = torch.full((1, H, W), float("nan"), device="cuda")
    idx = torch.zeros(1, H, W, dtype=torch.int32, device="cuda")
    splat._abi_rasterize_fwd(B=1, N=N, img_h=H, img_w=W, planar=0, tile_bins=ws.tile_bins, sorted_ids=ws.sorted_ids,
                             capacity=ws.capacity, records=records, with_extra=0, background=bg, out_img=out, final_Ts=Ts,
                             final_idx=idx)
    torch.cuda.synchronize()
    return out.cpu(), Ts.cpu()


@pytest.mark.parametrize("seed", [0, 1])
def test_prune_contract(seed):
    """Every tile of prune_scene: the pruned list is an order-preserving subsequence of gsplat's, holds every pair the
    float64 reference can see, and stays inside its reservation.  The forward render over the pruned lists is bit-equal
    to the render over gsplat's lists (same records): pruning never changes an image."""
    from goliath_amd import build, splat

    scene, (ids, bins), live = prune_case(seed)
    xys, depths, radii, conics, opac, H, W = scene
    N, I = xys.shape[0], ids.numel()
    full = run_hip([scene], H, W, I)
    assert_exact(full, 0, ids, bins)
    ws = run_hip([scene], H, W, I, pruned=True)
    kept = check_pruned(ws, 0, N, ids, bins, live, I)
    assert kept.sum() < kept.size
    colors = torch.rand(N, 3, generator=torch.Generator().manual_seed(seed)).cuda()
    bg = torch.tensor([0.3, 0.1, 0.2]).cuda()
    records = splat._pack_records(1, N, xys.cuda(), conics.cuda(), colors, None, opac.cuda())
    img_f, T_f = _render(full, records, N, H, W, bg)
    img_p, T_p = _render(ws, records, N, H, W, bg)
    assert torch.isfinite(img_f).all() and float(T_f.min()) < 0.5
    assert torch.equal(img_p, img_f) and torch.equal(T_p, T_f)
    # information only: how many pairs that no pixel can see the kernel still keeps
    tight = {"what": "share of the (Gaussian, tile) pairs of gsplat's lists that no pixel centre of the tile can see "
                     "(float64 brute force) which gol_bin_sort's pruned mode still keeps; tests/binning_cases.py: prune_scene",
             "seed": seed, "pairs": int(kept.size), "live": int(live.sum()), "kept": int(kept.sum()),
             "kept_not_live": int((kept & ~live).sum()),
             "share_of_dead_pairs_kept": float((kept & ~live).sum() / max(1, (~live).sum())),
             "csrc_sha16": build.source_digest()}
    print("prune tightness:", json.dumps(tight))     # (profiles/binning_prune_tightness.json keeps a copy of these lines)


# ---- (i) ---------------------------------------------------------------------------------------------------------------
def test_capacity_overflow():
    """Scenario (a) with room for half of the intersections: the cut falls inside the 9000-entry list of tile 13."""
    scene, ids, bins = planned("a")
    xys, depths, radii, H, W, plan = scene
    I = ids.numel()
    cap = I // 2
    assert int(bins[13, 0]) + 4096 < cap < int(bins[13, 1])
    ws = run_hip([scene], H, W, cap)
    assert int(ws.n_isect[0]) == I
    hb = ws.tile_bins[0].cpu()
    got = ws.sorted_ids[0].cpu()
    assert int(hb.max()) <= cap and int(hb.min()) >= 0
    for t in range(bins.shape[0]):
        s, e = bins[t].tolist()
        if e <= cap:                                   # fits: exactly the oracle's list
            assert (e == s and hb[t, 1] == hb[t, 0]) or hb[t].tolist() == [s, e], t
            assert torch.equal(got[s:e], ids[s:e]), t
        elif s < cap:                                  # straddles: a sorted part of the oracle's list
            assert hb[t].tolist() == [s, cap]
            part = got[s:cap]
            assert bc.in_list_order(depths, part), t
            assert set(part.tolist()) <= set(ids[s:e].tolist())
        else:                                          # beyond: empty
            assert hb[t, 0] == hb[t, 1], t


# ---- (j) ---------------------------------------------------------------------------------------------------------------
def test_library_statics_in_a_fresh_process():
    """GOL_SORT_BIG_NO_LDS, GOL_BIN_WGS and GOL_BIN_WGS2 are read once per process: tests/_binning_statics_worker.py runs
    scenario (b), the two-tile chunk scene and prune_scene under them and exits on its first failure."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_binning_statics_worker.py")
    r = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GOL_SORT_BIG_NO_LDS="1", GOL_BIN_WGS="1", GOL_BIN_WGS2="1"))
    assert r.returncode == 0 and "BINNING_STATICS_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
