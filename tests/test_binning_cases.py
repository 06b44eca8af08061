"""Guards the inputs of tests/test_gpu_binning.py on the CPU: a scenario whose builder drifted must fail here, loudly,
instead of silently no longer reaching the kernel branch it was built for.  Needs only the CPU oracle."""
import numpy as np
import pytest
import torch

import binning_cases as bc

PLANNED = [("a", bc.PLAN_A), ("b", bc.PLAN_B)] + [(f"c{T}", p) for T, p in sorted(bc.PLANS_C.items())]


@pytest.mark.parametrize("name,spec", PLANNED, ids=[n for n, _ in PLANNED])
def test_planned_lists_give_their_planned_lengths(name, spec):
    H, W, plan = spec
    xys, depths, radii, H, W, plan = bc.planned_lists(H, W, plan)
    ids, bins = bc.oracle_lists(xys, depths, radii, H, W)
    T = bins.shape[0]
    assert (bins[:, 1] - bins[:, 0]).tolist() == [plan.get(t, 0) for t in range(T)]
    assert ids.numel() == sum(plan.values()) == xys.shape[0]
    assert sorted(ids.tolist()) == list(range(xys.shape[0]))     # every Gaussian in exactly one list


def test_queue_scenarios_reach_their_classes():
    """(a): MID and BIG lists together, fewer than the per-queue cap; (b): more of either than the cap; (c): a MID and a
    BIG list wherever T allows."""
    def classes(spec):
        H, W, plan = spec
        tx, ty = bc.tiles_of(H, W)
        T = tx * ty
        mid = sum(1 for n in plan.values() if 2048 < n <= 4096)
        big = sum(1 for n in plan.values() if n > 4096)
        return T, (T - 2) // 2 if T > 2 else 0, mid, big

    T, cap, mid, big = classes(bc.PLAN_A)
    assert (T, cap) == (16, 7) and 0 < mid <= cap and 0 < big <= cap
    T, cap, mid, big = classes(bc.PLAN_B)
    assert (T, cap) == (8, 3) and mid == 4 and big == 4
    for T_want, spec in bc.PLANS_C.items():
        T, cap, mid, big = classes(spec)
        assert T == T_want and cap == (0 if T <= 3 else 1)
        assert mid >= 1 and (big >= 1 or T == 1)
        assert mid + big > 2 * cap                    # at least one list finds its queue full


def test_two_tile_chunk_scene():
    xys, depths, radii, H, W, plan = bc.two_tile_chunk_scene()
    ids, bins = bc.oracle_lists(xys, depths, radii, H, W)
    assert (bins[:, 1] - bins[:, 0]).tolist() == [plan[0], plan[1]] == [4096, 9096]
    first = ids[:4096].sort().values
    assert torch.equal(first, torch.arange(4096, dtype=torch.int32))     # tile 0 holds exactly the first chunk's ids


@pytest.mark.parametrize("kind", bc.DEPTH_SETS)
@pytest.mark.parametrize("n", [300, 3000, 6000])
def test_depth_cases_are_single_tile_and_ordered_by_bits(n, kind):
    xys, depths, radii, H, W = bc.depth_case(n, kind)
    ids, bins = bc.oracle_lists(xys, depths, radii, H, W)
    assert (bins[:, 1] - bins[:, 0]).tolist() == [n] + [0] * 15
    assert bc.in_list_order(depths, ids)              # the oracle's order IS (depth bits unsigned, id)
    bits = depths.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    distinct = int(torch.unique(bits).numel())
    if kind == "tie_groups":
        counts = torch.unique(bits, return_counts=True)[1]
        sizes = counts[counts > 1]                      # (random float32 depths may collide in pairs by themselves)
        assert sorted(sizes[sizes > 2].tolist()) == [8, 8, 40, 40] and int((sizes == 2).sum()) >= 2
    elif kind == "all_equal":
        assert distinct == 1
    elif kind == "two_ulp":
        assert sorted(torch.unique(bits).tolist()) == [0x3F800000, 0x3F800001]
    elif kind == "clustered_outliers":
        d = depths.double()
        assert float(((d >= 1) & (d <= 1 + 1e-6)).double().mean()) >= 0.99 - 1e-9
        assert int((depths == 50).sum()) >= 1 and int((depths == 1e4).sum()) >= 1
    elif kind == "subnormal":
        assert int((bits < 0x00800000).sum()) > n // 4 and int((bits >= 0x00800000).sum()) > n // 20
        span = float(depths.max()) - float(depths.min())
        with np.errstate(over="ignore"):               # buckets per unit depth: not a finite float32
            assert 0 < span and float(np.float32(min(n, 1024)) / np.float32(span)) == float("inf")
    elif kind == "specials":
        got = set(bits.tolist())
        assert {0x00000000, 0x80000000, 0xBF800000, 0x7F800000} <= got and int(torch.isnan(depths).sum()) == 1


@pytest.mark.parametrize("seed", [0, 1])
def test_prune_scene_classes_and_live_share(seed):
    scene = bc.prune_scene(seed)
    xys, depths, radii, conics, opac, H, W = scene
    assert (H, W, xys.shape[0]) == (112, 160, 1500)
    lists = bc.oracle_lists(xys, depths, radii, H, W)
    live = bc.prune_reference(xys, radii, conics, opac, H, W, lists)
    share = float(live.mean())
    cls = bc.prune_scene_classes(scene, lists, live)
    print(f"prune_scene({seed}): {live.size} oracle pairs, live share {100 * share:.1f} %, classes {cls}")
    assert 0.25 <= share <= 0.85
    assert cls["op_cut_on_border"] >= 8 and cls["op_next_on_border"] >= 8 and cls["op_one_on_border"] >= 8
    assert cls["op_cut_on_border"] + cls["op_next_on_border"] + cls["op_one_on_border"] >= 32
    assert cls["outside_with_pairs"] >= 10 and cls["outside_beyond_radius"] >= 10
    assert cls["box_over_64"] >= 50 and cls["box_over_64_ellipse_spans_image"] >= 50
    assert cls["not_an_ellipse"] >= 20
    assert cls["row_without_pixel"] >= 20
    # the axis ratios and opacities cover their ranges
    a, b, c = conics.double().unbind(1)
    disc = ((0.5 * (a - c)) ** 2 + b * b).sqrt()
    ok = (a * c - b * b > 0) & (a > 0)
    ratio = (((0.5 * (a + c) + disc) / (0.5 * (a + c) - disc))[ok]).sqrt()
    assert float(ratio.min()) < 1.5 and 25 < float(ratio.max()) <= 30.0 * (1 + 1e-5)
    assert float(opac.min()) < 1 / 255 < 0.9 < float(opac.max()) <= 1.0


def test_prune_reference_on_hand_checked_pairs():
    """The reference itself, on pairs small enough to check by hand."""
    H = W = 32
    xys = torch.tensor([[15.5, 8.5], [15.5, 8.5], [8.0, 8.0], [8.0, 8.0]])
    radii = torch.tensor([6, 6, 3, 3], dtype=torch.int32)          # Gaussians 0, 1: box = tiles 0 and 1
    conics = torch.tensor([[1.0, 0.0, 1.0]]).repeat(4, 1)
    # sigma at the nearest pixel centre of tile 1 (16.5, 8.5) is 0.5: alpha = op exp(-0.5)
    op_dead, op_live = (0.99 / 255) * float(np.exp(0.5)), (1.01 / 255) * float(np.exp(0.5))
    opac = torch.tensor([op_dead, op_live, 0.9 / 255, 1.0])
    ids, bins = bc.oracle_lists(xys, torch.ones(4), radii, H, W)
    assert ids.tolist() == [0, 1, 2, 3, 0, 1] and bins.tolist() == [[0, 4], [4, 6], [0, 0], [0, 0]]
    live = bc.prune_reference(xys, radii, conics, opac, H, W)
    assert live.tolist() == [True, True, False, True, False, True]
