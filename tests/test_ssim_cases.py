"""Guards the inputs of the case-driven tests of tests/test_gpu_ssim.py on the CPU: the shapes must reach the strip walk,
the uneven strips and the padded XCD bands of csrc/ssim.hip, the partition replica must agree with the library's grid, and
the reference pair (oracle in float32 against the same oracle in float64) the GPU bars are built from must be usable."""
import math

import pytest
import torch

import ssim_cases as sc


def _parts():
    return {c[0]: sc.partition(c[3], c[4]) for c in sc.CASES}


def test_partition_replica_on_hand_checked_shapes():
    want = {
        (1, 1): ([1], 1, 7, 8), (5, 7): ([1], 1, 7, 8), (11, 10): ([1], 1, 7, 8), (32, 32): ([1], 1, 7, 8),
        (33, 225): ([2, 2, 2, 2, 0, 0], 1, 6, 48), (40, 200): ([2, 2, 2, 1, 0, 0], 1, 6, 48),
        (260, 390): ([3, 3, 3, 3, 1, 0], 2, 7, 96), (290, 65): ([1, 1, 1], 2, 6, 48),
        (2048, 1334): ([7] * 6, 8, 0, 384),            # the bench's size: divides evenly (what the older tests cover)
    }
    for (H, W), (lens, rows, pad, grid) in want.items():
        p = sc.partition(H, W)
        assert (p["strip_lens"], p["rows_per_xcd"], p["padding_slots"], p["grid"]) == (lens, rows, pad, grid), (H, W, p)
    assert {(c[3], c[4]) for c in sc.CASES} == set(want) - {(2048, 1334)}
    p = sc.partition(260, 390)
    assert (p["tiles_y"], p["tiles_x"]) == (9, 13) and 260 - 8 * 32 == 4 and 390 - 12 * 32 == 6
    assert 33 - 32 == 1 and 225 - 7 * 32 == 1          # the 1-row and the 1-column last tiles


def test_cases_reach_the_branches_the_gpu_tests_rely_on():
    parts = _parts()
    lens = [p["strip_lens"] for p in parts.values()]
    assert any(max(l) >= 3 for l in lens)                                        # two prefetches in flight in a row
    assert any(0 in l for l in lens)                                             # empty strip
    assert any(0 < l[k] < l[0] for l in lens for k in range(1, len(l)))          # short last strip
    assert any(p["rows_per_xcd"] >= 2 and p["padding_slots"] > 0 for p in parts.values())
    assert {c[5] for c in sc.CASES} == set(sc.MASK_KINDS)
    assert any(c[5] == "bc" and c[1] == 2 and c[2] == 3 for c in sc.CASES)       # mask_c = C with B = 2: bc != bc % C
    assert any(c[5] == "bc" and c[1] == 2 and (c[3], c[4]) == (40, 200) for c in sc.CASES)
    multi = {c[6] for c in sc.CASES if max(parts[c[0]]["strip_lens"]) >= 2}
    assert multi == set(sc.INPUT_KINDS)                                          # both input kinds walk a strip
    assert all(c[1] * c[2] <= 6 for c in sc.CASES)
    assert {c[7] for c in sc.CASES} == {1.0, -1.0, 0.37}
    assert len(set(sc.TAGS)) == len(sc.TAGS)


def test_generators_are_seeded_and_of_their_kind():
    for tag, B, C, H, W, mk, ik, g in sc.CASES:
        pred, target, mask, g_ = sc.make(tag)
        sc.make.cache_clear()
        again = sc.make(tag)
        assert torch.equal(pred, again[0]) and torch.equal(target, again[1]) and g_ == g
        assert pred.shape == target.shape == (B, C, H, W) and pred.dtype == torch.float32
        if mk == "none":
            assert mask is None
            continue
        assert torch.equal(mask, again[2])
        assert mask.shape == (B, C if mk == "bc" else 1, H, W)
        if mk == "zero":
            assert not mask.any()
        elif mk == "frac1":
            assert float(mask.min()) == 0.0 and 0.0 < float(mask.max()) < 1.0
            assert int(((mask > 0) & (mask < 1)).sum()) >= mask.numel() // 2     # genuinely fractional weights
        else:
            assert set(mask.unique().tolist()) <= {0.0, 1.0} and (mask.numel() < 64 or 0.5 < float(mask.mean()) < 0.9)
        if ik == "flat":
            lo, hi = torch.tensor([0.1, 0.9]).tolist()                           # the float32 values
            assert 0.001 < float((target == lo).float().mean()) < 0.05 and set(target.unique().tolist()) == {lo, hi}
            assert float((pred - target).abs().max()) < 0.06


def test_grid_size_equals_the_librarys():
    from goliath_amd import _lib

    lib = _lib.load()
    for H, W in sorted({(c[3], c[4]) for c in sc.CASES} | {(2048, 1334), (257, 193), (256, 192)}):
        assert sc.partition(H, W)["grid"] == lib.gol_ssim_blocks(H, W), (H, W)


@pytest.mark.parametrize("tag", sc.TAGS)
def test_reference_pair_is_usable(tag):
    """The GPU bar is 4x the float32 oracle's own distance from the float64 oracle: both must be finite; for the all-zero
    mask both must be exactly 0 (value and gradient)."""
    v32, G32 = sc.oracle(tag, torch.float32)
    v64, G64 = sc.oracle(tag, torch.float64)
    assert math.isfinite(v32) and math.isfinite(v64) and bool(torch.isfinite(G32).all()) and bool(torch.isfinite(G64).all())
    if sc.BY_TAG[tag][5] == "zero":
        assert v32 == 0.0 and v64 == 0.0 and not G32.any() and not G64.any()
        return
    e_ref, e_val = sc.max_err(G32, G64), abs(v32 - v64)
    print(f"{tag}: v64 {v64:+.9f}  |v32 - v64| {e_val:.2e}  e_ref {e_ref:.2e}  max|G64| {float(G64.abs().max()):.2e}")
    assert math.isfinite(e_ref) and math.isfinite(e_val) and float(G64.abs().max()) > 0
    if tag == "260x390":                               # the maps of the forward-localisation test
        m32, m64 = sc.oracle_map(tag, torch.float32), sc.oracle_map(tag, torch.float64)
        assert bool(torch.isfinite(m32).all()) and bool(torch.isfinite(m64).all())
        assert abs(float(m64.mean()) - v64) < 1e-12    # no mask, g = 1: the value is the map's mean
