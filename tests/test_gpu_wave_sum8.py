"""GPU: gol_wave_sum8 (gol_common.h), the 8-way wave64 reduction of the raster backward, through its self-test entry.

Eight rows of 64 lane values go in, the kernel returns what every lane holds afterwards.  The result-lane map is part of the
contract (the raster backward derives its LDS slot from the lane): lane 16 r + 7 = sum(a_r), lane 16 r + 15 = sum(a_{4+r}).
The bar is the one tests/test_gpu_primitives.py sets for gol_wave_sum4 (|error| < 1e-4 against the float64 sum of 64
standard-normal values); sums of +-1 and of a single non-zero lane are exact in float32 in any order and must come out exact.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
RESULT_LANE = [7, 23, 39, 55, 15, 31, 47, 63]     # of a0 .. a7


def _sum8(x):
    from goliath_amd import _lib

    assert x.shape == (8, 64) and x.dtype == torch.float32
    x = x.contiguous().cuda()
    out = torch.full((64,), float("nan"), device="cuda")
    _lib.call("gol_selftest_wave_sum8", _lib.fptr(x), _lib.fptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu()


def test_result_lane_map():
    """a_k = k + 1 in every lane: the sum 64 (k + 1) of a_k must sit in RESULT_LANE[k], exactly."""
    x = (torch.arange(8, dtype=torch.float32) + 1.0)[:, None].expand(8, 64)
    out = _sum8(x)
    assert out[RESULT_LANE].tolist() == [64.0 * (k + 1) for k in range(8)], out.tolist()


def test_random_against_float64():
    """Measured (MI355X): max |error| 1.3e-6 over 8 draws."""
    g = torch.Generator().manual_seed(8)
    worst = 0.0
    for _ in range(8):
        x = torch.randn(8, 64, generator=g)
        err = (_sum8(x)[RESULT_LANE].double() - x.double().sum(1)).abs().max().item()
        worst = max(worst, err)
    print("max |error| %.1e" % worst)
    assert worst < 1e-4


def test_sign_patterns_are_exact():
    """+-1 per lane: all +1, alternating by lane, by pair, by row of 16, by half, and random signs that differ per input."""
    lane = torch.arange(64)
    g = torch.Generator().manual_seed(9)
    pats = [torch.ones(8, 64)]
    pats += [(1.0 - 2.0 * ((lane // p) % 2).float())[None].expand(8, 64) for p in (1, 2, 8, 16, 32)]
    pats += [1.0 - 2.0 * torch.randint(0, 2, (8, 64), generator=g).float() for _ in range(3)]
    for x in pats:
        got = _sum8(x)[RESULT_LANE]
        assert torch.equal(got, x.sum(1)), (got, x.sum(1))
        assert torch.allclose(got.double(), x.double().sum(1), atol=1e-4)


def test_one_hot_lanes_are_exact():
    """Lane l alone holds a_k = k + 1 + l / 64: every lane reaches every sum once, and no input leaks into another's."""
    for l in range(64):
        x = torch.zeros(8, 64)
        x[:, l] = torch.arange(8, dtype=torch.float32) + 1.0 + l / 64.0
        got = _sum8(x)[RESULT_LANE]
        assert torch.equal(got, x[:, l]), (l, got)
        assert torch.allclose(got.double(), x.double().sum(1), atol=1e-4)
