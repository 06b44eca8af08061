"""GPU: gol_wave_colsum (gol_common.h), the column-first reduction of the two-pixel raster backward, through its self-test entry.

Six rows of 64 lane values (s0, s1, s2, m0, my, myy) and a factor dx per lane go in -- dx a function of the column l & 15, the
primitive's precondition -- and the kernel returns what every lane holds afterwards.  Nine lanes hold sums, and the map is
part of the contract (the raster backward derives its LDS slot from the lane):
    lane   7   39   23   55   15         31     47         63        19
    sum    s0  s1   s2   myy  M0 = m0    dx m0  My = my    dx my     dx^2 m0
Reference: float64 sums of the six rows and of dx m0, dx^2 m0 and dx my, lane by lane.  The bar on random input is the one
tests/test_gpu_wave_sum8.py holds gol_wave_sum8 to (|error| < 1e-4 against float64 for 64 standard-normal values; dx is drawn
from [-1, 1) here, so the weighted sums are no larger than the plain ones).  Sums of +-1 with small-integer dx and of a
single non-zero lane are exact in float32 in any order and must come out exact.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
#               s0  s1  s2  myy  M0  Mx  My  Mxy  Mxx
RESULT_LANE = [7, 39, 23, 55, 15, 31, 47, 63, 19]


def _colsum(x, dx):
    from goliath_amd import _lib

    assert x.shape == (6, 64) and x.dtype == torch.float32 and dx.shape == (64,) and dx.dtype == torch.float32
    assert torch.equal(dx[:16].repeat(4), dx), "precondition: dx equal in lanes l and l + 16"
    x, dx = x.contiguous().cuda(), dx.contiguous().cuda()
    out = torch.full((64,), float("nan"), device="cuda")
    _lib.call("gol_selftest_wave_colsum", _lib.fptr(x), _lib.fptr(dx), _lib.fptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu()[RESULT_LANE]


def _want(x, dx):
    """The nine sums in float64, in the order of RESULT_LANE."""
    x, dx = x.double(), dx.double()
    s0, s1, s2, m0, my, myy = x
    return torch.stack([s0.sum(), s1.sum(), s2.sum(), myy.sum(), m0.sum(), (dx * m0).sum(), my.sum(), (dx * my).sum(),
                        (dx * dx * m0).sum()])


def _columns(dx16):
    return torch.as_tensor(dx16, dtype=torch.float32).repeat(4)


def test_result_lane_map():
    """Row k = k + 1 in every lane, dx = 2: the plain sums are 64 (k + 1), the moments 2, 4 and 2 times theirs, exactly."""
    x = (torch.arange(6, dtype=torch.float32) + 1.0)[:, None].expand(6, 64)
    got = _colsum(x, torch.full((64,), 2.0))
    assert got.tolist() == [64.0, 128.0, 192.0, 384.0, 256.0, 512.0, 320.0, 640.0, 1024.0], got.tolist()


def test_random_against_float64():
    """Measured (MI355X): max |error| 9.6e-7 over 8 draws."""
    g = torch.Generator().manual_seed(19)
    worst = 0.0
    for _ in range(8):
        x = torch.randn(6, 64, generator=g)
        dx = _columns(2.0 * torch.rand(16, generator=g) - 1.0)
        err = (_colsum(x, dx).double() - _want(x, dx)).abs().max().item()
        worst = max(worst, err)
    print("max |error| %.1e" % worst)
    assert worst < 1e-4


def test_sign_patterns_are_exact():
    """+-1 per lane (all +1, alternating by lane, pair, half row, row of 16, half wave, random signs per input) with dx = the
    column's offset from the middle, -8 .. 7 as in a tile, and with dx alternating +-3: every partial sum is a small integer."""
    lane = torch.arange(64)
    g = torch.Generator().manual_seed(20)
    pats = [torch.ones(6, 64)]
    pats += [(1.0 - 2.0 * ((lane // p) % 2).float())[None].expand(6, 64) for p in (1, 2, 8, 16, 32)]
    pats += [1.0 - 2.0 * torch.randint(0, 2, (6, 64), generator=g).float() for _ in range(3)]
    for dx in (_columns(torch.arange(16) - 8.0), _columns(3.0 - 6.0 * (torch.arange(16) % 2))):
        for x in pats:
            got, want = _colsum(x, dx), _want(x, dx)
            assert torch.equal(got.double(), want), (got, want)


def test_one_hot_lanes_are_exact():
    """Lane l alone holds row k = k + 1 + l / 64, dx = 1 + (l & 15) % 5 in its column (1 .. 5: products of a 9-bit value
    with at most 25 are exact): every lane is hit once, reaches every sum it belongs to, and leaks into no other."""
    dx = _columns(1.0 + (torch.arange(16) % 5))
    hit = set()
    for l in range(64):
        x = torch.zeros(6, 64)
        x[:, l] = torch.arange(6, dtype=torch.float32) + 1.0 + l / 64.0
        got, want = _colsum(x, dx), _want(x, dx)
        s0, s1, s2, m0, my, myy = x[:, l].tolist()
        d = float(dx[l])
        assert want.tolist() == [s0, s1, s2, myy, m0, d * m0, my, d * my, d * d * m0]
        assert torch.equal(got.double(), want), (l, got, want)
        hit.add(l)
    assert hit == set(range(64))
