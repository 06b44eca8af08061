"""GPU: gol_depth_disc_mask and gol_mask_erode (csrc/imgfam.hip, goliath_amd.imageops) against the reference's own outputs
in tests/golden/imgfam_golden.npz (tests/golden/make_imgfam_golden.py; the scenes are described in tests/imgfam_cases.py).

The kernels work on output tiles of 64 x 16 pixels (imgfam_cases.TILE_W x TILE_H): the sizes are the issue's six plus one
tile, one tile + 1 and two tiles + 1 in each axis.  Exact cases: integer depths in [0, 512], so every Sobel sum and
gx^2 + gy^2 is exact in float32 and the output must equal the reference's in every pixel.  Float case: a paraboloid blob;
pixels whose float64 Sobel norm is within tau of the threshold are flagged and the rest must equal the reference's."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import imgfam_cases as cases  # noqa: E402
import npz_parts  # noqa: E402

POISON = 0xAB


@pytest.fixture(scope="module")
def golden():
    return npz_parts.load(os.path.join(HERE, "golden", "imgfam_golden.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw_disc(depth, pool, threshold):
    """The entry itself on depth [S,H,W], into an output pre-filled with a poison byte."""
    from goliath_amd import _lib
    from goliath_amd._lib import c_float, c_int, fptr, ptr, stream_ptr

    S, H, W = depth.shape
    out = torch.full((S, H, W), POISON, device="cuda", dtype=torch.uint8)
    _lib.call("gol_depth_disc_mask", c_int(S), c_int(H), c_int(W), c_int(pool), c_float(threshold), fptr(depth),
              ptr(out, torch.uint8), stream_ptr())
    return out


def _raw_erode(x, ks):
    from goliath_amd import _lib
    from goliath_amd._lib import c_int, fptr, ptr, stream_ptr

    S, H, W = x.shape
    is_u8 = x.dtype == torch.bool
    out = torch.full((S, H, W), POISON, device="cuda", dtype=torch.uint8).repeat_interleave(4, -1).view(torch.float32)
    assert out.shape == x.shape and out.is_contiguous()
    _lib.call("gol_mask_erode", c_int(S), c_int(H), c_int(W), c_int(ks), c_int(int(is_u8)),
              ptr(x.view(torch.uint8) if is_u8 else x), fptr(out), stream_ptr())
    return out


def _batches(S):
    """B = 1, B = 3 (twice, so that every one of the six common scenes is seen) and the whole stack."""
    return [slice(0, 1), slice(0, 3), slice(3, 6), slice(0, S)]


@pytest.mark.parametrize("pool", cases.POOLS)
@pytest.mark.parametrize("H,W", cases.SIZES)
def test_depth_disc_mask_equals_the_reference_on_exact_scenes(golden, H, W, pool):
    tag = cases.size_tag(H, W)
    depth = _dev(golden[f"disc/{tag}/depth"])
    for ti, thr in enumerate(cases.THRESHOLDS):
        ref = _dev(golden[f"disc/{tag}/p{pool}t{ti}"])
        for sl in _batches(depth.shape[0]):
            got = _raw_disc(depth[sl].contiguous(), pool, thr)
            assert got.max() <= 1, "a pixel was not written"
            assert torch.equal(got.bool(), ref[sl]), (tag, pool, ti, sl, int((got.bool() != ref[sl]).sum()))


@pytest.mark.parametrize("pool", cases.POOLS)
def test_depth_disc_mask_float_scene(golden, pool):
    from goliath_amd import imageops

    depth = golden["disc/float/depth"]
    ref = golden[f"disc/float/p{pool}"]
    yes, no = cases.decide(depth, pool)
    flagged = ~(yes | no)
    assert flagged.mean() <= cases.FLAGGED_CAP and yes.any() and no.any()
    got = _raw_disc(_dev(depth), pool, 40.0)
    assert got.max() <= 1
    got = got.bool().cpu().numpy()
    assert got[yes].all() and not got[no].any()
    assert np.array_equal(got[yes | no], ref[yes | no])
    pub = imageops.depth_discontinuity_mask(_dev(depth)[:, None], pool_ksize=pool)
    assert pub.dtype == torch.bool and pub.shape == (1, 1) + depth.shape[1:] and np.array_equal(pub[:, 0].cpu().numpy(), got)


def test_depth_discontinuity_mask_public_defaults(golden):
    """threshold 40, pool 3, kscale ignored; [B,1,H,W] in, torch.bool [B,1,H,W] out."""
    from goliath_amd import imageops

    tag = cases.size_tag(33, 35)
    depth = _dev(golden[f"disc/{tag}/depth"])[:, None]
    ref = _dev(golden[f"disc/{tag}/p3t1"])[:, None]
    assert cases.THRESHOLDS[1] == 40.0
    a = imageops.depth_discontinuity_mask(depth)
    b = imageops.depth_discontinuity_mask(depth, 40.0, 123.0, 3)
    assert a.dtype == torch.bool and torch.equal(a, ref) and torch.equal(b, ref)
    with pytest.raises(ValueError):
        imageops.depth_discontinuity_mask(depth[:, 0])


@pytest.mark.parametrize("ks", cases.ERODE_KS)
@pytest.mark.parametrize("H,W", cases.SIZES)
def test_erode_equals_the_reference(golden, H, W, ks):
    from goliath_amd import imageops

    tag = cases.size_tag(H, W)
    x = _dev(golden[f"erode/{tag}/x"])
    ref_f, ref_b = _dev(golden[f"erode/{tag}/f{ks}"]), _dev(golden[f"erode/{tag}/b{ks}"])
    assert ref_f.dtype == torch.float32 and ref_b.dtype == torch.bool
    xb = x == 1.0
    S = x.shape[0]
    for sl in (slice(0, 1), slice(0, 3), slice(2, 5), slice(0, S)):
        got_f, got_b = _raw_erode(x[sl].contiguous(), ks), _raw_erode(xb[sl].contiguous(), ks)
        for got, ref in ((got_f, ref_f[sl]), (got_b, ref_b[sl].float())):
            assert ((got == 0) | (got == 1)).all(), "a pixel was not written"
            assert torch.equal(got, ref), (tag, ks, sl, int((got != ref).sum()))
    # the public operator: the input's dtype, 3-D -> 4-D
    pf, pb = imageops.erode(x, ks), imageops.erode(xb[:, None], ks)
    assert pf.dtype == torch.float32 and pf.shape == (S, 1, H, W) and torch.equal(pf[:, 0], ref_f)
    assert pb.dtype == torch.bool and pb.shape == (S, 1, H, W) and torch.equal(pb[:, 0], ref_b)
    # an all-ones image stays all ones up to the border (scene 2)
    assert bool(ref_f[2].all()) and bool(_raw_erode(x[2:3].contiguous(), ks).eq(1).all())


def test_unsupported_windows_raise():
    from goliath_amd import _lib, imageops

    depth = torch.zeros(1, 1, 8, 8, device="cuda")
    with pytest.raises(_lib.GoliathHipError, match="pool size 7"):
        imageops.depth_discontinuity_mask(depth, pool_ksize=7)
    for ks in (33, 4, 0, -3):
        with pytest.raises(_lib.GoliathHipError, match=f"window size {ks}"):
            imageops.erode(depth, ks)
    torch.cuda.synchronize()
