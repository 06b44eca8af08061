"""GPU: the UV topology images of goliath_amd/uvtopo.py (csrc/uvtopo.hip) against the numpy float64 oracle of
tests/uvtopo_cases.py, which tests/test_uvtopo_cpu.py pins to the reference's own geom.py.

Cases (a)-(e): index_image, face_index_image, valid_mask and the impaint source map are IDENTICAL on every texel (the
fixtures' coordinates are dyadic: every fp32 product of the coverage test is exact, on-edge samples are exact zeros).
Case (f), a jittered non-dyadic grid: identical outside the oracle's edge band (at most 2 texels, asserted on the oracle
first); inside it either neighbouring face or -1.  bary_image everywhere: |HIP - fp64| <= 2 x (the reference formula's own
fp32-vs-fp64 error on that case) + 4 eps32, the bound of tests/test_gpu_uvgeom.py, nothing excluded."""
import numpy as np
import pytest
import torch

import uvtopo_cases as U

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _images(name, **kw):
    from goliath_amd import uvtopo

    c = U.CASES[name]
    return uvtopo.index_images(_t(c.vi), _t(c.vt), _t(c.vti), c.S, flip_uv=c.flip_uv, **kw)


def _check_bary(name, got, o):
    got = got.double().cpu().numpy()
    err = np.abs(got - o.bary64).max()
    ref_err = np.abs(o.bary32.astype(np.float64) - o.bary64).max()
    bound = 2.0 * ref_err + 4.0 * EPS
    print(f"[uvtopo] {name}: |hip - fp64| = {err:.3e}, the formula's own fp32 = {ref_err:.3e}, bound = {bound:.3e}, "
          f"ratio = {err / bound:.3f}")
    assert np.isfinite(got).all()
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("name", U.EXACT)
def test_images_identical_to_the_oracle(name):
    from goliath_amd import uvtopo

    c, o = U.CASES[name], U.oracle(name)
    img = _images(name)
    assert img.index_image.dtype == torch.int64 and tuple(img.index_image.shape) == (c.S, c.S, 3)
    assert img.face_index_image.dtype == torch.int64 and tuple(img.face_index_image.shape) == (c.S, c.S)
    assert img.bary_image.dtype == torch.float32 and tuple(img.bary_image.shape) == (c.S, c.S, 3)
    assert img.valid_mask.dtype == torch.bool and tuple(img.valid_mask.shape) == (c.S, c.S, 1)
    assert all(t.is_cuda for t in img)
    assert o.valid.any() and not o.band.any()
    assert np.array_equal(img.face_index_image.cpu().numpy(), o.face)
    assert np.array_equal(img.index_image.cpu().numpy(), o.index_image)
    assert np.array_equal(img.valid_mask[..., 0].cpu().numpy(), o.valid)
    assert (img.bary_image[~img.valid_mask[..., 0]] == 0).all()
    _check_bary(name, img.bary_image, o)
    face = uvtopo.uv_face_index(_t(c.vt), _t(c.vti), c.S, flip_uv=c.flip_uv)
    assert face.dtype == torch.int64 and np.array_equal(face.cpu().numpy(), o.face)


def test_on_edge_samples_zero_area_overlap_and_clipping_are_in_the_fixtures():
    """What (a) and (b) claim to hold, on the oracle and on the HIP images: exact on-edge / on-vertex samples that are
    covered, a zero-area face 0 that covers nothing, the lower index winning an overlap, a face cut by the image border."""
    a, b = U.oracle("a"), U.oracle("b")
    assert (a.bary64[a.valid] == 0).any(-1).sum() >= 20 and ((a.bary64[a.valid] == 1).any(-1)).sum() >= 9
    img = _images("a")
    got = img.bary_image[img.valid_mask[..., 0]]
    assert int((got == 0).any(-1).sum()) == int((a.bary64[a.valid] == 0).any(-1).sum())
    assert not (b.face == 0).any() and (b.face == 1).sum() > 20 and not (b.face == 18).any()
    assert (b.face[-1] == 19).any() and (np.asarray(U.CASES["b"].vt)[:, 1] > 1).any()
    assert (U.CASES["b"].vi != U.CASES["b"].vti).any()


def test_jittered_grid_identical_outside_the_edge_band():
    c, o = U.CASES["f"], U.oracle("f")
    assert int(o.band.sum()) <= 2                                    # on the oracle alone, first
    img = _images("f")
    face = img.face_index_image.cpu().numpy()
    out = ~o.band
    assert np.array_equal(face[out], o.face[out])
    assert np.array_equal(img.index_image.cpu().numpy()[out], o.index_image[out])
    assert np.array_equal(img.valid_mask[..., 0].cpu().numpy()[out], o.valid[out])
    for r, col in zip(*np.nonzero(o.band)):
        # a neighbouring face: one that shares a uv vertex with the oracle's face (or the oracle's face itself), or -1
        near = {-1} | {f for f, tri in enumerate(c.vti) if o.face[r, col] < 0 or set(tri) & set(c.vti[o.face[r, col]])}
        assert face[r, col] in near, (r, col, face[r, col])
    # barycentrics: on the texels where the face agrees (all of them outside the band), nothing else excluded
    same = face == o.face
    got = img.bary_image.double().cpu().numpy()
    err = np.abs(got - o.bary64)[same].max()
    bound = 2.0 * np.abs(o.bary32.astype(np.float64) - o.bary64).max() + 4.0 * EPS
    print(f"[uvtopo] f: |hip - fp64| = {err:.3e}, bound = {bound:.3e}, ratio = {err / bound:.3f}")
    assert same[out].all() and err <= bound


@pytest.mark.parametrize("name,threshold", U.IMPAINT)
def test_impaint_identical_to_the_oracle(name, threshold):
    from goliath_amd import uvtopo

    o, n = U.oracle(name), U.oracle_nearest(name, threshold)
    src = uvtopo.nearest_valid(_t(o.valid), threshold)
    assert src.dtype == torch.int32 and np.array_equal(src.cpu().numpy(), n.src)
    if threshold < 100.0:
        assert ((n.src < 0) & ~o.valid).any() and (n.src >= 0).any()       # some texels stay empty
    else:
        assert (~n.unique & (n.src >= 0)).any()                            # the tie rule is exercised
    img = _images(name, impaint=True, impaint_threshold=threshold)
    assert np.array_equal(img.valid_mask[..., 0].cpu().numpy(), o.valid)   # taken before the impaint
    assert np.array_equal(img.index_image.cpu().numpy(), U.impaint(o.index_image, n.src))
    assert np.array_equal(img.face_index_image.cpu().numpy(), U.impaint(o.face, n.src))
    plain = _images(name)
    assert np.array_equal(img.bary_image.cpu().numpy(), U.impaint(plain.bary_image.cpu().numpy(), n.src))
    # the reference's signature: 3-D with barycentrics, and 2-D alone
    idx2, bary2 = uvtopo.impaint(plain.index_image, plain.bary_image, threshold)
    assert torch.equal(idx2, img.index_image) and torch.equal(bary2, img.bary_image)
    assert torch.equal(uvtopo.impaint(plain.face_index_image, distance_threshold=threshold), img.face_index_image)


def test_strict_threshold_at_d2_6_25():
    """threshold 2.5: d2 = 4 and 5 are taken, d2 = 8 is not (the reference's strict `dists < distance_threshold`); an
    integer threshold excludes its own square."""
    from goliath_amd import uvtopo

    n = U.oracle_nearest("b", 2.5)
    inv = ~U.oracle("b").valid
    assert (n.d2[inv & (n.src >= 0)] <= 5).all() and (n.d2[inv & (n.src >= 0)] == 5).any()
    assert (n.d2[inv & (n.src < 0)] >= 8).all() and (n.d2[inv & (n.src < 0)] == 8).any()
    assert [uvtopo.max_d2_of(t, 24, 24) for t in (2.5, 3.0, 100.0, 0.0, float("inf"))] == [6, 8, 2 * 23 * 23, -1, 2 * 23 * 23]
    n3 = U.oracle_nearest("b", 3.0)
    assert (n3.d2[inv & (n3.src < 0)] == 9).any()
    assert np.array_equal(uvtopo.nearest_valid(_t(U.oracle("b").valid), 3.0).cpu().numpy(), n3.src)


@pytest.mark.parametrize("which", ["empty", "corner", "inner"])
def test_empty_and_single_texel_maps(which):
    from goliath_amd import uvtopo

    valid = U.masks_e()[which]
    for threshold in (100.0, 5.0):
        want = U.nearest_valid(valid, threshold).src
        got = uvtopo.nearest_valid(_t(valid), threshold).cpu().numpy()
        assert np.array_equal(got, want)
        assert (got >= 0).any() == valid.any()
    idx = np.where(valid[..., None], np.array([3, 1, 4]), -1).astype(np.int64)
    out = uvtopo.impaint(_t(idx)).cpu().numpy()
    assert np.array_equal(out, U.impaint(idx, U.nearest_valid(valid, 100.0).src))
    if which == "empty":
        assert (out == -1).all()
        # ... and a mesh without faces: everything empty, the impaint leaves it so
        img = uvtopo.index_images(torch.zeros(0, 3, dtype=torch.int64).cuda(), torch.zeros(4, 2).cuda(),
                                  torch.zeros(0, 3, dtype=torch.int64).cuda(), 20, impaint=True)
        assert (img.index_image == -1).all() and (img.face_index_image == -1).all() and (img.bary_image == 0).all()
        assert not img.valid_mask.any()


def test_uv_topology_feeds_values_to_uv():
    """uvtopo.uv_topology -> uvgeom.values_to_uv against the composition on the oracle's images, in the uvgeom bound."""
    from goliath_amd import uvgeom, uvtopo

    for name, kw in (("b", {}), ("f", {}), ("b", dict(impaint=True, impaint_threshold=3.0))):
        c, o = U.CASES[name], U.oracle(name)
        idx, b64, b32 = o.index_image, o.bary64, o.bary32
        if kw:
            src = U.oracle_nearest(name, 3.0).src
            idx, b64, b32 = U.impaint(idx, src), U.impaint(b64, src), U.impaint(b32, src)
        V = int(np.asarray(c.vi).max()) + 1
        values = np.random.default_rng(1).standard_normal((2, V, 4)).astype(np.float32)
        topo = uvtopo.uv_topology(_t(c.vi), _t(c.vt), _t(c.vti), c.S, flip_uv=c.flip_uv, n_verts=V, **kw)
        assert isinstance(topo, uvgeom.UVTopology) and topo.S == c.S
        got = uvgeom.values_to_uv(_t(values), topo).double().cpu().numpy()
        ok = (idx != -1).all(-1)

        def compose(dt, bary):
            out = np.zeros((2, 4, c.S, c.S), dt)
            for k in range(3):
                out += (values.astype(dt)[:, np.clip(idx[..., k], 0, None)] * (bary[..., k] * ok).astype(dt)[None, ..., None]
                        ).transpose(0, 3, 1, 2)
            return out

        r64, r32 = compose(np.float64, b64), compose(np.float32, b32)
        err, ref_err = np.abs(got - r64).max(), np.abs(r32.astype(np.float64) - r64).max()
        bound = 2.0 * ref_err + 4.0 * EPS * np.abs(values).max()
        print(f"[uvtopo] values_to_uv {name} {kw}: err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        assert np.array_equal(topo.covered_mask().cpu().numpy(), ok)
        assert err <= bound
