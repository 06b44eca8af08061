"""GPU: the camera-to-UV view textures of goliath_amd/viewtex.py (csrc/viewtex.hip) against the numpy float64 oracle of
tests/viewtex_cases.py, which tests/test_viewtex_cpu.py pins to the reference's own geom.py, and against the reference's
recorded fp32 outputs (tests/golden/viewtex_golden.npz).

Visibility and masks are IDENTICAL everywhere.  Textures are identical to the oracle outside its band (texels whose
sample coordinate lies within 1e-3 px of a rounding boundary of the nearest fetch in some view: at most 1 % of a case,
asserted on the oracle first); inside the band a texel equals the oracle under one of the four rounding choices.  Nothing
else is excluded.  The accumulate mode is bitwise the sequential fp32 sum of the materialised textures in view order."""
import os
import types

import numpy as np
import pytest
import torch

import viewtex_cases as C

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = float(np.finfo(np.float32).eps)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "viewtex_golden.npz")) as z:
        return {k: z[k] for k in z.files}


def _args(c, views=None, index_dtype=np.int64):
    """The reference's argument list of compute_view_texture for case c (optionally a selection of its views)."""
    sel = slice(None) if views is None else list(views)
    verts = c.verts if c.verts.shape[0] == 1 else c.verts[sel]
    return [_t(verts), _t(c.faces), _t(c.image[sel]), _t(c.index_img[sel].astype(index_dtype)), None, _t(c.K[sel]),
            _t(c.Rt[sel]), _t(c.index_image_uv), _t(c.bary_image_uv), _t(c.face_index_uv)]


def _topology(c):
    from goliath_amd import viewtex

    return viewtex.ViewTexTopology(_t(c.index_image_uv), _t(c.bary_image_uv), _t(c.face_index_uv))


def _sub_oracle(c, views, threshold=None):
    v = list(views)
    verts = c.verts if c.verts.shape[0] == 1 else c.verts[v]
    return C.compute(verts, c.image[v], c.index_img[v], c.K[v], c.Rt[v], c.index_image_uv, c.bary_image_uv,
                     c.face_index_uv, c.F, threshold)


# ---- visibility -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("name", C.NAMES)
def test_visibility_identical_to_the_oracle(name, index_dtype):
    from goliath_amd import viewtex

    c, o = C.case(name), C.oracle(name)
    C.check_fixture(name)
    img = _t(c.index_img.astype(index_dtype))
    fv = viewtex.face_visibility(img, c.F)
    assert fv.dtype == torch.bool and tuple(fv.shape) == (C.B, c.F) and np.array_equal(_np(fv), o.face_vis)
    assert not _np(fv)[1].any() and _np(fv)[0, 0] and _np(fv)[0, c.F - 1]           # the empty view; faces 0 and F - 1
    uv = viewtex.uv_visibility(img, c.F, _t(c.face_index_uv))
    assert uv.dtype == torch.bool and tuple(uv.shape) == (C.B, c.S, c.S) and np.array_equal(_np(uv), o.mask[:, 0])
    # indices outside [-1, F) planted in pixels that held -1 or a face seen elsewhere too: ignored
    planted = c.index_img.copy()
    holes = np.argwhere(planted[0] == -1)
    planted[0, holes[0][0], holes[0][1]] = c.F
    planted[0, holes[1][0], holes[1][1]] = c.F + 1000
    planted[1, 3, 5] = -7
    planted[1, 0, 0] = 2 ** 31 - 1
    assert np.array_equal(_np(viewtex.face_visibility(_t(planted.astype(index_dtype)), c.F)), o.face_vis)
    # a second call into a dirty buffer: the entry zeroes it
    dirty = torch.full((C.B, c.F), 0xFF, dtype=torch.uint8, device="cuda")
    viewtex._abi_face_visibility(B=C.B, F=c.F, H=C.H, W=C.W, index_img=img.to(torch.int32).contiguous(), face_vis=dirty)
    assert np.array_equal(_np(dirty), o.face_vis.astype(np.uint8))


# ---- compute_view_texture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("threshold", [None, C.THRESHOLD])
@pytest.mark.parametrize("name", C.NAMES)
def test_view_texture_against_the_oracle_and_the_golden(golden, name, threshold, index_dtype):
    from goliath_amd import viewtex

    c, o = C.case(name), C.oracle(name, threshold)
    assert o.band.mean() <= 0.01 and C.H != C.W                                     # on the oracle alone, first
    tex, mask = viewtex.compute_view_texture(*_args(c, index_dtype=index_dtype), intensity_threshold=threshold,
                                             normal_threshold=0.1)
    assert tex.dtype == torch.float32 and tuple(tex.shape) == (C.B, 3, c.S, c.S)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (C.B, 1, c.S, c.S)
    tex, mask = _np(tex), _np(mask)
    assert np.array_equal(mask, o.mask)                                             # identical everywhere
    out = ~o.band
    differ = int((tex != o.tex).any(1).any(0)[o.band].sum())
    print(f"[viewtex] {name} thr={threshold}: band {int(o.band.sum())} texels ({100 * o.band.mean():.2f} %), "
          f"hip differs from the float64 oracle on {differ} of them")
    assert np.isfinite(tex).all()
    assert np.array_equal(tex[..., out], o.tex[..., out])                           # identical outside the band
    assert C.in_alts(tex, o, o.band).all()                                          # inside: a rounding candidate
    gold = golden[f"{name}/tex_thr" if threshold else f"{name}/tex"]
    assert np.array_equal(tex[..., out], gold[..., out]) and np.array_equal(mask, golden[f"{name}/mask"])
    if threshold is None:                                                           # 0 is "no filter" as well
        tex0, _ = viewtex.compute_view_texture(*_args(c, index_dtype=index_dtype), intensity_threshold=0)
        assert np.array_equal(_np(tex0), tex)


# ---- accumulate mode --------------------------------------------------------------------------------------------------------
def test_accumulate_is_the_sequential_sum_in_view_order():
    from goliath_amd import viewtex

    c = C.case("f")
    rng = np.random.default_rng(5)
    start_total = (rng.random((3, c.S, c.S)) * 300).astype(np.float32)
    start_count = rng.integers(0, 9, (c.S, c.S)).astype(np.float32)
    tm = viewtex.TexMean(_topology(c), c.F, "cuda")
    assert tuple(tm.total.shape) == (3, c.S, c.S) and tuple(tm.count.shape) == (c.S, c.S) and not tm.total.any()
    tm.total.copy_(_t(start_total))
    tm.count.copy_(_t(start_count))
    batches = [((0, 1, 2), None), ((2, 0), C.THRESHOLD)]
    texs, masks, otexs, band = [], [], [], np.zeros((c.S, c.S), bool)
    for views, thr in batches:
        a = _args(c, views, np.int32)
        tm.add(a[0], a[2], a[5], a[6], index_img=a[3], intensity_threshold=thr)
        tex, mask = viewtex.compute_view_texture(*a, intensity_threshold=thr)
        o = _sub_oracle(c, views, thr)
        band |= o.band
        for b in range(len(views)):
            texs.append(_np(tex)[b])
            masks.append(_np(mask)[b, 0])
            otexs.append(o.tex[b])
    total, count = _np(tm.total), _np(tm.count)
    assert np.array_equal(total.view(np.uint32), C.sequential_sum(start_total, texs).view(np.uint32))     # bitwise
    assert np.array_equal(count, start_count + np.sum(masks, 0).astype(np.float32))                       # exact
    clear = ~band
    assert clear.mean() > 0.98 and np.array_equal(total[:, clear], C.sequential_sum(start_total, otexs)[:, clear])
    tm.reset()
    assert not tm.total.any() and not tm.count.any()


@pytest.mark.parametrize("name", ["f", "b"])
def test_both_modes_in_one_call_agree_with_the_separate_calls(name):
    from goliath_amd import viewtex

    c = C.case(name)
    topo = _topology(c)
    a = _args(c, index_dtype=np.int32)
    verts, image, K, Rt = viewtex._views("test", a[0], a[2], a[5], a[6])
    tex, mask = viewtex.view_texture(topo, c.F, verts, image, K, Rt, a[3], C.THRESHOLD)
    tm = viewtex.TexMean(topo, c.F, "cuda")
    tm.total.fill_(1.5)
    tm.count.fill_(2.0)
    tm.add(verts, image, K, Rt, index_img=a[3], intensity_threshold=C.THRESHOLD)
    tex2, mask2 = torch.full_like(tex, 7.0), torch.ones_like(mask)
    total2, cnt2 = torch.full_like(tm.total, 1.5), torch.full_like(tm.count, 2.0)
    face_vis = viewtex._face_vis(a[3], c.F)
    viewtex._launch(topo, c.F, verts, image, K, Rt, face_vis, C.THRESHOLD, tex=tex2, mask=mask2, total=total2, cnt=cnt2)
    for x, y in ((tex, tex2), (tm.total, total2), (tm.count, cnt2)):
        assert np.array_equal(_np(x).view(np.uint32), _np(y).view(np.uint32))
    assert torch.equal(mask, mask2) and tm.total.max() > 1.5


def test_broadcast_verts_equal_the_expanded_copy():
    from goliath_amd import viewtex

    c = C.case("f_bcast")
    assert c.verts.shape[0] == 1
    a = _args(c)
    tex, mask = viewtex.compute_view_texture(*a)
    a[0] = a[0].expand(C.B, -1, -1).contiguous()
    tex_e, mask_e = viewtex.compute_view_texture(*a)
    assert np.array_equal(_np(tex).view(np.uint32), _np(tex_e).view(np.uint32)) and torch.equal(mask, mask_e)
    topo = _topology(c)
    one, full = viewtex.TexMean(topo, c.F), viewtex.TexMean(topo, c.F)
    one.add(_t(c.verts), a[2], a[5], a[6], index_img=a[3])
    full.add(a[0], a[2], a[5], a[6], index_img=a[3])
    assert np.array_equal(_np(one.total).view(np.uint32), _np(full.total).view(np.uint32))
    assert torch.equal(one.count, full.count) and one.total.any()


# ---- mean -------------------------------------------------------------------------------------------------------------------
def test_mean_and_its_permutations():
    from goliath_amd import viewtex

    c = C.case("f")
    tm = viewtex.TexMean(_topology(c), c.F)
    a = _args(c)
    for _ in range(3):
        tm.add(a[0], a[2], a[5], a[6], index_img=a[3])
    total, cnt = _np(tm.total).astype(np.float64), _np(tm.count).astype(np.float64)
    assert cnt.max() == 6 and (cnt == 0).any()
    want = (total / (cnt + 1e-5)).transpose(1, 2, 0)
    mean = tm.mean()
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (c.S, c.S, 3)
    got = _np(mean).astype(np.float64)
    ratio = (np.abs(got - want) / np.maximum(4.0 * EPS * np.abs(want), 1e-300)).max()
    print(f"[viewtex] mean: max |mean - total / (cnt + 1e-5)| / (4 eps32 |value|) = {ratio:.3f}")
    assert (np.abs(got - want) <= 4.0 * EPS * np.abs(want)).all()
    plain = _np(mean)
    assert np.array_equal(_np(tm.mean(flip_rows=True)), plain[::-1])
    assert np.array_equal(_np(tm.mean(bgr=True)), plain[..., ::-1])
    assert np.array_equal(_np(tm.mean(flip_rows=True, bgr=True)), plain[::-1, :, ::-1])
    other = _np(tm.mean(eps=0.5)).astype(np.float64)
    assert np.abs(other - (total / (cnt + 0.5)).transpose(1, 2, 0)).max() <= 4.0 * EPS * np.abs(total).max()


# ---- stated behaviour -------------------------------------------------------------------------------------------------------
def test_nan_under_invisible_texels_leaves_the_texture_finite():
    from goliath_amd import viewtex

    c, o = C.case("f"), C.oracle("f")
    a = _args(c)
    tex, _ = viewtex.compute_view_texture(*a)
    # view 1 shows nothing at all; in view 2, the pixels no visible texel samples (under any rounding choice)
    image = c.image.copy()
    image[1] = np.nan
    sampled = np.zeros((C.H, C.W), bool)
    show = o.mask[2, 0] & (c.index_image_uv[..., 0] != -1)
    s = np.clip(o.pix[2][show] - 0.5, 0, [C.W - 1, C.H - 1])
    for fx in (np.floor, np.ceil):
        for fy in (np.floor, np.ceil):
            sampled[fy(s[:, 1]).astype(int), fx(s[:, 0]).astype(int)] = True
    assert (~sampled).sum() >= 10
    image[2][:, ~sampled] = np.nan
    a[2] = _t(image)
    tex_nan, _ = viewtex.compute_view_texture(*a)
    assert torch.isfinite(tex_nan).all() and torch.equal(tex_nan, tex)


def test_pz_zero_gives_zero_and_leaves_the_other_texels_alone():
    from goliath_amd import viewtex

    # 2x2 texels, each sitting exactly on a vertex (barycentrics 1, 0, 0); identity camera: p = the vertex itself
    idx = np.array([[[0, 1, 2], [0, 1, 2]], [[1, 2, 0], [2, 0, 1]]], np.int64)
    bary = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (2, 2, 1))
    face = np.zeros((2, 2), np.int64)
    verts = np.array([[[3.0, 2.0, 0.0], [4.2, 2.6, 2.0], [-9.0, 50.0, 1.0]]], np.float32)
    image = np.arange(1, 3 * 4 * 6 + 1, dtype=np.float32).reshape(1, 3, 4, 6)
    K, Rt = np.eye(3, dtype=np.float32)[None], np.eye(4, dtype=np.float32)[None, :3]
    index_img = np.zeros((1, 4, 6), np.int64)
    o = C.compute(verts, image, index_img, K, Rt, idx, bary, face, 1)
    assert (o.cam_z[0, 0] == 0).all() and (o.tex[0, :, 0] == 0).all() and (o.tex[0, :, 1] != 0).all() and not o.band.any()
    tex, mask = viewtex.compute_view_texture(_t(verts), torch.zeros(1, 3, dtype=torch.int64).cuda(), _t(image), _t(index_img),
                                             None, _t(K), _t(Rt), _t(idx), _t(bary), _t(face))
    assert np.array_equal(_np(tex), o.tex) and _np(mask).all()
    assert _np(tex)[0, :, 1, 0].tolist() == image[0, :, 1, 2].tolist()          # pix (2.1, 1.3) -> pixel (2, 1)
    assert _np(tex)[0, :, 1, 1].tolist() == image[0, :, 3, 0].tolist()          # pix (-9, 50) -> the border


# ---- drop-in ----------------------------------------------------------------------------------------------------------------
def test_patched_stand_in_module_runs_viewtex():
    from goliath_amd import dropin, viewtex

    m = types.ModuleType("stand_in_geom")

    def refuse(*a, **k):
        raise AssertionError("the reference must not run for CUDA float32 inputs")

    m.compute_face_visibility = m.compute_uv_visiblity_face = m.compute_view_texture = refuse
    assert dropin.patch_view_texture(m, None) is m
    c, o = C.case("b"), C.oracle("b", C.THRESHOLD)
    a = _args(c)
    tex, mask = m.compute_view_texture(*a, intensity_threshold=C.THRESHOLD, normal_threshold=0.1)
    tex_v, mask_v = viewtex.compute_view_texture(*a, intensity_threshold=C.THRESHOLD, normal_threshold=0.1)
    assert np.array_equal(_np(tex).view(np.uint32), _np(tex_v).view(np.uint32)) and torch.equal(mask, mask_v)
    assert np.array_equal(_np(mask), o.mask)
    assert np.array_equal(_np(m.compute_face_visibility(a[3], a[1])), o.face_vis)
    assert np.array_equal(_np(m.compute_uv_visiblity_face(a[3], a[1], a[9])), o.mask[:, 0])
    with pytest.raises(AssertionError):
        m.compute_face_visibility(a[3].cpu(), a[1].cpu())                         # non-CUDA: the reference


# ---- get_tex_rl -------------------------------------------------------------------------------------------------------------
def test_get_tex_rl_rasterises_the_mesh_itself():
    from goliath_amd import meshraster, viewtex

    c = C.case("f")                                                                # a watertight grid mesh
    views = [0, 1]
    verts = _t(c.verts[0:1])
    image, K, Rt = _t(c.image[views]), _t(c.K[views]), _t(c.Rt[views])
    tex, mask = viewtex.get_tex_rl(None, image, (verts, _t(c.faces)), Rt, K, _t(c.face_index_uv), _t(c.index_image_uv),
                                   _t(c.bary_image_uv))
    index_img = meshraster.rasterize(meshraster.transform(verts.expand(2, -1, -1), K, Rt), _t(c.faces), C.H, C.W,
                                     with_bary=False)[0]
    index_img = _np(index_img).astype(np.int64)
    assert ((index_img >= 0).mean(axis=(1, 2)) > 0.5).all() and len(np.unique(index_img)) > 20
    o = C.compute(c.verts[0:1], c.image[views], index_img, c.K[views], c.Rt[views], c.index_image_uv, c.bary_image_uv,
                  c.face_index_uv, c.F)
    assert tuple(tex.shape) == (2, 3, c.S, c.S) and tuple(mask.shape) == (2, 1, c.S, c.S) and mask.dtype == torch.bool
    assert np.array_equal(_np(mask), o.mask) and o.mask.any() and not o.mask.all()
    out = ~o.band
    assert np.array_equal(_np(tex)[..., out], o.tex[..., out]) and C.in_alts(_np(tex), o, o.band).all()
