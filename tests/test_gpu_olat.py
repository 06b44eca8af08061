"""GPU: csrc/olat.hip -- the MVP teacher's UNet input (gol_olat_features_fwd) and OLAT sum (gol_olat_combine_fwd / _bwd).

Yardsticks: the reference's own forward_rgb (tests/golden/urhand_model_golden.npz at B = 1, L = 2 in eval mode,
tests/golden/olat_golden.npz at B = 2, L = 3 in train mode, both made on the CPU by the reference's code) and the torch
lines the kernels replace, run in float64 (tests/olat_cases.py).  Bars: rel-L2 < 1e-6 on the UNet input (what
test_gpu_urhand_model.py holds it to), < 2e-6 on the combine's outputs (the project's bar for primrgb), < 3e-5 on gradients
and model-level outputs (the project's gradient bar); the features' largest error may be at most 8 x that of the float32
torch lines against the same float64.  Every test prints what it measured.

Measured on an MI355X (rel-L2 unless stated): features against the reference's UNet input 4.8e-8 (directions) and 0
(1 - shadow); against float64 <= 5.9e-8 in every case, largest error <= 1.8e-7 where the float32 torch lines have
1.1-1.6e-7 (ratio <= 1.43); combine forward <= 6.2e-8, backward <= 6.7e-8; the fused forward_rgb against the train golden
<= 5.4e-8 on the outputs and <= 3.2e-7 on the gradients, against the unfused function in eval mode <= 9.4e-8.
"""
import functools
import os

import numpy as np
import pytest
import torch

import olat_cases as C
import urhand_shaped as S
from scenes import rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
GOLD_EVAL = np.load(os.path.join(HERE, "golden", "urhand_model_golden.npz"))
GOLD = np.load(os.path.join(HERE, "golden", "olat_golden.npz"))


def _cuda(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


def _features(case):
    from goliath_amd import olat

    return olat.features(*(case[k] for k in C.GEOM_KEYS), case["shadow"], case["primsize"], case["npx"], case["npy"],
                         case["volradius"])


def _features_ref(case, dtype):
    return C.features_ref(*(case[k] for k in C.GEOM_KEYS), case["shadow"], case["primsize"], case["npx"], case["npy"],
                          case["volradius"], dtype=dtype)


# ------------------------------------------------------------------------------------------------------------- features
def test_features_match_the_reference_unet_input():
    """Against forward_rgb's own UNet input.  The kernel is fed the golden's shadow volume, recovered from the golden's
    1 - shadow channels; that round trip is not exact in float32, so those channels share the rel-L2 bar."""
    want = torch.from_numpy(GOLD_EVAL["teacher_unet_input"]).cuda()
    Z = 2
    case = _cuda({**C.standin_case(1, 2), "shadow": C.uv_to_prim(1.0 - want[:, 6 * Z:].cpu(), (4, 4, 2), 4, 4)})
    x = _features(case)
    assert x.shape == want.shape and not x.requires_grad
    e_dirs, e_shadow = rel_l2(x[:, :6 * Z], want[:, :6 * Z]), rel_l2(x[:, 6 * Z:], want[:, 6 * Z:])
    print("\nOLAT_FEATURES reference", dict(dirs=e_dirs, one_minus_shadow=e_shadow))
    assert e_dirs < 1e-6 and e_shadow < 1e-6


FEATURE_CASES = [("standin", b, l) for b in (1, 2) for l in (1, 2, 3)] + [("odd", 2, 2), ("degenerate", 1, 2)]


@pytest.mark.parametrize("name,B,L", FEATURE_CASES)
def test_features_against_float64(name, B, L):
    hit = None
    if name == "standin":
        case = C.standin_case(B, L)
    elif name == "odd":
        case = C.odd_case()
    else:
        case, hit = C.degenerate_case()
    case = _cuda(case)
    X, Y, Z = case["primsize"]
    npx, npy = case["npx"], case["npy"]
    x = _features(case)
    ref = _features_ref(case, torch.float64)
    f32 = _features_ref(case, torch.float32)
    assert x.shape == ref.shape == (B * L, 7 * Z, npy * Y, npx * X)
    dirs = slice(0, 6 * Z)
    e = rel_l2(x[:, dirs], ref[:, dirs])
    worst = float((x[:, dirs].double() - ref[:, dirs]).abs().max())
    worst32 = float((f32[:, dirs].double() - ref[:, dirs]).abs().max())
    print("\nOLAT_FEATURES", name, B, L, dict(rel_l2=e, max_err=worst, max_err_torch32=worst32, ratio=worst / worst32))
    assert e < 1e-6
    assert worst <= 8.0 * worst32
    # 1 - shadow: the test made shadow itself, so the kernel's subtraction must be torch's bit for bit
    assert torch.equal(x[:, 6 * Z:], 1.0 - C.prim_to_uv(case["shadow"], case["primsize"], npx, npy))
    dead = (case["valid_prims"] == 0).reshape(npy, npx).repeat_interleave(Y, 0).repeat_interleave(X, 1)
    if bool(dead.any()):
        assert bool((x[:, dirs][:, :, dead] == 0).all())
        assert bool((x[:, dirs][:, :, ~dead] != 0).any())
    if hit is not None:     # the light sits on these voxels: the yardstick's direction is the zero vector
        assert float(ref[hit.cuda()].abs().max()) == 0.0
        assert bool(torch.isfinite(x[hit.cuda()]).all())
    assert bool(torch.isfinite(x).all())
    assert torch.equal(x, _features(case))


# -------------------------------------------------------------------------------------------------------------- combine
def _combine_case(geom, B, L):
    if geom == "standin":
        return _cuda(C.combine_case(B, L))
    return _cuda(C.combine_case(B, L, primsize=(2, 4, 3), npx=6, npy=3))      # a lane owns one texel


def _combine(cc, tex, use_shadow, want_texolat):
    from goliath_amd import olat

    return olat.combine(tex, cc["light_intensity"], cc["shadow"], cc["primsize"], cc["npx"], cc["npy"], use_shadow,
                        want_texolat)


@pytest.mark.parametrize("geom", ["standin", "odd"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("use_shadow", [False, True])
@pytest.mark.parametrize("want_texolat", [False, True])
def test_combine_forward(geom, L, use_shadow, want_texolat):
    B = 2
    cc = _combine_case(geom, B, L)
    rgb, texolat, primshadow = _combine(cc, cc["tex"], use_shadow, want_texolat)
    r_rgb, r_texolat, r_ps = C.combine_ref(cc["tex"], cc["light_intensity"], cc["shadow"], cc["primsize"], cc["npx"],
                                           cc["npy"], use_shadow)
    assert rgb.shape == r_rgb.shape and primshadow.shape == r_ps.shape and primshadow.is_contiguous()
    errs = dict(rgb=rel_l2(rgb, r_rgb), primshadow=rel_l2(primshadow, r_ps))
    if want_texolat:
        assert texolat.shape == r_texolat.shape
        errs["texolat"] = rel_l2(texolat, r_texolat)
        for n, c, r, q in cc["kinks"]:
            assert float(texolat.reshape(B * L, -1, 3, *texolat.shape[-2:])[n, c // 4, c % 4 - 1, r, q]) == 0.0
    else:
        assert texolat is None
    print("\nOLAT_COMBINE fwd", geom, L, use_shadow, want_texolat, errs)
    assert all(v < 2e-6 for v in errs.values()), errs
    again = _combine(cc, cc["tex"], use_shadow, want_texolat)
    assert all(torch.equal(a, b) for a, b in zip(again, (rgb, texolat, primshadow)) if a is not None)


@pytest.mark.parametrize("geom", ["standin", "odd"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("use_shadow", [False, True])
@pytest.mark.parametrize("g_texolat", ["used", "unused", "absent"])
def test_combine_backward(geom, L, use_shadow, g_texolat):
    """g_texolat: "used" = the loss reads texolat; "unused" = texolat is returned but receives no gradient; "absent" =
    texolat is not formed at all."""
    B = 2
    cc = _combine_case(geom, B, L)
    X, Y, Z = cc["primsize"]
    g = torch.Generator().manual_seed(31)
    r1 = torch.randn(B, Z, 3, cc["npy"] * Y, cc["npx"] * X, generator=g).cuda()
    r2 = torch.randn(B, L, Z, 3, cc["npy"] * Y, cc["npx"] * X, generator=g).cuda()

    def grad_of(fn, tex):
        tex = tex.clone().requires_grad_(True)
        rgb, texolat, primshadow = fn(tex)
        assert not primshadow.requires_grad
        loss = (rgb * r1.to(rgb.dtype)).sum()
        if g_texolat == "used":
            loss = loss + (texolat * r2.to(rgb.dtype)).sum()
        loss.backward()
        return tex.grad

    got = grad_of(lambda t: _combine(cc, t, use_shadow, g_texolat != "absent"), cc["tex"])
    want = grad_of(lambda t: C.combine_ref(t, cc["light_intensity"], cc["shadow"], cc["primsize"], cc["npx"], cc["npy"],
                                           use_shadow), cc["tex"].double())
    assert got.shape == cc["tex"].shape and got.dtype == torch.float32
    e = rel_l2(got, want)
    print("\nOLAT_COMBINE bwd", geom, L, use_shadow, g_texolat, e)
    assert e < 3e-5
    if use_shadow:
        assert bool((got[:, 0::4] == 0).all())
    else:
        assert bool((got[:, 0::4] != 0).any())
    for n, c, r, q in cc["kinks"]:      # texolat is exactly 0 there: the relu passes nothing, 25 g_texolat remains
        expect = 25.0 * float(r2.reshape(B * L, Z, 3, *r2.shape[-2:])[n, c // 4, c % 4 - 1, r, q]) if g_texolat == "used" else 0.0
        assert float(got[n, c, r, q]) == np.float32(expect), (n, c, r, q)
    assert torch.equal(got, grad_of(lambda t: _combine(cc, t, use_shadow, g_texolat != "absent"), cc["tex"]))


# ---------------------------------------------------------------------------------------------------------- model level
def _decoder(training):
    from goliath_amd import mvp

    return S.ShapedOLATRGBDecoder(mvp.Raymarcher(200.0), 200.0, seed=0).cuda().train(training)


@pytest.mark.parametrize("tag,iteration", [("it0", 0), ("it5000", 5000)])
def test_fused_forward_rgb_matches_the_reference_in_train_mode(tag, iteration, monkeypatch):
    """The reference's forward_rgb in train mode (iteration 0: the shadow warm-up branch), with the golden's own deep-shadow
    volume replayed so that everything after the march is compared at rounding level."""
    from goliath_amd import urhand

    B, L = 2, 3
    volume = torch.from_numpy(GOLD[f"{tag}_shadow"]).cuda()
    monkeypatch.setattr(urhand, "deep_shadow", lambda *a, **k: volume)
    dec = _decoder(True)
    captured = {}
    dec.enc_layers[0].register_forward_pre_hook(lambda m, a: captured.__setitem__("x", a[0]))
    inp = _cuda(S.teacher_inputs(B=B, L=L))
    inp["joint_feat"].requires_grad_(True)
    res = urhand.olat_rgb_decoder_forward_rgb_fused(dec, **inp, iteration=iteration)
    assert set(res) == {"primrgb", "primshadow", "texolat"} and not captured["x"].requires_grad
    errs = {k: rel_l2(res[k], torch.from_numpy(GOLD[f"{tag}_{k}"])) for k in ("primrgb", "primshadow", "texolat")}
    errs["unet_input"] = rel_l2(captured["x"], torch.from_numpy(GOLD[f"{tag}_unet_input"]))
    g = torch.Generator().manual_seed(7)
    r1 = torch.randn(res["primrgb"].shape, generator=g).cuda()
    r2 = torch.randn(res["texolat"].shape, generator=g).cuda()
    ((res["primrgb"] * r1).sum() + (res["texolat"] * r2).sum()).backward()
    grads = dict(joint_feat=inp["joint_feat"].grad, enc0_weight=dec.enc_layers[0][0].weight.grad,
                 declast_weight=dec.dec_layers[-1][0].weight.grad)
    gerrs = {k: rel_l2(v, torch.from_numpy(GOLD[f"{tag}_grad_{k}"])) for k, v in grads.items()}
    print("\nOLAT_MODEL train", tag, errs, gerrs)
    assert all(v < 3e-5 for v in errs.values()), errs
    assert all(v < 3e-5 for v in gerrs.values()), gerrs


def test_fused_forward_rgb_matches_the_unfused_one_in_eval_mode():
    """Same GPU inputs, the march included (both functions run it themselves)."""
    from goliath_amd import urhand

    dec = _decoder(False)
    inp = _cuda(S.teacher_inputs(B=2, L=3))
    with torch.no_grad():
        want = urhand.olat_rgb_decoder_forward_rgb(dec, **inp)
        got = urhand.olat_rgb_decoder_forward_rgb_fused(dec, **inp)
    assert set(got) == set(want) == {"primrgb", "primshadow"}
    errs = {k: rel_l2(got[k], want[k]) for k in want}
    print("\nOLAT_MODEL eval fused vs unfused", errs)
    assert all(v < 3e-5 for v in errs.values()), errs
