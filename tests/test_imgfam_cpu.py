"""CPU: the image-loss and mask operators of goliath_amd.losses / goliath_amd.imageops refuse CPU tensors,
dropin.patch_losses(images=True) rebinds exactly IMAGE_LOSSES, dropin.patch_image_ops rebinds only names that exist, the
parameter lists are the reference's, and the committed fixture holds what the GPU tests rely on."""
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import imgfam_cases as cases  # noqa: E402
import npz_parts  # noqa: E402

REF = "/root/reference"
FIVE = ("rgb_l2", "psnr", "rgb_l1_focus", "rgb_l1_phys", "pose_shadow_l2")
SEVEN = ("bound_primscale", "negcolor", "l2_reg", "list_l1_reg", "backlit_reg", "alphaprior", "mask_l1")


@pytest.fixture(scope="module")
def golden():
    return npz_parts.load(os.path.join(HERE, "golden", "imgfam_golden.npz"))


def test_cpu_tensors_raise():
    from goliath_amd import _lib, imageops, losses

    img, m = torch.rand(2, 3, 5, 7), torch.ones(2, 1, 5, 7)
    dd = torch.zeros(2, 1, 5, 7, dtype=torch.bool)
    preds = {"rendered_rgb": img, "rendered_rgb_blur": img, "rendered_phys_rgb": img, "rendered_mask": m, "depth_disc_mask": dd,
             "pose_shadow_map": m, "shadow_map": m}
    targets = {"image": img, "image_mask": m}
    calls = {
        "image_penalty": lambda: losses.image_penalty(img, img, losses.IMG_SQ, m, dd),
        "rgb_l2": lambda: losses.rgb_l2(preds, targets),
        "rgb_l2 eroded": lambda: losses.rgb_l2(preds, targets, mask_erode=3),
        "rgb_l2 no mask": lambda: losses.rgb_l2({"rendered_rgb": img}, {"image": img}, mask_erode=3),
        "psnr": lambda: losses.psnr(preds, targets),
        "rgb_l1_focus": lambda: losses.rgb_l1_focus(preds, targets, mask_erode=3, self_mask=True),
        "rgb_l1_phys": lambda: losses.rgb_l1_phys(preds, targets),
        "pose_shadow_l2": lambda: losses.pose_shadow_l2(preds),
        "depth_discontinuity_mask": lambda: imageops.depth_discontinuity_mask(m),
        "erode": lambda: imageops.erode(m, 3),
        "erode bool": lambda: imageops.erode(dd, 3),
    }
    assert set(FIVE) <= set(calls)
    for name, fn in calls.items():
        with pytest.raises(_lib.GoliathHipError):
            fn()
        pytest.raises(RuntimeError, fn)   # (GoliathHipError is a RuntimeError, as the reference's CHECK_INPUT raises)


def _stand_in_registry():
    class FnLoss(torch.nn.Module):  # same contract as ca_code/loss/registry.py:40-56
        def __init__(self, fn, function_args):
            super().__init__()
            self.fn, self.extra_args = fn, function_args

        def forward(self, preds, targets):
            return self.fn(preds, targets, **self.extra_args)

    entries = {name: "reference" for name in SEVEN + FIVE}
    entries.update(rgb_l1="reference", rgb_ssim="reference", kl="untouched", primvolsum="untouched", vgg="untouched")
    return types.SimpleNamespace(loss_registry=entries, FnLoss=FnLoss)


def _changed(reg, before):
    assert set(reg.loss_registry) == set(before)
    return {k for k in reg.loss_registry if reg.loss_registry[k] is not before[k]}


def test_the_two_existing_modes_rebind_what_they_did():
    from goliath_amd import dropin

    reg = _stand_in_registry()
    before = dict(reg.loss_registry)
    assert dropin.patch_losses(reg) is reg
    assert _changed(reg, before) == {"rgb_l1", "rgb_ssim"}
    reg = _stand_in_registry()
    assert dropin.patch_losses(reg, regularizers=True) is reg
    assert _changed(reg, before) == set(SEVEN) | {"rgb_l1", "rgb_ssim"}
    assert inspect.signature(dropin.patch_losses).parameters["images"].default is False


def test_images_rebinds_exactly_the_five():
    from goliath_amd import dropin, losses

    assert tuple(dropin.IMAGE_LOSSES) == FIVE
    reg = _stand_in_registry()
    before = dict(reg.loss_registry)
    assert dropin.patch_losses(reg, images=True) is reg
    assert _changed(reg, before) == set(FIVE) | {"rgb_l1", "rgb_ssim"}
    for name in FIVE:
        mod = reg.loss_registry[name](None)
        assert isinstance(mod, reg.FnLoss) and mod.fn is getattr(losses, name) and mod.extra_args == {}
    mod = reg.loss_registry["rgb_l1_focus"](None, mask_erode=3, self_mask=True)
    assert mod.fn is losses.rgb_l1_focus and mod.extra_args == {"mask_erode": 3, "self_mask": True}
    reg = _stand_in_registry()
    dropin.patch_losses(reg, regularizers=True, images=True)
    assert _changed(reg, before) == set(FIVE) | set(SEVEN) | {"rgb_l1", "rgb_ssim"}


def test_patch_image_ops_rebinds_only_names_that_exist():
    from goliath_amd import dropin, imageops

    theirs = lambda *a, **k: None
    model = types.SimpleNamespace(__name__="model", depth_discontuity_mask=theirs, dilate=theirs)
    loss = types.SimpleNamespace(__name__="loss", erode=theirs, rgb_l1=theirs)
    both = types.SimpleNamespace(__name__="both", depth_discontuity_mask=theirs, erode=theirs)
    neither = types.SimpleNamespace(__name__="neither", other=theirs)
    done = dropin.patch_image_ops(model, loss, both, neither)
    assert model.depth_discontuity_mask is imageops.depth_discontinuity_mask and model.dilate is theirs
    assert not hasattr(model, "erode") and not hasattr(loss, "depth_discontuity_mask")
    assert loss.erode is imageops.erode and loss.rgb_l1 is theirs
    assert both.depth_discontuity_mask is imageops.depth_discontinuity_mask and both.erode is imageops.erode
    assert vars(neither) == {"__name__": "neither", "other": theirs}
    assert done == [("model", "depth_discontuity_mask"), ("loss", "erode"), ("both", "depth_discontuity_mask"), ("both", "erode")]
    assert dropin.IMAGE_OP_MODULES == ("ca_code.models.urhand", "ca_code.models.mesh_vae", "ca_code.models.mesh_vae_drivable",
                                       "ca_code.loss")


def test_kind_constants_are_the_headers_enum():
    from goliath_amd import losses, optim

    assert (losses.IMG_ABS, losses.IMG_SQ, losses.IMG_EXPW) == (0, 1, 2)
    assert losses.imgloss_chunk_elems() == optim.chunk_elems() == 4096   # csrc/gol_stream.h's one constant; cases.HWS sit on it
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "goliath_hip.h")).read()
    for name, value in (("ABS", 0), ("SQ", 1), ("EXPW", 2)):
        assert f"GOL_IMGLOSS_{name} = {value}" in hdr    # the Python constants are the header's enum
    assert [cases.KINDS.index(k) for k in ("abs", "sq", "expw")] == [losses.IMG_ABS, losses.IMG_SQ, losses.IMG_EXPW]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
def test_parameter_lists_equal_the_reference():
    from goliath_amd import imageops, losses

    sys.path.insert(0, os.path.join(HERE, "golden"))
    import ref_stubs

    ref_stubs.install()
    sys.modules.setdefault("sgutilslib", types.ModuleType("sgutilslib"))
    import ca_code.loss as L
    import ca_code.utils.geom as geom
    import ca_code.utils.image as image

    params = lambda fn: [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]
    theirs = {"rgb_l2": L.rgb_l2, "psnr": L.psnr, "rgb_l1_focus": L.rgb_l1_focus, "rgb_l1_phys": L.rgb_l1_phys,
              "pose_shadow_l2": L.pose_to_shadow_l2_loss}
    assert set(theirs) == set(FIVE)
    for name, fn in theirs.items():
        assert params(getattr(losses, name)) == params(fn), name
    assert params(imageops.depth_discontinuity_mask) == params(geom.depth_discontuity_mask)
    assert params(imageops.erode) == params(image.erode)


# ---- the committed fixture ------------------------------------------------------------------------------------------------
def test_fixture_float_scene_stays_under_the_cap(golden):
    depth = golden["disc/float/depth"]
    assert depth.dtype == np.float32 and depth.min() == 0.0 and (depth == 0).mean() > 0.3    # a blob on a zero background
    for pool in cases.POOLS:
        ref = golden[f"disc/float/p{pool}"]
        yes, no = cases.decide(depth, pool)
        flagged = ~(yes | no)
        assert flagged.mean() <= cases.FLAGGED_CAP, (pool, int(flagged.sum()))
        assert yes.sum() > 100 and no.sum() > 100                      # the norm crosses the threshold inside the image
        assert ref[yes].all() and not ref[no].any()                    # the reference's own float32 output agrees
    s, _ = cases.sobel_norm64(depth)
    ring = (s > 39.0) & (s < 41.0)
    assert ring.sum() > 20                                             # ... along a circle, not at a jump


def test_fixture_exact_scenes(golden):
    for H, W in cases.SIZES:
        tag = cases.size_tag(H, W)
        depth = golden[f"disc/{tag}/depth"]
        assert depth.shape[1:] == (H, W) and depth.shape[0] >= 6
        assert depth.min() >= 0 and depth.max() <= 512 and np.array_equal(depth, np.round(depth))
        hot, seam = cases.marks(H, W)
        assert all(depth[0][p] == 512 for p in hot) and all(depth[1][p] == 512 for p in seam)
        assert depth[2][0, 0] == 300                                   # the plateau on the border
        # exact integers: the float64 norm decides every pixel as the reference's float32 did
        s, _ = cases.sobel_norm64(depth)
        n = np.round(s * s)
        for pool in cases.POOLS:
            for ti, thr in enumerate(cases.THRESHOLDS):
                fire = np.sqrt(n.astype(np.float32)) > np.float32(thr)
                assert np.array_equal(cases.window_any(fire, pool), golden[f"disc/{tag}/p{pool}t{ti}"]), (tag, pool, ti)
    # the thresholds separate n = 1600 (the straight steps) from its neighbours
    tag = cases.size_tag(*cases.STEP_SIZE)
    assert golden[f"disc/{tag}/depth"].shape[0] == 6 + cases.TILE_W + 2 + cases.TILE_H + 2
    counts = [int(golden[f"disc/{tag}/p1t{ti}"].sum()) for ti in range(len(cases.THRESHOLDS))]
    assert counts[0] > counts[1] == counts[2] > counts[3] > 0
    seams_x, seams_y = cases.seams(cases.STEP_SIZE[1], cases.TILE_W), cases.seams(cases.STEP_SIZE[0], cases.TILE_H)
    assert seams_x == [63, 64, 127, 128] and seams_y == [15, 16, 31, 32]


def test_fixture_erosion_scenes(golden):
    """0.5 vetoes like 0 and 1.0 does not: the single-half scene (4) loses exactly the half's window."""
    tag = cases.size_tag(33, 35)
    x, out = golden[f"erode/{tag}/x"], golden[f"erode/{tag}/f3"]
    assert set(np.unique(x)) == {0.0, 0.5, 1.0} and (x[4] == 0.5).sum() == 1
    assert (out[4] == 0).sum() == 9 and out[4][15:18, 16:19].sum() == 0
    for H, W in cases.SIZES:
        t = cases.size_tag(H, W)
        for ks in cases.ERODE_KS:
            f, b = golden[f"erode/{t}/f{ks}"], golden[f"erode/{t}/b{ks}"]
            assert f.dtype == np.float32 and b.dtype == np.bool_ and np.array_equal(f > 0, b)
            assert f[2].all()                                          # all ones stays all ones up to the border
            assert np.array_equal(f, (~cases.window_any(golden[f"erode/{t}/x"] < 1.0, ks)).astype(np.float32))


def test_fixture_loss_inputs_hold_the_kinks(golden):
    for B, C in cases.BCS:
        for HW in cases.HWS:
            tag = f"loss/{cases.shape_tag(B, C, HW)}/"
            pred, target, m1, mc, veto = (golden[tag + k] for k in ("pred", "target", "mask1", "maskc", "veto"))
            assert pred.shape == target.shape == mc.shape == (B, C, HW) and m1.shape == veto.shape == (B, 1, HW)
            assert pred.dtype == np.float32 and veto.dtype == np.bool_
            for kind in cases.KINDS:
                for mk in cases.MASKS:
                    for vk in cases.VETOS:
                        pre = f"{tag}{kind}/{mk}-{vk}/"
                        assert golden[pre + "grad64"].dtype == np.float64 and golden[pre + "grad32"].dtype == np.float32
                        assert golden[pre + "grad64"].shape == pred.shape and golden[pre + "loss64"].shape == ()
            if HW < 4095:
                continue
            r = pred.astype(np.float64) - target
            assert (r == 0).any()                                              # pred == target exactly
            assert ((r > 0) & (r < 1e-4)).any() and ((r < 0) & (r > -1e-4)).any()   # both signs next to 0
            assert np.abs(r).max() == 255.0                                    # the focus weight reaches e
            for m in (m1, mc):
                assert (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any()
            assert 0.05 < veto.mean() < 0.15
            if (B, C) != (1, 1):                                               # the planes differ
                assert not np.array_equal(pred[0, 0], pred[0, 1]) and not np.array_equal(pred[0], pred[1])
    e = golden[f"loss/{cases.shape_tag(2, 3, 4097)}/expw/full-veto/grad64"]
    assert np.isfinite(e).all() and (e == 0).any() and (e > 0).any() and (e < 0).any()
