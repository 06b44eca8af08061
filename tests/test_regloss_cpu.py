"""CPU: the regulariser operators of goliath_amd.losses refuse CPU tensors, dropin.patch_losses(regularizers=True) rebinds
exactly their registry names, and their parameter lists are the reference's."""
import inspect
import os
import sys
import types

import pytest
import torch

REF = "/root/reference"
SEVEN = ("bound_primscale", "negcolor", "l2_reg", "list_l1_reg", "backlit_reg", "alphaprior", "mask_l1")


def test_cpu_tensors_raise():
    from goliath_amd import _lib, losses

    x = torch.rand(2, 5, 3)
    cw = torch.rand(2, 5, 1) - 0.5
    calls = {
        "penalty_mean": lambda: losses.penalty_mean(x, losses.SQ),
        "backlit": lambda: losses.backlit(x, cw),
        "bound_primscale": lambda: losses.bound_primscale({"primscale_preclip": x}),
        "negcolor": lambda: losses.negcolor({"diff_color": x}),
        "l2_reg": lambda: losses.l2_reg({"spec_dnml": x}),
        "list_l1_reg": lambda: losses.list_l1_reg({"spec_dnml": [x, x[0]]}),
        "backlit_reg": lambda: losses.backlit_reg({"color_rand": x, "cos_weight": cw}),
        "alphaprior": lambda: losses.alphaprior({"alpha": torch.rand(2, 4, 4)}),
        "mask_l1": lambda: losses.mask_l1({"rendered_mask": torch.rand(2, 1, 4, 4)}, {"image_mask": torch.rand(2, 1, 4, 4)}),
    }
    assert set(SEVEN) <= set(calls)
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

    entries = {name: "reference" for name in SEVEN}
    entries.update(rgb_l1="reference", rgb_ssim="reference", kl="untouched", primvolsum="untouched")
    return types.SimpleNamespace(loss_registry=entries, FnLoss=FnLoss)


def test_patch_losses_default_leaves_the_regularisers():
    from goliath_amd import dropin, losses

    reg = _stand_in_registry()
    assert dropin.patch_losses(reg) is reg
    assert all(reg.loss_registry[name] == "reference" for name in SEVEN)
    assert reg.loss_registry["kl"] == "untouched" and reg.loss_registry["primvolsum"] == "untouched"
    assert reg.loss_registry["rgb_l1"](None).fn is losses.rgb_l1


def test_patch_losses_regularizers_rebinds_exactly_the_seven():
    from goliath_amd import dropin, losses

    reg = _stand_in_registry()
    before = dict(reg.loss_registry)
    assert dropin.patch_losses(reg, regularizers=True) is reg
    changed = {k for k in reg.loss_registry if reg.loss_registry[k] is not before.get(k)}
    assert changed == set(SEVEN) | {"rgb_l1", "rgb_ssim"}
    assert set(reg.loss_registry) == set(before)
    assert reg.loss_registry["kl"] == "untouched" and reg.loss_registry["primvolsum"] == "untouched"
    assert tuple(dropin.REGULARIZER_LOSSES) == SEVEN
    for name in SEVEN:
        mod = reg.loss_registry[name](None)
        assert isinstance(mod, reg.FnLoss) and mod.fn is getattr(losses, name) and mod.extra_args == {}
    mod = reg.loss_registry["bound_primscale"](None, min_scale=0.2, max_scale=5.0)
    assert mod.fn is losses.bound_primscale and mod.extra_args == {"min_scale": 0.2, "max_scale": 5.0}


def test_kind_constants_are_the_headers_enum():
    from goliath_amd import losses, optim

    assert (losses.BOUND, losses.NEG_SQ, losses.SQ, losses.ABS, losses.ALPHAPRIOR) == (0, 1, 2, 3, 4)
    assert losses.regloss_chunk_elems() == optim.chunk_elems()   # both entries return csrc/gol_stream.h's one constant
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "goliath_hip.h")).read()
    for name, value in (("BOUND", 0), ("NEG_SQ", 1), ("SQ", 2), ("ABS", 3), ("ALPHAPRIOR", 4)):
        assert f"GOL_REGLOSS_{name} = {value}" in hdr    # the Python constants are the header's enum


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
def test_parameter_lists_equal_the_reference():
    from goliath_amd import losses

    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import ref_stubs

    ref_stubs.install()
    sys.modules.setdefault("sgutilslib", types.ModuleType("sgutilslib"))
    import ca_code.loss as L

    params = lambda fn: [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]
    theirs = {"bound_primscale": L.loss_bound_primscale, "negcolor": L.loss_negcolor, "l2_reg": L.loss_l2_reg,
              "list_l1_reg": L.loss_list_l1_reg, "backlit_reg": L.loss_backlight_reg, "alphaprior": L.loss_alphaprior,
              "mask_l1": L.mask_l1}
    assert set(theirs) == set(SEVEN)
    for name, fn in theirs.items():
        assert params(getattr(losses, name)) == params(fn), name
