"""CPU: the public surface of the fused relight visualisation (goliath_amd/envbg.py, dropin.patch_relight_vis, the
gol_envbg_* entries) -- everything that can be checked without a GPU."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gol_envbg_blur_taps", "gol_envbg_scratch_floats", "gol_envbg_image", "gol_envbg_compose")


def test_blur_taps_are_the_normalised_reference_vector():
    from goliath_amd import envbg

    k = envbg.blur_taps()
    assert k.dtype == torch.float64 and tuple(k.shape) == (101,)
    assert torch.equal(k, k.flip(0))
    assert abs(float(k.sum()) - 1.0) <= 1e-15
    want = torch.exp(-torch.linspace(-4.0, 4.0, 101, dtype=torch.float64) ** 2)
    want = want / want.sum()
    # equal up to the rounding of the abscissae: a linspace point may differ by one ulp of 4 (8.9e-16) between two correct
    # constructions (fused or plain start + i * step), which exp(-t^2) turns into a relative 2 |t| dt <= 7.1e-15 = 32 eps;
    # exp, the sum (in symmetric pairs in the library) and the division add a few eps more
    assert bool(((k - want).abs() <= 40 * torch.finfo(torch.float64).eps * want).all())


def test_blur_taps_is_the_librarys_vector():
    """One definition: blur_taps() returns what gol_envbg_blur_taps writes, the values gol_envbg_image hands to its kernels."""
    from goliath_amd import _lib, envbg

    buf = (ctypes.c_double * 101)()
    assert _lib.load().gol_envbg_blur_taps(buf) == 0
    assert torch.equal(envbg.blur_taps(), torch.tensor(list(buf), dtype=torch.float64))


def _inputs(B=1, H=200, W=200):
    return (torch.zeros(B, 3, H, W), torch.zeros(B, 1, H, W), torch.zeros(B, 3, 8, 16), torch.eye(3)[None].repeat(B, 1, 1),
            torch.eye(4)[:3][None].repeat(B, 1, 1))


def test_cpu_tensors_raise():
    from goliath_amd import _lib, envbg

    render, alpha, env, K, Rt = _inputs()
    with pytest.raises(_lib.GoliathHipError):
        envbg.compose_envmap(render, alpha, env, K, Rt)
    with pytest.raises(_lib.GoliathHipError):
        envbg.env_background(env, K, Rt, 200, 200)
    with pytest.raises(_lib.GoliathHipError):
        envbg.env_background(env, K, Rt, 20, 20, blur=False)


@pytest.mark.parametrize("H,W", [(199, 200), (200, 199)])
def test_an_image_smaller_than_the_ball_is_a_value_error(H, W):
    from goliath_amd import envbg

    with pytest.raises(ValueError):
        envbg.compose_envmap(*_inputs(1, H, W))


def test_patch_relight_vis_sets_a_class_flag_once():
    from goliath_amd import dropin, rgca

    class AutoEncoder:
        pass

    mod = types.SimpleNamespace(AutoEncoder=AutoEncoder)
    assert getattr(AutoEncoder, rgca.RELIGHT_VIS_FLAG, False) is False
    assert getattr(AutoEncoder(), rgca.RELIGHT_VIS_FLAG, False) is False
    assert dropin.patch_relight_vis(mod) is mod
    assert getattr(AutoEncoder(), rgca.RELIGHT_VIS_FLAG) is True
    before = dict(vars(AutoEncoder))
    assert dropin.patch_relight_vis(mod) is mod
    assert dict(vars(AutoEncoder)) == before


def test_render_views_extra_colors_is_forward_only():
    """Grad mode on and an input that requires grad: raises before anything is launched (CPU tensors never get that far)."""
    from goliath_amd import _lib, splat

    a = lambda *s: torch.ones(*s)
    extra = torch.ones(1, 4, 6, requires_grad=True)
    with pytest.raises(_lib.GoliathHipError, match="forward-only"):
        splat.render_views(a(1, 4, 3), a(1, 4, 3), a(1, 4, 4), a(1, 4), a(1, 4, 3), torch.eye(4)[:3][None], a(1, 4), 32, 32,
                           extra_colors=extra)


def test_entries_are_declared_bound_and_exported():
    from goliath_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goliath_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in goliath_hip.h"
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name)
    fn = lib.gol_envbg_scratch_floats
    fn.restype = ctypes.c_int64
    assert fn(ctypes.c_int(2), ctypes.c_int(1334), ctypes.c_int(2048)) == 2 * 2 * 3 * 1334 * 2048   # two [B,3,H,W] planes
