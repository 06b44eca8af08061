"""CPU: the public surface of the fused SG prefilter (goliath_amd/envprefilter.py, dropin.patch_env_prefilter, the
gol_envprefilter_* entries) and the composition the GPU tests lean on -- everything that can be checked without a GPU."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import envprefilter_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gol_envprefilter_scratch_floats", "gol_envprefilter_sg")
CTYPES = {"int": ctypes.c_int, "double": ctypes.c_double, "int64_t": ctypes.c_int64}


def _header():
    hdr = open(os.path.join(ROOT, "include", "goliath_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


@pytest.fixture(scope="module")
def golden():
    return np.load(PC.GOLDEN)


def test_entries_are_declared_bound_and_exported():
    from goliath_amd import _lib

    hdr = _header()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", hdr), f"{name} is not declared in goliath_hip.h"
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name)


def test_scratch_is_one_16_byte_texel_per_map_texel():
    from goliath_amd import envprefilter

    assert envprefilter._scratch_floats(2, 33, 70) == 4 * 2 * 33 * 70
    assert envprefilter._scratch_floats(1, 1, 1) == 4
    assert envprefilter._scratch_floats(0, 4, 4) == 0


def test_marshaller_follows_the_header(monkeypatch):
    """envprefilter._abi_envprefilter_sg passes exactly the parameters the header declares, in its order and with its C types."""
    from goliath_amd import _lib, envprefilter

    entry = "gol_envprefilter_sg"
    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header())
    assert decl, f"{entry} is not declared in goliath_hip.h"
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.group(1).split(",")]
    fn = envprefilter._abi_envprefilter_sg
    assert set(inspect.signature(fn).parameters) == {n for _, n in params} - {"stream"}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in inspect.signature(fn).parameters.values())
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        cls, v = (ctypes.c_void_p, 0x10000 * (i + 1)) if "*" in ctype else (CTYPES[ctype], i + 1)
        if name == "stream":
            v = 0xBEEF
        else:
            kw[name] = float(v) if cls is ctypes.c_double else v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(envprefilter, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


def test_bad_arguments_come_back_as_errors():
    """The entry checks before it launches: no GPU is touched by a refused call."""
    from goliath_amd import _lib

    lib = _lib.load()
    fn = lib.gol_envprefilter_sg
    p = ctypes.c_void_p(0x1000)

    def call(B=1, H=2, W=2, He=2, We=2, S=1, sigma=0.2, v=p, env=p, off=0, scratch=p, out=p):
        return fn(ctypes.c_int(B), ctypes.c_int(H), ctypes.c_int(W), ctypes.c_int(He), ctypes.c_int(We), ctypes.c_int(S),
                  ctypes.c_double(sigma), v, env, ctypes.c_void_p(0), ctypes.c_int64(0), ctypes.c_int64(off), scratch, out,
                  ctypes.c_void_p(0))

    null = ctypes.c_void_p(0)
    for bad in (dict(B=0), dict(H=0), dict(We=0), dict(S=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
                dict(sigma=float("inf")), dict(v=null), dict(env=null), dict(scratch=null), dict(out=null), dict(off=-1),
                dict(scratch=ctypes.c_void_p(0x1004)), dict(B=4, H=1 << 15, W=1 << 15), dict(He=1 << 15, We=1 << 15)):
        assert call(**bad) != 0, bad
        assert b"gol_envprefilter_sg" in lib.gol_last_error()


def test_cpu_tensors_raise():
    from goliath_amd import _lib, envprefilter

    v, env = torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 4, 8)
    with pytest.raises(_lib.GoliathHipError):
        envprefilter.prefilter_sg(0.2, v, env, 4)
    with pytest.raises(_lib.GoliathHipError):
        envprefilter.build_pyramid(torch.zeros(3, 16, 32))


def test_inputs_that_require_grad_raise():
    """The forward-only check comes before any device work: it holds for every input and only with grad mode on."""
    from goliath_amd import _lib, envprefilter

    meta = lambda *s, **k: torch.zeros(*s, device="meta", **k)
    for which in range(3):
        t = [meta(1, 3, 2, 2), meta(1, 3, 4, 8), meta(4, 1, 2, 2, 2)]
        t[which].requires_grad_(True)
        with pytest.raises(_lib.GoliathHipError, match="forward-only"):
            envprefilter.prefilter_sg(0.2, t[0], t[1], 4, xi=t[2])
    with pytest.raises(_lib.GoliathHipError, match="forward-only"):
        envprefilter.build_pyramid(meta(3, 16, 32, requires_grad=True))


def test_level_directions_are_the_references_expressions():
    from goliath_amd import envprefilter

    for H, W in ((64, 128), (6, 12), (4, 8)):
        got = envprefilter.level_directions(H, W)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, H, W)
        assert torch.equal(got, PC.level_directions(H, W))
    assert int((envprefilter.level_directions(64, 128)[0, 2] >= 0.999).sum()) == 4


def test_halved_levels_are_the_restated_reference_lines():
    from goliath_amd import envprefilter

    image = PC.pyramid_image()
    for env, (_, _, want) in zip(envprefilter.halved_levels(image, PC.PYR_LEVELS), PC.pyramid_inputs(image)):
        assert torch.equal(env, want)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_float32_composition_is_the_recorded_reference(golden, name):
    """Pins the composition the GPU tests lean on: in float32 on the CPU it is within the reference's own float32 error of
    the reference's recording (it is the same sequence of ATen calls), and the draws are the recorded ones."""
    sigma, v, env, xi = PC.case(name)
    assert PC.checksum(xi) == str(golden[f"{name}/xi_checksum"])
    assert int(golden[f"{name}/near_cut"]) == 0
    got = PC.compose(sigma, v, env, xi, torch.float32)
    err, bar = PC.max_err(got, torch.from_numpy(golden[f"{name}/ref"])), float(golden[f"{name}/err_ref32"])
    print(f"{name}: float32 composition vs recording {err:.3e} (err_ref32 {bar:.3e})")
    assert got.dtype == torch.float32 and err <= bar


def test_float32_composition_is_the_recorded_pyramid(golden):
    image = PC.pyramid_image()
    assert PC.checksum(image) == str(golden["pyramid/checksum"])
    for (i, dirs, env), xi in zip(PC.pyramid_inputs(image), PC.pyramid_draws()):
        got = PC.compose(i * PC.PYR_SIGMA_STEP, dirs, env, xi, torch.float32)
        err, bar = PC.max_err(got, torch.from_numpy(golden[f"pyramid/level{i}"])), float(golden[f"pyramid/err_ref32/level{i}"])
        print(f"pyramid level {i}: {err:.3e} (err_ref32 {bar:.3e})")
        assert err <= bar


def _stub_module():
    seen = []

    def original(sigma, v, env_tex, num_samples=1):
        seen.append((sigma, v, env_tex, num_samples))
        return torch.zeros_like(v)

    return types.SimpleNamespace(prefilterEnvmapSG=original), original, seen


def test_patch_env_prefilter_wraps_once_and_keeps_the_reference():
    from goliath_amd import dropin

    mod, original, _ = _stub_module()
    assert dropin.patch_env_prefilter(mod) is mod
    wrapper = mod.prefilterEnvmapSG
    assert wrapper is not original and wrapper.reference is original
    assert dropin.patch_env_prefilter(mod) is mod
    assert mod.prefilterEnvmapSG is wrapper and wrapper.reference is original       # not wrapped twice
    assert list(inspect.signature(wrapper).parameters) == list(inspect.signature(original).parameters)


def test_patch_env_prefilter_hands_what_it_does_not_take_to_the_original():
    """CPU tensors, float64 and (grad mode on) inputs that require grad reach the recorded original."""
    from goliath_amd import dropin

    mod, _, seen = _stub_module()
    dropin.patch_env_prefilter(mod)
    v, env = torch.ones(1, 3, 2, 2), torch.ones(1, 3, 4, 8)
    for i, (a, b) in enumerate([(v, env), (v.double(), env.double()), (v.clone().requires_grad_(True), env)]):
        out = mod.prefilterEnvmapSG(0.4, a, b, 5)
        assert len(seen) == i + 1 and seen[-1][0] == 0.4 and seen[-1][1] is a and seen[-1][2] is b and seen[-1][3] == 5
        assert tuple(out.shape) == tuple(a.shape)
