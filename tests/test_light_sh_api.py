"""CPU: the public surface of the fused light path (goliath_amd/lights.py, dropin.patch_sh, the gol_sh_* / gol_light_sh_fwd
entries) -- everything that can be checked without a GPU."""
import ctypes
import inspect
import math
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gol_sh_norm_constants", "gol_sh_basis_fwd", "gol_light_sh_fwd")


def _header():
    hdr = open(os.path.join(ROOT, "include", "goliath_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_norm_constants_are_the_closed_form():
    """sqrt((2n + 1) / (4 pi) (n - |m|)! / (n + |m|)!), times sqrt 2 for m != 0, in the reference's order.  Both sides take
    one square root of a product of a few correctly rounded factors (and one more rounding for the sqrt 2): 8 eps covers it."""
    from goliath_amd import lights

    k = lights.sh_norm_constants(8)
    assert k.dtype == torch.float64 and tuple(k.shape) == (81,)
    want = []
    for n in range(9):
        for m in range(-n, n + 1):
            v = math.sqrt((2 * n + 1) / (4 * math.pi) * math.factorial(n - abs(m)) / math.factorial(n + abs(m)))
            want.append(v * math.sqrt(2.0) if m else v)
    want = torch.tensor(want, dtype=torch.float64)
    assert bool(((k - want).abs() <= 8 * torch.finfo(torch.float64).eps * want).all())
    for deg in (0, 1, 2, 5):   # a lower degree is a prefix
        assert torch.equal(lights.sh_norm_constants(deg), k[:(deg + 1) ** 2])


def test_norm_constants_is_the_librarys_vector():
    from goliath_amd import _lib, lights

    buf = (ctypes.c_double * 81)()
    assert _lib.load().gol_sh_norm_constants(ctypes.c_int(8), buf) == 0
    assert torch.equal(lights.sh_norm_constants(8), torch.tensor(list(buf), dtype=torch.float64))
    assert _lib.load().gol_sh_norm_constants(ctypes.c_int(9), buf) != 0


def test_entries_are_declared_bound_and_exported():
    from goliath_amd import _lib

    hdr = _header()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in goliath_hip.h"
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name)


@pytest.mark.parametrize("entry", ["gol_sh_basis_fwd", "gol_light_sh_fwd"])
def test_marshallers_follow_the_header(entry, monkeypatch):
    """lights._abi_* pass exactly the parameters the header declares, in its order and with its C types."""
    from goliath_amd import _lib, lights

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header())
    assert decl, f"{entry} is not declared in goliath_hip.h"
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.group(1).split(",")]
    fn = getattr(lights, "_abi_" + entry[len("gol_"):])
    assert set(inspect.signature(fn).parameters) == {n for _, n in params} - {"stream"}
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        cls, v = (ctypes.c_void_p, 0x10000 * (i + 1)) if "*" in ctype else {"int": (ctypes.c_int, i + 1)}[ctype]
        if name == "stream":
            v = 0xBEEF
        else:
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(lights, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


def test_cpu_tensors_raise():
    from goliath_amd import _lib, lights

    with pytest.raises(_lib.GoliathHipError):
        lights.dir2sh(8, torch.zeros(4, 3))
    with pytest.raises(_lib.GoliathHipError):
        lights.headrel_light_sh(torch.zeros(1, 2, 3), torch.ones(1, 2, 1), torch.eye(4)[:3][None], 8)
    with pytest.raises(_lib.GoliathHipError):
        lights.headrel_light_sh(torch.zeros(1, 2, 3), torch.ones(1, 2, 3), None, 8)
    with pytest.raises(_lib.GoliathHipError):
        lights.random_light_sh(8, 2, "cpu", torch.float32)


def test_degree_nine_is_a_value_error():
    from goliath_amd import lights

    with pytest.raises(ValueError):
        lights.sh_norm_constants(9)
    with pytest.raises(ValueError):
        lights.dir2sh(9, torch.zeros(4, 3))
    with pytest.raises(ValueError):
        lights.headrel_light_sh(torch.zeros(1, 2, 3), torch.ones(1, 2, 1), None, 9)
    with pytest.raises(ValueError):
        lights.random_light_sh(9, 2, "cpu", torch.float32)
    with pytest.raises(ValueError):
        lights.dir2sh(-1, torch.zeros(4, 3))


def _stub_modules():
    seen = []

    def original(deg, dirs):
        seen.append((deg, dirs))
        return torch.zeros(*dirs.shape[:-1], (deg + 1) ** 2, dtype=dirs.dtype)

    class AutoEncoder:
        pass

    class PrimDecoder:
        pass

    return types.SimpleNamespace(dir2sh_torch=original), types.SimpleNamespace(AutoEncoder=AutoEncoder,
                                                                                PrimDecoder=PrimDecoder), original, seen


def test_patch_sh_sets_the_flags_and_wraps_once():
    from goliath_amd import dropin, rgca

    sh, mod, original, _ = _stub_modules()
    for cls in (mod.AutoEncoder, mod.PrimDecoder):
        assert getattr(cls(), rgca.LIGHT_SH_FLAG, False) is False
    assert dropin.patch_sh(sh, mod) == (sh, mod)
    for cls in (mod.AutoEncoder, mod.PrimDecoder):
        assert getattr(cls(), rgca.LIGHT_SH_FLAG) is True
    wrapper = sh.dir2sh_torch
    assert wrapper is not original and wrapper.reference is original
    before = [dict(vars(c)) for c in (mod.AutoEncoder, mod.PrimDecoder)]
    assert dropin.patch_sh(sh, mod) == (sh, mod)
    assert sh.dir2sh_torch is wrapper and wrapper.reference is original       # not wrapped twice
    assert [dict(vars(c)) for c in (mod.AutoEncoder, mod.PrimDecoder)] == before


def test_patch_sh_wrapper_hands_what_it_does_not_take_to_the_original():
    """CPU tensors, float64 and (grad mode on) directions that require grad reach the recorded original; so does deg = 9."""
    from goliath_amd import dropin

    sh, mod, _, seen = _stub_modules()
    dropin.patch_sh(sh, mod)
    cpu = torch.ones(2, 5, 3)
    f64 = torch.ones(4, 3, dtype=torch.float64)
    grad = torch.ones(4, 3, requires_grad=True)
    for i, (deg, d) in enumerate([(8, cpu), (2, f64), (8, grad), (9, cpu)]):
        out = sh.dir2sh_torch(deg, d)
        assert len(seen) == i + 1 and seen[-1][0] == deg and seen[-1][1] is d
        assert tuple(out.shape) == (*d.shape[:-1], (deg + 1) ** 2)
