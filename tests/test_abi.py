"""CPU: the C-ABI library builds, loads, and exports every symbol include/goliath_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    hdr = open(os.path.join(ROOT, "include", "goliath_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(gol_[a-z0-9_]+)\s*\(", _header())))


def test_library_exports_every_declared_symbol():
    from goliath_amd import build, _lib

    path = build.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    names = _declared()
    assert len(names) >= 9
    for n in names:
        assert hasattr(lib, n), f"{n} declared in goliath_hip.h but not exported"
    # the python binding knows the same set
    assert set(names) == set(_lib.exported_symbols())
    assert b"gfx950" in ctypes.cast(lib.gol_version, ctypes.CFUNCTYPE(ctypes.c_char_p))()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "goliath_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "liboracle" not in src, f


def test_missing_gpu_fails_loudly():
    import pytest
    import torch

    from goliath_amd import sg, splat, _lib

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError):
        sg.evaluate_gaussian(x, torch.ones(1, 4), torch.ones(1, 1, 3), torch.ones(1, 1, 3), x,
                             torch.ones(1, dtype=torch.int32))
    with pytest.raises(_lib.GoliathHipError):
        splat.render_views(torch.zeros(1, 4, 3), torch.ones(1, 4, 3), torch.ones(1, 4, 4), torch.ones(1, 4),
                           torch.ones(1, 4, 3), torch.eye(4)[:3][None], torch.ones(1, 4), 32, 32)


@pytest.mark.parametrize("entry", ["gol_bin_sort", "gol_project_fwd", "gol_project_bwd", "gol_rasterize_fwd",
                                   "gol_rasterize_bwd"])
def test_splat_marshallers_follow_the_header(entry, monkeypatch):
    """splat's marshaller of an entry passes exactly the parameters goliath_hip.h declares, in its order and with its C
    types (the library sets no argtypes: a miscounted or swapped list would reach a kernel as a garbage pointer)."""
    import inspect

    from goliath_amd import _lib, splat

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(splat, "_abi_" + entry[len("gol_"):])
    assert set(inspect.signature(fn).parameters) == {n for _, n in params} - {"block", "stream"}
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "int64_t": (ctypes.c_int64, (1 << 40) + i),
                      "float": (ctypes.c_float, i + 0.5)}[ctype]
        v = {"block": 16, "stream": 0xBEEF}.get(name, v)
        if name not in ("block", "stream"):
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(splat, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)
