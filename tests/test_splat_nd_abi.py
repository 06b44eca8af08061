"""CPU: the N-channel rasterizer's marshallers follow include/goliath_hip.h, and rasterize_gaussians takes C != 3 colours
to the C ABI (no NotImplementedError; without a GPU the ABI layer refuses the CPU tensors)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    hdr = open(os.path.join(ROOT, "include", "goliath_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


@pytest.mark.parametrize("entry", ["gol_rasterize_nd_fwd", "gol_rasterize_nd_bwd"])
def test_nd_marshallers_follow_the_header(entry, monkeypatch):
    """_abi_rasterize_nd_* pass exactly the parameters the header declares, in its order and with its C types."""
    from goliath_amd import _lib, splat

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header())
    assert decl, f"{entry} is not declared in goliath_hip.h"
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.group(1).split(",")]
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


@pytest.mark.parametrize("C", [1, 4, 17])
def test_nd_colours_reach_the_abi(C):
    """C != 3 is no longer refused up front: with a nonzero intersection count (no I < 1 early return) the call goes on to
    the C ABI, which rejects CPU tensors with GoliathHipError.  (The error comes from the first ABI call, gol_bin_sort: this
    only shows that NotImplementedError is gone; test_nd_colours_dispatch_to_the_nd_entries shows which entries run.)"""
    from goliath_amd import _lib, splat

    N = 4
    with pytest.raises(_lib.GoliathHipError):
        splat.rasterize_gaussians(torch.rand(N, 2) * 16, torch.ones(N), torch.ones(N, dtype=torch.int32),
                                  torch.tensor([[1.0, 0.0, 1.0]]).repeat(N, 1), torch.ones(N, dtype=torch.int32),
                                  torch.rand(N, C), torch.full((N, 1), 0.5), 16, 16, 16)


@pytest.mark.parametrize("C", [1, 3, 5, 12, 17])
def test_nd_colours_dispatch_to_the_nd_entries(C, monkeypatch):
    """C != 3 runs gol_rasterize_nd_fwd / _bwd with this C (forward and backward), C == 3 the 3-channel entries: the
    binning, packing and marshallers are replaced by recorders, so this runs without a GPU."""
    from goliath_amd import splat

    calls = []
    monkeypatch.setattr(splat, "_bin_sort", lambda *a, **k: None)
    monkeypatch.setattr(splat, "_pack_records", lambda B, N, xys, conics, colors, extra, opac: (
        calls.append(("pack", colors is None)) or torch.zeros(B, N, splat.SPLAT_RECORD)))
    for name in ("rasterize_fwd", "rasterize_bwd", "rasterize_nd_fwd", "rasterize_nd_bwd"):
        monkeypatch.setattr(splat, "_abi_" + name, lambda _n=name, **kw: calls.append((_n, kw.get("C"))))
    N = 4
    xys = (torch.rand(N, 2) * 16).requires_grad_(True)
    colors = torch.rand(N, C).requires_grad_(True)
    img = splat.rasterize_gaussians(xys, torch.ones(N), torch.ones(N, dtype=torch.int32),
                                    torch.tensor([[1.0, 0.0, 1.0]]).repeat(N, 1), torch.ones(N, dtype=torch.int32),
                                    colors, torch.full((N, 1), 0.5), 16, 16, 16)
    assert img.shape == (16, 16, C)
    img.sum().backward()
    if C == 3:
        assert calls == [("pack", False), ("rasterize_fwd", None), ("rasterize_bwd", None)]
    else:
        assert calls == [("pack", True), ("rasterize_nd_fwd", C), ("rasterize_nd_bwd", C)]
