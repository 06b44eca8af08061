"""CPU: the env-relight driver (goliath_amd/envdriver.py, dropin.patch_env_driver, gol_envspin_frame, the device mip scale
of gol_shade_in) -- everything that can be checked without a GPU.  Cases and the float64 composition: envdriver_cases.py;
the recorded reference results: tests/golden/env_driver_golden.npz (make_env_driver_golden.py)."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import envdriver_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(EC.GOLDEN)


def _calls():
    return [(name, tag) for name in EC.images() for tag, _ in EC.batches()]


def test_images_are_the_recorded_ones(golden):
    for name, image in EC.images().items():
        assert EC.checksum(image) == str(golden[f"{name}/checksum"]), name
        assert np.float32(np.percentile(image.numpy(), 90)) == golden[f"{name}/perc90"]
    assert EC.checksum(EC.full_image()) == str(golden["full/checksum"])


@pytest.mark.parametrize("name,tag", _calls())
def test_float64_composition_against_the_recorded_reference(golden, name, tag):
    """Our float64 statement of the formulas is what the reference computes: within 1 x the reference's own float32 error
    (the error IS the distance between the two, recorded over the whole arrays; this recomputes it on another machine)."""
    image = EC.images()[name]
    _, H, W = image.shape
    key = f"{name}/{tag}"
    rot = torch.from_numpy(golden[f"{key}/rot"])
    want = EC.compose64(image, rot, golden[f"{name}/perc90"])
    slack = 1.0 + 1e-6    # float64 libm differences between machines
    for b in range(rot.shape[0]):
        rec = torch.from_numpy(golden[f"{key}/envbg"][b])
        assert EC.max_err(rec, want["envbg"][b][:, EC.recorded_rows(H, W, b)]) <= slack * float(golden[f"{key}/err_ref32/envbg"])
    envmap = torch.from_numpy(golden[f"{key}/envmap"])
    assert EC.max_err(envmap, want["envmap"]) <= slack * float(golden[f"{key}/err_ref32/envmap"])
    assert EC.max_err(envmap.reshape(len(rot), 3, -1).transpose(1, 2), want["light_intensity"]) <= \
        slack * float(golden[f"{key}/err_ref32/light_intensity"])
    for k in ("norm_scale", "mip_scale"):
        assert EC.max_err(torch.from_numpy(golden[f"{key}/{k}"]), want[k]) <= slack * float(golden[f"{key}/err_ref32/{k}"]) + 1e-18


@pytest.mark.parametrize("H,W", [(512, 1024), (48, 96), (40, 72), (33, 70), (16, 32)])
def test_tap_tables_reproduce_the_antialiased_interpolate(H, W):
    from goliath_amd import envdriver

    ys, yw, xs, xw = envdriver.tap_tables(H, W)
    assert ys.dtype == torch.int32 and yw.dtype == torch.float64 and tuple(ys.shape) == (16,) and tuple(xs.shape) == (32,)
    assert int(ys.min()) >= 0 and int(xs.min()) >= 0
    for start, w, n in ((ys, yw, H), (xs, xw, W)):   # every non-zero weight addresses a row / column of the map
        last = torch.tensor([int(torch.nonzero(r).max()) for r in w])
        assert bool((start + last < n).all())
    if (H, W) == (512, 1024):
        assert (yw.shape[1], xw.shape[1]) == (64, 64)
    if (H, W) == (16, 32):
        assert (yw.shape[1], xw.shape[1]) == (1, 1) and bool((yw == 1).all()) and bool((xw == 1).all())
    x = torch.rand(3, H, W, generator=torch.Generator().manual_seed(H), dtype=torch.float64)
    want = F.interpolate(x[None], (16, 32), mode="bilinear", antialias=True)[0]
    my, mx = torch.zeros(16, H, dtype=torch.float64), torch.zeros(32, W, dtype=torch.float64)
    for i in range(16):
        n = min(yw.shape[1], H - int(ys[i]))
        my[i, int(ys[i]):int(ys[i]) + n] = yw[i, :n]
    for j in range(32):
        n = min(xw.shape[1], W - int(xs[j]))
        mx[j, int(xs[j]):int(xs[j]) + n] = xw[j, :n]
    got = torch.einsum("ia,cab,jb->cij", my, x, mx)
    assert float((got - want).abs().max()) <= 1e-6 * float(x.max())


def test_spin_lightrot_against_the_recorded_rotations(golden):
    """<= 5e-7 per entry: entries are <= 1, at most three float32 roundings of values <= 1, sinf / cosf within 2 ulp."""
    from goliath_amd import envdriver

    for tag, indices in EC.batches():
        if indices is None:
            continue
        want = torch.from_numpy(golden[f"16x32/{tag}/rot"])
        for index in (indices, torch.tensor(indices)):
            got = envdriver.spin_lightrot(index, EC.CYCLE, "cpu")
            assert got.dtype == torch.float32 and tuple(got.shape) == (len(indices), 3, 3)
            assert float((got - want).abs().max()) <= 5e-7
    for index in ([0], torch.tensor([0]), [0, 0]):
        got = envdriver.spin_lightrot(index, EC.CYCLE, "cpu")
        assert torch.equal(got, torch.eye(3).expand_as(got))          # bitwise the identity (no -0 either)
        assert not bool(torch.signbit(got).any())
    with pytest.raises(ValueError):
        envdriver.spin_lightrot(torch.zeros(2, 2), EC.CYCLE, "cpu")


def test_argument_errors():
    from goliath_amd import _lib, envdriver

    image = EC.images()["16x32"]
    with pytest.raises(_lib.GoliathHipError):
        envdriver.EnvSpin(image, EC.ENV_SCALE, device="cpu")
    for bad in (torch.zeros(16, 32), torch.zeros(1, 16, 32), torch.zeros(3, 15, 32), torch.zeros(3, 16, 30), torch.zeros(3, 16, 33)):
        with pytest.raises(ValueError):
            envdriver.EnvSpin(bad, EC.ENV_SCALE, device="cpu")
    with pytest.raises(ValueError):
        envdriver.EnvSpin(image, EC.ENV_SCALE, perc90=0.0, device="cuda")
    with pytest.raises(ValueError):
        envdriver.tap_tables(16, 31)
    # frame(): the argument checks come before anything touches the device
    spin = object.__new__(envdriver.EnvSpin)
    spin.cycle, spin.device = EC.CYCLE, torch.device("cuda")
    with pytest.raises(ValueError):
        spin.frame()
    with pytest.raises(ValueError):
        spin.frame(index=[0], lightrot=torch.eye(3)[None])
    with pytest.raises(ValueError):
        spin.frame(lightrot=torch.eye(3))
    with pytest.raises(_lib.GoliathHipError):
        spin.frame(lightrot=torch.eye(3)[None])                      # a CPU tensor
    with pytest.raises(_lib.GoliathHipError):
        spin.frame(index=torch.zeros(2, requires_grad=True))


def _header():
    hdr = open(os.path.join(ROOT, "include", "goliath_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_entries_are_declared_bound_and_exported():
    from goliath_amd import _lib

    lib = _lib.load()
    for name in ("gol_envspin_scratch_floats", "gol_envspin_frame"):
        assert re.search(r"\b" + name + r"\s*\(", _header()), f"{name} is not declared in goliath_hip.h"
        assert name in _lib.exported_symbols() and hasattr(lib, name)
    fn = lib.gol_envspin_scratch_floats
    fn.restype = ctypes.c_int64
    assert fn(ctypes.c_int(2), ctypes.c_int(512), ctypes.c_int(1024)) >= 2 * 3 * 512 * 1024
    assert fn(ctypes.c_int(0), ctypes.c_int(512), ctypes.c_int(1024)) == 0


def test_bad_sizes_are_status_errors():
    """H >= 16, W >= 32, W even: checked before any pointer is looked at (no GPU needed)."""
    from goliath_amd import _lib

    lib = _lib.load()
    null = ctypes.c_void_p(0)
    for H, W in ((15, 32), (16, 30), (16, 33)):
        rc = lib.gol_envspin_frame(ctypes.c_int(1), ctypes.c_int(H), ctypes.c_int(W), null, null, null, null, ctypes.c_int(1),
                                   null, null, ctypes.c_int(1), ctypes.c_float(1.0), ctypes.c_double(18.0), null, null, null,
                                   null, null, null, null)
        assert rc != 0 and b"gol_envspin_frame" in lib.gol_last_error()


def test_marshaller_follows_the_header(monkeypatch):
    """envdriver._abi_envspin_frame passes exactly the parameters the header declares, in its order and with its C types."""
    from goliath_amd import _lib, envdriver

    decl = re.search(r"\bint\s+gol_envspin_frame\s*\(([^)]*)\)", _header())
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.group(1).split(",")]
    fn = envdriver._abi_envspin_frame
    assert set(inspect.signature(fn).parameters) == {n for _, n in params} - {"stream"}
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "float": (ctypes.c_float, i + 0.5), "double": (ctypes.c_double, i + 0.25)}[ctype]
        if name == "stream":
            v = 0xBEEF
        else:
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(envdriver, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == "gol_envspin_frame"
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


def test_shade_in_layout_ends_with_the_device_scale():
    from goliath_amd import shade

    fields = list(shade.ShadeIn._fields_)
    assert fields[-1] == ("mips_scale_dev", ctypes.c_void_p) and fields[-2][0] == "mips_scale"

    class Old(ctypes.Structure):
        _fields_ = fields[:-1]

    assert ctypes.sizeof(shade.ShadeIn) == ctypes.sizeof(Old) + 8
    assert shade.ShadeIn.mips_scale_dev.offset == ctypes.sizeof(Old)
    assert shade.ShadeIn().mips_scale_dev is None                     # NULL by default: the host float decides
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\}\s*gol_shade_in;", _header(), flags=re.S).group(1)
    assert re.search(r"const\s+float\s*\*\s*mips_scale_dev\s*;\s*$", body.strip())


def test_shared_mipmap_keeps_a_float_scale_a_float():
    """A float (or CPU tensor) scale behaves exactly as before; only a CUDA tensor stays a tensor (checked on the GPU)."""
    from goliath_amd import dropin

    holder = types.SimpleNamespace(miplevel=2, mipmap_0=torch.rand(1, 3, 16, 32), mipmap_1=torch.rand(1, 3, 8, 16))
    for scale in (2.5, torch.tensor(2.5)):
        for m in dropin._shared_mipmap(holder, 3, "cpu", scale):
            assert type(m._gol_scale) is float and m._gol_scale == 2.5 and m.stride(0) == 0


def test_patch_env_driver_wraps_once_and_keeps_the_reference():
    from goliath_amd import dropin

    def original(self, **data):
        return ("reference", data)

    class EnvSpinDecorator:
        forward = original

    mod = types.SimpleNamespace(EnvSpinDecorator=EnvSpinDecorator)
    assert dropin.patch_env_driver(mod) is mod
    wrapper = EnvSpinDecorator.forward
    assert wrapper is not original and wrapper.reference is original
    assert dropin.patch_env_driver(mod) is mod and EnvSpinDecorator.forward is wrapper      # not wrapped twice
    # a decorator on the CPU (no GPU path) stays on the reference
    d = EnvSpinDecorator()
    d.image, d.env_scale, d.cycle, d.envmap_dist = EC.images()["16x32"], EC.ENV_SCALE, EC.CYCLE, EC.ENVMAP_DIST
    out = d.forward(campos=torch.zeros(1, 3), index=[3])
    assert out[0] == "reference" and out[1]["index"] == [3]
