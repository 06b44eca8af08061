"""CPU: the public surface of the primitive assembly (goliath_amd/mvpprims.py, dropin.patch_hand_mvp, the gol_mvp_template_* /
gol_mvp_primtransf_* entries) and the restatements of tests/mvpprims_cases.py against the reference's own code -- everything
that can be checked without a GPU."""
import ctypes
import inspect
import os
import re
import sys
import types

import pytest
import torch

import mvpprims_cases as C
from test_dropin_real_classes import REF   # where the reference tree lies, when it exists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gol_mvp_template_fwd", "gol_mvp_template_bwd", "gol_mvp_primtransf_fwd", "gol_mvp_primtransf_bwd")
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")


def _header():
    hdr = open(os.path.join(ROOT, "include", "goliath_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_entries_are_declared_bound_and_exported():
    from goliath_amd import _lib

    hdr = _header()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in goliath_hip.h"
        assert name in _lib.exported_symbols()
        assert hasattr(lib, name)


@pytest.mark.parametrize("entry", ENTRIES)
def test_marshallers_follow_the_header(entry, monkeypatch):
    """mvpprims._abi_* pass exactly the parameters the header declares, in its order and with its C types."""
    from goliath_amd import _lib, mvpprims

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header())
    assert decl, f"{entry} is not declared in goliath_hip.h"
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.group(1).split(",")]
    fn = getattr(mvpprims, "_abi_" + entry[len("gol_"):])
    assert set(inspect.signature(fn).parameters) == {n for _, n in params} - {"stream"}
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        cls, v = (ctypes.c_void_p, 0x10000 * (i + 1)) if "*" in ctype else {"int": (ctypes.c_int, i + 1),
                                                                            "float": (ctypes.c_float, i + 0.5)}[ctype]
        if name == "stream":
            v = 0xBEEF
        else:
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(mvpprims, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


@pytest.mark.parametrize("name", C.MASKS)
@pytest.mark.parametrize("dtype", [torch.bool, torch.float32])
def test_prim_slots(name, dtype):
    from goliath_amd import mvpprims

    K = 8
    mask = C.mask_of(name, K)
    m = mask.to(dtype)
    slot, live, Kv = mvpprims.prim_slots(m, compact=True)
    assert slot.dtype == torch.int32 and live is None and Kv == int(mask.sum())
    want = [-1] * K
    for j, k in enumerate(torch.nonzero(mask)[:, 0].tolist()):
        want[k] = j
    assert slot.tolist() == want
    slot, live, Kv = mvpprims.prim_slots(m, compact=False)
    assert slot.tolist() == list(range(K)) and live.dtype == torch.int32 and live.tolist() == mask.int().tolist() and Kv == K


def test_prim_slots_are_cached_per_mask_and_follow_writes():
    from goliath_amd import mvpprims

    m = C.mask_of("ends", 8)
    a = mvpprims.prim_slots(m)
    assert mvpprims.prim_slots(m)[0] is a[0]                       # the same tables, not rebuilt
    assert mvpprims.prim_slots(m, compact=False)[0] is not a[0]
    m[0] = True                                                     # an in-place write bumps the version counter
    b = mvpprims.prim_slots(m)
    assert b[2] == 7 and b[0].tolist() == [0, 1, 2, 3, 4, 5, 6, -1]
    other = m.clone()
    assert mvpprims.prim_slots(other)[0] is not b[0]
    with pytest.raises(ValueError):
        mvpprims.prim_slots(torch.ones(2, 4, dtype=torch.bool))


def test_shape_and_dtype_errors_raise_before_any_library_call(monkeypatch):
    from goliath_amd import _lib, mvpprims

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "call", boom)
    (TW, TH, TD), (ny, nx), B = C.TEMPLATE_SHAPES[2]
    rgb, alpha = C.slabs(C.TEMPLATE_SHAPES[2])
    ps = (TW, TH, TD)
    with pytest.raises(ValueError):
        mvpprims.assemble_template(rgb, alpha, (TW, TH, TD + 1))              # depth does not match
    with pytest.raises(ValueError):
        mvpprims.assemble_template(rgb, alpha, (3, TH, TD))                   # the slab does not tile
    with pytest.raises(ValueError):
        mvpprims.assemble_template(rgb[:, :, :2], alpha, ps)                  # two colour planes
    with pytest.raises(ValueError):
        mvpprims.assemble_template(rgb.double(), alpha, ps)                   # mixed dtypes
    with pytest.raises(ValueError):
        mvpprims.assemble_template(None, alpha.long(), ps)                    # integer slab
    with pytest.raises(ValueError):
        mvpprims.assemble_template(rgb, alpha, ps, valid_prims=torch.ones(ny * nx + 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        mvpprims.assemble_template(rgb, alpha, ps, rgb_affine=(1.0,))
    with pytest.raises(ValueError):
        mvpprims.assemble_template(rgb, alpha[:, :, 0, 0], ps)                # not a slab
    t = {k: v.float() for k, v in C.transform_inputs(1, 4).items()}
    for key, bad in (("posbase", t["posbase"][:, :3]), ("rotbase", t["rotbase"].reshape(1, 4, 9)),
                     ("delta_rvec", t["delta_rvec"][..., :2]), ("delta_scale", t["delta_scale"].long()),
                     ("delta_pos", t["delta_pos"][0])):
        with pytest.raises(ValueError):
            mvpprims.prim_transforms(**dict(t, **{key: bad}), prim_scale=512.0)
    with pytest.raises(ValueError):
        mvpprims.prim_transforms(**dict(t, posbase=t["posbase"].clone().requires_grad_(True)), prim_scale=512.0)


def test_missing_gpu_fails_loudly():
    from goliath_amd import _lib, mvpprims

    rgb, alpha = C.slabs(C.TEMPLATE_SHAPES[2])
    ps = C.TEMPLATE_SHAPES[2][0]
    with pytest.raises(_lib.GoliathHipError):
        mvpprims.assemble_template(rgb, alpha, ps)
    with pytest.raises(_lib.GoliathHipError):
        mvpprims.assemble_template(None, alpha, ps, valid_prims=C.mask_of("ends", 8), compact=False)
    t = {k: v.float() for k, v in C.transform_inputs(1, 4).items()}
    with pytest.raises(_lib.GoliathHipError):
        mvpprims.prim_transforms(**t, prim_scale=512.0)


def test_template_entries_reject_bad_arguments_without_a_gpu():
    """The argument checks of the C entries come before any HIP call."""
    from goliath_amd import _lib

    lib = _lib.load()
    i, f, null = ctypes.c_int, ctypes.c_float, ctypes.c_void_p(0)
    odd = ctypes.c_void_p(0x1004)
    # a slot table is missing although Kout != K; a template that is not 16-byte aligned
    assert lib.gol_mvp_template_fwd(i(1), i(2), i(2), i(4), i(2), i(2), null, odd, null, null, i(3), i(0), f(1), f(0), null,
                                    null, null) != 0
    assert b"gol_mvp_template_fwd" in lib.gol_last_error()
    assert lib.gol_mvp_template_fwd(i(1), i(2), i(2), i(4), i(2), i(2), null, odd, null, null, i(4), i(0), f(1), f(0), odd,
                                    null, null) != 0
    assert lib.gol_mvp_template_bwd(i(1), i(2), i(2), i(4), i(2), i(2), null, null, null, null, i(4), i(1), f(1), f(0), null,
                                    null, null, odd, null) != 0            # the activation's mask needs the input
    assert lib.gol_mvp_primtransf_fwd(i(1), i(4), null, null, null, null, null, f(1), null, null, null, null) != 0
    assert lib.gol_mvp_primtransf_bwd(i(-1), i(4), null, null, f(1), null, null, null, null, null, null, null) != 0
    # nothing to do is not an error
    assert lib.gol_mvp_template_fwd(i(0), i(2), i(2), i(4), i(2), i(2), null, null, null, null, i(4), i(0), f(1), f(0), null,
                                    null, null) == 0
    assert lib.gol_mvp_primtransf_fwd(i(2), i(0), null, null, null, null, null, f(1), null, null, null, null) == 0


def _stub_module():
    class AutoEncoder:
        def render(self, K, Rt, preds, with_shadow=False):
            return "reference"

    class GeomDecoder:
        def forward(self, pose, joint, iteration=-1):
            return "reference"

    return types.SimpleNamespace(AutoEncoder=AutoEncoder, GeomDecoder=GeomDecoder)


def test_patch_hand_mvp_installs_both_functions_and_the_flag():
    from goliath_amd import dropin, mvpprims

    mod = _stub_module()
    assert dropin.patch_hand_mvp(mod) is mod
    assert mod.AutoEncoder.render is mvpprims.hand_mvp_render and mod.GeomDecoder.forward is mvpprims.geom_decoder_forward
    assert getattr(mod.AutoEncoder(), mvpprims.FULL_TEMPLATE_FLAG) is False
    assert dropin.patch_hand_mvp(mod, full_template=True) is mod
    assert getattr(mod.AutoEncoder(), mvpprims.FULL_TEMPLATE_FLAG) is True


# ------------------------------------------------------------------------------------------- against the reference's code
@pytest.fixture(scope="module")
def ref_mvp():
    """ca_code.models.hand_mvp and ca_code.utils.render_raymarcher, imported unchanged (native / third-party imports
    stubbed, tests/golden/ref_stubs.py)."""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import ref_stubs

    ref_stubs.install()
    for n in ("sgutilslib", "utilslib", "mvpraymarchlib"):
        sys.modules.setdefault(n, types.ModuleType(n))
    import ca_code.models.hand_mvp as M
    import ca_code.utils.render_raymarcher as RM

    return types.SimpleNamespace(M=M, RM=RM)


def _params(fn):
    return [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]


@needs_ref
def test_patched_methods_keep_the_reference_parameter_lists(ref_mvp):
    from goliath_amd import dropin, mvpprims

    M = ref_mvp.M
    saved = (M.AutoEncoder.render, M.GeomDecoder.forward)
    had_flag = mvpprims.FULL_TEMPLATE_FLAG in vars(M.AutoEncoder)
    try:
        assert dropin.patch_hand_mvp(M) is M
        assert M.AutoEncoder.render is mvpprims.hand_mvp_render and M.GeomDecoder.forward is mvpprims.geom_decoder_forward
        assert _params(M.AutoEncoder.render) == _params(saved[0])
        assert _params(M.GeomDecoder.forward) == _params(saved[1])
    finally:
        M.AutoEncoder.render, M.GeomDecoder.forward = saved
        if not had_flag:
            delattr(M.AutoEncoder, mvpprims.FULL_TEMPLATE_FLAG)


@needs_ref
def test_rotation_restatement_equals_the_references_axisangle_to_matrix(ref_mvp):
    t = C.transform_inputs(2, 130)
    r = t["delta_rvec"]
    want = ref_mvp.M.axisangle_to_matrix(r)
    got = C.rotation_of(r)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12
    # ... and the tail, with the reference's own lines (hand_mvp.py:417-425)
    B = r.shape[0]
    primpos = t["posbase"] + torch.bmm(t["rotbase"].view(-1, 3, 3), t["delta_pos"].view(-1, 3, 1)).reshape(B, -1, 3)
    primrot = torch.bmm(t["rotbase"].view(-1, 3, 3), want.view(-1, 3, 3)).view(B, -1, 3, 3)
    mine = C.transform_tail(**t, prim_scale=512)
    for a, b in zip(mine, (primpos, primrot, 512 * t["delta_scale"])):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@needs_ref
@pytest.mark.parametrize("shape", C.TEMPLATE_SHAPES)
@pytest.mark.parametrize("mask", C.MASKS)
def test_template_restatement_equals_the_references_render_and_raymarcher(ref_mvp, shape, mask, monkeypatch):
    """AutoEncoder.render's rearrangement (run on a stand-in `self`) and Raymarcher.forward's filtering (the real class,
    its march recorded instead of run), on CPU: exact."""
    (TW, TH, TD), (ny, nx), B = shape
    K = ny * nx
    rgb, alpha = C.slabs(shape, dtype=torch.float64)
    valid = C.mask_of(mask, K)
    seen = {}

    def record(raypos, raydir, dt, tminmax, primtransf, template=None, **kw):
        seen.update(primtransf=primtransf, template=template)
        return torch.zeros(B, 2, 3, 4)

    monkeypatch.setattr(ref_mvp.RM, "mvpraymarch", record)
    monkeypatch.setattr(ref_mvp.M, "compute_raydirs", lambda *a: (torch.zeros(B, 2, 3, 3), torch.zeros(B, 2, 3, 3),
                                                                 torch.zeros(B, 2, 3, 2)))
    me = types.SimpleNamespace(primsize=(TW, TH, TD), n_prim_x=nx, n_prim_y=ny, n_prims=K, pixel_coords=torch.zeros(2, 3, 2),
                               raymarcher=ref_mvp.RM.Raymarcher(volradius=4.0))
    g = torch.Generator().manual_seed(1)
    preds = dict(primrgb=rgb, primalpha=alpha, valid_prims=valid, primpos=torch.randn(B, K, 3, generator=g),
                 primrot=torch.randn(B, K, 3, 3, generator=g), primscale=torch.randn(B, K, 3, generator=g))
    Kc, Rt = torch.eye(3)[None].repeat(B, 1, 1), torch.eye(4)[None, :3].repeat(B, 1, 1)
    ref_mvp.M.AutoEncoder.render(me, Kc, Rt, preds)
    full = C.slab_template(rgb, alpha, (TW, TH, TD), ny, nx)
    assert torch.equal(preds["primrgba"], full)
    assert torch.equal(seen["template"], C.keep_valid(full, valid))
    for got, name in zip(seen["primtransf"], ("primpos", "primrot", "primscale")):
        src = preds[name] / 4.0 if name == "primpos" else preds[name]
        assert torch.equal(got, C.keep_valid(src, valid))
    # the one-channel variant and the teacher's masking (hand_teacher_mvp.py:305-311, restated there from the same lines)
    a1 = alpha.reshape(B, TD, 1, ny, TH, nx, TW).permute(0, 3, 5, 1, 4, 6, 2).reshape(B, K, TD, TH, TW)
    assert torch.equal(C.slab_template(None, alpha, (TW, TH, TD), ny, nx), a1)
    assert torch.equal(C.zero_invalid(a1, valid), valid[None, :, None, None, None] * a1)
