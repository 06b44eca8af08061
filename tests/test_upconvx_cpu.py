"""CPU: the arithmetic of the split-bf16 texture-decoder layer (goliath_amd.texdec.upconv_*_split_torch, the twins of
gol_upconvx_*) against plain float64 on the cases of tests/upconvx_cases.py, the twins' autograd against the written-out
products, that the bar discriminates, the sign condition, the region bound of the input gradient's tile, the routing of
`texture_branches(..., precision=...)`, the drop-in keyword and the marshallers against the header."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import upconvx_cases as uc
from upconvx_cases import BAR, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gol_upconvx_pack", "gol_upconvx_fwd", "gol_upconvx_bwd_x", "gol_upconvx_bwd_w", "gol_upconvx_bwd_gate")
QUERIES = {"gol_upconvx_packed_elems": ["int Co", "int Ci"],
           "gol_upconvx_bwd_w_scratch_floats": ["int B", "int Ci", "int Co", "int Hi", "int Wi"]}
CONV_KEYS = ("y", "g_x", "g_w", "g_gate")        # the keys with a split product in them
STREAM_KEYS = ("g_bias", "g_gb")                 # sums / copies of the SAME float32 values on both sides


@pytest.mark.parametrize("i,variant", uc.PARAMS, ids=uc.PARAM_IDS)
def test_split_twin_against_float64(i, variant):
    """The float64-accumulated twin's y and every gradient are <= 1e-5 rel-L2 from plain float64 (U and the convolution in
    float64; mode 0 under the float64 reference's sign mask), every element of the products is within 3.1 2^-16 sum |a||b|,
    and g_bias / g_gb -- the SAME float32 values on both sides -- are equal to rounding."""
    ref = uc.reference(i, variant)
    for k in uc.keys(variant):
        e = rel_l2(ref[k], ref[k + "64"])
        print(uc.IDS[i], variant, k, "rel-L2 %.3e" % e)
        assert ref[k].dtype == torch.float64 and ref[k].shape == ref[k + "64"].shape and float(ref[k + "64"].abs().max()) > 0
        assert e <= BAR, (k, e)
        if k in STREAM_KEYS:
            assert e <= 1e-7, e
        else:
            assert bool(((ref[k] - ref[k + "64"]).abs() <= uc.ELEMENT_BOUND * ref["m_" + k]).all()), k


@pytest.mark.parametrize("i", range(len(uc.CASES)), ids=uc.IDS)
def test_signs_differ_from_float64_only_next_to_zero(i):
    """Mode 0: the twin's sign of y in float32 accumulation differs from float64's only where |pre64| < 1e-5 rms(pre64) and at
    no more than 0.1 % of the elements; float32 library accumulation alone stays within the same cap on these draws; and
    fewer elements lie that near zero than the cap, so the GPU test's cap can be met."""
    from goliath_amd import texdec

    inp = uc.inputs(i)
    pos64 = uc.forward64(i, "lrelu")["pre"] > 0
    near = uc.near_zero(i)
    y32 = texdec.upconv_lrelu_split_torch(inp["x"], inp["w"], inp["bias"], uc.LEAK, acc_dtype=torch.float32)
    lib32 = F.conv2d(uc.up64(inp["x"]), inp["w"], None, 1, 1) + inp["bias"][None]
    assert y32.dtype == torch.float32
    differs, differs_lib = (y32 > 0) != pos64, (lib32 > 0) != pos64
    print(uc.IDS[i], int(differs.sum()), "twin signs differ,", int(differs_lib.sum()), "library signs differ,",
          int(near.sum()), "elements near zero, of", near.numel())
    assert not bool((differs & ~near).any())
    cap = uc.SIGN_CAP * near.numel()
    assert int(differs.sum()) <= cap and int(differs_lib.sum()) <= cap and int(near.sum()) <= cap


@pytest.mark.parametrize("i,variant", [(0, "lrelu"), (1, "gated_gb"), (7, "gated"), (3, "lrelu")])
def test_twin_autograd_is_the_written_out_split_products(i, variant):
    """lo hi + hi lo + hi hi with the operand pairs (U, w), (g_pre, w), (g_pre, U); U blended in float32 and THEN split,
    g_pre formed in float32 and THEN split.  Bitwise for the convolutions' own outputs; the adjoint and the epilogues are
    float64 expressions written twice (1e-14)."""
    ref = uc.reference(i, variant)
    out = uc.written_out(i, variant, uc.forward64(i, variant)["pre"] > 0 if variant == "lrelu" else None)
    assert torch.equal(ref["g_w"], out["g_w"])
    for k in uc.keys(variant):
        assert rel_l2(ref[k], out[k]) <= 1e-14, k


@pytest.mark.parametrize("i,variant", [(1, "lrelu"), (3, "gated_gb"), (7, "gated")])
def test_dropping_a_cross_term_or_truncating_lands_above_the_bar(i, variant):
    """Without lo hi, without hi lo, hi hi alone: each product lands above 10 x BAR; a split that truncates instead of
    rounding lands above BAR.  g_bias and g_gb have no product in them and are left out."""
    ref = uc.reference(i, variant)
    positive = uc.forward64(i, variant)["pre"] > 0 if variant == "lrelu" else None
    conv_keys = [k for k in uc.keys(variant) if k in CONV_KEYS]
    for first, second in (("hh", "lh"), ("lh", "hh"), ("h", "h")):
        out = uc.written_out(i, variant, positive, first, second)
        for k in conv_keys:
            e = rel_l2(out[k], ref[k + "64"])
            print(uc.IDS[i], variant, first, second, k, "%.3e" % e)
            assert e > 10 * BAR, (first, second, k, e)
    out = uc.truncated(i, variant, positive)
    for k in conv_keys:
        e = rel_l2(out[k], ref[k + "64"])
        print(uc.IDS[i], variant, "truncated", k, "%.3e" % e)
        assert e > BAR, (k, e)


def test_twins_split_as_perceptual_return_input_dtypes_and_check_shapes():
    from goliath_amd import perceptual, texdec

    assert texdec._three is perceptual._three and texdec._precision is perceptual._precision
    inp = uc.inputs(1)
    leaves = [inp[k].clone().requires_grad_(True) for k in ("x", "w", "gate", "gb")]
    y = texdec.upconv_gated_split_torch(*leaves)
    grads = torch.autograd.grad((y * inp["up"].double()).sum(), leaves)
    assert y.dtype == torch.float64 and all(g.dtype == torch.float32 and g.shape == t.shape for g, t in zip(grads, leaves))
    y32 = texdec.upconv_gated_split_torch(*leaves, acc_dtype=torch.float32)
    assert y32.dtype == torch.float32 and rel_l2(y32, y) <= 1e-6
    # only the gradients that are required are formed; a broadcast gainbias gets the summed gradient
    x, w, gate = (inp[k].clone() for k in ("x", "w", "gate"))
    gb = inp["gb"][:, :, :1, :1].clone().requires_grad_(True)
    y = texdec.upconv_gated_split_torch(x, w, gate, gb)
    (g_gb,) = torch.autograd.grad((y * inp["up"].double()).sum(), (gb,))
    assert g_gb.shape == gb.shape and rel_l2(g_gb, (uc.SCALE * inp["up"]).sum((2, 3), keepdim=True)) <= 1e-6
    # U by the rule is the library's resize
    U = texdec.up2_rule(inp["x"].double())
    assert rel_l2(U, uc.up64(inp["x"].double())) <= 1e-7
    one = torch.randn(1, 2, 1, 1)
    assert torch.equal(texdec.up2_rule(one), one.expand(1, 2, 2, 2))
    with pytest.raises(Exception, match="shapes"):
        texdec.upconv_lrelu_split_torch(x, torch.zeros(32, 64, 4, 4), inp["bias"])
    with pytest.raises(Exception, match="bias"):
        texdec.upconv_lrelu_split_torch(x, w, inp["bias"][0])
    with pytest.raises(Exception, match="gate"):
        texdec.upconv_gated_split_torch(x, w, gate[:, :1])


def test_operators_refuse_what_the_kernels_do_not_take(monkeypatch):
    from goliath_amd import _lib, texdec

    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a launch"))
    z = torch.zeros
    with pytest.raises(_lib.GoliathHipError, match="no CPU path"):
        texdec.upconv_lrelu(z(1, 32, 4, 4), z(16, 32, 3, 3), z(16, 8, 8), precision="bf16x3")
    with pytest.raises(_lib.GoliathHipError, match="no CPU path"):
        texdec.upconv_gated(z(1, 32, 4, 4), z(16, 32, 3, 3), z(1, 16, 8, 8), precision="bf16x3")
    with pytest.raises(ValueError, match="precision"):
        texdec.upconv_lrelu(z(1, 32, 4, 4), z(16, 32, 3, 3), z(16, 8, 8), precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        texdec.upconv_gated(z(1, 32, 4, 4), z(16, 32, 3, 3), z(1, 16, 8, 8), precision="tf32")


def test_supported_bf16x3():
    from goliath_amd import texdec

    table = {(128, 256, 32, 32): True, (256, 128, 64, 64): True, (128, 128, 128, 128): True, (128, 64, 256, 256): True,
             (64, 32, 512, 512): True, (32, 16, 1024, 1024): True, (16, 4, 2048, 2048): False,      # the seven layers
             (32, 16, 1, 1): True, (32, 48, 5, 17): True, (32, 8, 4, 4): False, (32, 4, 4, 4): False, (48, 16, 4, 4): False,
             (8, 16, 4, 4): False, (0, 16, 4, 4): False, (32, 0, 4, 4): False, (32, 16, 0, 4): False, (32, 16, 4, 0): False}
    for shape, want in table.items():
        assert texdec.supported_bf16x3(*shape) is want, shape
    size = 32
    for ci, co in texdec.CHANNELS:
        assert texdec.supported_bf16x3(ci, co, size, size) == ((ci, co) != (16, 4))
        size *= 2
    assert all(texdec.supported_bf16x3(*c[1:]) for c in uc.CASES)
    assert all(len(k) == 5 and v is True and k[0] in (0, 1) and texdec.supported_bf16x3(*k[1:])
               for k, v in texdec.DISPATCH_BF16X3.items())


# ---- the input gradient's tile -------------------------------------------------------------------------------------------
def _first_row(i, n, nout):
    return 0 if (i <= 0 or n <= 1) else ((i - 1) * (nout - 1)) // (n - 1) + 1


def _constants():
    src = open(os.path.join(ROOT, "goliath_amd", "csrc", "upconvx.hip")).read()
    core = open(os.path.join(ROOT, "goliath_amd", "csrc", "gol_conv3x_core.h")).read()
    xh, xw = map(int, re.search(r"constexpr int kXH = (\d+), kXW = (\d+);", src).groups())
    th, tw = map(int, re.search(r"constexpr int kTH = (\d+), kTW = (\d+);", core).groups())
    return xh, xw, th, tw


def test_bwd_x_tile_constants():
    assert _constants() == (2, 14, 8, 32)


@pytest.mark.parametrize("axis", (0, 1))
def test_input_gradient_region_holds_every_contributing_row(axis):
    """gol_upconvx_bwd_x gathers, per source row i, from the 5 rows of U starting at up_first_row(i), inside a region of 8 rows
    (32 columns) per tile of 2 (14) source rows (columns) starting at up_first_row(tile origin): every row of U that the
    coordinate rule blends into row i lies inside both, for every tile of every size."""
    xh, xw, th, tw = _constants()
    tile, region = ((xh, th), (xw, tw))[axis]
    for n in list(range(1, 201)) + [1024, 2048, 2049, 4095, 4096]:
        nout = 2 * n
        reach = {}
        for r in range(nout):
            nr, d = r * (n - 1), nout - 1
            a = nr // d
            if nr - a * d < d:                  # weight 1 - frac > 0
                reach.setdefault(a, []).append(r)
            if nr - a * d > 0:                  # weight frac > 0
                reach.setdefault(min(a + 1, n - 1), []).append(r)
        for i0 in range(0, n, tile):
            lo0 = _first_row(i0, n, nout)
            for i in range(i0, min(i0 + tile, n)):
                lo = _first_row(i, n, nout)
                assert lo >= lo0
                for r in reach[i]:
                    assert lo <= r < lo + 5 and lo0 <= r < lo0 + region, (n, i0, i, r)


@pytest.mark.parametrize("span,name", [(3, "kSR"), (34, "kSC")])
def test_weight_gradient_source_window_holds_every_texel(span, name):
    """gol_upconvx_bwd_w keeps, per chunk, the rows r - 1 .. r + 1 (columns X0 - 1 .. X0 + 32) of U's SOURCE in LDS: kSR rows
    (kSC columns) of x starting at the source index of the first row (column) inside the image.  Every r0 and r1 of the
    window lies inside, for every origin of every size."""
    src = open(os.path.join(ROOT, "goliath_amd", "csrc", "upconvx.hip")).read()
    cap = int(re.search(r"\b%s = (\d+)" % name, src).group(1))
    assert (name, cap) in (("kSR", 3), ("kSC", 20))
    for n in list(range(1, 201)) + [1024, 2048, 2049, 4095, 4096]:
        nout, d = 2 * n, 2 * n - 1
        for origin in range(-1, nout):
            lo, hi = max(origin, 0), min(origin + span - 1, nout - 1)
            first, last = (lo * (n - 1)) // d, min((hi * (n - 1)) // d + 1, n - 1)
            assert last - first + 1 <= cap, (n, origin)


# ---- texture_branches and the drop-in ------------------------------------------------------------------------------------
def test_texture_branches_on_cpu_runs_the_library_lines(monkeypatch):
    from goliath_amd import texdec

    monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")
    monkeypatch.setattr(texdec, "upconv_lrelu", lambda *a, **k: pytest.fail("the operator on CPU tensors"))
    monkeypatch.setattr(texdec, "upconv_gated", lambda *a, **k: pytest.fail("the operator on CPU tensors"))
    dec = uc.stack()
    jf, z, gbs = uc.stack_inputs()
    with torch.no_grad():
        want = uc.library_loops(dec, jf, z, gbs)
        for kw in ({}, {"precision": "fp32"}, {"precision": "bf16x3"}):
            assert torch.equal(texdec.texture_branches(dec, jf, z, gbs, first_size=8, **kw), want), kw
        twin = uc.twin_loops(dec, jf, z, gbs)
    assert want.shape == (2, 16, 32, 32) and 0 < rel_l2(twin, want) <= 1e-4
    with pytest.raises(ValueError, match="precision"):
        texdec.texture_branches(dec, jf, z, gbs, first_size=8, precision="bf16")


def test_texture_branches_bf16x3_routes_by_its_own_table(monkeypatch):
    """With the tensors taken for GPU tensors: an empty DISPATCH_BF16X3 sends nothing to the split operator, a listed shape
    goes there, GOLIATH_FUSED_TEXDEC_ALL=1 sends every supported one, and "fp32" never does."""
    from goliath_amd import texdec

    taken = []

    def lrelu(x, w, bias, leak, precision="fp32"):
        taken.append((0, precision, w.shape[1], w.shape[0], x.shape[2], x.shape[3]))
        return texdec.upconv_lrelu_split_torch(x, w, bias, leak).to(x.dtype)

    def gated(x, w, gate, gb, scale, precision="fp32"):
        taken.append((1, precision, w.shape[1], w.shape[0], x.shape[2], x.shape[3]))
        return texdec.upconv_gated_split_torch(x, w, gate, gb, scale).to(x.dtype)

    monkeypatch.setattr(texdec, "upconv_lrelu", lrelu)
    monkeypatch.setattr(texdec, "upconv_gated", gated)
    monkeypatch.setattr(texdec, "_on_gpu", lambda *t: True)
    monkeypatch.setattr(texdec, "DISPATCH", {})
    monkeypatch.delenv("GOLIATH_FUSED_TEXDEC_ALL", raising=False)
    dec = uc.stack()
    jf, z, gbs = uc.stack_inputs()
    run = lambda **kw: texdec.texture_branches(dec, jf, z, gbs, first_size=8, **kw)
    with torch.no_grad():
        want = uc.library_loops(dec, jf, z, gbs)
        monkeypatch.setattr(texdec, "DISPATCH_BF16X3", {})
        assert torch.equal(run(precision="bf16x3"), want) and not taken
        monkeypatch.setattr(texdec, "DISPATCH_BF16X3", {(1, 64, 32, 8, 8): True})
        run(precision="bf16x3")
        assert taken == [(1, "bf16x3", 64, 32, 8, 8)]
        del taken[:]
        assert torch.equal(run(), want) and not taken              # the default precision does not look at that table
        # a shape in the fp32 table only: exactly today's decision, also at "bf16x3"
        monkeypatch.setattr(texdec, "DISPATCH_BF16X3", {})
        monkeypatch.setattr(texdec, "DISPATCH", {(0, 32, 64, 4, 4): True})
        run(precision="bf16x3")
        assert taken == [(0, "fp32", 32, 64, 4, 4)]
        del taken[:]
        monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")
        got = run(precision="bf16x3")
        assert taken == [(m, "bf16x3", *s) for m in (0, 1) for s in uc.STACK_SHAPES]
        assert 0 < rel_l2(got, want) <= 1e-4
        del taken[:]
        run()
        assert taken == [(m, "fp32", *s) for m in (0, 1) for s in uc.STACK_SHAPES]


def test_patch_urhand_stores_the_precision_on_the_class():
    from goliath_amd import dropin, texdec

    mod = types.SimpleNamespace(ConvTeacherDecoder=type("ConvTeacherDecoder", (), {}))
    assert texdec.TEXDEC_PRECISION_FLAG == "_gol_texture_decoder_precision"
    assert inspect.signature(dropin.patch_urhand).parameters["texture_decoder_precision"].default == "fp32"
    assert dropin.patch_urhand(mod, texture_decoder=True) is mod
    assert getattr(mod.ConvTeacherDecoder, texdec.TEXDEC_PRECISION_FLAG) == "fp32"
    assert getattr(mod.ConvTeacherDecoder, texdec.TEXTURE_DECODER_FLAG) is True
    for _ in range(2):                                            # idempotent
        dropin.patch_urhand(mod, texture_decoder=True, texture_decoder_precision="bf16x3")
        assert getattr(mod.ConvTeacherDecoder, texdec.TEXDEC_PRECISION_FLAG) == "bf16x3"
        assert getattr(mod.ConvTeacherDecoder, texdec.TEXTURE_DECODER_FLAG) is True
    dropin.patch_urhand(mod)
    assert getattr(mod.ConvTeacherDecoder, texdec.TEXDEC_PRECISION_FLAG) == "fp32"
    assert getattr(mod.ConvTeacherDecoder, texdec.TEXTURE_DECODER_FLAG) is False
    for bad in ("bf16", "tf32", None):
        with pytest.raises(ValueError, match="precision"):
            dropin.patch_urhand(mod, texture_decoder=True, texture_decoder_precision=bad)


# ---- the binding -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "goliath_hip.h")).read(), flags=re.S)


def test_header_declares_and_binding_exports_the_entries():
    from goliath_amd import _lib

    for name in ENTRIES + tuple(QUERIES):
        assert re.search(r"\b" + name + r"\s*\(", _header()), name
        assert name in _lib.exported_symbols(), name


@pytest.mark.parametrize("entry", ENTRIES + ("gol_upconv_bwd",))
def test_marshallers_follow_the_header(entry, monkeypatch):
    """Each marshaller passes exactly the parameters goliath_hip.h declares, by name, in its order and with its C types."""
    from goliath_amd import _lib, texdec

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(texdec, "_abi_" + entry[len("gol_"):])
    sig = inspect.signature(fn).parameters
    assert set(sig) == {n for _, n in params} - {"stream"}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in sig.values())
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "float": (ctypes.c_float, i + 0.5)}[ctype]
        v = {"stream": 0xBEEF}.get(name, v)
        if name != "stream":
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(texdec, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


@pytest.mark.parametrize("entry", sorted(QUERIES))
def test_size_queries_follow_the_header(entry, monkeypatch):
    from goliath_amd import _lib, texdec

    decl = re.search(r"\blong long\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    assert [" ".join(p.split()) for p in decl.split(",")] == QUERIES[entry]
    seen = []

    def fake(*args):
        seen.append(args)
        return 7

    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(**{entry: fake}))
    n = len(QUERIES[entry])
    helper = texdec.packed_elems_bf16x3 if n == 2 else texdec.bwd_w_scratch_floats_bf16x3
    assert helper(*range(1, n + 1)) == 7
    assert [(type(a), a.value) for a in seen[0]] == [(ctypes.c_int, v) for v in range(1, n + 1)]
    assert fake.restype is ctypes.c_longlong


def test_block_formula_of_the_k_split_case():
    assert uc.bwd_w_blocks(*uc.CASES[uc.KSPLIT]) == uc.KSPLIT_BLOCKS
    assert uc.bwd_w_blocks(*uc.CASES[0]) == 4 and uc.bwd_w_blocks(1, 32, 16, 1024, 1024) == 512
    # bounded whatever B, Hi and Wi: blocks <= 512 / pairs + 1
    for c in ((64, 64, 32, 512, 512), (1, 128, 256, 32, 32), (7, 256, 128, 64, 64)):
        pairs = (c[1] // 32) * -(-c[2] // 64)
        assert uc.bwd_w_blocks(*c) * pairs <= 512 + pairs
