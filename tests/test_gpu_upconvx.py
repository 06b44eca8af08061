"""GPU: the split-bf16 texture-decoder layer (goliath_amd.texdec.upconv_lrelu / upconv_gated at precision "bf16x3":
gol_upconvx_*) against the float64-accumulated split twin and plain float64 on the cases of tests/upconvx_cases.py: the packed
layout, values, every gradient, the sign condition, gradient subsets, the ABI's return codes, reproducibility, graph capture,
a small stack through texture_branches and the drop-in keyword.

The twin blends U in float32 by the same expression and splits the same float32 values, so only the fp32 summation order (and
the contraction of the blend) separates the operator from it (about 1e-7 expected).  A kernel that truncates instead of
rounding, or drops a cross term, lands above BAR = 1e-5.  Mode 0's gradients are compared under the OPERATOR's sign of y
(tests/conv3ub_cases.py says why)."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import upconvx_cases as uc
from upconvx_cases import BAR, LEAK, SCALE, rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _cuda(i):
    return {k: v.cuda() for k, v in uc.inputs(i).items()}


def _run(i, variant, need=None):
    """y and the gradients (None where not needed) of the operator on case i, by uc.keys(variant)."""
    from goliath_amd import texdec

    t = _cuda(i)
    ns = uc.names(variant)
    need = (True,) * len(ns) if need is None else need
    leaves = {k: t[k].requires_grad_(n) for k, n in zip(ns, need)}
    y = uc.call(variant, texdec.upconv_lrelu, texdec.upconv_gated, leaves, precision="bf16x3")
    wanted = [k for k in ns if leaves[k].requires_grad]
    grads = dict(zip(wanted, torch.autograd.grad((y * t["up"]).sum(), [leaves[k] for k in wanted])))
    return dict(y=y.detach(), **{"g_" + k: grads.get(k) for k in ns})


@functools.lru_cache(maxsize=None)
def _full(i, variant):
    return _run(i, variant)


def _dims(i, mode, full=True):
    d = dict(zip(("B", "Ci", "Co", "Hi", "Wi"), uc.CASES[i]))
    return dict(d, mode=mode, leak=LEAK if mode == 0 else 1.0, scale=1.0 if mode == 0 else SCALE) if full else d


def _pack(w):
    from goliath_amd import texdec

    Co, Ci = w.shape[:2]
    packed = torch.empty(texdec.packed_elems_bf16x3(Co, Ci), device="cuda", dtype=torch.int16)
    texdec._abi_upconvx_pack(Co=Co, Ci=Ci, weight=w, packed=packed)
    return packed


@pytest.mark.parametrize("i", (1, 3))
def test_packed_weight_is_the_split(i):
    """packed = [hi | lo][9 taps][Cop / 8][Ci / 8][8 co][8 ci], bit for bit the round-to-nearest-even split of the twin, with
    zero rows past Co (case 3: Co = 48 in Cop = 64)."""
    from goliath_amd import perceptual, texdec

    w = uc.inputs(i)["w"]
    Co, Ci = w.shape[:2]
    Cop = (Co + 31) // 32 * 32
    packed = _pack(w.cuda()).cpu()
    assert packed.numel() == 2 * 9 * Cop * Ci == texdec.packed_elems_bf16x3(Co, Ci)
    assert texdec.packed_elems_bf16x3(4, 16) == 0 and texdec.packed_elems_bf16x3(16, 16) == 0
    assert texdec.packed_elems_bf16x3(8, 32) == 0 and texdec.packed_elems_bf16x3(16, 32) == 2 * 9 * 32 * 32
    got = packed.view(2, 9, Cop // 8, Ci // 8, 8, 8)
    wp = torch.zeros(Cop, Ci, 3, 3)
    wp[:Co] = w
    for plane, part in enumerate(perceptual.split_bf16(wp)):
        want = part.view(torch.int16).view(Cop // 8, 8, Ci // 8, 8, 9).permute(4, 0, 2, 1, 3)
        assert torch.equal(got[plane], want)
    if Cop != Co:
        assert int(got[:, :, Co // 8:].abs().max()) == 0


@pytest.mark.parametrize("i,variant", uc.PARAMS, ids=uc.PARAM_IDS)
def test_matches_the_split_twin(i, variant):
    """y and each of g_x, g_w, g_bias or g_gate, g_gb <= 1e-5 rel-L2 against the float64-accumulated split twin on the same
    fp32 inputs (about 1e-7 expected) and against plain float64; mode 0's gradients with the references' g_pre formed under
    the operator's own sign of y."""
    got = _full(i, variant)
    ref = uc.gradients(i, variant, got["y"].cpu() > 0) if variant == "lrelu" else uc.reference(i, variant)
    fwd = uc.reference(i, variant)
    err = {"y": (rel_l2(got["y"], fwd["y"]), rel_l2(got["y"], fwd["y64"]))}
    for k in uc.keys(variant)[1:]:
        err[k] = (rel_l2(got[k], ref[k]), rel_l2(got[k], ref[k + "64"]))
    print(uc.IDS[i], variant, {k: "twin %.2e float64 %.2e" % v for k, v in err.items()})
    for k, (e_twin, e_64) in err.items():
        assert got[k].shape == ref[k].shape and float(ref[k].abs().max()) > 0
        assert e_twin <= BAR and e_64 <= BAR, (uc.IDS[i], variant, k, e_twin, e_64)


@pytest.mark.parametrize("i", range(len(uc.CASES)), ids=uc.IDS)
def test_sign_differs_from_float64_only_next_to_zero(i):
    """Mode 0: the operator's sign of y may differ from float64's only where |pre64| < 1e-5 rms(pre64), and at no more than
    0.1 % of the elements."""
    differs = (_full(i, "lrelu")["y"].cpu() > 0) != (uc.forward64(i, "lrelu")["pre"] > 0)
    near = uc.near_zero(i)
    print(uc.IDS[i], int(differs.sum()), "signs differ,", int(near.sum()), "elements near zero, of", near.numel())
    assert not bool((differs & ~near).any())
    assert int(differs.sum()) <= uc.SIGN_CAP * differs.numel()


SUBSETS = {"lrelu": ((True, False, False), (False, True, False), (False, False, True), (True, True, False),
                     (False, True, True)),
           "gated_gb": ((True, False, False, False), (False, True, False, False), (False, False, True, False),
                        (False, False, False, True), (False, False, True, True), (True, True, False, True)),
           "gated": ((True, False, False), (False, False, True), (True, True, True))}


@pytest.mark.parametrize("variant", uc.VARIANTS)
def test_gradient_subsets(variant):
    """Each needs_input_grad combination launches only its kernels -- bwd_x, bwd_w, the fp32 operator's streaming pass for
    g_bias or for g_gb alone, bwd_gate (with g_gb riding along) -- and returns bitwise what the full backward returns."""
    from goliath_amd import texdec

    i = 3
    full = _full(i, variant)
    calls = []
    names = ("_abi_upconvx_bwd_x", "_abi_upconvx_bwd_w", "_abi_upconvx_bwd_gate", "_abi_upconv_bwd")
    real = {n: getattr(texdec, n) for n in names}
    outs = lambda kw: tuple(k for k in ("g_x", "g_w", "g_bias", "g_gate", "g_gb") if kw.get(k) is not None)
    try:
        for n, fn in real.items():
            setattr(texdec, n, lambda fn=fn, n=n, **kw: (calls.append((n[len("_abi_"):], outs(kw))), fn(**kw))[1])
        for need in SUBSETS[variant]:
            del calls[:]
            got = _run(i, variant, need)
            wanted = dict(zip(uc.names(variant), need))
            want_calls = []
            if wanted["x"]:
                want_calls.append(("upconvx_bwd_x", ("g_x",)))
            if wanted["w"]:
                want_calls.append(("upconvx_bwd_w", ("g_w",)))
            if wanted.get("bias"):
                want_calls.append(("upconv_bwd", ("g_bias",)))
            if wanted.get("gate"):
                want_calls.append(("upconvx_bwd_gate", ("g_gate", "g_gb") if wanted.get("gb") else ("g_gate",)))
            elif wanted.get("gb"):
                want_calls.append(("upconv_bwd", ("g_gb",)))
            assert calls == want_calls, (need, calls)
            assert torch.equal(got["y"], full["y"])
            for k, n in zip(uc.keys(variant)[1:], need):
                assert (got[k] is None) == (not n), (need, k)
                assert not n or torch.equal(got[k], full[k]), (need, k)
    finally:
        for n, fn in real.items():
            setattr(texdec, n, fn)


def test_null_outputs_launch_nothing():
    """The ABI itself: NULL outputs are GOL_OK and launch nothing (a g_gb handed to bwd_gate without g_gate stays untouched)."""
    from goliath_amd import texdec

    i = 3
    t = _cuda(i)
    packed = _pack(t["w"])
    for mode, variant in ((0, "lrelu"), (1, "gated_gb")):
        d = _dims(i, mode)
        y = _full(i, variant)["y"]
        aux = dict(y=y, gate=None) if mode == 0 else dict(y=None, gate=t["gate"])
        texdec._abi_upconvx_bwd_x(**d, packed=packed, **aux, g_y=t["up"], g_x=None)
        texdec._abi_upconvx_bwd_w(**d, x=t["x"], **aux, g_y=t["up"], g_w=None, scratch=None)
    seven = torch.full_like(t["up"], 7.0)
    texdec._abi_upconvx_bwd_gate(**_dims(i, 1, full=False), scale=SCALE, x=t["x"], packed=packed, g_y=t["up"], g_gate=None,
                                 g_gb=seven)
    torch.cuda.synchronize()
    assert bool((seven == 7.0).all())


def test_return_codes():
    """Unsupported shapes answer GOL_ERR_UNSUPPORTED and invalid calls GOL_ERR_INVALID_ARG before any launch: outputs
    pre-filled with 7.0 stay untouched.  B == 0 is GOL_OK (bwd_w zeroes g_w)."""
    from goliath_amd import _lib, texdec

    lib = _lib.load()
    i = 3                                                         # (1, 32, 48, 5, 17)
    t = _cuda(i)
    packed = _pack(t["w"])
    seven = lambda ref: torch.full_like(ref, 7.0)
    y, g_x, g_w, g_gate, g_gb = seven(t["up"]), seven(t["x"]), seven(t["w"]), seven(t["up"]), seven(t["up"])
    scratch = torch.full((texdec.bwd_w_scratch_floats_bf16x3(*uc.CASES[i]),), 7.0, device="cuda")
    null, s, c, f = ctypes.c_void_p(0), _lib.stream_ptr(), ctypes.c_int, ctypes.c_float
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    px, pk, pu, pb, pg, py = p(t["x"]), p(packed), p(t["up"]), p(t["bias"]), p(t["gate"]), p(y)
    dims = lambda B, Ci, Co, Hi, Wi: (c(B), c(Ci), c(Co), c(Hi), c(Wi))
    fwd = lambda *d, mode=0, leak=LEAK, x=px: lib.gol_upconvx_fwd(*dims(*d), c(mode), f(leak), f(SCALE), x, pk, pb, pg, null,
                                                                   py, s)
    bwd_x = lambda *d, mode=0, leak=LEAK, x=pu: lib.gol_upconvx_bwd_x(*dims(*d), c(mode), f(leak), f(SCALE), pk, py, pg, x,
                                                                       p(g_x), s)
    bwd_w = lambda *d, mode=0, leak=LEAK, x=px: lib.gol_upconvx_bwd_w(*dims(*d), c(mode), f(leak), f(SCALE), x, py, pg, pu,
                                                                       p(g_w), p(scratch), s)
    bwd_g = lambda *d, x=px: lib.gol_upconvx_bwd_gate(*dims(*d), f(SCALE), x, pk, pu, p(g_gate), p(g_gb), s)
    OK, INVALID, UNSUPPORTED = 0, -1, -3
    scr = lib.gol_upconvx_bwd_w_scratch_floats
    scr.restype = ctypes.c_longlong
    good = uc.CASES[i]
    bad = ((1, 16, 4, 5, 17),             # the last layer: stays on gol_upconv_*
           (1, 32, 8, 5, 17),             # Co = 8
           (1, 32, 40, 5, 17),            # Co = 40
           (1, 48, 48, 5, 17),            # Ci = 48
           (1, 8, 16, 5, 17),             # Ci = 8
           (1, 0, 48, 5, 17),             # Ci = 0
           (1, 32, 0, 5, 17),             # Co = 0
           (1, 32, 48, 0, 17),            # Hi = 0
           (1, 32, 48, 5, 0),             # Wi = 0
           (65536, 32, 48, 5, 17))        # B = 65536 (dims only: nothing is read)
    for fn in (fwd, bwd_x, bwd_w, bwd_g):
        for d in bad:
            assert fn(*d) == UNSUPPORTED, d
        assert b"gol_upconvx" in lib.gol_last_error()
        assert fn(-1, *good[1:]) == INVALID
        assert fn(1, 32, 48, -5, 17) == INVALID
        assert fn(*good, x=null) == INVALID                       # x / g_y
    for fn in (fwd, bwd_x, bwd_w):
        assert fn(*good, leak=0.0) == INVALID and fn(*good, leak=-0.2) == INVALID
        assert fn(*good, mode=2) == INVALID
        assert fn(*good, mode=1, leak=0.0, x=null) == INVALID     # mode 1 does not look at leak; the pointer is still needed
    for d in bad:
        assert scr(*dims(*d)) == 0, d
    assert scr(*dims(0, *good[1:])) == 0
    assert scr(*dims(*good)) == uc.bwd_w_blocks(*good) * 9 * 48 * 32 == 20 * 9 * 48 * 32
    assert lib.gol_upconvx_pack(c(4), c(16), px, pk, s) == UNSUPPORTED
    assert lib.gol_upconvx_pack(c(16), c(48), px, pk, s) == UNSUPPORTED
    assert lib.gol_upconvx_pack(c(48), c(32), null, pk, s) == INVALID
    assert lib.gol_upconvx_pack(c(-16), c(32), px, pk, s) == INVALID
    torch.cuda.synchronize()
    for out in (y, g_x, g_w, g_gate, g_gb, scratch):
        assert bool((out == 7.0).all())                            # nothing was launched
    # B == 0: no kernel; the sum over an empty batch is zero
    assert fwd(0, *good[1:]) == OK and bwd_x(0, *good[1:]) == OK and bwd_w(0, *good[1:]) == OK and bwd_g(0, *good[1:]) == OK
    torch.cuda.synchronize()
    assert all(bool((out == 7.0).all()) for out in (y, g_x, g_gate, g_gb)) and bool((g_w == 0.0).all())
    assert fwd(*good) == OK and bwd_x(*good) == OK and bwd_w(*good) == OK and bwd_g(*good) == OK
    torch.cuda.synchronize()
    for out in (y, g_x, g_w, g_gate, g_gb):
        assert not bool((out == 7.0).any()) and float(out.abs().max()) > 0


@pytest.mark.parametrize("variant", ("lrelu", "gated_gb"))
def test_forward_and_backward_are_bitwise_reproducible(variant):
    """On the K-split case: 90 K blocks of three chunks, the last one chunk."""
    from goliath_amd import texdec

    c = uc.CASES[uc.KSPLIT]
    assert uc.bwd_w_blocks(*c) == uc.KSPLIT_BLOCKS
    assert texdec.bwd_w_scratch_floats_bf16x3(*c) == uc.KSPLIT_BLOCKS * 9 * c[2] * c[1]
    a, b = _full(uc.KSPLIT, variant), _run(uc.KSPLIT, variant)
    for k in uc.keys(variant):
        assert torch.equal(a[k], b[k]) and float(a[k].abs().max()) > 0, k


@pytest.mark.parametrize("mode", (0, 1))
def test_no_host_sync_and_graph_replay(mode):
    """The calls of a layer's forward and backward on the caller's buffers: no host synchronisation (sync debug mode
    "error"), and captured into one graph they replay bitwise what the eager calls give, also after new values were written
    into the same input tensors."""
    from goliath_amd import texdec

    i = uc.KSPLIT
    d = _dims(i, mode)
    small = _dims(i, mode, full=False)
    t = _cuda(i)
    Co, Ci = d["Co"], d["Ci"]
    scratch = torch.empty(texdec.bwd_w_scratch_floats_bf16x3(*uc.CASES[i]), device="cuda")          # before capture
    packed = torch.empty(texdec.packed_elems_bf16x3(Co, Ci), device="cuda", dtype=torch.int16)
    none = dict(x=None, w_eff=None, g_x=None, g_w=None, g_bias=None, g_gate=None, g_gb=None, scratch=None)

    def step(y, g_x, g_w, g_a, g_gb):
        aux = dict(y=y, gate=None) if mode == 0 else dict(y=None, gate=t["gate"])
        texdec._abi_upconvx_pack(Co=Co, Ci=Ci, weight=t["w"], packed=packed)
        texdec._abi_upconvx_fwd(**d, x=t["x"], packed=packed, bias=t["bias"] if mode == 0 else None, gate=aux["gate"],
                                gb=t["gb"] if mode == 1 else None, y=y)
        texdec._abi_upconvx_bwd_x(**d, packed=packed, **aux, g_y=t["up"], g_x=g_x)
        texdec._abi_upconvx_bwd_w(**d, x=t["x"], **aux, g_y=t["up"], g_w=g_w, scratch=scratch)
        if mode == 0:
            texdec._abi_upconv_bwd(**d, **dict(none, g_bias=g_a), **aux, g_y=t["up"])
        else:
            texdec._abi_upconvx_bwd_gate(**small, scale=SCALE, x=t["x"], packed=packed, g_y=t["up"], g_gate=g_a, g_gb=g_gb)

    buffers = lambda: tuple(torch.empty_like(t[k]) for k in ("up", "x", "w", "bias" if mode == 0 else "gate", "gb"))
    o0 = buffers()
    step(*o0)                                              # (first call: code objects)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step(*o0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    o1 = buffers()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*o1)
    graph.replay()
    torch.cuda.synchronize()
    written = slice(0, 4 if mode == 0 else 5)
    assert all(torch.equal(a, b) for a, b in zip(o1[written], o0[written]))
    t["x"].mul_(-0.5)                                      # new values in the SAME tensors
    t["up"].add_(0.25)
    t["w"].mul_(1.5)
    t["bias"].neg_()
    t["gate"].add_(0.5)
    t["gb"].neg_()
    graph.replay()
    step(*o0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(o1[written], o0[written])) and all(float(a.abs().max()) > 0 for a in o1[written])


def test_stack_through_texture_branches(monkeypatch):
    """upconvx_cases.SmallTexDecoder (channels 32, 64, 32, 16 in both branches, from 4^2, gainbias on the first two layers),
    fp32 on the GPU: with GOLIATH_FUSED_TEXDEC_ALL=1 and precision="bf16x3" all six layers run on the split operator,
    F.interpolate is not called, and the output and every parameter and input gradient are <= 1e-5 from the twin chain
    accumulated in float64; the distance from plain float64 is printed; with the default precision the output is bitwise the
    parent path's."""
    from goliath_amd import texdec

    dec, dec64 = uc.stack().cuda(), uc.stack(torch.float64).cuda()
    jf, z, gbs = uc.stack_inputs()
    jf, z, gbs = jf.cuda(), z.cuda(), [g.cuda() for g in gbs]
    taken = []
    lrelu, gated = texdec.upconv_lrelu, texdec.upconv_gated

    def spy(mode, op):
        def f(x, w, *a, **k):
            taken.append((mode, k.get("precision", "fp32"), w.shape[1], w.shape[0], x.shape[2], x.shape[3]))
            return op(x, w, *a, **k)
        return f

    monkeypatch.setattr(texdec, "upconv_lrelu", spy(0, lrelu))
    monkeypatch.setattr(texdec, "upconv_gated", spy(1, gated))
    monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")
    interpolate = F.interpolate
    monkeypatch.setattr(F, "interpolate", lambda *a, **k: pytest.fail("a resize"))
    run = lambda m, a, b, g: texdec.texture_branches(m, a, b, g, first_size=8, precision="bf16x3")
    out, g_in, grads = uc.stack_run(dec, jf, z, gbs, run)
    monkeypatch.setattr(F, "interpolate", interpolate)
    assert taken == [(m, "bf16x3", *s) for m in (0, 1) for s in uc.STACK_SHAPES]
    to64 = lambda v: v.double()
    out_t, g_in_t, grads_t = uc.stack_run(dec64, to64(jf), to64(z), [to64(g) for g in gbs], uc.twin_loops)
    out_p, g_in_p, grads_p = uc.stack_run(dec64, to64(jf), to64(z), [to64(g) for g in gbs], uc.library_loops)
    assert set(grads) == set(grads_t) and len(grads) == 3 * 3 + 3 * 2 and set(g_in) == {"joint_feat", "z", "gainbias0", "gainbias1"}
    err = {"out": rel_l2(out, out_t), **{"g_" + n: rel_l2(g_in[n], g_in_t[n]) for n in g_in},
           **{"grad " + n: rel_l2(grads[n], grads_t[n]) for n in grads}}
    plain = {"out": rel_l2(out, out_p), **{"g_" + n: rel_l2(g_in[n], g_in_p[n]) for n in g_in},
             **{"grad " + n: rel_l2(grads[n], grads_p[n]) for n in grads}}
    for n, e in err.items():
        print("stack", n, "twin %.3e" % e, "plain float64 (chained; not asserted) %.3e" % plain[n])
    assert all(float(g.norm()) > 0 for g in list(grads_t.values()) + list(g_in_t.values()))
    assert max(err.values()) <= BAR, max(err.items(), key=lambda kv: kv[1])
    # the default precision: the split operator is not reached, and the output is the parent path's bits (the library is
    # asked for its deterministic solvers: two runs of the SAME library lines are not bitwise equal otherwise)
    del taken[:]
    monkeypatch.delenv("GOLIATH_FUSED_TEXDEC_ALL", raising=False)
    monkeypatch.setattr(texdec, "DISPATCH", {})
    monkeypatch.setattr(texdec, "DISPATCH_BF16X3", {(0, 32, 64, 4, 4): True})      # not looked at by "fp32"
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            y0 = texdec.texture_branches(dec, jf, z, gbs, first_size=8)
            y1 = texdec.texture_branches(dec, jf, z, gbs, first_size=8, precision="fp32")
            y2 = uc.library_loops(dec, jf, z, gbs)
            assert not taken
            # and with every fp32 shape forced, "fp32" is the fp32 operator's path, as on the parent
            monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")
            y3 = texdec.texture_branches(dec, jf, z, gbs, first_size=8)
            y4 = texdec.texture_branches(dec, jf, z, gbs, first_size=8, precision="fp32")
    finally:
        torch.backends.cudnn.deterministic = det
    assert torch.equal(y0, y1) and torch.equal(y0, y2) and torch.equal(y3, y4)
    assert taken == [(m, "fp32", *s) for m in (0, 1) for s in uc.STACK_SHAPES] * 2


def test_dropin_keyword(monkeypatch):
    """patch_urhand(texture_decoder=True, texture_decoder_precision="bf16x3") on the shaped decoder whose first texture layers
    are 32 -> 16 at 32^2 -> 64^2 reaches the split operator for the shapes put into DISPATCH_BF16X3; the default keyword does
    not; and with the flag at "fp32" the shaped decoder's results are bitwise those without the keyword."""
    import urhand_shaped as shaped
    from goliath_amd import dropin, texdec

    class Twin(shaped.ShapedConvTeacherDecoder):
        def __init__(self):
            super().__init__(seed=0)
            torch.manual_seed(11)
            self.init_uv_size = 32
            self.joint_conv_block_tex = nn.Conv2d(5 + 3, 32, 3, padding=1)
            self.featenc.z, self.featenc.gb = nn.Conv2d(4, 32, 3, padding=1), nn.Conv2d(4, 16, 3, padding=1)
            self.texmod0 = nn.ModuleList([texdec.Conv3WNUB(32, 16, 64, 64), texdec.Conv3WNUB(16, 4, 128, 128)])
            self.texmod1 = nn.ModuleList([texdec.Conv3WN(32, 16), texdec.Conv3WN(16, 4)])
            with torch.no_grad():
                for m in self.texmod0:
                    m.bias.normal_(0, 0.3)

    Twin.__module__ = shaped.__name__   # the forward looks its geometry helpers up in the module that defines the class
    gold = np.load(os.path.join(HERE, "golden", "urhand_model_golden.npz"))
    dec = Twin().cuda().eval()
    depths = [torch.from_numpy(gold[f"urhand_eval_depth{i}"]) for i in range(2)]
    dec.rl = shaped.ReplayRenderLayer(512, 512, depths * 4)     # four forwards, two shadow passes each
    inp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in shaped.urhand_inputs(B=1, L=2).items()}
    module = types.SimpleNamespace(ConvTeacherDecoder=Twin, get_shadow_map=None)
    taken = []
    lrelu, gated = texdec.upconv_lrelu, texdec.upconv_gated
    monkeypatch.setattr(texdec, "upconv_lrelu", lambda *a, **k: (taken.append((0, k.get("precision", "fp32"))), lrelu(*a, **k))[1])
    monkeypatch.setattr(texdec, "upconv_gated", lambda *a, **k: (taken.append((1, k.get("precision", "fp32"))), gated(*a, **k))[1])
    monkeypatch.delenv("GOLIATH_FUSED_TEXDEC_ALL", raising=False)
    monkeypatch.setattr(texdec, "DISPATCH", {})
    monkeypatch.setattr(texdec, "DISPATCH_BF16X3", {(0, 32, 16, 32, 32): True, (1, 32, 16, 32, 32): True})
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            dropin.patch_urhand(module, texture_decoder=True)
            assert getattr(Twin, texdec.TEXDEC_PRECISION_FLAG) == "fp32"
            plain = dec(**inp)
            assert not taken                                       # the default keyword does not reach it
            dropin.patch_urhand(module, texture_decoder=True, texture_decoder_precision="fp32")
            same = dec(**inp)
            assert not taken
            dropin.patch_urhand(module, texture_decoder=False, texture_decoder_precision="bf16x3")
            off = dec(**inp)
            assert not taken                                       # no effect without texture_decoder=True
            dropin.patch_urhand(module, texture_decoder=True, texture_decoder_precision="bf16x3")
            assert getattr(Twin, texdec.TEXDEC_PRECISION_FLAG) == "bf16x3"
            split = dec(**inp)
    finally:
        torch.backends.cudnn.deterministic = det
        del Twin.forward
    assert taken == [(0, "bf16x3"), (1, "bf16x3")]
    assert set(same) == set(plain) and all(torch.equal(same[k], plain[k]) for k in plain if torch.is_tensor(plain[k]))
    assert all(torch.equal(off[k], plain[k]) for k in plain if torch.is_tensor(plain[k]))
    e = rel_l2(split["tex"], plain["tex"])
    print("drop-in tex", e)
    assert float(plain["tex"].abs().max()) > 0 and 0 < e <= 1e-4      # the split layers are in the result
