"""GPU: the split-bf16 3x3 convolution of two sources + untied bias + LeakyReLU (goliath_amd.olatunet.conv3_ub_lrelu:
gol_conv3ub_*) against the float64-accumulated split twin and plain float64 on the cases of tests/conv3ub_cases.py: the
packed layout, values, the five gradients, the sign condition, gradient subsets, the ABI's return codes, reproducibility,
graph capture, a whole UNet and the drop-in keyword.

The twin splits the same float32 inputs to the same bits, so only the fp32 summation order separates the operator from it
(about 1e-7 expected).  A kernel that truncates instead of rounding, or drops a cross term, lands above BAR = 1e-5.  The
gradients are compared under the OPERATOR's sign of y (tests/conv3ub_cases.py says why)."""
import ctypes
import functools
import types

import pytest
import torch

import conv3ub_cases as cc
from conv3ub_cases import BAR, KEYS, LEAK, rel_l2

pytestmark = pytest.mark.gpu
NAMES = ("xa", "xb", "w", "bias")


def _cuda(i):
    inp = cc.inputs(i)
    return {k: None if v is None else v.cuda() for k, v in inp.items()}


def _run(i, need=(True, True, True, True)):
    """y and the gradients (None where not needed or absent) of olatunet.conv3_ub_lrelu on case i, by KEYS."""
    from goliath_amd import olatunet

    t = _cuda(i)
    leaves = {k: t[k].requires_grad_(n) for k, n in zip(NAMES, need) if t[k] is not None}
    y = olatunet.conv3_ub_lrelu(t["xa"], t["xb"], t["w"], t["bias"], LEAK)
    wanted = [k for k in leaves if leaves[k].requires_grad]
    grads = dict(zip(wanted, torch.autograd.grad((y * t["up"]).sum(), [leaves[k] for k in wanted])))
    return dict(y=y.detach(), g_xa=grads.get("xa"), g_xb=grads.get("xb"), g_w=grads.get("w"), g_bias=grads.get("bias"))


@functools.lru_cache(maxsize=None)
def _full(i):
    return _run(i)


def _dims(i, leak=True):
    d = dict(zip(("B", "Ca", "Cb", "Co", "H", "W"), cc.CASES[i]))
    return dict(d, leak=LEAK) if leak else d


def _pack(w):
    from goliath_amd import olatunet

    Co, Ci = w.shape[:2]
    packed = torch.empty(olatunet.packed_elems(Co, Ci), device="cuda", dtype=torch.int16)
    olatunet._abi_conv3ub_pack(Co=Co, Ci=Ci, weight=w, packed=packed)
    return packed


@pytest.mark.parametrize("i", (1, 2))
def test_packed_weight_is_the_split(i):
    """packed = [hi | lo][9 taps][Co / 8][Cip / 8][8 co][8 ci], bit for bit the round-to-nearest-even split of the twin, with
    zeros for the channels past Ci (case 1: Ci = 56 in Cip = 64)."""
    from goliath_amd import olatunet, perceptual

    w = cc.inputs(i)["w"]
    Co, Ci = w.shape[:2]
    Cip = (Ci + 31) // 32 * 32
    packed = _pack(w.cuda()).cpu()
    assert packed.numel() == 2 * 9 * Co * Cip == olatunet.packed_elems(Co, Ci)
    assert olatunet.packed_elems(16, 32) == 0 and olatunet.packed_elems(32, 12) == 0 and olatunet.packed_elems(32, 56) == 2 * 9 * 32 * 64
    got = packed.view(2, 9, Co // 8, Cip // 8, 8, 8)
    wp = torch.zeros(Co, Cip, 3, 3)
    wp[:, :Ci] = w
    for plane, part in enumerate(perceptual.split_bf16(wp)):
        want = part.view(torch.int16).view(Co // 8, 8, Cip // 8, 8, 9).permute(4, 0, 2, 1, 3)
        assert torch.equal(got[plane], want)
    if Cip != Ci:
        assert int(got[:, :, :, Ci // 8:].abs().max()) == 0


@pytest.mark.parametrize("i", range(len(cc.CASES)), ids=cc.IDS)
def test_matches_the_split_twin(i):
    """y <= 1e-5 rel-L2 against the float64-accumulated split twin on the same fp32 inputs (about 1e-7 expected: the fp32
    summation order) and against plain float64; the gradients to xa, xb, weight and bias the same, with the references'
    g_pre formed under the operator's own sign of y."""
    got = _full(i)
    ref = cc.gradients(i, got["y"].cpu() > 0)
    fwd = cc.reference(i)
    err = {"y": (rel_l2(got["y"], fwd["y"]), rel_l2(got["y"], fwd["y64"]))}
    for k in KEYS[1:]:
        assert (got[k] is None) == (ref[k] is None), k
        if got[k] is not None:
            err[k] = (rel_l2(got[k], ref[k]), rel_l2(got[k], ref[k + "64"]))
    print(cc.IDS[i], {k: "twin %.2e float64 %.2e" % v for k, v in err.items()})
    for k, (e_twin, e_64) in err.items():
        assert got[k].shape == ref[k].shape and float(ref[k].abs().max()) > 0
        assert e_twin <= BAR and e_64 <= BAR, (cc.IDS[i], k, e_twin, e_64)


@pytest.mark.parametrize("i", range(len(cc.CASES)), ids=cc.IDS)
def test_sign_differs_from_float64_only_next_to_zero(i):
    """The operator's sign of y may differ from float64's only where |pre64| < 1e-5 rms(pre64), and at no more than 0.1 % of
    the elements."""
    differs = (_full(i)["y"].cpu() > 0) != (cc.forward64(i)["pre"] > 0)
    near = cc.near_zero(i)
    print(cc.IDS[i], int(differs.sum()), "signs differ,", int(near.sum()), "elements near zero, of", near.numel())
    assert not bool((differs & ~near).any())
    assert int(differs.sum()) <= cc.SIGN_CAP * differs.numel()


def test_gradient_subsets():
    """Each needs_input_grad combination launches only its kernels (bwd_x once for xa and / or xb, with NULL for the one not
    wanted), and what it returns is bitwise what the full backward returns."""
    from goliath_amd import olatunet

    i = 2
    full = _full(i)
    calls = []
    names = ("_abi_conv3ub_bwd_x", "_abi_conv3ub_bwd_w", "_abi_conv3ub_bwd_bias")
    real = {n: getattr(olatunet, n) for n in names}
    x_outs = lambda kw: tuple(k for k in ("g_xa", "g_xb") if kw.get(k) is not None)
    try:
        for n, fn in real.items():
            setattr(olatunet, n, lambda fn=fn, n=n, **kw: (calls.append((n[len("_abi_conv3ub_"):], x_outs(kw))), fn(**kw))[1])
        for need in ((True, False, False, False), (False, True, False, False), (False, False, True, False),
                     (False, False, False, True), (True, True, False, False), (False, True, True, True)):
            del calls[:]
            got = _run(i, need)
            want_calls = []
            if need[0] or need[1]:
                want_calls.append(("bwd_x", tuple(k for k, n in zip(("g_xa", "g_xb"), need) if n)))
            if need[2]:
                want_calls.append(("bwd_w", ()))
            if need[3]:
                want_calls.append(("bwd_bias", ()))
            assert calls == want_calls, (need, calls)
            assert torch.equal(got["y"], full["y"])
            for k, n in zip(KEYS[1:], need):
                assert (got[k] is None) == (not n), (need, k)
                assert not n or torch.equal(got[k], full[k]), (need, k)
    finally:
        for n, fn in real.items():
            setattr(olatunet, n, fn)
    # the ABI itself: NULL outputs launch nothing and are GOL_OK
    t = _cuda(i)
    d = _dims(i)
    y = full["y"]
    olatunet._abi_conv3ub_bwd_x(**d, packed=_pack(t["w"]), y=y, g_y=t["up"], g_xa=None, g_xb=None)
    olatunet._abi_conv3ub_bwd_w(**d, xa=t["xa"], xb=t["xb"], y=y, g_y=t["up"], g_w=None, scratch=None)
    olatunet._abi_conv3ub_bwd_bias(B=d["B"], Co=d["Co"], H=d["H"], W=d["W"], leak=LEAK, y=y, g_y=t["up"], g_bias=None)
    torch.cuda.synchronize()


def test_return_codes():
    """Unsupported shapes answer GOL_ERR_UNSUPPORTED and invalid calls GOL_ERR_INVALID_ARG before any launch: outputs
    pre-filled with 7.0 stay untouched.  B == 0 is GOL_OK (bwd_w and bwd_bias zero their outputs)."""
    from goliath_amd import _lib, olatunet

    lib = _lib.load()
    i = 6                                                         # (1, 32, 24, 32, 6, 40): two sources
    t = _cuda(i)
    packed = _pack(t["w"])
    seven = lambda ref: torch.full_like(ref, 7.0)
    y, g_xa, g_xb, g_w, g_b = seven(t["up"]), seven(t["xa"]), seven(t["xb"]), seven(t["w"]), seven(t["bias"])
    scratch = torch.full((olatunet.bwd_w_scratch_floats(**_dims(i, leak=False)),), 7.0, device="cuda")
    null, s, c, f = ctypes.c_void_p(0), _lib.stream_ptr(), ctypes.c_int, ctypes.c_float
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    pxa, pxb, pk, pu, pb, py = p(t["xa"]), p(t["xb"]), p(packed), p(t["up"]), p(t["bias"]), p(y)
    dims = lambda B, Ca, Cb, Co, H, W: (c(B), c(Ca), c(Cb), c(Co), c(H), c(W))
    fwd = lambda *d, leak=LEAK, xa=pxa: lib.gol_conv3ub_fwd(*dims(*d), f(leak), xa, pxb, pk, pb, py, s)
    bwd_x = lambda *d, leak=LEAK, xa=pu: lib.gol_conv3ub_bwd_x(*dims(*d), f(leak), pk, py, xa, p(g_xa), p(g_xb), s)
    bwd_w = lambda *d, leak=LEAK, xa=pxa: lib.gol_conv3ub_bwd_w(*dims(*d), f(leak), xa, pxb, py, pu, p(g_w), p(scratch), s)
    bwd_b = lambda B, Co, H, W, leak=LEAK, gy=pu: lib.gol_conv3ub_bwd_bias(c(B), c(Co), c(H), c(W), f(leak), py, gy, p(g_b), s)
    OK, INVALID, UNSUPPORTED = 0, -1, -3
    scr = lib.gol_conv3ub_bwd_w_scratch_floats
    scr.restype = ctypes.c_longlong
    good = cc.CASES[i]
    bad = ((1, 32, 24, 16, 6, 40),        # Co = 16
           (1, 32, 24, 48, 6, 40),        # Co = 48
           (1, 12, 0, 32, 6, 40),         # Ca = 12
           (1, 32, 20, 32, 6, 40),        # Cb = 20
           (1, 56, 8, 32, 6, 40),         # Ca = 56 with a second source
           (1, 0, 32, 32, 6, 40),         # Ca = 0
           (1, 32, 24, 32, 0, 40),        # H = 0
           (1, 32, 24, 32, 6, 0),         # W = 0
           (65536, 32, 24, 32, 6, 40))    # B = 65536 (dims only: nothing is read)
    for fn in (fwd, bwd_x, bwd_w):
        for d in bad:
            assert fn(*d) == UNSUPPORTED, d
        assert b"gol_conv3ub" in lib.gol_last_error()
        assert fn(-1, *good[1:]) == INVALID
        assert fn(*good, leak=0.0) == INVALID
        assert fn(*good, xa=null) == INVALID                      # xa / g_y
    for d in bad:
        assert scr(*dims(*d)) == 0, d
    assert scr(*dims(0, *good[1:])) == 0
    assert scr(*dims(*good)) == cc.bwd_w_blocks(*good) * 9 * 32 * 56 == 12 * 9 * 32 * 56
    assert bwd_b(1, 48, 6, 40) == UNSUPPORTED and bwd_b(1, 32, 0, 40) == UNSUPPORTED and bwd_b(65536, 32, 6, 40) == UNSUPPORTED
    assert bwd_b(-1, 32, 6, 40) == INVALID and bwd_b(1, 32, 6, 40, leak=-1.0) == INVALID and bwd_b(1, 32, 6, 40, gy=null) == INVALID
    assert lib.gol_conv3ub_pack(c(48), c(32), pxa, pk, s) == UNSUPPORTED
    assert lib.gol_conv3ub_pack(c(32), c(12), pxa, pk, s) == UNSUPPORTED
    assert lib.gol_conv3ub_pack(c(32), c(56), null, pk, s) == INVALID
    torch.cuda.synchronize()
    for out in (y, g_xa, g_xb, g_w, g_b, scratch):
        assert bool((out == 7.0).all())                            # nothing was launched
    # B == 0: no kernel; the sums over an empty batch are zeros
    assert fwd(0, *good[1:]) == OK and bwd_x(0, *good[1:]) == OK and bwd_w(0, *good[1:]) == OK and bwd_b(0, 32, 6, 40) == OK
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((g_xa == 7.0).all()) and bool((g_xb == 7.0).all())
    assert bool((g_w == 0.0).all()) and bool((g_b == 0.0).all())
    assert fwd(*good) == OK and bwd_x(*good) == OK and bwd_w(*good) == OK and bwd_b(1, 32, 6, 40) == OK
    torch.cuda.synchronize()
    for out in (y, g_xa, g_xb, g_w, g_b):
        assert not bool((out == 7.0).any()) and float(out.abs().max()) > 0


def test_forward_and_backward_are_bitwise_reproducible():
    """On the K-split case: 101 K blocks, two chunks each, the last one chunk."""
    from goliath_amd import olatunet

    d = _dims(cc.KSPLIT, leak=False)
    assert cc.bwd_w_blocks(*cc.CASES[cc.KSPLIT]) == cc.KSPLIT_BLOCKS
    assert olatunet.bwd_w_scratch_floats(**d) == cc.KSPLIT_BLOCKS * 9 * d["Co"] * (d["Ca"] + d["Cb"])
    a, b = _full(cc.KSPLIT), _run(cc.KSPLIT)
    for k in KEYS:
        assert torch.equal(a[k], b[k]) and float(a[k].abs().max()) > 0, k


def test_no_host_sync_and_graph_replay():
    """The six calls on the caller's buffers: no host synchronisation (sync debug mode "error"), and captured into one graph
    they replay bitwise what the eager calls give, also after new values were written into the same input tensors."""
    from goliath_amd import olatunet

    i = cc.KSPLIT
    d = _dims(i)
    t = _cuda(i)
    Co, Ci = d["Co"], d["Ca"] + d["Cb"]
    scratch = torch.empty(olatunet.bwd_w_scratch_floats(**_dims(i, leak=False)), device="cuda")   # before capture
    packed = torch.empty(olatunet.packed_elems(Co, Ci), device="cuda", dtype=torch.int16)

    def step(y, g_xa, g_xb, g_w, g_b):
        olatunet._abi_conv3ub_pack(Co=Co, Ci=Ci, weight=t["w"], packed=packed)
        olatunet._abi_conv3ub_fwd(**d, xa=t["xa"], xb=t["xb"], packed=packed, bias=t["bias"], y=y)
        olatunet._abi_conv3ub_bwd_x(**d, packed=packed, y=y, g_y=t["up"], g_xa=g_xa, g_xb=g_xb)
        olatunet._abi_conv3ub_bwd_w(**d, xa=t["xa"], xb=t["xb"], y=y, g_y=t["up"], g_w=g_w, scratch=scratch)
        olatunet._abi_conv3ub_bwd_bias(B=d["B"], Co=Co, H=d["H"], W=d["W"], leak=LEAK, y=y, g_y=t["up"], g_bias=g_b)

    buffers = lambda: tuple(torch.empty_like(t[k]) for k in ("up", "xa", "xb", "w", "bias"))
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
    assert all(torch.equal(a, b) for a, b in zip(o1, o0))
    t["xa"].mul_(-0.5)                                     # new values in the SAME tensors
    t["xb"].add_(0.25)
    t["up"].add_(0.25)
    t["w"].mul_(1.5)
    t["bias"].neg_()
    graph.replay()
    step(*o0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(o1, o0)) and all(float(a.abs().max()) > 0 for a in o1)


def test_unet_through_the_operator(monkeypatch):
    """conv3ub_cases.SmallOLATUNet on [2,56,32,32] with a 32-channel joint_feat, fp32 on the GPU: with
    GOLIATH_FUSED_OLATUNET_ALL=1 and precision="bf16x3" all six levels run on conv3_ub_lrelu (the skips and joint_feat as xb),
    and the output, the joint_feat gradient and every parameter gradient are <= 1e-5 from the twin chain accumulated in
    float64; with the default precision the output is bitwise the library path's."""
    from goliath_amd import olatunet

    dec, dec64 = cc.unet().cuda(), cc.unet(torch.float64).cuda()
    x, jf = (v.cuda() for v in cc.unet_inputs())
    taken = []
    op = olatunet.conv3_ub_lrelu

    def spy(xa, xb, w, bias, leak):
        taken.append((xa.shape[1], 0 if xb is None else xb.shape[1], w.shape[0], xa.shape[2], xa.shape[3]))
        return op(xa, xb, w, bias, leak)

    monkeypatch.setattr(olatunet, "conv3_ub_lrelu", spy)
    monkeypatch.setenv("GOLIATH_FUSED_OLATUNET_ALL", "1")
    cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **k: pytest.fail("a concatenation"))
    out, g_jf, grads = cc.unet_run(dec, x, jf, lambda m, a, b: olatunet.forward(m, a, b, "bf16x3"))
    monkeypatch.setattr(torch, "cat", cat)
    assert taken == cc.UNET_SHAPES
    twin = lambda xa, xb, w, bias, leak: olatunet.conv3_ub_lrelu_split_torch(xa, xb, w, bias, leak).to(xa.dtype)
    out_t, g_jf_t, grads_t = cc.unet_run(dec64, x.double(), jf.double(),
                                         lambda m, a, b: olatunet.forward(m, a, b, "bf16x3", op=twin))
    assert set(grads) == set(grads_t) and len(grads) == 6 * 3
    err = {"out": rel_l2(out, out_t), "g_joint_feat": rel_l2(g_jf, g_jf_t),
           **{"grad " + n: rel_l2(grads[n], grads_t[n]) for n in grads}}
    for n, e in err.items():
        print("unet", n, "%.3e" % e)
    assert all(float(g.norm()) > 0 for g in grads_t.values()) and float(g_jf_t.norm()) > 0
    assert max(err.values()) <= BAR, max(err.items(), key=lambda kv: kv[1])
    # the default precision: nothing reaches the operator, and the output is the library path's bits
    # (the library is asked for its deterministic solvers: two runs of the SAME library lines are not bitwise equal otherwise)
    del taken[:]
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            y0 = olatunet.forward(dec, x, jf)
            y1 = olatunet.forward(dec, x, jf, precision="fp32")
            y2 = cc.module_loop(dec, x, jf)
    finally:
        torch.backends.cudnn.deterministic = det
    assert not taken and torch.equal(y0, y1) and torch.equal(y0, y2)


def test_dropin_keyword(monkeypatch):
    """patch_hand_teacher(olat_fused=True, unet_precision="bf16x3") on a shaped stand-in whose second encoder level is a
    Conv3WNUB 32 -> 32 at 8^2 reaches conv3_ub_lrelu once per forward for that admitted shape; the default keyword does not.
    The existing ShapedOLATRGBDecoder (plain nn.Conv2d, 8 channels) falls through to its own lines with unchanged results."""
    import torch.nn as nn

    import urhand_shaped as S
    from goliath_amd import dropin, mvp, olatunet, texdec, urhand

    # the deep-shadow march accumulates with float atomics: one volume, computed once, is replayed to every forward, so that
    # what follows it can be compared bitwise
    march, volume = urhand.deep_shadow, []

    def replayed(*a, **k):
        if not volume:
            volume.append(march(*a, **k))
        return volume[0]

    monkeypatch.setattr(urhand, "deep_shadow", replayed)

    class Twin(S.ShapedOLATRGBDecoder):
        def __init__(self):
            super().__init__(mvp.Raymarcher(200.0), 200.0, seed=0)
            torch.manual_seed(17)
            act = lambda: nn.LeakyReLU(0.2, inplace=True)
            self.enc_layers = nn.ModuleList([nn.Sequential(texdec.Conv3WNUB(14, 32, 16, 16), act()),     # Ca = 14: the library
                                             nn.Sequential(texdec.Conv3WNUB(32, 32, 8, 8), act())])      # the operator
            self.dec_layers = nn.ModuleList([nn.Sequential(texdec.Conv3WNUB(32 + 6, 32, 8, 8), act()),   # Cb = 6: the library
                                             nn.Sequential(texdec.Conv3WNUB(64, 8, 16, 16), act())])     # Co = 8: the library

    Twin.__module__ = S.__name__      # the forward looks its helpers up in the module that defines the class
    inp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in S.teacher_inputs(B=1, L=2).items()}
    taken = []
    op = olatunet.conv3_ub_lrelu
    monkeypatch.setattr(olatunet, "conv3_ub_lrelu", lambda *a: (taken.append(tuple(a[0].shape)), op(*a))[1])
    monkeypatch.delenv("GOLIATH_FUSED_OLATUNET_ALL", raising=False)
    monkeypatch.setattr(olatunet, "DISPATCH", {(32, 0, 32, 8, 8): True})
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            dec = Twin().cuda().eval()
            module = types.SimpleNamespace(OLATRGBDecoder=Twin)
            dropin.patch_hand_teacher(module, olat_fused=True)
            assert getattr(Twin, olatunet.UNET_PRECISION_FLAG) == "fp32"
            plain = dec.forward_rgb(**inp)
            assert not taken
            dropin.patch_hand_teacher(module, olat_fused=True, unet_precision="bf16x3")
            assert getattr(Twin, olatunet.UNET_PRECISION_FLAG) == "bf16x3"
            split = dec.forward_rgb(**inp)
            assert taken == [(2, 32, 8, 8)]
            e = rel_l2(split["primrgb"], plain["primrgb"])
            print("drop-in primrgb", e)
            assert float(plain["primrgb"].abs().max()) > 0 and 0 < e <= 1e-4      # the split level is in the result
            # plain nn.Conv2d levels: nothing to take, even with every supported shape forced
            del taken[:]
            monkeypatch.setenv("GOLIATH_FUSED_OLATUNET_ALL", "1")
            shaped = S.ShapedOLATRGBDecoder(mvp.Raymarcher(200.0), 200.0, seed=0).cuda().eval()
            module = types.SimpleNamespace(OLATRGBDecoder=S.ShapedOLATRGBDecoder)
            try:
                dropin.patch_hand_teacher(module, olat_fused=True)
                want = shaped.forward_rgb(**inp)
                dropin.patch_hand_teacher(module, olat_fused=True, unet_precision="bf16x3")
                got = shaped.forward_rgb(**inp)
            finally:
                del S.ShapedOLATRGBDecoder.forward_rgb
                delattr(S.ShapedOLATRGBDecoder, olatunet.UNET_PRECISION_FLAG)
            assert not taken and set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    finally:
        torch.backends.cudnn.deterministic = det
