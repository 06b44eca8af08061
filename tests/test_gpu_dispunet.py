"""GPU: the fused DisplacementUNet decoder level (goliath_amd.dispunet: gol_upcat_conv_fwd/bwd) against its float64 torch
twin, the golden's UNet through `forward` against the library lines and the reference's float64 run, the model drop-in and
the ABI's error answers."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from scenes import rel_l2
from test_dispunet_cpu import golden, golden_unet

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# (B, Ca, Cb, Co, Hi, Wi, act)
CASES = [
    (2, 8, 8, 16, 1, 1, 0),        # 2x2 output; every tap overhangs; degenerate axis
    (3, 8, 16, 1, 3, 5, 1),        # Co = 1 head with tanh; Ca != Cb (concat offset); odd batch
    (2, 24, 8, 16, 5, 17, 0),      # Ca not a multiple of 16; W = 34 crosses the 32-column tile by two; H = 10 the 8-row tile
    (1, 72, 40, 32, 6, 6, 0),      # several K stages in both halves; the hand-over from the blended to the plain loader
    (2, 64, 64, 64, 17, 33, 0),    # the model's channel counts over many workgroups; split-K with a tail
    (2, 64, 64, 1, 16, 20, 1),     # the model's head over many tiles
    (9, 8, 8, 4, 3, 2, 1),         # batch above a tile of views; Co = 4; width 2
]
IDS = ["x".join(map(str, s)) for s in CASES]
HEAD = ("tanh", 0.25, 0.55)        # the roughness head: scale and shift both at work
NAMES = ("g_xa", "g_xb", "g_w", "g_bias")
BAR = 1e-5                         # rel-L2 against float64: the bar of test_gpu_texdec.py, test_gpu_trunk.py, test_gpu_encoder.py


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs of case i (CPU, float32) and the float64 twin's output and gradients on them, computed once."""
    from goliath_amd import dispunet

    B, Ca, Cb, Co, Hi, Wi, act = CASES[i]
    torch.manual_seed(700 + i)
    xa = torch.randn(B, Ca, Hi, Wi)
    flat = xa.view(-1)
    flat[::7] = 0.0                                         # exact zeros (the adjoint takes leak there); negatives abound
    xb = torch.randn(B, Cb, 2 * Hi, 2 * Wi)
    weight_v = torch.randn(Co, Ca + Cb, 3, 3)
    weight = (weight_v.double() * ((torch.rand(Co, 1, 1, 1).double() + 0.5) / weight_v.double().norm())).float()
    if act:                                                 # keep the tanh in its sensitive range
        weight = weight * 20.0
    bias = 0.5 * torch.randn(Co, 2 * Hi, 2 * Wi)
    up = torch.randn(B, Co, 2 * Hi, 2 * Wi)
    leaves = [t.double().cuda().requires_grad_(True) for t in (xa, xb, weight, bias)]
    y64 = dispunet.upcat_conv_torch(*leaves, 0.2, HEAD if act else None)
    g64 = torch.autograd.grad((y64 * up.double().cuda()).sum(), leaves)
    assert int((xa == 0).sum()) >= 3 and float(g64[0][(xa == 0).cuda()].abs().max()) > 0
    return dict(inputs=(xa, xb, weight, bias), up=up, act=HEAD if act else None, y=y64.detach().cpu(),
                grads=[g.cpu() for g in g64])


def _run(case, need=(True, True, True, True)):
    from goliath_amd import dispunet

    leaves = [t.cuda().requires_grad_(n) for t, n in zip(case["inputs"], need)]
    y = dispunet.upcat_conv(*leaves, 0.2, case["act"])
    wanted = [t for t, n in zip(leaves, need) if n]
    grads = iter(torch.autograd.grad((y * case["up"].cuda()).sum(), wanted))
    return y.detach(), [next(grads) if n else None for n in need]


def _check(tag, case, y, grads):
    err = {"y": rel_l2(y.cpu(), case["y"])}
    for n, a, b in zip(NAMES, grads, case["grads"]):
        if a is not None:
            err[n] = rel_l2(a.cpu(), b)
    print(tag, err)
    for n, v in err.items():
        assert v <= BAR, (tag, n, v)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_matches_float64(i):
    """y, g_xa, g_xb, g_w and g_bias <= 1e-5 rel-L2 against `upcat_conv_torch` in float64 on the same inputs.  No kink
    masking: the only kink is on the input xa, which is identical on both sides (exact zeros are planted in it)."""
    case = _case(i)
    y, grads = _run(case)
    assert tuple(y.shape) == tuple(case["y"].shape)
    _check(CASES[i], case, y, grads)


@pytest.mark.parametrize("i", [2, 5])
def test_gradient_subsets(i):
    """Each of xa, xb, the weight and the bias not requiring a gradient, one at a time: its output is skipped and the
    remaining gradients are bitwise unchanged."""
    case = _case(i)
    y0, full = _run(case)
    for skip in range(4):
        need = tuple(k != skip for k in range(4))
        y, grads = _run(case, need)
        assert torch.equal(y, y0) and [g is not None for g in grads] == list(need)
        for a, b in zip(grads, full):
            assert a is None or torch.equal(a, b)


def test_backward_is_bitwise_reproducible():
    for i in (4, 5):
        y1, g1 = _run(_case(i))
        y2, g2 = _run(_case(i))
        assert torch.equal(y1, y2)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)


# ---- the golden's UNet through forward ---------------------------------------------------------------------------------
def _kink_margin():
    """Smallest |pre-activation| in front of the decoder's LeakyReLUs in the float64 run of the golden's UNet."""
    unet, g, pre = golden_unet(), golden(), []
    for layer in list(unet.dec_layers[:-1]) + list(unet.dec_layers_roughness[:-1]):
        layer.register_forward_hook(lambda m, i, o: pre.append(float(o.abs().min())))
    with torch.no_grad():
        unet(torch.from_numpy(g["feat_uv"]).double(), torch.from_numpy(g["pose_cond"]).double())
    assert len(pre) == 10
    return min(pre)


def test_stack_operator_equals_library_lines_and_the_float64_golden(monkeypatch):
    """The golden's UNet (64^2, 8 channels, loaded from the fixture) in fp32 on the GPU, every decoder level forced onto the
    operator against DISPATCH = {} without the override: outputs <= 1e-5, every parameter's gradient <= 1e-4 and non-zero,
    ten operator calls against zero; against the reference's float64 run outputs <= 1e-5.  The smallest decoder
    pre-activation of the float64 run is 3.1e-7 (asserted > 1e-7), above the fp32 rounding of these sums (~1e-8 absolute), so
    no leaky mask differs between the paths."""
    from goliath_amd import dispunet

    margin = _kink_margin()
    print("kink margin", margin)
    assert margin > 1e-7
    g = golden()
    unet = golden_unet(torch.float32).cuda()
    feat_uv, pose_cond = torch.from_numpy(g["feat_uv"]).cuda(), torch.from_numpy(g["pose_cond"]).cuda()
    up_d, up_r = torch.from_numpy(g["g_disp"]).cuda(), torch.from_numpy(g["g_roughness"]).cuda()
    names, params = zip(*unet.named_parameters())
    taken = []
    op = dispunet.upcat_conv
    monkeypatch.setattr(dispunet, "upcat_conv", lambda *a: (taken.append(a[5]), op(*a))[1])

    def run():
        disp, rough, interm = dispunet.forward(unet, feat_uv, pose_cond)
        return (disp, rough, interm), torch.autograd.grad((disp * up_d).sum() + (rough * up_r).sum(), params)

    monkeypatch.delenv("GOLIATH_FUSED_DISPUNET_ALL", raising=False)
    monkeypatch.setattr(dispunet, "DISPATCH", {})
    out0, g0 = run()
    assert not taken
    monkeypatch.setenv("GOLIATH_FUSED_DISPUNET_ALL", "1")
    out1, g1 = run()
    assert taken == [None] * 4 + [("tanh", 3.0, 0.0)] + [None] * 4 + [("tanh", 0.25, 0.55)]
    for name, a, b in zip(("disp", "roughness", "interm_feat"), out1, out0):
        e, e64 = rel_l2(a, b), rel_l2(a.cpu(), torch.from_numpy(g[name]))
        print("stack", name, e, "against float64", e64)
        assert a.shape == b.shape and e <= 1e-5 and e64 <= 1e-5, name
    for n, a, b in zip(names, g1, g0):
        assert float(b.norm()) > 0 and float(a.norm()) > 0, n
        e = rel_l2(a, b)
        print("stack grad", n, e, "against float64", rel_l2(a.cpu(), torch.from_numpy(g["grad." + n])))
        assert e <= 1e-4, n


# ---- through the drop-in ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("texture_decoder", [False, True], ids=["alone", "with_texture_decoder"])
def test_patch_urhand_displacement_unet_drop_in(monkeypatch, texture_decoder):
    """dropin.patch_urhand(displacement_unet=True) on the shaped decoder whose refiner is the twin (64^2, 8 channels:
    8 + 8 -> 8 at 2^2 -> 4^2 ... 8 + 8 -> 1 at 32^2 -> 64^2 in both branches): the patched forward reproduces the unpatched
    predictions and the refiner's leaf gradients, with the dispatch table as committed and with every level forced; with
    texture_decoder=True as well the two flags compose."""
    import urhand_shaped as shaped
    from goliath_amd import dispunet, dropin, texdec, urhand

    class Twin(shaped.ShapedConvTeacherDecoder):
        def __init__(self):
            super().__init__(seed=0)
            torch.manual_seed(12)
            self.init_uv_size = 2
            self.geo_refiner = dispunet.DisplacementUNet(64, 2, 1.5, 4, [8] * 6)
            self.joint_conv_block_tex = nn.Conv2d(8 + 4 + 3, 8, 3, padding=1)
            self.featenc.z, self.featenc.gb = nn.Conv2d(4, 8, 3, padding=1), nn.Conv2d(4, 16, 3, padding=1)
            self.texmod0 = nn.ModuleList([texdec.Conv3WNUB(8, 16, 64, 64), texdec.Conv3WNUB(16, 4, 128, 128)])
            self.texmod1 = nn.ModuleList([texdec.Conv3WN(8, 16), texdec.Conv3WN(16, 4)])
            with torch.no_grad():
                for m in list(self.texmod0) + [l for ls in self.geo_refiner.children() for l in ls]:
                    m.bias.normal_(0, 0.3)

    Twin.__module__ = shaped.__name__   # the forward looks its geometry helpers up in the module that defines the class
    gold = np.load(os.path.join(HERE, "golden", "urhand_model_golden.npz"))
    dec = Twin().cuda().eval()
    depths = [torch.from_numpy(gold[f"urhand_eval_depth{i}"]) for i in range(2)]
    dec.rl = shaped.ReplayRenderLayer(512, 512, depths * 3)     # three forwards, two shadow passes each
    inp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in shaped.urhand_inputs(B=1, L=2).items()}
    module = types.SimpleNamespace(ConvTeacherDecoder=Twin, get_shadow_map=None)
    names, params = zip(*dec.geo_refiner.named_parameters())
    taken, tex_taken = [], []
    op, lrelu, gated = dispunet.upcat_conv, texdec.upconv_lrelu, texdec.upconv_gated
    monkeypatch.setattr(dispunet, "upcat_conv", lambda *a: (taken.append(1), op(*a))[1])
    monkeypatch.setattr(texdec, "upconv_lrelu", lambda *a: (tex_taken.append(0), lrelu(*a))[1])
    monkeypatch.setattr(texdec, "upconv_gated", lambda *a: (tex_taken.append(1), gated(*a))[1])
    monkeypatch.delenv("GOLIATH_FUSED_DISPUNET_ALL", raising=False)
    monkeypatch.setenv("GOLIATH_FUSED_TEXDEC_ALL", "1")
    keys = ("tex", "displacement", "roughness", "verts_displaced", "id_pose_conv")

    def run():
        out = dec(**inp)
        loss = sum((out[k] * torch.linspace(0.5, 1.5, out[k].numel(), device="cuda").view(out[k].shape)).sum()
                   for k in ("tex", "displacement", "roughness"))
        return out, torch.autograd.grad(loss, params)

    try:
        dropin.patch_urhand(module, texture_decoder=texture_decoder)
        assert Twin.forward is urhand.conv_teacher_decoder_forward and not getattr(Twin, dispunet.DISPLACEMENT_UNET_FLAG)
        plain, g_plain = run()
        assert not taken
        assert dropin.patch_urhand(module, texture_decoder=texture_decoder, displacement_unet=True) is module
        assert getattr(Twin, dispunet.DISPLACEMENT_UNET_FLAG) is True
        assert getattr(Twin, texdec.TEXTURE_DECODER_FLAG) is texture_decoder
        committed, g_committed = run()
        n_committed = len(taken)
        monkeypatch.setenv("GOLIATH_FUSED_DISPUNET_ALL", "1")
        forced, g_forced = run()
    finally:
        del Twin.forward
    assert n_committed <= 10 and len(taken) == n_committed + 10
    assert len(tex_taken) == (9 if texture_decoder else 0)       # texmod0[1], texmod1[0] and texmod1[1], three forwards
    assert float(plain["tex"].abs().max()) > 0 and float(plain["displacement"].abs().max()) > 0
    for out, grads in ((committed, g_committed), (forced, g_forced)):
        assert set(out) == set(plain)
        for k in keys:
            e = rel_l2(out[k], plain[k])
            print("drop-in", k, e)
            assert e <= 1e-5, k
        errs = {n: rel_l2(a, b) for n, a, b in zip(names, grads, g_plain)}
        print("drop-in grads, worst", max(errs.items(), key=lambda kv: kv[1]))
        for (n, e), b in zip(errs.items(), g_plain):
            assert float(b.norm()) > 0 and e <= 1e-4, n


# ---- the ABI's error answers ---------------------------------------------------------------------------------------------
def test_abi_errors_and_empty_batch():
    from goliath_amd import _lib
    from goliath_amd._lib import c_float, c_int, fptr, stream_ptr

    lib = _lib.load()
    OK, INVALID, UNSUPPORTED = 0, -1, -3

    def tensors(B, Ca, Cb, Co, Hi=2, Wi=3):
        return [torch.zeros(s, device="cuda") for s in ((max(B, 1), max(Ca, 1), Hi, Wi), (max(B, 1), max(Cb, 1), 2 * Hi, 2 * Wi),
                                                         (Co, max(Ca + Cb, 1), 3, 3), (Co, 2 * Hi, 2 * Wi),
                                                         (max(B, 1), Co, 2 * Hi, 2 * Wi))]

    def fwd(B, Ca, Cb, Co, ptrs=None, Hi=2, Wi=3, act=0):
        t = tensors(B, Ca, Cb, Co, Hi, Wi)
        ptrs = [fptr(q) for q in t] if ptrs is None else [fptr(q) if keep else fptr(None) for q, keep in zip(t, ptrs)]
        rc = lib.gol_upcat_conv_fwd(c_int(B), c_int(Ca), c_int(Cb), c_int(Co), c_int(Hi), c_int(Wi), c_int(act), c_float(0.2),
                                    c_float(1.0), c_float(0.0), *ptrs, stream_ptr())
        torch.cuda.synchronize()
        return rc, t[4]

    assert fwd(1, 8, 8, 16)[0] == OK
    for Ca, Cb, Co in ((12, 8, 16), (8, 0, 16), (8, 12, 16), (8, 8, 5), (8, 8, 20)):
        assert fwd(1, Ca, Cb, Co)[0] == UNSUPPORTED, (Ca, Cb, Co)
        assert b"gol_upcat_conv" in lib.gol_last_error()
    assert fwd(65536, 8, 8, 16, ptrs=[False] * 5)[0] == UNSUPPORTED              # B above the grid limit, before any access
    for k in range(5):
        assert fwd(1, 8, 8, 16, ptrs=[j != k for j in range(5)])[0] == INVALID, k
    assert fwd(1, 8, 8, 16, Hi=0)[0] == INVALID and fwd(1, 8, 8, 16, act=2)[0] == INVALID
    assert fwd(0, 8, 8, 16, ptrs=[False] * 5)[0] == OK                           # B == 0: nothing to do, nothing touched
    # backward: g_y missing is an invalid argument; B == 0 zeroes the sums it is asked for
    dims = lambda B: (c_int(B), c_int(8), c_int(8), c_int(16), c_int(2), c_int(3), c_int(0), c_float(0.2), c_float(1.0), c_float(0.0))
    xa, xb, w, bias, y = tensors(1, 8, 8, 16)
    g_w, g_b = torch.ones_like(w), torch.ones_like(bias)
    null = fptr(None)
    rc = lib.gol_upcat_conv_bwd(*dims(1), fptr(xa), fptr(xb), fptr(w), null, null, null, null, null, fptr(g_b), null, stream_ptr())
    assert rc == INVALID
    rc = lib.gol_upcat_conv_bwd(*dims(0), null, null, null, null, null, null, null, fptr(g_w), fptr(g_b), null, stream_ptr())
    torch.cuda.synchronize()
    assert rc == OK and float(g_w.abs().max()) == 0 and float(g_b.abs().max()) == 0
    fn = lib.gol_upcat_conv_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    assert fn(*dims(0)[:6]) == 0 and fn(*dims(1)[:6]) == 2 * 1 * 9 * 256          # (1 co tile) x (1 + 1 ci tiles) x 1 K block


# ---- no host sync, capturable as a linear graph ----------------------------------------------------------------------------
def test_no_host_sync_and_graph_replay():
    """Forward and backward through the C ABI on the caller's buffers: no host synchronisation (sync debug mode "error"), and
    both calls captured into one graph replay bitwise what the eager calls give, also after new values were written into the
    same input tensors."""
    from goliath_amd import _lib
    from goliath_amd._lib import c_float, c_int, fptr, stream_ptr

    B, Ca, Cb, Co, Hi, Wi, _ = CASES[5]
    dims = (c_int(B), c_int(Ca), c_int(Cb), c_int(Co), c_int(Hi), c_int(Wi), c_int(1), c_float(0.2), c_float(HEAD[1]),
            c_float(HEAD[2]))
    xa, xb, w, bias = [t.cuda() for t in _case(5)["inputs"]]
    g = _case(5)["up"].cuda()
    fn = _lib.load().gol_upcat_conv_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    scratch = torch.empty(int(fn(*dims[:6])), device="cuda")

    def step(y, outs):
        _lib.call("gol_upcat_conv_fwd", *dims, fptr(xa), fptr(xb), fptr(w), fptr(bias), fptr(y), stream_ptr())
        _lib.call("gol_upcat_conv_bwd", *dims, fptr(xa), fptr(xb), fptr(w), fptr(y), fptr(g), *[fptr(o) for o in outs],
                  fptr(scratch), stream_ptr())

    def buffers():
        return torch.empty_like(g), [torch.empty_like(t) for t in (xa, xb, w, bias)]

    y0, o0 = buffers()
    step(y0, o0)                                           # (first call: code objects)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step(y0, o0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    y1, o1 = buffers()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(y1, o1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y1, y0) and all(torch.equal(a, b) for a, b in zip(o1, o0))
    xa.mul_(-0.5)                                          # new values in the SAME tensors
    g.add_(0.25)
    graph.replay()
    step(y0, o0)
    torch.cuda.synchronize()
    assert torch.equal(y1, y0) and all(torch.equal(a, b) for a, b in zip(o1, o0))
    assert float(o1[0].abs().max()) > 0
