"""GPU: the fused front of URHand's FeatEncoderUNet (goliath_amd.featenc: gol_featenc_front_fwd/bwd) against its float64
torch twin and the reference's float64 golden, a whole encoder through `forward` against the library lines, the model
drop-in and the ABI's answers."""
import functools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from scenes import rel_l2
from test_featenc_cpu import golden, golden_grad_names, golden_layers

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# (B, Cx, Cm, Co, H, W).  The kernels work on 8x8 output tiles (16x16 positions of the intermediate), K stages of 16
# intermediate channels, 16-channel output tiles in groups of 4 (12 in the forward above 64 channels).
CASES = [
    (2, 4, 16, 16, 2, 2),       # one output pixel: every 4x4 tap row/col -1 and 2 lands on hpad = 0, most 7x7 taps overhang
    (3, 1, 16, 32, 6, 10),      # Cx = 1 (zero-padded K stage: 49 = 12 x 4 + 1), odd batch
    (2, 3, 32, 48, 14, 6),      # Cx = 3; Co = 48 not a multiple of 32 (a wave without a channel tile); narrow image
    (9, 8, 16, 16, 4, 4),       # Cx = 8 (the wide variant of the w_p gradient); batch above any per-workgroup view count
    (1, 4, 64, 192, 16, 16),    # the model's channels in one 8x8 output tile: all K stages of both GEMMs
    (2, 4, 64, 192, 34, 70),    # the model's channels over many workgroups: output 17x35 crosses 8/16/32 tiles by one and
                                # three; halo regions of neighbouring tiles overlap; the backward's tile walk has a tail
    (1, 4, 32, 64, 66, 130),    # output 33x65: one past 32 and 64 on both axes
    (1, 2, 16, 80, 10, 18),     # 5 channel tiles: the forward's group of 12 is ragged inside a wave, the w_f gradient's
                                # second group of 4 holds one tile
    (1, 5, 16, 208, 18, 4),     # 13 channel tiles: a second forward group with one tile; Cx = 5 (K = 245 = 61 x 4 + 1)
]
IDS = ["x".join(map(str, s)) for s in CASES]
NAMES = ("g_w_p", "g_w_f")
BAR = 1e-5                      # rel-L2 against float64: the project's bar (test_gpu_dispunet.BAR, test_gpu_encoder.py)


def _direction(*shape):
    """A random direction divided by its global norm, times a per-channel magnitude in [0.5, 1.5] (fp32)."""
    v = torch.randn(*shape).double()
    return (v * ((torch.rand(shape[0], 1, 1, 1).double() + 0.5) / v.norm())).float()


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs of case i (CPU, float32) and the float64 twin's output and gradients on them, computed once."""
    from goliath_amd import featenc

    B, Cx, Cm, Co, H, W = CASES[i]
    torch.manual_seed(900 + i)
    x = torch.randn(B, Cx, H, W)
    w_p, w_f = _direction(Cm, Cx, 7, 7), _direction(Co, Cm, 4, 4)
    up = torch.randn(B, Co, H // 2, W // 2)
    x64 = x.double().cuda()
    leaves = [t.double().cuda().requires_grad_(True) for t in (w_p, w_f)]
    y64 = featenc.front_torch(x64, *leaves)
    g64 = torch.autograd.grad((y64 * up.double().cuda()).sum(), leaves)
    return dict(inputs=(x, w_p, w_f), up=up, y=y64.detach().cpu(), grads=[g.cpu() for g in g64])


def _run(case, need=(True, True)):
    from goliath_amd import featenc

    x = case["inputs"][0].cuda()
    leaves = [t.cuda().requires_grad_(n) for t, n in zip(case["inputs"][1:], need)]
    y = featenc.front(x, *leaves)
    wanted = [t for t, n in zip(leaves, need) if n]
    grads = iter(torch.autograd.grad((y * case["up"].cuda()).sum(), wanted)) if wanted else iter(())
    return y.detach(), [next(grads) if n else None for n in need]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_matches_float64(i):
    """y, g_w_p and g_w_f <= 1e-5 rel-L2 against `front_torch` in float64 on the same float32 inputs; no element is
    masked (the operator is linear)."""
    case = _case(i)
    y, grads = _run(case)
    assert tuple(y.shape) == tuple(case["y"].shape)
    err = {"y": rel_l2(y.cpu(), case["y"])}
    for n, a, b in zip(NAMES, grads, case["grads"]):
        assert a.shape == b.shape and float(b.norm()) > 0
        err[n] = rel_l2(a.cpu(), b)
    print(CASES[i], err)
    for n, v in err.items():
        assert v <= BAR, (CASES[i], n, v)


def test_golden_through_the_operator():
    """`front` on the fixture's tensors, the four parameter gradients through `wn_weight`: <= 1e-5 against the float64 run
    of the reference's own layers."""
    from goliath_amd import featenc, tail

    g = golden()
    proj, feat = (m.cuda() for m in golden_layers(torch.float32))
    y = featenc.front(torch.from_numpy(g["x"]).cuda(), tail.wn_weight(proj), tail.wn_weight(feat))
    params = [proj.weight_v, proj.weight_g, feat.weight_v, feat.weight_g]
    grads = torch.autograd.grad((y * torch.from_numpy(g["g_y"]).cuda()).sum(), params)
    err = {"y": rel_l2(y.detach().cpu(), torch.from_numpy(g["y"]))}
    for n, got in zip(golden_grad_names(), grads):
        err[n] = rel_l2(got.cpu(), torch.from_numpy(g["grad." + n]))
    print("golden", err)
    for n, v in err.items():
        assert v <= BAR, (n, v)


@pytest.mark.parametrize("i", [2, 5])
def test_gradient_subsets(i, monkeypatch):
    """With w_proj or w_feat not requiring a gradient the other gradient and y are bitwise unchanged; with neither there is
    no backward launch."""
    from goliath_amd import _lib

    case = _case(i)
    y0, full = _run(case)
    for need in ((True, False), (False, True)):
        y, grads = _run(case, need)
        assert torch.equal(y, y0) and [g is not None for g in grads] == list(need)
        for a, b in zip(grads, full):
            assert a is None or torch.equal(a, b)
    calls = []
    call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), call(name, *a))[1])
    y, grads = _run(case, (False, False))
    assert torch.equal(y, y0) and grads == [None, None] and not y.requires_grad
    assert calls == ["gol_featenc_front_fwd"]


def test_forward_and_backward_are_bitwise_reproducible():
    for i in (4, 5):
        y1, g1 = _run(_case(i))
        y2, g2 = _run(_case(i))
        assert torch.equal(y1, y2)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)


def test_no_host_sync_and_graph_replay():
    """Forward and backward through the C ABI on the caller's buffers: no host synchronisation (sync debug mode "error"), and
    both calls captured into one graph replay bitwise what the eager calls give, also after new values were written into the
    same input tensors."""
    from goliath_amd import featenc

    B, Cx, Cm, Co, H, W = CASES[5]
    dims = dict(B=B, Cx=Cx, Cm=Cm, Co=Co, H=H, W=W)
    x, w_p, w_f = [t.cuda() for t in _case(5)["inputs"]]
    g = _case(5)["up"].cuda()
    scratch = torch.empty(featenc.bwd_scratch_floats(**dims), device="cuda")

    def step(y, outs):
        featenc._abi_featenc_front_fwd(**dims, x=x, w_p=w_p, w_f=w_f, y=y)
        featenc._abi_featenc_front_bwd(**dims, x=x, w_p=w_p, w_f=w_f, g_y=g, g_w_p=outs[0], g_w_f=outs[1], scratch=scratch)

    def buffers():
        return torch.empty_like(g), [torch.empty_like(w_p), torch.empty_like(w_f)]

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
    x.mul_(-0.5)                                           # new values in the SAME tensors
    g.add_(0.25)
    graph.replay()
    step(y0, o0)
    torch.cuda.synchronize()
    assert torch.equal(y1, y0) and all(torch.equal(a, b) for a, b in zip(o1, o0))
    assert float(o1[0].abs().max()) > 0 and float(o1[1].abs().max()) > 0


# ---- a whole encoder through forward ---------------------------------------------------------------------------------------
def test_whole_encoder_operator_against_the_library_lines_in_float64(monkeypatch):
    """FeatEncoderUNet(1, 3, 32, base=16) on [2,4,64,64] in fp32 on the GPU with the front forced onto the operator, against
    the same module's library lines in float64: z, every gb[i] and every parameter's gradient <= 1e-5."""
    from goliath_amd import featenc

    torch.manual_seed(21)
    fe = featenc.FeatEncoderUNet(1, 3, 32, base=16)
    with torch.no_grad():
        for m in fe.modules():
            if isinstance(m, featenc.ConvWN):
                m.weight_g.mul_(torch.rand_like(m.weight_g) + 0.5)
        fe.enc.bias.normal_(0, 0.3)
    x = torch.randn(2, 4, 64, 64)
    fe64 = featenc.FeatEncoderUNet(1, 3, 32, base=16)
    fe64.load_state_dict(fe.state_dict())
    fe64 = fe64.double().cuda()
    fe = fe.cuda()

    def run(module, xin, op):
        z, gb = featenc.forward(module, xin, op=op)
        outs = [z] + list(gb)
        torch.manual_seed(22)
        loss = sum((o * torch.randn(o.shape).to(o)).sum() for o in outs)
        names, params = zip(*module.named_parameters())
        return outs, dict(zip(names, torch.autograd.grad(loss, params)))

    taken = []
    op = featenc.front
    monkeypatch.setattr(featenc, "front", lambda *a: (taken.append(tuple(a[0].shape)), op(*a))[1])
    monkeypatch.setenv("GOLIATH_FUSED_FEATENC_ALL", "1")
    outs, grads = run(fe, x.cuda(), None)
    assert taken == [(2, 4, 64, 64)]
    want, want_grads = run(fe64, x.double().cuda(), False)
    assert len(taken) == 1 and len(outs) == len(want) == 5 and set(grads) == set(want_grads) and len(grads) == 2 * 9 + 3
    for k, (a, b) in enumerate(zip(outs, want)):
        e = rel_l2(a, b)
        print("encoder", "z" if k == 0 else "gb[%d]" % (k - 1), tuple(a.shape), e)
        assert a.shape == b.shape and e <= BAR
    for n in grads:
        e = rel_l2(grads[n], want_grads[n])
        print("encoder grad", n, e)
        assert float(want_grads[n].norm()) > 0 and e <= BAR, n


# ---- through the drop-in ---------------------------------------------------------------------------------------------------
class _StubFeatEnc(nn.Module):
    """The attributes `featenc.forward` walks, sized for the shaped decoder (z: 6 channels, gb[0]: 5 channels at 64^2)."""

    def __init__(self):
        from goliath_amd import featenc

        super().__init__()
        self.proj = featenc.ConvWN(4, 16, 7, 1, 3, bias=False)
        self.feat_mod = nn.ModuleList([featenc.ConvWN(16, 16, 4, 2, 1, bias=False)])
        self.gb_mod = nn.ModuleList([nn.Sequential(featenc.ConvWN(16, 5, 1, 1, 0, bias=False), nn.Upsample(scale_factor=2))])
        self.n_layers = 1
        self.enc = featenc.ConvWN(16, 6, 4, 2, 1)

    def forward(self, x):
        from goliath_amd import featenc

        return featenc.forward(self, x, op=False)


def test_patch_urhand_feat_encoder_drop_in(monkeypatch):
    """dropin.patch_urhand(feat_encoder=True) on the shaped decoder whose feature encoder is a twin-layered stub: the call
    site takes the operator with the flag set and the plain module with it cleared; predictions agree to 1e-5 and the
    encoder's parameter gradients to 1e-4."""
    import urhand_shaped as shaped
    from goliath_amd import dropin, featenc, urhand

    class Twin(shaped.ShapedConvTeacherDecoder):
        def __init__(self):
            super().__init__(seed=0)
            torch.manual_seed(13)
            self.featenc = _StubFeatEnc()

    Twin.__module__ = shaped.__name__   # the forward looks its geometry helpers up in the module that defines the class
    gold = np.load(os.path.join(HERE, "golden", "urhand_model_golden.npz"))
    dec = Twin().cuda().eval()
    depths = [torch.from_numpy(gold[f"urhand_eval_depth{i}"]) for i in range(2)]
    dec.rl = shaped.ReplayRenderLayer(512, 512, depths * 2)     # two forwards, two shadow passes each
    inp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in shaped.urhand_inputs(B=1, L=2).items()}
    module = types.SimpleNamespace(ConvTeacherDecoder=Twin, get_shadow_map=None)
    names, params = zip(*dec.featenc.named_parameters())
    taken, plain_calls = [], []
    op = featenc.front
    monkeypatch.setattr(featenc, "front", lambda *a: (taken.append(tuple(a[0].shape)), op(*a))[1])
    dec.featenc.register_forward_hook(lambda *a: plain_calls.append(1))
    monkeypatch.setenv("GOLIATH_FUSED_FEATENC_ALL", "1")

    def run():
        out = dec(**inp)
        loss = (out["tex"] * torch.linspace(0.5, 1.5, out["tex"].numel(), device="cuda").view(out["tex"].shape)).sum()
        return out, torch.autograd.grad(loss, params)

    try:
        dropin.patch_urhand(module)
        assert Twin.forward is urhand.conv_teacher_decoder_forward and not getattr(Twin, featenc.FEATENC_FLAG)
        plain, g_plain = run()
        assert not taken and plain_calls == [1]
        assert dropin.patch_urhand(module, feat_encoder=True) is module
        assert getattr(Twin, featenc.FEATENC_FLAG) is True
        fused, g_fused = run()
        assert taken == [(1, 4, 64, 64)] and plain_calls == [1]
    finally:
        del Twin.forward
    assert set(fused) == set(plain) and float(plain["tex"].detach().abs().max()) > 0
    for k in ("tex", "interm_features2reg"):
        a, b = (fused[k][0], plain[k][0]) if k == "interm_features2reg" else (fused[k], plain[k])
        e = rel_l2(a, b)
        print("drop-in", k, e)
        assert e <= 1e-5, k
    for n, a, b in zip(names, g_fused, g_plain):
        e = rel_l2(a, b)
        print("drop-in grad", n, e)
        assert float(b.norm()) > 0 and e <= 1e-4, n


# ---- the ABI's answers -----------------------------------------------------------------------------------------------------
def test_abi_answers():
    from goliath_amd import _lib, featenc
    from goliath_amd._lib import c_int, fptr, stream_ptr

    lib = _lib.load()
    OK, INVALID, UNSUPPORTED = 0, -1, -3

    def fwd(B=1, Cx=4, Cm=16, Co=16, H=4, W=6, null_x=False):
        t = [torch.zeros(s, device="cuda") for s in ((max(B, 1), Cx, max(H, 1), max(W, 1)), (Cm, Cx, 7, 7), (Co, Cm, 4, 4),
                                                      (max(B, 1), Co, max(H // 2, 1), max(W // 2, 1)))]
        ptrs = [fptr(q) for q in t]
        if null_x:
            ptrs[0] = fptr(None)
        rc = lib.gol_featenc_front_fwd(c_int(B), c_int(Cx), c_int(Cm), c_int(Co), c_int(H), c_int(W), *ptrs, stream_ptr())
        torch.cuda.synchronize()
        return rc

    assert fwd() == OK
    for bad in (dict(Cx=9), dict(Cm=8), dict(H=5), dict(Co=24), dict(W=0)):
        assert fwd(**bad) == UNSUPPORTED, bad
        assert b"gol_featenc_front" in lib.gol_last_error()
        assert featenc.bwd_scratch_floats(**{**dict(B=1, Cx=4, Cm=16, Co=16, H=4, W=6), **bad}) == 0, bad
    assert fwd(null_x=True) == INVALID
    assert fwd(B=0, null_x=True) == OK                      # B == 0: nothing to do, nothing touched
    # backward: a missing g_y is an invalid argument; B == 0 is OK
    x, w_p, w_f = torch.zeros(1, 4, 4, 6, device="cuda"), torch.zeros(16, 4, 7, 7, device="cuda"), torch.zeros(16, 16, 4, 4, device="cuda")
    g_p, g_f = torch.ones_like(w_p), torch.ones_like(w_f)
    scratch = torch.empty(featenc.bwd_scratch_floats(1, 4, 16, 16, 4, 6), device="cuda")
    null = fptr(None)
    dims = lambda B: (c_int(B), c_int(4), c_int(16), c_int(16), c_int(4), c_int(6))
    rc = lib.gol_featenc_front_bwd(*dims(1), fptr(x), fptr(w_p), fptr(w_f), null, fptr(g_p), fptr(g_f), fptr(scratch), stream_ptr())
    assert rc == INVALID
    rc = lib.gol_featenc_front_bwd(*dims(0), null, null, null, null, fptr(g_p), fptr(g_f), null, stream_ptr())
    torch.cuda.synchronize()
    assert rc == OK and float(g_p.abs().max()) == 0 and float(g_f.abs().max()) == 0


def test_scratch_at_the_models_shape_stays_below_64_mib():
    """A pure host call: the partial sums of both weight gradients at 4 -> 64 -> 192, 1024^2, B = 1 (38.0 MiB), a quarter
    of the 268 MB tensor the operator removes at the most."""
    from goliath_amd import featenc

    n = featenc.bwd_scratch_floats(1, 4, 64, 192, 1024, 1024)
    assert 0 < n * 4 <= 64 * 2 ** 20
    assert n == 9961472
