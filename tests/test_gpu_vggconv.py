"""GPU: the fused VGG layer (goliath_amd.perceptual.conv3_relu: gol_conv3_fwd / gol_conv3_bwd_x) against its float64 torch
twin on the cases of tests/vgg_cases.py, the pool's values and position bytes, the ABI's return codes, reproducibility and
graph capture."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import vgg_cases as vc
from scenes import rel_l2

pytestmark = pytest.mark.gpu


def _args(x, weight, pool, image_in):
    from goliath_amd import perceptual

    return perceptual._dims(x, weight, pool, image_in)


def _raw_fwd(x, weight, bias, pool, image_in):
    """gol_conv3_fwd on CUDA tensors: (out, position bytes or None)."""
    from goliath_amd import _lib

    B, _, H, W = x.shape
    out = torch.empty((B, weight.shape[0], H // 2, W // 2) if pool else (B, weight.shape[0], H, W), device=x.device)
    pos = torch.empty(out.shape, device=x.device, dtype=torch.uint8) if pool else None
    _lib.call("gol_conv3_fwd", *_args(x, weight, pool, image_in), _lib.fptr(x), _lib.fptr(weight), _lib.fptr(bias),
              _lib.fptr(out), _lib.ptr(pos, torch.uint8), _lib.stream_ptr())
    return out, pos


def _raw_bwd(x, weight, out, pos, g, pool, image_in, g_x=None):
    from goliath_amd import _lib

    g_x = torch.empty_like(x) if g_x is None else g_x
    _lib.call("gol_conv3_bwd_x", *_args(x, weight, pool, image_in), _lib.fptr(x), _lib.fptr(weight), _lib.fptr(out),
              _lib.ptr(pos, torch.uint8), _lib.fptr(g), _lib.fptr(g_x), _lib.stream_ptr())
    return g_x


def _cuda(i):
    inp = vc.inputs(i)
    return inp["x"].cuda(), inp["weight"].cuda(), inp["bias"].cuda()


@pytest.mark.parametrize("i", range(len(vc.CASES)), ids=vc.IDS)
def test_matches_float64(i):
    """y (or p) and g_x <= 1e-5 rel-L2 against the float64 twin under a random upstream gradient, zeroed at the twin's kinks
    (the fp32 library convolution itself is off float64 by at most 2.8e-6 absolute on these cases)."""
    from goliath_amd import perceptual

    _, pool, image_in = vc.CASES[i]
    ref = vc.reference(i)
    print("zeroed", ref["zeroed"])
    assert ref["zeroed"] <= vc.ZEROED_CAP
    x, weight, bias = _cuda(i)
    x.requires_grad_(True)
    out = perceptual.conv3_relu(x, weight, bias, pool, image_in)
    g_x, = torch.autograd.grad((out * ref["up"].cuda()).sum(), x)
    err = {"out": rel_l2(out, ref["out"]), "g_x": rel_l2(g_x, ref["g_x"])}
    print(vc.IDS[i], err)
    assert tuple(out.shape) == tuple(ref["out"].shape) and float(ref["g_x"].abs().max()) > 0
    for n, v in err.items():
        assert v <= vc.BAR, (vc.IDS[i], n, v)


@pytest.mark.parametrize("i", vc.POOLED, ids=[vc.IDS[i] for i in vc.POOLED])
def test_pool_values_and_positions(i):
    """The pooled value equals max_pool2d of the un-pooled HIP output bitwise; the position bytes name an element that
    holds that value, equal the float64 twin's argmax outside the zeroed windows, and a dead window reports position 0."""
    ref = vc.reference(i)
    x, weight, bias = _cuda(i)
    image_in = vc.CASES[i][2]
    y, none = _raw_fwd(x, weight, bias, False, image_in)
    p, pos = _raw_fwd(x, weight, bias, True, image_in)
    assert none is None and pos.dtype == torch.uint8 and pos.shape == p.shape
    assert torch.equal(p, F.max_pool2d(y, 2))
    win = vc.windows(y.cpu())
    pos_l = pos.cpu().long()
    assert int(pos_l.max()) <= 3
    assert torch.equal(win.gather(-1, pos_l[..., None])[..., 0], p.cpu())
    assert torch.equal(pos_l, win.argmax(-1))                # the first maximum wins a tie (all-zero windows: 0)
    safe = ~ref["unsafe"]
    assert float(safe.float().mean()) > 0.99
    assert torch.equal(pos_l[safe], ref["argmax"][safe])


@pytest.mark.parametrize("i", vc.POOLED[:2], ids=[vc.IDS[i] for i in vc.POOLED[:2]])
def test_rows_and_columns_dropped_by_the_floor_receive_zero(i):
    """With centre-tap weights g_x[r,c] depends on g_pre[r,c] alone: the last odd row / column, which belongs to no window,
    receives exactly 0, and elements of live windows do not."""
    x, weight, bias = _cuda(i)
    centre = torch.zeros_like(weight)
    centre[:, :, 1, 1] = weight[:, :, 1, 1] + 0.5
    p, pos = _raw_fwd(x, centre, bias, True, False)
    g = torch.randn_like(p) + 3.0
    g_x = _raw_bwd(x, centre, p, pos, g, True, False)
    H, W = x.shape[2:]
    assert W % 2 == 1 and float(g_x[..., W - 1].abs().max()) == 0.0
    if H % 2 == 1:
        assert float(g_x[:, :, H - 1].abs().max()) == 0.0
    assert float(g_x[:, :, :2 * (H // 2), :2 * (W // 2)].abs().max()) > 0 and int((p > 0).sum()) > 0


def test_return_codes():
    from goliath_amd import _lib

    lib = _lib.load()
    x, weight, bias = _cuda(1)
    y = torch.empty(2, 16, 8, 32, device="cuda")
    pos = torch.empty(2, 16, 4, 16, device="cuda", dtype=torch.uint8)
    null, s = ctypes.c_void_p(0), _lib.stream_ptr()
    c = ctypes.c_int
    px, pw, pb, py, pp = (ctypes.c_void_p(t.data_ptr()) for t in (x, weight, bias, y, pos))

    def fwd(B, Ci, Co, H, W, img, pool, xs=px, ys=py, ps=pp):
        return lib.gol_conv3_fwd(c(B), c(Ci), c(Co), c(H), c(W), c(img), c(pool), xs, pw, pb, ys, ps, s)

    def bwd(B, Ci, Co, H, W, img, pool, xs=px, gs=py, ps=pp):
        return lib.gol_conv3_bwd_x(c(B), c(Ci), c(Co), c(H), c(W), c(img), c(pool), xs, pw, py, ps, gs, px, s)

    OK, INVALID, UNSUPPORTED = 0, -1, -3
    for fn in (fwd, bwd):
        assert fn(2, 12, 16, 8, 32, 0, 0) == UNSUPPORTED        # Ci not a multiple of 8
        assert fn(2, 3, 16, 8, 32, 0, 0) == UNSUPPORTED         # Ci = 3 is the image input only
        assert fn(2, 8, 16, 8, 32, 1, 0) == UNSUPPORTED         # image input needs Ci = 3
        assert fn(2, 8, 24, 8, 32, 0, 0) == UNSUPPORTED         # Co not a multiple of 16
        assert fn(2, 8, 16, 1, 32, 0, 1) == UNSUPPORTED         # pool needs H >= 2
        assert fn(2, 8, 16, 8, 1, 0, 1) == UNSUPPORTED          # ... and W >= 2
        assert fn(65536, 8, 16, 8, 32, 0, 0) == UNSUPPORTED     # B > 65535
        assert fn(2, 8, 16, 0, 32, 0, 0) == INVALID
        assert fn(-1, 8, 16, 8, 32, 0, 0) == INVALID
        assert fn(2, 8, 16, 8, 32, 0, 0, null) == (INVALID if fn is fwd else OK)    # the backward reads x with image_in only
        assert fn(2, 8, 16, 8, 32, 0, 1, px, py, null) == INVALID                   # pool without the bytes
        assert fn(0, 8, 16, 8, 32, 0, 0, null, null, null) == OK                    # B = 0: no launch
    assert fwd(2, 8, 16, 8, 32, 0, 0, px, null) == INVALID
    assert bwd(2, 8, 16, 8, 32, 0, 0, px, null) == INVALID
    assert b"gol_conv3" in lib.gol_last_error()
    assert fwd(2, 8, 16, 8, 32, 0, 0) == OK and fwd(2, 8, 16, 1, 1, 0, 0) == OK
    torch.cuda.synchronize()


def test_backward_is_bitwise_reproducible():
    for i in (0, 4, 5):
        _, pool, image_in = vc.CASES[i]
        x, weight, bias = _cuda(i)
        out, pos = _raw_fwd(x, weight, bias, pool, image_in)
        g = vc.inputs(i)["up"].cuda()
        a = _raw_bwd(x, weight, out, pos, g, pool, image_in)
        b = _raw_bwd(x, weight, out, pos, g, pool, image_in)
        out2, pos2 = _raw_fwd(x, weight, bias, pool, image_in)
        assert torch.equal(a, b) and torch.equal(out, out2) and (pos is None or torch.equal(pos, pos2))
        assert float(a.abs().max()) > 0


def test_graph_capture_replays_to_the_same_bits():
    """A pooled layer's forward and backward captured into one torch.cuda.graph (no host sync, no allocation in the ABI
    calls) replay, on new input values, to the bits of the eager run."""
    from goliath_amd import perceptual

    i = 5
    x, weight, bias = _cuda(i)
    up = vc.inputs(i)["up"].cuda()
    xs = torch.zeros_like(x)
    B, _, H, W = x.shape
    p = torch.empty(B, weight.shape[0], H // 2, W // 2, device="cuda")
    pos = torch.zeros(p.shape, device="cuda", dtype=torch.uint8)
    g_x = torch.zeros_like(x)

    def step():
        from goliath_amd import _lib

        _lib.call("gol_conv3_fwd", *_args(xs, weight, True, False), _lib.fptr(xs), _lib.fptr(weight), _lib.fptr(bias),
                  _lib.fptr(p), _lib.ptr(pos, torch.uint8), _lib.stream_ptr())
        _raw_bwd(xs, weight, p, pos, up, True, False, g_x)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    xs.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    xe = x.clone().requires_grad_(True)
    pe = perceptual.conv3_relu(xe, weight, bias, pool=True)
    ge, = torch.autograd.grad((pe * up).sum(), xe)
    assert torch.equal(p, pe) and torch.equal(g_x, ge) and float(ge.abs().max()) > 0
