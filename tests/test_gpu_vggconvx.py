"""GPU: the split-bf16 VGG layer (goliath_amd.perceptual.conv3_relu(precision="bf16x3"): gol_conv3x_pack / gol_conv3x_fwd /
gol_conv3x_bwd_x) against the float64-accumulated split twin on the cases of tests/vggx_cases.py: values, position bytes,
input gradient, the packed layout, the ABI's return codes, reproducibility and graph capture.

The twin splits the same float32 inputs to the same bits, so only the fp32 summation order separates the operator from
it (about 1e-7 expected).  A kernel that truncates instead of rounding, or drops a cross term, lands above BAR = 1e-5."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import vgg_cases as vc
import vggx_cases as vx
from scenes import rel_l2

pytestmark = pytest.mark.gpu


def _dims(x, Co, pool):
    B, Ci, H, W = x.shape
    return tuple(ctypes.c_int(v) for v in (B, Ci, Co, H, W, int(pool)))


def _raw_fwd(x, packed, bias, pool, out=None, pos=None):
    """gol_conv3x_fwd on CUDA tensors: (out, position bytes or None)."""
    from goliath_amd import _lib

    B, _, H, W = x.shape
    Co = bias.shape[0]
    if out is None:
        out = torch.empty((B, Co, H // 2, W // 2) if pool else (B, Co, H, W), device=x.device)
        pos = torch.empty(out.shape, device=x.device, dtype=torch.uint8) if pool else None
    _lib.call("gol_conv3x_fwd", *_dims(x, Co, pool), _lib.fptr(x), _lib.ptr(packed, torch.int16), _lib.fptr(bias),
              _lib.fptr(out), _lib.ptr(pos, torch.uint8), _lib.stream_ptr())
    return out, pos


def _raw_bwd(x, packed, out, pos, g, pool, g_x=None):
    from goliath_amd import _lib

    g_x = torch.empty_like(x) if g_x is None else g_x
    _lib.call("gol_conv3x_bwd_x", *_dims(x, out.shape[1], pool), _lib.ptr(packed, torch.int16), _lib.fptr(out),
              _lib.ptr(pos, torch.uint8), _lib.fptr(g), _lib.fptr(g_x), _lib.stream_ptr())
    return g_x


def _cuda(i):
    from goliath_amd import perceptual

    inp = vx.inputs(i)
    weight = inp["weight"].cuda()
    return inp["x"].cuda(), weight, inp["bias"].cuda(), perceptual.pack_bf16x3(weight)


def test_packed_weight_is_the_split_in_blocks_of_8_by_8():
    """packed = [hi | lo][tap][Co / 8][Ci / 8][8 co][8 ci], bit for bit the round-to-nearest-even split of the twin."""
    from goliath_amd import _lib, perceptual

    weight = vx.inputs(1)["weight"]
    Co, Ci = weight.shape[:2]
    packed = perceptual.pack_bf16x3(weight.cuda()).cpu()
    fn = _lib.load().gol_conv3x_packed_elems
    fn.restype = ctypes.c_longlong
    assert packed.dtype == torch.int16 and packed.numel() == 2 * 9 * Co * Ci == fn(ctypes.c_int(Co), ctypes.c_int(Ci))
    assert fn(ctypes.c_int(16), ctypes.c_int(32)) == 0 and fn(ctypes.c_int(32), ctypes.c_int(48)) == 0
    got = packed.view(2, 9, Co // 8, Ci // 8, 8, 8)
    for plane, part in enumerate(perceptual.split_bf16(weight)):
        want = part.view(torch.int16).view(Co // 8, 8, Ci // 8, 8, 9).permute(4, 0, 2, 1, 3)
        assert torch.equal(got[plane], want)


@pytest.mark.parametrize("i", range(len(vx.CASES)), ids=vx.IDS)
def test_matches_the_split_twin(i):
    """y (or p) and g_x <= 1e-5 rel-L2 against the float64-accumulated split twin under a random upstream gradient, zeroed
    at the twin's kinks."""
    from goliath_amd import perceptual

    _, pool = vx.CASES[i]
    ref = vx.reference(i)
    assert ref["zeroed"] <= vc.ZEROED_CAP
    x, weight, bias, packed = _cuda(i)
    x.requires_grad_(True)
    out = perceptual.conv3_relu(x, weight, bias, pool, precision="bf16x3")
    g_x, = torch.autograd.grad((out * ref["up"].cuda()).sum(), x)
    again = perceptual.conv3_relu(x, weight, bias, pool, precision="bf16x3", packed=packed)
    err = {"out": rel_l2(out, ref["out"]), "g_x": rel_l2(g_x, ref["g_x"])}
    print(vx.IDS[i], err)
    assert tuple(out.shape) == tuple(ref["out"].shape) and float(ref["g_x"].abs().max()) > 0
    assert torch.equal(out, again)
    for n, v in err.items():
        assert v <= vc.BAR, (vx.IDS[i], n, v)


@pytest.mark.parametrize("i", vx.POOLED, ids=[vx.IDS[i] for i in vx.POOLED])
def test_pool_values_and_positions(i):
    """The pooled value equals max_pool2d of the un-pooled HIP output bitwise; the position bytes name an element that
    holds that value, the first maximum wins (a dead window reports 0), and they equal the twin's argmax wherever the
    top two of a window differ by more than KINK."""
    ref = vx.reference(i)
    x, _, bias, packed = _cuda(i)
    y, none = _raw_fwd(x, packed, bias, False)
    p, pos = _raw_fwd(x, packed, bias, True)
    assert none is None and pos.dtype == torch.uint8 and pos.shape == p.shape
    assert torch.equal(p, F.max_pool2d(y, 2))
    win = vc.windows(y.cpu())
    pos_l = pos.cpu().long()
    assert int(pos_l.max()) <= 3
    assert torch.equal(win.gather(-1, pos_l[..., None])[..., 0], p.cpu())
    assert torch.equal(pos_l, win.argmax(-1))
    top = vc.windows(F.relu(ref["pre"])).topk(2, -1).values
    clear = top[..., 0] - top[..., 1] > vc.KINK
    assert float(clear[top[..., 0] > 0].float().mean()) > 0.99     # of the live windows (a dead one has no top two)
    assert torch.equal(pos_l[clear], ref["argmax"][clear])


@pytest.mark.parametrize("i", vx.POOLED[:2], ids=[vx.IDS[i] for i in vx.POOLED[:2]])
def test_rows_and_columns_dropped_by_the_floor_receive_zero(i):
    """With centre-tap weights g_x[r,c] depends on g_pre[r,c] alone: the last odd row / column, which belongs to no window,
    receives exactly 0, and elements of live windows do not."""
    from goliath_amd import perceptual

    x, weight, bias, _ = _cuda(i)
    centre = torch.zeros_like(weight)
    centre[:, :, 1, 1] = weight[:, :, 1, 1] + 0.5
    packed = perceptual.pack_bf16x3(centre)
    p, pos = _raw_fwd(x, packed, bias, True)
    g = torch.randn_like(p) + 3.0
    g_x = _raw_bwd(x, packed, p, pos, g, True)
    H, W = x.shape[2:]
    assert W % 2 == 1 and float(g_x[..., W - 1].abs().max()) == 0.0
    if H % 2 == 1:
        assert float(g_x[:, :, H - 1].abs().max()) == 0.0
    assert float(g_x[:, :, :2 * (H // 2), :2 * (W // 2)].abs().max()) > 0 and int((p > 0).sum()) > 0


def test_return_codes():
    from goliath_amd import _lib

    lib = _lib.load()
    x, weight, bias, packed = _cuda(0)
    y = torch.empty(2, 32, 8, 32, device="cuda")
    pos = torch.empty(2, 32, 4, 16, device="cuda", dtype=torch.uint8)
    null, s = ctypes.c_void_p(0), _lib.stream_ptr()
    c = ctypes.c_int
    px, pw, pk, pb, py, pp = (ctypes.c_void_p(t.data_ptr()) for t in (x, weight, packed, bias, y, pos))

    def fwd(B, Ci, Co, H, W, pool, xs=px, ys=py, ps=pp):
        return lib.gol_conv3x_fwd(c(B), c(Ci), c(Co), c(H), c(W), c(pool), xs, pk, pb, ys, ps, s)

    def bwd(B, Ci, Co, H, W, pool, ys=py, gs=py, ps=pp):
        return lib.gol_conv3x_bwd_x(c(B), c(Ci), c(Co), c(H), c(W), c(pool), pk, ys, ps, gs, px, s)

    OK, INVALID, UNSUPPORTED = 0, -1, -3
    for fn in (fwd, bwd):
        assert fn(2, 48, 32, 8, 32, 0) == UNSUPPORTED          # Ci not a multiple of 32
        assert fn(2, 32, 16, 8, 32, 0) == UNSUPPORTED          # Co not a multiple of 32
        assert fn(2, 3, 32, 8, 32, 0) == UNSUPPORTED           # there is no image layer
        assert fn(2, 32, 32, 1, 32, 1) == UNSUPPORTED          # pool needs H >= 2
        assert fn(2, 32, 32, 8, 1, 1) == UNSUPPORTED           # ... and W >= 2
        assert fn(65536, 32, 32, 8, 32, 0) == UNSUPPORTED      # B > 65535
        assert fn(2, 32, 32, 0, 32, 0) == INVALID
        assert fn(-1, 32, 32, 8, 32, 0) == INVALID
        assert fn(2, 32, 32, 8, 32, 0, null) == INVALID        # x / y
        assert fn(2, 32, 32, 8, 32, 1, px if fn is fwd else py, py, null) == INVALID    # pool without the bytes
        assert fn(0, 32, 32, 8, 32, 0, null, null, null) == OK                          # B = 0: no launch
    assert b"gol_conv3x" in lib.gol_last_error()
    assert lib.gol_conv3x_pack(c(32), c(48), pw, pk, s) == UNSUPPORTED
    assert lib.gol_conv3x_pack(c(32), c(32), null, pk, s) == INVALID
    assert lib.gol_conv3x_pack(c(32), c(32), pw, null, s) == INVALID
    assert fwd(2, 32, 32, 8, 32, 0) == OK and fwd(2, 32, 32, 1, 1, 0) == OK
    torch.cuda.synchronize()


def test_forward_and_backward_are_bitwise_reproducible():
    for i in (1, 3, 5):
        _, pool = vx.CASES[i]
        x, _, bias, packed = _cuda(i)
        out, pos = _raw_fwd(x, packed, bias, pool)
        g = vx.inputs(i)["up"].cuda()
        a = _raw_bwd(x, packed, out, pos, g, pool)
        b = _raw_bwd(x, packed, out, pos, g, pool)
        out2, pos2 = _raw_fwd(x, packed, bias, pool)
        assert torch.equal(a, b) and torch.equal(out, out2) and (pos is None or torch.equal(pos, pos2))
        assert float(a.abs().max()) > 0


def test_graph_capture_replays_to_the_same_bits():
    """A pooled layer's forward and backward captured into one torch.cuda.graph (no host sync, no allocation in the ABI
    calls) replay, on new input values, to the bits of the eager run."""
    from goliath_amd import perceptual

    i = 5
    x, weight, bias, packed = _cuda(i)
    up = vx.inputs(i)["up"].cuda()
    xs = torch.zeros_like(x)
    B, _, H, W = x.shape
    p = torch.empty(B, weight.shape[0], H // 2, W // 2, device="cuda")
    pos = torch.zeros(p.shape, device="cuda", dtype=torch.uint8)
    g_x = torch.zeros_like(x)

    def step():
        _raw_fwd(xs, packed, bias, True, p, pos)
        _raw_bwd(xs, packed, p, pos, up, True, g_x)

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
    pe = perceptual.conv3_relu(xe, weight, bias, pool=True, precision="bf16x3", packed=packed)
    ge, = torch.autograd.grad((pe * up).sum(), xe)
    assert torch.equal(p, pe) and torch.equal(g_x, ge) and float(ge.abs().max()) > 0
