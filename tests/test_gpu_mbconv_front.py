"""GPU: the fused MBConv front (goliath_amd.effnet.mbconv_front: gol_mbconv_front_fwd / gol_mbconv_front_bwd_x) against its
float64 torch twin on the cases of tests/effnet_cases.py, each gradient path alone, reproducibility, the ABI's return codes
and the empty batch."""
import ctypes

import pytest
import torch

import effnet_cases as ec

pytestmark = pytest.mark.gpu


def _run(i, g_z=True, g_ssum=True):
    """(z, ssum, g_x) of case i from the HIP operator."""
    from goliath_amd import effnet

    inp = ec.inputs(i)
    c = lambda t: None if t is None else t.cuda()
    x = inp["x"].cuda().requires_grad_(True)
    z, ssum = effnet.mbconv_front(x, c(inp["w_e"]), c(inp["b_e"]), c(inp["w_d"]), c(inp["b_d"]), inp["k"], inp["stride"])
    up = (z * inp["g_z"].cuda()).sum() * float(g_z) + (ssum * inp["g_ssum"].cuda()).sum() * float(g_ssum)
    g_x, = torch.autograd.grad(up, x)
    return z.detach(), ssum.detach(), g_x


@pytest.mark.parametrize("i", range(len(ec.CASES)), ids=ec.IDS)
def test_matches_float64(i):
    """z, ssum and g_x <= 1e-5 rel-L2 against the float64 twin, nothing excluded; two runs are bitwise equal."""
    ref = ec.reference(i)
    got = _run(i)
    err = dict(zip(("z", "ssum", "g_x"), (ec.rel(a, b) for a, b in zip(got, ref))))
    print(ec.IDS[i], err)
    assert all(a.shape == b.shape and a.dtype == torch.float32 for a, b in zip(got, ref))
    assert float(ref[2].abs().max()) > 0
    for n, v in err.items():
        assert v <= ec.BAR, (ec.IDS[i], n, v)
    again = _run(i)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("i", range(len(ec.CASES)), ids=ec.IDS)
def test_each_gradient_path_alone(i):
    """g_x with g_ssum = 0 (the transposed depthwise of g_z alone) and with g_z = 0 (the squeeze's SiLU'(z) term alone)."""
    for g_z, g_ssum in ((True, False), (False, True)):
        want = ec.reference(i, g_z, g_ssum)[2]
        got = _run(i, g_z, g_ssum)[2]
        err = ec.rel(got, want)
        print(ec.IDS[i], "g_z" if g_z else "g_ssum", err)
        assert float(want.abs().max()) > 0 and err <= ec.BAR


def test_unsupported_arguments_through_the_binding():
    from goliath_amd import _lib, effnet

    x = torch.randn(1, 16, 9, 9, device="cuda")

    def call(Ci, Ce, k, stride):
        xx = torch.randn(1, Ci, 9, 9, device="cuda")
        args = (torch.randn(Ce, Ci, device="cuda"), torch.zeros(Ce, device="cuda"), torch.randn(Ce, k, k, device="cuda"),
                torch.zeros(Ce, device="cuda"))
        return effnet.mbconv_front(xx, *args, k, stride)

    for bad in ((16, 32, 7, 1), (16, 32, 3, 3), (12, 32, 3, 1), (16, 24, 3, 1)):
        with pytest.raises(_lib.GoliathHipError, match=r"gol_mbconv_front_fwd failed \(-3\)"):
            call(*bad)
    with pytest.raises(_lib.GoliathHipError, match=r"failed \(-3\)"):      # no expand needs Ci == Ce
        effnet.mbconv_front(x, None, None, torch.randn(32, 3, 3, device="cuda"), torch.zeros(32, device="cuda"), 3, 1)
    z, ssum = call(16, 32, 3, 1)
    assert tuple(z.shape) == (1, 32, 9, 9) and tuple(ssum.shape) == (1, 32)


def test_return_codes():
    from goliath_amd import _lib

    lib = _lib.load()
    inp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in ec.inputs(1).items()}      # 2 x 16 -> 96, 9 x 35, k3 s2
    z = torch.empty(2, 96, 5, 18, device="cuda")
    g_x = torch.empty(2, 16, 9, 35, device="cuda")
    assert lib.gol_mbconv_front_tiles(9, 35, 3, 2) == 2 and lib.gol_mbconv_front_tiles(9, 35, 7, 2) == 0
    part = torch.empty(2, 96, 2, device="cuda", dtype=torch.float64)
    null, s, c = ctypes.c_void_p(0), _lib.stream_ptr(), ctypes.c_int
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    px, pwe, pbe, pwd, pbd, pz, pp, pgz, pgs, pgx = (P(t) for t in (inp["x"], inp["w_e"], inp["b_e"], inp["w_d"], inp["b_d"], z,
                                                                    part, inp["g_z"], inp["g_ssum"], g_x))

    def fwd(B, Ci, Ce, H, W, k, st, ex, xs=px, zs=pz, ps=pp):
        return lib.gol_mbconv_front_fwd(c(B), c(Ci), c(Ce), c(H), c(W), c(k), c(st), c(ex), xs, pwe, pbe, pwd, pbd, zs, ps, s)

    def bwd(B, Ci, Ce, H, W, k, st, ex, xs=px, zs=pz, gs=pgs):
        return lib.gol_mbconv_front_bwd_x(c(B), c(Ci), c(Ce), c(H), c(W), c(k), c(st), c(ex), xs, pwe, pbe, pwd, zs, pgz, gs,
                                          pgx, s)

    OK, INVALID, UNSUPPORTED = 0, -1, -3
    for fn in (fwd, bwd):
        assert fn(2, 16, 96, 9, 35, 7, 2, 1) == UNSUPPORTED
        assert fn(2, 16, 96, 9, 35, 3, 3, 1) == UNSUPPORTED
        assert fn(2, 12, 96, 9, 35, 3, 2, 1) == UNSUPPORTED
        assert fn(2, 16, 24, 9, 35, 3, 2, 1) == UNSUPPORTED
        assert fn(2, 16, 96, 9, 35, 3, 2, 0) == UNSUPPORTED        # no expand needs Ci == Ce
        assert fn(65536, 16, 96, 9, 35, 3, 2, 1) == UNSUPPORTED
        assert fn(2, 16, 96, 0, 35, 3, 2, 1) == INVALID
        assert fn(-1, 16, 96, 9, 35, 3, 2, 1) == INVALID
        assert fn(2, 16, 96, 9, 35, 3, 2, 1, null) == INVALID
        assert fn(2, 16, 96, 9, 35, 3, 2, 1, px, null) == INVALID
        assert fn(2, 16, 96, 9, 35, 3, 2, 1, px, pz, null) == INVALID
        assert fn(0, 16, 96, 9, 35, 3, 2, 1, null, null, null) == OK       # B = 0: no launch
    assert b"gol_mbconv_front" in lib.gol_last_error()
    assert fwd(2, 16, 96, 9, 35, 3, 2, 1) == OK and bwd(2, 16, 96, 9, 35, 3, 2, 1) == OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(g_x).all())


def test_empty_batch():
    from goliath_amd import effnet

    inp = ec.inputs(3)
    x = torch.zeros(0, 24, 17, 34, device="cuda", requires_grad=True)
    z, ssum = effnet.mbconv_front(x, inp["w_e"].cuda(), inp["b_e"].cuda(), inp["w_d"].cuda(), inp["b_d"].cuda(), 5, 2)
    assert tuple(z.shape) == (0, 144, 9, 17) and tuple(ssum.shape) == (0, 144)
    g_x, = torch.autograd.grad(z.sum() + ssum.sum(), x)
    assert tuple(g_x.shape) == tuple(x.shape)
