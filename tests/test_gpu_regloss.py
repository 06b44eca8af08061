"""GPU: the fused regularisers of goliath_amd.losses (csrc/regloss.hip) against tests/golden/regloss_golden.npz, which
holds each case's inputs, the reference's own function on them in float64 and the same in float32 on the CPU
(tests/golden/make_regloss_golden.py).

Parity bound, per loss and per gradient element, nothing excluded:
    |hip - f64| <= 2 |f32 - f64| + 4 eps32 |f64|
(twice the reference's own float32 deviation plus four float32 roundings of the value itself; the magnitude is the
element's own for gradients).  The largest error / bound ratio of every case goes to regloss_parity.json in the directory
GOLIATH_PARITY_DIR names (profiles/regloss_parity.json is a copy of one such run)."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS32 = float(np.finfo(np.float32).eps)
UNARY = ("bound_primscale", "negcolor", "l2_reg", "list_l1_reg", "alphaprior")
UNARY_TAGS = ("n1", "n3", "n4", "n4095", "n4097", "n12293", "real")
BACKLIT_TAGS = ("one", "rows1023", "rows1025", "c1", "c4", "allpos")
KEYS = {"bound_primscale": "primscale_preclip", "negcolor": "diff_color", "l2_reg": "spec_dnml", "list_l1_reg": "spec_dnml",
        "alphaprior": "alpha"}
WEIGHTS = {"bound_primscale": 0.01, "negcolor": 0.01, "l2_reg": 0.001, "backlit_reg": 1.0}   # the four RGCA regularisers, any weights


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "regloss_golden.npz")))


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _ratio(got, f64, f32):
    """Largest |got - f64| / (2 |f32 - f64| + 4 eps32 |f64|) over the elements; a zero bound admits a zero error only."""
    got, f64, f32 = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (got, f64, f32))
    err = np.abs(got - f64)
    bound = 2.0 * np.abs(f32 - f64) + 4.0 * EPS32 * np.abs(f64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


_REPORT = {}


def _report(case, loss_ratio, grad_ratio):
    _REPORT[case] = {"loss": loss_ratio, "grad": grad_ratio}
    out = os.environ.get("GOLIATH_PARITY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    from goliath_amd import build, losses

    json.dump({"what": "goliath_amd.losses regularisers vs the reference's functions in float64 on the inputs of "
                       "tests/golden/regloss_golden.npz: largest |hip - f64| / (2 |f32 - f64| + 4 eps32 |f64|) of the loss "
                       "and over the gradient's elements, per case (<= 1 passes)",
               "csrc_sha16": build.source_digest(), "chunk_elems": losses.regloss_chunk_elems(), "cases": _REPORT},
              open(os.path.join(out, "regloss_parity.json"), "w"), indent=1)


def _unary(losses, kind, x, golden):
    if kind == "bound_primscale":
        lo, hi = (float(v) for v in golden["bound_primscale/params"])
        return losses.bound_primscale({KEYS[kind]: x}, min_scale=lo, max_scale=hi)
    if kind == "list_l1_reg":
        return losses.list_l1_reg({KEYS[kind]: [x]})
    return getattr(losses, kind)({KEYS[kind]: x})


@pytest.mark.parametrize("tag", UNARY_TAGS)
@pytest.mark.parametrize("kind", UNARY)
def test_unary_parity_with_the_reference_in_float64(golden, kind, tag):
    from goliath_amd import losses

    pre = f"{kind}/{tag}/"
    x = _dev(golden[pre + "x"], grad=True)
    loss = _unary(losses, kind, x, golden)
    (grad,) = torch.autograd.grad(loss, x)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.shape == x.shape
    rl = _ratio(loss.item(), golden[pre + "loss64"], golden[pre + "loss32"])
    rg = _ratio(grad.cpu().numpy(), golden[pre + "grad64"], golden[pre + "grad32"])
    print(f"{pre} loss {loss.item():.9g} (f64 {float(golden[pre + 'loss64']):.9g}) error/bound: loss {rl:.3g}, grad {rg:.3g}")
    _report(pre[:-1], rl, rg)
    assert rl <= 1.0 and rg <= 1.0, (pre, rl, rg)


@pytest.mark.parametrize("tag", BACKLIT_TAGS)
def test_backlit_parity_with_the_reference_in_float64(golden, tag):
    from goliath_amd import losses

    pre = f"backlit_reg/{tag}/"
    color, cw = _dev(golden[pre + "color"], grad=True), _dev(golden[pre + "cos_weight"])
    loss = losses.backlit_reg({"color_rand": color, "cos_weight": cw})
    (grad,) = torch.autograd.grad(loss, color)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.shape == color.shape
    rl = _ratio(loss.item(), golden[pre + "loss64"], golden[pre + "loss32"])
    rg = _ratio(grad.cpu().numpy(), golden[pre + "grad64"], golden[pre + "grad32"])
    print(f"{pre} loss {loss.item():.9g} (f64 {float(golden[pre + 'loss64']):.9g}) error/bound: loss {rl:.3g}, grad {rg:.3g}")
    _report(pre[:-1], rl, rg)
    assert rl <= 1.0 and rg <= 1.0, (pre, rl, rg)
    if tag == "allpos":   # no backlit row: the loss is 0, the denominator exactly 1 and every gradient 0
        assert loss.item() == 0.0 and not grad.any()


def _loss_and_grad(fn, x):
    x = x.detach().requires_grad_(True)
    loss = fn(x)
    (g,) = torch.autograd.grad(loss, x)
    return loss, g


@pytest.mark.parametrize("kind", UNARY)
def test_misaligned_base_pointer_gives_the_aligned_bits(golden, kind):
    """x_big[1:] is contiguous and starts 4 bytes past a 16-byte boundary: the scalar path on every chunk."""
    from goliath_amd import losses

    big = _dev(np.concatenate([golden[f"{kind}/n12293/x"][:1], golden[f"{kind}/n12293/x"]]))
    off, aligned = big[1:], big[1:].clone()
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    fn = lambda x: _unary(losses, kind, x, golden)
    (l0, g0), (l1, g1) = _loss_and_grad(fn, off), _loss_and_grad(fn, aligned)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_backlit_misaligned_base_pointers_give_the_aligned_bits(golden):
    from goliath_amd import losses

    col, cw = golden["backlit_reg/rows1025/color"].reshape(-1), golden["backlit_reg/rows1025/cos_weight"].reshape(-1)
    M = cw.size
    big_col, big_cw = _dev(np.concatenate([col[:1], col])), _dev(np.concatenate([cw[:1], cw]))
    ref = _loss_and_grad(lambda c: losses.backlit(c, big_cw[1:].clone().reshape(M, 1)), big_col[1:].clone().reshape(M, 3))
    for c_off, w_off in ((True, False), (False, True), (True, True)):
        c = big_col[1:].reshape(M, 3) if c_off else big_col[1:].clone().reshape(M, 3)
        w = big_cw[1:].reshape(M, 1) if w_off else big_cw[1:].clone().reshape(M, 1)
        assert c.data_ptr() % 16 == (4 if c_off else 0) and w.data_ptr() % 16 == (4 if w_off else 0)
        l, g = _loss_and_grad(lambda t: losses.backlit(t, w), c)
        assert torch.equal(l, ref[0]) and torch.equal(g, ref[1])


def _rgca_preds(golden, grad=True):
    p = {KEYS[k]: _dev(golden[f"{k}/real/x"], grad) for k in ("bound_primscale", "negcolor", "l2_reg")}
    p["color_rand"] = _dev(golden["backlit_reg/rows1025/color"], grad)
    p["cos_weight"] = _dev(golden["backlit_reg/rows1025/cos_weight"])
    return p


LEAVES = ("primscale_preclip", "diff_color", "spec_dnml", "color_rand")


def _rgca_total(preds, targets=None):
    """The four RGCA regularisers summed with weights, as ModularLoss.forward does (ca_code/loss/__init__.py:137-170)."""
    from goliath_amd import losses

    total = 0.0
    for name, w in WEIGHTS.items():
        total = total + w * getattr(losses, name)(preds, targets)
    return total


def _rgca_step(preds, upstream=None):
    loss = _rgca_total(preds)
    grads = torch.autograd.grad(loss, [preds[k] for k in LEAVES], grad_outputs=upstream)
    return (loss.detach(), *grads)


def test_two_runs_are_bit_identical(golden):
    from goliath_amd import losses

    a, b = _rgca_step(_rgca_preds(golden)), _rgca_step(_rgca_preds(golden))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for kind in ("list_l1_reg", "alphaprior"):
        x = _dev(golden[f"{kind}/n12293/x"])
        fn = lambda t: _unary(losses, kind, t, golden)
        (l0, g0), (l1, g1) = _loss_and_grad(fn, x), _loss_and_grad(fn, x)
        assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_upstream_gradient_scales_exactly(golden):
    from goliath_amd import losses

    one = _rgca_step(_rgca_preds(golden))
    quarter = _rgca_step(_rgca_preds(golden), upstream=torch.tensor(0.25, device="cuda"))
    assert torch.equal(one[0], quarter[0])
    for a, b in zip(one[1:], quarter[1:]):
        assert a.abs().max() > 0 and torch.equal(0.25 * a, b)
    for kind in ("list_l1_reg", "alphaprior"):
        x = _dev(golden[f"{kind}/n4097/x"], grad=True)
        (a,) = torch.autograd.grad(_unary(losses, kind, x, golden), x)
        (b,) = torch.autograd.grad(0.25 * _unary(losses, kind, x, golden), x)
        assert torch.equal(0.25 * a, b)


def test_no_backward_for_an_input_without_grad(golden):
    from goliath_amd import _lib, losses

    preds = _rgca_preds(golden, grad=False)
    for name in WEIGHTS:
        assert not getattr(losses, name)(preds).requires_grad
    preds["diff_color"].requires_grad_(True)      # one term with a gradient: only its backward kernel may run
    _lib.TIMING = []
    try:
        _rgca_total(preds).backward()
        names = [n for n, _, _ in _lib.TIMING]
    finally:
        _lib.TIMING = None
    assert sorted(names) == ["gol_backlit_fwd", "gol_regloss_bwd", "gol_regloss_fwd", "gol_regloss_fwd", "gol_regloss_fwd"]
    assert preds["diff_color"].grad is not None and all(preds[k].grad is None for k in LEAVES if k != "diff_color")
    # straight at the Function: no launch, None for the input
    x = preds["spec_dnml"]
    ctx = types.SimpleNamespace(needs_input_grad=(False, False, False, False), saved_tensors=(x,), args=(losses.SQ, 0.0, 0.0))
    _lib.TIMING = []
    try:
        assert losses._Penalty.backward(ctx, torch.ones((), device="cuda")) == (None, None, None, None)
        ctx = types.SimpleNamespace(needs_input_grad=(False, False), saved_tensors=(preds["color_rand"], preds["cos_weight"], x))
        assert losses._Backlit.backward(ctx, torch.ones((), device="cuda")) == (None, None)
        assert _lib.TIMING == []
    finally:
        _lib.TIMING = None


def test_argument_errors(golden):
    from goliath_amd import _lib, losses
    from goliath_amd._lib import c_float, c_i64, c_int, fptr, ptr, stream_ptr

    color, cw = _dev(golden["backlit_reg/c4/color"]), _dev(golden["backlit_reg/c4/cos_weight"])
    with pytest.raises(ValueError):
        losses.backlit(color, cw.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        losses.backlit(color, cw[:, :-1])
    with pytest.raises(ValueError):
        losses.penalty_mean(torch.empty(0, 3, device="cuda"), losses.SQ)
    with pytest.raises(ValueError):
        losses.backlit(torch.empty(1, 0, 3, device="cuda"), torch.empty(1, 0, 1, device="cuda"))
    x = torch.ones(8, device="cuda")
    partial = torch.zeros(1, device="cuda", dtype=torch.float64)
    gs = torch.ones(1, device="cuda")
    for entry, tail in (("gol_regloss_fwd", (ptr(partial, torch.float64),)), ("gol_regloss_bwd", (fptr(gs), fptr(x.clone())))):
        with pytest.raises(_lib.GoliathHipError, match="unknown penalty kind 99"):
            _lib.call(entry, c_int(99), c_i64(8), c_float(0), c_float(0), fptr(x), *tail, stream_ptr())
        with pytest.raises(_lib.GoliathHipError, match="negative count"):
            _lib.call(entry, c_int(losses.SQ), c_i64(-1), c_float(0), c_float(0), fptr(x), *tail, stream_ptr())
        with pytest.raises(_lib.GoliathHipError, match="null pointer"):
            _lib.call(entry, c_int(losses.SQ), c_i64(8), c_float(0), c_float(0), ctypes.c_void_p(0), *tail, stream_ptr())
        # nothing to do: no launch, no pointer is looked at
        _lib.call(entry, c_int(losses.SQ), c_i64(0), c_float(0), c_float(0), *([ctypes.c_void_p(0)] * (1 + len(tail))), stream_ptr())
    with pytest.raises(_lib.GoliathHipError, match="null pointer"):
        _lib.call("gol_backlit_fwd", c_i64(2), c_int(3), fptr(x), ctypes.c_void_p(0), ptr(partial, torch.float64), stream_ptr())
    _lib.call("gol_backlit_fwd", c_i64(0), c_int(3), ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0), stream_ptr())
    _lib.call("gol_backlit_bwd", c_i64(0), c_int(3), *([ctypes.c_void_p(0)] * 4), stream_ptr())
    torch.cuda.synchronize()
    assert float(partial) == 0.0


def test_list_l1_reg_is_the_sum_of_its_terms(golden):
    from goliath_amd import losses

    terms = [_dev(golden["list_l1_reg/n4097/x"], grad=True), _dev(golden["list_l1_reg/real/x"], grad=True),
             _dev(golden["list_l1_reg/n3/x"], grad=True)]
    loss = losses.list_l1_reg({"spec_dnml": terms})
    grads = torch.autograd.grad(loss, terms)
    singles = [losses.penalty_mean(t, losses.ABS) for t in terms]
    assert torch.equal(loss, singles[0] + singles[1] + singles[2])
    for t, g, s in zip(terms, grads, singles):
        assert torch.equal(g, torch.autograd.grad(s, t)[0])


def test_mask_l1_is_l1_image_without_a_mask():
    from goliath_amd import losses

    g = torch.Generator().manual_seed(5)
    pred = torch.rand(2, 1, 37, 53, generator=g).cuda().requires_grad_(True)
    target = (torch.rand(2, 1, 37, 53, generator=g) > 0.5).float().cuda()
    a = losses.mask_l1({"rendered_mask": pred}, {"image_mask": target})
    b = losses.l1_image(pred, target)
    assert torch.equal(a, b)
    ref = (pred.detach().double() - target.double()).abs().mean()
    assert abs(a.item() - ref.item()) <= 4 * EPS32 * ref.item()
    (ga,) = torch.autograd.grad(a, pred)
    (gb,) = torch.autograd.grad(b, pred)
    assert torch.equal(ga, gb)
    assert torch.allclose(ga, torch.sign(pred.detach() - target) / pred.numel(), rtol=1e-6, atol=0.0)


def test_no_host_sync(golden):
    preds = _rgca_preds(golden)
    _rgca_step(preds)                         # loads the library outside the guarded region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = _rgca_step(preds)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(t).all() for t in out)


def test_graph_capture_replays_the_eager_step(golden):
    preds = _rgca_preds(golden)
    eager = [t.clone() for t in _rgca_step(preds)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _rgca_step(preds)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _rgca_step(preds)
    for t in static:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, static))
    # new values in the same tensors: the replay follows them
    with torch.no_grad():
        preds["diff_color"].neg_()
    graph.replay()
    torch.cuda.synchronize()
    again = _rgca_step(preds)
    assert all(torch.equal(a, b) for a, b in zip(again, static))
    assert not torch.equal(static[2], eager[2])


def test_registry_path_returns_the_direct_bits(golden):
    from goliath_amd import dropin, losses

    class FnLoss(torch.nn.Module):  # same contract as ca_code/loss/registry.py:40-56
        def __init__(self, fn, function_args):
            super().__init__()
            self.fn, self.extra_args = fn, function_args

        def forward(self, preds, targets):
            return self.fn(preds, targets, **self.extra_args)

    reg = types.SimpleNamespace(loss_registry={"kl": "untouched"}, FnLoss=FnLoss)
    dropin.patch_losses(reg, regularizers=True)
    mod = reg.loss_registry["bound_primscale"](None, min_scale=0.2, max_scale=5.0)
    x = _dev(golden["bound_primscale/n4097/x"], grad=True)
    a = mod({"primscale_preclip": x}, {})
    b = losses.bound_primscale({"primscale_preclip": x}, min_scale=0.2, max_scale=5.0)
    c = losses.bound_primscale({"primscale_preclip": x})
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(torch.autograd.grad(a, x)[0], torch.autograd.grad(b, x)[0])
    assert reg.loss_registry["kl"] == "untouched"
