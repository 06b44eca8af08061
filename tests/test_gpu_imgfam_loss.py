"""GPU: the masked image penalties of goliath_amd.losses (csrc/imgfam.hip: gol_imgloss_*) against
tests/golden/imgfam_golden.npz, which holds each case's inputs, the reference's own function on them in float64 and the same
in float32 on the CPU (tests/golden/make_imgfam_golden.py).

Parity bound, per loss and per gradient element, nothing excluded:
    |hip - f64| <= 2 |f32 - f64| + 4 eps32 |f64|
(the regloss bar: twice the reference's own float32 deviation plus four float32 roundings of the value itself).  The largest
error / bound ratio per kind goes to imgfam_parity.json in the directory GOLIATH_PARITY_DIR names
(profiles/imgfam_parity.json is a copy of one such run)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import imgfam_cases as cases  # noqa: E402
import npz_parts  # noqa: E402

EPS32 = cases.EPS32
KIND_ID = {"abs": 0, "sq": 1, "expw": 2}
PUB_FOCUS = [f"{fn}_sm{sm}_blur{bl}_{dd}" for fn in ("rgb_l1_focus", "rgb_l1_phys") for sm in (0, 1) for bl in (0, 1)
             for dd in ("bool", "float")]


@pytest.fixture(scope="module")
def golden():
    return npz_parts.load(os.path.join(HERE, "golden", "imgfam_golden.npz"))


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


def _report(kind, case, loss_ratio, grad_ratio):
    k = _REPORT.setdefault(kind, {"loss": 0.0, "loss_case": None, "grad": 0.0, "grad_case": None, "cases": 0})
    k["cases"] += 1
    if loss_ratio >= k["loss"]:
        k["loss"], k["loss_case"] = loss_ratio, case
    if grad_ratio >= k["grad"]:
        k["grad"], k["grad_case"] = grad_ratio, case
    out = os.environ.get("GOLIATH_PARITY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    from goliath_amd import build, losses

    json.dump({"what": "goliath_amd.losses image penalties vs the reference's functions in float64 on the inputs of "
                       "tests/golden/imgfam_golden.npz: largest |hip - f64| / (2 |f32 - f64| + 4 eps32 |f64|) of the loss and "
                       "over the gradient's elements, per kind over its cases and per public function (<= 1 passes)",
               "csrc_sha16": build.source_digest(), "chunk_elems": losses.imgloss_chunk_elems(), "kinds": _REPORT},
              open(os.path.join(out, "imgfam_parity.json"), "w"), indent=1)


def _inputs(golden, B, C, HW):
    tag = f"loss/{cases.shape_tag(B, C, HW)}/"
    return tag, {k: _dev(golden[tag + k]) for k in ("pred", "target", "mask1", "maskc", "veto")}


def _pick(x, mk, vk):
    return {"none": None, "one": x["mask1"], "full": x["maskc"]}[mk], (x["veto"] if vk == "veto" else None)


def _loss_and_grad(fn, pred, upstream=None):
    pred = pred.detach().requires_grad_(True)
    loss = fn(pred)
    (g,) = torch.autograd.grad(loss, pred, grad_outputs=upstream)
    return loss.detach(), g


@pytest.mark.parametrize("HW", cases.HWS)
@pytest.mark.parametrize("B,C", cases.BCS)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_kernel_parity_with_the_reference_in_float64(golden, kind, B, C, HW):
    """Every mask (none, [B,1,HW], [B,C,HW]) and veto (none, ~10 % set) configuration of one kind and shape."""
    from goliath_amd import losses

    tag, x = _inputs(golden, B, C, HW)
    worst = (0.0, 0.0)
    for mk in cases.MASKS:
        for vk in cases.VETOS:
            mask, veto = _pick(x, mk, vk)
            loss, grad = _loss_and_grad(lambda p: losses.image_penalty(p, x["target"], KIND_ID[kind], mask, veto), x["pred"])
            assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.shape == x["pred"].shape
            pre = f"{tag}{kind}/{mk}-{vk}/"
            rl = _ratio(loss.item(), golden[pre + "loss64"], golden[pre + "loss32"])
            rg = _ratio(grad.cpu().numpy(), golden[pre + "grad64"], golden[pre + "grad32"])
            print(f"{pre} loss {loss.item():.9g} (f64 {float(golden[pre + 'loss64']):.9g}) error/bound: loss {rl:.3g}, grad {rg:.3g}")
            _report(kind, pre[:-1], rl, rg)
            worst = (max(worst[0], rl), max(worst[1], rg))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (tag, kind, worst)


def test_fixture_inputs_reach_the_kernel_with_their_kinks(golden):
    """The veto really vetoes and the mask really masks: a vetoed or zero-masked element has a zero gradient, the others of
    the SQ kind a non-zero one wherever pred != target."""
    from goliath_amd import losses

    _, x = _inputs(golden, 2, 3, 4097)
    _, g = _loss_and_grad(lambda p: losses.image_penalty(p, x["target"], losses.IMG_SQ, x["maskc"], x["veto"]), x["pred"])
    dead = x["veto"].expand_as(g) | (x["maskc"] == 0) | (x["pred"] == x["target"])
    assert dead.any() and (~dead).any()
    assert not g[dead].any() and g[~dead].ne(0).all()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_misaligned_base_pointers_give_the_aligned_bits(golden, kind):
    """Views one float (the veto: one byte) past a 16-byte boundary take the scalar path (the veto: byte loads) on every chunk
    of every plane and give the bits of the aligned copies."""
    from goliath_amd import losses

    _, x = _inputs(golden, 2, 3, 4096)

    def off(t):
        big = torch.cat([t.reshape(-1)[:1], t.reshape(-1)])
        v = big[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size() and torch.equal(v, t)
        return v

    fn = lambda p, t, m, v: _loss_and_grad(lambda q: losses.image_penalty(q, t, KIND_ID[kind], m, v), p)
    ref = fn(x["pred"], x["target"], x["maskc"], x["veto"])
    assert all(x[k].data_ptr() % 16 == 0 for k in x)
    for which in (("pred",), ("target",), ("maskc",), ("veto",), ("pred", "target", "maskc", "veto")):
        y = {k: (off(v) if k in which else v) for k, v in x.items()}
        l, g = fn(y["pred"], y["target"], y["maskc"], y["veto"])
        assert torch.equal(l, ref[0]) and torch.equal(g, ref[1]), which


@pytest.mark.parametrize("kind", cases.KINDS)
def test_odd_plane_length_gives_the_bits_of_aligned_planes(golden, kind):
    """HW = 4097 with C = 3: planes 1 and 2 of every image start off 16-byte alignment.  Chunk sums and gradients equal those
    of per-plane calls on aligned copies (the entries themselves: one g_scale for both)."""
    from goliath_amd import _lib, losses
    from goliath_amd._lib import c_int, fptr, ptr, stream_ptr

    B, C, HW = 2, 3, 4097
    _, x = _inputs(golden, B, C, HW)
    nb = -(-HW // losses.imgloss_chunk_elems())
    gs = torch.full((1,), 0.37, device="cuda")

    def run(b, c, pred, target, mask, veto):
        partial = torch.full((b * c * nb,), -1.0, device="cuda", dtype=torch.float64)
        grad = torch.full_like(pred, float("nan"))
        head = (c_int(KIND_ID[kind]), c_int(b), c_int(c), c_int(HW), c_int(mask.shape[1]), fptr(pred), fptr(target), fptr(mask),
                ptr(veto, torch.uint8))
        _lib.call("gol_imgloss_fwd", *head, ptr(partial, torch.float64), stream_ptr())
        _lib.call("gol_imgloss_bwd", *head, fptr(gs), fptr(grad), stream_ptr())
        return partial.view(b * c, nb), grad

    veto = x["veto"].view(torch.uint8)
    full_p, full_g = run(B, C, x["pred"], x["target"], x["maskc"], veto)
    assert x["pred"][0, 1].data_ptr() % 16 != 0
    for b in range(B):
        for c in range(C):
            one = lambda t, ch: t[b:b + 1, ch:ch + 1].clone()
            args = (one(x["pred"], c), one(x["target"], c), one(x["maskc"], c), one(veto, 0))
            assert all(a.data_ptr() % 16 == 0 for a in args)
            p, g = run(1, 1, *args)
            assert torch.equal(p[0], full_p[b * C + c]) and torch.equal(g[0, 0], full_g[b, c]), (b, c)
    assert torch.isfinite(full_g).all() and (full_p >= 0).all()


def test_two_runs_agree_and_the_upstream_gradient_scales_exactly(golden):
    from goliath_amd import losses

    _, x = _inputs(golden, 2, 3, 2 * 4096 + 5)
    for kind in cases.KINDS:
        fn = lambda p: losses.image_penalty(p, x["target"], KIND_ID[kind], x["mask1"], x["veto"])
        (l0, g0), (l1, g1) = _loss_and_grad(fn, x["pred"]), _loss_and_grad(fn, x["pred"])
        assert torch.equal(l0, l1) and torch.equal(g0, g1)
        l2, g2 = _loss_and_grad(fn, x["pred"], upstream=torch.tensor(0.25, device="cuda"))
        assert torch.equal(l0, l2) and g0.abs().max() > 0 and torch.equal(0.25 * g0, g2)


def test_no_backward_for_a_prediction_without_grad(golden):
    from goliath_amd import _lib, losses

    _, x = _inputs(golden, 2, 3, 4097)
    w = torch.ones((), device="cuda", requires_grad=True)
    _lib.TIMING = []
    try:
        loss = losses.image_penalty(x["pred"], x["target"], losses.IMG_EXPW, x["mask1"], x["veto"])
        assert not loss.requires_grad
        (w * loss).backward()
        names = [n for n, _, _ in _lib.TIMING]
    finally:
        _lib.TIMING = None
    assert names == ["gol_imgloss_fwd", "gol_imgloss_finalize"]
    _lib.TIMING = []
    try:
        p = x["pred"].clone().requires_grad_(True)
        losses.image_penalty(p, x["target"], losses.IMG_EXPW, x["mask1"], x["veto"]).backward()
        names = [n for n, _, _ in _lib.TIMING]
    finally:
        _lib.TIMING = None
    assert names == ["gol_imgloss_fwd", "gol_imgloss_finalize", "gol_imgloss_bwd"] and p.grad is not None


def test_a_veto_of_all_ones_gives_zero(golden):
    from goliath_amd import losses

    _, x = _inputs(golden, 2, 3, 4097)
    for kind in cases.KINDS:
        for mask in (None, x["maskc"]):
            l, g = _loss_and_grad(lambda p: losses.image_penalty(p, x["target"], KIND_ID[kind], mask,
                                                                torch.ones_like(x["veto"])), x["pred"])
            assert l.item() == 0.0 and not g.any()


# ---- the public functions ----------------------------------------------------------------------------------------------
def _public(golden, case, fn_name, kw, pred_key):
    """(loss, grad of pred) of losses.<fn_name> on the fixture's dictionaries; every non-differentiated tensor requires
    grad and must come back without one, and the prediction keys the call must not read hold other numbers."""
    from goliath_amd import losses

    pre = f"pub/{case}/"
    pred = _dev(golden[pre + "pred"], grad=True)
    target = _dev(golden[pre + "target"], grad=True)
    preds = {k: pred.detach() + 1.0 for k in ("rendered_rgb", "rendered_rgb_blur", "rendered_phys_rgb")}
    preds[pred_key] = pred
    targets = {"image": target}
    others = [target]
    if pre + "image_mask" in golden:
        targets["image_mask"] = _dev(golden[pre + "image_mask"])
        preds["rendered_mask"] = _dev(golden[pre + "rendered_mask"], grad=True)
        others.append(preds["rendered_mask"])
    if pre + "depth_disc_mask" in golden:
        dd = golden[pre + "depth_disc_mask"]
        preds["depth_disc_mask"] = _dev(dd, grad=dd.dtype != np.bool_)
        if dd.dtype != np.bool_:
            others.append(preds["depth_disc_mask"])
    loss = getattr(losses, fn_name)(preds, targets, **kw)
    grads = torch.autograd.grad(loss, [pred] + others, allow_unused=True)
    assert all(g is None for g in grads[1:])
    rl = _ratio(loss.item(), golden[pre + "loss64"], golden[pre + "loss32"])
    rg = _ratio(grads[0].cpu().numpy(), golden[pre + "grad64"], golden[pre + "grad32"])
    print(f"{pre} loss {loss.item():.9g} (f64 {float(golden[pre + 'loss64']):.9g}) error/bound: loss {rl:.3g}, grad {rg:.3g}")
    _report(fn_name, pre[:-1], rl, rg)
    return rl, rg


@pytest.mark.parametrize("case,fn_name,kw", [("rgb_l2_erode3", "rgb_l2", {"mask_erode": 3}), ("rgb_l2_nomask", "rgb_l2", {}),
                                             ("psnr", "psnr", {"data_range": 255.0})])
def test_rgb_l2_and_psnr_parity(golden, case, fn_name, kw):
    rl, rg = _public(golden, case, fn_name, kw, "rendered_rgb")
    assert rl <= 1.0 and rg <= 1.0, (case, rl, rg)


@pytest.mark.parametrize("case", PUB_FOCUS)
def test_focus_losses_parity(golden, case):
    fn_name = case[:len("rgb_l1_focus")] if case.startswith("rgb_l1_focus") else "rgb_l1_phys"
    sm, blur = "_sm1_" in case, "_blur1_" in case
    key = "rendered_phys_rgb" if fn_name == "rgb_l1_phys" else ("rendered_rgb_blur" if blur else "rendered_rgb")
    rl, rg = _public(golden, case, fn_name, {"self_mask": sm, "img_blur": blur, "mask_erode": 3 if sm == blur else None}, key)
    assert rl <= 1.0 and rg <= 1.0, (case, rl, rg)


def test_pose_shadow_l2_parity(golden):
    from goliath_amd import losses

    pre = "pub/pose_shadow_l2/"
    pred, target = _dev(golden[pre + "pred"], grad=True), _dev(golden[pre + "target"], grad=True)
    loss = losses.pose_shadow_l2({"pose_shadow_map": pred, "shadow_map": target})
    gp, gt = torch.autograd.grad(loss, [pred, target], allow_unused=True)
    assert gt is None                                   # .detach() in the reference
    rl = _ratio(loss.item(), golden[pre + "loss64"], golden[pre + "loss32"])
    rg = _ratio(gp.cpu().numpy(), golden[pre + "grad64"], golden[pre + "grad32"])
    print(f"{pre} error/bound: loss {rl:.3g}, grad {rg:.3g}")
    _report("pose_shadow_l2", pre[:-1], rl, rg)
    assert rl <= 1.0 and rg <= 1.0


def test_argument_errors(golden):
    from goliath_amd import _lib, losses
    from goliath_amd._lib import c_i64, c_int, fptr, ptr, stream_ptr

    x = torch.ones(1, 2, 8, device="cuda")
    partial = torch.zeros(2, device="cuda", dtype=torch.float64)
    gs, null = torch.ones(1, device="cuda"), ctypes.c_void_p(0)
    head = lambda kind, mask_c=1, pred=None, mask=None: (c_int(kind), c_int(1), c_int(2), c_int(8), c_int(mask_c),
                                                         fptr(x) if pred is None else pred, fptr(x), mask or null, null)
    for entry, tail in (("gol_imgloss_fwd", (ptr(partial, torch.float64),)), ("gol_imgloss_bwd", (fptr(gs), fptr(x.clone())))):
        with pytest.raises(_lib.GoliathHipError, match="unknown penalty kind 3"):
            _lib.call(entry, *head(3), *tail, stream_ptr())
        with pytest.raises(_lib.GoliathHipError, match="1 or C channels"):
            _lib.call(entry, *head(losses.IMG_SQ, mask_c=3, mask=fptr(x)), *tail, stream_ptr())
        with pytest.raises(_lib.GoliathHipError, match="null pointer"):
            _lib.call(entry, *head(losses.IMG_SQ, pred=null), *tail, stream_ptr())
        with pytest.raises(_lib.GoliathHipError, match="65535"):
            _lib.call(entry, c_int(0), c_int(65536), c_int(1), c_int(8), c_int(0), fptr(x), fptr(x), null, null, *tail, stream_ptr())
        # nothing to do: no launch, no pointer is looked at
        _lib.call(entry, c_int(0), c_int(1), c_int(2), c_int(0), c_int(0), *([null] * (4 + len(tail))), stream_ptr())
        _lib.call(entry, c_int(0), c_int(0), c_int(2), c_int(8), c_int(0), *([null] * (4 + len(tail))), stream_ptr())
    _lib.call("gol_imgloss_finalize", c_i64(0), c_i64(0), null, null, null, stream_ptr())
    with pytest.raises(_lib.GoliathHipError, match="null pointer"):
        _lib.call("gol_imgloss_finalize", c_i64(2), c_i64(16), null, null, null, stream_ptr())
    with pytest.raises(ValueError):
        losses.image_penalty(x, x, losses.IMG_SQ, mask=torch.ones(1, 3, 8, device="cuda"))
    with pytest.raises(ValueError):
        losses.image_penalty(x, x, losses.IMG_SQ, veto=torch.ones(1, 1, 8, device="cuda"))
    torch.cuda.synchronize()
    assert float(partial.sum()) == 0.0


# ---- no host sync, graph capture ---------------------------------------------------------------------------------------
def _scene(golden):
    pre = "pub/rgb_l1_focus_sm0_blur0_bool/"
    B, _, H, W = golden[pre + "pred"].shape
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.where((yy - 9) ** 2 + (xx - 8) ** 2 < 30, 300.0, 500.0).astype(np.float32)[None, None].repeat(B, 0)
    return {"pred": _dev(golden[pre + "pred"]), "target": _dev(golden[pre + "target"]),
            "mask": _dev(golden[pre + "image_mask"]), "depth": _dev(depth)}


def _step(s):
    """depth -> depth_disc_mask -> rgb_l2(mask_erode=3) + rgb_l1_focus, forward and backward."""
    from goliath_amd import imageops, losses

    pred = s["pred"].detach().requires_grad_(True)
    dd = imageops.depth_discontinuity_mask(s["depth"])
    preds, targets = {"rendered_rgb": pred, "depth_disc_mask": dd}, {"image": s["target"], "image_mask": s["mask"]}
    l2 = losses.rgb_l2(preds, targets, mask_erode=3)
    lf = losses.rgb_l1_focus(preds, targets)
    (g,) = torch.autograd.grad(l2 + lf, pred)
    return l2.detach(), lf.detach(), g, dd


def test_no_host_sync(golden):
    s = _scene(golden)
    _step(s)                                  # loads the library outside the guarded region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = _step(s)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out[3].dtype == torch.bool and out[3].any() and not out[3].all()
    assert all(torch.isfinite(t).all() for t in out[:3]) and out[2].any()


def test_graph_capture_replays_the_eager_step(golden):
    s = _scene(golden)
    eager = [t.clone() for t in _step(s)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(s)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _step(s)
    for t in static:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, static))
    # new values in the same tensors: the replay follows them
    with torch.no_grad():
        s["pred"].mul_(0.5)
        s["depth"].copy_(s["depth"].flip(-1))
    graph.replay()
    torch.cuda.synchronize()
    again = _step(s)
    assert all(torch.equal(a, b) for a, b in zip(again, static))
    assert not torch.equal(static[2], eager[2]) and not torch.equal(static[3], eager[3])
