"""GPU: the EfficientNet feature loss of goliath_amd.effnet (real widths, random weights, tests/effnet_cases.py:loss_case)
against its float64 twin with every block forced onto the fused operator, without a mask, with a target that requires
grad, through the registry entries of the drop-in, and captured as a graph.

Bar: 1e-5 for the loss (relative) and for the image gradient (rel-L2), the project's bar against float64.  The network is
smooth except for the clamp of the normalisation: the image gradient is compared where no image value of the pixel lies
within 1e-4 of 0 or 255; the draw is uniform over 330 grey levels, so that share is < 2e-3 of the pixels (asserted)."""
import copy
import functools
import types

import pytest
import torch

import effnet_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _all_fused(monkeypatch):
    monkeypatch.setenv("GOLIATH_FUSED_EFFNET_ALL", "1")


@functools.lru_cache(maxsize=None)
def _reference(masked=True, target_grad=False):
    """float64 loss and gradients of the twin."""
    from goliath_amd import effnet

    feats, x, y, mask = ec.loss_case()
    x, y = x.double().requires_grad_(True), y.double().requires_grad_(target_grad)
    loss = effnet.effnet_loss_torch(feats, x, y, mask.double() if masked else None)
    grads = torch.autograd.grad(loss, [x, y] if target_grad else [x])
    return loss.detach(), grads


@functools.lru_cache(maxsize=None)
def _gpu_case():
    feats, x, y, mask = ec.loss_case()
    return copy.deepcopy(feats).cuda(), x.cuda(), y.cuda(), mask.cuda()


def _keep():
    _, x, y, _ = ec.loss_case()
    keep = ec.kink_mask(x, y)
    share = float((~keep).any(1).double().mean())
    print("pixels with an image value at a clamp kink:", share)
    assert share < ec.ZEROED_CAP
    return keep.double()


def _count_calls(monkeypatch):
    from goliath_amd import effnet

    taken, op = [], effnet.mbconv_front
    monkeypatch.setattr(effnet, "mbconv_front", lambda *a: (taken.append(tuple(a[0].shape)), op(*a))[1])
    return taken


@pytest.mark.parametrize("masked", [True, False], ids=["soft-mask", "mask-none"])
def test_loss_and_image_gradient_match_float64(masked, monkeypatch):
    from goliath_amd import effnet

    l64, (g64,) = _reference(masked)
    taken = _count_calls(monkeypatch)
    feats, x, y, mask = _gpu_case()
    x = x.clone().requires_grad_(True)
    net = effnet.EfficientNetLoss(feats)
    loss = net(x, y, mask) if masked else net(x, y)
    g, = torch.autograd.grad(loss, x)
    keep = _keep()
    err = [abs(float(loss.detach()) - float(l64)) / abs(float(l64)), ec.rel(g.cpu().double() * keep, g64 * keep)]
    print("HIP against float64:", err, "operator calls", len(taken))
    assert len(taken) == 10 and taken[0] == (2, 32, 19, 25) and taken[4] == (2, 40, 5, 7)     # five blocks, prediction and target
    assert float(l64) > 0 and float(g64.abs().max()) > 0
    assert err[0] <= ec.BAR and err[1] <= ec.BAR


def test_target_that_requires_grad(monkeypatch):
    """The `dst_key` case: a target that requires grad takes the twin's elementwise tap lines; the gradient reaches it."""
    from goliath_amd import effnet

    l64, g64 = _reference(True, True)
    taken = _count_calls(monkeypatch)
    feats, x, y, mask = _gpu_case()
    x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    loss = effnet.EfficientNetLoss(feats)(x, y, mask)
    g = torch.autograd.grad(loss, [x, y])
    keep = _keep()
    err = [abs(float(loss.detach()) - float(l64)) / abs(float(l64))] + \
        [ec.rel(a.cpu().double() * keep, b * keep) for a, b in zip(g, g64)]
    print("HIP against float64:", err)
    assert len(taken) == 10 and float(g64[1].abs().max()) > 0
    assert max(err) <= ec.BAR


def test_target_branch_saves_nothing(monkeypatch):
    from goliath_amd import effnet

    feats, x, y, mask = _gpu_case()
    seen = []
    fwd = effnet._Front.forward

    def spy(ctx, xx, *rest):
        out = fwd(ctx, xx, *rest)
        seen.append(bool(ctx.needs_input_grad[0]))
        return out

    monkeypatch.setattr(effnet._Front, "forward", staticmethod(spy))
    effnet.EfficientNetLoss(feats)(x.clone().requires_grad_(True), y, mask)
    assert seen == [True] * 5 + [False] * 5


def test_registry_entries_through_patch_losses():
    """dropin.patch_losses(effnet=features) on a stand-in registry: `effnet` and `effnet_phys`, built and called the way
    ModularLoss does, return the number EfficientNetLoss returns; with mask_erode the mask goes through imageops.erode."""
    from goliath_amd import dropin, effnet, imageops

    feats, x, y, mask = _gpu_case()
    reg = types.SimpleNamespace(loss_registry={"vgg": "untouched", "effnet": "untouched", "effnet_phys": "untouched"}, FnLoss=None)
    assert dropin.patch_losses(reg, effnet=feats) is reg and reg.loss_registry["vgg"] == "untouched"
    direct = effnet.EfficientNetLoss(feats)(x, y, mask)
    got = reg.loss_registry["effnet"](None)({"rendered_rgb": x, "rendered_phys_rgb": y}, {"image": y, "image_mask": mask})
    assert torch.equal(got, direct)
    phys = reg.loss_registry["effnet_phys"](None)({"rendered_rgb": y, "rendered_phys_rgb": x}, {"image": y, "image_mask": mask})
    assert torch.equal(phys, direct) and float(direct) > 0
    got = reg.loss_registry["effnet"](None, dst_key="other", mask_key="alpha")({"rendered_rgb": x, "other": y, "alpha": mask}, {})
    assert torch.equal(got, direct)
    hard = (mask > 0.5).float()
    eroded = effnet.EffNetLoss(None, features=feats, mask_erode=3)({"rendered_rgb": x}, {"image": y, "image_mask": hard})
    assert torch.equal(eroded, effnet.EfficientNetLoss(feats)(x, y, imageops.erode(hard, 3)))
    assert float(eroded) != float(effnet.EfficientNetLoss(feats)(x, y, hard))


def test_graph_capture_replays_to_the_same_bits():
    """Forward and backward of the loss captured on one stream as a graph (no host sync in the ABI calls) and replayed
    twice on new input values give the bits of the eager run."""
    from goliath_amd import effnet

    feats, x, y, mask = _gpu_case()
    net = effnet.EfficientNetLoss(feats)
    xe = x.clone().requires_grad_(True)
    le = net(xe, y, mask)
    ge, = torch.autograd.grad(le, xe)

    xs = torch.zeros_like(x).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(net(xs, y, mask), xs)       # warm-up: allocations and lazy initialisation outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ls = net(xs, y, mask)
        gs, = torch.autograd.grad(ls, xs)
    for _ in range(2):
        with torch.no_grad():
            xs.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ls, le) and torch.equal(gs, ge) and float(ge.abs().max()) > 0
        with torch.no_grad():
            xs.zero_()
