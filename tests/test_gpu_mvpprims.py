"""GPU: primitive assembly of the MVP hand model (goliath_amd/mvpprims.py on csrc/mvpprims.hip) against the PyTorch
restatements of tests/mvpprims_cases.py, and the patched model methods against the parent path on stand-in objects."""
import json
import math
import os
import types

import pytest
import torch

import mvpprims_cases as C
import scenes

pytestmark = pytest.mark.gpu


def _ints(shape, seed):
    """Integer-valued upstream gradients: sums of two of them are exact."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-50, 50, tuple(shape), generator=g).float()


_REF = {}


def _reference(shape, channels):
    """Per (shape, channels), once: the slabs, the full-K template by the restatement, upstream gradients for the full-K
    template.  Everything else (selection, masking, their gradients) is indexing of these."""
    key = (shape, channels)
    if key not in _REF:
        (TW, TH, TD), (ny, nx), B = shape
        rgb, alpha = C.slabs(shape)
        if channels == 1:
            rgb = None
        full = C.slab_template(rgb, alpha, (TW, TH, TD), ny, nx)
        _REF[key] = dict(rgb=rgb, alpha=alpha, full=full, g=_ints(full.shape, 1), g2=_ints(full.shape, 2))
    return _REF[key]


def _slab_grads(shape, channels, g_full_k):
    """Gradients of the slabs for an upstream gradient g_full_k[B,K,...] of the full-K template: the restatement's own
    autograd (a move: exact)."""
    (TW, TH, TD), (ny, nx), B = shape
    r = _reference(shape, channels)
    rgb = None if r["rgb"] is None else r["rgb"].clone().requires_grad_(True)
    alpha = r["alpha"].clone().requires_grad_(True)
    C.slab_template(rgb, alpha, (TW, TH, TD), ny, nx).backward(g_full_k)
    return (None if rgb is None else rgb.grad), alpha.grad


@pytest.mark.parametrize("channels", [4, 1])
@pytest.mark.parametrize("mask", C.MASKS)
@pytest.mark.parametrize("shape", C.TEMPLATE_SHAPES)
def test_template_is_an_exact_move_forward_and_backward(shape, mask, channels, monkeypatch):
    """Activation off: compact, live and full=True (both outputs, both upstream gradients) are torch.equal to the
    restatement -- it is a move, no tolerance applies.  Kv = 0 returns empty tensors and zero gradients without a launch."""
    from goliath_amd import _lib, mvpprims

    (TW, TH, TD), (ny, nx), B = shape
    K = ny * nx
    r = _reference(shape, channels)
    valid = C.mask_of(mask, K)
    vd = valid.cuda()
    Kv = int(valid.sum())
    leaf = lambda t: None if t is None else t.cuda().requires_grad_(True)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])

    # compact: template[:, valid]
    rgb, alpha = leaf(r["rgb"]), leaf(r["alpha"])
    out = mvpprims.assemble_template(rgb, alpha, (TW, TH, TD), valid_prims=vd, compact=True)
    assert out.shape == (B, Kv, TD, TH, TW, 4)[:6 if channels == 4 else 5]
    assert torch.equal(out.cpu(), C.keep_valid(r["full"], valid))
    out.backward(C.keep_valid(r["g"], valid).cuda())
    want_rgb, want_a = _slab_grads(shape, channels, C.zero_invalid(r["g"], valid))
    assert torch.equal(alpha.grad.cpu(), want_a)
    assert channels == 1 or torch.equal(rgb.grad.cpu(), want_rgb)
    if Kv == 0:
        assert calls == [] and out.numel() == 0 and not alpha.grad.any()
    else:
        assert calls == ["gol_mvp_template_fwd", "gol_mvp_template_bwd"]

    # live: valid * template, every primitive keeps its place
    rgb, alpha = leaf(r["rgb"]), leaf(r["alpha"])
    out = mvpprims.assemble_template(rgb, alpha, (TW, TH, TD), valid_prims=vd, compact=False)
    assert torch.equal(out.cpu(), C.zero_invalid(r["full"], valid))
    out.backward(r["g"].cuda())
    assert torch.equal(alpha.grad.cpu(), want_a)
    assert channels == 1 or torch.equal(rgb.grad.cpu(), want_rgb)

    # full=True: the compacted template and the full-K one from the same loads, gradients through both
    rgb, alpha = leaf(r["rgb"]), leaf(r["alpha"])
    out, full = mvpprims.assemble_template(rgb, alpha, (TW, TH, TD), valid_prims=vd, compact=True, full=True)
    assert torch.equal(out.cpu(), C.keep_valid(r["full"], valid)) and torch.equal(full.cpu(), r["full"])
    torch.autograd.backward([out, full], [C.keep_valid(r["g"], valid).cuda(), r["g2"].cuda()])
    want_rgb, want_a = _slab_grads(shape, channels, C.zero_invalid(r["g"], valid) + r["g2"])
    assert torch.equal(alpha.grad.cpu(), want_a)
    assert channels == 1 or torch.equal(rgb.grad.cpu(), want_rgb)

    # no mask at all: all K primitives
    with torch.no_grad():
        out = mvpprims.assemble_template(None if channels == 1 else r["rgb"].cuda(), r["alpha"].cuda(), (TW, TH, TD))
    assert torch.equal(out.cpu(), r["full"])


@pytest.mark.parametrize("channels", [4, 1])
@pytest.mark.parametrize("shape", C.TEMPLATE_SHAPES)
def test_template_takes_four_byte_aligned_and_non_contiguous_slabs(shape, channels):
    from goliath_amd import mvpprims

    (TW, TH, TD), (ny, nx), B = shape
    r = _reference(shape, channels)
    valid = C.mask_of("ends", ny * nx)

    def odd(t):   # a contiguous view that starts at element 1 of a flat buffer: 4-byte aligned only
        flat = torch.empty(t.numel() + 1, device="cuda")
        flat[1:] = t.reshape(-1).cuda()
        v = flat[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    rgb = None if channels == 1 else odd(r["rgb"]).requires_grad_(True)
    alpha = odd(r["alpha"]).requires_grad_(True)
    out = mvpprims.assemble_template(rgb, alpha, (TW, TH, TD), valid_prims=valid.cuda())
    assert torch.equal(out.cpu(), C.keep_valid(r["full"], valid))
    g = C.keep_valid(r["g"], valid)
    out.backward(odd(g))                       # ... and an upstream gradient at an odd address
    want_rgb, want_a = _slab_grads(shape, channels, C.zero_invalid(r["g"], valid))
    assert torch.equal(alpha.grad.cpu(), want_a) and (channels == 1 or torch.equal(rgb.grad.cpu(), want_rgb))
    # non-contiguous: the slab stored with x and y swapped
    alpha_t = r["alpha"].cuda().transpose(-1, -2).contiguous().transpose(-1, -2)
    rgb_t = None if channels == 1 else r["rgb"].cuda().transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not alpha_t.is_contiguous()
    with torch.no_grad():
        out = mvpprims.assemble_template(rgb_t, alpha_t, (TW, TH, TD), valid_prims=valid.cuda())
    assert torch.equal(out.cpu(), C.keep_valid(r["full"], valid))
    # the 4-D alpha slab of the teacher
    with torch.no_grad():
        out = mvpprims.assemble_template(None, r["alpha"][:, :, 0].cuda(), (TW, TH, TD), valid_prims=valid.cuda(), compact=False)
    assert torch.equal(out.cpu(), C.zero_invalid(_reference(shape, 1)["full"], valid))


@pytest.mark.parametrize("channels", [4, 1])
@pytest.mark.parametrize("shape", C.TEMPLATE_SHAPES)
def test_template_backward_writes_every_element(shape, channels):
    """The C entry itself, with g_rgb / g_alpha full of NaN beforehand: every element is written (dropped primitives get
    zeros), so the wrapper may allocate with `empty`."""
    from goliath_amd import _lib, mvpprims

    (TW, TH, TD), (ny, nx), B = shape
    r = _reference(shape, channels)
    valid = C.mask_of("alternating", ny * nx)
    slot, live, Kv = mvpprims.prim_slots(valid.cuda())
    g_out = C.keep_valid(r["g"], valid).cuda()
    g_rgb = torch.full(r["rgb"].shape, float("nan"), device="cuda") if channels == 4 else None
    g_alpha = torch.full(r["alpha"].shape, float("nan"), device="cuda")
    with _lib.device_guard(g_out.device):
        mvpprims._abi_mvp_template_bwd(B=B, TD=TD, TH=TH, TW=TW, ny=ny, nx=nx, rgb=None, alpha=None, slot=slot, live=live,
                                       Kout=Kv, act=0, rgb_scale=1.0, rgb_shift=0.0, g_out=g_out, g_out_full=None,
                                       g_rgb=g_rgb, g_alpha=g_alpha)
    want_rgb, want_a = _slab_grads(shape, channels, C.zero_invalid(r["g"], valid))
    assert torch.equal(g_alpha.cpu(), want_a) and (channels == 1 or torch.equal(g_rgb.cpu(), want_rgb))


def _ulp(x):
    ax = x.abs()
    return torch.nextafter(ax, torch.full_like(ax, math.inf)) - ax


@pytest.mark.parametrize("channels", [4, 1])
@pytest.mark.parametrize("shape", C.TEMPLATE_SHAPES)
def test_template_with_the_activation_fused(shape, channels):
    """relu(scale x + shift) on the colours, relu(x) on alpha.  Forward: within 2 ulp of the float32 composition
    relu(scale * x + shift).  The bound would allow a kernel that contracts the multiply-add to one FMA wherever the
    product does not cancel against the shift; the inputs here are the hard case on purpose -- the reference's 25 x + 100
    with x around -4, results of +-0.5 under intermediates of 100, where an FMA would be up to 64 ulp of the result away --
    and the kernel rounds product and sum separately, so it meets the bound there too.  The inputs keep
    |scale x + shift| > 1e-3 (away from the kink).  Backward: the relu masks are identical, values within 2 ulp
    (g * scale is one product on both sides)."""
    from goliath_amd import mvpprims

    (TW, TH, TD), (ny, nx), B = shape
    K = ny * nx
    scale, shift = 25.0, 100.0
    g = torch.Generator().manual_seed(7)
    rgb = -4.0 + 0.02 * torch.randn(B, TD, 3, ny * TH, nx * TW, generator=g)   # 25 x + 100 ~ N(0, 0.5): half are cut
    rgb = torch.where((scale * rgb + shift).abs() > 2e-3, rgb, rgb + 1e-3)
    alpha = torch.randn(B, TD, 1, ny * TH, nx * TW, generator=g)
    alpha = torch.where(alpha.abs() > 1e-3, alpha, alpha + 1e-2)
    assert float((scale * rgb + shift).abs().min()) > 1e-3 and float(alpha.abs().min()) > 1e-3
    valid = C.mask_of("ends", K)
    rgb_d = None if channels == 1 else rgb.cuda().requires_grad_(True)
    alpha_d = alpha.cuda().requires_grad_(True)
    out, full = mvpprims.assemble_template(rgb_d, alpha_d, (TW, TH, TD), valid_prims=valid.cuda(), rgb_affine=(scale, shift),
                                           full=True)
    rgb_r = None if channels == 1 else rgb.clone().requires_grad_(True)
    alpha_r = alpha.clone().requires_grad_(True)
    want_full = C.slab_template(*C.activate(rgb_r, alpha_r, scale, shift), (TW, TH, TD), ny, nx)
    want = C.keep_valid(want_full, valid)
    assert bool(((out.cpu() - want).abs() <= 2 * _ulp(want)).all())
    assert bool(((full.cpu() - want_full).abs() <= 2 * _ulp(want_full)).all())
    assert 0.2 < float((want_full == 0).float().mean()) < 0.8       # both sides of the kink are exercised
    go, gf = 1.0 + torch.rand(want.shape, generator=g), 1.0 + torch.rand(want_full.shape, generator=g)   # never zero
    torch.autograd.backward([out, full], [go.cuda(), gf.cuda()])
    torch.autograd.backward([want, want_full], [go, gf])
    pairs = [(alpha_d.grad.cpu(), alpha_r.grad)] + ([] if channels == 1 else [(rgb_d.grad.cpu(), rgb_r.grad)])
    for got, ref in pairs:
        assert torch.equal(got != 0, ref != 0)
        assert bool(((got - ref).abs() <= 2 * _ulp(ref)).all())
    # relu=True alone: alpha cut, colours relu(x)
    with torch.no_grad():
        out = mvpprims.assemble_template(None, alpha.cuda(), (TW, TH, TD), relu=True)
    assert torch.equal(out.cpu(), C.slab_template(None, torch.relu(alpha), (TW, TH, TD), ny, nx))


# ------------------------------------------------------------------------------------------------- primitive transforms
_PARITY = {}


def _write_parity():
    """mvpprims_parity.json in the project's report directory (where bench.py leaves its detail report and conftest.py the
    parity ledger), when that directory exists."""
    import bench

    out_dir = os.path.dirname(bench.DETAIL_PATH)
    if os.path.isdir(out_dir):
        json.dump(_PARITY, open(os.path.join(out_dir, "mvpprims_parity.json"), "w"), indent=1)


@pytest.mark.parametrize("K", [5, 130])
def test_prim_transforms_against_float64(K):
    """Forward and the three gradients against the float64 restatement, rel-L2.  The bar is what single precision costs the
    PyTorch composition on the same inputs (measured here, float32 restatement on the CPU against float64), times 4, with a
    floor of 1e-6: fast sin / cos / rsqrt against libm, a few ulp per operation over about 20 operations."""
    from goliath_amd import mvpprims

    B = 2
    t64 = C.transform_inputs(B, K, seed=K)
    g = torch.Generator().manual_seed(3)
    ups64 = [torch.randn(B, K, 3, generator=g, dtype=torch.float64), torch.randn(B, K, 3, 3, generator=g, dtype=torch.float64),
             torch.randn(B, K, 3, generator=g, dtype=torch.float64)]
    t32 = {k: v.float() for k, v in t64.items()}           # what both float32 paths see
    t64 = {k: v.double() for k, v in t32.items()}
    ups32 = [u.float() for u in ups64]
    ups64 = [u.double() for u in ups32]
    names = ("delta_pos", "delta_rvec", "delta_scale")

    def run(t, ups, fn, dev):
        t = {k: v.detach().clone().to(dev) for k, v in t.items()}
        for k in names:
            t[k].requires_grad_(True)
        outs = fn(**t, prim_scale=512.0)
        torch.autograd.backward(list(outs), [u.to(dev) for u in ups])
        return list(outs) + [t[k].grad for k in names]

    ref = run(t64, ups64, C.transform_tail, "cpu")
    f32 = run(t32, ups32, C.transform_tail, "cpu")
    got = run(t32, ups32, mvpprims.prim_transforms, "cuda")
    rec = {}
    for name, r, a, b in zip(("primpos", "primrot", "primscale", "g_delta_pos", "g_delta_rvec", "g_delta_scale"), ref, f32, got):
        assert bool(torch.isfinite(b).all()), name            # rows 0 of delta_rvec are exactly zero
        e_torch = scenes.rel_l2(a, r)
        e_kernel = scenes.rel_l2(b, r)
        bar = max(4.0 * e_torch, 1e-6)
        rec[name] = dict(float32_torch=e_torch, kernel=e_kernel, bar=bar)
        print(f"PRIMTRANSF K={K} {name}: kernel {e_kernel:.3e}  float32 torch {e_torch:.3e}  bar {bar:.3e}")
    _PARITY[f"prim_transforms_K{K}"] = rec
    _write_parity()
    for name, v in rec.items():
        assert v["kernel"] <= v["bar"], (name, v)
    assert not t32["delta_rvec"][:, 0].any() and bool(torch.isfinite(got[4][:, 0]).all())   # finite at r = 0


# ------------------------------------------------------------------------------------------------------- model level
VOLRADIUS = 2.0
PRIMSIZE = (16, 16, 8)
UV, NY, NX, IMG_H, IMG_W = 64, 4, 4, 64, 96


def _autoencoder(full_template=False):
    from goliath_amd import mvp, mvpprims

    y, x = torch.meshgrid(torch.arange(IMG_H), torch.arange(IMG_W), indexing="ij")
    ae = types.SimpleNamespace(primsize=PRIMSIZE, n_prim_x=NX, n_prim_y=NY, n_prims=NY * NX,
                               pixel_coords=torch.stack([x, y], dim=-1).float().cuda(),
                               raymarcher=mvp.Raymarcher(volradius=VOLRADIUS, dt=0.1))
    setattr(ae, mvpprims.FULL_TEMPLATE_FLAG, full_template)
    return ae


def _model_inputs(B=2, seed=11):
    """16 boxes on a 4 x 4 lattice in a volume of radius 2, seen from z = -6."""
    g = torch.Generator().manual_seed(seed)
    K = NY * NX
    lin = torch.linspace(-0.6, 0.6, 4)
    cy, cx = torch.meshgrid(lin, lin, indexing="ij")
    centres = torch.stack([cx, cy, 0.2 * torch.sin(3 * cx + 2 * cy)], -1).reshape(1, K, 3)
    primpos = VOLRADIUS * (centres + 0.03 * torch.randn(B, K, 3, generator=g))
    t = C.transform_inputs(B, K, seed=seed)
    primrot = t["rotbase"].float()
    primscale = 4.0 * (0.8 + 0.4 * torch.rand(B, K, 3, generator=g))
    S = UV
    primrgb = torch.nn.functional.softplus(1.5 * torch.randn(B, PRIMSIZE[2], 3, S, S, generator=g))
    primalpha = torch.nn.functional.softplus(1.5 * torch.randn(B, PRIMSIZE[2], 1, S, S, generator=g) - 1.0)
    valid = C.mask_of("ends", K)
    valid[5] = False
    campos = torch.tensor([[0.2, -0.4, -6.0]]).repeat(B, 1) + 0.1 * torch.randn(B, 3, generator=g)
    Rt = torch.cat([torch.eye(3)[None].repeat(B, 1, 1), -campos[..., None]], -1)      # camrot = I: t = -campos
    Km = torch.zeros(B, 3, 3)
    Km[:, 0, 0] = Km[:, 1, 1] = 1.6 * IMG_W
    Km[:, 0, 2], Km[:, 1, 2], Km[:, 2, 2] = IMG_W / 2, IMG_H / 2, 1.0
    leaves = dict(primrgb=primrgb, primalpha=primalpha, primpos=primpos, primrot=primrot, primscale=primscale)
    return leaves, valid, Km, Rt


def _parent_render(ae, K, Rt, preds, with_shadow=False):
    """The path of the parent commit: hand_mvp.AutoEncoder.render restated on the PyTorch rearrangement, the explicit pixel
    grid and goliath_amd.mvp.Raymarcher (boolean-mask selection)."""
    from goliath_amd import mvp

    B = K.shape[0]
    preds["primrgba"] = C.slab_template(preds["primrgb"], preds["primalpha"], ae.primsize, ae.n_prim_y, ae.n_prim_x)
    focal = torch.diagonal(K[:, :2, :2].contiguous(), dim1=1, dim2=2).contiguous()
    princpt = K[:, :2, 2].contiguous()
    camrot = Rt[:, :3, :3].contiguous()
    campos = -(camrot.transpose(-2, -1) @ Rt[:, :3, 3:4])[..., 0]
    pixelcoords = ae.pixel_coords[None].expand(B, -1, -1, -1).contiguous()
    raypos, raydir, tminmax = mvp.compute_raydirs(campos, camrot, focal, princpt, pixelcoords, ae.raymarcher.volume_radius)
    rayrgb, rayalpha, _, shadow = ae.raymarcher(raypos, raydir, tminmax, preds, with_shadow=with_shadow)
    return rayrgb, rayalpha, shadow


def _step(render, ae, leaves, valid, Km, Rt, weights=None, with_shadow=False):
    leaf = {k: v.cuda().requires_grad_(True) for k, v in leaves.items()}
    preds = dict(leaf, valid_prims=valid)
    rgb, alpha, shadow = render(ae, Km, Rt, preds, with_shadow=with_shadow)
    if weights is None:
        g = torch.Generator().manual_seed(5)
        weights = (torch.randn(rgb.shape, generator=g).cuda(), torch.randn(alpha.shape, generator=g).cuda())
    torch.autograd.backward([rgb, alpha], list(weights))
    return rgb, alpha, shadow, {k: v.grad for k, v in leaf.items()}, preds, weights


def test_patched_render_equals_the_parent_path():
    """Same kernels, same template bits: rgb and alpha are torch.equal; the gradients agree to the project's 1e-4 rel-L2
    bar (the march backward's float atomics reorder between runs)."""
    from goliath_amd import mvpprims

    leaves, valid, Km, Rt = _model_inputs()
    valid, Km, Rt = valid.cuda(), Km.cuda(), Rt.cuda()
    ae = _autoencoder()
    rgb0, alpha0, sh0, grads0, preds0, w = _step(_parent_render, ae, leaves, valid, Km, Rt, with_shadow=True)
    rgb1, alpha1, sh1, grads1, preds1, _ = _step(mvpprims.hand_mvp_render, ae, leaves, valid, Km, Rt, w, with_shadow=True)
    assert float(alpha0.detach().max()) > 0.2 and float((alpha0.detach() > 0).float().mean()) > 0.2   # the boxes are in view
    assert rgb1.shape == (2, 3, IMG_H, IMG_W) and alpha1.shape == (2, 1, IMG_H, IMG_W)
    assert torch.equal(rgb1, rgb0) and torch.equal(alpha1, alpha0)
    assert sh1.shape == sh0.shape and scenes.rel_l2(sh1, sh0) < 1e-4
    assert "primrgba" not in preds1
    for k in grads0:
        assert float(grads0[k].abs().max()) > 0
        e = scenes.rel_l2(grads1[k], grads0[k])
        assert e < 1e-4, (k, e)
    # full_template=True: preds["primrgba"] is the reference's full-K template
    out = _step(mvpprims.hand_mvp_render, _autoencoder(full_template=True), leaves, valid, Km, Rt, w)
    assert torch.equal(out[0], rgb0) and torch.equal(out[4]["primrgba"], preds0["primrgba"])
    # a pixel grid that is not the standard one is handed over as it is
    ae2 = _autoencoder()
    ae2.pixel_coords = ae2.pixel_coords + 0.25
    a, b = _step(_parent_render, ae2, leaves, valid, Km, Rt, w), _step(mvpprims.hand_mvp_render, ae2, leaves, valid, Km, Rt, w)
    assert torch.equal(a[0], b[0]) and not torch.equal(a[0], rgb0)


def test_patched_render_with_no_valid_primitive(monkeypatch):
    from goliath_amd import _lib, mvpprims

    leaves, valid, Km, Rt = _model_inputs(B=1)
    none = torch.zeros_like(valid).cuda()
    mvpprims.prim_slots(none)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    leaf = {k: v.cuda().requires_grad_(True) for k, v in leaves.items()}
    rgb, alpha, shadow = mvpprims.hand_mvp_render(_autoencoder(), Km.cuda(), Rt.cuda(), dict(leaf, valid_prims=none))
    assert calls == [] and shadow is None
    assert rgb.shape == (1, 3, IMG_H, IMG_W) and alpha.shape == (1, 1, IMG_H, IMG_W) and not rgb.any() and not alpha.any()


def test_render_and_transforms_run_without_a_host_sync():
    from goliath_amd import mvpprims

    leaves, valid, Km, Rt = _model_inputs()
    valid, Km, Rt = valid.cuda(), Km.cuda(), Rt.cuda()
    ae = _autoencoder()
    t = {k: v.float().cuda() for k, v in C.transform_inputs(2, NY * NX, seed=2).items()}
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(2, 3, IMG_H, IMG_W, generator=g).cuda(), torch.randn(2, 1, IMG_H, IMG_W, generator=g).cuda())

    def step():
        d = {k: t[k].clone().requires_grad_(True) for k in ("delta_pos", "delta_rvec", "delta_scale")}
        pos, rot, scale = mvpprims.prim_transforms(t["posbase"], t["rotbase"], **d, prim_scale=512.0)
        (pos.sum() + rot.sum() + scale.sum()).backward()
        out = _step(mvpprims.hand_mvp_render, ae, leaves_d, valid, Km, Rt, w)
        return [out[0], out[1], *out[3].values(), *(v.grad for v in d.values())]

    leaves_d = {k: v.cuda() for k, v in leaves.items()}
    step()                                     # loads the library, builds the tables of the mask and checks the pixel grid
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(o).all()) for o in out)


# ---- GeomDecoder.forward on a stand-in class (the helpers are looked up in the module that defines it: this one) ----------
def make_postex(geom, vidx_img, bary_img):
    return (geom[:, vidx_img] * bary_img[None, ..., None]).sum(-2).permute(0, 3, 1, 2)       # [B,3,n,n]


def compute_tbn(geom, vt, vidx_img, vtidx_img):
    tri = geom[:, vidx_img]                                                                   # [B,n,n,3,3]
    t = torch.nn.functional.normalize(tri[..., 1, :] - tri[..., 0, :], dim=-1)
    n = torch.nn.functional.normalize(torch.cross(t, tri[..., 2, :] - tri[..., 0, :], dim=-1), dim=-1)
    return t, torch.cross(n, t, dim=-1), n


class _Lbs:
    def __init__(self, V):
        g = torch.Generator().manual_seed(4)
        self.lbs_template_verts = torch.randn(1, V, 3, generator=g).cuda()
        self.basis = torch.randn(6, V, 3, generator=g).cuda()

    def pose(self, verts, pose):
        return verts + self.lbs_template_verts + torch.einsum("bp,pvc->bvc", pose, self.basis)


class StandInGeomDecoder(torch.nn.Module):
    def __init__(self, n=4, V=20, primsize_z=8, uv_size=64):
        super().__init__()
        g = torch.Generator().manual_seed(6)
        self.lbs_fn, self.geo_fn = _Lbs(V), types.SimpleNamespace(vt=None)
        self.n_prims, self.primsize_z, self.uv_size, self.prim_scale, self.primposstart = n * n, primsize_z, uv_size, 512, 1000
        self.register_buffer("prim_vidx_img", torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(n * n)]).reshape(n, n, 3))
        self.register_buffer("prim_vtidx_img", self.prim_vidx_img.clone())
        self.register_buffer("prim_bary_img", torch.softmax(torch.randn(n, n, 3, generator=g), -1))
        self.trans = torch.nn.Linear(6, n * n * 9)
        self.alpha = torch.nn.Linear(6, primsize_z * 8 * 8)

    def transdecoder(self, joint):
        out = self.trans(joint).view(joint.shape[0], -1, 9)
        return out[:, :, 0:3], out[:, :, 3:6] * 0.3, torch.exp(0.1 * out[:, :, 6:9])

    def alphadecoder(self, joint):
        a = self.alpha(joint).view(joint.shape[0], self.primsize_z, 8, 8)
        return torch.nn.functional.interpolate(a, (self.uv_size, self.uv_size), mode="bilinear")

    def forward(self, pose, joint, iteration=-1):
        """GeomDecoder.forward with the transform tail as the PyTorch restatement."""
        B = pose.shape[0]
        with torch.no_grad():
            geom_lbs = self.lbs_fn.pose(torch.zeros_like(self.lbs_fn.lbs_template_verts), pose)
            posbase = make_postex(geom_lbs, self.prim_vidx_img, self.prim_bary_img).permute(0, 2, 3, 1).reshape(B, -1, 3)
            tbn = compute_tbn(geom_lbs, None, self.prim_vidx_img, self.prim_vtidx_img)
            rotbase = torch.stack(tbn, dim=-2).reshape(B, self.n_prims, 3, 3).permute(0, 1, 3, 2).contiguous()
        dp, dr, ds = self.transdecoder(joint)
        if self.training and iteration < self.primposstart:
            dp, dr, ds = dp * 0.0, dr * 0.0, ds * 0.0 + 1.0
        primpos, primrot, primscale = C.transform_tail(posbase, rotbase, dp, dr, ds, self.prim_scale)
        alpha = torch.relu(self.alphadecoder(joint).view(B, self.primsize_z, 1, self.uv_size, self.uv_size))
        return {"primalpha": alpha, "primpos": primpos, "primscale": primscale, "primrot": primrot, "geom_lbs": geom_lbs}


@pytest.mark.parametrize("training,iteration", [(False, -1), (True, 5), (True, 2000)])
def test_patched_geom_decoder_forward(training, iteration):
    """The same sub-module calls, the warm-up branch (delta_rvec exactly zero) and the relu on alpha; the transform tail on the
    kernel.  float32 on both sides: 1e-5 rel-L2 for the outputs, the project's 1e-4 for the parameter gradients."""
    from goliath_amd import mvpprims

    dec = StandInGeomDecoder().cuda().train(training)
    g = torch.Generator().manual_seed(8)
    pose, joint = torch.randn(2, 6, generator=g).cuda(), torch.randn(2, 6, generator=g).cuda()
    ups = None
    res = []
    for fn in (StandInGeomDecoder.forward, mvpprims.geom_decoder_forward):
        dec.zero_grad()
        out = fn(dec, pose, joint, iteration)
        keys = ("primpos", "primrot", "primscale", "primalpha")
        if ups is None:
            ups = [torch.randn(out[k].shape, generator=g).cuda() for k in keys]
        torch.autograd.backward([out[k] for k in keys], ups)
        res.append((out, [None if p.grad is None else p.grad.clone() for p in dec.parameters()]))
    (a, ga), (b, gb) = res
    assert list(a) == list(b) and torch.equal(a["geom_lbs"], b["geom_lbs"]) and torch.equal(a["primalpha"], b["primalpha"])
    for k in ("primpos", "primrot", "primscale"):
        assert bool(torch.isfinite(b[k]).all()) and scenes.rel_l2(b[k], a[k]) < 1e-5, k
    for x, y in zip(ga, gb):
        assert bool(torch.isfinite(y).all()) and (scenes.rel_l2(y, x) < 1e-4 or not x.any() and not y.any())
