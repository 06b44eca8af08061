"""mvptail on the GPU: the fused decoder tail against the float64 twin, its layout contract, and the model binding."""
import itertools
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mvptail_cases as C
import scenes

pytestmark = pytest.mark.gpu


def _leaves(i, one_channel=False, requires=None):
    d = C.draws(i)
    names = C.LEAVES[3:] if one_channel else C.LEAVES
    requires = names if requires is None else requires
    leaf = {k: d[k].float().cuda().requires_grad_(k in requires) for k in names}
    return leaf, [leaf.get(k) for k in C.LEAVES]


def _upstream(i, mask=None, compact=True, one_channel=False):
    g = C.reference(i)["g_out"]
    g = g[..., 3] if one_channel else g
    if mask is not None and compact:
        g = g[:, mask]
    return g.float().contiguous().cuda()


def _run(i, mask=None, compact=True, one_channel=False, requires=None, g_out=None):
    from goliath_amd import mvptail

    leaf, args = _leaves(i, one_channel, requires)
    m = None if mask is None else mask.cuda()
    out = mvptail.decode_template(*args, C.primsize(C.SHAPES[i]), valid_prims=m, compact=compact, rgb_affine=C.AFFINE)
    if any(v.requires_grad for v in leaf.values()):
        out.backward(_upstream(i, mask, compact, one_channel) if g_out is None else g_out)
    return out.detach(), {k: v.grad for k, v in leaf.items()}


# ----------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("i", range(len(C.SHAPES)))
def test_parity_with_the_float64_twin(i):
    """The template and the six gradients against decode_template_torch in float64: 1e-5 rel-L2, the bar of
    test_gpu_trunk.py, test_gpu_encoder.py and test_gpu_texdec.py."""
    want, gwant = C.twin_grads(i)
    got, ggot = _run(i)
    assert got.shape == want.shape and got.dtype == torch.float32
    errs = {"out": scenes.rel_l2(got, want), **{k: scenes.rel_l2(ggot[k], gwant[k]) for k in C.LEAVES}}
    print(C.SHAPES[i], {k: f"{v:.2e}" for k, v in errs.items()})
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)


@pytest.mark.parametrize("i", [0, 2, 5])
def test_one_channel_variant(i):
    """x_rgb = None: relu(pre_alpha) in the teacher's one-channel template layout, and its three gradients."""
    want, gwant = C.twin_grads(i, one_channel=True)
    B, TD, TH, TW, ny, nx = C.SHAPES[i]
    assert want.shape == (B, ny * nx, TD, TH, TW) and torch.equal(want, C.reference(i)["out"][..., 3])
    got, ggot = _run(i, one_channel=True)
    assert got.shape == want.shape
    errs = {"out": scenes.rel_l2(got, want), **{k: scenes.rel_l2(ggot[k], gwant[k]) for k in C.LEAVES[3:]}}
    print(C.SHAPES[i], {k: f"{v:.2e}" for k, v in errs.items()})
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)


# ----------------------------------------------------------------------------------------------------------------- layout
def _reach(mask, shape):
    """which bias texels [Sy,Sx] and which input pixels [h,w] a kept primitive reaches"""
    _, _, TH, TW, ny, nx = shape
    texel = mask.view(ny, nx).repeat_interleave(TH, 0).repeat_interleave(TW, 1)
    pixel = F.conv2d(texel[None, None].float(), torch.ones(1, 1, 4, 4), stride=2, padding=1)[0, 0] > 0
    return texel, pixel


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("kind", C.MASKS)
def test_written_primitives_and_exact_zeros(kind, compact, monkeypatch):
    from goliath_amd import _lib

    i = C.MASK_SHAPE
    shape = C.SHAPES[i]
    B, TD, TH, TW, ny, nx = shape
    mask = C.mask_of(kind, ny * nx)
    Kv = int(mask.sum()) if compact else ny * nx
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    cmask = mask.cuda()
    from goliath_amd import mvptail

    leaf, args = _leaves(i)
    out = mvptail.decode_template(*args, C.primsize(shape), valid_prims=cmask, compact=compact)
    assert out.shape == (B, Kv, TD, TH, TW, 4)
    g = _upstream(i, mask, compact)
    torch.autograd.backward([out], [g])
    grads = {k: v.grad.cpu() for k, v in leaf.items()}
    if Kv == 0:
        assert calls == [] and out.numel() == 0
        assert all(not v.any() and v.shape == leaf[k].shape for k, v in grads.items())
        return
    assert calls == ["gol_mvp_tail_fwd", "gol_mvp_tail_bwd"]
    want, gwant = C.twin_grads(i, mask, compact)
    keep = C.select(C.reference(i)["keep"], mask, compact) != 0
    got = out.detach().cpu()
    assert torch.equal((got != 0) & keep, (want != 0) & keep)
    if not compact:
        assert not got[:, ~mask].any()
    assert scenes.rel_l2(got, want) <= 1e-5
    for k in C.LEAVES:
        assert scenes.rel_l2(grads[k], gwant[k]) <= 1e-5 or not gwant[k].any(), k
    texel, pixel = _reach(mask, shape)
    for k in ("bias_rgb", "bias_alpha"):
        assert not grads[k][:, ~texel].any(), k
    for k in ("x_rgb", "x_alpha"):
        assert not grads[k][:, :, ~pixel].any(), k
    if not mask.any():
        assert not grads["w_rgb"].any() and not grads["w_alpha"].any()


# --------------------------------------------------------------------------------------------------- the autograd contract
def test_every_subset_of_needs_input_grad():
    i = 2
    _, full = _run(i)
    for r in range(len(C.LEAVES)):
        for sub in itertools.combinations(C.LEAVES, r):
            _, grads = _run(i, requires=sub)
            for k in C.LEAVES:
                if k in sub:
                    assert torch.equal(grads[k], full[k]), (sub, k)
                else:
                    assert grads[k] is None, (sub, k)


def test_two_calls_are_bitwise_equal():
    i = C.MASK_SHAPE
    mask = C.mask_of("ends", 45)
    a, ga = _run(i, mask)
    b, gb = _run(i, mask)
    assert torch.equal(a, b) and all(torch.equal(ga[k], gb[k]) for k in C.LEAVES)


@pytest.mark.parametrize("one_channel", [False, True])
def test_upstream_gradient_at_an_odd_address(one_channel):
    i = 2
    g = _upstream(i, one_channel=one_channel)
    buf = torch.empty(g.numel() + 8, device="cuda")
    off = 1 + (-(buf.data_ptr() // 4) % 4)             # element offset that lands at 4 (mod 16) bytes
    odd = buf[off:off + g.numel()].view(g.shape)
    odd.copy_(g)
    assert odd.data_ptr() % 16 == 4
    _, want = _run(i, one_channel=one_channel, g_out=g)
    _, got = _run(i, one_channel=one_channel, g_out=odd)
    assert all(torch.equal(got[k], want[k]) for k in want)


# ------------------------------------------------------------------------------------------------------------ model level
VOLRADIUS = 2.0
PRIMSIZE = (4, 4, 2)
UV, NY, NX, IMG_H, IMG_W = 32, 8, 8, 64, 96
EMB = 8


def make_postex(geom, vidx_img, bary_img):
    return (geom[:, vidx_img] * bary_img[None, ..., None]).sum(-2).permute(0, 3, 1, 2)


def compute_tbn(geom, vt, vidx_img, vtidx_img):
    tri = geom[:, vidx_img]
    t = F.normalize(tri[..., 1, :] - tri[..., 0, :], dim=-1)
    n = F.normalize(torch.cross(t, tri[..., 2, :] - tri[..., 0, :], dim=-1), dim=-1)
    return t, torch.cross(n, t, dim=-1), n


class _Lbs:
    def __init__(self, V):
        g = torch.Generator().manual_seed(4)
        self.lbs_template_verts = (0.5 * torch.randn(1, V, 3, generator=g)).cuda()
        self.basis = (0.05 * torch.randn(6, V, 3, generator=g)).cuda()

    def pose(self, verts, pose):
        return verts + self.lbs_template_verts + torch.einsum("bp,pvc->bvc", pose, self.basis)


class DeconvContentDecoder(nn.Module):
    """hand_mvp.DeconvContentDecoder at a quarter of its depth, behind a pooling of the 64^2 embedding:
    inch x 64^2 -> inch x 8^2 -> 16 x 16^2 -> TD outch x 32^2"""

    def __init__(self, primsize_z, inch, outch, plain_last=False):
        super().__init__()
        from goliath_amd.decoder import ConvTranspose2dWNUB

        last = nn.ConvTranspose2d(16, primsize_z * outch, 4, 2, 1) if plain_last else \
            ConvTranspose2dWNUB(16, primsize_z * outch, UV, UV, alpha=1.0)
        self.texbranch = nn.Sequential(nn.AvgPool2d(8), ConvTranspose2dWNUB(inch, 16, UV // 2, UV // 2), nn.LeakyReLU(0.2), last)

    def forward(self, x):
        return self.texbranch(x)


class GeomDecoder(nn.Module):
    def __init__(self, plain_last=False, V=40):
        super().__init__()
        g = torch.Generator().manual_seed(6)
        self.lbs_fn, self.geo_fn = _Lbs(V), types.SimpleNamespace(vt=None)
        self.n_prims, self.primsize_z, self.uv_size, self.prim_scale, self.primposstart = NY * NX, PRIMSIZE[2], UV, 4.0, 1000
        self.register_buffer("prim_vidx_img", torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(NY * NX)]).reshape(NY, NX, 3))
        self.register_buffer("prim_vtidx_img", self.prim_vidx_img.clone())
        self.register_buffer("prim_bary_img", torch.softmax(torch.randn(NY, NX, 3, generator=g), -1))
        self.trans = nn.Linear(EMB * 64, NY * NX * 9)
        self.alphadecoder = DeconvContentDecoder(PRIMSIZE[2], EMB, 1, plain_last)

    def transdecoder(self, joint):
        out = self.trans(F.avg_pool2d(joint, 8).flatten(1)).view(joint.shape[0], -1, 9)
        return out[:, :, 0:3] * 0.01, out[:, :, 3:6] * 0.1, torch.exp(0.1 * out[:, :, 6:9])

    def forward(self, pose, joint, iteration=-1):       # replaced by patch_hand_mvp
        raise NotImplementedError


class RGBSlabDecoder(nn.Module):
    def __init__(self, plain_last=False):
        super().__init__()
        self.primsize_z, self.uv_size = PRIMSIZE[2], UV
        self.texdecoder = DeconvContentDecoder(PRIMSIZE[2], EMB + 2, 3, plain_last)

    def forward(self, view_cos_uv, joint, ambient_occlusion):
        """hand_mvp.RGBSlabDecoder.forward restated"""
        B = joint.shape[0]
        ao_ds = F.interpolate(ambient_occlusion, (64, 64), mode="bilinear")
        view_cond = torch.cat((joint, view_cos_uv, ao_ds), 1)
        rgb = self.texdecoder(view_cond).view(B, self.primsize_z, 3, self.uv_size, self.uv_size)
        return F.relu(25.0 * rgb + 100.0)


class AutoEncoder(nn.Module):
    def __init__(self, plain_last=False):
        super().__init__()
        from goliath_amd import mvp

        torch.manual_seed(21)
        self.primsize, self.n_prim_x, self.n_prim_y, self.n_prims = PRIMSIZE, NX, NY, NY * NX
        self.geomdecoder, self.rgbdecoder = GeomDecoder(plain_last), RGBSlabDecoder(plain_last)
        self.raymarcher = mvp.Raymarcher(volradius=VOLRADIUS, dt=0.1)
        y, x = torch.meshgrid(torch.arange(IMG_H), torch.arange(IMG_W), indexing="ij")
        self.register_buffer("pixel_coords", torch.stack([x, y], dim=-1).float(), persistent=False)
        valid = torch.ones(NY * NX, dtype=torch.bool)
        valid[[0, 5, 17, 40, 63]] = False
        self.register_buffer("valid_prims", valid, persistent=False)
        with torch.no_grad():       # both sides of both kinks: the colours around 25 x + 100 = 0, alpha around 0
            for dec, bias, spread in ((self.geomdecoder.alphadecoder, 0.0, 0.5), (self.rgbdecoder.texdecoder, -4.0, 0.04)):
                last = dec.texbranch[-1]
                if not plain_last:
                    last.bias.copy_(bias + spread * torch.randn(last.bias.shape))
                    last.weight_g.mul_(4.0)

    def render(self, K, Rt, preds, with_shadow=False):  # replaced by patch_hand_mvp
        raise NotImplementedError

    def forward(self, pose, joint, view_cos_uv, ao, K, Rt):
        """hand_mvp.AutoEncoder.forward (:224-247) from the pose embedding on"""
        geo_preds = self.geomdecoder(pose, joint, 2000)
        primrgb = self.rgbdecoder(view_cos_uv, joint, ao)
        preds = {"primrgb": primrgb, "valid_prims": self.valid_prims, **geo_preds}
        rgb, alpha, _ = self.render(K, Rt, preds, with_shadow=False)
        preds.update(rgb=rgb, alpha=alpha)
        return preds


def _module():
    return types.SimpleNamespace(AutoEncoder=AutoEncoder, GeomDecoder=GeomDecoder, RGBSlabDecoder=RGBSlabDecoder)


def _model_inputs(B=2):
    g = torch.Generator().manual_seed(11)
    pose, joint = 0.3 * torch.randn(B, 6, generator=g), torch.randn(B, EMB, 64, 64, generator=g)
    view_cos_uv, ao = torch.rand(B, 1, 64, 64, generator=g), torch.rand(B, 1, 16, 16, generator=g)
    campos = torch.tensor([[0.2, -0.4, -6.0]]).repeat(B, 1) + 0.1 * torch.randn(B, 3, generator=g)
    Rt = torch.cat([torch.eye(3)[None].repeat(B, 1, 1), -campos[..., None]], -1)
    Km = torch.zeros(B, 3, 3)
    Km[:, 0, 0] = Km[:, 1, 1] = 1.6 * IMG_W
    Km[:, 0, 2], Km[:, 1, 2], Km[:, 2, 2] = IMG_W / 2, IMG_H / 2, 1.0
    w = (torch.randn(B, 3, IMG_H, IMG_W, generator=g), torch.randn(B, 1, IMG_H, IMG_W, generator=g))
    return [t.cuda() for t in (pose, joint, view_cos_uv, ao, Km, Rt)], [t.cuda() for t in w]


def _step(ae, inputs, weights, monkeypatch):
    """one forward + backward; returns the images, the template the march took, the recorded ABI calls, preds, gradients"""
    from goliath_amd import _lib, mvp

    seen, calls = {}, []
    real_march, real_call = mvp.mvpraymarch, _lib.call

    def march(*a, template=None, **kw):
        seen["template"] = template.detach().clone()
        return real_march(*a, template=template, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(mvp, "mvpraymarch", march)
        mp.setattr(_lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
        ae.zero_grad()
        preds = ae(*inputs)
        torch.autograd.backward([preds["rgb"], preds["alpha"]], weights)
    grads = {n: p.grad.clone() for n, p in ae.named_parameters() if p.grad is not None}
    return preds, seen["template"], calls, grads


def test_model_binding(monkeypatch):
    """A twin of the student's AutoEncoder (UV 32^2, primitives of 4 x 4 x 2, B = 2, five primitives dropped) under
    patch_hand_mvp(fused_tail=True) against patch_hand_mvp(): the template to 1e-5, the images and the gradients of every
    decoder parameter to the project's 1e-4."""
    from goliath_amd import dropin, mvptail

    M = _module()
    ae = AutoEncoder().cuda()
    inputs, weights = _model_inputs()
    own_rgb_forward = RGBSlabDecoder.forward
    try:
        dropin.patch_hand_mvp(M)
        p0, t0, calls0, g0 = _step(ae, inputs, weights, monkeypatch)
        assert "gol_mvp_template_fwd" in calls0 and "gol_mvp_tail_fwd" not in calls0
        a0 = p0["alpha"].detach()
        assert float(a0.max()) > 0.2 and float((a0 > 0).float().mean()) > 0.1     # the primitives are in view
        zr, za = float((p0["primrgb"] == 0).float().mean()), float((p0["primalpha"] == 0).float().mean())
        assert 0.1 < zr < 0.9 and 0.1 < za < 0.9, (zr, za)

        dropin.patch_hand_mvp(M, fused_tail=True)
        p1, t1, calls1, g1 = _step(ae, inputs, weights, monkeypatch)
        assert "gol_mvp_tail_fwd" in calls1 and "gol_mvp_tail_bwd" in calls1 and "gol_mvp_template_fwd" not in calls1
        assert "primrgba" not in p1
        assert isinstance(p1["primrgb"], mvptail.TailHandle) and isinstance(p1["primalpha"], mvptail.TailHandle)
        errs = {"template": scenes.rel_l2(t1, t0), "rgb": scenes.rel_l2(p1["rgb"], p0["rgb"]),
                "alpha": scenes.rel_l2(p1["alpha"], p0["alpha"])}
        print({k: f"{v:.2e}" for k, v in errs.items()})
        assert t1.shape == t0.shape and errs["template"] <= 1e-5
        assert errs["rgb"] <= 1e-4 and errs["alpha"] <= 1e-4
        assert set(g1) == set(g0)
        gerr = {n: scenes.rel_l2(g1[n], g0[n]) for n in g0}
        print({k: f"{v:.2e}" for k, v in gerr.items()})
        for n in g0:
            assert float(g0[n].abs().max()) > 0 and gerr[n] <= 1e-4, (n, gerr[n])
        for k in ("primrgb", "primalpha"):
            assert scenes.rel_l2(p1[k].materialize(), p0[k]) <= 1e-6, k

        # full_template=True (HandMVPSummary) keeps today's path
        dropin.patch_hand_mvp(M, full_template=True, fused_tail=True)
        p2, t2, calls2, _ = _step(ae, inputs, weights, monkeypatch)
        assert "gol_mvp_template_fwd" in calls2 and "gol_mvp_tail_fwd" not in calls2
        assert "primrgba" in p2 and torch.equal(t2, t0)

        # a later patch_hand_mvp() restores the default
        dropin.patch_hand_mvp(M)
        assert RGBSlabDecoder.forward is own_rgb_forward
        p3, t3, calls3, _ = _step(ae, inputs, weights, monkeypatch)
        assert "gol_mvp_tail_fwd" not in calls3 and torch.is_tensor(p3["primrgb"]) and torch.equal(t3, t0)
        assert torch.equal(p3["rgb"], p0["rgb"])

        # a decoder whose last layer is a plain ConvTranspose2d falls back: the parent's numbers bitwise
        plain = AutoEncoder(plain_last=True).cuda()
        q0, u0, _, _ = _step(plain, inputs, weights, monkeypatch)
        dropin.patch_hand_mvp(M, fused_tail=True)
        q1, u1, callsq, _ = _step(plain, inputs, weights, monkeypatch)
        assert "gol_mvp_tail_fwd" not in callsq and "gol_mvp_template_fwd" in callsq
        assert torch.equal(u1, u0) and torch.equal(q1["rgb"], q0["rgb"]) and torch.equal(q1["alpha"], q0["alpha"])
    finally:
        dropin.patch_hand_mvp(M)
        RGBSlabDecoder.forward = own_rgb_forward
