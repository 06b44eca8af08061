"""goliath_amd.uvtex on the host (no GPU): the seam pack, the argument checks, the drop-in keyword and -- in the build
container -- `autoencoder_forward` without the flag against the reference's own AutoEncoder.forward.

  * pack_seams: the CSR tap list applied to a random vector equals, in float64, autograd of `w * grid_sample(., uv)` (the
    dense transpose of the bilinear operator), on the synthetic seams of tests/uvtex_cases.py (border, texel centres,
    last row / column, a row of ~200 entries);
  * texture_tail / pack_rgba / normal_rgba refuse CPU tensors, C outside {2, 4, 6} and non-square textures;
  * dropin.patch_urhand(texture_tail=True) rebinds AutoEncoder.forward to a callable with the same parameter list and sets
    the flag; the default leaves the original function object bound (and restores it after an earlier True);
  * autoencoder_forward (flag off) == AutoEncoder.forward of /root/reference run as an unbound method on the same stand-in
    (S = 1024: the reference hard-codes it; B = 1): every `preds` key and the gradients to 1e-6 relative L2."""
import inspect
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import uvtex_cases as cases  # noqa: E402
import uvtex_standin as standin  # noqa: E402

REF = "/root/reference"


def _csr_apply(pack, g):
    """out[t] = sum_{e in row(t)} coeff[e] g[src[e]] in float64, for g[S*S]."""
    rs, src, coeff = pack.row_start.long(), pack.src.long(), pack.coeff.double()
    rows = torch.repeat_interleave(torch.arange(rs.numel() - 1), rs[1:] - rs[:-1])
    return torch.zeros(rs.numel() - 1, dtype=torch.float64).index_add_(0, rows, coeff * g[src])


@pytest.mark.parametrize("S,wshape", [(40, (40, 40)), (72, (1, 72, 72)), (37, (1, 1, 37, 37))])
def test_pack_seams_is_the_transpose_of_the_bilinear_operator(S, wshape):
    from goliath_amd import uvtex

    uvs, weights, info = cases.make_seams(S, 3, wshape)
    pack = uvtex.pack_seams(uvs, weights)
    assert pack.uvs.shape == (S, S, 2) and pack.weights.shape == (S, S) and pack.size == S
    assert pack.row_start.dtype == torch.int32 and pack.src.dtype == torch.int32 and pack.coeff.dtype == torch.float32
    rs = pack.row_start.long()
    assert rs[0] == 0 and rs[-1] == pack.src.numel() == pack.coeff.numel() and bool((rs[1:] >= rs[:-1]).all())
    assert int((rs[1:] - rs[:-1])[info["dest"]]) >= info["n_long"]          # the long row: ~200 entries on one texel
    assert bool((weights.reshape(S, S)[info["r2"]] == 1).all())
    assert bool((pack.weights.reshape(-1)[pack.src.long()] != 0).all())     # only band texels are sources
    gen = torch.Generator().manual_seed(S)
    g = torch.randn(S * S, generator=gen, dtype=torch.float64)
    x = torch.randn(1, 1, S, S, generator=gen, dtype=torch.float64, requires_grad=True)
    grid = 2.0 * (uvs.double()[None] - 0.5)
    y = weights.double().reshape(1, 1, S, S) * F.grid_sample(x, grid, align_corners=False, padding_mode="border")
    (want,) = torch.autograd.grad((y.reshape(-1) * g).sum(), x)
    got = _csr_apply(pack, g)
    # the coefficients are float32 products of float32 fractions: 1e-6 relative per entry, far below this bar
    assert cases.rel_l2(got.numpy(), want.reshape(-1).numpy()) < 1e-5
    again = uvtex.pack_seams(uvs, weights)
    assert torch.equal(again.src, pack.src) and torch.equal(again.coeff, pack.coeff)


def test_seams_of_caches_on_the_sampler():
    from goliath_amd import uvtex

    sampler = standin._Seams(40, 1)
    p = uvtex.seams_of(sampler)
    assert uvtex.seams_of(sampler) is p
    sampler.weights.mul_(0.5)                       # a changed buffer rebuilds the pack
    q = uvtex.seams_of(sampler)
    assert q is not p and torch.allclose(q.coeff, 0.5 * p.coeff)


def test_argument_checks():
    """Shapes are checked first (ValueError), then the device (GoliathHipError: there is no CPU path), like imgtail."""
    from goliath_amd import uvtex
    from goliath_amd._lib import GoliathHipError

    S = 8
    tex, mean = torch.rand(1, 4, S, S), torch.rand(1, 3, S, S)
    for fn in (lambda: uvtex.texture_tail(tex, mean, 64.0, None),
               lambda: uvtex.texture_tail(tex, mean, 64.0, uvtex.pack_seams(torch.rand(S, S, 2), torch.rand(S, S))),
               lambda: uvtex.pack_rgba(torch.rand(1, 3, S, S), 255.0, 0.0, 255.0),
               lambda: uvtex.normal_rgba(torch.rand(1, 3, S, S), torch.rand(1, 3, 4))):
        with pytest.raises(GoliathHipError):
            fn()
    for fn in ([lambda C=C: uvtex.texture_tail(torch.rand(1, C, S, S), mean, 64.0, None) for C in (1, 3, 5, 8)] + [   # C
               lambda: uvtex.texture_tail(torch.rand(1, 4, S, S + 1), torch.rand(1, 3, S, S + 1), 64.0, None),    # non-square
               lambda: uvtex.texture_tail(tex, torch.rand(1, 3, S + 1, S + 1), 64.0, None),
               lambda: uvtex.texture_tail(tex, torch.rand(2, 3, S, S), 64.0, None),
               lambda: uvtex.pack_rgba(torch.rand(1, 3, S, S + 1)),
               lambda: uvtex.pack_rgba(torch.rand(1, 4, S, S)),
               lambda: uvtex.normal_rgba(torch.rand(1, 3, S, S), torch.rand(1, 3, 3)),
               lambda: uvtex.normal_rgba(torch.rand(1, 3, S + 1, S), torch.rand(1, 3, 4)),
               lambda: uvtex.pack_seams(torch.rand(S, S + 1, 2), torch.rand(S, S + 1)),
               lambda: uvtex.pack_seams(torch.rand(S, S, 2), torch.rand(S - 1, S - 1))]):
        with pytest.raises(ValueError):
            fn()


def _params(fn):
    return [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]


def _stand_in_module():
    """A module shaped like ca_code.models.urhand where patch_urhand looks: ConvTeacherDecoder, AutoEncoder, the names."""
    m = types.ModuleType("urhand_stand_in")

    class ConvTeacherDecoder:
        def forward(self, lbs_motion, id_mesh, tex_mean, verts_rec, cam_pos, light_pos, light_intensity, seam_sampler=None,
                    ccm=None, falloff_dist=None, nearfield=False, iteration=None):
            raise NotImplementedError

    class AutoEncoder:
        def forward(self, pose, campos, K, Rt, light_pos=None, light_intensity=None, camera_id=None, frame_id=None,
                    iteration=None, **kwargs):
            raise NotImplementedError

    m.ConvTeacherDecoder, m.AutoEncoder, m.RenderLayer, m.get_shadow_map = ConvTeacherDecoder, AutoEncoder, object, None
    return m


def test_patch_urhand_texture_tail_keyword():
    from goliath_amd import dropin, urhand, uvtex

    m = _stand_in_module()
    original = m.AutoEncoder.__dict__["forward"]
    assert dropin.patch_urhand(m) is m
    assert m.AutoEncoder.__dict__["forward"] is original                   # the default leaves the function object bound
    assert not getattr(m.AutoEncoder, uvtex.TEXTURE_TAIL_FLAG, False)
    assert dropin.patch_urhand(m, texture_tail=True) is m
    assert m.AutoEncoder.forward is urhand.autoencoder_forward
    assert getattr(m.AutoEncoder, uvtex.TEXTURE_TAIL_FLAG) is True
    assert _params(m.AutoEncoder.forward) == _params(original)             # what filter_inputs introspects
    dropin.patch_urhand(m, texture_tail=True)                               # twice: the original is still remembered
    dropin.patch_urhand(m)                                                  # and back
    assert m.AutoEncoder.__dict__["forward"] is original
    assert getattr(m.AutoEncoder, uvtex.TEXTURE_TAIL_FLAG) is False


@pytest.fixture(scope="module")
def ref_urhand():
    if not os.path.isdir(REF):
        pytest.skip("reference tree only exists in the build container")
    import ref_stubs

    ref_stubs.install()
    sys.modules.setdefault("sgutilslib", types.ModuleType("sgutilslib"))
    import ca_code.models.urhand as U

    return U


def test_patch_urhand_keeps_the_reference_signature(ref_urhand):
    from goliath_amd import dropin, urhand

    U = ref_urhand
    saved = (U.ConvTeacherDecoder.forward, U.AutoEncoder.__dict__["forward"], U.get_shadow_map)
    try:
        dropin.patch_urhand(U)
        assert U.AutoEncoder.__dict__["forward"] is saved[1]
        dropin.patch_urhand(U, texture_tail=True)
        assert U.AutoEncoder.forward is urhand.autoencoder_forward
        assert _params(U.AutoEncoder.forward) == _params(saved[1])
        dropin.patch_urhand(U)
        assert U.AutoEncoder.__dict__["forward"] is saved[1]
    finally:
        U.ConvTeacherDecoder.forward, U.AutoEncoder.forward, U.get_shadow_map = saved


def _run(model, forward, batch):
    model.zero_grad()
    preds = forward(model, **batch)
    g = torch.Generator().manual_seed(11)
    loss = 0
    for k in ("rendered_rgb", "rendered_phys_rgb", "texrec_before_warp", "tex_rec"):
        loss = loss + (preds[k] * torch.randn(preds[k].shape, generator=g)).sum()
    loss.backward()
    grads = dict(tex=model.decoder_relight.tex.grad.clone(), phys_tex=model.decoder_relight.phys_tex.grad.clone(),
                 cal=model.cal.holder.params.grad.clone())
    return preds, grads


def test_flag_off_forward_is_the_reference_forward(ref_urhand, monkeypatch):
    """Same arithmetic, same order: 1e-6 relative L2 on every preds key and on the gradients w.r.t. the decoder's tex,
    phys_tex and the cal parameters (a real CalV5 in train() mode, a real SeamSampler)."""
    from ca_code.nn.color_cal import CalV5
    from ca_code.utils.seams import SeamSampler

    from goliath_amd import urhand

    U = ref_urhand
    S, B = 1024, 1
    uvs, weights, _ = cases.make_seams(S, 5, (1, 1, S, S))
    sampler = SeamSampler(dict(dst_ij=torch.zeros(1, 2, dtype=torch.long), src_ij=torch.zeros(1, 2, dtype=torch.long),
                               uvs=uvs, weights=weights))
    model = standin.StandInAutoEncoder(S=S, B=B, C=6, seed=4, cal=False, seam_sampler=sampler)
    model.cal = CalV5(cameras=cases.CAMERAS, identity_camera=cases.IDENTITY)
    with torch.no_grad():
        model.cal.holder.params.copy_(cases.make_inputs("s40_b3_c2", 9)["cal_params"])
    model.train()
    model.forward_tex = types.MethodType(U.AutoEncoder.forward_tex, model)
    for name in ("euler_angles_to_matrix", "matrix_to_axis_angle", "depth_discontuity_mask"):
        monkeypatch.setattr(U, name, getattr(standin, name))
    batch = standin.StandInAutoEncoder.batch(B, seed=4, cams=("410011",))
    want, g_want = _run(model, U.AutoEncoder.forward, batch)
    got, g_got = _run(model, urhand.autoencoder_forward, batch)
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        if want[k].dtype == torch.bool:
            assert torch.equal(got[k], want[k]), k
        else:
            assert cases.rel_l2(got[k].detach().numpy(), want[k].detach().numpy()) <= 1e-6, k
    for k in g_want:
        assert float(g_want[k].abs().max()) > 0, k
        assert cases.rel_l2(g_got[k].numpy(), g_want[k].numpy()) <= 1e-6, k
