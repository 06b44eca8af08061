"""GPU: goliath_amd.uvtex (csrc/uvtex.hip) against the reference's own code in float64.

tests/golden/uvtex_golden.partNN.npz (tests/golden/make_uvtex_golden.py) holds, per case of tests/uvtex_cases.py, the
inputs, AutoEncoder.forward_tex + a real CalV5 (train() mode) + SeamSampler.resample run in float64, the gradients of a
seeded linear loss, and the reference's own float32-vs-float64 error.  Bars:
  * per-texel tensors (texrec_before_warp, tex_rgba, the gradient of tex, pack_rgba, normal_rgba): 3e-5 relative L2, the
    project's bar for float32 model outputs against float64 (tests/test_gpu_urhand_model.py);
  * the cal-parameter gradients (sums over 3 S^2 terms): 4 x the reference's own float32-vs-float64 error stored in the
    golden (the margin the uvframes tests give a different summation order), floored at 3e-5.
Nothing is excluded: the generator guarantees that no pre-clamp value is within 1e-3 of 0 or 255.
Measured on an MI355X (maxima over the cases; each test prints its figures before asserting): see DESIGN.md section 8
"uvtex"."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import npz_parts  # noqa: E402
import uvtex_cases as cases  # noqa: E402
import uvtex_standin as standin  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 3e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uvtex_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return npz_parts.load(GOLDEN)


def _dev(golden, name, key):
    return torch.from_numpy(np.asarray(golden[f"{name}/{key}"])).cuda()


def _fused(golden, name, seams=True, before_grad=True):
    """texture_tail on a case's inputs with the golden's loss: outputs and gradients (cal gradient as [cameras, 6])."""
    from goliath_amd import imgtail, uvtex

    c = cases.CASES[name]
    tex = _dev(golden, name, "tex").requires_grad_(True)
    cal = M = b = None
    if c["cams"] is not None:
        cal = cases.StandInCal(torch.from_numpy(np.asarray(golden[f"{name}/cal_params"]))).cuda()
        M, b = imgtail.cal_v5_matrix(cal, cal.name_to_idx(c["cams"]))
    pack = uvtex.pack_seams(_dev(golden, name, "uvs"), _dev(golden, name, "weights")) if seams else None
    before, rgba = uvtex.texture_tail(tex, _dev(golden, name, "tex_mean"), cases.TEX_STD, pack, M, b)
    loss = (rgba[:, :3] * _dev(golden, name, "w_rec")).sum()
    if before_grad:
        loss = loss + (before * _dev(golden, name, "w_before")).sum()
    loss.backward()
    return before.detach(), rgba.detach(), tex.grad, None if cal is None else cal.params.grad


@pytest.mark.parametrize("name", list(cases.CASES))
def test_texture_tail_matches_the_reference_in_float64(golden, name):
    before, rgba, g_tex, g_cal = _fused(golden, name)
    ref = lambda k: np.asarray(golden[f"{name}/ref64/{k}"])
    errs = dict(before=cases.rel_l2(before.cpu().numpy(), ref("before")),
                tex_rec=cases.rel_l2(rgba[:, :3].cpu().numpy(), ref("tex_rec")),
                g_tex=cases.rel_l2(g_tex.cpu().numpy(), ref("g_tex")))
    bars = dict(before=BAR, tex_rec=BAR, g_tex=BAR)
    if g_cal is not None:
        errs["g_cal"] = cases.rel_l2(g_cal.cpu().numpy(), ref("g_cal"))
        bars["g_cal"] = max(4.0 * float(golden[f"{name}/err32/g_cal"]), BAR)
    print(f"uvtex parity {name}:", {k: f"{v:.3e} (bar {bars[k]:.1e})" for k, v in errs.items()})
    assert bool((rgba[:, 3] == 1).all())                                   # alpha exactly 1
    assert float(np.abs(ref("g_tex")).max()) > 0
    for k, v in errs.items():
        assert v <= bars[k], (name, k, v, bars[k])


def test_no_seams_means_out_equals_pre_bit_for_bit(golden):
    name = "s40_b3_c6"
    before, rgba, g_tex, _ = _fused(golden, name, seams=False)
    assert torch.equal(rgba[:, :3], before)
    assert bool((rgba[:, 3] == 1).all())
    assert cases.rel_l2(before.cpu().numpy(), np.asarray(golden[f"{name}/ref64/before"])) <= BAR
    assert bool(torch.isfinite(g_tex).all()) and float(g_tex.abs().max()) > 0


@pytest.mark.parametrize("name", ["s72_b1_c4", "s40_b3_c2"])
def test_two_backward_runs_are_bit_identical(golden, name):
    a = _fused(golden, name)
    b = _fused(golden, name)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _float64_lines(tex, tex_mean, M, b, uvs, weights, w_rec):
    """The reference's lines (urhand.py:721-747 with the cal as a matrix, seams.py:21-25) in float64 on the CPU."""
    tex = tex.double().cpu().requires_grad_(True)
    C = tex.shape[1]
    ng = 1 if C == 2 else 3
    raw = tex_mean.double().cpu() * tex[:, :ng] + tex[:, ng:] * cases.TEX_STD
    x = torch.einsum("bcj,bjhw->bchw", M.double().cpu(), raw.expand(-1, 3, -1, -1)) + b.double().cpu()[:, :, None, None]
    pre = x.clamp(0, 255)
    grid = 2.0 * (uvs.double().cpu()[None].expand(tex.shape[0], -1, -1, -1) - 0.5)
    w = weights.double().cpu()
    out = (1.0 - w) * pre + w * F.grid_sample(pre, grid, align_corners=False, padding_mode="border")
    (out * w_rec.double().cpu()).sum().backward()
    return pre.detach(), out.detach(), tex.grad, x.detach()


def test_scalar_path_at_an_odd_size():
    """S = 37: S*S is odd, so the kernels take their 4-byte path and the last lane of the last workgroup holds one texel.
    Reference: the same lines in float64 (restated above), bars as for the golden cases."""
    from goliath_amd import uvtex

    S, B, C = 37, 2, 4
    g = torch.Generator().manual_seed(37)
    uvs, weights, _ = cases.make_seams(S, 37)
    while True:
        tex = torch.randn(B, C, S, S, generator=g)
        tex[:, :3] = 1.2 + 0.7 * tex[:, :3]
        tex_mean = 255.0 * torch.rand(1, 3, S, S, generator=g)
        M = torch.eye(3)[None] + 0.2 * torch.randn(B, 3, 3, generator=g)
        b = 8.0 * torch.randn(B, 3, generator=g)
        w_rec = torch.randn(B, 3, S, S, generator=g)
        pre, out, g_tex, x = _float64_lines(tex, tex_mean, M, b, uvs, weights, w_rec)
        if min(float(x.abs().min()), float((x - 255).abs().min())) >= 1e-3:   # no clamp tie
            break
    t = tex.cuda().requires_grad_(True)
    before, rgba = uvtex.texture_tail(t, tex_mean.cuda(), cases.TEX_STD, uvtex.pack_seams(uvs.cuda(), weights.cuda()),
                                      M.cuda(), b.cuda())
    (rgba[:, :3] * w_rec.cuda()).sum().backward()
    errs = (cases.rel_l2(before.detach().cpu().numpy(), pre.numpy()), cases.rel_l2(rgba[:, :3].detach().cpu().numpy(), out.numpy()),
            cases.rel_l2(t.grad.cpu().numpy(), g_tex.numpy()))
    print("uvtex parity S=37 (before, tex_rec, g_tex):", ["%.3e" % e for e in errs])
    assert bool((rgba[:, 3] == 1).all()) and max(errs) <= BAR


@pytest.mark.parametrize("S,B", [(40, 3), (37, 1)])
def test_pack_rgba_and_normal_rgba(S, B):
    """urhand.py:788-790 + :826 and :828-832 restated in float64."""
    from goliath_amd import uvtex

    g = torch.Generator().manual_seed(S)
    while True:
        x = 0.5 + 0.4 * torch.randn(B, 3, S, S, generator=g)
        if min(float((255.0 * x.double()).abs().min()), float((255.0 * x.double() - 255).abs().min())) >= 1e-3:
            break
    w = torch.randn(B, 4, S, S, generator=g)
    xd = x.double().requires_grad_(True)
    want = torch.cat([(xd * 255.0).clamp(min=0, max=255), torch.ones(B, 1, S, S, dtype=torch.float64)], dim=1)
    (want * w.double()).sum().backward()
    xg = x.cuda().requires_grad_(True)
    got = uvtex.pack_rgba(xg, 255.0, 0.0, 255.0)
    (got * w.cuda()).sum().backward()
    e_f, e_b = cases.rel_l2(got.detach().cpu().numpy(), want.detach().numpy()), cases.rel_l2(xg.grad.cpu().numpy(), xd.grad.numpy())
    share = (float((xd * 255 < 0).double().mean()), float((xd * 255 > 255).double().mean()))
    print(f"pack_rgba S={S}: fwd {e_f:.3e} bwd {e_b:.3e}; clamped below / above {share}")
    assert min(share) > 0.02 and bool((got[:, 3] == 1).all()) and e_f <= BAR and e_b <= BAR
    nml = F.normalize(torch.randn(B, 3, S, S, generator=g), dim=1)
    for rows in (3, 4):
        Rt = torch.randn(B, rows, 4, generator=g)
        n = torch.bmm(nml.double().permute(0, 2, 3, 1).reshape(B, -1, 3), Rt.double()[:, :3, :3].permute(0, 2, 1))
        n = (1 - n.reshape(B, S, S, 3).permute(0, 3, 1, 2)) * 127.5
        want_n = torch.cat([n, torch.ones_like(n[:, :1])], dim=1)
        got_n = uvtex.normal_rgba(nml.cuda(), Rt.cuda())
        e_n = cases.rel_l2(got_n.cpu().numpy(), want_n.numpy())
        print(f"normal_rgba S={S} Rt[{rows},4]: {e_n:.3e}")
        assert bool((got_n[:, 3] == 1).all()) and not got_n.requires_grad and e_n <= BAR


def _model_run(model, batch, flag):
    from goliath_amd import urhand, uvtex

    setattr(model, uvtex.TEXTURE_TAIL_FLAG, flag)
    model.zero_grad()
    preds = urhand.autoencoder_forward(model, **batch)
    g = torch.Generator().manual_seed(11)
    loss = 0
    for k in ("rendered_rgb", "rendered_phys_rgb", "texrec_before_warp", "tex_rec"):
        loss = loss + (preds[k] * torch.randn(preds[k].shape, generator=g).cuda()).sum()
    loss.backward()
    grads = dict(tex=model.decoder_relight.tex.grad.clone(), phys_tex=model.decoder_relight.phys_tex.grad.clone())
    if hasattr(model, "cal"):
        grads["cal"] = model.cal.params.grad.clone()
    return preds, grads


@pytest.mark.parametrize("C,cal,impaint", [(4, True, True), (6, True, False), (2, False, True)])
def test_drop_in_flag_on_against_flag_off(C, cal, impaint):
    """autoencoder_forward on a stand-in AutoEncoder (tests/uvtex_standin.py; S = 64, B = 2; a colour and a grey camera; cal
    in train() mode): every preds key and the gradients w.r.t. the decoder's tex, phys_tex and the cal parameters, fused
    path against the reference's lines as torch operators on the same GPU, at the same bars (both sides are float32
    evaluations of one formula; they differ by less than either differs from float64)."""
    from goliath_amd import uvtex

    S, B = 64, 2
    model = standin.StandInAutoEncoder(S=S, B=B, C=C, seed=C, cal=cal, impaint_uv=impaint).cuda().train()
    batch = standin.StandInAutoEncoder.batch(B, seed=C, device="cuda", cams=("400002", "410011"))
    want, g_want = _model_run(model, batch, False)
    got, g_got = _model_run(model, batch, True)
    assert list(got) == list(want)
    assert got["tex_rec"]._base is not None and got["tex_rec"].shape == (B, 3, S, S)   # a view of the RGBA texture
    worst = {}
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        if want[k].dtype == torch.bool:
            assert torch.equal(got[k], want[k]), k
        else:
            worst[k] = cases.rel_l2(got[k].detach().cpu().numpy(), want[k].detach().cpu().numpy())
    for k in g_want:
        assert float(g_want[k].abs().max()) > 0, k
        worst["grad " + k] = cases.rel_l2(g_got[k].cpu().numpy(), g_want[k].cpu().numpy())
    print(f"uvtex drop-in C={C} cal={cal} impaint={impaint}:", {k: f"{v:.2e}" for k, v in worst.items() if v > 0})
    for k, v in worst.items():
        assert v <= BAR, (k, v)
    assert bool((got["old_normals_uv"][:, 3] == 1).all()) and bool((got["normals_uv"][:, 3] == 1).all())
    setattr(model, uvtex.TEXTURE_TAIL_FLAG, False)
