"""GPU parity: URHand UV light-loop kernels (C ABI gol_uvlight_*) vs golden vectors produced by the
reference's own source lines (tests/golden/urhand_golden.npz) and vs the torch oracle at 256x256 with
32 lights (the OLAT sweep of BASELINE config 4).  Tolerance rel-L2 <= 1e-4."""
import pytest
import torch
import torch.nn.functional as F

from scenes import rel_l2
from test_oracle_urhand import load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.mark.parametrize("tag", ["sh", "nosh"])
def test_uvlight_matches_reference_golden(tag):
    from goliath_amd import uvlight

    G = load_golden()
    c = lambda k: G[f"in/{k}"].cuda()
    leaf = {k: c(k).requires_grad_(True) for k in ("p_uv", "nml", "roughness", "tex_mean")}
    sh = c("shadow_map") if tag == "sh" else None
    d, s = uvlight.phong_features(leaf["p_uv"], leaf["nml"], c("cam_pos"), c("light_pos"), c("light_intensity"), sh)
    assert rel_l2(d, G[f"{tag}/phong/diff"]) < TOL and rel_l2(s, G[f"{tag}/phong/spec"]) < TOL
    ((d * G[f"{tag}/phong/w_diff"].cuda()).sum() + (s * G[f"{tag}/phong/w_spec"].cuda()).sum()).backward()
    assert rel_l2(leaf["p_uv"].grad, G[f"{tag}/phong/g_p_uv"]) < TOL
    assert rel_l2(leaf["nml"].grad, G[f"{tag}/phong/g_nml"]) < TOL
    for t in leaf.values():
        t.grad = None
    f, rgb = uvlight.ggx_features(leaf["p_uv"], leaf["nml"], c("cam_pos"), c("light_pos"), c("light_intensity"),
                                  leaf["roughness"], leaf["tex_mean"], sh)
    assert rel_l2(f, G[f"{tag}/ggx/feat"].reshape(f.shape)) < TOL and rel_l2(rgb, G[f"{tag}/ggx/rgb"]) < TOL
    ((f * G[f"{tag}/ggx/w_feat"].reshape(f.shape).cuda()).sum() + (rgb * G[f"{tag}/ggx/w_rgb"].cuda()).sum()).backward()
    for k, n in (("p_uv", "g_p_uv"), ("nml", "g_nml"), ("roughness", "g_roughness"), ("tex_mean", "g_tex")):
        assert rel_l2(leaf[k].grad, G[f"{tag}/ggx/{n}"]) < TOL, (k, rel_l2(leaf[k].grad, G[f"{tag}/ggx/{n}"]))


def test_uvlight_olat_32_lights_vs_oracle():
    from goliath_amd import uvlight
    from oracle import urhand_ref

    g = torch.Generator().manual_seed(9)
    B, L, S = 1, 32, 256
    p_uv = 40 * torch.randn(B, 3, S, S, generator=g)
    nml = F.normalize(torch.randn(B, 3, S, S, generator=g), dim=1)
    cam = torch.tensor([[20.0, 10.0, -800.0]])
    lp = F.normalize(torch.randn(B, L, 3, generator=g), dim=-1) * 1100
    li = torch.zeros(B, L, 1)
    li[:, 7] = 1.0  # one-light-at-a-time frame
    li = li + 0.05
    rough = 0.3 + 0.6 * torch.rand(B, 1, S, S, generator=g)  # below ~0.3 the GGX lobe is ill-conditioned in fp32
    tex = 255 * torch.rand(B, 3, S, S, generator=g)
    shm = torch.rand(B, L, 1, S, S, generator=g)
    cpu = [t.clone().requires_grad_(True) for t in (p_uv, nml, rough, tex)]
    gpu = [t.clone().cuda().requires_grad_(True) for t in (p_uv, nml, rough, tex)]
    rf, rr = urhand_ref.ggx_features(cpu[0], cpu[1], cam, lp, li, cpu[2], cpu[3], shm)
    of, orr = uvlight.ggx_features(gpu[0], gpu[1], cam.cuda(), lp.cuda(), li.cuda(), gpu[2], gpu[3], shm.cuda())
    assert rel_l2(of, rf) < TOL and rel_l2(orr, rr) < TOL
    wf, wr = torch.randn(rf.shape, generator=g), torch.randn(rr.shape, generator=g)
    ((rf * wf).sum() + (rr * wr).sum()).backward()
    ((of * wf.cuda()).sum() + (orr * wr.cuda()).sum()).backward()
    # fp64 evaluation of the same reference expression with the same upstream gradient
    c64 = [t.clone().double().requires_grad_(True) for t in (p_uv, nml, rough, tex)]
    rf64, rr64 = urhand_ref.ggx_features(c64[0], c64[1], cam.double(), lp.double(), li.double(), c64[2], c64[3], shm.double())
    ((rf64 * wf.double()).sum() + (rr64 * wr.double()).sum()).backward()
    for a, b, c, n in zip(gpu, cpu, c64, ("p_uv", "nml", "roughness", "tex")):
        # torch yields NaN (0 * inf) where spec^31 overflows behind the clamp(max=1) -- a quirk of the
        # reference expression that the kernel does not reproduce (it returns the gated 0); compare elsewhere
        ok = torch.isfinite(b.grad) & torch.isfinite(c.grad.float())
        assert float(ok.float().mean()) > 0.99 and bool(torch.isfinite(a.grad).all())
        # 32 lights x pow(., 32): the fp32 torch evaluation is itself ill-conditioned here.  Yardstick = the SAME reference
        # code in fp64 (c): HIP must be within 1e-4 of it, or at least as close to it as the fp32 reference is (measured,
        # profiles/r04_parity_ledger.json: HIP vs fp32 reference 2.3e-4 on the worst tensor -- and the fp32 reference is that
        # far from its own fp64 evaluation)
        e_hip64 = rel_l2(a.grad.cpu().double()[ok], c.grad[ok])
        e_ref64 = rel_l2(b.grad.double()[ok], c.grad[ok])
        print(f"\nOLAT_GRAD {n}: hip vs fp64 {e_hip64:.2e}, fp32 reference vs fp64 {e_ref64:.2e}, "
              f"hip vs fp32 reference {rel_l2(a.grad.cpu()[ok], b.grad[ok]):.2e}")
        assert e_hip64 < max(TOL, 1.5 * e_ref64), (n, e_hip64, e_ref64)
    # Phong path, no shadow map
    rd, rs = urhand_ref.phong_features(p_uv, nml, cam, lp, li, None)
    od, os_ = uvlight.phong_features(p_uv.cuda(), nml.cuda(), cam.cuda(), lp.cuda(), li.cuda(), None)
    assert rel_l2(od, rd) < TOL and rel_l2(os_, rs) < TOL


# ---- edge shapes against the float64 oracle (inputs: tests/urhand_cases.py, guarded on the CPU by tests/test_urhand_cases.py)
def _hip(tag):
    import urhand_cases as uc
    from goliath_amd import uvlight

    return uc.run_uv(uvlight, uc.uv_inputs(tag), lambda v: v.cuda())


@pytest.mark.parametrize("tag", ["tail_unit", "tail_nosh", "nonunit", "highlight", "p0", "p1", "lowrough", "dark"])
def test_uvlight_edge_shapes_vs_float64_oracle(tag):
    """Multi-block launches with a partial tail at B > 1, P = 0 / 1 / 3 / 4 powers, non-unit normals (the upper halves of
    clamp(n.L, 0, 1) and of min(s^p, 1)), a GGX lobe above 1, low roughness, zero total intensity: every output and every
    input gradient of both kernels over ALL elements against the float64 oracle, bar max(1e-4, 1.5 e_ref64) per tensor
    (e_ref64: what the float32 oracle itself is away from float64, tests/urhand_cases.py; measured there: at most 7.5e-5,
    on ggx g_roughness of `nonunit`, so the bar is 1e-4 .. 1.13e-4).  Measured, HIP vs float64 (UV_EDGE lines), worst tensor
    of each case: tail_unit 2.2e-5 (ggx g_nml), tail_nosh 5.8e-6, nonunit 7.1e-5 (ggx g_roughness; float32 oracle 7.5e-5),
    highlight 6.2e-5 (ggx g_p_uv; float32 oracle 6.8e-5), p0 2.7e-6, p1 4.5e-6, lowrough 2.4e-5 (ggx g_roughness; float32 oracle
    1.4e-5); every Phong tensor <= 6e-6."""
    import urhand_cases as uc

    got, ref, e64 = _hip(tag), uc.uv_oracle(tag, torch.float64), uc.e_ref64(tag)
    c = uc.UV[tag]
    B, H, W, P = c["B"], c["H"], c["W"], len(c["powers"])
    assert got["phong/spec"].shape == (B, P, 1, H, W) and got["ggx/feat"].shape == (B, 1 + P, H, W)
    fails = []
    for k in uc.PHONG_KEYS + uc.GGX_KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, (tag, k)
        assert bool(torch.isfinite(got[k]).all()), (tag, k)
        if c.get("dark"):
            assert not got[k].any() and not ref[k].any(), (tag, k)                # exactly 0, outputs and gradients
            continue
        e_hip, bar = rel_l2(got[k], ref[k]), max(TOL, 1.5 * e64[k][0])
        print(f"\nUV_EDGE {tag} {k}: hip vs fp64 {e_hip:.2e}, fp32 reference vs fp64 {e64[k][0]:.2e}, bar {bar:.2e}")
        if not e_hip < bar:
            fails.append((k, e_hip, bar))
    assert not fails, (tag, fails)


def _args(tag, L=None):
    import urhand_cases as uc

    t = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in uc.uv_inputs(tag).items()}
    if L is not None:
        t["light_pos"], t["light_intensity"] = t["light_pos"][:, :L], t["light_intensity"][:, :L]
        t["shadow_map"] = t["shadow_map"][:, :L]
    return t


def test_uvlight_no_lights():
    """L == 0: Phong is an empty sum (zeros, zero gradients); GGX is a mean over lights and refuses, by an argument check
    that returns before any launch."""
    from goliath_amd import _lib, uvlight

    t = _args("p1", L=0)
    assert t["light_pos"].shape == (2, 0, 3) and t["shadow_map"].shape == (2, 0, 1, 9, 29)
    p, n = t["p_uv"].clone().requires_grad_(True), t["nml"].clone().requires_grad_(True)
    for sh in (t["shadow_map"], None):
        d, s = uvlight.phong_features(p, n, t["cam_pos"], t["light_pos"], t["light_intensity"], sh, spec_powers=(1, 16))
        assert d.shape == (2, 1, 9, 29) and s.shape == (2, 2, 1, 9, 29) and not d.any() and not s.any()
        gp, gn = torch.autograd.grad(d.sum() + (s * 3.0).sum(), (p, n))
        assert gp.shape == p.shape and not gp.any() and not gn.any()
    with pytest.raises(_lib.GoliathHipError, match="L must be > 0"):
        uvlight.ggx_features(p, n, t["cam_pos"], t["light_pos"], t["light_intensity"], t["roughness"], t["tex_mean"], None)
    torch.cuda.synchronize()


def test_uvlight_wrapper_forms():
    """[B,L] and [B,L,1] intensities, a stride-0 expanded camera row, and a backward with one leaf only."""
    import urhand_cases as uc
    from goliath_amd import uvlight

    t = _args("tail_unit")
    base = uc.run_uv(uvlight, t, lambda v: v)
    flat = uc.run_uv(uvlight, dict(t, light_intensity=t["light_intensity"][..., 0]), lambda v: v)
    assert t["light_intensity"].dim() == 3 and all(torch.equal(base[k], flat[k]) for k in base)
    one = dict(t, cam_pos=t["cam_pos"][:1].expand(3, 3))
    assert one["cam_pos"].stride(0) == 0
    a = uc.run_uv(uvlight, one, lambda v: v)
    b = uc.run_uv(uvlight, dict(t, cam_pos=t["cam_pos"][:1].repeat(3, 1)), lambda v: v)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["phong/spec"], base["phong/spec"])
    # only nml requires grad
    n = t["nml"].clone().requires_grad_(True)
    fixed = (t["cam_pos"], t["light_pos"], t["light_intensity"])
    d, s = uvlight.phong_features(t["p_uv"], n, *fixed, t["shadow_map"])
    (g,) = torch.autograd.grad((d * t["w_diff"]).sum() + (s * t["w_spec"]).sum(), n)
    assert torch.equal(g, base["phong/g_nml"])
    f, rgb = uvlight.ggx_features(t["p_uv"], n, *fixed, t["roughness"], t["tex_mean"], t["shadow_map"])
    (g,) = torch.autograd.grad((f * t["w_feat"]).sum() + (rgb * t["w_rgb"]).sum(), n)
    assert torch.equal(g, base["ggx/g_nml"])


def test_uvlight_rejects_powers_outside_the_domain():
    """More than GOL_UV_MAX_POW powers, and any power below 1 (infinite derivative at s = 0 in the reference expression
    too; at p = 0 the kernel's exp2(p log2 s) is NaN at s = 0, where torch.pow gives 1): ValueError before any launch."""
    from goliath_amd import uvlight

    t = _args("p1")
    ph = lambda pw: uvlight.phong_features(t["p_uv"], t["nml"], t["cam_pos"], t["light_pos"], t["light_intensity"], None,
                                           spec_powers=pw)
    gg = lambda pw: uvlight.ggx_features(t["p_uv"], t["nml"], t["cam_pos"], t["light_pos"], t["light_intensity"],
                                         t["roughness"], t["tex_mean"], None, spec_powers=pw)
    for f in (ph, gg):
        with pytest.raises(ValueError, match="at most 4"):
            f((1, 2, 4, 8, 16))
        for bad in ((0,), (1, 0.5), (16, -1.0), (float("nan"),)):
            with pytest.raises(ValueError, match=">= 1"):
                f(bad)
        f((1.0,))          # the boundary itself is in the domain
    torch.cuda.synchronize()
