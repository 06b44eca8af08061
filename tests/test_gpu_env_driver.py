"""GPU: the fused env-relight driver (goliath_amd.envdriver -> gol_envspin_frame), the device-side mip scale of the shading
kernel and dropin.patch_env_driver.

Parity bars (the ones tests/test_gpu_light_sh.py uses): against the float64 composition of envdriver_cases.py, evaluated on
OUR float32 rotations, every output is within 2 x the reference's own float32 error recorded in
tests/golden/env_driver_golden.npz (ours is another float32 evaluation order); against the reference's float32 recording,
3 x.  Every figure is printed before it is judged."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import envdriver_cases as EC

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def golden():
    return np.load(EC.GOLDEN)


def _spin(name):
    """(image, EnvSpin) of a case image, built once per session."""
    from goliath_amd import envdriver

    if name not in _CACHE:
        image = EC.full_image() if name == "full" else EC.images()[name]
        _CACHE[name] = (image, envdriver.EnvSpin(image, EC.ENV_SCALE, cycle=EC.CYCLE, envmap_dist=EC.ENVMAP_DIST))
    return _CACHE[name]


def _frame(spin, golden, key, indices, **kw):
    if indices is None:
        return spin.frame(lightrot=torch.from_numpy(golden[f"{key}/rot"]).cuda(), **kw)
    return spin.frame(index=indices, **kw)


def _outputs(fr):
    return {k: getattr(fr, k) for k in EC.OUTPUTS}


def _calls():
    small = [(name, tag, idx) for name in EC.images() for tag, idx in EC.batches()]
    return small + [("full", tag, idx) for tag, idx in EC.batches(full=True)]


@pytest.mark.parametrize("name,tag,indices", _calls(), ids=lambda v: v if isinstance(v, str) else None)
def test_parity_with_the_float64_composition_and_the_recording(golden, name, tag, indices):
    """The tightest bar is a scalar's: mip_scale of 33x70-generic, where the reference's float32 landed 6.8e-10 from the
    float64 value although half an ulp there is 1.86e-09 (bar 1.37e-09).  The kernel rounds norm_scale and mip_scale ONCE
    from double, so each is the float32 nearest to the float64 value or its neighbour across a near-tie: never further
    from it than a float32 evaluation can get by luck."""
    image, spin = _spin(name)
    _, H, W = image.shape
    key = f"{name}/{tag}"
    fr = _frame(spin, golden, key, indices)
    assert float(spin.perc90) == float(golden[f"{name}/perc90"])
    rot = fr.lightrot.cpu()
    assert float((rot - torch.from_numpy(golden[f"{key}/rot"])).abs().max()) <= 5e-7
    want = EC.compose64(image, rot, golden[f"{name}/perc90"])
    got = _outputs(fr)
    shapes = dict(envbg=(len(rot), 3, H, W), envmap=(len(rot), 3, 16, 32), light_intensity=(len(rot), 512, 3),
                  norm_scale=(len(rot),), mip_scale=(1,))
    failed = []
    for k in EC.OUTPUTS:
        assert tuple(got[k].shape) == shapes[k] and got[k].dtype == torch.float32
        assert bool(torch.isfinite(got[k]).all()), k
        err, bar = EC.max_err(got[k], want[k]), 2.0 * float(golden[f"{key}/err_ref32/{k}"])
        print(f"{key} {k}: vs float64 {err:.3e} (bar {bar:.3e})")
        if not err <= bar:
            failed.append((k, "float64", err, bar))
    if name != "full":
        envmap = torch.from_numpy(golden[f"{key}/envmap"])
        rec = dict(envmap=envmap, light_intensity=envmap.reshape(len(rot), 3, -1).transpose(1, 2),
                   norm_scale=torch.from_numpy(golden[f"{key}/norm_scale"]), mip_scale=torch.from_numpy(golden[f"{key}/mip_scale"]))
        errs = {k: EC.max_err(got[k], rec[k]) for k in rec}
        errs["envbg"] = max(EC.max_err(got["envbg"][b][:, EC.recorded_rows(H, W, b)], torch.from_numpy(golden[f"{key}/envbg"][b]))
                            for b in range(len(rot)))
        for k in EC.OUTPUTS:
            bar = 3.0 * float(golden[f"{key}/err_ref32/{k}"])
            print(f"{key} {k}: vs reference float32 {errs[k]:.3e} (bar {bar:.3e})")
            if not errs[k] <= bar:
                failed.append((k, "reference float32", errs[k], bar))
    assert not failed, failed
    assert torch.equal(fr.light_intensity, fr.envmap.reshape(len(rot), 3, -1).transpose(1, 2))
    assert torch.equal(fr.light_pos, (EC.ENVMAP_DIST * _sphvec().t())[None].expand(len(rot), -1, -1).cuda())
    assert tuple(fr.n_lights.shape) == (len(rot), 1) and bool((fr.n_lights == 512).all())


def _sphvec():
    L = 16                                                                  # light_decorator.py:42-52
    theta, phi = np.meshgrid((np.arange(L, dtype=np.float32) + 0.5) * np.pi / L,
                             (np.arange(-L, L, dtype=np.float32) + 0.5) * np.pi / L, indexing="ij")
    sph = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], axis=0).reshape((3, -1))
    return torch.from_numpy(sph)


@pytest.mark.parametrize("name", ["33x70", "48x96", "16x32"])   # the scalar-store path (H W % 4 != 0), the 16-byte one, 1 tap
def test_reproducible_batch_independent_and_envbg_optional(name):
    _, spin = _spin(name)
    idx = [7, 128, 201]
    a, b = spin.frame(index=idx), spin.frame(index=idx)
    for k in EC.OUTPUTS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for v, i in enumerate(idx):
        one = spin.frame(index=[i])
        for k in ("envbg", "envmap", "light_intensity", "norm_scale"):
            assert torch.equal(getattr(one, k)[0], getattr(a, k)[v]), (k, v)
    assert torch.equal(spin.frame(index=[7]).mip_scale, a.mip_scale)          # frame 0's value for the whole batch
    none = spin.frame(index=idx, want_envbg=False)
    assert none.envbg is None
    for k in EC.OUTPUTS[1:]:
        assert torch.equal(getattr(none, k), getattr(a, k)), k


def test_no_host_sync_and_graph_replay():
    _, spin = _spin("40x72")
    idx = torch.tensor([7, 128, 201], device="cuda")
    spin.frame(index=idx)                                                   # (first-call allocations)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = spin.frame(index=idx)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        spin.frame(index=idx)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = spin.frame(index=idx)
    graph.replay()
    for k in EC.OUTPUTS + ("lightrot",):
        assert torch.equal(getattr(captured, k), getattr(eager, k)), k
    idx.copy_(torch.tensor([-5, 64, 33], device="cuda"))                    # new indices into the SAME tensor
    graph.replay()
    again = spin.frame(index=idx)
    for k in EC.OUTPUTS + ("lightrot",):
        assert torch.equal(getattr(captured, k), getattr(again, k)), k
    assert not torch.equal(again.envmap, eager.envmap)


class _Deco:
    """The attribute layout of EnvSpinDecorator (light_decorator.py:18-52, 96-100)."""

    def __init__(self, image, levels):
        from goliath_amd import dropin

        self.image, self.env_scale, self.cycle, self.envmap_dist = image, EC.ENV_SCALE, EC.CYCLE, EC.ENVMAP_DIST
        self.sigma_step, self.miplevel = 0.2, len(levels)
        for i, m in enumerate(levels):
            setattr(self, f"mipmap_{i}", m)
        self.sphvec = _sphvec()
        self.mod = lambda **data: data
        self.mipmap = types.MethodType(dropin._shared_mipmap, self)


@pytest.mark.parametrize("fused_projection", [False, True])
def test_device_mip_scale_equals_the_host_float_bitwise(fused_projection, monkeypatch):
    """The scene of test_gpu_shade.py's shared-pyramid test; the levels carry `_gol_scale` once as the float s and once as a
    CUDA tensor holding s (gol_shade_in.mips_scale_dev): every output and every input gradient is bitwise equal, and the
    tensor variant runs without a host sync."""
    from goliath_amd import dropin, render_gs, shade

    monkeypatch.setenv("GOLIATH_CHECK_LIGHTROT", "0")
    B, S = 3, 24
    N = S * S
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    base = dict(f_vn=0.3 * r(B, 125, S, S), f_vc=0.3 * r(B, 4, S, S), postex=60.0 * r(B, 3, S, S), tn=F.normalize(r(B, 3, S, S), dim=1),
                albedo=0.2 + 0.6 * torch.rand(1, N, 3, generator=g), light_sh=0.3 * r(B, 3, 81), campos=torch.tensor([[30.0, -40.0, -900.0]]).repeat(B, 1),
                lightrot=torch.linalg.qr(r(B, 3, 3))[0], rand=0.3 * r(B, 3, 81))
    base = {k: v.cuda() for k, v in base.items()}
    deco = _Deco(None, [(torch.rand(1, 3, 16 >> i, 32 >> i, generator=g) * 1.6).cuda() for i in range(3)])
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = 300.0
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 48.0, 64.0, 1.0
    Rt = torch.eye(3, 4)[None].repeat(B, 1, 1)
    Rt[:, 2, 3] = 900.0
    vs = render_gs.view_set(K.cuda(), Rt.cuda(), 128, 96) if fused_projection else None
    wgen = torch.Generator().manual_seed(9)
    weights = {}

    def run(scale, no_sync):
        leaf = {k: base[k].clone().requires_grad_(True) for k in ("f_vn", "f_vc", "postex", "tn", "albedo")}
        mips = dropin._shared_mipmap(deco, B, torch.device("cuda"), scale)
        if no_sync:
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
        try:
            out = shade.shading_tail(leaf["f_vn"], leaf["f_vc"], leaf["postex"], leaf["tn"], leaf["albedo"], base["light_sh"],
                                     base["campos"], preconv_envmap=mips, lightrot=base["lightrot"], light_sh_rand=base["rand"],
                                     views=vs)
            terms = {k: v for k, v in sorted(out.items()) if torch.is_tensor(v) and v.requires_grad}
            if fused_projection:
                terms["records"] = out["projected"].records
            for k, v in terms.items():
                if k not in weights:
                    weights[k] = torch.randn(v.shape, generator=wgen).cuda()
            sum((v * weights[k]).sum() for k, v in terms.items()).backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return {k: v.detach() for k, v in out.items() if torch.is_tensor(v)}, {k: v.grad for k, v in leaf.items()}, mips

    s = 2.37
    run(s, False)                                   # fills `weights` and the packed-level cache outside the no-sync window
    o1, g1, m1 = run(s, False)
    dev = torch.tensor([s], device="cuda")
    o2, g2, m2 = run(dev, True)
    assert all(type(m._gol_scale) is float for m in m1) and all(m._gol_scale is dev for m in m2)
    assert len(o1) >= 10
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    o3, _, _ = run(torch.tensor([2.0 * s], device="cuda"), True)      # ... and the kernel really reads the device value
    assert not torch.equal(o3["spec_color"], o1["spec_color"])


def test_drop_in_forward(golden):
    from goliath_amd import dropin

    name, tag, idx = "33x70", "idx7_128_201", [7, 128, 201]
    image, _ = _spin(name)
    _, H, W = image.shape
    B = len(idx)
    seen = []

    class EnvSpinDecorator(_Deco):
        def forward(self, **data):
            seen.append(data)
            return "reference"

    mod = dropin.patch_env_driver(types.SimpleNamespace(EnvSpinDecorator=EnvSpinDecorator))
    levels = [torch.rand(1, 3, 16 >> i, 32 >> i) for i in range(3)]         # registered buffers live on the host
    d = mod.EnvSpinDecorator(image, levels)
    given = dict(campos=torch.zeros(B, 3, device="cuda"), index=idx, extra="kept")
    data = d.forward(**given)
    assert not seen
    want = dict(envmap=(B, 3, 16, 32), lightrot=(B, 3, 3), light_intensity=(B, 512, 3), light_pos=(B, 512, 3),
                envbg=(B, 3, H, W), n_lights=(B, 1), is_fullylit_frame=(1,))
    assert set(data) == set(given) | set(want) | {"preconv_envmap", "sigma_step", "light_type"}     # light_decorator.py:151-162
    for k, shape in want.items():
        assert tuple(data[k].shape) == shape and data[k].dtype == torch.float32 and data[k].is_cuda, k
    assert data["light_type"] == "envmap" and data["sigma_step"] == 0.2 and data["extra"] == "kept"
    assert bool((data["n_lights"] == 512).all()) and bool((data["is_fullylit_frame"] == 0).all())
    assert torch.equal(data["light_pos"].cpu(), (EC.ENVMAP_DIST * _sphvec().t())[None].expand(B, -1, -1))
    key = f"{name}/{tag}"
    envmap = torch.from_numpy(golden[f"{key}/envmap"])
    rec = dict(envmap=envmap, light_intensity=envmap.reshape(B, 3, -1).transpose(1, 2))
    for k, ref in rec.items():
        err, bar = EC.max_err(data[k], ref), 3.0 * float(golden[f"{key}/err_ref32/{k}"])
        print(f"drop-in {k}: {err:.3e} (bar {bar:.3e})")
        assert err <= bar, k
    err = max(EC.max_err(data["envbg"][b][:, EC.recorded_rows(H, W, b)], torch.from_numpy(golden[f"{key}/envbg"][b])) for b in range(B))
    assert err <= 3.0 * float(golden[f"{key}/err_ref32/envbg"])
    assert float((data["lightrot"].cpu() - torch.from_numpy(golden[f"{key}/rot"])).abs().max()) <= 5e-7
    mips = data["preconv_envmap"]
    scale = mips[0]._gol_scale
    assert torch.is_tensor(scale) and scale.is_cuda and scale.numel() == 1 and all(m._gol_scale is scale for m in mips)
    err, bar = EC.max_err(scale, torch.from_numpy(golden[f"{key}/mip_scale"])), 3.0 * float(golden[f"{key}/err_ref32/mip_scale"])
    assert err <= bar, (err, bar)
    for m, lvl in zip(mips, levels):                                       # what other readers of the pyramid see
        assert tuple(m.shape) == (B, *lvl.shape[1:]) and torch.allclose(m[0].cpu(), lvl[0] * float(scale), rtol=1e-6)
    # the state is cached on the image; a decorator whose percentile is not positive stays on the reference
    state = d.__dict__["_gol_env_spin"][1]
    d.forward(**given)
    assert d.__dict__["_gol_env_spin"][1] is state
    dark = torch.zeros(3, H, W)
    dark[:, 0, :5] = 1.0
    d2 = mod.EnvSpinDecorator(dark, levels)
    assert d2.forward(**given) == "reference" and len(seen) == 1 and seen[0]["index"] == idx
