"""GPU: the fused light path (goliath_amd/lights.py over csrc/lightsh.hip, dropin.patch_sh) against the reference's own
`dir2sh_torch` recorded in float64 (tests/golden/light_sh_golden.npz, made by tests/golden/make_light_sh_golden.py) and
against the calls the reference's model code made (tests/golden/rgca_model_golden.npz).

The yardstick of the basis is the reference's OWN float32 error on the same directions, err_ref32 = max |dir2sh_torch(float32)
- dir2sh_torch(float64)|, recorded per direction set: ours is another float32 evaluation order of the same recurrences and
is held to 2 x that; against a float32 RECORDING of the reference (which carries 1 x itself) to 3 x.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

import npz_parts
import rgca_shaped as S
from scenes import rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BAR_FRAME = 3e-5   # rel-L2, the bar tests/test_gpu_rgca_model_golden.py applies to headrel_light_sh (BAR_PER_GAUSSIAN)
FRAMES = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "light_sh_golden.npz")))


@pytest.fixture(scope="module")
def model_gold():
    return npz_parts.load(os.path.join(HERE, "golden", "rgca_model_golden.npz"))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- basis -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [8, 0, 1, 2])
@pytest.mark.parametrize("name", ["generic", "polar"])
def test_basis_within_twice_the_references_float32_error(gold, name, deg):
    """Every output finite, max |Y_hip - truth| <= 2 err_ref32 of the set; deg < 8 is a prefix of the same truth."""
    from goliath_amd import lights

    dirs, truth = _t(gold[f"{name}/dirs"]).cuda(), _t(gold[f"{name}/truth"])
    n = (deg + 1) ** 2
    got = lights.dir2sh(deg, dirs)
    assert got.dtype == torch.float32 and tuple(got.shape) == (dirs.shape[0], n)
    assert bool(torch.isfinite(got).all())
    err = float((got.double().cpu() - truth[:, :n]).abs().max())
    bar = 2.0 * float(gold[f"{name}/err_ref32"])
    print(f"\nLIGHT_SH basis {name} deg={deg} max_abs_err={err:.3e} bar={bar:.3e}")
    assert err <= bar, (name, deg, err, bar)


@pytest.mark.parametrize("M", [1, 65, 257])
def test_basis_row_counts_one_row_wave_plus_one_workgroup_plus_one(gold, M):
    """Slices of the generic set: each row equals (bitwise) the row of the full call, and meets the same bar."""
    from goliath_amd import lights

    dirs, truth = _t(gold["generic/dirs"]).cuda(), _t(gold["generic/truth"])
    assert dirs.shape[0] >= 257
    full = lights.dir2sh(8, dirs)
    got = lights.dir2sh(8, dirs[:M])
    assert tuple(got.shape) == (M, 81) and torch.equal(got, full[:M])
    lead = lights.dir2sh(8, dirs[:M].reshape(1, M, 1, 3))       # leading dimensions are kept
    assert tuple(lead.shape) == (1, M, 1, 81) and torch.equal(lead.reshape(M, 81), got)
    err = float((got.double().cpu() - truth[:M]).abs().max())
    assert err <= 2.0 * float(gold["generic/err_ref32"]), (M, err)


def test_basis_against_the_recorded_reference_calls(gold, model_gold):
    """Every dir2sh_torch call the reference's model code made while the model fixture was recorded (float32, CPU):
    3 x err_ref32(generic) = our 2 x plus the recording's own 1 x."""
    from goliath_amd import lights

    G = model_gold
    keys = [k for k in G.files if k.endswith("/dirs") and "/sh" in k]
    assert keys
    bar = 3.0 * float(gold["generic/err_ref32"])
    for k in keys:
        coeffs = _t(G[k[:-len("dirs")] + "coeffs"])
        deg = int(round(coeffs.shape[-1] ** 0.5)) - 1
        got = lights.dir2sh(deg, _t(G[k]).cuda()).cpu()
        assert tuple(got.shape) == tuple(coeffs.shape)
        err = float((got.double() - coeffs.double()).abs().max())
        print(f"\nLIGHT_SH recorded {k} {tuple(coeffs.shape)} max_abs_err={err:.3e} bar={bar:.3e}")
        assert err <= bar, (k, err, bar)


# ---- fused frame -----------------------------------------------------------------------------------------------------------
def _frame(gold, i):
    return {k: _t(gold[f"frame{i}/{k}"]) for k in ("light_pos", "light_intensity", "head_pose", "headrel_light_pos",
                                                   "headrel_light_sh")}


@pytest.mark.parametrize("i", FRAMES)
def test_frame_against_the_float64_composition(gold, i):
    """(B=1, L=1, identity), (B=2, L=3, C=1), (B=2, L=512, C=3), (B=3, L=257, C=1, 100 padded): both outputs to rel-L2 3e-5
    against rgca.py:175-191 composed in float64 with the reference's dir2sh_torch."""
    from goliath_amd import lights

    f = _frame(gold, i)
    pos, sh = lights.headrel_light_sh(f["light_pos"].cuda(), f["light_intensity"].cuda(), f["head_pose"].cuda(), 8)
    assert tuple(pos.shape) == tuple(f["headrel_light_pos"].shape) and tuple(sh.shape) == tuple(f["headrel_light_sh"].shape)
    assert bool(torch.isfinite(pos).all()) and bool(torch.isfinite(sh).all())
    e_pos, e_sh = rel_l2(pos.cpu(), f["headrel_light_pos"]), rel_l2(sh.cpu(), f["headrel_light_sh"])
    print(f"\nLIGHT_SH frame{i} rel_l2 headrel_light_pos={e_pos:.3e} headrel_light_sh={e_sh:.3e} bar={BAR_FRAME:.0e}")
    assert e_pos <= BAR_FRAME and e_sh <= BAR_FRAME, (i, e_pos, e_sh)
    if i == 0:   # identity pose handed over as None
        pos0, sh0 = lights.headrel_light_sh(f["light_pos"].cuda(), f["light_intensity"].cuda(), None, 8)
        assert torch.equal(pos0, pos) and torch.equal(sh0, sh)


def test_padded_lights_contribute_exactly_nothing(gold):
    """The padded case against the same case truncated to its 157 real lights: BITWISE (torch.equal) -- the sum runs in light
    order into one accumulator per output and a padded light adds Y * 0 to it."""
    from goliath_amd import lights

    f = _frame(gold, 3)
    padded = int(gold["frame3/padded"])
    real = f["light_pos"].shape[1] - padded
    assert (padded, real) == (100, 157)
    assert not f["light_intensity"][:, real:].any() and not f["light_pos"][:, real:].any()
    lp, li, hp = f["light_pos"].cuda(), f["light_intensity"].cuda(), f["head_pose"].cuda()
    pos, sh = lights.headrel_light_sh(lp, li, hp, 8)
    pos_t, sh_t = lights.headrel_light_sh(lp[:, :real], li[:, :real], hp, 8)
    assert torch.equal(sh, sh_t) and torch.equal(pos[:, :real], pos_t)


def _model_batches(G):
    from test_gpu_rgca_model_golden import _cuda, _env_batch, _stored

    yield "train_point", _cuda(S.batch_inputs(2, 0, stored=_stored(G, "train_point")))
    yield "eval_env", _env_batch(G, "eval_env", 2, 100, with_envbg=False)
    yield "vis_env", _env_batch(G, "vis_env", 1, 200, with_envbg=True)


def test_frame_against_the_recorded_model_outputs(model_gold):
    """The batches tests/test_gpu_rgca_model_golden.py builds for its three cases: headrel_light_sh against what the
    reference's AutoEncoder.forward returned (float32, CPU), to that test's bar."""
    from goliath_amd import lights

    for tag, batch in _model_batches(model_gold):
        want = _t(model_gold[f"{tag}/out/headrel_light_sh"])
        _, sh = lights.headrel_light_sh(batch["light_pos"], batch["light_intensity"], batch["head_pose"], 8)
        assert tuple(sh.shape) == tuple(want.shape)
        err = rel_l2(sh.cpu(), want)
        print(f"\nLIGHT_SH model {tag} L={batch['light_pos'].shape[1]} rel_l2 headrel_light_sh={err:.3e} bar={BAR_FRAME:.0e}")
        assert err <= BAR_FRAME, (tag, err)


# ---- no sync, repeatable ----------------------------------------------------------------------------------------------------
def test_no_host_sync(gold):
    from goliath_amd import lights

    f = _frame(gold, 2)
    lp, li, hp = f["light_pos"].cuda(), f["light_intensity"].cuda(), f["head_pose"].cuda()
    probe = torch.ones(1, device="cuda")
    lights.headrel_light_sh(lp, li, hp, 8)        # (library load, first launch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        live = False
        try:
            probe.item()
        except RuntimeError:
            live = True
        if live:
            pos, sh = lights.headrel_light_sh(lp, li, hp, 8)
            ld, lsh = lights.random_light_sh(8, 4, lp.device, torch.float32)
            basis = lights.dir2sh(8, lp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') is inert on this build: .item() does not raise under it")
    assert tuple(sh.shape) == (2, 3, 81) and tuple(lsh.shape) == (4, 3, 81) and tuple(ld.shape) == (4, 1, 3)
    assert bool(torch.isfinite(sh).all() and torch.isfinite(lsh).all() and torch.isfinite(basis).all())


def test_bitwise_repeatable(gold):
    from goliath_amd import lights

    f = _frame(gold, 2)
    lp, li, hp = f["light_pos"].cuda(), f["light_intensity"].cuda(), f["head_pose"].cuda()
    a, b = lights.headrel_light_sh(lp, li, hp, 8), lights.headrel_light_sh(lp, li, hp, 8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(lights.dir2sh(8, lp), lights.dir2sh(8, lp))


def test_random_light_is_the_basis_of_its_direction():
    """random_light_sh: unit directions, and light_sh[b, c] = dir2sh(light_dir[b]) for each of the three channels (a sum
    over ONE light of unit intensity; the fused entry normalises once more, which moves a unit vector by an ulp)."""
    from goliath_amd import lights

    ld, lsh = lights.random_light_sh(8, 5, "cuda", torch.float32)
    assert tuple(ld.shape) == (5, 1, 3) and tuple(lsh.shape) == (5, 3, 81) and lsh.is_contiguous()
    assert float((ld.norm(dim=-1) - 1.0).abs().max()) < 1e-6
    want = lights.dir2sh(8, ld)[:, 0]
    for c in range(3):
        assert float((lsh[:, c] - want).abs().max()) < 1e-5
    assert torch.equal(lsh[:, 0], lsh[:, 1]) and torch.equal(lsh[:, 0], lsh[:, 2])


# ---- wiring ----------------------------------------------------------------------------------------------------------------
class _CountingSh:
    """`ca_code.utils.sh` as a module whose dir2sh_torch counts its calls (and is no spherical harmonic)."""

    def __init__(self):
        self.calls = 0
        self.module = types.ModuleType("ca_code.utils.sh")
        self.module.dir2sh_torch = self.dir2sh_torch

    def dir2sh_torch(self, n, d):
        self.calls += 1
        return torch.cos(d[..., :1] + torch.arange((n + 1) ** 2, device=d.device, dtype=d.dtype))

    def __enter__(self):
        names = ("ca_code", "ca_code.utils", "ca_code.utils.sh")
        self._saved = {k: sys.modules.get(k) for k in names}
        for name in names[:2]:
            sys.modules[name] = types.ModuleType(name)
        sys.modules["ca_code.utils.sh"] = self.module
        sys.modules["ca_code.utils"].sh = self.module
        sys.modules["ca_code"].utils = sys.modules["ca_code.utils"]
        return self

    def __exit__(self, *exc):
        for k, v in self._saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_wiring_through_the_model_forward(model_gold):
    """The stand-in of tests/rgca_shaped.py with the forwards dropin.patch_rgca() installs.  Unpatched, the module's
    dir2sh_torch is called once in eval and twice in training; after dropin.patch_sh() not at all, headrel_light_sh is
    lights.headrel_light_sh of the batch, and the other keys are there as before."""
    from goliath_amd import dropin, lights, rgca
    from test_gpu_rgca_model_golden import _cuda, _model, _stored

    G = model_gold
    st = _stored(G, "train_point")
    embs, geom = (t.detach().cuda() for t in S.leaves(2, 0, st))
    m = _model(G, embs, geom)
    batch = _cuda(S.batch_inputs(2, 0, stored=st))
    classes = types.SimpleNamespace(AutoEncoder=type(m), PrimDecoder=type(m.decoder))
    assert not getattr(m, rgca.LIGHT_SH_FLAG, False) and not getattr(m.decoder, rgca.LIGHT_SH_FLAG, False)
    with _CountingSh() as sh, torch.no_grad():
        before = {}
        for mode, calls in (("eval", 1), ("train", 2)):
            getattr(m, mode)()
            sh.calls = 0
            before[mode] = m.forward(**batch)
            assert sh.calls == calls, (mode, sh.calls)
        try:
            assert dropin.patch_sh(sh.module, classes) == (sh.module, classes)
            wrapper = sh.module.dir2sh_torch
            # the wrapper itself: CUDA float32 runs the kernel, float64 / requires_grad go to the original
            sh.calls = 0
            d = batch["light_pos"]
            assert torch.equal(wrapper(8, d), lights.dir2sh(8, d)) and sh.calls == 0
            wrapper(8, d.double())
            with torch.enable_grad():
                wrapper(8, d.clone().requires_grad_(True))
            assert sh.calls == 2
            want_pos, want_sh = lights.headrel_light_sh(batch["light_pos"], batch["light_intensity"], batch["head_pose"], 8)
            for mode in ("eval", "train"):
                getattr(m, mode)()
                sh.calls = 0
                preds = m.forward(**batch)
                assert sh.calls == 0, (mode, sh.calls)
                assert torch.equal(preds["headrel_light_sh"], want_sh)
                assert set(preds) == set(before[mode]), set(preds) ^ set(before[mode])
                for k, v in preds.items():
                    if torch.is_tensor(v):
                        assert v.shape == before[mode][k].shape and bool(torch.isfinite(v).all()), k
        finally:   # the flags are class attributes: later tests build the same classes
            for cls in (classes.AutoEncoder, classes.PrimDecoder):
                if rgca.LIGHT_SH_FLAG in vars(cls):
                    delattr(cls, rgca.LIGHT_SH_FLAG)
