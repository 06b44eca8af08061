"""GPU: gol_shadow_pcf (goliath_amd.shadowmap) vs the golden vectors made by the reference's get_shadow_map."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "shadow_golden.npz")


def _cases():
    G = np.load(GOLD)
    for tag in ("a", "b"):
        yield tag, {k.split("/")[1]: torch.from_numpy(G[k]).cuda() for k in G.files if k.startswith(tag + "/")}


def _close(a, b, frac=0.005):
    # nearest-neighbour lookups: a rounding tie may fall on the other side for a handful of texels
    bad = ((a - b).abs() > 1e-3 * (1 + b.abs())).float().mean()
    return float(bad) < frac


def test_shadow_pcf_matches_reference_golden():
    from goliath_amd import shadowmap

    for tag, c in _cases():
        got = shadowmap.shadow_pcf(c["depth"], c["Rt"], c["postex"], c.get("nml"))
        assert got.shape == c["out"].shape
        assert _close(got, c["out"]), tag
        # the same comparison as ONE number (parity ledger): rel-L2 over all texels; measured 6.7e-7 -- no tie texel in
        # these two cases (the _close() allowance above is for scenes that have one)
        from scenes import rel_l2

        assert rel_l2(got, c["out"]) < 1e-5, tag
        fused = shadowmap.shadow_pcf(c["depth"], c["Rt"], c["postex"], c.get("nml"), exp_scale=8.0)
        assert torch.allclose(fused, torch.exp(-got / 8.0), atol=1e-6)


def test_get_shadow_map_dropin_and_light_inner_loop():
    from goliath_amd import shadowmap

    tag, c = next(_cases())

    class RL:
        h, w = c["depth"].shape[-2:]

        def __call__(self, verts, tex, K, Rt):
            assert float(K[0, 0, 0]) == 1000.0 and float(K[0, 0, 2]) == self.w / 2
            return {"depth_img": c["depth"]}

    got = shadowmap.get_shadow_map(RL(), c["Rt"], None, torch.zeros(3, 10, 3).cuda(), c["postex"], c["nml"])
    assert _close(got, c["out"])
    # native form: one set of texels, L light cameras -> same as repeating the texels per light
    p0, n0 = c["postex"][:1], c["nml"][:1]
    L = c["Rt"].shape[0]
    a = shadowmap.shadow_pcf(c["depth"], c["Rt"], p0, n0)
    b = shadowmap.shadow_pcf(c["depth"], c["Rt"], p0.expand(L, -1, -1, -1).contiguous(), n0.expand(L, -1, -1, -1).contiguous())
    assert torch.equal(a, b)


# ---- edge shapes against the float64 oracle (inputs: tests/urhand_cases.py, guarded on the CPU by tests/test_urhand_cases.py)
def _scene(tag):
    import urhand_cases as uc

    s = uc.shadow_scene(tag)
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in s.items()}
    return dev, uc.shadow_oracle(tag, torch.float64)


def _assert_every_texel(got, ref, tag):
    """The file's per-texel bound with NO exception allowed (the case inputs hold no rounding tie: every sample coordinate
    is >= 0.05 px from k + 0.5, the float32 coordinate error is of order 1e-3 px), and the file's rel-L2 bar."""
    from scenes import rel_l2

    assert got.shape == ref.shape, tag
    err = (got.double().cpu() - ref).abs() / (1 + ref.abs())
    e = rel_l2(got, ref)
    print(f"\nSHADOW_EDGE {tag}: rel-L2 {e:.2e}, worst |d| / (1 + |ref|) {float(err.max()):.2e}, "
          f"texels over 1e-3: {int((err > 1e-3).sum())} of {err.numel()}")
    assert e < 1e-5, tag
    assert bool((err <= 1e-3).all()), (tag, int((err > 1e-3).sum()), float(err.max()))


@pytest.mark.parametrize("tag", ["native_BL", "native_BL_nonml", "tall", "dyadic_ties"])
def test_shadow_pcf_edge_shapes_vs_float64_oracle(tag):
    """[B, L] native form with B, L > 1 on a non-square map (bl = b * L + l addresses depth, Rt and out; dh / dw and
    cx / cy differ), a tall map, and exact rounding ties (round half to even, inclusive 0 / exclusive size in-bounds
    edges).  Measured (SHADOW_EDGE lines): rel-L2 5.4e-8 / 5.6e-7 / 5.4e-8 / 6.7e-7, worst |d| / (1 + |ref|) 7.2e-5 /
    1.5e-5 / 5.9e-5 / 1.0e-5, no texel of 2622 / 2622 / 768 / 1600 over 1e-3 -- the same figures as the float32 oracle."""
    from goliath_amd import shadowmap

    s, ref = _scene(tag)
    got = shadowmap.shadow_pcf(s["depth"], s["Rt"], s["postex"], s["nml"], focal=s["focal"])
    _assert_every_texel(got, ref, tag)
    if tag == "native_BL":
        fused = shadowmap.shadow_pcf(s["depth"], s["Rt"], s["postex"], s["nml"], exp_scale=8.0, focal=s["focal"])
        assert torch.allclose(fused.double().cpu(), torch.exp(-ref / 8.0), atol=1e-6)
        # a permuted (non-contiguous) view of the texels and a float64 depth image: bit-equal to their plain copies
        view = s["postex"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not view.is_contiguous() and torch.equal(view, s["postex"])
        assert torch.equal(shadowmap.shadow_pcf(s["depth"], s["Rt"], view, s["nml"]), got)
        assert torch.equal(shadowmap.shadow_pcf(s["depth"].double(), s["Rt"], s["postex"], s["nml"]), got)


def test_get_shadow_map_on_a_tall_render_layer():
    """The drop-in with a render layer whose h != w: the K handed to the layer carries cx = w / 2, cy = h / 2, and the
    lookup uses the depth image's own height and width."""
    from goliath_amd import shadowmap

    s, ref = _scene("tall")

    class RL:
        h, w = s["depth"].shape[-2:]

        def __call__(self, verts, tex, K, Rt):
            assert (self.h, self.w) == (48, 20) and K.shape == (3, 3, 3)
            want = torch.tensor([[1000.0, 0.0, self.w / 2], [0.0, 1000.0, self.h / 2], [0.0, 0.0, 1.0]])
            assert all(torch.equal(k.cpu(), want) for k in K)
            return {"depth_img": s["depth"]}

    got = shadowmap.get_shadow_map(RL(), s["Rt"], None, torch.zeros(3, 10, 3).cuda(), s["postex"], s["nml"])
    _assert_every_texel(got, ref, "tall/get_shadow_map")


def test_shadow_pcf_empty_forms():
    from goliath_amd import shadowmap

    z = lambda *shape: torch.zeros(*shape, device="cuda")
    assert shadowmap.shadow_pcf(z(0, 8, 12), z(0, 3, 4), z(0, 3, 5, 7), z(0, 3, 5, 7)).shape == (0, 1, 5, 7)   # B == 0
    assert shadowmap.shadow_pcf(z(0, 8, 12), z(0, 3, 4), z(2, 3, 5, 7), None).shape == (0, 1, 5, 7)            # L == 0
    torch.cuda.synchronize()
