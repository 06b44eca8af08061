"""Guards the inputs of the case-driven tests of tests/test_gpu_shadow.py and tests/test_gpu_uvlight.py on the CPU: the
shadow scenes must hold no rounding tie and must reach every border, hole and behind-the-camera class of the 3x3 taps, the
UV light cases must reach both halves of every clamp of oracle/urhand_ref.py, and the reference pair (the oracle in float32
against the same oracle in float64) the GPU bars are built from must be usable.  Every class is derived from the float64
oracle, never from the code under test."""
import math

import pytest
import torch

import urhand_cases as uc


# ------------------------------------------------------------------------------------------------------ shadow PCF
def test_shadow_oracle_follows_its_input_dtype():
    for tag in uc.SHADOW_TAGS:
        o32, o64 = uc.shadow_oracle(tag, torch.float32), uc.shadow_oracle(tag, torch.float64)
        s = uc.shadow_scene(tag)
        assert o32.dtype == torch.float32 and o64.dtype == torch.float64
        assert o32.shape == o64.shape == (s["B"] * s["L"], 1) + tuple(s["postex"].shape[-2:])
        assert bool(torch.isfinite(o64).all()) and bool(torch.isfinite(o32).all())


def test_shadow_taps_helper_is_the_pixel_coordinate_minus_one():
    """The centre tap of the reference's normalisation samples at u_pix - 1 (u_pix = f X / Z + c): checked against a
    projection written out by hand, on a non-square map."""
    from oracle import urhand_ref

    s = uc.shadow_scene("native_BL")
    depth, Rt, postex, _ = uc.shadow_oracle_inputs("native_BL", torch.float64)
    ix, iy, Z = urhand_ref.shadow_pcf_taps(depth.float(), Rt.float(), postex.float(), s["focal"])   # float32 in, float64 out
    assert ix.dtype == iy.dtype == Z.dtype == torch.float64
    pc = torch.einsum("bij,bjhw->bihw", Rt[:, :, :3], postex) + Rt[:, :, 3, None, None]
    dh, dw = depth.shape[-2:]
    assert (dh, dw) == (40, 56)
    assert torch.allclose(ix, s["focal"] * pc[:, 0] / pc[:, 2] + dw / 2 - 1, rtol=0, atol=1e-9)
    assert torch.allclose(iy, s["focal"] * pc[:, 1] / pc[:, 2] + dh / 2 - 1, rtol=0, atol=1e-9)
    assert torch.equal(Z, pc[:, 2])


@pytest.mark.parametrize("tag", list(uc.SHADOW))
def test_shadow_scene_has_no_tie_and_reaches_every_tap_class(tag):
    """Measured (share of (camera, texel) pairs): native_BL all-inside 0.54, left / right / top / bottom 0.037 / 0.027 /
    0.039 / 0.037, all-outside 0.32, all-holes 0.12, mixed 0.49, 168 pairs behind the camera, 52 % of the candidate
    texels accepted by the tie rule at L = 3 (0.9^6 = 53 %); tall: all-inside 0.44, borders 0.06 .. 0.10, 80 % accepted at
    L = 1 (0.9^2 = 81 %).  The float32 oracle then agrees with the float64 oracle at EVERY texel: worst
    |d| / (1 + |ref|) 7.2e-5 (native_BL), 1.5e-5 (no normals), 5.9e-5 (tall) -- the GPU tests' per-texel bar is 1e-3."""
    c, s, k = uc.SHADOW[tag], uc.shadow_scene(tag), uc.shadow_classes(tag)
    assert s["postex"].shape == (c["B"], 3, c["H"], c["W"]) and s["postex"].dtype == torch.float32
    assert s["depth"].shape == (c["B"] * c["L"], c["dh"], c["dw"]) and s["Rt"].shape == (c["B"] * c["L"], 3, 4)
    assert (s["nml"] is not None) == c["nml"] and s["focal"] == 1000.0 and max(c["dh"], c["dw"]) <= 64
    assert len({tuple(m.flatten().tolist()) for m in s["Rt"]}) == c["B"] * c["L"]            # every camera its own Rt ...
    assert all(not torch.equal(s["depth"][i], s["depth"][j])                                 # ... and its own depth image
               for i in range(c["B"] * c["L"]) for j in range(i))
    # depth: 650 + 150 rand, a quarter of the pixels holes, and an all-hole rectangle of at least 8 x 8
    hit = s["depth"][s["depth"] > 0]
    assert 650 <= float(hit.min()) and float(hit.max()) <= 800
    y0, y1, x0, x1 = c["hole"]
    assert y1 - y0 >= 8 and x1 - x0 >= 8 and not s["depth"][:, y0:y1, x0:x1].any()
    outside_rect = torch.ones_like(s["depth"], dtype=torch.bool)
    outside_rect[:, y0:y1, x0:x1] = False
    assert 0.20 < float((s["depth"][outside_rect] == 0).float().mean()) < 0.30
    # no tie: the margin holds for the float32 positions the kernel is given (the classes are evaluated on those)
    print(f"{tag}: accepted {s['accepted']:.3f}, min margin {float(k['margin'].min()):.4f} px")
    assert float(k["margin"].min()) >= uc.TIE_MARGIN
    assert 0.3 < s["accepted"] < 0.95                 # the rule did reject, and was not starved
    # coverage of the tap classes
    share = {n: float(k[n].float().mean()) for n in ("all_inside", "left", "right", "top", "bottom", "all_outside",
                                                     "all_holes", "mixed")}
    print(tag, " ".join(f"{n} {v:.3f}" for n, v in share.items()), "behind", int((k["Z"] < 0).sum()))
    assert all(v >= 0.02 for v in share.values()), share
    assert int((k["Z"] < 0).sum()) >= 8 and float(k["Z"].abs().min()) >= 1.0
    if tag == "tall":
        assert c["dh"] > c["dw"] and c["L"] == 1 and share["all_inside"] >= 0.20
    else:
        assert c["dh"] < c["dw"] and c["B"] > 1 and c["L"] > 1 and c["H"] * c["W"] == 437      # 256 + 181: a partial block
    # the float32 oracle has no tie flip either: it meets the GPU tests' per-texel bound against float64 everywhere
    o32, o64 = uc.shadow_oracle(tag, torch.float32), uc.shadow_oracle(tag, torch.float64)
    worst = float(((o32 - o64).abs() / (1 + o64.abs())).max())
    print(f"{tag}: float32 oracle vs float64 oracle, worst |d| / (1 + |ref|) {worst:.2e}, rel-L2 {uc.rel(o32, o64):.2e}")
    assert worst < 1e-3


def test_shadow_nonml_case_is_the_same_scene():
    a, b = uc.shadow_scene("native_BL"), uc.shadow_scene("native_BL_nonml")
    assert all(torch.equal(a[k], b[k]) for k in ("depth", "Rt", "postex")) and b["nml"] is None and a["nml"] is not None
    assert not torch.equal(uc.shadow_oracle("native_BL", torch.float64), uc.shadow_oracle("native_BL_nonml", torch.float64))


def test_shadow_dyadic_ties_case():
    """Measured: 75 % of the 1600 texels have a coordinate exactly on k + 0.5; Z - d > 0 for 43 % of the texels; float32
    oracle vs float64 oracle max |d| 1.25e-5, worst |d| / (1 + |ref|) 1.0e-5 (same sample positions in both)."""
    s, k = uc.shadow_scene("dyadic_ties"), uc.shadow_classes("dyadic_ties")
    assert s["postex"].shape == (1, 3, 40, 40) and s["depth"].shape == (1, 16, 16) and s["focal"] == 1024.0
    assert torch.equal(s["Rt"][0], torch.eye(3, 4))
    # exactly representable: the float64 helper gives x + 7, y + 7 without rounding
    assert torch.equal(k["ix"][0], (s["postex"][0, 0].double() + 7).flatten())
    assert torch.equal(k["iy"][0], (s["postex"][0, 1].double() + 7).flatten())
    tie_x, tie_y = (k["ix"] % 1 == 0.5), (k["iy"] % 1 == 0.5)
    assert float(tie_x.float().mean()) == 0.5 and float(tie_y.float().mean()) == 0.5
    # tap coordinates that tie right at both borders: -0.5 -> 0 (inside; half away from zero would leave the map), 15.5 -> 16
    # (outside; half down would stay inside), and ties that go down (0.5 -> 0, 14.5 -> 14) as well as up (1.5 -> 2); the
    # indices -1 and 16 = dw are reached as taps
    for c in (k["ix"][0], k["iy"][0]):
        taps = set((c[:, None] + torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)).flatten().tolist())
        assert {-1.5, -0.5, 0.5, 1.5, 14.5, 15.5, 16.5} <= taps
        assert {-1.0, 0.0, 15.0, 16.0} <= {float(round(t)) for t in taps}        # Python's round: half to even, too
    o32, o64 = uc.shadow_oracle("dyadic_ties", torch.float32), uc.shadow_oracle("dyadic_ties", torch.float64)
    pos = float((o64 > 0).float().mean())
    worst = float(((o32 - o64).abs() / (1 + o64.abs())).max())
    print(f"dyadic_ties: Z - d > 0 for {pos:.3f} of the texels; float32 vs float64 oracle max |d| "
          f"{float((o32 - o64).abs().max()):.2e}, worst |d| / (1 + |ref|) {worst:.2e}")
    assert pos >= 0.25 and worst < 1e-3
    assert all(float(k[n].float().mean()) >= 0.02 for n in ("all_inside", "left", "right", "top", "bottom", "all_outside"))


def test_shadow_generators_are_seeded():
    for tag in uc.SHADOW_TAGS:
        a = uc.shadow_scene(tag)
        uc.shadow_scene.cache_clear()
        b = uc.shadow_scene(tag)
        assert all(torch.equal(a[k], b[k]) for k in ("depth", "Rt", "postex"))
    uc.shadow_classes.cache_clear()
    uc.shadow_oracle.cache_clear()


# -------------------------------------------------------------------------------------------------- UV light loops
def test_uv_cases_are_the_shapes_and_kinds_the_gpu_tests_rely_on():
    for tag, c in uc.UV.items():
        t = uc.uv_inputs(tag)
        B, L, H, W, P = c["B"], c["L"], c["H"], c["W"], len(c["powers"])
        assert t["p_uv"].shape == t["nml"].shape == t["tex_mean"].shape == (B, 3, H, W)
        assert t["light_pos"].shape == (B, L, 3) and t["light_intensity"].shape == (B, L, 1) and t["cam_pos"].shape == (B, 3)
        assert (t["shadow_map"] is not None) == c["shadow"] and (not c["shadow"] or t["shadow_map"].shape == (B, L, 1, H, W))
        assert H * W > 256 and (H * W) % 256 != 0 and B > 1                       # several blocks, a partial tail, B > 1
        assert torch.allclose(t["light_pos"].norm(dim=-1), torch.tensor(1100.0), rtol=1e-5)
        assert float((t["cam_pos"] - torch.tensor([20.0, 10.0, -800.0])).abs().max()) < 150
        assert not torch.equal(t["cam_pos"][0], t["cam_pos"][1])
        lo, hi = c["rough"]
        assert lo <= float(t["roughness"].min()) and float(t["roughness"].max()) <= hi
        assert float(t["roughness"].min()) < lo + 0.05 * (hi - lo)                # the lower bound is approached ...
        assert float(t["roughness"].max()) > lo + 0.75 * (hi - lo)                # ... and the upper quarter is reached
        ln = t["nml"].norm(dim=1)
        if c["normals"] == "unit":
            assert float((ln - 1).abs().max()) < 1e-6
        else:
            assert 0.6 <= float(ln.min()) < 0.65 and 1.45 < float(ln.max()) <= 1.5 + 1e-6
        if c.get("dark"):
            assert not t["light_intensity"].any()
        else:
            assert 0.05 <= float(t["light_intensity"].min()) and not torch.equal(t["light_intensity"][0], t["light_intensity"][1])
        assert t["w_spec"].shape == (B, P, 1, H, W) and t["w_feat"].shape == (B, 1 + P, H, W)
    assert (uc.UV["tail_unit"]["H"] * uc.UV["tail_unit"]["W"], uc.UV["p1"]["H"] * uc.UV["p1"]["W"]) == (527, 261)
    assert {len(c["powers"]) for c in uc.UV.values()} == {0, 1, 3, 4}             # P = 0, 1, 3 and GOL_UV_MAX_POW
    assert all(p >= 1 for c in uc.UV.values() for p in c["powers"])
    first = uc.uv_inputs("nonunit")
    uc.uv_inputs.cache_clear()
    again = uc.uv_inputs("nonunit")
    assert first is not again and all(torch.equal(first[k], again[k]) for k in ("p_uv", "nml", "roughness", "w_feat"))


def test_uv_cases_reach_both_halves_of_every_clamp():
    """Measured share of (texel, light) pairs: tail_unit n.L < 0 0.50, ref.L < 0 0.48, V.n < 0 0.48 (and n.L > 1,
    ref.L > 1: none -- unit normals never reach the upper clamps); nonunit n.L > 1 0.053, ref.L > 1 0.061; highlight
    n.L > 1 0.157, ref.L > 1 0.320, GGX specular > 1 0.119 (largest 4.8: under the float32 overflow of power 64 at 4.09
    for all but 0.2 % of the pairs, see urhand_cases.uv_inputs)."""
    m = uc.uv_intermediates("tail_unit")
    sh = lambda x: float(x.double().mean())
    print("tail_unit: n.L<0 %.3f ref.L<0 %.3f V.n<0 %.3f" % (sh(m["ndl"] < 0), sh(m["rdl"] < 0), sh(m["vdn"] < 0)))
    assert sh(m["ndl"] < 0) >= 0.20 and sh(m["rdl"] < 0) >= 0.20 and sh(m["vdn"] < 0) >= 0.20
    assert sh(m["ndl"] > 1) == 0.0 and sh(m["rdl"] > 1) == 0.0                     # why the non-unit cases exist
    for tag, bar in (("nonunit", 0.04), ("highlight", 0.10)):
        m = uc.uv_intermediates(tag)
        print("%s: n.L>1 %.3f ref.L>1 %.3f" % (tag, sh(m["ndl"] > 1), sh(m["rdl"] > 1)))
        assert sh(m["ndl"] > 1) >= bar and sh(m["rdl"] > 1) >= bar, tag
    sp = uc.ggx_specular("highlight")
    over = sh(sp.nan_to_num(0.0) > 1)
    print("highlight: GGX specular>1 %.3f (max %.1f)" % (over, float(sp.nan_to_num(0.0).max())))
    assert over >= 0.10


@pytest.mark.parametrize("tag", uc.UV_TAGS)
def test_uv_reference_pair_is_usable(tag):
    """The GPU bar of a tensor is max(1e-4, 1.5 e_ref64), e_ref64 = the float32 oracle's rel-L2 from the float64 oracle over
    the elements where the float32 oracle is finite.  Measured e_ref64 (worst tensor of each case; all others below):
    tail_unit 2.3e-5 (ggx g_roughness), tail_nosh 7.4e-6, nonunit 7.5e-5 (ggx g_roughness), highlight 6.8e-5 (ggx
    g_p_uv), p0 7.3e-6, p1 8.4e-6, lowrough 1.4e-5, dark 0 (every tensor is exactly 0).  Non-finite share of the
    float32 oracle (0 * inf behind clamp(max=1), in the three GGX gradients that pass through specular^p): tail_unit
    0.0006, nonunit 0.0013, highlight 0.0019, none elsewhere."""
    o64, e = uc.uv_oracle(tag, torch.float64), uc.e_ref64(tag)
    assert set(o64) == set(uc.PHONG_KEYS + uc.GGX_KEYS)
    for k, v in o64.items():
        assert v.dtype == torch.float64 and bool(torch.isfinite(v).all()), (tag, k)
    print(tag, "e_ref64 / non-finite share of the float32 oracle:",
          "  ".join(f"{k} {a:.1e} / {b:.4f}" for k, (a, b) in e.items()))
    for k, (err, bad) in e.items():
        assert math.isfinite(err), (tag, k)
        assert bad <= 0.01, (tag, k, bad)
    if uc.UV[tag].get("dark"):
        assert all(not v.any() for v in o64.values()) and all(a == 0.0 for a, _ in e.values())
    else:
        assert all(float(v.abs().max()) > 0 for k, v in o64.items() if v.numel())
    P = len(uc.UV[tag]["powers"])
    assert o64["phong/spec"].shape[1] == P and o64["ggx/feat"].shape[1] == 1 + P


def test_uvlight_power_domain_is_checked_before_anything_else():
    """Host-side argument check of goliath_amd.uvlight (no GPU involved): more than 4 powers, or a power below 1, is a
    ValueError that says why; inside the domain the call goes on to the next check (CPU tensors: there is no CPU path)."""
    from goliath_amd import _lib, uvlight

    t = uc.uv_inputs("p1")
    ph = lambda pw: uvlight.phong_features(t["p_uv"], t["nml"], t["cam_pos"], t["light_pos"], t["light_intensity"], None,
                                           spec_powers=pw)
    gg = lambda pw: uvlight.ggx_features(t["p_uv"], t["nml"], t["cam_pos"], t["light_pos"], t["light_intensity"],
                                         t["roughness"], t["tex_mean"], None, spec_powers=pw)
    for f in (ph, gg):
        with pytest.raises(ValueError, match="at most 4"):
            f((1, 2, 4, 8, 16))
        for bad in ((0,), (1, 0.5), (16, -1.0), (float("nan"),)):
            with pytest.raises(ValueError, match=">= 1.*infinite derivative"):
                f(bad)
        for good in ((), (1,), (1.0, 2.5, 16, 64)):
            with pytest.raises(_lib.GoliathHipError, match="no CPU path"):
                f(good)
