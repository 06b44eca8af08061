"""GPU: the shading tail (goliath_amd/csrc/shade.hip, forward and backward) at its clamps, poles, seam and sharp lobes,
judged by float64.

The scene (tests/shade_cases.py; tests/test_shade_cases.py checks it on the CPU) populates both sides of every branch of
the kernel.  A whole-tensor rel-L2 there is the conditioning noise of the sharp lobes and of the near-pole rows, so HIP is
compared with the float64 run of oracle/shade_ref.py PER CLASS of (view, Gaussian) and held to the project's rule
(test_gpu_project_edges.py / test_gpu_lbs.py / test_gpu_uvgeom.py):

    rel-L2(HIP, float64)  <=  2 x rel-L2(float32 oracle, float64)  +  4 eps32          over the same members.

(view, Gaussian) pairs at which float32 and float64 may legitimately take different branches (a lookup coordinate within
1e-4 px of a texel edge, the u = +-1 seam, an integer mip level, a clamp threshold, a lobe cosine within float32 rounding of
+-1) are left out; the exclusion is capped at 1 % of the pairs and 10 % of a class (test_shade_cases.py).  In the `sharp` and
`aligned` classes -- and only there -- a figure that misses the factor 2 is held, with the same factor, to the oracle's
EXPECTED error (shade_cases.conditioning: root mean square over 8 copies of the scene moved by one float32 rounding); both
ratios are recorded.  Every figure is printed as SHADE_PARITY and written to shade_parity.json in the report directory."""
import functools
import json
import os

import pytest
import torch

import shade_cases as sc

pytestmark = pytest.mark.gpu

_PARITY = {}


def _write_parity():
    import bench

    out_dir = os.path.dirname(bench.DETAIL_PATH)
    if os.path.isdir(out_dir):
        json.dump(_PARITY, open(os.path.join(out_dir, "shade_parity.json"), "w"), indent=1)


def _hip_run(s, env, n, ups, rand=True, coefs=(sc.NCOL, sc.NMONO)):
    """shade.shading_tail_coefs on the first n Gaussians of scene `s`, backward of sum(out[k] * ups[k]) (ups may be None:
    forward only).  Returns (outputs, leaf gradients) on the CPU in the oracle's shapes."""
    from goliath_amd import shade

    leaf = {k: s[k][:, :, :n].contiguous().cuda().requires_grad_(ups is not None) for k in ("f_vnocond", "f_vcond", "postex", "tn")}
    leaf["albedo"] = s["albedo"][:, :n].contiguous().cuda().requires_grad_(ups is not None)
    kw = (dict(preconv_envmap=[m.cuda() for m in s["mips"]], lightrot=s["rot"].cuda()) if env else
          dict(light_intensity=s["light_intensity"].cuda(), headrel_light_pos=s["light_pos"].cuda(), n_lights=s["n_lights"].cuda()))
    if rand:
        kw["light_sh_rand"] = s["light_sh_rand"].cuda()
    out = shade.shading_tail_coefs(leaf["f_vnocond"], leaf["f_vcond"], leaf["postex"], leaf["tn"], leaf["albedo"],
                                   s["light_sh"].cuda(), s["campos"].cuda(), coefs[0], coefs[1], **kw)
    grads = None
    if ups is not None:
        sum((out[k] * ups[k][:, :n].cuda()).sum() for k in out if k in ups).backward()
        grads = {k: v.grad.cpu() for k, v in leaf.items()}
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}, grads


@functools.lru_cache(maxsize=None)
def _hip(env, n):
    """One forward and one backward launch per (mode, N) with the dense upstream gradients, shared by the tests."""
    return sc.quantities(*_hip_run(sc.scene(), env, n, sc.upstream()))


def _judge(tag, hip, q32, q64, items, conditioning=None):
    """The rule of the module docstring for every (class, quantity) of `items` = [(class, mask, quantity names)]; prints and
    records every figure, then asserts.  conditioning() -> {(class, quantity): expected oracle error}, asked only when a
    figure of a class in shade_cases.FALLBACK_CLASSES misses the factor 2."""
    rec, bad, cond = {}, [], None
    for cname, mask, names in items:
        n = int(mask.sum())
        for o in names:
            if o not in hip:
                continue
            cut = lambda t: t[:, :mask.shape[1]]
            e_hip, e_32 = sc.class_rel_l2(hip[o], cut(q64[o]), mask), sc.class_rel_l2(cut(q32[o]), cut(q64[o]), mask)
            ratio = e_hip / (e_32 + 2.0 * sc.EPS32)          # the rule: ratio <= 2
            rec[f"{cname}/{o}"] = dict(n=n, hip=e_hip, oracle32=e_32, ratio=ratio)
            line = f"SHADE_PARITY {tag} {cname:>12s} {o:>17s} n={n:5d} hip={e_hip:.2e} oracle32={e_32:.2e} ratio={ratio:.2f}"
            if not e_hip <= 2.0 * e_32 + 4.0 * sc.EPS32:
                if conditioning is not None and cname in sc.FALLBACK_CLASSES:
                    cond = cond or conditioning()
                    e_c = cond[(cname, o)]
                    rec[f"{cname}/{o}"].update(oracle32_expected=e_c, ratio_expected=e_hip / (e_c + 2.0 * sc.EPS32))
                    line += f"  -> expected oracle32={e_c:.2e} ratio={e_hip / (e_c + 2.0 * sc.EPS32):.2f}"
                    if not e_hip <= 2.0 * e_c + 4.0 * sc.EPS32:
                        bad.append((cname, o, n, e_hip, e_32, e_c))
                else:
                    bad.append((cname, o, n, e_hip, e_32))
            print(line)
    _PARITY[tag] = rec
    _write_parity()
    assert rec and not bad, (tag, bad)


@pytest.mark.parametrize("n", [sc.N, sc.N_ODD])   # 16-byte planes; scalar planes, the last lane three Gaussians short
@pytest.mark.parametrize("env", [True, False])
def test_every_class_against_float64(env, n):
    """Every output and every input gradient, dense upstream gradients of all 14 outputs, the RAND kernels.

    Measured on an MI355X: every ratio at or below 0.72 in both modes and at both N, none through the expected-error
    fallback.  The kernel forms the env direction in double and the lobe angle as atan2(|d x l|, d . l): `pole` spec_color
    0.05, g_tn 0.007; `sharp` spec_color 0.06; `aligned` at most 0.02.  With the direction carried in float and the angle as
    acos of the cosine (the kernel this test was first run on) `one_light` missed the rule -- color 2.13, spec_color 2.57 --
    and `pole` g_vis stood at 1.96."""
    ref, hip = sc.reference(env), _hip(env, n)
    print()
    for k, v in hip.items():
        assert bool(torch.isfinite(v).all()), k
    _judge(f"{'env' if env else 'sg'} N={n}", hip, ref["q32"], ref["q64"], sc.judged(ref, n), lambda: sc.conditioning(env))
    # the shared albedo's gradient, over the Gaussians no view excludes
    keep = ref["keep"][:, :n].all(0)[None]
    _judge(f"{'env' if env else 'sg'} N={n} albedo", hip, ref["q32"], ref["q64"], [("all_views", keep, ("g_albedo",))])


def test_polar_class_hip_beside_the_float32_oracle():
    """The kernel forms the polar angle as atan2(|r_xz|, r_y) where the oracle forms acos(r_y): recorded side by side over
    the `pole` class (within 2 pi / 16 of either pole, down to 2e-3 rad), on what the angle reaches."""
    ref, hip = sc.reference(True), _hip(True, sc.N)
    mask = ref["classes"]["pole"] & ref["keep"]
    rec = {}
    print()
    for o in ("spec_color", "color", "g_tn", "g_dnml", "g_postex", "g_pos", "g_vis"):
        e_hip, e_32 = sc.class_rel_l2(hip[o], ref["q64"][o], mask), sc.class_rel_l2(ref["q32"][o], ref["q64"][o], mask)
        rec[o] = dict(hip=e_hip, oracle32=e_32, hip_below_oracle=e_hip < e_32)
        print(f"SHADE_POLE {o:>12s} n={int(mask.sum())} hip={e_hip:.2e} oracle32={e_32:.2e} hip/oracle32={e_hip / e_32:.3f}")
        assert e_hip <= 2.0 * e_32 + 4.0 * sc.EPS32, (o, e_hip, e_32)
    _PARITY["pole: HIP beside the float32 oracle"] = rec
    _write_parity()


@pytest.mark.parametrize("key", sc.OUT_KEYS)
@pytest.mark.parametrize("env", [True, False])
def test_one_upstream_gradient_at_a_time(env, key):
    """Each differentiable output alone (N = 1061): the input gradients pass the per-class rule, and wherever both oracles'
    gradient is exactly zero -- the output does not reach that input there: a clamp blocks it, or there is no path at all,
    e.g. sigma alone reaches only the roughness channel and only above the floor -- HIP's is exactly zero too.

    Measured on an MI355X: every ratio at or below 0.77.  With the env direction carried in float, `color` alone missed
    the rule in the `pole` class (g_vis 4.57, g_tn 2.77; 1.03 and 0.50 with spec_color alone: the figure of the two or three
    rows within a few mrad of a pole, whose azimuth float32 cannot resolve, moves by that much with the weights), and with
    the lobe angle as acos of the cosine in the `mid` class (g_pos 2.02)."""
    ref, n = sc.reference(env), sc.N_ODD
    ups = {key: ref["ups"][key]}
    q64 = sc.quantities(*sc.run_oracle(ref["scene"], torch.float64, env, ups))
    q32 = sc.quantities(*sc.run_oracle(ref["scene"], torch.float32, env, ups))
    hip = sc.quantities(*_hip_run(ref["scene"], env, n, ups))
    grads = sc.GRAD_KEYS + ("g_albedo",)
    keep = ref["keep"][:, :n]
    zeros = 0
    for o in grads:
        assert bool(torch.isfinite(hip[o]).all()), o
        m = keep.all(0)[None] if o == "g_albedo" else keep
        dead = (q64[o][:, :n] == 0) & (q32[o][:, :n] == 0) & m[..., None]
        zeros += int(dead.sum())
        assert not bool(hip[o][dead].any()), (o, int((hip[o][dead] != 0).sum()), int(dead.sum()))
    assert zeros > 0
    print()
    items = [(c, m, [o for o in qs if o in grads]) for c, m, qs in sc.judged(ref, n)]
    items.append(("all_views", keep.all(0)[None], ("g_albedo",)))
    _judge(f"{'env' if env else 'sg'} only {key}", {o: hip[o] for o in grads}, q32, q64, items,
           lambda: sc.conditioning(env, only=key))


@pytest.mark.parametrize("n", [sc.N, sc.N_ODD])
def test_zero_sh_block_gets_the_random_light_gradient(n):
    """Where the SH planes are exactly zero the random-light sum is exactly 0, and clamp(min=0) passes the gradient at 0
    (rgca.py:616, torch's clamp): with color_rand as the only upstream gradient the block's SH planes receive
    u_rand x light_sh_rand.  The kernel keeps only the clamped output and marks a clamped element by its sign bit."""
    s, ups = sc.scene(), {"color_rand": sc.upstream()["color_rand"]}
    lo, hi = sc.BLOCKS["zero_sh"]
    q64 = sc.quantities(*sc.run_oracle(s, torch.float64, False, ups))
    q32 = sc.quantities(*sc.run_oracle(s, torch.float32, False, ups))
    out, grads = _hip_run(s, False, n, ups)
    hip = sc.quantities(out, grads)
    assert not bool(out["color_rand"][:, lo:hi].any())                      # -0.0 == 0: the output's value is unchanged
    assert bool((out["color_rand"] >= 0).all())
    block = torch.zeros(sc.B, n, dtype=torch.bool)
    block[:, lo:hi] = True
    assert float(q64["g_sh"][:, :n][block].abs().min()) > 0
    print()
    _judge(f"zero_sh N={n} only color_rand", {"g_sh": hip["g_sh"]}, q32, q64,
           [("zero_sh", block, ("g_sh",)), ("elsewhere", ~block & sc.reference(False)["keep"][:, :n], ("g_sh",))])


@pytest.mark.parametrize("env", [True, False])
def test_degenerate_rows_are_finite_and_the_pole_guards_hold(env):
    """HIP only (shade_cases.degenerate_scene: these rows make torch's acos NaN and its grid_sample backward crash).  Every
    output and input gradient is finite; the forward agrees with the float64 evaluation that forms the polar angle as
    atan2(|r_xz|, r_y), by the rule against the same evaluation in float32; with spec_color as the only upstream gradient the
    rows whose reflection is exactly at a pole send exactly nothing to tn, f_vcond[1:4] and the position."""
    s = sc.degenerate_scene()
    g = torch.Generator().manual_seed(23)
    ups = {k: torch.randn(sc.B, sc.DEG, generator=g) if k == "sigma" else
           torch.randn(sc.B, sc.DEG, 4 if k == "primqvec" else 1 if k in ("opacity", "spec_vis") else 3, generator=g) for k in sc.OUT_KEYS}
    out, grads = _hip_run(s, env, sc.DEG, ups)
    for k, v in {**out, **grads}.items():
        assert bool(torch.isfinite(v).all()), k
    o64, o32 = sc.degenerate_forward(torch.float64, env), sc.degenerate_forward(torch.float32, env)
    rows = torch.zeros(sc.B, sc.DEG, dtype=torch.bool)
    rows[:, :12] = True
    print()
    _judge(f"degenerate {'env' if env else 'sg'} forward", sc.quantities(out, None), sc.quantities(o32, None),
           sc.quantities(o64, None), [("degenerate", rows, sc.OUT_KEYS)])
    if env:
        _, g1 = _hip_run(s, env, sc.DEG, {"spec_color": ups["spec_color"]})
        q = sc.quantities(out, g1)
        for row in (sc.DEG_ROWS["pole_up"], sc.DEG_ROWS["pole_down"]):
            for o in ("g_tn", "g_dnml", "g_postex", "g_pos"):
                assert not bool(q[o][:, row].any()), (row, o, q[o][:, row])
        assert bool(q["g_tn"][:, 12:].any())                                # the fillers do get a gradient


PYRAMIDS = {"one_level": ((8, 16),), "eight_levels": tuple((128 >> i, 256 >> i) for i in range(8))}


@pytest.mark.parametrize("records", [True, False])
@pytest.mark.parametrize("pyramid", sorted(PYRAMIDS))
def test_pyramid_depth_against_float64(pyramid, records, monkeypatch):
    """A single-level pyramid (the q == 1 paths of env_lookup) and GOL_MAX_MIPS = 8 levels down to a 1-row level, both lookup
    forms, N = 260: whole-tensor against float64 with the near-branch exclusion, by the rule."""
    monkeypatch.setenv("GOLIATH_ENVMAP_RECORDS", "1" if records else "0")
    n = 260
    ref = sc.small_reference(n, (sc.NCOL, sc.NMONO), PYRAMIDS[pyramid], True, True)
    keep = ref["keep"]
    assert int((~keep).sum()) <= 0.01 * keep.numel() + 1, int((~keep).sum())
    hip = sc.quantities(*_hip_run(ref["scene"], True, n, ref["ups"]))
    print()
    _judge(f"pyramid {pyramid} records={int(records)}", hip, ref["q32"], ref["q64"],
           [("kept", keep, sc.OUT_KEYS + sc.GRAD_KEYS), ("all_views", keep.all(0)[None], ("g_albedo",))])


@pytest.mark.parametrize("rand", [True, False])
@pytest.mark.parametrize("n", [259, 260])
@pytest.mark.parametrize("coefs", [(1, 0), (3, 2), (9, 0), (4, 5)])
def test_sh_layouts_against_float64(coefs, n, rand):
    """SH layouts other than 16 + 65 through shading_tail_coefs: waves with no plane to stream, a ragged k += 4, no mono
    block; scalar and 16-byte planes; with and without the random light.  Point lights, whole-tensor against float64 on what
    the layout reaches."""
    ref = sc.small_reference(n, coefs, sc.PYRAMID, False, rand, seed=1)
    hip = sc.quantities(*_hip_run(ref["scene"], False, n, ref["ups"], rand=rand, coefs=coefs), nd=3 * coefs[0] + coefs[1])
    names = ("diff_color", "opacity", "primpos", "primqvec", "primscale", "sigma", "g_sh", "g_quat", "g_scale", "g_opac") + (
        ("color_rand",) if rand else ())
    print()
    _judge(f"coefs={coefs} N={n} rand={int(rand)}", hip, ref["q32"], ref["q64"],
           [("kept", ref["keep"], names), ("all_views", ref["keep"].all(0)[None], ("g_albedo",))])
