"""CPU: the edge scene of tests/project_cases.py is what tests/test_gpu_project_edges.py needs it to be -- a partition into
conditioning classes with enough Gaussians in each, float32 and float64 oracles that agree on every integer output -- and the
oracle wrappers keep their converted arguments alive."""
import pytest
import torch

import project_cases as pc
from oracle import cref, cref64


@pytest.mark.parametrize("cfg", [0, 1])
def test_every_gaussian_of_every_view_is_in_exactly_one_class(cfg):
    r = pc.reference(cfg)
    count = sum(m.to(torch.int32) for m in r["classes"].values())
    assert set(r["classes"]) == set(pc.CLASSES) and count.shape == (3, pc.N)
    assert bool((count == 1).all())
    # the classes mean what their names say (float64 quantities)
    f64, cl = r["f64"], r["classes"]
    tz = pc.camera_space(r["scene"])[..., 2]
    assert bool((tz[cl["culled"]] <= r["clip"]).all()) and bool((tz[~cl["culled"]] > r["clip"]).all())
    assert bool((f64["radii"][cl["culled"] | cl["no_tile"]] == 0).all())
    assert bool((f64["conics"][cl["no_tile"]].abs().sum(-1) > 0).all())      # written before the tile-area test
    visible = ~(cl["culled"] | cl["no_tile"])
    assert bool((f64["radii"][visible] > 0).all()) and bool((f64["tiles"][visible] > 0).all())
    assert bool(pc.fov_clamped(r["scene"])[cl["fov_clamped"]].all())
    for name in pc.VISIBLE_CLASSES[1:]:
        assert not bool(pc.fov_clamped(r["scene"])[cl[name]].any()), name


def test_every_judged_class_is_populated_in_some_configuration():
    counts = {name: [int(pc.reference(c)["classes"][name].sum()) for c in range(len(pc.CONFIGS))] for name in pc.CLASSES}
    print("\nPROJECT_EDGE_CLASSES", counts)
    for name, n in counts.items():
        assert max(n) >= pc.MIN_CLASS, (name, n)
    # three views that differ: the two close ones clamp and cull, the benign one does neither
    for c in range(len(pc.CONFIGS)):
        cl = pc.reference(c)["classes"]
        assert int(cl["fov_clamped"][0].sum()) >= pc.MIN_CLASS and int(cl["fov_clamped"][1].sum()) >= pc.MIN_CLASS
        assert int(cl["culled"][1].sum()) >= pc.MIN_CLASS
        assert int(cl["fov_clamped"][2].sum()) == 0 and int(cl["culled"][2].sum()) == 0
    k = pc.edge_scene()["intrins"]
    assert bool((k[:, 0] != k[:, 1]).all()) and bool((k[:, 2] != pc.W / 2).all()) and bool((k[:, 3] != pc.H / 2).all())
    q = pc.edge_scene()["quats"].norm(dim=-1)
    assert float(q.min()) < 0.3 and float(q.max()) > 3.0
    assert pc.N % 256 != 0      # a partial last workgroup


@pytest.mark.parametrize("cfg", [0, 1])
def test_float32_and_float64_oracles_agree_on_radii_and_tile_counts(cfg):
    r = pc.reference(cfg)
    assert torch.equal(r["f32"]["radii"], r["f64"]["radii"])
    assert torch.equal(r["f32"]["tiles"], r["f64"]["tiles"])


def test_constructed_rows_are_what_they_claim():
    c = pc.constructed_rows()
    f32, f64 = (pc.oracle_fwd(c, c["glob_scale"], c["clip"], fp64) for fp64 in (False, True))
    assert torch.equal(f32["radii"], f64["radii"]) and torch.equal(f32["tiles"], f64["tiles"])
    rad, tiles, xys = f32["radii"][0], f32["tiles"][0], f32["xys"][0]
    assert float(c["means"][0, 0, 2]) == c["clip"] and float(c["means"][0, 1, 2]) > c["clip"]
    assert float(c["means"][0, 1, 2]) - c["clip"] < 1e-7
    assert int(rad[0]) == 0 and int(tiles[0]) == 0 and not bool(f32["conics"][0, 0].any())      # z == clip: culled
    assert int(rad[1]) > 0 and int(tiles[1]) > 0                                                 # one ulp further: kept
    all_tiles = ((pc.H + pc.BLOCK - 1) // pc.BLOCK) * ((pc.W + pc.BLOCK - 1) // pc.BLOCK)
    assert int(rad[2]) > max(pc.H, pc.W) and int(tiles[2]) == all_tiles                          # scale 500: every tile
    assert float(xys[3, 0]) < 0.0 and float(xys[3, 0]) + int(rad[3]) > pc.BLOCK and 0 < int(tiles[3]) < all_tiles
    assert bool((rad[4:] > 0).all())


def test_oracle_wrappers_keep_converted_arguments_alive():
    """project_bwd converts what it is given to its own precision: the converted copies must live until the C call returns.
    float32 arguments and the same values in float64 give the same answer, bit for bit."""
    r = pc.reference(0)
    scene, up = r["scene"], r["up"]
    b = 1
    fx, fy = float(scene["intrins"][b, 0]), float(scene["intrins"][b, 1])
    geo = (scene["means"][b], scene["scales"][b], r["glob_scale"], scene["quats"][b], scene["viewmats"][b], fx, fy)
    fw32 = [r["f32"][k][b] for k in ("cov3d", "radii", "conics", "comp")]
    g32 = [up[k][b] for k in ("v_xy", "v_depth", "v_conic", "v_comp")]
    as64 = lambda ts: [t if t.dtype == torch.int32 else t.double() for t in ts]
    # float32 values into the float64 oracle: every argument is converted
    want = cref64.project_bwd(*geo, *as64(fw32), *as64(g32))
    got = cref64.project_bwd(*geo, *fw32, *g32)
    for a, w in zip(got, want):
        assert torch.equal(a, w) and bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0
    # and float64 values into the float32 oracle
    want = cref.project_gaussians_backward(*geo, *fw32, *g32)
    got = cref.project_gaussians_backward(*geo, *as64(fw32), *as64(g32))
    for a, w in zip(got, want):
        assert torch.equal(a, w) and bool(torch.isfinite(w).all())
    # int64 radii are converted, too
    got = cref64.project_bwd(*geo, fw32[0], fw32[1].long(), *fw32[2:], *g32)
    want = cref64.project_bwd(*geo, *as64(fw32), *as64(g32))
    for a, w in zip(got, want):
        assert torch.equal(a, w)
