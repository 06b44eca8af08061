"""GPU: the uvframes operator (goliath_amd/uvframes.py, csrc/uvframes.hip) against the reference's own float64 results
(tests/golden/uvframes_golden.partNN.npz, written by tests/golden/make_uvframes_golden.py from ca_code/utils/geom.py's
vert_normals / xyz2normals / compute_tbn_uv_given_normal in the order of ca_code/models/urhand.py:366-392, :467-486, :573-578).

The bound of every comparison is the project's own (tests/test_gpu_uvgeom.py): |HIP - fp64| <= 2 x |the reference's fp32 -
fp64| (same case, same views) + 4 eps32 x the magnitude of the quantity (1 for unit vectors, max |g_fp64| for a gradient).
Nothing is excluded.  Measured ratios (error / bound) are printed before each assertion and recorded in DESIGN.md section 8.

Measured on an MI355X, largest error / bound over the cases, mode A / mode B: frames 0.21 / 0.53, nml 0.16 / 0.45, viewout
0.20 / 0.46, g_verts 0.22 / 0.22, g_posmap 0.20 / 0.45, g_cam_pos 0.13 / 0.18; clamp cases 0.04-0.50."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import npz_parts
import uvframes_cases as cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = float(np.finfo(np.float32).eps)
OUTPUTS = ("nml", "viewout", "frames")
GRADS = ("g_verts", "g_posmap", "g_cam_pos")


@pytest.fixture(scope="module")
def G():
    return npz_parts.load(os.path.join(HERE, "golden", "uvframes_golden.npz"))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(geo on the GPU, topology, inputs on the GPU): built once per case, never modified."""
    from goliath_amd import uvframes

    geo, inp = cases.inputs(name)
    geo = geo.cuda()
    return geo, uvframes.UVFramesTopology(geo), {k: v.cuda() for k, v in inp.items()}, cases.checksum(inp)


def _run(name, mode_b, flip, views, want_frames=True):
    """The operator with backward against the case's cotangents: outputs and gradients."""
    from goliath_amd import uvframes

    geo, topo, inp, _ = _case(name)
    leaves = [inp[k][:views].clone().requires_grad_(True) for k in ("verts", "posmap", "cam_pos")]
    nml, viewout, frames = uvframes.uv_frames(leaves[0], topo, posmap=leaves[1], flip_normal=flip, cam_pos=leaves[2],
                                              want_frames=want_frames, normals_from_posmap=mode_b)
    loss = (nml * inp["g_nml"][:views]).sum() + (viewout * inp["g_viewout"][:views]).sum()
    if want_frames:
        loss = loss + (frames * inp["g_frames"][:views]).sum()
    grads = torch.autograd.grad(loss, leaves)
    return dict(nml=nml.detach(), viewout=viewout.detach(), frames=None if frames is None else frames.detach(),
                g_verts=grads[0], g_posmap=grads[1], g_cam_pos=grads[2])


def _bound_check(name, got, ref64, ref_err, scale):
    """|got - ref64| <= 2 ref_err + 4 eps32 scale, over everything passed."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    err = np.abs(got - np.asarray(ref64, dtype=np.float64)).max()
    bound = 2.0 * float(ref_err) + 4.0 * EPS * scale
    print(f"[uvframes] {name}: |hip - fp64| = {err:.3e}, reference fp32's own = {float(ref_err):.3e}, bound = {bound:.3e}, "
          f"ratio = {err / bound:.3f}")
    assert np.isfinite(got).all(), name
    assert err <= bound, (name, err, bound)


def _runs():
    return [(c, *r) for c in cases.CASES for r in cases.RUNS.get(c, cases.DEFAULT_RUNS)]


@pytest.mark.parametrize("name,run,mode_b,flip,views", _runs())
def test_parity_with_the_reference_in_float64(G, name, run, mode_b, flip, views):
    geo, topo, inp, chk = _case(name)
    assert chk == float(G[f"checksum/{name}"]), "the inputs are not the ones the golden was generated from"
    mask = topo.covered_mask()
    for nb in sorted({1, views}):           # B = 1 is the first view of the same fixture: views are independent
        res = _run(name, mode_b, flip, nb)
        key = f"{name}/{run}"
        f64 = G[f"ref64/{key}/frames"][:nb]
        tag = f"{key} B={nb}"
        _bound_check(f"frames {tag}", res["frames"][:, mask], f64, G[f"err32/{key}/frames/B{nb}"], 1.0)
        _bound_check(f"nml {tag}", res["nml"][:, :, mask], f64[:, :, 2].transpose(0, 2, 1), G[f"err32/{key}/nml/B{nb}"], 1.0)
        _bound_check(f"viewout {tag}", res["viewout"][:, :, mask], G[f"ref64/{key}/viewout"][:nb],
                     G[f"err32/{key}/viewout/B{nb}"], 1.0)
        for k in GRADS:
            g64 = G[f"ref64/{key}/{k}"][:nb]
            _bound_check(f"{k} {tag}", res[k], g64, G[f"err32/{key}/{k}/B{nb}"], float(np.abs(g64).max()))
        for k in OUTPUTS:                   # uncovered texels: exactly zero
            x = res[k] if k == "frames" else res[k].permute(0, 2, 3, 1)
            assert (x[:, ~mask] == 0).all(), k
        # the planar normal map IS the frames' third row, and the decoder's path (no frames tensor) gives the same bits
        assert torch.equal(res["nml"], res["frames"][:, :, :, 2].permute(0, 3, 1, 2))
        lean = _run(name, mode_b, flip, nb, want_frames=False)
        assert lean["frames"] is None and torch.equal(lean["nml"], res["nml"]) and torch.equal(lean["viewout"], res["viewout"])


def _dilate(m):
    return F.max_pool2d(m[None, None].float(), 3, stride=1, padding=1)[0, 0] > 0


def _grouped(G, key, k, got, groups):
    """One bound per group of elements that share a scale (boolean masks over the gradient's shape, together everything)."""
    r32, r64 = G[f"ref32/{key}/{k}"], G[f"ref64/{key}/{k}"]
    got = got.detach().cpu().numpy()
    total = np.zeros(r64.shape, bool)
    for gname, m in groups:
        m = np.broadcast_to(m, r64.shape)
        total |= m
        _bound_check(f"{key} {k} [{gname}]", got[m], r64[m], np.abs(np.float64(r32[m]) - r64[m]).max(),
                     float(np.abs(r64[m]).max()))
    assert total.all()


def test_clamps_zero_area_triangle_and_camera_on_a_texel(G):
    """clamp_a: |t0 raw| = 0 on face 40 (and with it |n x t0| = |b x n| = 0 there), cam_pos on texel (30, 30)."""
    geo, topo, inp, chk = _case("clamp_a")
    assert chk == float(G["checksum/clamp_a"])
    res = _run("clamp_a", False, False, 1)
    key, mask = "clamp_a/A0", topo.covered_mask()
    f64 = G[f"ref64/{key}/frames"]
    on_face = ((geo.face_index_image == cases.CLAMP_FACE) & mask)
    assert int(on_face.sum()) > 10 and (res["frames"][0, on_face][:, :2] == 0).all()      # t = b = 0 there, exactly
    r, c = cases.CLAMP_TEXEL
    assert (res["viewout"][0, :, r, c] == 0).all() and bool(mask[r, c])                   # v = 0 / 1e-12
    _bound_check("clamp_a frames", res["frames"][:, mask], f64, G[f"err32/{key}/frames/B1"], 1.0)
    _bound_check("clamp_a viewout", res["viewout"][:, :, mask], G[f"ref64/{key}/viewout"], G[f"err32/{key}/viewout/B1"], 1.0)
    vi = geo.vi.cpu().numpy()
    tri = np.zeros(topo.V, bool)
    tri[vi[cases.CLAMP_FACE]] = True
    ring = np.zeros(topo.V, bool)
    ring[vi[np.isin(vi, vi[cases.CLAMP_FACE]).any(1)].reshape(-1)] = True
    ring &= ~tri
    assert float(np.abs(G[f"ref64/{key}/g_verts"][0, tri]).max()) > 1e12
    _grouped(G, key, "g_verts", res["g_verts"],
             [("the collapsed triple", tri[None, :, None]), ("its one-ring", ring[None, :, None]),
              ("regular", ~(tri | ring)[None, :, None])])
    at = np.zeros((cases.S, cases.S), bool)
    at[r, c] = True
    assert float(np.abs(G[f"ref64/{key}/g_posmap"][0, :, r, c]).max()) > 1e10
    _grouped(G, key, "g_posmap", res["g_posmap"], [("the camera's texel", at[None, None]), ("regular", ~at[None, None])])
    _grouped(G, key, "g_cam_pos", res["g_cam_pos"], [("all", np.ones((1, 3), bool))])


def test_clamps_normal_parallel_to_tangent_and_flat_patch(G):
    """clamp_b: n x t0 = 0 on face 40, U x V = 0 on the zero patch of the position map."""
    geo, topo, inp, chk = _case("clamp_b")
    assert chk == float(G["checksum/clamp_b"])
    res = _run("clamp_b", True, True, 1)
    key, mask = "clamp_b/B1", topo.covered_mask()
    on_face = (geo.face_index_image == cases.CLAMP_FACE) & mask
    patch = torch.zeros_like(mask)
    patch[cases.ZERO_PATCH[0], cases.ZERO_PATCH[1]] = True
    assert int(on_face.sum()) > 10 and (res["frames"][0, on_face][:, :2] == 0).all()      # b = t = 0, n = (0, 0, 1) flipped
    inner = torch.zeros_like(mask)                     # (the patch's four corner texels see a non-zero U and V)
    inner[cases.ZERO_PATCH[0].start + 1:cases.ZERO_PATCH[0].stop - 1, cases.ZERO_PATCH[1].start + 1:cases.ZERO_PATCH[1].stop - 1] = True
    assert (res["frames"][0, inner] == 0).all() and bool(mask[patch].all())               # n = 0 / 1e-8
    _bound_check("clamp_b frames", res["frames"][:, mask], G[f"ref64/{key}/frames"], G[f"err32/{key}/frames/B1"], 1.0)
    _bound_check("clamp_b viewout", res["viewout"][:, :, mask], G[f"ref64/{key}/viewout"], G[f"err32/{key}/viewout/B1"], 1.0)
    tri = np.zeros(topo.V, bool)
    tri[geo.vi.cpu().numpy()[cases.CLAMP_FACE]] = True
    _grouped(G, key, "g_verts", res["g_verts"], [("the parallel triple", tri[None, :, None]), ("regular", ~tri[None, :, None])])
    near_patch, near_face = _dilate(patch).cpu().numpy(), _dilate(on_face).cpu().numpy()
    assert not (near_patch & near_face).any()
    _grouped(G, key, "g_posmap", res["g_posmap"],
             [("around the flat patch", near_patch[None, None]), ("around the parallel face", near_face[None, None]),
              ("regular", ~(near_patch | near_face)[None, None])])
    _grouped(G, key, "g_cam_pos", res["g_cam_pos"], [("all", np.ones((1, 3), bool))])


def test_negative_tiny_fin_loses_its_sign():
    """seam: the triple (3, 4, 12) has fin = -3e-9, which becomes +1e-8 (geom.py:453); parity is in the `seam` runs above."""
    geo, topo, _, _ = _case("seam")
    tid = int((topo.geo.triples == torch.tensor([3, 4, 12], device="cuda", dtype=torch.int32)).all(-1).nonzero()[0])
    assert float(topo.tri_const[tid, 0]) == float(np.float32(1.0) / np.float32(1e-8))


@pytest.mark.parametrize("mode_b", [False, True])
def test_poisoned_buffers_come_back_fully_written(mode_b):
    """Through the ABI marshallers: every output and every gradient element is written, uncovered texels with exact 0."""
    from goliath_amd import uvframes

    geo, topo, inp, _ = _case("impaint" if not mode_b else "dome")
    g, n = topo.geo, topo.nrm
    B, V, S = 2 if not mode_b else 3, topo.V, topo.S
    B = min(B, inp["verts"].shape[0])
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    mode = int(mode_b)
    verts, posmap, cam = inp["verts"][:B].contiguous(), inp["posmap"][:B].contiguous(), inp["cam_pos"][:B].contiguous()
    vn, t0, nml, viewout, frames = nan(B, V, 3), nan(B, g.T, 3), nan(B, 3, S, S), nan(B, 3, S, S), nan(B, S, S, 3, 3)
    args = uvframes._topology_args(topo)
    uvframes._abi_uvframes_fwd(B=B, V=V, F=g.F, S=S, T=g.T, Tn=n.T, mode=mode, flip_normal=1, verts=verts, posmap=posmap,
                               cam_pos=cam, vn=vn if not mode_b else None, t0=t0, nml=nml, viewout=viewout, frames=frames,
                               **args)
    scratch = nan(uvframes._abi_uvframes_bwd_scratch_floats(B=B, V=V, S=S, T=g.T, I=g.I, In=n.I, mode=mode))
    g_verts, g_posmap, g_cam = nan(B, V, 3), nan(B, 3, S, S), nan(B, 3)
    uvframes._abi_uvframes_bwd(B=B, V=V, F=g.F, S=S, T=g.T, Tn=n.T, I=g.I, In=n.I, mode=mode, flip_normal=1, verts=verts,
                               item_start=g.item_start, texel_of=g.texel_of, tri_item_start=topo.tri_item_start,
                               vq_start=topo.vq_start, vq_slot=topo.vq_slot, nitem_start=n.item_start,
                               ntexel_of=n.texel_of, nvt_start=n.vt_start, nvt_slot=n.vt_slot, posmap=posmap, cam_pos=cam,
                               vn=vn if not mode_b else None, t0=t0, g_nml=inp["g_nml"][:B].contiguous(),
                               g_viewout=inp["g_viewout"][:B].contiguous(), g_frames=inp["g_frames"][:B].contiguous(),
                               scratch=scratch, g_verts=g_verts, g_posmap=g_posmap, g_cam_pos=g_cam, **args)
    for name, t in dict(t0=t0, nml=nml, viewout=viewout, frames=frames, g_verts=g_verts, g_posmap=g_posmap,
                        g_cam=g_cam).items():
        assert torch.isfinite(t).all(), name
    un = ~topo.covered_mask()
    if mode_b:
        assert un.any()
    assert (nml[:, :, un] == 0).all() and (viewout[:, :, un] == 0).all() and (frames[:, un] == 0).all()
    # ... and they are the autograd function's numbers
    res = _run("impaint" if not mode_b else "dome", mode_b, True, B)
    assert torch.equal(res["nml"], nml) and torch.equal(res["g_verts"], g_verts) and torch.equal(res["g_posmap"], g_posmap)
    assert torch.equal(res["g_cam_pos"], g_cam)


@pytest.mark.parametrize("name,mode_b", [("coarse", False), ("impaint", False), ("dome", True)])
def test_two_runs_are_bitwise_equal(name, mode_b):
    a = _run(name, mode_b, True, cases.n_views(name))
    b = _run(name, mode_b, True, cases.n_views(name))
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mode_b", [False, True])
def test_training_step_captures_as_a_graph(mode_b):
    """forward -> weighted sum -> backward on one stream, captured once and replayed with changed inputs: the same bits."""
    from goliath_amd import uvframes

    geo, topo, inp, _ = _case("dome")
    static = [inp[k].clone().requires_grad_(True) for k in ("verts", "posmap", "cam_pos")]

    def step():
        nml, viewout, _ = uvframes.uv_frames(static[0], topo, posmap=static[1], flip_normal=mode_b, cam_pos=static[2],
                                             normals_from_posmap=mode_b)
        loss = (nml * inp["g_nml"]).sum() + (viewout * inp["g_viewout"]).sum()
        return (nml, viewout) + torch.autograd.grad(loss, static)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    gen = torch.Generator().manual_seed(3)
    for i in range(2):
        with torch.no_grad():
            for s, k in zip(static, ("verts", "posmap", "cam_pos")):
                s.copy_(inp[k] + (0.3 * (i + 1) * torch.randn(s.shape, generator=gen)).cuda())
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        for a, b in zip(got, step()):
            assert torch.equal(a, b), i


def test_shapes_and_devices_are_validated():
    from goliath_amd import _lib, uvframes

    geo, topo, inp, _ = _case("coarse")
    v, pm, cam = inp["verts"], inp["posmap"], inp["cam_pos"]
    for kw in (dict(posmap=pm[:, :2]), dict(posmap=pm.cpu()), dict(cam_pos=cam), dict(posmap=pm, cam_pos=cam[:, :2]),
               dict(normals_from_posmap=True)):
        with pytest.raises(_lib.GoliathHipError):
            uvframes.uv_frames(v, topo, **kw)
    with pytest.raises(_lib.GoliathHipError):
        uvframes.uv_frames(v[:, :5], topo)
    with pytest.raises(_lib.GoliathHipError):
        uvframes.uv_frames(v, topo.to("cpu"))
    nml, viewout, frames = uvframes.uv_frames(v, topo)
    assert nml.shape == (1, 3, 64, 64) and viewout is None and frames is None


def test_second_backward_raises():
    from goliath_amd import uvframes

    geo, topo, inp, _ = _case("coarse")
    x = inp["verts"].clone().requires_grad_(True)
    loss = uvframes.uv_frames(x, topo)[0].sum()
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()


# ---- through the drop-in ---------------------------------------------------------------------------------------------------
MODEL_KEYS = ("tex", "phys_tex", "diff_feature", "spec_feature", "diff_feature_raw", "spec_feature_raw", "shadow", "shadow_raw",
              "feature_normal", "verts_displaced", "displacement", "roughness", "id_pose_conv")


def _decoder(tag):
    import urhand_shaped as shaped

    gold = np.load(os.path.join(HERE, "golden", "urhand_model_golden.npz"))
    dec = shaped.ShapedConvTeacherDecoder(seed=0).cuda().train(tag == "train")
    dec.rl = shaped.ReplayRenderLayer(512, 512, [torch.from_numpy(gold[f"urhand_{tag}_depth{i}"]) for i in range(2)])
    inp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in shaped.urhand_inputs(B=1, L=2).items()}
    return gold, dec, inp


@pytest.mark.parametrize("tag", ["eval", "train"])
def test_decoder_through_patch_urhand_matches_the_reference_forward(tag):
    """The tags, keys and tolerances of tests/test_gpu_urhand_model.py (3e-5 relative L2 against the reference's own
    forward), with the decoder's frames, normal maps and view conditioning on the fused operator."""
    import types

    import urhand_shaped as shaped
    from goliath_amd import dropin, urhand
    from scenes import rel_l2

    gold, dec, inp = _decoder(tag)
    module = types.SimpleNamespace(ConvTeacherDecoder=shaped.ShapedConvTeacherDecoder, get_shadow_map=None)
    leaves = {k: inp[k].clone().requires_grad_(True) for k in ("verts_rec", "tex_mean")}
    try:
        dropin.patch_urhand(module, uv_frames=True)
        assert shaped.ShapedConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward_uv_frames
        res = dec(**{**inp, **leaves})
    finally:
        del shaped.ShapedConvTeacherDecoder.forward
    worst = {}
    for k in MODEL_KEYS:
        want = torch.from_numpy(gold[f"urhand_{tag}_{k}"])
        assert tuple(res[k].shape) == tuple(want.shape), (k, res[k].shape, want.shape)
        worst[k] = rel_l2(res[k].detach().cpu(), want)
    print("\nURHAND_MODEL uv_frames outputs", tag, {k: float("%.2e" % v) for k, v in worst.items()})
    for k in MODEL_KEYS:
        assert worst[k] < 3e-5, (k, worst[k])
    g = torch.Generator().manual_seed(5)
    loss = sum((res[k] * torch.randn(res[k].shape, generator=g).cuda()).sum() for k in ("tex", "phys_tex", "diff_feature_raw"))
    loss.backward()
    for k, v in leaves.items():
        e = rel_l2(v.grad.cpu(), torch.from_numpy(gold[f"urhand_{tag}_grad_{k}"]))
        worst["grad_" + k] = e
        assert e < 3e-5, (k, e)
    params = dict(dec.named_parameters())
    for n in ("global_scale", "global_albedo_scale", "geo_refiner.geo.weight", "texmod1.0.weight"):
        e = rel_l2(params[n].grad.cpu(), torch.from_numpy(gold[f"urhand_{tag}_grad_{n}"]))
        worst["grad_" + n] = e
        assert e < 3e-5, (n, e)
    print("\nURHAND_MODEL uv_frames", tag, {k: float("%.2e" % v) for k, v in worst.items()})
    assert "_gol_uv_frames_topology" in dec.__dict__          # packed once, cached on the decoder


def test_default_binding_is_the_parents_forward_bit_for_bit():
    """uv_frames=False binds goliath_amd.urhand.conv_teacher_decoder_forward, whose frames are the parent's ATen lines: the
    two normal maps (the outputs that depend on nothing but those lines and the run's own displacement) equal a
    restatement of the parent's lines bit for bit, and no topology is packed.  (The other outputs carry the decoder's
    convolutions, whose sums are not ordered from run to run.)"""
    import types

    import urhand_shaped as shaped
    from goliath_amd import dropin, urhand

    _, dec, inp = _decoder("eval")
    module = types.SimpleNamespace(ConvTeacherDecoder=shaped.ShapedConvTeacherDecoder, get_shadow_map=None)
    try:
        dropin.patch_urhand(module)
        assert shaped.ShapedConvTeacherDecoder.forward is urhand.conv_teacher_decoder_forward
        with torch.no_grad():
            res = dec(**inp)
    finally:
        del shaped.ShapedConvTeacherDecoder.forward
    with torch.no_grad():
        frames, _ = urhand._uv_frames(dec, shaped, inp["verts_rec"])
        assert torch.equal(res["feature_normal_raw"], urhand._normal_map(frames))
        frames2, _ = urhand._uv_frames(dec, shaped, res["verts_displaced"], normals_from=_displaced_map(dec, res, inp),
                                       flip_normal=True)
        assert torch.equal(res["feature_normal"], urhand._normal_map(frames2))
    assert "_gol_uv_frames_topology" not in dec.__dict__


def _displaced_map(dec, res, inp):
    p_uv = dec.geo_fn.to_uv(inp["verts_rec"])
    return p_uv + res["feature_normal_raw"] * res["displacement"]
