"""GPU: the lbs operators (goliath_amd/lbs.py, csrc/lbs.hip) against the reference's own float64 results
(tests/golden/lbs_golden.npz, written by tests/golden/make_lbs_golden.py from ca_code/utils/lbs.py's LBSModule).

The bound of every comparison is test_gpu_uvgeom.py's: |HIP - fp64| <= 2 x |the reference's fp32 - fp64| (same fixture, same
views) + a floor of 4 eps32 x the magnitude of the quantity (max |fp64 value| over what is compared).  Nothing is excluded:
all joints, all vertices, all parameters.  Measured ratios (error / bound) are printed before each assertion and recorded in
DESIGN.md section 8.  Cases (see the generator): a random tree J = 23; b chain J = 70; c star with two roots; d J = 1;
e one joint owning every vertex."""
import os
import types

import numpy as np
import pytest
import torch

import npz_parts

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = float(np.finfo(np.float32).eps)
CASES = ["a", "b", "c", "d", "e"]
SOURCES = ("joint_parents", "joint_offset", "joint_rotation", "bind_state", "skin_indices", "skin_weights", "mesh_vertices",
           "transform", "transform_offsets")


@pytest.fixture(scope="module")
def G():
    return npz_parts.load(os.path.join(HERE, "golden", "lbs_golden.npz"))


def _t(a, dev="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_SKELETONS = {}


def _skeleton(G, case):
    from goliath_amd import lbs

    if case not in _SKELETONS:
        _SKELETONS[case] = lbs.Skeleton(*(_t(G[f"{case}/{k}"]) for k in SOURCES))
    return _SKELETONS[case]


def _inputs(G, case, B, grad=True):
    """motion, a [B,NS] scales leaf (lbs_scale expanded), verts_unposed; template, global_scaling."""
    motion = _t(G[f"{case}/motion"][:B]).requires_grad_(grad)
    scales = _t(G[f"{case}/lbs_scale"]).expand(B, -1).clone().requires_grad_(grad)
    unposed = _t(G[f"{case}/verts_unposed"][:B]).requires_grad_(grad)
    return motion, scales, unposed, _t(G[f"{case}/template"]), _t(G[f"{case}/global_scaling"])


def _check(name, got, ref32, ref64):
    """|got - ref64| <= 2 |ref32 - ref64| + 4 eps32 max|ref64| (max norms over everything passed: nothing left out)."""
    got, ref32, ref64 = (np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64)
                         for x in (got, ref32, ref64))
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    err, ref_err = np.abs(got - ref64).max(), np.abs(ref32 - ref64).max()
    bound = 2.0 * ref_err + 4.0 * EPS * np.abs(ref64).max()
    print(f"[lbs] {name}: |hip - fp64| = {err:.3e}, reference fp32's own = {ref_err:.3e}, bound = {bound:.3e}, "
          f"ratio = {err / bound:.3f}")
    assert np.isfinite(got).all(), name
    assert err <= bound, (name, err, bound)


def _ref(G, case, key, B):
    return G[f"ref32/{case}/{key}"][:B], G[f"ref64/{case}/{key}"][:B]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", CASES)
def test_skeleton_parity(G, case, B):
    from goliath_amd import lbs

    sk = _skeleton(G, case)
    for op, out_key, cot in ((lbs.skeleton_states, "states", "g_states"), (lbs.rigid_transforms, "mats", "g_mats")):
        motion, scales, *_ = _inputs(G, case, B)
        out = op(sk, motion, scales)
        (out * _t(G[f"{case}/{cot}"][:B])).sum().backward()
        _check(f"{case} B={B} {out_key}", out, *_ref(G, case, out_key, B))
        _check(f"{case} B={B} g_motion({out_key})", motion.grad, *_ref(G, case, f"g_motion_{out_key}", B))
        _check(f"{case} B={B} g_scales({out_key})", scales.grad, *_ref(G, case, f"g_scales_{out_key}", B))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", CASES)
def test_pose_vertices_parity(G, case, B):
    from goliath_amd import lbs

    sk = _skeleton(G, case)
    motion, scales, unposed, template, gs = _inputs(G, case, B)
    verts = lbs.pose_vertices(sk, motion, scales, unposed, template, gs)
    (verts * _t(G[f"{case}/g_verts"][:B])).sum().backward()
    _check(f"{case} B={B} verts", verts, *_ref(G, case, "verts", B))
    _check(f"{case} B={B} g_motion", motion.grad, *_ref(G, case, "g_motion", B))
    _check(f"{case} B={B} g_scales", scales.grad, *_ref(G, case, "g_scales", B))
    _check(f"{case} B={B} g_verts_unposed", unposed.grad, *_ref(G, case, "g_verts_unposed", B))
    # the two other call shapes of the reference: the rest mesh for every view with one [1,NS] row of scales
    # (LinearBlendSkinning.forward without verts_unposed), and LBSModule.template_pose
    one_row = _t(G[f"{case}/lbs_scale"])
    _check(f"{case} B={B} verts(rest mesh)", lbs.pose_vertices(sk, motion.detach(), one_row),
           *_ref(G, case, "verts_rest", B))
    _check(f"{case} B={B} verts(template)",
           lbs.pose_vertices(sk, motion.detach(), one_row, None, None, gs, rest_vertices=template),
           *_ref(G, case, "verts_template", B))


def test_one_row_of_scales_gets_the_summed_gradient(G):
    """scales as [1,NS] (what LBSModule.pose passes) and as its expansion: the gradient is the sum over the views."""
    from goliath_amd import lbs

    sk = _skeleton(G, "a")
    motion, scales, unposed, template, gs = _inputs(G, "a", 3)
    w = _t(G["a/g_verts"])
    (lbs.pose_vertices(sk, motion, scales, unposed, template, gs) * w).sum().backward()
    for shape in ("row", "expanded"):
        row = _t(G["a/lbs_scale"]).requires_grad_(True)
        s = row if shape == "row" else row.expand(3, -1)
        (lbs.pose_vertices(sk, motion.detach(), s, unposed.detach(), template, gs) * w).sum().backward()
        assert row.grad.shape == (1, sk.P - motion.shape[1])
        assert torch.equal(row.grad, scales.grad.sum(0, keepdim=True)), shape


def test_null_verts_unposed_is_the_rest_mesh_bitwise(G):
    from goliath_amd import lbs

    for case in ("a", "d"):
        sk = _skeleton(G, case)
        motion, scales, _, template, gs = _inputs(G, case, 3, grad=False)
        rest = sk.mesh_vertices[None].expand(3, -1, -1).contiguous()
        assert torch.equal(lbs.pose_vertices(sk, motion, scales), lbs.pose_vertices(sk, motion, scales, rest))
        assert torch.equal(lbs.pose_vertices(sk, motion, scales, None, template, gs),
                           lbs.pose_vertices(sk, motion, scales, rest, template, gs))


def _step(sk, G, case, B, which=("motion", "scales", "unposed")):
    """One forward + backward of pose_vertices with gradients required for `which`: (verts, {name: grad or None})."""
    from goliath_amd import lbs

    motion, scales, unposed, template, gs = _inputs(G, case, B, grad=False)
    leaves = {"motion": motion, "scales": scales, "unposed": unposed}
    for k in which:
        leaves[k].requires_grad_(True)
    verts = lbs.pose_vertices(sk, motion, scales, unposed, template, gs)
    if which:
        (verts * _t(G[f"{case}/g_verts"][:B])).sum().backward()
    return verts.detach(), {k: v.grad for k, v in leaves.items()}


def test_padded_slots_contribute_exactly_nothing(G):
    from goliath_amd import lbs

    sk = _skeleton(G, "a")
    arrays = {k: _t(G[f"a/{k}"]) for k in SOURCES}
    pad = arrays["skin_weights"] == 0
    assert pad.any() and (~pad).any()
    g = torch.Generator().manual_seed(2)
    arrays["skin_indices"] = torch.where(pad, torch.randint(0, sk.J, pad.shape, generator=g, dtype=torch.int32).cuda(),
                                         arrays["skin_indices"])
    assert not torch.equal(arrays["skin_indices"], _t(G["a/skin_indices"]))
    rewritten = lbs.Skeleton(*(arrays[k] for k in SOURCES))
    v0, g0 = _step(sk, G, "a", 3)
    v1, g1 = _step(rewritten, G, "a", 3)
    assert torch.equal(v0, v1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    # a vertex whose weights are all zero: a zero row, and no gradient to its unposed position
    arrays["skin_weights"] = arrays["skin_weights"].clone()
    arrays["skin_weights"][7] = 0.0
    v2, g2 = _step(lbs.Skeleton(*(arrays[k] for k in SOURCES)), G, "a", 3)
    assert (v2[:, 7] == 0).all() and (g2["unposed"][:, 7] == 0).all()
    keep = torch.arange(sk.V, device="cuda") != 7
    assert torch.equal(v2[:, keep], v0[:, keep]) and torch.isfinite(g2["motion"]).all()


@pytest.mark.parametrize("which", [("motion",), ("unposed",), (), ("scales",)])
def test_requires_grad_combinations(G, which):
    sk = _skeleton(G, "a")
    v_full, g_full = _step(sk, G, "a", 3)
    v, g = _step(sk, G, "a", 3, which)
    assert torch.equal(v, v_full)
    for k in g_full:
        if k in which:
            assert torch.equal(g[k], g_full[k]), k
        else:
            assert g[k] is None, k


def test_runs_are_bitwise_reproducible(G):
    for case in ("b", "e"):
        sk = _skeleton(G, case)
        v0, g0 = _step(sk, G, case, 3)
        v1, g1 = _step(sk, G, case, 3)
        assert torch.equal(v0, v1) and all(torch.equal(g0[k], g1[k]) for k in g0), case


@pytest.mark.parametrize("through", ["pose_vertices", "rigid_transforms"])
def test_training_step_captures_as_a_graph(G, through):
    """Forward + backward on one stream, captured once and replayed with changed poses and vertices; no host sync."""
    from goliath_amd import lbs

    case, B = "a", 3
    sk = _skeleton(G, case)
    motion, scales, unposed, template, gs = _inputs(G, case, B)
    w = _t(G[f"{case}/g_verts"]) if through == "pose_vertices" else _t(G[f"{case}/g_mats"])

    def step():
        if through == "pose_vertices":
            out = lbs.pose_vertices(sk, motion, scales, unposed, template, gs)
            grads = torch.autograd.grad((out * w).sum(), (motion, scales, unposed))
        else:
            out = lbs.rigid_transforms(sk, motion, scales)
            grads = torch.autograd.grad((out * w).sum(), (motion, scales))
        return (out,) + grads

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")       # a host sync inside the step raises
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    gen = torch.Generator().manual_seed(3)
    for i in range(3):
        with torch.no_grad():
            motion.add_((0.2 * torch.randn(motion.shape, generator=gen)).cuda())
            unposed.add_((0.01 * torch.randn(unposed.shape, generator=gen)).cuda())
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        for a, b in zip(got, step()):
            assert torch.equal(a, b), (through, i)             # bitwise: every sum has a fixed order


def test_second_backward_raises(G):
    from goliath_amd import lbs

    sk = _skeleton(G, "c")
    for fn in (lbs.skeleton_states, lbs.rigid_transforms, lbs.pose_vertices):
        motion, scales, *_ = _inputs(G, "c", 2)
        loss = fn(sk, motion, scales).sum()
        loss.backward()
        with pytest.raises(RuntimeError):
            loss.backward()


def test_wrong_shapes_raise(G):
    from goliath_amd import _lib, lbs

    sk = _skeleton(G, "c")
    motion, scales, unposed, *_ = _inputs(G, "c", 2, grad=False)
    with pytest.raises(_lib.GoliathHipError):
        lbs.pose_vertices(sk, motion[:, :-1], scales)
    with pytest.raises(_lib.GoliathHipError):
        lbs.pose_vertices(sk, motion, scales, unposed[:, :-1])
    with pytest.raises(_lib.GoliathHipError):
        lbs.pose_vertices(sk, motion, scales[:1].expand(3, -1))


# ---- through the drop-in ---------------------------------------------------------------------------------------------------
class ParameterTransform(torch.nn.Module):
    def __init__(self, transform, transform_offsets):
        super().__init__()
        self.register_buffer("transform", transform)
        self.register_buffer("transform_offsets", transform_offsets)


class LinearBlendSkinning(torch.nn.Module):
    """LinearBlendSkinning-shaped: the reference's buffer names, filled from the golden; the methods are placeholders that
    patch_lbs replaces (the reference itself is not on the GPU machine)."""

    def __init__(self, G, case):
        super().__init__()
        for k in SOURCES[:7]:
            a = _t(G[f"{case}/{k}"], "cpu")
            self.register_buffer(k, a.long() if a.dtype == torch.int32 else a)
        self.joint_parents = self.joint_parents.reshape(-1, 1)
        self.param_transform = ParameterTransform(_t(G[f"{case}/transform"], "cpu"), _t(G[f"{case}/transform_offsets"], "cpu"))

    def forward(self, poses, scales, verts_unposed=None):
        raise NotImplementedError

    compute_rigid_transforms = compute_rigid_transforms_matrix = forward


class LBSModule(torch.nn.Module):
    def __init__(self, G, case):
        super().__init__()
        self.lbs_fn = LinearBlendSkinning(G, case)
        self.register_buffer("lbs_scale", _t(G[f"{case}/lbs_scale"], "cpu"))
        self.register_buffer("lbs_template_verts", _t(G[f"{case}/template"], "cpu"))
        self.register_buffer("global_scaling", _t(G[f"{case}/global_scaling"], "cpu"))

    def pose(self, verts_unposed, motion, template=None):
        raise NotImplementedError

    def template_pose(self, motion):
        raise NotImplementedError


def test_module_through_patch_lbs(G):
    from goliath_amd import dropin, lbs

    case, B = "a", 3
    names = [(LinearBlendSkinning, n) for n in ("forward", "compute_rigid_transforms", "compute_rigid_transforms_matrix")]
    names += [(LBSModule, n) for n in ("pose", "template_pose")]
    old = {k: getattr(*k) for k in names}
    module = types.SimpleNamespace(LinearBlendSkinning=LinearBlendSkinning, LBSModule=LBSModule)
    sk = _skeleton(G, case)
    motion, scales, unposed, template, gs = _inputs(G, case, B, grad=False)
    row = _t(G[f"{case}/lbs_scale"])
    try:
        assert dropin.patch_lbs(module) is module and dropin.patch_lbs(module) is module
        m = LBSModule(G, case).cuda()
        built = lbs.skeleton_of(m.lbs_fn)
        for k in lbs.Skeleton._TENSORS:
            assert torch.equal(getattr(built, k), getattr(sk, k)), k
        u = unposed.clone().requires_grad_(True)
        mo = motion.clone().requires_grad_(True)
        posed = m.pose(u, mo)
        g_u, g_m = torch.autograd.grad((posed * _t(G[f"{case}/g_verts"])).sum(), (u, mo))
        v_ref, g_ref = _step(sk, G, case, B, ("motion", "unposed"))
        assert torch.equal(posed, v_ref) and torch.equal(g_u, g_ref["unposed"]) and torch.equal(g_m, g_ref["motion"])
        assert torch.equal(m.pose(unposed, motion, template=2.0 * template),
                           lbs.pose_vertices(sk, motion, row, unposed, 2.0 * template, gs))
        assert torch.equal(m.template_pose(motion),
                           lbs.pose_vertices(sk, motion, row, template[None].expand(B, -1, -1), None, gs))
        assert torch.equal(m.lbs_fn(motion, scales), lbs.pose_vertices(sk, motion, scales))
        assert torch.equal(m.lbs_fn(motion, scales, unposed), lbs.pose_vertices(sk, motion, scales, unposed))
        assert torch.equal(m.lbs_fn.compute_rigid_transforms_matrix(motion[:, :6], motion[:, 6:], scales),
                           lbs.rigid_transforms(sk, motion, scales))
        assert torch.equal(m.lbs_fn.compute_rigid_transforms(motion[:, :6], motion[:, 6:], scales),
                           lbs.skeleton_states(sk, motion, scales))
        assert lbs.skeleton_of(m.lbs_fn) is built                         # cached: nothing is packed per call
        keep = m.lbs_fn.joint_offset
        m.lbs_fn.joint_offset = keep.clone()                              # a replaced buffer: packed again
        assert lbs.skeleton_of(m.lbs_fn) is not built
    finally:
        for (c, n), fn in old.items():
            setattr(c, n, fn)
