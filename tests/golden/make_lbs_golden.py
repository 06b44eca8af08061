"""Generate tests/golden/lbs_golden.npz by running the REFERENCE's own `LBSModule` / `LinearBlendSkinning`
(/root/reference/ca_code/utils/lbs.py) on the CPU, once in float32 and once on `module.double()` in float64, with backward
against fixed seeded cotangents.  Build container only (imports ca_code through tests/golden/ref_stubs.py).  Only numbers
are stored: skeleton arrays, inputs, cotangents, and results under `ref32/<case>/` and `ref64/<case>/`.

Every case builds the reference's module from a synthetic `model_json` / `lbs_config_dict` (the constructor computes the
bind state and packs the K = 8 influence slots itself: zero-weight slots keep index 0), with a non-uniform
`global_scaling`, non-zero `lbs_scale`, non-zero `transform_offsets` and translations on non-root joints.  B = 3 views (the
tests take B = 1 as the first view: views are independent).  Cases:
    a  random tree, J = 23, V = 300, 1-4 influences per vertex
    b  pure chain, J = 70 (more than one wave of joints, depth J), V = 64
    c  star with two roots, J = 9 (depth 1), V = 40
    d  J = 1, V = 17
    e  case a's skeleton with joint 5 among the influences of EVERY vertex (one joint's run longer than any item)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import npz_parts  # noqa: E402
import ref_stubs  # noqa: E402

ref_stubs.install()
from ca_code.utils.lbs import LBSModule  # noqa: E402

B, K = 3, 8
CASES = {   # parents: tree shape; NP / NS: pose / scale parameter counts; V: vertices; own: a joint every vertex carries
    "a": dict(tree="random", J=23, V=300, NP=40, NS=5, own=None),
    "b": dict(tree="chain", J=70, V=64, NP=30, NS=3, own=None),
    "c": dict(tree="star2", J=9, V=40, NP=12, NS=2, own=None),
    "d": dict(tree="single", J=1, V=17, NP=6, NS=1, own=None),
    "e": dict(tree="random", J=23, V=300, NP=40, NS=5, own=5),
}
SKELETON = ("joint_parents", "joint_offset", "joint_rotation", "bind_state", "skin_indices", "skin_weights",
            "mesh_vertices")


def parents_of(tree, J, g):
    if tree == "chain":
        return [-1] + list(range(J - 1))
    if tree == "star2":
        return [-1, -1] + [int(i % 2) for i in range(J - 2)]
    if tree == "single":
        return [-1]
    return [-1] + [int(torch.randint(0, j, (1,), generator=g)) for j in range(1, J)]


def build_module(cfg, g):
    J, V, NP, NS = cfg["J"], cfg["V"], cfg["NP"], cfg["NS"]
    chain = cfg["tree"] == "chain"
    parents = parents_of(cfg["tree"], J, g)
    rot = torch.nn.functional.normalize(torch.randn(J, 4, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 0.0, 1.0]), dim=-1)
    off = torch.randn(J, 3, generator=g) * (0.02 if chain else 0.08)
    bones = [{"Name": f"joint{j}", "Parent": parents[j], "PreRotation": rot[j].tolist(),
              "TranslationOffset": off[j].tolist()} for j in range(J)]
    rest = torch.randn(V, 3, generator=g) * 0.15
    n_inf = torch.randint(1, 5, (V,), generator=g)
    pairs, offsets = [], [0]
    for v in range(V):
        n = int(n_inf[v])
        ids = torch.randperm(J, generator=g)[:min(n, J)].tolist()
        if cfg["own"] is not None and cfg["own"] not in ids:
            ids[0] = cfg["own"]
        w = torch.rand(len(ids), generator=g) + 0.1
        w = w / w.sum()
        pairs += [[int(i), float(x)] for i, x in zip(ids, w)]
        offsets.append(len(pairs))
    model_json = {
        "Skeleton": {"Bones": bones},
        "SkinnedModel": {"RestPositions": rest.tolist(), "RestVertexNormals": torch.zeros(V, 3).tolist(),
                         "SkinningWeights": pairs, "SkinningOffsets": offsets,
                         "Faces": {"Indices": [0, 0, 0], "TextureIndices": [0, 0, 0]},
                         "TextureCoordinates": [0.0, 0.0]},
    }
    # parameter transform [7J, NP + NS]: about a third of the entries set; translations (non-root joints included) of a few
    # centimetres per unit parameter, angles of a few tenths of a radian, scale exponents of a few hundredths
    P = NP + NS
    row_gain = torch.tensor([0.03, 0.03, 0.03, 0.35, 0.35, 0.35, 0.04]) * (0.3 if chain else 1.0)
    T = torch.randn(7 * J, P, generator=g) * (torch.rand(7 * J, P, generator=g) < 0.35)
    T = T * row_gain.repeat(J)[:, None] / np.sqrt(0.35 * P) * 3.0
    T_off = torch.randn(1, 7 * J, generator=g) * row_gain.repeat(J)[None] * 0.5
    lbs_cfg = {"channel_names": ["tx", "ty", "tz", "rx", "ry", "rz", "sc"], "transform_offsets": T_off.tolist(),
               "transform": T.tolist(), "limits": [], "nr_scaling_params": NS, "nr_position_params": NP}
    template = torch.randn(V, 3, generator=g) * 0.01
    lbs_scale = torch.randn(1, NS, generator=g) * 0.5
    global_scaling = [10.0, 7.5, 12.5]
    return LBSModule(model_json, lbs_cfg, template.numpy(), lbs_scale.numpy(), global_scaling)


def run(module, dtype, x, cot):
    """The reference's lines in `dtype`; results as numpy arrays of that precision."""
    m = module.double() if dtype == torch.float64 else module
    f = lambda t: t.to(dtype)
    motion = f(x["motion"]).clone().requires_grad_(True)
    unposed = f(x["verts_unposed"]).clone().requires_grad_(True)
    verts = m.pose(unposed, motion)
    g_motion, g_unposed = torch.autograd.grad((verts * f(cot["g_verts"])).sum(), (motion, unposed))
    # the scales' gradient: the same lines with a [B, NS] leaf handed to lbs_fn directly
    scales = m.lbs_scale.expand(B, -1).clone().requires_grad_(True)
    verts_s = m.lbs_fn(f(x["motion"]), scales, f(x["verts_unposed"]) + m.lbs_template_verts) * m.global_scaling
    (g_scales,) = torch.autograd.grad((verts_s * f(cot["g_verts"])).sum(), scales)
    # the rigid transforms and the skeleton states, with their own pose / scale gradients
    gp, lp = motion[:, :6], motion[:, 6:]
    mats = m.lbs_fn.compute_rigid_transforms_matrix(gp, lp, scales)
    g_motion_mats, g_scales_mats = torch.autograd.grad((mats * f(cot["g_mats"])).sum(), (motion, scales))
    states = m.lbs_fn.compute_rigid_transforms(gp, lp, scales)
    g_motion_states, g_scales_states = torch.autograd.grad((states * f(cot["g_states"])).sum(), (motion, scales))
    rest = m.lbs_fn(f(x["motion"]), m.lbs_scale.expand(B, -1))                      # verts_unposed = None
    tpl = m.template_pose(f(x["motion"]))
    out = dict(verts=verts, g_motion=g_motion, g_verts_unposed=g_unposed, g_scales=g_scales, mats=mats, states=states,
               g_motion_mats=g_motion_mats, g_scales_mats=g_scales_mats, g_motion_states=g_motion_states,
               g_scales_states=g_scales_states, verts_rest=rest, verts_template=tpl)
    assert torch.equal(verts_s.detach(), verts.detach())
    return {k: v.detach().numpy() for k, v in out.items()}


def main():
    out = {}
    for name, cfg in CASES.items():
        g = torch.Generator().manual_seed(4100 + ord(name[0]) - (4 if name == "e" else 0))   # e shares a's seed
        module = build_module(cfg, g)
        fn = module.lbs_fn
        J, V, NP = cfg["J"], cfg["V"], cfg["NP"]
        x = {"motion": torch.randn(B, NP, generator=g), "verts_unposed": torch.randn(B, V, 3, generator=g) * 0.02}
        cot = {"g_verts": torch.randn(B, V, 3, generator=g), "g_mats": torch.randn(B, J, 3, 4, generator=g),
               "g_states": torch.randn(B, J, 8, generator=g)}
        for k in SKELETON:
            a = getattr(fn, k).numpy()
            out[f"{name}/{k}"] = a.astype(np.int32) if a.dtype == np.int64 else a
        out[f"{name}/transform"] = fn.param_transform.transform.numpy()
        out[f"{name}/transform_offsets"] = fn.param_transform.transform_offsets.numpy()
        out[f"{name}/lbs_scale"] = module.lbs_scale.numpy()
        out[f"{name}/template"] = module.lbs_template_verts.numpy()
        out[f"{name}/global_scaling"] = module.global_scaling.numpy().astype(np.float32)
        out.update({f"{name}/{k}": v.numpy() for k, v in {**x, **cot}.items()})
        r32 = run(module, torch.float32, x, cot)
        r64 = run(module, torch.float64, x, cot)
        out.update({f"ref32/{name}/{k}": v for k, v in r32.items()})
        out.update({f"ref64/{name}/{k}": v for k, v in r64.items()})
        w = out[f"{name}/skin_weights"]
        print(f"case {name}: J = {J}, V = {V}, influences per vertex {int((w > 0).sum(1).min())}-{int((w > 0).sum(1).max())}, "
              f"longest joint run {int(np.bincount(out[f'{name}/skin_indices'][w > 0], minlength=J).max())}")
        for k in r32:
            print(f"  {k:18s} max |fp64| = {np.abs(r64[k]).max():.3e}   fp32 - fp64 = "
                  f"{np.abs(r32[k].astype(np.float64) - r64[k]).max():.3e}")
    path = os.path.join(HERE, "lbs_golden.npz")
    np.savez_compressed(path, **out)
    written = [path] if os.path.getsize(path) < npz_parts.LIMIT else npz_parts.save(path, out)
    for p in written:
        print(p, os.path.getsize(p))


if __name__ == "__main__":
    main()
