"""CPU: the host side of goliath_amd/lbs.py -- the Skeleton packing from the arrays of tests/golden/lbs_golden.npz (written
by tests/golden/make_lbs_golden.py from the reference's own LBSModule), the C-ABI marshallers against the header, the loud
errors, and, where the reference tree exists, `Skeleton.from_module` / `dropin.patch_lbs` against the real classes."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import npz_parts

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")
CASES = ["a", "b", "c", "d", "e"]
SOURCES = ("joint_parents", "joint_offset", "joint_rotation", "bind_state", "skin_indices", "skin_weights", "mesh_vertices",
           "transform", "transform_offsets")


@pytest.fixture(scope="module")
def G():
    return npz_parts.load(os.path.join(HERE, "golden", "lbs_golden.npz"))


def _skeleton(G, case, dev="cpu"):
    from goliath_amd import lbs

    return lbs.Skeleton(*(torch.from_numpy(np.ascontiguousarray(G[f"{case}/{k}"])).to(dev) for k in SOURCES))


@pytest.mark.parametrize("case", CASES)
def test_skeleton_packing(G, case):
    from goliath_amd import lbs

    sk = _skeleton(G, case)
    parents = G[f"{case}/joint_parents"].reshape(-1)
    idx, w = G[f"{case}/skin_indices"], G[f"{case}/skin_weights"]
    J, (V, K) = parents.size, idx.shape
    assert (sk.J, sk.V, sk.K, sk.P) == (J, V, K, G[f"{case}/transform"].shape[1])
    assert all(getattr(sk, k).dtype == torch.int32 for k in ("parents", "level_start", "level_joints", "child_start",
                                                             "child_slot", "jv_start", "jv_slot", "item_start", "ji_start"))
    assert sk.bind_inv.dtype == torch.float64 and sk.parents.tolist() == parents.tolist()
    # levels: every joint once, ascending inside a level, a child exactly one level below its parent
    ls, lj = sk.level_start.tolist(), sk.level_joints.tolist()
    assert ls[0] == 0 and ls[-1] == J and len(ls) == sk.L + 1 and sorted(lj) == list(range(J))
    level_of = {}
    for l in range(sk.L):
        run = lj[ls[l]:ls[l + 1]]
        assert run and run == sorted(run)
        level_of.update({j: l for j in run})
    for j, p in enumerate(parents.tolist()):
        assert level_of[j] == (level_of[p] + 1 if p >= 0 else 0)
    expect_depth = {"b": J, "c": 2, "d": 1}.get(case)
    assert expect_depth is None or sk.L == expect_depth
    # children CSR: every (joint, child) exactly once, ascending
    cs, ch = sk.child_start.tolist(), sk.child_slot.tolist()
    pairs = [(j, c) for j in range(J) for c in ch[cs[j]:cs[j + 1]]]
    assert pairs == sorted((int(p), j) for j, p in enumerate(parents.tolist()) if p >= 0)
    assert cs[0] == 0 and cs[-1] == len(ch) == int((parents >= 0).sum())
    # joint -> (vertex, slot): every slot of non-zero weight exactly once, under its joint, ascending; no padded slot
    js, sl = sk.jv_start.tolist(), sk.jv_slot.tolist()
    flat_i, flat_w = idx.reshape(-1), w.reshape(-1)
    assert sorted(sl) == np.flatnonzero(flat_w != 0).tolist() and sk.E == len(sl) == js[-1]
    for j in range(J):
        run = sl[js[j]:js[j + 1]]
        assert run == sorted(run) and all(flat_i[s] == j for s in run)
    # items: a joint's run in pieces of at most ITEM_ENTRIES, in order
    it, ji = sk.item_start.tolist(), sk.ji_start.tolist()
    assert len(it) == sk.I + 1 and it[-1] == sk.E and ji[0] == 0 and ji[-1] == sk.I
    for j in range(J):
        cuts = it[ji[j]:ji[j + 1]] + [js[j + 1]]
        n = js[j + 1] - js[j]
        assert ji[j + 1] - ji[j] == -(-n // lbs.ITEM_ENTRIES)
        if n:
            assert cuts[0] == js[j] and all(0 < b - a <= lbs.ITEM_ENTRIES for a, b in zip(cuts, cuts[1:]))
    if case == "e":   # one joint owns every vertex: longer than any item
        assert max(js[j + 1] - js[j] for j in range(J)) == V > lbs.ITEM_ENTRIES and sk.I > J
    # the bind inverse (bt, br, bs): br is the bind rotation's inverse and bs the scale's, exactly; bt is checked through
    # the matrices on the GPU (the stored quaternions are unit only to float32 rounding, so no exact identity holds for it)
    bind = torch.from_numpy(G[f"{case}/bind_state"]).reshape(J, 8).double()
    br, bs = sk.bind_inv[:, 3:7], sk.bind_inv[:, 7]
    one = torch.ones(J, dtype=torch.float64)
    assert torch.allclose(bs * bind[:, 7], one, rtol=0, atol=1e-14)
    q = bind[:, 3:7]
    assert torch.allclose((q * br * q.new_tensor([-1.0, -1.0, -1.0, 1.0])).sum(-1), one, rtol=0, atol=1e-14)
    assert torch.allclose(torch.linalg.cross(q[:, :3], br[:, :3]), torch.zeros(J, 3, dtype=torch.float64), atol=1e-14)


def test_zero_weight_slots_do_not_enter_the_packing(G):
    """Rewriting the index of every padded slot leaves the joint -> (vertex, slot) lists and the items as they were."""
    sk = _skeleton(G, "a")
    arrays = {k: torch.from_numpy(np.ascontiguousarray(G[f"a/{k}"])) for k in SOURCES}
    g = torch.Generator().manual_seed(1)
    pad = arrays["skin_weights"] == 0
    assert pad.any()
    arrays["skin_indices"] = torch.where(pad, torch.randint(0, sk.J, pad.shape, generator=g, dtype=torch.int32),
                                         arrays["skin_indices"])
    from goliath_amd import lbs

    other = lbs.Skeleton(*(arrays[k] for k in SOURCES))
    for k in ("jv_start", "jv_slot", "item_start", "ji_start"):
        assert torch.equal(getattr(sk, k), getattr(other, k)), k


@pytest.mark.parametrize("parents", [[-1, 2, 1], [0, 0, 1], [-1, 0, -2]])
def test_bad_parent_order_raises(G, parents):
    from goliath_amd import lbs

    J = len(parents)
    with pytest.raises(ValueError):
        lbs.Skeleton(torch.tensor(parents), torch.zeros(J, 3), torch.tensor([[0.0, 0.0, 0.0, 1.0]] * J),
                     torch.tensor([[0.0] * 6 + [1.0, 1.0]] * J)[None], torch.zeros(4, 2, dtype=torch.long),
                     torch.full((4, 2), 0.5), torch.zeros(4, 3), torch.zeros(7 * J, 5), torch.zeros(1, 7 * J))


def test_to_keeps_the_object_on_the_same_device(G):
    sk = _skeleton(G, "c")
    assert sk.to("cpu") is sk and sk.to(torch.device("cpu")) is sk


def _header():
    hdr = open(os.path.join(ROOT, "include", "goliath_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


@pytest.mark.parametrize("entry", ["gol_lbs_skeleton_fwd", "gol_lbs_skeleton_bwd", "gol_lbs_skin_fwd", "gol_lbs_skin_bwd"])
def test_lbs_marshallers_follow_the_header(entry, monkeypatch):
    """The marshaller of an entry passes exactly the parameters goliath_hip.h declares, in its order and with its C types
    (the library sets no argtypes: a miscounted or swapped list would reach a kernel as a garbage pointer)."""
    from goliath_amd import _lib, lbs

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(lbs, "_abi_" + entry[len("gol_"):])
    sig = inspect.signature(fn).parameters
    assert set(sig) == {n for _, n in params} - {"stream"}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in sig.values())
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "float": (ctypes.c_float, i + 0.5)}[ctype]
        if name == "stream":
            v = 0xBEEF
        else:
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(lbs, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


def test_math_header_derivatives_match_finite_differences(tmp_path):
    """goliath_amd/csrc/gol_lbs_math.h compiled for the host: every derivative of the skeleton backward against central
    differences (tests/lbs_math_fd.cpp).  Needs a host C++ compiler on the test machine: `c++` or `g++` where present,
    otherwise the hipcc the build itself uses; without any, the test fails (it does not skip)."""
    import shutil
    import subprocess

    from goliath_amd import build

    cxx = shutil.which("c++") or shutil.which("g++") or build.HIPCC
    exe = str(tmp_path / "lbs_math_fd")
    subprocess.run([cxx, "-O1", "-std=c++17", os.path.join(HERE, "lbs_math_fd.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.count("worst") == 6, r.stdout


def test_cpu_tensors_raise(G):
    from goliath_amd import _lib, lbs

    sk = _skeleton(G, "c")
    motion = torch.from_numpy(G["c/motion"])
    scales = torch.from_numpy(G["c/lbs_scale"])
    for fn in (lbs.skeleton_states, lbs.rigid_transforms, lbs.pose_vertices):
        with pytest.raises(_lib.GoliathHipError):
            fn(sk, motion, scales)
    with pytest.raises(TypeError):
        lbs.pose_vertices(object(), motion, scales)


# ---- against the real classes ----------------------------------------------------------------------------------------------
def _real_module(G, case):
    """The reference's LBSModule rebuilt from the golden's arrays (the constructor computes the bind state itself)."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import ref_stubs

    ref_stubs.install()
    import ca_code.utils.lbs as ref_lbs

    g = lambda k: G[f"{case}/{k}"]
    parents, idx, w = g("joint_parents").reshape(-1), g("skin_indices"), g("skin_weights")
    bones = [{"Name": f"joint{j}", "Parent": int(p), "PreRotation": g("joint_rotation")[j].tolist(),
              "TranslationOffset": g("joint_offset")[j].tolist()} for j, p in enumerate(parents)]
    pairs, offsets = [], [0]
    for v in range(idx.shape[0]):
        pairs += [[int(i), float(x)] for i, x in zip(idx[v], w[v]) if x != 0]
        offsets.append(len(pairs))
    V = idx.shape[0]
    model_json = {"Skeleton": {"Bones": bones},
                  "SkinnedModel": {"RestPositions": g("mesh_vertices").tolist(), "RestVertexNormals": [[0.0] * 3] * V,
                                   "SkinningWeights": pairs, "SkinningOffsets": offsets,
                                   "Faces": {"Indices": [0, 0, 0], "TextureIndices": [0, 0, 0]},
                                   "TextureCoordinates": [0.0, 0.0]}}
    NS = g("lbs_scale").shape[1]
    cfg = {"channel_names": ["tx", "ty", "tz", "rx", "ry", "rz", "sc"], "transform_offsets": g("transform_offsets").tolist(),
           "transform": g("transform").tolist(), "limits": [], "nr_scaling_params": NS,
           "nr_position_params": g("transform").shape[1] - NS}
    return ref_lbs, ref_lbs.LBSModule(model_json, cfg, g("template"), g("lbs_scale"), g("global_scaling").tolist())


@needs_ref
@pytest.mark.parametrize("case", ["a", "c"])
def test_from_module_on_the_real_class_reproduces_the_golden(G, case):
    from goliath_amd import lbs

    _, module = _real_module(G, case)
    assert np.array_equal(module.lbs_fn.bind_state.numpy(), G[f"{case}/bind_state"])
    got, want = lbs.Skeleton.from_module(module.lbs_fn), _skeleton(G, case)
    for k in lbs.Skeleton._TENSORS:
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    assert lbs.skeleton_of(module.lbs_fn) is lbs.skeleton_of(module.lbs_fn)          # cached on the module
    module.lbs_fn.joint_offset = module.lbs_fn.joint_offset.clone()                  # a replaced buffer: rebuilt
    assert isinstance(lbs.skeleton_of(module.lbs_fn), lbs.Skeleton)


@needs_ref
def test_patch_lbs_keeps_the_signatures(G):
    from goliath_amd import dropin

    ref_lbs, _ = _real_module(G, "d")
    params = lambda fn: [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]
    names = [(ref_lbs.LinearBlendSkinning, n) for n in ("forward", "compute_rigid_transforms",
                                                        "compute_rigid_transforms_matrix")]
    names += [(ref_lbs.LBSModule, n) for n in ("pose", "template_pose")]
    untouched = [(ref_lbs.LinearBlendSkinning, n) for n in ("unpose", "unskinning", "compute_root_rigid_transform")]
    old = {(c, n): getattr(c, n) for c, n in names + untouched}
    try:
        assert dropin.patch_lbs(ref_lbs) is ref_lbs
        first = {k: getattr(*k) for k in names}
        assert dropin.patch_lbs(ref_lbs) is ref_lbs                                  # idempotent
        for k in names:
            assert getattr(*k) is first[k] and getattr(*k) is not old[k]
            assert params(getattr(*k)) == params(old[k]), k
        for k in untouched:
            assert getattr(*k) is old[k]
    finally:
        for (c, n), fn in old.items():
            setattr(c, n, fn)
