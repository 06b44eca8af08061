"""lbs probe: a plain-torch composition of the reference's skeleton solve + skinning vs the fused HIP operators.

Synthetic skeletons (random trees, J in {23, 160}), V in {8192, 65536} vertices with 1-4 of K = 8 influences, B in {1, 8}.
Per-call medians over --reps passes after --warmup, timed with HIP events, of the forward and of forward + backward
(gradients to the pose and the unposed vertices) of  pose(verts_unposed, motion) = skinning(verts_unposed + template) *
global_scaling  for
  (a) torch: the math of ca_code/utils/lbs.py written for this probe with the reference's structure -- a Python loop over
      the joints that reads every parent index from the device buffer, quaternion products as stacked elementwise ops, the
      gathered [B,V,K,3,4] matrix tensor;
  (b) goliath_amd.lbs.pose_vertices (csrc/lbs.hip).
For each: the host syncs of one forward + backward (torch's sync debug mode, counted as warnings) and, for (b), the C-ABI
calls (the kernel launches are in profiles/lbs_kernel_stats.csv).  Prints one JSON line and writes it to --out.

    python tools/lbs_probe.py [--reps 9] [--warmup 3] [--out profiles/lbs_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from goliath_amd import _lib, build, lbs  # noqa: E402

K, NS = 8, 5


def qmul(q, r):
    qx, qy, qz, qw = q.unbind(-1)
    rx, ry, rz, rw = r.unbind(-1)
    return torch.stack([qx * rw + qy * rz - qz * ry + qw * rx, -qx * rz + qy * rw + qz * rx + qw * ry,
                        qx * ry - qy * rx + qz * rw + qw * rz, -qx * rx - qy * ry - qz * rz + qw * rw], -1)


def qrot(q, v):
    av = torch.linalg.cross(q[..., :3], v)
    return v + 2.0 * (av * q[..., 3:] + torch.linalg.cross(q[..., :3], av))


def from_xyz(r):
    h = r * r.new_tensor([-0.5, 0.5, 0.5])
    c, s = torch.cos(h), torch.sin(h)
    c0, c1, c2 = c.unbind(-1)
    s0, s1, s2 = s.unbind(-1)
    return torch.stack([-s0 * c1 * c2 - c0 * s1 * s2, c0 * s1 * c2 - s0 * c1 * s2, c0 * c1 * s2 + s0 * s1 * c2,
                        c0 * c1 * c2 - s0 * s1 * s2], -1)


def torch_states(params, joint_offset, joint_rotation, joint_parents):
    """solve_skeleton_state: one joint at a time, the parent index read from the device buffer (a host sync each)."""
    B = params.shape[0]
    jp = params.view(B, -1, 7)
    lt = jp[:, :, 0:3] + joint_offset[None]
    lr = qmul(joint_rotation[None].expand(B, -1, -1), from_xyz(jp[:, :, 3:6]))
    ls = torch.pow(torch.tensor([2.0], device=params.device), jp[:, :, 6:7])
    state = []
    for index, parent in enumerate(joint_parents):
        p = int(parent)
        if p != -1:
            ps = state[p]
            gr = qmul(ps[:, :, 3:7], lr[:, index, None])
            gt = qrot(ps[:, :, 3:7], lt[:, index, None] * ps[:, :, 7:8]) + ps[:, :, 0:3]
            state.append(torch.cat((gt, gr, ps[:, :, 7:8] * ls[:, index, None]), 2))
        else:
            state.append(torch.cat((lt[:, index], lr[:, index], ls[:, index]), 1).view(B, 1, 8))
    return torch.cat(state, 1)


def torch_matrices(bind, st):
    q = bind[:, :, 3:7]
    br = q * q.new_tensor([-1.0, -1.0, -1.0, 1.0]) * (q * q).sum(2, keepdim=True).reciprocal()
    bs = bind[:, :, 7:8].reciprocal()
    bt = qrot(br, -bind[:, :, 0:3]) * bs
    tr = qmul(st[:, :, 3:7], br.expand(st.shape[0], -1, -1))
    ts = st[:, :, 7:8] * bs
    tt = qrot(st[:, :, 3:7], bt * st[:, :, 7:8]) + st[:, :, 0:3]
    x, y, z, w = tr.unbind(-1)
    rows = [torch.stack((1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)), 2),
            torch.stack((2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)), 2),
            torch.stack((2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)), 2)]
    return torch.cat((torch.stack(rows, 2) * ts[..., None], tt[..., None]), 3)


class TorchLBS:
    def __init__(self, s):
        self.__dict__.update(s)

    def states(self, motion, scale):
        params = self.transform.mm(torch.cat((motion, scale), 1).t()).t() + self.transform_offsets
        return torch_states(params, self.joint_offset, self.joint_rotation, self.joint_parents)

    def pose(self, verts_unposed, motion):
        mat = torch_matrices(self.bind_state, self.states(motion, self.lbs_scale.expand(motion.shape[0], -1)))
        v = verts_unposed + self.template
        v4 = torch.cat((v, torch.ones_like(v[:, :, :1])), 2)[:, :, None, :, None]
        vs = torch.matmul(mat[:, self.skin_indices], v4)
        return (vs * self.skin_weights[None, :, :, None, None]).sum(2).squeeze(3) * self.global_scaling


def make_scene(J, V, seed):
    g = torch.Generator().manual_seed(seed)
    NP = min(3 * J + 6, 128)
    parents = torch.tensor([-1] + [int(torch.randint(0, j, (1,), generator=g)) for j in range(1, J)])
    rot = torch.nn.functional.normalize(torch.randn(J, 4, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 0.0, 1.0]), dim=-1)
    gain = torch.tensor([0.03, 0.03, 0.03, 0.35, 0.35, 0.35, 0.04]).repeat(J)[:, None]
    T = torch.randn(7 * J, NP + NS, generator=g) * (torch.rand(7 * J, NP + NS, generator=g) < 0.2) * gain / (NP ** 0.5) * 4.0
    n_inf = torch.randint(1, 5, (V, 1), generator=g)
    w = torch.rand(V, K, generator=g) + 0.1
    w = w * (torch.arange(K)[None] < n_inf)
    s = dict(joint_parents=parents[:, None], joint_offset=torch.randn(J, 3, generator=g) * 0.08, joint_rotation=rot,
             transform=T, transform_offsets=torch.randn(1, 7 * J, generator=g) * gain.t() * 0.5,
             skin_indices=torch.randint(0, J, (V, K), generator=g) * (w > 0), skin_weights=w / w.sum(1, keepdim=True),
             mesh_vertices=torch.randn(V, 3, generator=g) * 0.15, template=torch.randn(V, 3, generator=g) * 0.01,
             lbs_scale=torch.randn(1, NS, generator=g) * 0.5, global_scaling=torch.tensor([10.0, 7.5, 12.5]))
    s = {k: v.cuda() for k, v in s.items()}
    ref = TorchLBS(s)
    ref.bind_state = ref.states(torch.zeros(1, NP, device="cuda"), torch.zeros(1, NS, device="cuda"))
    return ref, NP, g


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def _host_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in caught)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbs_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lbs_probe needs a GPU: a timing without one says nothing")
    res = {"probe": "lbs", "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "K": K,
           "NS": NS, "reps": args.reps, "rows": []}
    for J in (23, 160):
        for V in (8192, 65536):
            ref, NP, g = make_scene(J, V, seed=J + V)
            skel = lbs.Skeleton(ref.joint_parents, ref.joint_offset, ref.joint_rotation, ref.bind_state, ref.skin_indices,
                                ref.skin_weights, ref.mesh_vertices, ref.transform, ref.transform_offsets)
            for B in (1, 8):
                motion = torch.randn(B, NP, generator=g).cuda().requires_grad_(True)
                unposed = (torch.randn(B, V, 3, generator=g) * 0.02).cuda().requires_grad_(True)
                w = torch.randn(B, V, 3, generator=g).cuda()
                fwd_a = lambda: ref.pose(unposed, motion)
                fwd_b = lambda: lbs.pose_vertices(skel, motion, ref.lbs_scale, unposed, ref.template, ref.global_scaling)
                both = lambda fwd: torch.autograd.grad(fwd(), (motion, unposed), w)
                row = {"B": B, "J": J, "V": V, "NP": NP, "levels": skel.L, "entries": skel.E, "items": skel.I}
                va, vb = fwd_a(), fwd_b()
                ga, gb = both(fwd_a), both(fwd_b)
                row["max_abs_diff"] = {"verts": float((va - vb).detach().abs().max()), "verts_max": float(va.abs().max()),
                                       "g_motion": float((ga[0] - gb[0]).abs().max()), "g_motion_max": float(ga[0].abs().max()),
                                       "g_verts": float((ga[1] - gb[1]).abs().max()), "g_verts_max": float(ga[1].abs().max())}
                del va, vb, ga, gb
                for name, fwd in (("torch", fwd_a), ("fused", fwd_b)):
                    row[f"{name}_fwd_ms"] = _median_ms(fwd, args.reps, args.warmup)
                    row[f"{name}_fwd_bwd_ms"] = _median_ms(lambda: both(fwd), args.reps, args.warmup)
                    row[f"{name}_host_syncs_fwd_bwd"] = _host_syncs(lambda: both(fwd))
                _lib.TIMING = []
                both(fwd_b)
                torch.cuda.synchronize()
                row["fused_abi_calls_fwd_bwd"] = [name for name, _, _ in _lib.TIMING]
                _lib.TIMING = None
                res["rows"].append(row)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
