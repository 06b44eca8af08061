"""uvgeom probe: the PyTorch operator sequence of the reference's mesh -> UV lines vs the fused HIP operators.

Scene: a UV map of 1024^2 texels, a grid mesh of (n+1)^2 vertices (n = 100: V = 10201, F = 20000) whose uv island covers
[0.1, 0.9]^2 (the layout of tests/urhand_shaped.py:FakeGeo, built here vectorised), a dome with 0.1 mm of noise (a tenth
of a cell),
B in {1, 8}.  Per-call medians over --reps passes after --warmup, timed with HIP events, of the forward (vertices
requiring grad, as in training) and of forward + backward of  postex = to_uv(verts), tn = normalize(to_uv(vn(verts)))  for
  (a) torch: boolean-mask gather / product / masked scatter and three scatter_add_ calls (the parent path of these lines),
  (b) goliath_amd.uvgeom.uv_geometry (csrc/uvgeom.hip),
and for (b) the forward and backward ABI calls by themselves against their algorithmic bytes (16 + 24 B per texel and
direction) as a fraction of 8 TB/s.  Prints one JSON line and writes it to --out.

    python tools/uvgeom_probe.py [--reps 9] [--warmup 3] [--out profiles/uvgeom_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from goliath_amd import _lib, build, uvgeom  # noqa: E402

S, N = 1024, 100
HBM = 8e12


def grid_topology(S, n):
    """vi[F,3], index_image[S,S,3], bary_image[S,S,3] of an (n+1)^2 grid whose cells map to [0.1, 0.9]^2 of the map."""
    i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    vid = lambda a, b: a * (n + 1) + b
    lower = torch.stack([vid(i, j), vid(i, j + 1), vid(i + 1, j)], -1)
    upper = torch.stack([vid(i + 1, j + 1), vid(i + 1, j), vid(i, j + 1)], -1)
    vi = torch.stack([lower, upper], 2).reshape(-1, 3)
    c = ((torch.arange(S, dtype=torch.float64) + 0.5) / S - 0.1) / 0.8 * n
    v, u = torch.meshgrid(c, c, indexing="ij")
    inside = (u >= 0) & (u < n) & (v >= 0) & (v < n)
    cj, ci = u.clamp(0, n - 1).floor().long(), v.clamp(0, n - 1).floor().long()
    fu, fv = u - cj, v - ci
    low = fu + fv <= 1.0
    face = 2 * (ci * n + cj) + (~low).long()
    w = torch.where(low[..., None], torch.stack([1 - fu - fv, fu, fv], -1), torch.stack([fu + fv - 1, 1 - fu, 1 - fv], -1))
    index_image = torch.where(inside[..., None], vi[face], torch.full_like(vi[face], -1))
    bary_image = torch.where(inside[..., None], w, torch.zeros_like(w)).float()
    return vi, index_image, bary_image


def torch_vert_normals(v, vi, eps=1e-5):
    p = v[:, vi]
    n = torch.cross(p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0], dim=-1)
    n = n / n.norm(dim=-1, keepdim=True).clamp(min=eps)
    n = n[:, :, None].expand(-1, -1, 3, -1).reshape(v.shape[0], -1, 3)
    flat = vi.reshape(1, -1).expand(v.shape[0], -1)
    out = torch.zeros_like(v)
    for k in range(3):
        out[..., k].scatter_add_(1, flat, n[..., k])
    return out / out.norm(dim=-1, keepdim=True).clamp(min=eps)


def torch_to_uv(values, index_image, bary_image):
    mask = (index_image != -1).all(-1)                     # boolean-mask indexing: nonzero + a host sync, twice
    flat = (values[:, index_image[mask]].permute(0, 3, 1, 2) * bary_image[mask]).sum(-1)
    out = torch.zeros(values.shape[0], values.shape[-1], *index_image.shape[:2], dtype=values.dtype, device=values.device)
    out[:, :, mask] = flat
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uvgeom_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uvgeom_probe needs a GPU: a timing without one says nothing")
    vi, idx, bary = (t.cuda() for t in grid_topology(S, N))
    topo = uvgeom.UVTopology(vi, idx, bary)
    t = torch.linspace(-1.0, 1.0, N + 1)
    gv, gu = torch.meshgrid(t, t, indexing="ij")
    dome = torch.stack([80.0 * gu, 100.0 * gv, -60.0 * (1.0 - 0.5 * (gu * gu + gv * gv))], -1).reshape(-1, 3)
    res = {"probe": "uvgeom", "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "S": S,
           "V": topo.V, "F": topo.F, "T": topo.T, "M": topo.M, "I": topo.I, "reps": args.reps, "rows": []}
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        verts = (dome[None] + 0.1 * torch.randn(B, topo.V, 3, generator=g)).cuda().requires_grad_(True)
        w_p, w_n = torch.randn(B, 3, S, S, generator=g).cuda(), torch.randn(B, 3, S, S, generator=g).cuda()

        def fwd_a():
            return torch_to_uv(verts, idx, bary), F.normalize(torch_to_uv(torch_vert_normals(verts, vi), idx, bary), dim=1)

        def fwd_b():
            return uvgeom.uv_geometry(verts, topo)

        def both(fwd):
            postex, tn = fwd()
            torch.autograd.grad([postex, tn], verts, [w_p, w_n])

        row = {"B": B}
        pa, na = fwd_a()
        pb, nb = fwd_b()
        ga = torch.autograd.grad([pa, na], verts, [w_p, w_n])[0]
        gb = torch.autograd.grad([pb, nb], verts, [w_p, w_n])[0]
        row["max_abs_diff"] = {"postex": float((pa - pb).detach().abs().max()), "tn": float((na - nb).detach().abs().max()),
                               "g_verts": float((ga - gb).abs().max()), "g_verts_max": float(ga.abs().max())}
        del pa, na, pb, nb, ga, gb
        for name, fwd in (("torch", fwd_a), ("fused", fwd_b)):
            row[f"{name}_fwd_ms"] = _median_ms(fwd, args.reps, args.warmup)
            row[f"{name}_fwd_bwd_ms"] = _median_ms(lambda: both(fwd), args.reps, args.warmup)
        # the two ABI calls of (b) by themselves
        _lib.TIMING = []
        for _ in range(args.reps):
            both(fwd_b)
        torch.cuda.synchronize()
        per = {}
        for name, e0, e1 in _lib.TIMING:
            per.setdefault(name, []).append(e0.elapsed_time(e1))
        _lib.TIMING = None
        bytes_dir = S * S * (16 + 24 * B)
        for name, ts in per.items():
            ms = statistics.median(ts)
            row[name] = {"ms": ms, "algorithmic_bytes": bytes_dir, "fraction_of_8TBs": bytes_dir / (ms * 1e-3) / HBM}
        res["rows"].append(row)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
