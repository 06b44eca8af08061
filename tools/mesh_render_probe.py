"""Textured mesh render probe: meshraster.RenderLayer (PyTorch composition) vs FusedRenderLayer (csrc/meshrender.hip).

Scene: W x H = 2048 x 1334, C = 4, a 1024^2 texture, bench.py's hand stand-in (tests/scenes.icosphere(4), and (5), ~90 mm
radius with the same bumps) seen from 400 mm at focal 2000, B in {1, 4}.  Per-call medians over --reps passes after
--warmup, timed with HIP events, of the forward (leaves requiring grad, as in training) and of forward + backward with
edge_grad off and on.  For the fused layer the three new entries are also timed one by one (HIP events around each ABI
call) and set against their algorithmic bytes: fraction of 8 TB/s, and the float-atomic bytes against the ~1.3 TB/s
chip-wide atomic rate.  Prints one JSON line and writes it to --out.

    python tools/mesh_render_probe.py [--reps 7] [--warmup 2] [--out profiles/mesh_render_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from goliath_amd import _lib, build, meshraster  # noqa: E402
from scenes import icosphere  # noqa: E402

H, W, C, T = 1334, 2048, 4, 1024
HBM, ATOMIC = 8e12, 1.3e12


def _scene(subdiv, B):
    v, faces = icosphere(subdiv, radius=90.0)
    v = v * (1.0 + 0.08 * torch.sin(0.05 * v[:, :1] + 0.07 * v[:, 1:2]))
    g = torch.Generator().manual_seed(subdiv)
    vt = 0.5 + 0.45 * v[:, :2] / v[:, :2].abs().max()    # a uv atlas of about a texel per pixel
    K = torch.tensor([[2000.0, 0.0, W / 2.0], [0.0, 2000.0, H / 2.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    Rt = torch.cat([torch.eye(3), torch.tensor([[0.0], [0.0], [400.0]])], 1).repeat(B, 1, 1)
    tex = torch.rand(B, C, T, T, generator=g)
    return v[None].repeat(B, 1, 1).cuda(), faces, vt, K.cuda(), Rt.cuda(), tex.cuda()


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(statistics.median(times), 3)


def _entry_times(fn, reps):
    """median ms of each gol_mesh_render_* call of fn (HIP events around the ABI calls)."""
    per = {}
    for _ in range(reps):
        _lib.TIMING = []
        try:
            fn()
            torch.cuda.synchronize()
            for name, e0, e1 in _lib.TIMING:
                if name.startswith("gol_mesh_render"):
                    per.setdefault(name, []).append(e0.elapsed_time(e1))
        finally:
            _lib.TIMING = None
    return {k: round(statistics.median(v), 4) for k, v in per.items()}


def _bytes(B, hit, cand):
    """Algorithmic bytes of the three kernels (upstream gradient on render only; edges: the candidate pairs)."""
    npix = B * H * W
    fwd = npix * (4 + 12 + 8 + 4 * C + 4) + hit * 4 * C * 4
    bwd = npix * 4 + hit * (12 + 4 * C + 4 * C * 4 + 9 * 4)      # + the vertex records (L2-resident, not counted)
    bwd_atomic = hit * 4 * C * 4 + hit * 9 * 4                     # texture taps + vertex gradients before the wave sums
    edge = npix * 12 + cand * (2 * 4 * C * 2 + 8 + 4 * 4)
    return dict(gol_mesh_render_fwd=(fwd, 0), gol_mesh_render_bwd=(bwd, bwd_atomic),
                gol_mesh_render_edge_bwd=(edge, cand * 4 * 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_render_probe.json"))
    a = ap.parse_args()
    rows = []
    for subdiv in (4, 5):
        for B in (1, 4):
            verts, faces, vt, K, Rt, tex = _scene(subdiv, B)
            up = torch.randn(B, C, H, W, device="cuda")
            row = dict(mesh=f"icosphere({subdiv})", V=int(verts.shape[1]), F=int(faces.shape[0]), B=B)
            fns = {}
            for name, cls in (("RenderLayer", meshraster.RenderLayer), ("FusedRenderLayer", meshraster.FusedRenderLayer)):
                layer = cls(H, W, faces, vt, faces).cuda()
                vg, tg = verts.clone().requires_grad_(True), tex.clone().requires_grad_(True)

                def fwd(layer=layer, vg=vg, tg=tg):
                    return layer(vg, tg, K, Rt, edge_grad=False)

                def fwd_bwd(edge, layer=layer, vg=vg, tg=tg):
                    vg.grad, tg.grad = None, None
                    (layer(vg, tg, K, Rt, edge_grad=edge)["render"] * up).sum().backward()

                row[name] = dict(fwd_ms=_median_ms(fwd, a.reps, a.warmup),
                                 fwd_bwd_ms=_median_ms(lambda: fwd_bwd(False), a.reps, a.warmup),
                                 fwd_bwd_edge_ms=_median_ms(lambda: fwd_bwd(True), a.reps, a.warmup))
                fns[name] = (fwd, fwd_bwd)
            for k in ("fwd_ms", "fwd_bwd_ms", "fwd_bwd_edge_ms"):
                row["speedup_" + k[:-3]] = round(row["RenderLayer"][k] / row["FusedRenderLayer"][k], 2)
            out = fns["FusedRenderLayer"][0]()
            idx = out["index_img"]
            hit = int((idx >= 0).sum())
            cand = int((idx[:, :, 1:] != idx[:, :, :-1]).sum() + (idx[:, 1:] != idx[:, :-1]).sum())
            row.update(hit_pixels=hit, candidate_pairs=cand)
            kt = _entry_times(lambda: fns["FusedRenderLayer"][1](True), a.reps)
            kern = {}
            for name, (nbytes, abytes) in _bytes(B, hit, cand).items():
                ms = kt.get(name)
                kern[name] = dict(ms=ms, bytes=nbytes, hbm_fraction=round(nbytes / (ms * 1e-3) / HBM, 3) if ms else None,
                                  atomic_bytes=abytes,
                                  atomic_fraction=round(abytes / (ms * 1e-3) / ATOMIC, 3) if ms and abytes else None)
            row["fused_kernels"] = kern
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
    res = dict(probe="mesh_render", H=H, W=W, C=C, tex=T, reps=a.reps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), source_digest=build.source_digest(), rows=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
