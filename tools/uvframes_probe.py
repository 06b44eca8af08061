"""uvframes probe: the parent's `_uv_frames` + `_normal_map` + view-conditioning lines of goliath_amd/urhand.py against the
fused operator of goliath_amd/uvframes.py, and the share of a URHand decoder step that these lines take.

Scene: S = bench.py's URHand map size (1024), a grid mesh of (n+1)^2 vertices with n = 50 (2601 vertices, 5000 faces: the
size of the icosphere(4) bench.py's URHand workload builds, 2562 / 5120 -- that mesh has no uv map, so the uv layout is
tools/uvgeom_probe.py's grid island over [0.1, 0.9]^2), a dome with 0.1 mm of noise, B in {1, 8}.

What is timed, per B, forward and forward + backward, alternating parent and fused in ONE process on the same inputs, HIP
events, --warmup passes then --reps repeats of each:
    pass 1   frames / normal map of the LBS surface (interpolated vertex normals)          urhand.py:366-392
    pass 2   frames / normal map of the displaced surface (xyz2normals, flipped normal)    urhand.py:467-486
    view     frame . normalize(cam_pos - p_uv)                                             urhand.py:573-578
i.e. exactly what one decoder forward runs.  A row counts as faster only when the fused median is below the parent's median
by more than the parent's own run-to-run spread (max - min of its repeats).  Then one decoder forward + backward of
tests/urhand_shaped.py's stand-in (its small sub-modules, S = 1024, 8 lights, shadow maps off: the share printed is an upper
bound on the real model's) under patch_urhand() and patch_urhand(uv_frames=True).

    python tools/uvframes_probe.py [--reps 9] [--warmup 3] [--out profiles/uvframes_probe.json]
    python tools/uvframes_probe.py --kernels-only      # the fused passes alone, for a kernel trace in a run of its own
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
import urhand_shaped as shaped  # noqa: E402
from goliath_amd import build, dropin, urhand, uvframes  # noqa: E402
from scenes import icosphere  # noqa: E402
from uvgeom_probe import grid_topology  # noqa: E402

S = bench.URHAND_CFG["uv"]
HBM = 8e12


class Geo(torch.nn.Module):
    """GeometryModule-shaped: the buffers the frames read, to_uv / from_uv as tests/urhand_shaped.py:FakeGeo has them."""

    def __init__(self, S, n):
        super().__init__()
        vi, index_image, bary_image = grid_topology(S, n)
        t = torch.arange(n + 1, dtype=torch.float32) / n
        ii, jj = torch.meshgrid(t, t, indexing="ij")
        self.uv_size = S
        self.register_buffer("vt", torch.stack([0.1 + 0.8 * jj, 0.1 + 0.8 * ii], -1).reshape(-1, 2))
        self.register_buffer("vi", vi)
        self.register_buffer("v2uv", torch.arange((n + 1) ** 2)[:, None])
        self.register_buffer("index_image", index_image)
        # the face of a texel: the row of vi that equals its triple (grid_topology lists the two triangles of a cell in turn)
        c = ((torch.arange(S, dtype=torch.float64) + 0.5) / S - 0.1) / 0.8 * n
        v, u = torch.meshgrid(c, c, indexing="ij")
        cj, ci = u.clamp(0, n - 1).floor().long(), v.clamp(0, n - 1).floor().long()
        face = 2 * (ci * n + cj) + ((u - cj) + (v - ci) > 1.0).long()
        self.register_buffer("face_index_image", face)
        self.register_buffer("bary_image", bary_image)

    to_uv = shaped.FakeGeo.to_uv
    from_uv = shaped.FakeGeo.from_uv


class Pooled(torch.nn.Module):
    """The stand-in's feature encoder expects a 64^2 map (its gain / bias feed the 64^2 level of the texture branch)."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(F.adaptive_avg_pool2d(x, 64))


def _times(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def _alternate(a, b, reps, warmup):
    """reps timings of a and of b, taken in turn (a, b, a, b, ...) after `warmup` passes of each."""
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta += _times(a, 1)
        tb += _times(b, 1)
    return ta, tb


def _stat(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "spread_ms": max(ts) - min(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uvframes_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uvframes_probe needs a GPU: a timing without one says nothing")
    bench_verts, bench_faces = icosphere(4, radius=90.0)
    n = 50
    geo = Geo(S, n).cuda()
    holder = types.SimpleNamespace(geo_fn=geo)
    topo = uvframes.topology_of(holder)
    V = topo.V
    t = torch.linspace(-1.0, 1.0, n + 1)
    gv, gu = torch.meshgrid(t, t, indexing="ij")
    dome = torch.stack([80.0 * gu, 100.0 * gv, -60.0 * (1.0 - 0.5 * (gu * gu + gv * gv))], -1).reshape(-1, 3)
    res = {"probe": "uvframes", "device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "S": S,
           "V": V, "F": int(geo.vi.shape[0]), "bench_mesh": {"V": int(bench_verts.shape[0]), "F": int(bench_faces.shape[0])},
           "T": topo.T, "I": topo.geo.I, "reps": args.reps, "warmup": args.warmup, "rows": []}
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        verts = (dome[None] + 0.1 * torch.randn(B, V, 3, generator=g)).cuda().requires_grad_(True)
        verts2 = (verts.detach() + 0.05 * torch.randn(B, V, 3, generator=g).cuda()).requires_grad_(True)
        with torch.no_grad():
            p0 = geo.to_uv(verts2)
        bump = 0.05 * torch.randn(B, 3, S, S, generator=g).cuda()
        p_uv = (p0 + bump).requires_grad_(True)
        cam = (torch.tensor([[30.0, -40.0, 700.0]]).repeat(B, 1)).cuda()
        w1, w2, w3 = (torch.randn(B, 3, S, S, generator=g).cuda() for _ in range(3))
        leaves = [verts, verts2, p_uv]

        def parent():
            f1, _ = urhand._uv_frames(holder, shaped, verts)
            nml1 = urhand._normal_map(f1)
            f2, _ = urhand._uv_frames(holder, shaped, verts2, normals_from=p_uv, flip_normal=True)
            nml2 = urhand._normal_map(f2)
            v_uv = F.normalize(cam[..., None, None] - p_uv, dim=1)
            viewout = v_uv.permute(0, 2, 3, 1)[:, :, :, None, :] @ f2.transpose(-2, -1)
            return nml1, nml2, viewout[:, :, :, 0, :].permute(0, 3, 1, 2)

        def fused():
            nml1 = uvframes.uv_frames(verts, topo)[0]
            nml2, viewout, _ = uvframes.uv_frames(verts2, topo, posmap=p_uv, flip_normal=True, cam_pos=cam)
            return nml1, nml2, viewout

        def both(fwd):
            torch.autograd.grad(list(fwd()), leaves, [w1, w2, w3])

        if args.kernels_only:
            for _ in range(args.warmup + args.reps):
                both(fused)
            torch.cuda.synchronize()
            continue
        row = {"B": B}
        oa, ob = parent(), fused()
        ga, gb = (torch.autograd.grad(list(o), leaves, [w1, w2, w3]) for o in (oa, ob))
        row["max_abs_diff"] = {k: float((x - y).detach().abs().max()) for k, x, y in
                               zip(("nml1", "nml2", "viewout", "g_verts", "g_verts_displaced", "g_p_uv"), oa + ga, ob + gb)}
        row["g_max"] = {k: float(x.abs().max()) for k, x in zip(("g_verts", "g_verts_displaced", "g_p_uv"), ga)}
        del oa, ob, ga, gb
        for tag, fa, fb in (("fwd", parent, fused), ("fwd_bwd", lambda: both(parent), lambda: both(fused))):
            ta, tb = _alternate(fa, fb, args.reps, args.warmup)
            pa, fu = _stat(ta), _stat(tb)
            row[tag] = {"parent": pa, "fused": fu, "speedup": pa["median_ms"] / fu["median_ms"],
                        "faster_beyond_parent_spread": fu["median_ms"] + pa["spread_ms"] < pa["median_ms"]}
        # algorithmic bytes per texel of the fused passes, from the shapes: the topology record is read once for all views
        T = S * S
        fwd_b = (12 + 12 + 12 + 12) * B + 16 * 2          # nml1 | posmap in, nml2, viewout out | one record per pass
        # backward, pass 1: g_nml in, g_t0 / g_nraw planes out and in again; pass 2: posmap, g_nml, g_viewout in, g_t0 / g_U /
        # g_V / g_posmap out, the stencil's g_U / g_V / g_posmap in and g_posmap out, g_t0 in again; records and texel lists
        bwd_b = (12 + 24 + 24) * B + (36 + 48 + 36 + 12 + 12) * B + 16 * 2 + 16 + 4 * 3
        for tag, bts in (("fwd", fwd_b), ("fwd_bwd", fwd_b + bwd_b)):
            ms = row[tag]["fused"]["median_ms"]
            row[tag]["algorithmic_bytes_per_texel"] = bts
            row[tag]["fraction_of_8TBs"] = bts * T / (ms * 1e-3) / HBM
        res["rows"].append(row)
    if args.kernels_only:
        return
    # ---- the share of one decoder forward + backward ----------------------------------------------------------------------
    B, L = 1, 8
    dec = shaped.ShapedConvTeacherDecoder(seed=0)
    dec.geo_fn = Geo(S, n)
    dec.raw_index_mask = (dec.geo_fn.index_image != -1).any(dim=-1)
    dec.shadow = False
    dec.featenc = Pooled(dec.featenc)
    dec = dec.cuda().train()
    g = torch.Generator().manual_seed(1)
    inp = dict(lbs_motion=torch.randn(B, 4, generator=g), id_mesh=dome[None].repeat(B, 1, 1) * 0.9,
               tex_mean=255.0 * torch.rand(B, 3, S, S, generator=g), verts_rec=dome[None] + 0.1 * torch.randn(B, V, 3, generator=g),
               cam_pos=torch.tensor([[30.0, -40.0, 700.0]]).repeat(B, 1),
               light_pos=1100.0 * F.normalize(torch.randn(B, L, 3, generator=g) + torch.tensor([0.0, 0.0, 2.0]), dim=-1),
               light_intensity=0.5 + torch.rand(B, L, 1, generator=g))
    inp = {k: v.cuda() for k, v in inp.items()}
    inp["verts_rec"].requires_grad_(True)
    w_tex, w_phys = torch.randn(B, 3, S, S, generator=g).cuda(), torch.randn(B, 3, S, S, generator=g).cuda()
    module = types.SimpleNamespace(ConvTeacherDecoder=shaped.ShapedConvTeacherDecoder, get_shadow_map=None)

    def decoder_step(forward):
        out = forward(dec, **inp)
        loss = (out["tex"] * w_tex).sum() + (out["phys_tex"] * w_phys).sum()
        torch.autograd.grad(loss, [inp["verts_rec"]] + list(dec.parameters()), allow_unused=True)

    try:
        dropin.patch_urhand(module)
        plain = shaped.ShapedConvTeacherDecoder.forward
        dropin.patch_urhand(module, uv_frames=True)
        fused_fwd = shaped.ShapedConvTeacherDecoder.forward
    finally:
        del shaped.ShapedConvTeacherDecoder.forward
    ta, tb = _alternate(lambda: decoder_step(plain), lambda: decoder_step(fused_fwd), args.reps, args.warmup)
    pa, fu = _stat(ta), _stat(tb)
    lines = res["rows"][0]["fwd_bwd"]
    res["decoder"] = {"what": "tests/urhand_shaped.py stand-in sub-modules, S = 1024, B = 1, 8 lights, shadow maps off, "
                              "forward + backward; the real UNets and the shadow maps only add to the denominators",
                      "parent": pa, "uv_frames": fu,
                      "share_of_parent_step": lines["parent"]["median_ms"] / pa["median_ms"],
                      "share_of_uv_frames_step": lines["fused"]["median_ms"] / fu["median_ms"],
                      "faster_beyond_parent_spread": fu["median_ms"] + pa["spread_ms"] < pa["median_ms"]}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
