"""Generate tests/golden/uvframes_golden.partNN.npz by running the REFERENCE's own `vert_normals`, `xyz2normals`,
`compute_tbn_uv_given_normal` (/root/reference/ca_code/utils/geom.py:337-346, 665-686, 432-470), `index` and `F.normalize`
in the order of ConvTeacherDecoder.forward (ca_code/models/urhand.py:366-392, :467-486, :573-578) on the CPU, once in
float32 and once with the same float32 inputs in float64, with backward against seeded cotangents.  Build container only
(imports ca_code through tests/golden/ref_stubs.py).  Only numbers are stored.

Topologies and inputs: tests/uvframes_cases.py (plain tensors, rebuilt by the tests; a checksum of the inputs is stored).
Per case and run (A = interpolated vertex normals, B = xyz2normals(posmap); 0 / 1 = flip_normal) the golden holds
  ref64/<case>/<run>/{frames, viewout}   float64, on the covered texels only ([B,M,3,3], [B,3,M]); nml is frames' row 2
  ref64/<case>/<run>/{g_verts, g_posmap, g_cam_pos}   (the clamp cases also ref32/..., for comparisons in groups)
  err32/<case>/<run>/<quantity>/B<k>     max |float32 result - float64 result| over the first k views (k = 1 and all)
and per case `consts/<case>`: the reference's float32 (f, vt01.y, vt02.y) of every covered texel.
The generator prints the smallest |t0 raw|, |n x t0|, |U x V| (and |n raw|, |b x n|) of the general cases and asserts that
each is at least 10 x its clamp on cases 1-4: those cases test arithmetic, the clamps have cases of their own."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import npz_parts  # noqa: E402
import ref_stubs  # noqa: E402

ref_stubs.install()
from ca_code.utils.geom import compute_tbn_uv_given_normal, vert_normals, xyz2normals  # noqa: E402
from ca_code.utils.torchutils import index  # noqa: E402
import uvframes_cases as cases  # noqa: E402


def run(dtype, geo, inp, mode_b, flip, views):
    """The reference's lines in `dtype` on the first `views` views: outputs and gradients."""
    leaf = lambda k: inp[k][:views].to(dtype).clone().requires_grad_(True)
    verts, posmap, cam_pos = leaf("verts"), leaf("posmap"), leaf("cam_pos")
    B = views
    mask = (geo.index_image != -1).any(dim=-1)
    idxs = geo.index_image[mask]
    tri_uv = geo.vt.to(dtype)[geo.v2uv[idxs, 0].to(torch.long)]
    tri_xyz = verts[:, idxs]
    if mode_b:
        n = xyz2normals(posmap)
        n = n[:, :, mask].permute(0, 2, 1)
    else:
        vert_nml = vert_normals(verts, geo.vi)
        vi_img = geo.vi[geo.face_index_image[mask]]
        bary_img = geo.bary_image[mask].to(dtype)
        vn_img = [torch.stack([index(vert_nml[i], vi_img[..., k], 0) for i in range(B)]) for k in range(3)]
        vn_img = (torch.stack(vn_img, dim=3) * bary_img[None, :, None, :]).sum(-1)
        n = vn_img / torch.norm(vn_img, dim=-1, keepdim=True).clamp(min=1e-5)
    t, b, n = compute_tbn_uv_given_normal(tri_xyz, tri_uv, n)
    tbn = torch.stack((t, -b, -n if flip else n), dim=-2)
    S = geo.uv_size
    frames = torch.zeros((B, S, S, 3, 3), dtype=dtype)
    frames[:, mask] = tbn
    nml = frames[:, :, :, 2:].permute(0, 3, 4, 1, 2)[:, 0, ...]
    v_uv = F.normalize(cam_pos[..., None, None] - posmap, dim=1)
    viewout = v_uv.permute(0, 2, 3, 1)[:, :, :, None, :] @ frames.transpose(-2, -1)
    viewout = viewout[:, :, :, 0, :].permute(0, 3, 1, 2)
    cot = lambda k: inp[k][:views].to(dtype)
    loss = (nml * cot("g_nml")).sum() + (viewout * cot("g_viewout")).sum() + (frames * cot("g_frames")).sum()
    g_verts, g_posmap, g_cam_pos = torch.autograd.grad(loss, (verts, posmap, cam_pos))
    out = dict(frames=frames[:, mask], nml=nml[:, :, mask], viewout=viewout[:, :, mask], g_verts=g_verts, g_posmap=g_posmap,
               g_cam_pos=g_cam_pos)
    return {k: v.detach() for k, v in out.items()}


def smallest_norms(geo, inp):
    """float64 norms in front of every clamp, over all views: (|t0 raw|, |n raw| A, |U x V| B, |n x t0| A / B, |b x n| A / B)."""
    dt = torch.float64
    mask = (geo.index_image != -1).any(dim=-1)
    idxs = geo.index_image[mask]
    tri_uv = geo.vt.to(dt)[geo.v2uv[idxs, 0].long()]
    xyz = inp["verts"].to(dt)[:, idxs]
    v01, v02 = xyz[:, :, 1] - xyz[:, :, 0], xyz[:, :, 2] - xyz[:, :, 0]
    t01, t02 = tri_uv[:, 1] - tri_uv[:, 0], tri_uv[:, 2] - tri_uv[:, 0]
    fin = t01[:, 0] * t02[:, 1] - t01[:, 1] * t02[:, 0]
    raw = (1.0 / fin)[None, :, None] * (v01 * t02[None, :, 1:2] - v02 * t01[None, :, 1:2])
    t0 = raw / raw.norm(dim=-1, keepdim=True)
    vn = vert_normals(inp["verts"].to(dt), geo.vi)
    vi_img = geo.vi[geo.face_index_image[mask]]
    n_raw = (vn[:, vi_img] * geo.bary_image[mask].to(dt)[None, ..., None]).sum(2)
    p = F.pad(inp["posmap"].to(dt), (1, 1, 1, 1))
    U = (p[:, :, 2:, 1:-1] - p[:, :, :-2, 1:-1]) / -2
    V = (p[:, :, 1:-1, 2:] - p[:, :, 1:-1, :-2]) / -2
    uxv = torch.linalg.cross(U, V, dim=1)[:, :, mask].permute(0, 2, 1)
    res = {"|fin|": float(fin.abs().min()), "|t0 raw|": float(raw.norm(dim=-1).min()), "|n raw| (A)": float(n_raw.norm(dim=-1).min()),
           "|U x V| (B)": float(uxv.norm(dim=-1).min())}
    for tag, nn in (("A", n_raw), ("B", uxv)):
        n = nn / nn.norm(dim=-1, keepdim=True)
        braw = torch.linalg.cross(n, t0)
        b = braw / braw.norm(dim=-1, keepdim=True)
        res[f"|n x t0| ({tag})"] = float(braw.norm(dim=-1).min())
        res[f"|b x n| ({tag})"] = float(torch.linalg.cross(b, n).norm(dim=-1).min())
    return res


CLAMPS = {"|fin|": 1e-8, "|t0 raw|": 1e-5, "|n raw| (A)": 1e-5, "|U x V| (B)": 1e-8, "|n x t0| (A)": 1e-5, "|n x t0| (B)": 1e-5,
          "|b x n| (A)": 1e-5, "|b x n| (B)": 1e-5}


def main():
    out = {}
    for ci, name in enumerate(cases.CASES + cases.CLAMP_CASES):
        geo, inp = cases.inputs(name)
        mask = (geo.index_image != -1).any(dim=-1)
        out[f"checksum/{name}"] = np.float64(cases.checksum(inp))
        # the reference's float32 topology constants, per covered texel (geom.py:448-454)
        tri_uv = geo.vt[geo.v2uv[geo.index_image[mask], 0].long()]
        vt01, vt02 = tri_uv[:, 1] - tri_uv[:, 0], tri_uv[:, 2] - tri_uv[:, 0]
        fin = vt01[..., 0] * vt02[..., 1] - vt01[..., 1] * vt02[..., 0]
        raw_fin = fin.clone()
        fin[torch.abs(fin) < 1.0e-8] = 1.0e-8
        out[f"consts/{name}"] = torch.stack([1.0 / fin, vt01[..., 1], vt02[..., 1]], -1).numpy()
        print(f"== {name}: V = {inp['verts'].shape[1]}, covered = {int(mask.sum())} texels, smallest fin = {float(raw_fin.min()):.3e}")
        if name in cases.CASES:
            norms = smallest_norms(geo, inp)
            print("   smallest norms:", {k: float(f"{v:.3e}") for k, v in norms.items()})
            if ci < 4:
                for k, v in norms.items():
                    assert v >= 10.0 * CLAMPS[k], (name, k, v)
        if name == "seam":
            assert bool(((raw_fin < 0.0) & (raw_fin > -1e-8)).any())       # the negative tiny fin
            differs = (geo.vt[geo.v2uv[:, 0]] != geo.vt[:geo.v2uv.shape[0]]).any(-1)
            assert int(differs.sum()) == 3
        if name == "impaint":
            other = (geo.vi[geo.face_index_image[mask]] != geo.index_image[mask]).any(-1)
            print(f"   texels whose face_index_image triple differs: {int(other.sum())}")
            assert int(other.sum()) > 100
        for run_name, mode_b, flip, views in cases.RUNS.get(name, cases.DEFAULT_RUNS):
            r32 = run(torch.float32, geo, inp, mode_b, flip, views)
            r64 = run(torch.float64, geo, inp, mode_b, flip, views)
            for k, v in r64.items():
                if k != "nml":                      # frames' row 2
                    out[f"ref64/{name}/{run_name}/{k}"] = v.numpy()
                if name in cases.CLAMP_CASES and k.startswith("g_"):   # compared in groups of one scale each
                    out[f"ref32/{name}/{run_name}/{k}"] = r32[k].numpy()
                for nb in sorted({1, views}):
                    out[f"err32/{name}/{run_name}/{k}/B{nb}"] = np.float64((r32[k][:nb].double() - v[:nb]).abs().max())
                print(f"   {run_name} {k:10s} max |fp64| = {float(v.abs().max()):.3e}   fp32 - fp64 = "
                      f"{float((r32[k].double() - v).abs().max()):.3e}   finite = {bool(torch.isfinite(v).all())}")
                assert torch.isfinite(v).all() and torch.isfinite(r32[k]).all(), (name, run_name, k)
    for path in npz_parts.save(os.path.join(HERE, "uvframes_golden.npz"), out):
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
