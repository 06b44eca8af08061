"""viewtex probe: the time to add B camera images to the mean-texture accumulators with goliath_amd.viewtex.TexMean.add
beside a plain-torch restatement of the reference's way, on the same inputs and the same GPU.

Scene: UV 1024^2 over the two-island grid mesh of tools/uvtopo_probe.py (V = 6962, F = 13456, impainted), bent into a
bumpy sheet that fills most of a 2048 x 1334 camera image; the cameras' face index images come from meshraster.rasterize
and are handed to both sides (the rasteriser is not timed).  B = 1 and B = 8.  Recorded, not asserted:
  (i)  torch: compute_face_visibility, compute_uv_visiblity_face and compute_view_texture restated line by line from
       their description (a th.unique and a boolean-mask write per view, boolean-mask gathers, two matmuls, grid_sample,
       a masked scatter into a zeroed [B,3,S,S]) plus the script's two accumulator adds into [1,3,S,S] tensors -- once per
       camera, as run_gen_texmean.py loops (`torch_per_camera_ms`, B iterations), and as one batch of B
       (`torch_batched_ms`);
  (ii) hip: TexMean.add of the B cameras (`hip_ms`), and its two ABI entries by themselves.
Each figure is the median, minimum and maximum over --reps timed windows after --warmup, device events around the window
with a synchronise, the sides alternating; a window is one call of (i) or --hip-calls back-to-back calls of (ii), reported
per call.  `hip_hbm_fraction` is the algorithmic bytes of (ii) -- index images read once, the
visibility bytes written and read, topology and vertex table read once (the vertex gathers hit a table of 84 KB: cache,
not HBM), one 3-channel pixel per texel and view that shows something, the accumulators read and written once -- over the
median time, as a share of the 6.3 TB/s a streaming copy achieves on this GPU.  `texels_equal` compares the two sides' totals after one add from zero.
Prints one JSON line and writes it to --out.

    python tools/viewtex_probe.py [--reps 15] [--warmup 3] [--out profiles/viewtex_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from goliath_amd import _lib, build, meshraster, uvtopo, viewtex  # noqa: E402
from uvtopo_probe import two_island_mesh  # noqa: E402

S, H, W = 1024, 2048, 1334
HBM_ACHIEVABLE = 6.3e12


# ---- (i): the reference's three functions, restated ---------------------------------------------------------------------------
def face_visibility(index_img, n_faces):
    out = torch.zeros((index_img.shape[0], n_faces), dtype=torch.bool, device=index_img.device)
    for b in range(index_img.shape[0]):
        out[b, torch.unique(index_img[b][index_img[b] != -1].reshape(-1))] = True
    return out


def uv_visibility(face_index_image, n_faces, face_index_uv):
    B, s = face_index_image.shape[0], face_index_uv.shape[0]
    vis = torch.zeros((B, s, s), dtype=torch.bool, device=face_index_image.device)
    face_mask = face_visibility(face_index_image, n_faces)
    for b in range(B):
        mask = face_index_uv != -1
        vis[b][mask] = face_mask[b][face_index_uv[mask]]
    return vis


def view_texture(verts, n_faces, image, face_index_image, K, Rt, index_image_uv, bary_image_uv, face_index_uv):
    B, s = verts.shape[0], index_image_uv.shape[0]
    h, w = image.shape[2:4]
    uv_mask = index_image_uv[..., 0] != -1
    index_flat, bary_flat = index_image_uv[uv_mask], bary_image_uv[uv_mask]
    xyz = torch.sum(verts[:, index_flat] * bary_flat[None, :, :, None], dim=2)
    p_cam = xyz @ Rt[:, :3, :3].mT + Rt[:, :3, 3][:, None]
    p_pix = p_cam @ K.mT
    v_pix = p_pix[..., :2] / p_pix[:, :, 2:]
    yxs = 2.0 * torch.stack((v_pix[:, :, 0] / w, v_pix[:, :, 1] / h), dim=-1) - 1.0
    rgb = F.grid_sample(image, yxs[:, None], mode="nearest", align_corners=False, padding_mode="border")[:, :, 0]
    tex = torch.zeros((B, 3, s, s), dtype=rgb.dtype, device=verts.device)
    tex[:, :, uv_mask] = rgb
    vis = uv_visibility(face_index_image.long(), n_faces, face_index_uv)
    return tex * vis[:, None], vis[:, None]


def torch_add(total, cnt, per_camera, verts, n_faces, image, index_img, K, Rt, topo):
    groups = [slice(b, b + 1) for b in range(image.shape[0])] if per_camera else [slice(None)]
    for g in groups:
        tex, mask = view_texture(verts.expand(image.shape[0], -1, -1)[g], n_faces, image[g], index_img[g], K[g], Rt[g], *topo)
        if per_camera:
            total += tex
            cnt += mask.float()
        else:
            total += tex.sum(0, keepdim=True)
            cnt += mask.float().sum(0, keepdim=True)


# ---- scene --------------------------------------------------------------------------------------------------------------------
def scene(B, seed=0):
    vi, vt, vti = two_island_mesh()
    V = int(vi.max()) + 1
    uv = np.zeros((V, 2))
    uv[vi.reshape(-1)] = vt[vti.reshape(-1)]
    verts = np.stack([(uv[:, 0] - 0.5) * 2.0, (uv[:, 1] - 0.5) * 3.0, 0.25 * np.sin(5 * uv[:, 0]) * np.cos(4 * uv[:, 1])], -1)
    rng = np.random.default_rng(seed)
    K = np.stack([[[1900.0 + 20 * b, 0.5, W / 2 + 3 * b], [0, 1900.0 + 20 * b, H / 2 - 2 * b], [0, 0, 1]] for b in range(B)])
    Rt = []
    for b in range(B):
        a = 0.5 * (b - (B - 1) / 2) / max(B, 1)
        Rt.append([[np.cos(a), 0, np.sin(a), 0.02 * b], [0, 1, 0, 0.0], [-np.sin(a), 0, np.cos(a), 3.2]])
    cuda = lambda a, dt=torch.float32: torch.from_numpy(np.asarray(a)).to(device="cuda", dtype=dt)  # noqa: E731
    image = torch.from_numpy(rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)).cuda()
    return (cuda(vi, torch.int64), cuda(vt), cuda(vti, torch.int64), cuda(verts)[None], image, cuda(K), cuda(np.array(Rt)))


def timed_pair(fns, reps, warmup):
    """fns: {name: (callable, calls per timed window)}; the sides alternate; -> {name: {median, min, max}}, ms per call."""
    for _ in range(warmup):
        for f, _n in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, (f, n) in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(n):
                f()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / n)
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hip-calls", type=int, default=20, help="TexMean.add calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewtex_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "S": S, "H": H, "W": W,
           "reps": args.reps, "warmup": args.warmup, "hip_calls_per_window": args.hip_calls, "hbm_achievable_Bps": HBM_ACHIEVABLE, "cases": {}}
    for B in (1, 8):
        vi, vt, vti, verts, image, K, Rt = scene(B)
        n_faces = int(vi.shape[0])
        img = uvtopo.index_images(vi, vt, vti, S, impaint=True)
        topo_t = (img.index_image, img.bary_image, img.face_index_image)
        topo = viewtex.ViewTexTopology(*topo_t)
        index_img = meshraster.rasterize(meshraster.transform(verts.expand(B, -1, -1), K, Rt), vi, H, W, with_bary=False)[0]
        tm = viewtex.TexMean(topo, n_faces)
        total = torch.zeros(1, 3, S, S, device="cuda")
        cnt = torch.zeros(1, 3, S, S, device="cuda")
        # agreement first, from zero
        tm.add(verts, image, K, Rt, index_img=index_img)
        torch_add(total, cnt, True, verts, n_faces, image, index_img, K, Rt, topo_t)
        same = (tm.total == total[0]).all(0)
        shown = int((tm.count > 0).sum())
        visible_texel_views = float(tm.count.sum())
        case = {"B": B, "faces": n_faces, "vertices": int(verts.shape[1]),
                "pixels_covered_share": float((index_img >= 0).float().mean()),
                "texels_shown": shown, "texel_views_shown": visible_texel_views,
                "texels_equal": int(same.sum()), "texels": S * S,
                "counts_equal": bool(torch.equal(tm.count, cnt[0, 0]))}
        fns = {"torch_per_camera_ms": (lambda: torch_add(total, cnt, True, verts, n_faces, image, index_img, K, Rt, topo_t), 1),
               "torch_batched_ms": (lambda: torch_add(total, cnt, False, verts, n_faces, image, index_img, K, Rt, topo_t), 1),
               "hip_ms": (lambda: tm.add(verts, image, K, Rt, index_img=index_img), args.hip_calls)}
        case.update(timed_pair(fns, args.reps, args.warmup))
        _lib.TIMING = []
        tm.add(verts, image, K, Rt, index_img=index_img)
        torch.cuda.synchronize()
        case["hip_abi_ms"] = {name: e0.elapsed_time(e1) for name, e0, e1 in _lib.TIMING}
        _lib.TIMING = None
        P = S * S
        # compulsory traffic: index images, the visibility bytes written and read, topology, the (tiny, cached) vertex
        # table once, one 3-channel pixel per shown texel-view, the accumulators read and written
        nbytes = B * H * W * 4 + 2 * B * n_faces + P * 28 + verts.numel() * 4 + visible_texel_views * 12 + P * 32
        case["hip_algorithmic_bytes"] = nbytes
        case["hip_hbm_fraction"] = nbytes / (case["hip_ms"]["median"] * 1e-3) / HBM_ACHIEVABLE
        t = case["torch_per_camera_ms"]
        case["torch_per_camera_over_hip"] = t["median"] / case["hip_ms"]["median"]
        case["torch_batched_over_hip"] = case["torch_batched_ms"]["median"] / case["hip_ms"]["median"]
        case["hip_faster_than_torch_by_more_than_its_spread"] = bool(
            t["median"] - case["hip_ms"]["median"] > t["max"] - t["min"])
        mean = tm.mean(flip_rows=True, bgr=True)
        case["mean_finite"] = bool(torch.isfinite(mean).all())
        res["cases"][f"B{B}"] = case
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
