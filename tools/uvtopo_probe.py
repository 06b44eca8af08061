"""uvtopo probe: the time to build a model's UV topology images on the GPU (goliath_amd.uvtopo.index_images) beside the
KD-tree impaint of the reference on the same inputs and the same machine.

Scene: S = 1024, a head-sized grid mesh in two UV islands ([0.04, 0.48] and [0.52, 0.96] wide, [0.1, 0.9] high, 59 x 59
vertices each: V = 6962, F = 13456), impaint on with the reference's default threshold of 100 texels.  Recorded, not
asserted:
  * index_images(impaint=False) and index_images(impaint=True): medians over --reps calls after --warmup, HIP events
    around the whole call (workspace allocation included), and the ABI entries of one call by themselves;
  * where scikit-learn imports: the host time of the reference's impaint restated from its description -- a KDTree over
    the valid texels' (row, col), one nearest-neighbour query for every other texel, `dists < threshold`, the indexed
    copies into clones of index_image and bary_image, and the second tree for face_index_image (the reference builds it
    twice, ca_code/utils/geom.py:238-244) -- on the images this library produced, device-to-host copies not counted;
    and how many texels the two source maps disagree on (equidistant sources only: the tree's choice is unspecified).
Prints one JSON line and writes it to --out.

    python tools/uvtopo_probe.py [--reps 9] [--warmup 2] [--out profiles/uvtopo_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from goliath_amd import _lib, build, uvtopo  # noqa: E402

S, N, THRESHOLD = 1024, 58, 100.0


def two_island_mesh(n=N):
    """vi, vt, vti of two (n+1)^2-vertex grids side by side in uv; the islands share no uv vertex, the mesh vertices of the
    right island's left column are those of the left island's right column (a seam: vti != vi)."""
    parts, faces = [], []
    for k, (u0, u1) in enumerate(((0.04, 0.48), (0.52, 0.96))):
        u, v = np.linspace(u0, u1, n + 1), np.linspace(0.1, 0.9, n + 1)
        parts.append(np.stack(np.broadcast_arrays(u[None, :], v[:, None]), -1).reshape(-1, 2))
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        p = (k * (n + 1) ** 2 + i * (n + 1) + j).reshape(-1)
        faces.append(np.concatenate([np.stack([p, p + 1, p + n + 2], -1), np.stack([p, p + n + 2, p + n + 1], -1)]))
    vt, vti = np.concatenate(parts).astype(np.float32), np.concatenate(faces).astype(np.int64)
    vertex_of = np.arange(len(vt))
    rows = np.arange(n + 1) * (n + 1)
    vertex_of[(n + 1) ** 2 + rows] = rows + n
    return vertex_of[vti], vt, vti


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def kdtree_impaint(index_image, bary_image, face_index_image, threshold):
    """The reference's impaint, restated: returns (seconds, source map of the first query)."""
    from sklearn.neighbors import KDTree

    t0 = time.perf_counter()
    src_map = None
    for image, extra in ((index_image, bary_image), (face_index_image, None)):
        valid = (image != -1).any(-1) if image.ndim == 3 else image != -1
        valid_ij, invalid_ij = np.argwhere(valid), np.argwhere(~valid)
        dists, idxs = KDTree(valid_ij).query(invalid_ij)
        near = dists[:, 0] < threshold
        src, dst = valid_ij[idxs[:, 0]][near], invalid_ij[near]
        for a in (image, extra):
            if a is not None:
                b = a.copy()
                b[dst[:, 0], dst[:, 1]] = a[src[:, 0], src[:, 1]]
        if src_map is None:
            src_map = np.full(valid.shape, -1, np.int64)
            src_map[dst[:, 0], dst[:, 1]] = src[:, 0] * valid.shape[1] + src[:, 1]
    return time.perf_counter() - t0, src_map


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uvtopo_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    vi, vt, vti = (torch.from_numpy(a).cuda() for a in two_island_mesh())
    res = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "S": S,
           "vertices": int(vi.max()) + 1, "uv_vertices": int(vt.shape[0]), "faces": int(vti.shape[0]),
           "impaint_threshold": THRESHOLD, "reps": args.reps}
    res["hip_index_images_ms"] = timed(lambda: uvtopo.index_images(vi, vt, vti, S), args.reps, args.warmup)
    res["hip_index_images_impaint_ms"] = timed(
        lambda: uvtopo.index_images(vi, vt, vti, S, impaint=True, impaint_threshold=THRESHOLD), args.reps, args.warmup)
    _lib.TIMING = []
    uvtopo.index_images(vi, vt, vti, S, impaint=True, impaint_threshold=THRESHOLD)
    torch.cuda.synchronize()
    res["hip_abi_ms"] = {name: e0.elapsed_time(e1) for name, e0, e1 in _lib.TIMING}
    _lib.TIMING = None
    plain = uvtopo.index_images(vi, vt, vti, S)
    filled = uvtopo.index_images(vi, vt, vti, S, impaint=True, impaint_threshold=THRESHOLD)
    src = uvtopo.nearest_valid(plain.valid_mask[..., 0], THRESHOLD).cpu().numpy()
    res["covered_texels"] = int(plain.valid_mask.sum())
    res["impainted_texels"] = int((src >= 0).sum())
    res["texels_left_empty"] = int((filled.face_index_image < 0).sum())
    try:
        import sklearn

        host = [a.cpu().numpy() for a in (plain.index_image, plain.bary_image, plain.face_index_image)]
        times = []
        for _ in range(2):
            t, ref_src = kdtree_impaint(*host, THRESHOLD)
            times.append(t)
        res["sklearn"] = sklearn.__version__
        res["kdtree_impaint_host_s"] = {"median": statistics.median(times), "min": min(times), "max": max(times)}
        res["source_maps_differ_on_texels"] = int((ref_src != src).sum())
        res["kdtree_over_hip_impaint"] = (res["kdtree_impaint_host_s"]["median"] * 1e3
                                          / max(res["hip_index_images_impaint_ms"]["median"]
                                                - res["hip_index_images_ms"]["median"], 1e-6))
    except ImportError:
        res["sklearn"] = None
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
