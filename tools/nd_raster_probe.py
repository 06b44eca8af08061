"""N-channel rasterizer probe: gol_rasterize_nd_fwd / _bwd against the 3-channel kernels on the same lists.

Config-2 scene (one view, 2048x1334, 250k Gaussians of tests/scenes.head_scene), projected and binned on the
GPU (gol_bin_sort, the pruned lists rasterize_gaussians uses); forward and backward of gsplat's layout ([H,W,C] images,
dense gradients) timed with HIP events after a warm-up, for each C of --channels (C = 3 through the N-channel kernel)
and for gol_rasterize_fwd / _bwd.  Prints one JSON line (and writes it to --out).

    python tools/nd_raster_probe.py [--reps 20] [--warmup 3] [--channels 1,3,4,8,16,32] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from goliath_amd import build, splat  # noqa: E402
from scenes import head_scene  # noqa: E402


def _time_us(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return round(1000.0 * e0.elapsed_time(e1) / reps, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", default="1,3,4,8,16,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W, N = 2048, 1334, 250_000
    s = head_scene(N, H, W, seed=0)
    g = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in s.items()}
    xys, depths, radii, conics, comp, nth, _ = (t.detach() for t in splat.project_gaussians(
        g["means"], g["scales"], 1.0, g["quats"], g["viewmat"], s["fx"], s["fy"], s["cx"], s["cy"], H, W, 16, 0.1))
    opac = (g["opacity"][:, 0] * comp).contiguous()
    ws = splat._Workspace(1, N, splat._tiles(H, W), int(nth.sum()), "cuda")
    splat._bin_sort(1, N, xys, depths, radii, H, W, ws, conics, opac)
    lists = dict(B=1, N=N, img_h=H, img_w=W, tile_bins=ws.tile_bins, sorted_ids=ws.sorted_ids, capacity=ws.capacity)
    gen = torch.Generator(device="cuda").manual_seed(0)
    v_alpha = torch.randn(1, H, W, device="cuda", generator=gen)
    final_Ts = torch.empty(1, H, W, device="cuda")
    final_idx = torch.empty(1, H, W, dtype=torch.int32, device="cuda")
    grads = [torch.zeros(N, k, device="cuda") for k in (2, 3, 1)]   # v_xy, v_conic, v_opacity (accumulated: timing only)

    def bench(C, nd):
        colors = torch.rand(N, C, device="cuda", generator=gen)
        bg = torch.rand(C, device="cuda", generator=gen)
        out = torch.empty(1, H, W, C, device="cuda")
        v_out = torch.randn(1, H, W, C, device="cuda", generator=gen)
        v_col = torch.zeros(N, C, device="cuda")
        if nd:
            rec = splat._pack_records(1, N, xys, conics, None, None, opac)
            fwd = lambda: splat._abi_rasterize_nd_fwd(**lists, C=C, records=rec, colors=colors, background=bg, out_img=out,
                                                      final_Ts=final_Ts, final_idx=final_idx)
            bwd = lambda: splat._abi_rasterize_nd_bwd(**lists, C=C, records=rec, colors=colors, background=bg,
                                                      final_Ts=final_Ts, final_idx=final_idx, v_out_img=v_out,
                                                      v_out_alpha=v_alpha, v_xy=grads[0], v_conic=grads[1],
                                                      v_colors=v_col, v_opacity=grads[2])
        else:
            rec = splat._pack_records(1, N, xys, conics, colors, None, opac)
            fwd = lambda: splat._abi_rasterize_fwd(**lists, planar=0, records=rec, with_extra=0, background=bg, out_img=out,
                                                   final_Ts=final_Ts, final_idx=final_idx)
            bwd = lambda: splat._abi_rasterize_bwd(**lists, planar=0, records=rec, with_extra=0, background=bg,
                                                   final_Ts=final_Ts, final_idx=final_idx, v_out_img=v_out,
                                                   v_out_alpha=v_alpha, v_xy=grads[0], v_conic=grads[1], v_colors=v_col,
                                                   v_opacity=grads[2])
        fwd()
        return dict(fwd_us=_time_us(fwd, a.reps, a.warmup), bwd_us=_time_us(bwd, a.reps, a.warmup))

    ref = bench(3, nd=False)
    nd = {}
    for C in (int(c) for c in a.channels.split(",")):
        r = bench(C, nd=True)
        r["fwd_x"] = round(r["fwd_us"] / ref["fwd_us"], 2)
        r["bwd_x"] = round(r["bwd_us"] / ref["bwd_us"], 2)
        nd[str(C)] = r
    res = dict(probe="nd_raster", H=H, W=W, N=N, n_isect=int(ws.n_isect[0]), reps=a.reps, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), source_digest=build.source_digest(), ref_3ch=ref, nd=nd)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
