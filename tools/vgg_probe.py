#!/usr/bin/env python
"""Time the fused VGG layer (goliath_amd.perceptual.conv3_relu: gol_conv3_fwd / gol_conv3_bwd_x) against the library
composition it replaces -- F.conv2d(3x3, s1, p1) with its bias, relu, and max_pool2d(2) where the layer has one; the image
layer also the four normalisation passes of vgg.py:62-65 -- on the distinct layer shapes of VGG19 up to relu5_1 at the hand
configs' image size (2048 x 1334, B = 1), forward and forward + input gradient, and derive the dispatch table of
goliath_amd/perceptual.py.  Then the whole masked loss (prediction forward, target forward, image gradient) at B = 1 and
B = 4: `vgg_loss_torch` on the GPU against `VGGLossMasked` with the table just derived and with every layer forced, time and
peak memory; at B = 1 also how far either fp32 path is from the float64 twin at that size.

Method (that of tools/texdec_probe.py): every variant of a shape is warmed up, then the variants are timed alternately in
ROUNDS rounds inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds
and the spread (max - min over the rounds).  A shape is admitted to the dispatch table only if the HIP operator's forward +
backward median is below the torch composition's by more than the torch composition's own spread.
Outputs and input gradients of the two are compared at the timed size (rel-L2, the upstream gradient zeroed where a
pre-activation of the library's is within 1e-4 of the ReLU kink or the two largest values of a pool window are that close).  Needs the GPU; there is no fallback.

Usage: python tools/vgg_probe.py [--height 2048] [--width 1334] [--rounds 7] [--iters 3] [--loss-batches 1,4]
                                 [--out profiles/vgg_probe.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from goliath_amd import build, perceptual

KINK = 1e-4


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def alternate(variants, rounds, iters, warm=2):
    for fn in variants.values():   # warm-up: code objects, the library's algorithm choice, the allocator's blocks
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # alternate the variants inside every round
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    return {k: stats(v) for k, v in times.items()}


def layer_shapes(widths, H, W):
    """(Ci, Co, H, W, pool, image_in, how many of the 13 layers have this shape), in network order."""
    shapes, n_in = [], 3
    it = iter(perceptual.CONV_INDEX)
    for width, count in zip(widths, perceptual.GROUPS):
        for _ in range(count):
            i = next(it)
            key = (n_in, width, H, W, i in perceptual.POOLED, i == 0)
            if shapes and shapes[-1][:6] == key:
                shapes[-1] = key + (shapes[-1][6] + 1,)
            else:
                shapes.append(key + (1,))
            n_in = width
            if i in perceptual.POOLED:
                H, W = H // 2, W // 2
    return shapes


def probe_layer(B, Ci, Co, H, W, pool, image_in, rounds, iters):
    dev = "cuda"
    torch.manual_seed(Ci * 1000 + Co + H)
    x = (torch.rand(B, Ci, H, W, device=dev) * 330.0 - 40.0) if image_in else torch.randn(B, Ci, H, W, device=dev).relu()
    x.requires_grad_(True)
    weight = torch.randn(Co, Ci, 3, 3, device=dev) * (2.0 / (9 * Ci)) ** 0.5
    bias = 0.1 * torch.randn(Co, device=dev)
    ops = {"hip": lambda: perceptual.conv3_relu(x, weight, bias, pool, image_in),
           "torch": lambda: perceptual.conv3_relu_torch(x, weight, bias, pool, image_in)}

    def fwd(op):
        with torch.no_grad():
            return op()

    def fwd_bwd(op, up=None):
        y = op()
        return torch.autograd.grad(y, x, torch.ones_like(y) if up is None else up)[0]

    y = {k: fwd(op) for k, op in ops.items()}
    with torch.no_grad():
        pre = F.conv2d(perceptual.normalize(x) if image_in else x, weight, bias, 1, 1)
        near = pre.abs() < KINK
        keep = ~near
        if pool:    # also the windows whose two largest values are within KINK: the two fp32 paths may name either
            Hp, Wp = H // 2, W // 2
            win = pre.relu_()[:, :, :2 * Hp, :2 * Wp].reshape(B, Co, Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5)
            top = win.reshape(B, Co, Hp, Wp, 4).topk(2, -1).values
            keep = ~(F.max_pool2d(near.float(), 2) > 0) & ~((top[..., 0] > 0) & (top[..., 0] - top[..., 1] < KINK))
            del win, top
        del pre
    up = torch.randn_like(y["torch"]) * keep
    g = {k: fwd_bwd(op, up) for k, op in ops.items()}
    parity = {"y": rel_l2(y["hip"], y["torch"]), "g_x": rel_l2(g["hip"], g["torch"]),
              "zeroed_share": 1.0 - float(keep.double().mean())}
    del y, g, near, keep
    ones = torch.ones_like(up)
    del up
    variants = {f"{k}_{kind}": (lambda op=op, run=run: run(op)) for k, op in ops.items()
                for kind, run in (("fwd", fwd), ("fwd_bwd", lambda op: fwd_bwd(op, ones)))}
    times = alternate(variants, rounds, iters)
    gflop = 2.0 * 9 * Ci * Co * H * W * B / 1e9
    n_x, n_y = B * Ci * H * W, B * Co * H * W
    n_out = n_y // 4 if pool else n_y
    row = {"B": B, "Ci": Ci, "Co": Co, "H": H, "W": W, "pool": pool, "image_in": image_in, "gflop_fwd": gflop,
           "algorithmic_mb_fwd": 4 * (n_x + n_out) / 1e6, "unpooled_output_mb": 4 * n_y / 1e6, "parity_rel_l2": parity}
    for k, v in times.items():
        row[k + "_ms"] = v
    row["hip_fwd_tflops"] = gflop / row["hip_fwd_ms"]["median"]
    row["torch_fwd_tflops"] = gflop / row["torch_fwd_ms"]["median"]
    t, hp = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    row["admitted"] = bool(hp["median"] < t["median"] - t["spread"])
    return row


def probe_loss(B, H, W, dispatch, rounds, iters, float64=False):
    dev = "cuda"
    torch.manual_seed(B)
    feats = perceptual.Vgg19Features().to(dev)
    x = (torch.rand(B, 3, H, W, device=dev) * 330.0 - 40.0).requires_grad_(True)
    y = torch.rand(B, 3, H, W, device=dev) * 330.0 - 40.0
    mask = (torch.rand(B, 1, H, W, device=dev) > 0.3).float()
    net = perceptual.VGGLossMasked(feats)

    def run(kind):
        os.environ["GOLIATH_FUSED_VGG_ALL"] = "1" if kind == "all_fused" else "0"
        perceptual.DISPATCH = dispatch if kind == "dispatch" else {}
        loss = perceptual.vgg_loss_torch(feats, x, y, mask) if kind == "torch" else net(x, y, mask)
        g, = torch.autograd.grad(loss, x)
        return loss.detach(), g

    kinds = ("torch", "dispatch", "all_fused")
    out = {"B": B, "H": H, "W": W}
    ref = run("torch")
    for kind in kinds:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, g = run(kind)
        torch.cuda.synchronize()
        out[kind] = {"loss": float(loss), "loss_rel_to_torch": abs(float(loss) - float(ref[0])) / abs(float(ref[0])),
                     "g_image_rel_l2_to_torch": rel_l2(g, ref[1]),
                     "peak_memory_mb_above_inputs": (torch.cuda.max_memory_allocated() - base) / 1e6}
        del loss, g
    del ref
    if float64:     # how far the two fp32 paths are from the float64 twin at this size (ReLU and pool decisions flip in both)
        x64 =x.detach().double().requires_grad_(True)
        l64 = perceptual.vgg_loss_torch(feats, x64, y.double(), mask.double())
        g64, = torch.autograd.grad(l64, x64)
        for kind in ("torch", "all_fused"):
            loss, g = run(kind)
            out[kind]["loss_rel_to_float64"] = abs(float(loss) - float(l64.detach())) / abs(float(l64.detach()))
            out[kind]["g_image_rel_l2_to_float64"] = rel_l2(g, g64)
            del loss, g
        del l64, g64, x64
        torch.cuda.empty_cache()
    times = alternate({k: (lambda k=k: run(k)) for k in kinds}, rounds, iters, warm=1)
    for kind in kinds:
        out[kind]["fwd_bwd_ms"] = times[kind]
    os.environ.pop("GOLIATH_FUSED_VGG_ALL", None)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1334)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--loss-batches", default="1,4")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "vgg_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vgg_probe needs the GPU: there is nothing to measure without one")
    committed = dict(perceptual.DISPATCH)
    rows = []
    for Ci, Co, H, W, pool, image_in, count in layer_shapes((64, 128, 256, 512, 512), args.height, args.width):
        row = probe_layer(1, Ci, Co, H, W, pool, image_in, args.rounds, args.iters)
        row["layers_of_this_shape"] = count
        rows.append(row)
        print(f"{Ci:3d}->{Co:3d} @ {H}x{W}{' pool' if pool else ''}{' image' if image_in else ''}  fwd hip "
              f"{row['hip_fwd_ms']['median']:.3f} / torch {row['torch_fwd_ms']['median']:.3f} ms ({row['hip_fwd_tflops']:.1f} / "
              f"{row['torch_fwd_tflops']:.1f} TF)  fwd+bwd hip {row['hip_fwd_bwd_ms']['median']:.3f} / torch "
              f"{row['torch_fwd_bwd_ms']['median']:.3f} ms (torch spread {row['torch_fwd_bwd_ms']['spread']:.3f})  "
              f"admitted={row['admitted']}  parity y {row['parity_rel_l2']['y']:.1e} g_x {row['parity_rel_l2']['g_x']:.1e}",
              flush=True)
        torch.cuda.empty_cache()
    dispatch = [[r["Ci"], r["Co"], r["H"], r["W"], r["pool"]] for r in rows if r["admitted"]]
    table = {tuple(k): True for k in dispatch}
    losses = []
    for B in map(int, filter(None, args.loss_batches.split(","))):
        try:
            res = probe_loss(B, args.height, args.width, table, max(3, args.rounds // 2), 1, float64=B == 1)
        except torch.cuda.OutOfMemoryError as e:
            res = {"B": B, "H": args.height, "W": args.width, "does_not_fit": str(e)[:200]}
        losses.append(res)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()
    perceptual.DISPATCH = committed
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "rounds": args.rounds,
              "iters": args.iters, "kink": KINK, "layers": rows, "dispatch": dispatch,
              "committed_dispatch_matches": sorted(map(list, committed)) == sorted(dispatch), "loss": losses}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
