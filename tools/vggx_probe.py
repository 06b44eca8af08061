#!/usr/bin/env python
"""Time the split-bf16 VGG layer (goliath_amd.perceptual.conv3_relu(precision="bf16x3"): gol_conv3x_fwd / gol_conv3x_bwd_x,
the weight packed ahead) against the library composition -- F.conv2d(3x3, s1, p1) with its bias, relu, and max_pool2d(2)
where the layer has one -- on the wide layer shapes of VGG19 up to relu5_1 (Ci % 32 == 0) at the hand configs' image size
(2048 x 1334, B = 1), forward and forward + input gradient with achieved TF on 2 K M N, and derive the table
DISPATCH_BF16X3 of goliath_amd/perceptual.py.  Then the whole masked loss (prediction forward, target forward, image
gradient) at B = 1 and B = 4: `VGGLossMasked` at precision "fp32" with the committed DISPATCH (the configuration before this
precision existed) against precision "bf16x3" with the table just derived and with every supported layer forced: time,
peak memory, and the distance of loss and image gradient from the fp32 configuration.

Method: that of tools/vgg_probe.py (its `alternate`): every variant is warmed up, the variants are timed alternately in
ROUNDS rounds inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds
and the spread (max - min over the rounds).  A shape is admitted only if the operator's forward + backward median is below
the library composition's by more than the composition's own spread.  Outputs and input gradients of
the two are compared at the timed size (rel-L2, the upstream gradient zeroed where a pre-activation of the library's is
within 1e-4 of the ReLU kink or the two largest values of a pool window are that close).  Needs the GPU.

Usage: python tools/vggx_probe.py [--height 2048] [--width 1334] [--rounds 7] [--iters 3] [--loss-batches 1,4]
                                  [--out profiles/vggx_probe.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F

from goliath_amd import build, perceptual
from vgg_probe import KINK, alternate, layer_shapes, rel_l2


def probe_layer(B, Ci, Co, H, W, pool, rounds, iters):
    dev = "cuda"
    torch.manual_seed(Ci * 1000 + Co + H)
    x = torch.randn(B, Ci, H, W, device=dev).relu().requires_grad_(True)
    weight = torch.randn(Co, Ci, 3, 3, device=dev) * (2.0 / (9 * Ci)) ** 0.5
    bias = 0.1 * torch.randn(Co, device=dev)
    packed = perceptual.pack_bf16x3(weight)
    ops = {"hip": lambda: perceptual.conv3_relu(x, weight, bias, pool, precision="bf16x3", packed=packed),
           "torch": lambda: perceptual.conv3_relu_torch(x, weight, bias, pool)}

    def fwd(op):
        with torch.no_grad():
            return op()

    def fwd_bwd(op, up=None):
        y = op()
        return torch.autograd.grad(y, x, torch.ones_like(y) if up is None else up)[0]

    y = {k: fwd(op) for k, op in ops.items()}
    with torch.no_grad():
        pre = F.conv2d(x, weight, bias, 1, 1)
        near = pre.abs() < KINK
        keep = ~near
        if pool:
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
    row = {"B": B, "Ci": Ci, "Co": Co, "H": H, "W": W, "pool": pool, "gflop_fwd": gflop, "parity_rel_l2_to_library": parity}
    for k, v in times.items():
        row[k + "_ms"] = v
    for k in ("hip", "torch"):
        row[k + "_fwd_tflops"] = gflop / row[k + "_fwd_ms"]["median"]
        row[k + "_fwd_bwd_tflops"] = 2.0 * gflop / row[k + "_fwd_bwd_ms"]["median"]
    t, hp = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    row["admitted"] = bool(hp["median"] < t["median"] - t["spread"])
    return row


def probe_loss(B, H, W, table, rounds, iters):
    dev = "cuda"
    torch.manual_seed(B)
    feats = perceptual.Vgg19Features().to(dev)
    feats.pack()
    x = (torch.rand(B, 3, H, W, device=dev) * 330.0 - 40.0).requires_grad_(True)
    y = torch.rand(B, 3, H, W, device=dev) * 330.0 - 40.0
    mask = (torch.rand(B, 1, H, W, device=dev) > 0.3).float()
    net = perceptual.VGGLossMasked(feats)

    def run(kind):
        os.environ["GOLIATH_FUSED_VGG_ALL"] = "1" if kind == "bf16x3_all" else "0"
        feats.precision = "fp32" if kind == "fp32_committed" else "bf16x3"
        perceptual.DISPATCH_BF16X3 = table
        loss = net(x, y, mask)
        g, = torch.autograd.grad(loss, x)
        return loss.detach(), g

    kinds = ("fp32_committed", "bf16x3_dispatch", "bf16x3_all")
    out = {"B": B, "H": H, "W": W}
    ref = run("fp32_committed")
    for kind in kinds:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, g = run(kind)
        torch.cuda.synchronize()
        out[kind] = {"loss": float(loss),
                     "loss_rel_to_fp32_committed": abs(float(loss) - float(ref[0])) / abs(float(ref[0])),
                     "g_image_rel_l2_to_fp32_committed": rel_l2(g, ref[1]),
                     "peak_memory_mb_above_inputs": (torch.cuda.max_memory_allocated() - base) / 1e6}
        del loss, g
    del ref
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
                                                  "vggx_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vggx_probe needs the GPU: there is nothing to measure without one")
    committed = dict(perceptual.DISPATCH_BF16X3)
    rows = []
    for Ci, Co, H, W, pool, image_in, count in layer_shapes((64, 128, 256, 512, 512), args.height, args.width):
        if not perceptual.supported(Ci, Co, H, W, pool, image_in, "bf16x3"):
            continue
        row = probe_layer(1, Ci, Co, H, W, pool, args.rounds, args.iters)
        row["layers_of_this_shape"] = count
        rows.append(row)
        print(f"{Ci:3d}->{Co:3d} @ {H}x{W}{' pool' if pool else ''}  fwd bf16x3 {row['hip_fwd_ms']['median']:.3f} / torch "
              f"{row['torch_fwd_ms']['median']:.3f} ms ({row['hip_fwd_tflops']:.1f} / {row['torch_fwd_tflops']:.1f} TF)  "
              f"fwd+bwd bf16x3 {row['hip_fwd_bwd_ms']['median']:.3f} / torch {row['torch_fwd_bwd_ms']['median']:.3f} ms "
              f"(torch spread {row['torch_fwd_bwd_ms']['spread']:.3f})  admitted={row['admitted']}  parity y "
              f"{row['parity_rel_l2_to_library']['y']:.1e} g_x {row['parity_rel_l2_to_library']['g_x']:.1e}", flush=True)
        torch.cuda.empty_cache()
    dispatch = [[r["Ci"], r["Co"], r["H"], r["W"], r["pool"]] for r in rows if r["admitted"]]
    table = {tuple(k): True for k in dispatch}
    losses = []
    for B in map(int, filter(None, args.loss_batches.split(","))):
        try:
            res = probe_loss(B, args.height, args.width, table, max(3, args.rounds // 2), 1)
        except torch.cuda.OutOfMemoryError as e:
            res = {"B": B, "H": args.height, "W": args.width, "does_not_fit": str(e)[:200]}
        losses.append(res)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()
    perceptual.DISPATCH_BF16X3 = committed
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "rounds": args.rounds,
              "iters": args.iters, "kink": KINK, "layers": rows, "dispatch": dispatch,
              "committed_dispatch_matches": sorted(map(list, committed)) == sorted(dispatch), "loss": losses}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
