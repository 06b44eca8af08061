#!/usr/bin/env python
"""Time the fused MBConv front (goliath_amd.effnet.mbconv_front: gol_mbconv_front_fwd / gol_mbconv_front_bwd_x) on the five
front shapes of efficientnet_b0().features[1:4] at the hand configs' image size (2048 x 1334, B = 1), forward and
forward + input gradient, against
  (a) `folded`: the twin's lines -- F.conv2d 1x1 with the folded bias, silu, the depthwise F.conv2d with the folded bias,
      silu(z).sum -- and
  (b) `unfolded`: what the reference's torchvision modules run -- conv without bias, F.batch_norm in eval mode, silu as
      separate operators, twice, then the mean's sum,
and derive the dispatch table of goliath_amd/effnet.py.  Then the whole loss (one term: prediction with grad, target
without) at B = 1 and B = 4: `effnet_loss_torch` on the GPU against `EfficientNetLoss` with the table just derived and with
every front forced, time and peak memory; at B = 1 also how far either fp32 path is from the float64 twin at that size.

Method (that of tools/vgg_probe.py): every variant of a shape is warmed up, then the variants are timed alternately in
ROUNDS rounds inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds
and the spread (max - min over the rounds).  A shape is admitted to the dispatch table only if the HIP operator's forward +
backward median is below the folded lines' by more than the folded lines' own spread.  The achieved
bytes/s are over the operator's algorithmic bytes: forward x read + z written, backward x, z, g_z read + g_x written.
Needs the GPU; there is no fallback.

Usage: python tools/effnet_probe.py [--height 2048] [--width 1334] [--rounds 7] [--iters 3] [--loss-batches 1,4]
                                    [--out profiles/effnet_probe.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from goliath_amd import build, effnet


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


def front_shapes(H, W):
    """(block, Ci, Ce, H, W, k, stride) of the five fronts, in network order, for an H x W image."""
    H, W = effnet.out_size(H, 3, 2), effnet.out_size(W, 3, 2)      # the stem
    out = []
    for name, c_in, c_exp, _, k, stride, _ in effnet.BLOCKS:
        out.append((name, c_in, c_exp, H, W, k, stride))
        H, W = effnet.out_size(H, k, stride), effnet.out_size(W, k, stride)
    return out


def unfolded_front(x, conv_e, bn_e, conv_d, bn_d, k, stride):
    """The reference's operator sequence: conv, batch_norm (eval), silu, depthwise conv, batch_norm, [silu, mean]."""
    e = x
    if conv_e is not None:
        e = F.silu(F.batch_norm(F.conv2d(x, conv_e), bn_e[2], bn_e[3], bn_e[0], bn_e[1], False, 0.0, effnet.BN_EPS))
    z = F.conv2d(e, conv_d, None, stride, (k - 1) // 2, 1, conv_d.shape[0])
    z = F.batch_norm(z, bn_d[2], bn_d[3], bn_d[0], bn_d[1], False, 0.0, effnet.BN_EPS)
    return z, F.silu(z).sum((2, 3))


def probe_front(B, name, Ci, Ce, H, W, k, stride, rounds, iters):
    dev = "cuda"
    g = torch.Generator().manual_seed(Ci * 1000 + Ce + H)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    expand = Ce != Ci
    x = r(B, Ci, H, W).requires_grad_(True)
    bn = lambda: (1.0 + 0.3 * r(Ce), 0.3 * r(Ce), 0.3 * r(Ce), 0.5 + 1.5 * torch.rand(Ce, generator=g).to(dev))
    conv_e, bn_e = (r(Ce, Ci, 1, 1) / Ci ** 0.5, bn()) if expand else (None, None)
    conv_d, bn_d = r(Ce, 1, k, k) / k, bn()

    def fold(w, p):
        scale = p[0].double() / torch.sqrt(p[3].double() + effnet.BN_EPS)
        return (w.double() * scale.view(-1, 1, 1, 1)).float(), (p[1].double() - p[2].double() * scale).float()

    w_e, b_e = fold(conv_e, bn_e) if expand else (None, None)
    w_d, b_d = fold(conv_d, bn_d)
    w_e2 = w_e.reshape(Ce, Ci).contiguous() if expand else None
    w_d3 = w_d.reshape(Ce, k, k).contiguous()
    ops = {"hip": lambda: effnet.mbconv_front(x, w_e2, b_e, w_d3, b_d, k, stride),
           "folded": lambda: effnet.mbconv_front_torch(x, w_e, b_e, w_d, b_d, k, stride),
           "unfolded": lambda: unfolded_front(x, conv_e, bn_e, conv_d, bn_d, k, stride)}

    def fwd(op):
        with torch.no_grad():
            return op()

    def fwd_bwd(op, up):
        z, ssum = op()
        return torch.autograd.grad([z, ssum], x, up)[0]

    out = {kind: fwd(op) for kind, op in ops.items()}
    up = [torch.randn_like(out["folded"][0]), torch.randn_like(out["folded"][1])]
    grads = {kind: fwd_bwd(op, up) for kind, op in ops.items()}
    parity = {kind: {"z": rel_l2(out[kind][0], out["folded"][0]), "ssum": rel_l2(out[kind][1], out["folded"][1]),
                     "g_x": rel_l2(grads[kind], grads["folded"])} for kind in ("hip", "unfolded")}
    del out, grads
    variants = {f"{kind}_{what}": (lambda op=op, run=run: run(op)) for kind, op in ops.items()
                for what, run in (("fwd", fwd), ("fwd_bwd", lambda op: fwd_bwd(op, up)))}
    times = alternate(variants, rounds, iters)
    Ho, Wo = effnet.out_size(H, k, stride), effnet.out_size(W, k, stride)
    n_x, n_z, n_e = B * Ci * H * W, B * Ce * Ho * Wo, B * Ce * H * W
    row = {"block": name, "B": B, "Ci": Ci, "Ce": Ce, "H": H, "W": W, "k": k, "stride": stride, "expand": expand,
           "expanded_tensor_mb": 4 * n_e / 1e6 if expand else 0.0,
           "algorithmic_mb_fwd": 4 * (n_x + n_z) / 1e6, "algorithmic_mb_fwd_bwd": 4 * (3 * n_x + 3 * n_z) / 1e6,
           "gflop_fwd": 2.0 * ((Ci * n_e if expand else 0) + k * k * n_z) / 1e9, "parity_rel_l2_to_folded": parity}
    for kind, v in times.items():
        row[kind + "_ms"] = v
    row["hip_fwd_gb_per_s"] = row["algorithmic_mb_fwd"] / row["hip_fwd_ms"]["median"]
    row["hip_fwd_bwd_gb_per_s"] = row["algorithmic_mb_fwd_bwd"] / row["hip_fwd_bwd_ms"]["median"]
    t, hp = row["folded_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    row["admitted"] = bool(hp["median"] < t["median"] - t["spread"])
    return row


def probe_loss(B, H, W, dispatch, rounds, iters, float64=False):
    dev = "cuda"
    torch.manual_seed(B)
    feats = effnet.EffNetB0Features()
    with torch.no_grad():       # running statistics and affine terms away from the identity
        for key, t in feats.state_dict(keep_vars=True).items():
            if key.endswith("running_var"):
                t.copy_(0.5 + 1.5 * torch.rand(t.shape))
            elif t.dim() == 1:
                t.copy_((1.0 if key.endswith(".1.weight") else 0.0) + 0.3 * torch.randn(t.shape))
    feats = feats.to(dev)
    x = (torch.rand(B, 3, H, W, device=dev) * 330.0 - 40.0).requires_grad_(True)
    y = torch.rand(B, 3, H, W, device=dev) * 330.0 - 40.0
    mask = (torch.rand(B, 1, H, W, device=dev) > 0.3).float()
    net = effnet.EfficientNetLoss(feats)

    def run(kind):
        os.environ["GOLIATH_FUSED_EFFNET_ALL"] = "1" if kind == "all_fused" else "0"
        effnet.DISPATCH = dispatch if kind == "dispatch" else {}
        loss = effnet.effnet_loss_torch(feats, x, y, mask) if kind == "torch" else net(x, y, mask)
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
    if float64:     # how far the two fp32 paths are from the float64 twin at this size
        x64 = x.detach().double().requires_grad_(True)
        l64 = effnet.effnet_loss_torch(feats, x64, y.double(), mask.double())
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
    os.environ.pop("GOLIATH_FUSED_EFFNET_ALL", None)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1334)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--loss-batches", default="1,4")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "effnet_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("effnet_probe needs the GPU: there is nothing to measure without one")
    committed = dict(effnet.DISPATCH)
    rows = []
    for name, Ci, Ce, H, W, k, stride in front_shapes(args.height, args.width):
        row = probe_front(1, name, Ci, Ce, H, W, k, stride, args.rounds, args.iters)
        rows.append(row)
        print(f"{name} {Ci:3d}->{Ce:3d} @ {H}x{W} k{k} s{stride}  fwd hip {row['hip_fwd_ms']['median']:.3f} / folded "
              f"{row['folded_fwd_ms']['median']:.3f} / unfolded {row['unfolded_fwd_ms']['median']:.3f} ms  fwd+bwd hip "
              f"{row['hip_fwd_bwd_ms']['median']:.3f} / folded {row['folded_fwd_bwd_ms']['median']:.3f} (spread "
              f"{row['folded_fwd_bwd_ms']['spread']:.3f}) / unfolded {row['unfolded_fwd_bwd_ms']['median']:.3f} ms  "
              f"{row['hip_fwd_gb_per_s']:.0f} / {row['hip_fwd_bwd_gb_per_s']:.0f} GB/s  admitted={row['admitted']}  parity z "
              f"{row['parity_rel_l2_to_folded']['hip']['z']:.1e} g_x {row['parity_rel_l2_to_folded']['hip']['g_x']:.1e}",
              flush=True)
        torch.cuda.empty_cache()
    dispatch = [[r["Ci"], r["Ce"], r["H"], r["W"], r["k"], r["stride"]] for r in rows if r["admitted"]]
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
    effnet.DISPATCH = committed
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "rounds": args.rounds,
              "iters": args.iters, "fronts": rows, "dispatch": dispatch,
              "committed_dispatch_matches": sorted(map(list, committed)) == sorted(dispatch), "loss": losses}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
