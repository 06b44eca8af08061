#!/usr/bin/env python
"""Time the split-bf16 UNet level of the MVP teacher (goliath_amd.olatunet.conv3_ub_lrelu: gol_conv3ub_pack / _fwd / _bwd_x /
_bwd_w / _bwd_bias) against what the parent commit runs for a level of OLATRGBDecoder.forward_rgb's UNet
(ca_code/models/hand_teacher_mvp.py:444-467) -- th.cat + F.conv2d + bias[None] add + leaky_relu_ and their autograd backward
in fp32 -- per layer shape of the model at UV 1024^2 with primitives 16 x 16 x 8, for B L = 5 (one chunk of light images) and
B L = 1: forward, each of the four gradients alone, and forward + backward (the operator's times include the pack), and derive
`DISPATCH` of goliath_amd/olatunet.py.  It also times the whole ten-level UNet forward + backward to joint_feat and every
parameter: the parent's path (precision="fp32") against precision="bf16x3" with the derived table, and with every level forced.

Method (that of tools/conv4x_probe.py): every variant is warmed up, then the variants are timed alternately in ROUNDS rounds
inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds and the spread
(max - min over the rounds) of BOTH sides.  A shape is admitted only if the operator's forward + backward median is below the
library's by more than the sum of both spreads, at B L = 5 AND at B L = 1 (the table has no batch in its key; DESIGN.md
section 6a).  The first level's input carries no gradient in the model (goliath_amd.olat.features), so its forward + backward
leaves g_xa out on both sides.  Outputs and gradients are compared at the timed size (rel-L2 against the fp32 library result);
the allocator's peak of a forward + backward is taken each way.  Needs the GPU; there is no fallback.

A step (--steps: layer0 .. layer9, unet) is one process; its result is merged into the output file, so that every step can run
under a time limit of its own:
    for s in layer0 ... layer9 unet; do timeout -k 10 300 python tools/olatunet_probe.py --steps $s || break; done

Usage: python tools/olatunet_probe.py [--steps layer0,...,unet] [--batches 5,1] [--rounds 5] [--iters 3] [--out ...]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import torch.nn.functional as F

from goliath_amd import build, olatunet, texdec

# (Ca, Cb, Co, S) of the ten levels at the model's size (hand_teacher_mvp.py:185-241): five encoder, five decoder levels
LAYERS = [(56, 0, 64, 1024), (64, 0, 64, 512), (64, 0, 64, 256), (64, 0, 64, 128), (64, 0, 64, 64),
          (64, 64, 64, 64), (64, 64, 64, 128), (64, 64, 64, 256), (64, 64, 64, 512), (64, 64, 32, 1024)]
LEAK = 0.2
GRADS = ("g_xa", "g_xb", "g_w", "g_bias")


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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 1e6


def library_level(xa, xb, w, bias):
    """The reference's lines for one level: th.cat, Conv2dWNUB's conv + bias[None], LeakyReLU(0.2, inplace=True)."""
    x = xa if xb is None else torch.cat([xa, xb], dim=1)
    return F.leaky_relu(F.conv2d(x, w, None, 1, 1) + bias[None], LEAK, inplace=True)


def wins(row):
    t, hp = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    return bool(hp["median"] < t["median"] - t["spread"] - hp["spread"])


def probe_layer(B, Ca, Cb, Co, S, rounds, iters):
    torch.manual_seed(B)
    Ci = Ca + Cb
    first = Cb == 0 and Ca % 32 != 0            # the model's first level: its input carries no gradient
    xa = torch.randn(B, Ca, S, S, device="cuda").requires_grad_(not first)
    xb = torch.randn(B, Cb, S, S, device="cuda").requires_grad_(True) if Cb else None
    w = (torch.randn(Co, Ci, 3, 3, device="cuda") / (9.0 * Ci) ** 0.5).requires_grad_(True)
    bias = (0.3 * torch.randn(Co, S, S, device="cuda")).requires_grad_(True)
    g = torch.randn(B, Co, S, S, device="cuda")
    leaves = {n: t for n, t in zip(GRADS, (xa, xb, w, bias)) if t is not None and t.requires_grad}
    levels = {"hip": lambda *a: olatunet.conv3_ub_lrelu(*a, LEAK), "torch": library_level}
    ops = {name: (lambda level=level: level(xa, xb, w, bias)) for name, level in levels.items()}

    def fwd(op):
        with torch.no_grad():
            return op()

    def fwd_bwd(op):
        return torch.autograd.grad(op(), list(leaves.values()), g)

    variants = {f"{name}_{kind}": (lambda op=op, run=run: run(op))
                for name, op in ops.items() for kind, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
    y = {name: fwd(op) for name, op in ops.items()}
    parity = {"y": rel_l2(y["hip"], y["torch"])}
    grads = {name: fwd_bwd(op) for name, op in ops.items()}
    parity.update({n: rel_l2(p, q) for n, p, q in zip(leaves, grads["hip"], grads["torch"])})
    del y, grads
    # each gradient alone: the backward of a kept graph in which only that leaf requires a gradient (the operator decides
    # what to launch by requires_grad at forward time; the library prunes by the same graph)
    kept = {}
    for name, level in levels.items():
        for n, leaf in leaves.items():
            args = [t if t is leaf or t is None else t.detach() for t in (xa, xb, w, bias)]
            kept[name, n] = level(*args)
            variants[f"{name}_{n}"] = lambda k=(name, n), leaf=leaf: torch.autograd.grad(kept[k], [leaf], g, retain_graph=True)
    for fn in variants.values():   # warm-up: code objects, the library's algorithm choice, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # alternate the variants inside every round
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    del kept
    gflop = 2.0 * B * Co * Ci * 9 * S * S / 1e9
    n_conv = 1 + len([n for n in ("g_w",) if n in leaves]) + (1 if "g_xa" in leaves or "g_xb" in leaves else 0)
    row = {"B": B, "Ca": Ca, "Cb": Cb, "Co": Co, "H": S, "W": S, "gflop_per_direction": gflop,
           "gradients": list(leaves), "parity_rel_l2": parity}
    for k, v in times.items():
        row[k + "_ms"] = stats(v)
        kind = k.split("_", 1)[1]
        if kind in ("fwd", "g_w", "g_xa", "g_xb"):   # algorithmic: an input gradient alone is its share of the channels
            share = {"g_xa": Ca / Ci, "g_xb": Cb / Ci}.get(kind, 1.0)
            row[k + "_tflops"] = gflop * share / statistics.median(v)
        elif kind == "fwd_bwd":
            row[k + "_tflops"] = gflop * n_conv / statistics.median(v)
    row["peak_memory_mb_fwd_bwd"] = {name: peak_mb(lambda op=op: fwd_bwd(op)) for name, op in ops.items()}
    row["scratch_mb"] = 4 * olatunet.bwd_w_scratch_floats(B, Ca, Cb, Co, S, S) / 1e6
    row["hip_wins_by_the_rule"] = wins(row)
    return row


class UNet(nn.Module):
    """The UNet attributes of OLATRGBDecoder at the model's size, built from texdec.Conv3WNUB (la.Conv2dWNUB's twin)."""

    def __init__(self):
        super().__init__()
        self.sizes = [1024, 512, 256, 128, 64]
        level = lambda ca, cb, co, s: nn.Sequential(texdec.Conv3WNUB(ca + cb, co, s, s), nn.LeakyReLU(LEAK, inplace=True))
        self.enc_layers = nn.ModuleList(level(*d) for d in LAYERS[:5])
        self.dec_layers = nn.ModuleList(level(*d) for d in LAYERS[5:])


def whole_unet(B, table, rounds, iters):
    torch.manual_seed(7)
    net = UNet().cuda()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 3:
                p.normal_(0, 0.3)
    x = torch.randn(B, 56, 1024, 1024, device="cuda")
    jf = torch.randn(B, 64, 64, 64, device="cuda").requires_grad_(True)
    leaves = [jf] + list(net.parameters())
    measured = {tuple(k): True for k in table}

    def run(mode):
        os.environ["GOLIATH_FUSED_OLATUNET_ALL"] = "1" if mode == "forced" else "0"
        olatunet.DISPATCH = measured
        out = olatunet.forward(net, x, jf, precision="fp32" if mode == "library" else "bf16x3")
        return out.detach(), torch.autograd.grad((out * out).sum(), leaves)

    modes = ("library", "table", "forced")
    saved = olatunet.DISPATCH
    try:
        ref = run("library")
        parity = {}
        for mode in modes[1:]:
            got = run(mode)
            parity[mode] = {"out": rel_l2(got[0], ref[0]), "grad_max": max(rel_l2(a, b) for a, b in zip(got[1], ref[1]))}
            del got
        del ref
        for mode in modes:
            run(mode)
        torch.cuda.synchronize()
        times = {m: [] for m in modes}
        for _ in range(rounds):
            for m in modes:
                times[m].append(timed(lambda m=m: run(m), max(1, iters // 2)))
        peak = {m: peak_mb(lambda m=m: run(m)) for m in modes}
    finally:
        os.environ.pop("GOLIATH_FUSED_OLATUNET_ALL", None)
        olatunet.DISPATCH = saved
    return {"B": B, "table": [list(k) for k in measured], "fwd_bwd_ms": {m: stats(v) for m, v in times.items()},
            "peak_memory_mb_fwd_bwd": peak, "parity_rel_l2_against_library": parity}


def dispatch_of(result, batches):
    """Admission: a shape whose rows win at EVERY measured batch."""
    rows = {}
    for r in result.get("layers", []):
        rows.setdefault((r["Ca"], r["Cb"], r["Co"], r["H"], r["W"]), {})[r["B"]] = r["hip_wins_by_the_rule"]
    return [list(k) for k, v in rows.items() if all(v.get(B, False) for B in batches)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", default=",".join([f"layer{i}" for i in range(len(LAYERS))] + ["unet"]))
    ap.add_argument("--batches", default="5,1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "olatunet_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("olatunet_probe needs the GPU: there is nothing to measure without one")
    digest = build.source_digest()
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    if result.get("source_digest") != digest:      # measured on other code: start over
        result = {}
    result.update(device=torch.cuda.get_device_name(0), source_digest=digest, rounds=args.rounds, iters=args.iters)
    result.setdefault("layers", [])
    result.setdefault("unet", [])
    batches = list(map(int, args.batches.split(",")))
    key = lambda r: (r["B"], r["Ca"], r["Cb"], r["Co"], r["H"])
    for step in args.steps.split(","):
        for B in batches:
            if step.startswith("layer"):
                dims = LAYERS[int(step[len("layer"):])]
                row = probe_layer(B, *dims, args.rounds, args.iters)
                result["layers"] = [r for r in result["layers"] if key(r) != (B, *dims)] + [row]
                ms = lambda k: "%.3f" % row[k + "_ms"]["median"] if k + "_ms" in row else "-"
                print(f"B={B} {dims[0]}+{dims[1]}->{dims[2]} @ {dims[3]}^2  "
                      + "  ".join(f"{k} hip {ms('hip_' + k)} / torch {ms('torch_' + k)}" for k in ("fwd",) + GRADS)
                      + f"  fwd+bwd hip {ms('hip_fwd_bwd')} (spread {row['hip_fwd_bwd_ms']['spread']:.3f}, "
                      f"{row['hip_fwd_bwd_tflops']:.0f} TF) / torch {ms('torch_fwd_bwd')} (spread "
                      f"{row['torch_fwd_bwd_ms']['spread']:.3f}, {row['torch_fwd_bwd_tflops']:.0f} TF)  peak MB hip "
                      f"{row['peak_memory_mb_fwd_bwd']['hip']:.0f} / torch {row['peak_memory_mb_fwd_bwd']['torch']:.0f}  "
                      f"wins={row['hip_wins_by_the_rule']}  parity {max(row['parity_rel_l2'].values()):.1e}", flush=True)
            elif step == "unet":
                un = whole_unet(B, dispatch_of(result, batches), args.rounds, args.iters)
                result["unet"] = [e for e in result["unet"] if e["B"] != B] + [un]
                print(f"B={B} whole UNet fwd+bwd ms: "
                      + "  ".join(f"{m} {v['median']:.3f} (spread {v['spread']:.3f})" for m, v in un["fwd_bwd_ms"].items())
                      + "  peak MB " + "  ".join(f"{m} {v:.0f}" for m, v in un["peak_memory_mb_fwd_bwd"].items())
                      + f"  table {un['table']}", flush=True)
            else:
                raise SystemExit(f"unknown step {step!r}")
            torch.cuda.empty_cache()
    result["layers"].sort(key=lambda r: (-r["B"], LAYERS.index((r["Ca"], r["Cb"], r["Co"], r["H"]))))
    result["unet"].sort(key=lambda e: -e["B"])
    result["dispatch"] = dispatch_of(result, batches)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out, "dispatch", result["dispatch"])


if __name__ == "__main__":
    main()
