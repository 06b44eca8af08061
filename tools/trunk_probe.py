#!/usr/bin/env python
"""Time the fused hidden decoder layer (goliath_amd.trunk.convt_ub_lrelu: gol_trunk_conv_fwd / _bwd) against the library
composition it replaces (F.conv_transpose2d + bias[None] + in-place leaky_relu) on the seven layer shapes of the reference
decoders at B = 8, forward and forward + backward, and derive the dispatch table of goliath_amd/trunk.py.

Method: every variant of a shape is warmed up, then the variants are timed alternately in ROUNDS rounds inside one process
(device events around ITERS back-to-back calls); reported are the median over the rounds and the spread (max - min over the
rounds).  A shape is admitted to the dispatch table only if the HIP operator's forward + backward median is below the torch
composition's by more than the torch composition's own spread.  Outputs and gradients of the two are compared at the timed
size (rel-L2).  Needs the GPU; there is no fallback.

Usage: python tools/trunk_probe.py [--batch 8] [--rounds 7] [--iters 10] [--out profiles/trunk_probe.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from goliath_amd import _lib, build, trunk
from goliath_amd._lib import c_float, c_int, fptr, stream_ptr

# (Ci, Co, h = w of the input): vnocond_mod / vcond_mod hidden layers (ca_code/models/rgca.py:408-426,429-454)
LAYERS = [(256, 256, 8), (264, 256, 8), (256, 128, 16), (128, 128, 32), (128, 64, 64), (64, 32, 128), (32, 16, 256)]
LEAK = 0.2


def torch_layer(x, weight, bias, leak=LEAK):
    return F.leaky_relu_(F.conv_transpose2d(x, weight, None, 2, 1) + bias[None], leak)


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


def pieces(B, Ci, Co, h, x, weight, bias, g, rounds, iters):
    """The HIP operator's kernels one by one through the C ABI (ms, median over the rounds)."""
    dims = (c_int(B), c_int(Ci), c_int(Co), c_int(h), c_int(h), c_float(LEAK))
    x, weight, bias = x.detach(), weight.detach(), bias.detach()
    y = torch.empty_like(g)
    wt = weight.permute(1, 3, 0, 2).contiguous()
    fn = _lib.load().gol_trunk_conv_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    scratch = torch.empty(int(fn(*dims[:5])), device=x.device)
    gx, gw, gb = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(bias)
    fwd = lambda: _lib.call("gol_trunk_conv_fwd", *dims, fptr(x), fptr(weight), fptr(bias), fptr(y), stream_ptr())
    bwd = lambda a, b2, c: (lambda: _lib.call("gol_trunk_conv_bwd", *dims, fptr(x), fptr(wt), fptr(y), fptr(g), fptr(a),
                                              fptr(b2), fptr(c), fptr(scratch), stream_ptr()))
    calls = {"fwd": fwd, "bwd_x": bwd(gx, None, None), "bwd_w": bwd(None, gw, None), "bwd_b": bwd(None, None, gb)}
    out = {}
    for k, call in calls.items():
        call()
        torch.cuda.synchronize()
        out[k] = statistics.median(timed(call, iters) for _ in range(rounds))
    return out


def probe(B, Ci, Co, h, rounds, iters):
    dev = "cuda"
    torch.manual_seed(Ci * 1000 + Co)
    x = torch.randn(B, Ci, h, h, device=dev, requires_grad=True)
    weight = (torch.randn(Ci, Co, 4, 4, device=dev) / (4.0 * Ci) ** 0.5).requires_grad_(True)
    bias = (0.5 * torch.randn(Co, 2 * h, 2 * h, device=dev)).requires_grad_(True)
    g = torch.randn(B, Co, 2 * h, 2 * h, device=dev)
    leaves = [x, weight, bias]
    ops = {"hip": trunk.convt_ub_lrelu, "torch": torch_layer}

    def fwd(op):
        with torch.no_grad():
            return op(x, weight, bias, LEAK)

    def fwd_bwd(op):
        return torch.autograd.grad(op(x, weight, bias, LEAK), leaves, g)

    variants = {f"{name}_{kind}": (lambda op=op, run=run: run(op))
                for name, op in ops.items() for kind, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
    y = {name: fwd(op) for name, op in ops.items()}
    grads = {name: fwd_bwd(op) for name, op in ops.items()}
    parity = {"y": rel_l2(y["hip"], y["torch"])}
    parity.update({n: rel_l2(a, b) for n, a, b in zip(("g_x", "g_weight", "g_bias"), grads["hip"], grads["torch"])})
    del y, grads
    for fn in variants.values():   # warm-up: code objects, the library's algorithm choice, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # alternate the variants inside every round
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    flop = 2.0 * B * h * h * 16 * Ci * Co
    n_x, n_w, n_b, n_y = B * Ci * h * h, Ci * Co * 16, Co * 4 * h * h, B * Co * 4 * h * h
    bytes_fwd = 4 * (n_x + n_w + n_b + n_y)
    bytes_bwd = 4 * ((n_x + n_w + 2 * n_y) + (n_x + n_w + n_b))   # reads x, W, y, g_y; writes the three gradients
    row = {"B": B, "Ci": Ci, "Co": Co, "h": h, "w": h, "gflop_fwd": flop / 1e9, "gflop_fwd_bwd": 3 * flop / 1e9,
           "algorithmic_mb_fwd": bytes_fwd / 1e6, "algorithmic_mb_fwd_bwd": (bytes_fwd + bytes_bwd) / 1e6, "parity_rel_l2": parity}
    for k, v in times.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    for name in ops:
        row[name + "_fwd_tflops"] = flop / row[name + "_fwd_ms"]["median"] / 1e9
        row[name + "_fwd_bwd_tflops"] = 3 * flop / row[name + "_fwd_bwd_ms"]["median"] / 1e9
    t, hp = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    row["hip_kernels_ms"] = pieces(B, Ci, Co, h, x, weight, bias, g, rounds, iters)
    row["admitted"] = bool(hp["median"] < t["median"] - t["spread"])
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "trunk_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trunk_probe needs the GPU: there is nothing to measure without one")
    rows = []
    for Ci, Co, h in LAYERS:
        row = probe(args.batch, Ci, Co, h, args.rounds, args.iters)
        rows.append(row)
        print(f"{Ci:3d}->{Co:3d} @ {h:3d}^2  fwd hip {row['hip_fwd_ms']['median']:.3f} / torch {row['torch_fwd_ms']['median']:.3f} ms"
              f"  fwd+bwd hip {row['hip_fwd_bwd_ms']['median']:.3f} / torch {row['torch_fwd_bwd_ms']['median']:.3f} ms"
              f" (torch spread {row['torch_fwd_bwd_ms']['spread']:.3f})  hip {row['hip_fwd_tflops']:.1f} / {row['hip_fwd_bwd_tflops']:.1f} TF"
              f"  kernels {' '.join(f'{k} {v:.3f}' for k, v in row['hip_kernels_ms'].items())}"
              f"  admitted={row['admitted']}  parity {max(row['parity_rel_l2'].values()):.1e}", flush=True)
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "batch": args.batch,
              "rounds": args.rounds, "iters": args.iters, "leak": LEAK, "layers": rows,
              "dispatch": [[r["Ci"], r["Co"], r["h"], r["w"]] for r in rows if r["admitted"]]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
