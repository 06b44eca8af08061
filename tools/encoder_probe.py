#!/usr/bin/env python
"""Time the fused encoder layer (goliath_amd.encoder.conv_ub_lrelu: gol_enc_conv_fwd / _bwd) against the library composition
it replaces (F.conv2d + bias[None] + in-place leaky_relu; for the first layer behind `color / 255.0 - 0.5`) on the eight
layer shapes of the reference encoder at B = 8, forward and forward + backward, and derive the dispatch table of
goliath_amd/encoder.py.

Method (that of tools/trunk_probe.py): every variant of a shape is warmed up, then the variants are timed alternately in
ROUNDS rounds inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds
and the spread (max - min over the rounds).  A shape is admitted to the dispatch table only if the HIP operator's forward +
backward median is below the torch composition's by more than the torch composition's own spread.  The first layer is
timed without an input gradient, as the model runs it (its input is data).  Outputs and gradients of the two are compared
at the timed size (rel-L2; the gradients with the upstream gradient zeroed within 1e-4 of the LeakyReLU kink, as the tests
do).  The operator's kernels are also timed one by one through the C ABI, with the bytes and FLOP the algorithm needs and
the rates they give.  Needs the GPU; there is no fallback.

Usage: python tools/encoder_probe.py [--batch 8] [--rounds 7] [--iters 10] [--out profiles/encoder_probe.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from goliath_amd import _lib, build, encoder
from goliath_amd._lib import c_float, c_int, fptr, stream_ptr

# (Ci, Co, H = W of the input): texmod (ca_code/models/rgca.py:281-298)
LAYERS = [(3, 32, 1024), (32, 32, 512), (32, 64, 256), (64, 64, 128), (64, 128, 64), (128, 128, 32), (128, 256, 16),
          (256, 256, 8)]
LEAK = 0.2
KINK = 1e-4


def torch_layer(x, weight, bias, leak, in_scale, in_shift):
    if in_scale != 1.0 or in_shift != 0.0:
        x = x / 255.0 - 0.5                                   # rgca.py:314
    return F.leaky_relu_(F.conv2d(x, weight, None, 2, 1) + bias[None], leak)


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


def pieces(B, Ci, Co, H, affine, x, weight, bias, g, want_gx, rounds, iters):
    """The HIP operator's kernels one by one through the C ABI: ms (median over the rounds), algorithmic MB and GFLOP."""
    dims = (c_int(B), c_int(Ci), c_int(Co), c_int(H), c_int(H), c_float(LEAK), c_float(affine[0]), c_float(affine[1]))
    x, weight, bias = x.detach(), weight.detach(), bias.detach()
    y = torch.empty_like(g)
    fn = _lib.load().gol_enc_conv_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    scratch = torch.empty(int(fn(*dims[:5])), device=x.device)
    gx, gw, gb = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(bias)
    fwd = lambda: _lib.call("gol_enc_conv_fwd", *dims, fptr(x), fptr(weight), fptr(bias), fptr(y), stream_ptr())
    bwd = lambda a, b2, c: (lambda: _lib.call("gol_enc_conv_bwd", *dims, fptr(x), fptr(weight), fptr(y), fptr(g), fptr(a),
                                              fptr(b2), fptr(c), fptr(scratch), stream_ptr()))
    n_x, n_w, n_b, n_y = x.numel(), weight.numel(), bias.numel(), g.numel()
    flop = 2.0 * n_y * 16 * Ci
    calls = {"fwd": (fwd, n_x + n_w + n_b + n_y, flop), "bwd_w": (bwd(None, gw, None), n_x + 2 * n_y + n_w, flop),
             "bwd_b": (bwd(None, None, gb), 2 * n_y + n_b, 2.0 * n_y)}
    if want_gx:
        calls["bwd_x"] = (bwd(gx, None, None), 2 * n_y + n_w + n_x, flop)
    out = {}
    for k, (call, floats, fl) in calls.items():
        call()
        torch.cuda.synchronize()
        ms = statistics.median(timed(call, iters) for _ in range(rounds))
        out[k] = {"ms": ms, "algorithmic_mb": 4 * floats / 1e6, "gflop": fl / 1e9, "tb_per_s": 4 * floats / ms / 1e9,
                  "tflops": fl / ms / 1e9}
    return out


def probe(B, Ci, Co, H, rounds, iters):
    dev = "cuda"
    first = Ci == 3
    affine = (1.0 / 255.0, -0.5) if first else (1.0, 0.0)
    torch.manual_seed(Ci * 1000 + Co)
    x = (255.0 * torch.rand(B, Ci, H, H, device=dev)) if first else torch.randn(B, Ci, H, H, device=dev, requires_grad=True)
    weight = (torch.randn(Co, Ci, 4, 4, device=dev) / (16.0 * Ci) ** 0.5).requires_grad_(True)
    bias = (0.5 * torch.randn(Co, H // 2, H // 2, device=dev)).requires_grad_(True)
    g = torch.randn(B, Co, H // 2, H // 2, device=dev)
    leaves = [weight, bias] if first else [x, weight, bias]
    names = ("g_weight", "g_bias") if first else ("g_x", "g_weight", "g_bias")
    ops = {"hip": encoder.conv_ub_lrelu, "torch": torch_layer}

    def fwd(op):
        with torch.no_grad():
            return op(x, weight, bias, LEAK, *affine)

    def fwd_bwd(op, up=g):
        return torch.autograd.grad(op(x, weight, bias, LEAK, *affine), leaves, up)

    variants = {f"{name}_{kind}": (lambda op=op, run=run: run(op))
                for name, op in ops.items() for kind, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
    y = {name: fwd(op) for name, op in ops.items()}
    # gradient parity with the upstream gradient zeroed where the pre-activation is within KINK of the LeakyReLU kink: two
    # fp32 paths legitimately disagree on the mask of an element whose pre-activation is a rounding error away from zero
    keep = (y["torch"] > KINK) | (y["torch"] < -LEAK * KINK)
    grads = {name: fwd_bwd(op, g * keep) for name, op in ops.items()}
    parity = {"y": rel_l2(y["hip"], y["torch"]), "zeroed_share": 1.0 - float(keep.double().mean())}
    parity.update({n: rel_l2(a, b) for n, a, b in zip(names, grads["hip"], grads["torch"])})
    del y, grads, keep
    for fn in variants.values():   # warm-up: code objects, the library's algorithm choice, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # alternate the variants inside every round
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    n_x, n_w, n_b, n_y = x.numel(), weight.numel(), bias.numel(), g.numel()
    flop = 2.0 * n_y * 16 * Ci
    gemms = 2 if first else 3      # forward, weight gradient and (not for the first layer) input gradient
    bytes_fwd = 4 * (n_x + n_w + n_b + n_y)
    bytes_bwd = 4 * ((n_x + n_w + 2 * n_y) + (n_w + n_b) + (0 if first else n_x))   # reads x, W, y, g_y; writes the gradients
    row = {"B": B, "Ci": Ci, "Co": Co, "H": H, "W": H, "input_affine": first, "input_gradient": not first,
           "gflop_fwd": flop / 1e9, "gflop_fwd_bwd": gemms * flop / 1e9, "algorithmic_mb_fwd": bytes_fwd / 1e6,
           "algorithmic_mb_fwd_bwd": (bytes_fwd + bytes_bwd) / 1e6, "parity_rel_l2": parity}
    for k, v in times.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    for name in ops:
        row[name + "_fwd_tflops"] = flop / row[name + "_fwd_ms"]["median"] / 1e9
        row[name + "_fwd_bwd_tflops"] = gemms * flop / row[name + "_fwd_bwd_ms"]["median"] / 1e9
        row[name + "_fwd_tb_per_s"] = bytes_fwd / row[name + "_fwd_ms"]["median"] / 1e9
    t, hp = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    row["hip_kernels"] = pieces(B, Ci, Co, H, affine, x, weight, bias, g, not first, rounds, iters)
    row["admitted"] = bool(hp["median"] < t["median"] - t["spread"])
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "encoder_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encoder_probe needs the GPU: there is nothing to measure without one")
    rows = []
    for Ci, Co, H in LAYERS:
        row = probe(args.batch, Ci, Co, H, args.rounds, args.iters)
        rows.append(row)
        kernels = " ".join("%s %.3f" % (k, v["ms"]) for k, v in row["hip_kernels"].items())
        print(f"{Ci:3d}->{Co:3d} @ {H:4d}^2  fwd hip {row['hip_fwd_ms']['median']:.3f} / torch {row['torch_fwd_ms']['median']:.3f} ms"
              f"  fwd+bwd hip {row['hip_fwd_bwd_ms']['median']:.3f} / torch {row['torch_fwd_bwd_ms']['median']:.3f} ms"
              f" (torch spread {row['torch_fwd_bwd_ms']['spread']:.3f})  hip {row['hip_fwd_tflops']:.1f} / {row['hip_fwd_bwd_tflops']:.1f} TF"
              f"  kernels {kernels}"
              f"  admitted={row['admitted']}  parity {max(v for k, v in row['parity_rel_l2'].items() if k != 'zeroed_share'):.1e}", flush=True)
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "batch": args.batch,
              "rounds": args.rounds, "iters": args.iters, "leak": LEAK, "layers": rows,
              "dispatch": [[r["Ci"], r["Co"], r["H"], r["W"]] for r in rows if r["admitted"]]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
