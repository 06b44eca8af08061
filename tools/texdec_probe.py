#!/usr/bin/env python
"""Time the fused texture-decoder layer (goliath_amd.texdec.upconv_lrelu / upconv_gated: gol_upconv_fwd / _bwd) against the
library composition it replaces -- the lines of the two loops of goliath_amd/urhand.py (the reference's
ca_code/models/urhand.py:583-608): F.interpolate(bilinear, align_corners=True) to twice the size, F.conv2d(3x3, s1, p1) and
`+ bias[None]`, leaky_relu (mode 0, texmod0) or `* acts[i]`, `(x + gainbias[i]) * 0.707107` for the first four layers
(mode 1, texmod1) -- on the 14 (mode, layer) shapes of URHand's texture decoder at B = 1 (BASELINE config 4's frames per
GPU), forward and forward + backward, and derive the dispatch table of goliath_amd/texdec.py.

Method (that of tools/encoder_probe.py): every variant of a shape is warmed up, then the variants are timed alternately in
ROUNDS rounds inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds
and the spread (max - min over the rounds).  A shape is admitted to the dispatch table only if the HIP operator's forward +
backward median is below the torch composition's by more than the torch composition's own spread.
Outputs and gradients of the two are compared at the timed size (rel-L2; mode 0 with the upstream gradient zeroed within
1e-4 of the LeakyReLU kink, as the tests do).  The operator's kernels are also timed one by one through the C ABI, with the
bytes the algorithm needs and the rate they give.  Needs the GPU; there is no fallback.

Usage: python tools/texdec_probe.py [--batch 1] [--rounds 7] [--iters 5] [--out profiles/texdec_probe.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from goliath_amd import _lib, build, texdec
from goliath_amd._lib import c_float, c_int, fptr, stream_ptr

LEAK = 0.2
KINK = 1e-4
N_GAINBIAS = 4          # urhand.py:604: the layers of the linear branch that have a gainbias add it (the first four)


def torch_lrelu(x, weight, bias):
    hh = 2 * x.shape[2]
    x = F.interpolate(x, (hh, hh), mode="bilinear", align_corners=True)
    return F.leaky_relu(F.conv2d(x, weight, None, 1, 1) + bias[None], LEAK)


def torch_gated(x, weight, gate, gb=None):
    hh = 2 * x.shape[2]
    x = F.interpolate(x, (hh, hh), mode="bilinear", align_corners=True)
    x = F.conv2d(x, weight, None, 1, 1) * gate
    if gb is not None:
        x = (x + gb) * 0.707107
    return x


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


def pieces(mode, B, Ci, Co, Hi, scale, x, weight, a, gb, g, rounds, iters):
    """The HIP operator's kernels one by one through the C ABI: ms (median over the rounds) and algorithmic MB."""
    dims = (c_int(B), c_int(Ci), c_int(Co), c_int(Hi), c_int(Hi), c_int(mode), c_float(LEAK), c_float(scale))
    x, weight, a = x.detach(), weight.detach(), a.detach()
    gb = None if gb is None else gb.detach()
    y = torch.empty_like(g)
    fn = _lib.load().gol_upconv_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    scratch = torch.empty(int(fn(*dims[:5])), device=x.device)
    gx, gw, ga, ggb = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(a), torch.empty_like(g)
    bias, gate = (a, None) if mode == 0 else (None, a)
    fwd = lambda: _lib.call("gol_upconv_fwd", *dims, fptr(x), fptr(weight), fptr(bias), fptr(gate), fptr(gb), fptr(y),
                            stream_ptr())

    def bwd(o_x=None, o_w=None, o_b=None, o_gate=None, o_gb=None):
        return lambda: _lib.call("gol_upconv_bwd", *dims, fptr(x), fptr(weight), fptr(y if mode == 0 else None), fptr(gate),
                                 fptr(g), fptr(o_x), fptr(o_w), fptr(o_b), fptr(o_gate), fptr(o_gb), fptr(scratch),
                                 stream_ptr())

    n_x, n_w, n_a, n_y = x.numel(), weight.numel(), a.numel(), g.numel()
    calls = {"fwd": (fwd, n_x + n_w + n_a + n_y + (n_y if gb is not None else 0)),
             "bwd_x": (bwd(o_x=gx), 2 * n_y + n_w + n_x), "bwd_w": (bwd(o_w=gw), n_x + 2 * n_y + n_w)}
    if mode == 0:
        calls["bwd_bias"] = (bwd(o_b=ga), 2 * n_y + n_a)
    else:
        calls["bwd_gate"] = (bwd(o_gate=ga, o_gb=ggb if gb is not None else None),
                             n_x + n_w + n_y + n_y + (n_y if gb is not None else 0))
    out = {}
    fwd()
    for k, (call, floats) in calls.items():
        call()
        torch.cuda.synchronize()
        ms = statistics.median(timed(call, iters) for _ in range(rounds))
        out[k] = {"ms": ms, "algorithmic_mb": 4 * floats / 1e6, "tb_per_s": 4 * floats / ms / 1e9}
    return out


def probe(mode, layer, B, rounds, iters):
    dev = "cuda"
    Ci, Co = texdec.CHANNELS[layer]
    Hi = 32 << layer
    H = 2 * Hi
    with_gb = mode == 1 and layer < N_GAINBIAS
    scale = 0.707107 if with_gb else 1.0
    torch.manual_seed(1000 * mode + layer)
    x = torch.randn(B, Ci, Hi, Hi, device=dev, requires_grad=True)
    weight = (torch.randn(Co, Ci, 3, 3, device=dev) / (9.0 * Ci) ** 0.5).requires_grad_(True)
    g = torch.randn(B, Co, H, H, device=dev)
    if mode == 0:
        a = (0.5 * torch.randn(Co, H, H, device=dev)).requires_grad_(True)
        leaves, names = [x, weight, a], ("g_x", "g_weight", "g_bias")
        ops = {"hip": lambda: texdec.upconv_lrelu(x, weight, a, LEAK), "torch": lambda: torch_lrelu(x, weight, a)}
        gb = None
    else:
        a = torch.randn(B, Co, H, H, device=dev, requires_grad=True)
        gb = torch.randn(B, Co, H, H, device=dev, requires_grad=True) if with_gb else None
        leaves = [x, weight, a] + ([gb] if with_gb else [])
        names = ("g_x", "g_weight", "g_gate", "g_gb")[:len(leaves)]
        ops = {"hip": lambda: texdec.upconv_gated(x, weight, a, gb, scale), "torch": lambda: torch_gated(x, weight, a, gb)}

    def fwd(op):
        with torch.no_grad():
            return op()

    def fwd_bwd(op, up=g):
        return torch.autograd.grad(op(), leaves, up)

    variants = {f"{name}_{kind}": (lambda op=op, run=run: run(op))
                for name, op in ops.items() for kind, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
    y = {name: fwd(op) for name, op in ops.items()}
    parity = {"y": rel_l2(y["hip"], y["torch"])}
    up = g
    if mode == 0:   # two fp32 paths legitimately disagree on the mask of an element a rounding error away from the kink
        keep = (y["torch"] > KINK) | (y["torch"] < -LEAK * KINK)
        parity["zeroed_share"] = 1.0 - float(keep.double().mean())
        up = g * keep
    grads = {name: fwd_bwd(op, up) for name, op in ops.items()}
    parity.update({n: rel_l2(p, q) for n, p, q in zip(names, grads["hip"], grads["torch"])})
    del y, grads, up
    for fn in variants.values():   # warm-up: code objects, the library's algorithm choice, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # alternate the variants inside every round
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    n_x, n_w, n_a, n_y = x.numel(), weight.numel(), a.numel(), g.numel()
    n_gb = n_y if with_gb else 0
    bytes_fwd = 4 * (n_x + n_w + n_a + n_gb + n_y)
    # backward: g_x reads g_y, aux, W; g_w reads x, g_y, aux; the bias / gate gradient reads g_y (+ y, or x and W); writes
    bytes_bwd = 4 * ((2 * n_y + n_w + n_x) + (n_x + 2 * n_y + n_w) + (2 * n_y + n_a if mode == 0 else n_x + n_w + 2 * n_y + n_gb))
    # the composition also writes and reads the upsampled tensor (4 n_x floats) each way, and its elementwise passes
    row = {"mode": mode, "layer": layer, "B": B, "Ci": Ci, "Co": Co, "Hi": Hi, "Wi": Hi, "gainbias": with_gb,
           "gflop_fwd": 2.0 * n_y * 9 * Ci / 1e9, "algorithmic_mb_fwd": bytes_fwd / 1e6,
           "algorithmic_mb_fwd_bwd": (bytes_fwd + bytes_bwd) / 1e6, "upsampled_mb": 16 * n_x / 1e6, "parity_rel_l2": parity}
    for k, v in times.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}
    t, hp = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    row["hip_kernels"] = pieces(mode, B, Ci, Co, Hi, scale, x, weight, a, gb, g, rounds, iters)
    row["admitted"] = bool(hp["median"] < t["median"] - t["spread"])
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", default="0,1,2,3,4,5,6")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "texdec_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texdec_probe needs the GPU: there is nothing to measure without one")
    rows = []
    for mode in (0, 1):
        for layer in map(int, args.layers.split(",")):
            row = probe(mode, layer, args.batch, args.rounds, args.iters)
            rows.append(row)
            kernels = " ".join("%s %.3f" % (k, v["ms"]) for k, v in row["hip_kernels"].items())
            print(f"mode {mode} {row['Ci']:3d}->{row['Co']:3d} @ {row['Hi']:4d}^2  fwd hip {row['hip_fwd_ms']['median']:.3f} / torch "
                  f"{row['torch_fwd_ms']['median']:.3f} ms  fwd+bwd hip {row['hip_fwd_bwd_ms']['median']:.3f} / torch "
                  f"{row['torch_fwd_bwd_ms']['median']:.3f} ms (torch spread {row['torch_fwd_bwd_ms']['spread']:.3f})"
                  f"  kernels {kernels}  admitted={row['admitted']}"
                  f"  parity {max(v for k, v in row['parity_rel_l2'].items() if k != 'zeroed_share'):.1e}", flush=True)
            del row
            torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "batch": args.batch,
              "rounds": args.rounds, "iters": args.iters, "leak": LEAK, "layers": rows,
              "dispatch": [[r["mode"], r["Ci"], r["Co"], r["Hi"], r["Wi"]] for r in rows if r["admitted"]]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
