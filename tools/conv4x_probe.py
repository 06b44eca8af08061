#!/usr/bin/env python
"""Time the split-bf16 4x4 / stride 2 / pad 1 convolution (goliath_amd.featenc.conv4s2: gol_conv4x_pack / _fwd / _bwd_x /
_bwd_w) against what the parent commit runs for the feature layers feat_mod[0..3] of URHand's FeatEncoderUNet --
F.conv2d(x, w, None, 2, 1) and its autograd backward in fp32 (ca_code/models/urhand.py:93, :102) -- per layer shape of the
model at UV 1024^2, for B = 1 and B = 4, forward and forward + backward to x and to w (the operator's times include the
pack), and derive `DISPATCH_BF16X3` of goliath_amd/featenc.py.  It also times the whole FeatEncoderUNet(1, 3, 128) forward +
backward to every parameter: the library lines against precision="bf16x3" with the derived table, and with every layer forced.

Method (that of tools/vggx_probe.py / tools/featenc_probe.py): every variant is warmed up, then the variants are timed
alternately in ROUNDS rounds inside one process (device events around ITERS back-to-back calls); reported are the median over
the rounds and the spread (max - min over the rounds).  A shape is admitted only if the operator's forward + backward median
is below the library's by more than the library's own spread, at B = 1.  Outputs and gradients are
compared at the timed size (rel-L2 against the fp32 library result); the operator's kernels are also timed one by one
through the C ABI; the allocator's peak of a forward + backward is taken each way.  Needs the GPU; there is no fallback.

A step (--steps: layer0 .. layer3, encoder) is one process; its result is merged into the output file, so that every step
can run under a time limit of its own:
    for s in layer0 layer1 layer2 layer3 encoder; do timeout -k 10 300 python tools/conv4x_probe.py --steps $s || break; done

Usage: python tools/conv4x_probe.py [--steps layer0,...,encoder] [--batches 1,4] [--rounds 7] [--iters 5] [--out ...]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from goliath_amd import build, featenc

# (Ci, Co, H, W) of the input of feat_mod[0..3] at the model's size
LAYERS = [(64, 192, 1024, 1024), (192, 384, 512, 512), (384, 384, 256, 256), (384, 768, 128, 128)]
CX, SIZE, OUT_CH = 4, 1024, 128


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


def pieces(B, Ci, Co, H, W, x, w, g, rounds, iters):
    """The operator's kernels through the C ABI, one by one (ms, median over the rounds; algorithmic TF)."""
    d = dict(B=B, Ci=Ci, Co=Co, H=H, W=W)
    x, w = x.detach(), w.detach()
    packed = torch.empty(featenc.conv4x_packed_elems(Co, Ci), device=x.device, dtype=torch.int16)
    n_scratch = featenc.conv4x_bwd_w_scratch_floats(**d)
    scratch = torch.empty(n_scratch, device=x.device)
    y, g_x, g_w = torch.empty_like(g), torch.empty_like(x), torch.empty_like(w)
    calls = {"pack": lambda: featenc._abi_conv4x_pack(Co=Co, Ci=Ci, weight=w, packed=packed),
             "fwd": lambda: featenc._abi_conv4x_fwd(**d, x=x, packed=packed, y=y),
             "bwd_x": lambda: featenc._abi_conv4x_bwd_x(**d, packed=packed, g_y=g, g_x=g_x),
             "bwd_w": lambda: featenc._abi_conv4x_bwd_w(**d, x=x, g_y=g, g_w=g_w, scratch=scratch)}
    gflop = 2.0 * B * Co * Ci * 16 * (H // 2) * (W // 2) / 1e9
    out = {"scratch_mb": 4 * n_scratch / 1e6, "gflop_per_direction": gflop}
    for k, call in calls.items():
        call()
        torch.cuda.synchronize()
        ms = statistics.median(timed(call, iters) for _ in range(rounds))
        out[k] = {"ms": ms} if k == "pack" else {"ms": ms, "tflops": gflop / ms}
    return out


def probe_layer(B, Ci, Co, H, W, rounds, iters):
    torch.manual_seed(B)
    x = torch.randn(B, Ci, H, W, device="cuda").requires_grad_(True)
    w = (torch.randn(Co, Ci, 4, 4, device="cuda") / (16.0 * Ci) ** 0.5).requires_grad_(True)
    g = torch.randn(B, Co, H // 2, W // 2, device="cuda")
    ops = {"hip": lambda: featenc.conv4s2(x, w), "torch": lambda: F.conv2d(x, w, None, 2, 1)}

    def fwd(op):
        with torch.no_grad():
            return op()

    def fwd_bwd(op):
        return torch.autograd.grad(op(), [x, w], g)

    variants = {f"{name}_{kind}": (lambda op=op, run=run: run(op))
                for name, op in ops.items() for kind, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
    y = {name: fwd(op) for name, op in ops.items()}
    parity = {"y": rel_l2(y["hip"], y["torch"])}
    grads = {name: fwd_bwd(op) for name, op in ops.items()}
    parity.update({n: rel_l2(p, q) for n, p, q in zip(("g_x", "g_w"), grads["hip"], grads["torch"])})
    del y, grads
    for fn in variants.values():   # warm-up: code objects, the library's algorithm choice, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # alternate the variants inside every round
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    gflop = 2.0 * B * Co * Ci * 16 * (H // 2) * (W // 2) / 1e9
    row = {"B": B, "Ci": Ci, "Co": Co, "H": H, "W": W, "gflop_fwd": gflop, "parity_rel_l2": parity}
    for k, v in times.items():
        row[k + "_ms"] = stats(v)
        row[k + "_tflops"] = gflop * (3 if k.endswith("fwd_bwd") else 1) / statistics.median(v)
    row["peak_memory_mb_fwd_bwd"] = {name: peak_mb(lambda op=op: fwd_bwd(op)) for name, op in ops.items()}
    row["hip_kernels"] = pieces(B, Ci, Co, H, W, x, w, g, rounds, iters)
    t, hp = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    row["hip_wins_by_the_rule"] = bool(hp["median"] < t["median"] - t["spread"])
    return row


def whole_encoder(B, table, rounds, iters):
    """FeatEncoderUNet(1, 3, 128) forward + backward to every parameter at 1024^2: the library lines, precision="bf16x3" with
    `table` as DISPATCH_BF16X3, and with every feat_mod layer forced onto the operator."""
    torch.manual_seed(7)
    fe = featenc.FeatEncoderUNet(1, CX - 1, OUT_CH).cuda()
    x = torch.randn(B, CX, SIZE, SIZE, device="cuda")
    params = list(fe.parameters())
    measured = {tuple(k): True for k in table}

    def run(mode):
        os.environ["GOLIATH_FUSED_FEATENC_ALL"] = "1" if mode == "forced" else "0"
        featenc.DISPATCH_BF16X3 = measured
        z, gb = featenc.forward(fe, x, op=False, precision="fp32" if mode == "library" else "bf16x3")
        loss = z.sum() + sum((b * b).sum() for b in gb)
        grads = torch.autograd.grad(loss, params)
        return z.detach(), [b.detach() for b in gb], grads

    modes = ("library", "table", "forced")
    saved = featenc.DISPATCH_BF16X3
    try:
        ref = run("library")
        parity = {}
        for mode in modes[1:]:
            got = run(mode)
            parity[mode] = {"z": rel_l2(got[0], ref[0]), "gb_max": max(rel_l2(a, b) for a, b in zip(got[1], ref[1])),
                            "grad_max": max(rel_l2(a, b) for a, b in zip(got[2], ref[2]))}
            del got
        del ref
        for mode in modes:
            for _ in range(2):
                run(mode)
        torch.cuda.synchronize()
        times = {m: [] for m in modes}
        for _ in range(rounds):
            for m in modes:
                times[m].append(timed(lambda m=m: run(m), max(1, iters // 2)))
        peak = {m: peak_mb(lambda m=m: run(m)) for m in modes}
    finally:
        os.environ.pop("GOLIATH_FUSED_FEATENC_ALL", None)
        featenc.DISPATCH_BF16X3 = saved
    return {"B": B, "size": SIZE, "out_ch": OUT_CH, "table": [list(k) for k in measured],
            "fwd_bwd_ms": {m: stats(v) for m, v in times.items()}, "peak_memory_mb_fwd_bwd": peak,
            "parity_rel_l2_against_library": parity}


def dispatch_of(result):
    """Admission by the rows at B = 1."""
    return [[r["Ci"], r["Co"], r["H"], r["W"]] for r in result.get("layers", []) if r["B"] == 1 and r["hip_wins_by_the_rule"]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", default="layer0,layer1,layer2,layer3,encoder")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "conv4x_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv4x_probe needs the GPU: there is nothing to measure without one")
    digest = build.source_digest()
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    if result.get("source_digest") != digest:      # measured on other code: start over
        result = {}
    result.update(device=torch.cuda.get_device_name(0), source_digest=digest, rounds=args.rounds, iters=args.iters)
    result.setdefault("layers", [])
    result.setdefault("encoder", [])
    batches = list(map(int, args.batches.split(",")))
    for step in args.steps.split(","):
        for B in batches:
            if step.startswith("layer"):
                dims = LAYERS[int(step[len("layer"):])]
                row = probe_layer(B, *dims, args.rounds, args.iters)
                result["layers"] = [r for r in result["layers"] if (r["B"], r["Ci"], r["Co"], r["H"], r["W"]) != (B, *dims)]
                result["layers"].append(row)
                kernels = " ".join("%s %.3f" % (k, v["ms"]) for k, v in row["hip_kernels"].items() if isinstance(v, dict))
                print(f"B={B} {dims[0]}->{dims[1]} @ {dims[2]}^2  fwd hip {row['hip_fwd_ms']['median']:.3f} / torch "
                      f"{row['torch_fwd_ms']['median']:.3f} ms  fwd+bwd hip {row['hip_fwd_bwd_ms']['median']:.3f} (spread "
                      f"{row['hip_fwd_bwd_ms']['spread']:.3f}, {row['hip_fwd_bwd_tflops']:.0f} TF) / torch "
                      f"{row['torch_fwd_bwd_ms']['median']:.3f} ms (spread {row['torch_fwd_bwd_ms']['spread']:.3f}, "
                      f"{row['torch_fwd_bwd_tflops']:.0f} TF)  peak MB hip {row['peak_memory_mb_fwd_bwd']['hip']:.0f} / torch "
                      f"{row['peak_memory_mb_fwd_bwd']['torch']:.0f}  kernels {kernels}  wins={row['hip_wins_by_the_rule']}  "
                      f"parity {max(row['parity_rel_l2'].values()):.1e}", flush=True)
            elif step == "encoder":
                enc = whole_encoder(B, dispatch_of(result), args.rounds, args.iters)
                result["encoder"] = [e for e in result["encoder"] if e["B"] != B] + [enc]
                print(f"B={B} whole encoder fwd+bwd ms: "
                      + "  ".join(f"{m} {v['median']:.3f} (spread {v['spread']:.3f})" for m, v in enc["fwd_bwd_ms"].items())
                      + "  peak MB " + "  ".join(f"{m} {v:.0f}" for m, v in enc["peak_memory_mb_fwd_bwd"].items())
                      + f"  table {enc['table']}", flush=True)
            else:
                raise SystemExit(f"unknown step {step!r}")
            torch.cuda.empty_cache()
    result["layers"].sort(key=lambda r: (r["B"], -r["H"]))
    result["encoder"].sort(key=lambda e: e["B"])
    result["dispatch"] = dispatch_of(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out, "dispatch", result["dispatch"])


if __name__ == "__main__":
    main()
