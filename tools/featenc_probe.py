#!/usr/bin/env python
"""Time the fused front of URHand's FeatEncoderUNet (goliath_amd.featenc.front: gol_featenc_front_fwd / _bwd) against the two
library convolutions it replaces -- the reference's ca_code/models/urhand.py:100-102: F.conv2d(7x7, s1, p3) and
F.conv2d(4x4, s2, p1) on the effective weights, and their autograd backward with x detached (two weight-gradient
convolutions and the input gradient of the second) -- at the model's shape, 4 -> 64 -> 192 at 1024^2, for B = 1 and B = 4,
forward and forward + backward with both weight gradients, and derive the dispatch table of goliath_amd/featenc.py.  It
also times the whole FeatEncoderUNet forward + backward, on the library lines and with the front forced onto the operator.

Method (that of tools/dispunet_probe.py): every variant is warmed up, then the variants are timed alternately in ROUNDS
rounds inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds and the
spread (max - min over the rounds).  The shape is admitted to the dispatch table only if the HIP operator's forward +
backward median is below the library's by more than the library's own spread, at B = 1.  Outputs and
gradients of the two are compared at the timed size (rel-L2 against the fp32 library result).  The operator's kernels are also
timed one by one through the C ABI; peak memory of a forward + backward is taken from the allocator each way.  Needs the
GPU; there is no fallback.

Usage: python tools/featenc_probe.py [--batches 1,4] [--rounds 7] [--iters 5] [--out profiles/featenc_probe.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from goliath_amd import build, featenc

CX, CM, CO, SIZE, OUT_CH = 4, 64, 192, 1024, 128


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


def pieces(B, x, w_p, w_f, g, rounds, iters):
    """The HIP operator's kernels through the C ABI: forward, each weight gradient alone (ms, median over the rounds)."""
    dims = dict(B=B, Cx=CX, Cm=CM, Co=CO, H=SIZE, W=SIZE)
    x, w_p, w_f = x.detach(), w_p.detach(), w_f.detach()
    y, g_p, g_f = torch.empty_like(g), torch.empty_like(w_p), torch.empty_like(w_f)
    n_scratch = featenc.bwd_scratch_floats(**dims)
    scratch = torch.empty(n_scratch, device=x.device)
    bwd = lambda o_p, o_f: (lambda: featenc._abi_featenc_front_bwd(**dims, x=x, w_p=w_p, w_f=w_f, g_y=g, g_w_p=o_p, g_w_f=o_f,
                                                                  scratch=scratch))
    calls = {"fwd": lambda: featenc._abi_featenc_front_fwd(**dims, x=x, w_p=w_p, w_f=w_f, y=y),
             "bwd_w_f": bwd(None, g_f), "bwd_w_p": bwd(g_p, None)}
    gflop = {"fwd": 2.0 * B * (CM * CX * 49 * SIZE * SIZE + CO * CM * 16 * SIZE * SIZE / 4) / 1e9}
    out = {"scratch_mb": 4 * n_scratch / 1e6}
    for k, call in calls.items():
        call()
        torch.cuda.synchronize()
        ms = statistics.median(timed(call, iters) for _ in range(rounds))
        out[k] = {"ms": ms}
        if k in gflop:
            out[k].update(gflop_without_recompute=gflop[k], tflops_without_recompute=gflop[k] / ms)
    return out


def probe(B, rounds, iters):
    dev = "cuda"
    torch.manual_seed(B)
    x = torch.randn(B, CX, SIZE, SIZE, device=dev)
    w_p = (torch.randn(CM, CX, 7, 7, device=dev) / (49.0 * CX) ** 0.5).requires_grad_(True)
    w_f = (torch.randn(CO, CM, 4, 4, device=dev) / (16.0 * CM) ** 0.5).requires_grad_(True)
    g = torch.randn(B, CO, SIZE // 2, SIZE // 2, device=dev)
    leaves = [w_p, w_f]
    ops = {"hip": lambda: featenc.front(x, w_p, w_f), "torch": lambda: featenc.front_torch(x, w_p, w_f)}

    def fwd(op):
        with torch.no_grad():
            return op()

    def fwd_bwd(op):
        return torch.autograd.grad(op(), leaves, g)

    variants = {f"{name}_{kind}": (lambda op=op, run=run: run(op))
                for name, op in ops.items() for kind, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
    y = {name: fwd(op) for name, op in ops.items()}
    parity = {"y": rel_l2(y["hip"], y["torch"])}
    grads = {name: fwd_bwd(op) for name, op in ops.items()}
    parity.update({n: rel_l2(p, q) for n, p, q in zip(("g_w_proj", "g_w_feat"), grads["hip"], grads["torch"])})
    del y, grads
    for fn in variants.values():   # warm-up: code objects, the library's algorithm choice, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # alternate the variants inside every round
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    row = {"B": B, "Cx": CX, "Cm": CM, "Co": CO, "H": SIZE, "W": SIZE,
           # the tensor between the two layers, which the library writes, reads and keeps, and its gradient
           "intermediate_mb": 4.0 * B * CM * SIZE * SIZE / 1e6, "parity_rel_l2": parity}
    for k, v in times.items():
        row[k + "_ms"] = stats(v)
    row["peak_memory_mb_fwd_bwd"] = {name: peak_mb(lambda op=op: fwd_bwd(op)) for name, op in ops.items()}
    row["hip_kernels"] = pieces(B, x, w_p, w_f, g, rounds, iters)
    t, hp = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    row["hip_wins_by_the_rule"] = bool(hp["median"] < t["median"] - t["spread"])
    return row


def whole_encoder(B, rounds, iters):
    """FeatEncoderUNet(1, 3, 128) forward + backward at 1024^2: the library lines against the front forced onto the operator."""
    torch.manual_seed(7)
    fe = featenc.FeatEncoderUNet(1, CX - 1, OUT_CH).cuda()
    x = torch.randn(B, CX, SIZE, SIZE, device="cuda")
    params = list(fe.parameters())

    def run(mode):
        os.environ["GOLIATH_FUSED_FEATENC_ALL"] = "1" if mode == "forced" else "0"
        z, gb = featenc.forward(fe, x, op=False if mode == "library" else None)
        loss = z.sum() + sum((b * b).sum() for b in gb)
        grads = torch.autograd.grad(loss, params)
        return z.detach(), [b.detach() for b in gb], grads

    modes = ("library", "forced")
    try:
        ref, got = run("library"), run("forced")
        parity = {"z": rel_l2(got[0], ref[0]), "gb_max": max(rel_l2(a, b) for a, b in zip(got[1], ref[1])),
                  "grad_max": max(rel_l2(a, b) for a, b in zip(got[2], ref[2]))}
        del ref, got
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
    return {"B": B, "size": SIZE, "out_ch": OUT_CH, "fwd_bwd_ms": {m: stats(v) for m, v in times.items()},
            "peak_memory_mb_fwd_bwd": peak, "parity_rel_l2_against_library": parity}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-encoder", action="store_true", help="skip the whole-encoder rows")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "featenc_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("featenc_probe needs the GPU: there is nothing to measure without one")
    rows, encoders = [], []
    for B in map(int, args.batches.split(",")):
        row = probe(B, args.rounds, args.iters)
        rows.append(row)
        kernels = " ".join("%s %.3f" % (k, v["ms"]) for k, v in row["hip_kernels"].items() if isinstance(v, dict))
        print(f"B={B} {CX}->{CM}->{CO} @ {SIZE}^2  fwd hip {row['hip_fwd_ms']['median']:.3f} / torch "
              f"{row['torch_fwd_ms']['median']:.3f} ms  fwd+bwd hip {row['hip_fwd_bwd_ms']['median']:.3f} (spread "
              f"{row['hip_fwd_bwd_ms']['spread']:.3f}) / torch {row['torch_fwd_bwd_ms']['median']:.3f} ms (spread "
              f"{row['torch_fwd_bwd_ms']['spread']:.3f})  peak MB hip {row['peak_memory_mb_fwd_bwd']['hip']:.0f} / torch "
              f"{row['peak_memory_mb_fwd_bwd']['torch']:.0f}  kernels {kernels}  wins={row['hip_wins_by_the_rule']}  parity "
              f"{max(row['parity_rel_l2'].values()):.1e}", flush=True)
        torch.cuda.empty_cache()
        if not args.no_encoder:
            enc = whole_encoder(B, args.rounds, args.iters)
            encoders.append(enc)
            print(f"B={B} whole encoder fwd+bwd ms: "
                  + "  ".join(f"{m} {v['median']:.3f} (spread {v['spread']:.3f})" for m, v in enc["fwd_bwd_ms"].items())
                  + "  peak MB " + "  ".join(f"{m} {v:.0f}" for m, v in enc["peak_memory_mb_fwd_bwd"].items()), flush=True)
            torch.cuda.empty_cache()
    # admission: by the row at B = 1
    table = [[r["Cx"], r["Cm"], r["Co"], r["H"], r["W"]] for r in rows if r["B"] == 1 and r["hip_wins_by_the_rule"]]
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "rounds": args.rounds,
              "iters": args.iters, "front": rows, "encoder": encoders, "dispatch": table}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
