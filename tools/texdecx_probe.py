#!/usr/bin/env python
"""Time the texture-decoder layer at precision "bf16x3" (goliath_amd.texdec.upconv_lrelu / upconv_gated with
precision="bf16x3": gol_upconvx_pack / _fwd / _bwd_x / _bwd_w / _bwd_gate, pack included) against what precision="fp32" runs
for the same shape today -- the library lines of the two loops of goliath_amd/urhand.py (F.interpolate + F.conv2d + the
epilogue) for the five small layers, the fp32 operator gol_upconv_* for 32 -> 16 @ 1024^2 (texdec.DISPATCH) -- on the 12
(mode, layer) shapes the split kernels take, at B = 1, forward and forward + backward with all inputs requiring gradients, and
derive texdec.DISPATCH_BF16X3.  The seventh layer (16 -> 4) is timed on its fp32 path only, for the 14-layer sum.

Method (that of tools/texdec_probe.py): every variant of a shape is warmed up, then the variants are timed alternately in
ROUNDS rounds inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds
and the spread (max - min).  Admission (DESIGN.md section 6a as goliath_amd.olatunet applies it): a shape enters the table
only if the split operator's forward + backward median is below the other side's by more than the sum of both spreads.  Also reported:
the split operator's kernels one by one through the C ABI with the TFLOP/s they reach on the algorithmic FLOP
(2 x 9 Ci Co H W per product), the peak memory of a forward + backward of either side, the 14-layer sums, and the distance
of the whole two-branch stack at the model's sizes between precision="bf16x3" (every supported layer forced) and the "fp32"
path.  Needs the GPU; there is no fallback.  bench.py runs no texture decoder: none of these numbers is a bench.py number.

Usage: python tools/texdecx_probe.py [--batch 1] [--rounds 7] [--iters 5] [--out profiles/texdecx_probe.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import torch.nn.functional as F

from goliath_amd import build, texdec

LEAK = 0.2
N_GAINBIAS = 4          # urhand.py:604: the layers of the linear branch that have a gainbias add it (the first four)
SCALE = texdec.GAIN_SCALE


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


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def pieces(mode, B, Ci, Co, Hi, scale, x, weight, a, gb, g, rounds, iters):
    """The split operator's kernels one by one through the C ABI: ms (median over the rounds) and TFLOP/s."""
    x, weight, a = x.detach(), weight.detach(), a.detach()
    gb = None if gb is None else gb.detach()
    d = dict(B=B, Ci=Ci, Co=Co, Hi=Hi, Wi=Hi, mode=mode, leak=LEAK if mode == 0 else 1.0, scale=scale)
    small = dict(B=B, Ci=Ci, Co=Co, Hi=Hi, Wi=Hi)
    y = torch.empty_like(g)
    packed = torch.empty(texdec.packed_elems_bf16x3(Co, Ci), device=x.device, dtype=torch.int16)
    scratch = torch.empty(texdec.bwd_w_scratch_floats_bf16x3(**small), device=x.device)
    gx, gw, ga, ggb = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(a), torch.empty_like(g)
    bias, gate = (a, None) if mode == 0 else (None, a)
    aux = dict(y=y, gate=None) if mode == 0 else dict(y=None, gate=gate)
    none = dict(x=None, w_eff=None, g_x=None, g_w=None, g_bias=None, g_gate=None, g_gb=None, scratch=None)
    flop = 2.0 * g.numel() * 9 * Ci
    calls = {
        "pack": (lambda: texdec._abi_upconvx_pack(Co=Co, Ci=Ci, weight=weight, packed=packed), 0.0),
        "fwd": (lambda: texdec._abi_upconvx_fwd(**d, x=x, packed=packed, bias=bias, gate=gate, gb=gb, y=y), flop),
        "bwd_x": (lambda: texdec._abi_upconvx_bwd_x(**d, packed=packed, **aux, g_y=g, g_x=gx), flop),
        "bwd_w": (lambda: texdec._abi_upconvx_bwd_w(**d, x=x, **aux, g_y=g, g_w=gw, scratch=scratch), flop),
    }
    if mode == 0:
        calls["bwd_bias"] = (lambda: texdec._abi_upconv_bwd(**d, **dict(none, g_bias=ga), **aux, g_y=g), 0.0)
    else:
        calls["bwd_gate"] = (lambda: texdec._abi_upconvx_bwd_gate(**small, scale=scale, x=x, packed=packed, g_y=g, g_gate=ga,
                                                                  g_gb=ggb if gb is not None else None), flop)
    out = {}
    for k, (call, fl) in calls.items():
        call()
        torch.cuda.synchronize()
        ms = statistics.median(timed(call, iters) for _ in range(rounds))
        out[k] = {"ms": ms, "gflop": fl / 1e9, "tflops": fl / ms / 1e9}
    return out


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return (peak - base) / 1e6


def probe(mode, layer, B, rounds, iters):
    dev = "cuda"
    Ci, Co = texdec.CHANNELS[layer]
    Hi = 32 << layer
    H = 2 * Hi
    with_gb = mode == 1 and layer < N_GAINBIAS
    scale = SCALE if with_gb else 1.0
    split_ok = texdec.supported_bf16x3(Ci, Co, Hi, Hi)
    fp32_hip = bool(texdec.DISPATCH.get((mode, Ci, Co, Hi, Hi), False))
    torch.manual_seed(2000 * mode + layer)
    x = torch.randn(B, Ci, Hi, Hi, device=dev, requires_grad=True)
    weight = (torch.randn(Co, Ci, 3, 3, device=dev) / (9.0 * Ci) ** 0.5).requires_grad_(True)
    g = torch.randn(B, Co, H, H, device=dev)
    if mode == 0:
        a = (0.5 * torch.randn(Co, H, H, device=dev)).requires_grad_(True)
        gb = None
        leaves, names = [x, weight, a], ("g_x", "g_weight", "g_bias")
        other = (lambda: texdec.upconv_lrelu(x, weight, a, LEAK)) if fp32_hip else (lambda: torch_lrelu(x, weight, a))
        split = lambda: texdec.upconv_lrelu(x, weight, a, LEAK, precision="bf16x3")
    else:
        a = torch.randn(B, Co, H, H, device=dev, requires_grad=True)
        gb = torch.randn(B, Co, H, H, device=dev, requires_grad=True) if with_gb else None
        leaves = [x, weight, a] + ([gb] if with_gb else [])
        names = ("g_x", "g_weight", "g_gate", "g_gb")[:len(leaves)]
        other = ((lambda: texdec.upconv_gated(x, weight, a, gb, scale)) if fp32_hip
                 else (lambda: torch_gated(x, weight, a, gb)))
        split = lambda: texdec.upconv_gated(x, weight, a, gb, scale, precision="bf16x3")
    ops = {"other": other}
    if split_ok:
        ops["split"] = split

    def fwd(op):
        with torch.no_grad():
            return op()

    def fwd_bwd(op):
        return torch.autograd.grad(op(), leaves, g)

    variants = {f"{name}_{kind}": (lambda op=op, run=run: run(op))
                for name, op in ops.items() for kind, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
    row = {"mode": mode, "layer": layer, "B": B, "Ci": Ci, "Co": Co, "Hi": Hi, "Wi": Hi, "gainbias": with_gb,
           "other_side": "gol_upconv (fp32 operator)" if fp32_hip else "library lines", "gflop_fwd": 2.0 * g.numel() * 9 * Ci / 1e9}
    if split_ok:   # the distance between the two sides at the timed size (forward; the gradients go through the kink in mode 0)
        row["y_rel_l2_split_vs_other"] = rel_l2(fwd(split), fwd(other))
    for fn in variants.values():   # warm-up: code objects, the library's algorithm choice, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # alternate the variants inside every round
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    for k, v in times.items():
        row[k + "_ms"] = stats(v)
    row["peak_mb_fwd_bwd"] = {name: peak_mb(lambda op=op: fwd_bwd(op)) for name, op in ops.items()}
    if split_ok:
        row["split_kernels"] = pieces(mode, B, Ci, Co, Hi, scale, x, weight, a, gb, g, rounds, iters)
        s, o = row["split_fwd_bwd_ms"], row["other_fwd_bwd_ms"]
        row["admitted"] = bool(s["median"] < o["median"] - o["spread"] - s["spread"])
    else:
        row["admitted"] = False
    return row


class ModelStack(nn.Module):
    """The texture-branch attributes of ConvTeacherDecoder at the model's sizes (urhand.py:302-323)."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(7)
        self.n_layers_tex = len(texdec.CHANNELS)
        self.texmod0 = nn.ModuleList([texdec.Conv3WNUB(ci, co, 64 << k, 64 << k) for k, (ci, co) in enumerate(texdec.CHANNELS)])
        self.texmod1 = nn.ModuleList([texdec.Conv3WN(ci, co) for ci, co in texdec.CHANNELS])
        with torch.no_grad():
            for m in self.texmod0:
                m.bias.normal_(0, 0.3)


def whole_branch(B):
    """rel-L2 between texture_branches at "bf16x3" with every supported layer forced and at "fp32" (the committed dispatch:
    library lines for the five small layers, gol_upconv_* for the last two), forward, at the model's sizes."""
    dec = ModelStack().cuda()
    g = torch.Generator(device="cuda").manual_seed(8)
    jf = torch.randn(B, 128, 32, 32, device="cuda", generator=g)
    z = torch.randn(B, 128, 32, 32, device="cuda", generator=g)
    gbs = [torch.randn(B, texdec.CHANNELS[k][1], 64 << k, 64 << k, device="cuda", generator=g) for k in range(N_GAINBIAS)]
    env = os.environ.pop("GOLIATH_FUSED_TEXDEC_ALL", None)
    try:
        with torch.no_grad():
            ref = texdec.texture_branches(dec, jf, z, gbs)
            os.environ["GOLIATH_FUSED_TEXDEC_ALL"] = "1"
            fp32_all = texdec.texture_branches(dec, jf, z, gbs)
            got = texdec.texture_branches(dec, jf, z, gbs, precision="bf16x3")
    finally:
        os.environ.pop("GOLIATH_FUSED_TEXDEC_ALL", None)
        if env is not None:
            os.environ["GOLIATH_FUSED_TEXDEC_ALL"] = env
    return {"bf16x3_forced_vs_fp32_path": rel_l2(got, ref), "bf16x3_forced_vs_fp32_operator_forced": rel_l2(got, fp32_all),
            "fp32_operator_forced_vs_fp32_path": rel_l2(fp32_all, ref)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", default="0,1,2,3,4,5,6")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "texdecx_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texdecx_probe needs the GPU: there is nothing to measure without one")
    rows = []
    for mode in (0, 1):
        for layer in map(int, args.layers.split(",")):
            row = probe(mode, layer, args.batch, args.rounds, args.iters)
            rows.append(row)
            o = row["other_fwd_bwd_ms"]
            line = f"mode {mode} {row['Ci']:3d}->{row['Co']:3d} @ {row['Hi']:4d}^2  other ({row['other_side']}) fwd " \
                   f"{row['other_fwd_ms']['median']:.3f} fwd+bwd {o['median']:.3f} (spread {o['spread']:.3f})"
            if "split_fwd_bwd_ms" in row:
                s = row["split_fwd_bwd_ms"]
                kernels = " ".join("%s %.3f ms %.0f TF" % (k, v["ms"], v["tflops"]) for k, v in row["split_kernels"].items())
                line += f"  split fwd {row['split_fwd_ms']['median']:.3f} fwd+bwd {s['median']:.3f} (spread {s['spread']:.3f})" \
                        f"  kernels {kernels}  peak MB {row['peak_mb_fwd_bwd']}  admitted={row['admitted']}"
            print(line, flush=True)
            torch.cuda.empty_cache()
    total = lambda key: sum(r[key]["median"] for r in rows)
    sums = {"fp32_path_ms": total("other_fwd_bwd_ms"),
            "bf16x3_dispatched_ms": sum(r["split_fwd_bwd_ms" if r["admitted"] else "other_fwd_bwd_ms"]["median"] for r in rows),
            "bf16x3_every_supported_layer_forced_ms": sum(r.get("split_fwd_bwd_ms", r["other_fwd_bwd_ms"])["median"] for r in rows),
            "layers": len(rows)}
    print("14-layer sums (forward + backward, ms):", sums, flush=True)
    branch = whole_branch(args.batch) if len(rows) == 14 else None
    print("whole branch rel-L2:", branch, flush=True)
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "batch": args.batch,
              "rounds": args.rounds, "iters": args.iters, "leak": LEAK, "layers": rows, "sums_fwd_bwd_ms": sums,
              "whole_branch_rel_l2": branch,
              "dispatch": [[r["mode"], r["Ci"], r["Co"], r["Hi"], r["Wi"]] for r in rows if r["admitted"]]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
