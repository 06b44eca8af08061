#!/usr/bin/env python
"""Time the fused DisplacementUNet decoder level (goliath_amd.dispunet.upcat_conv: gol_upcat_conv_fwd / _bwd) against the
library composition it replaces -- the reference's ca_code/models/urhand.py:222-228 / :235-241: F.leaky_relu(x, 0.2),
F.interpolate(bilinear, align_corners=True) to the skip's size, th.cat([x, x_prev], 1), F.conv2d(3x3, s1, p1) and
`+ bias[None]`, with tanh and the affine after the last level -- on the five upsampling levels of both decoder branches at the
config's sizes (urhand_mesh_example.yml: uv_size 1024, init_uv_size 32, 64 channels: 64 + 64 -> 64 at 32^2 -> 64^2 up to
256^2 -> 512^2, and 64 + 64 -> 1 at 512^2 -> 1024^2 with the tanh head) at B = 1, forward and forward + backward, and derive
the dispatch table of goliath_amd/dispunet.py.  It also times the whole DisplacementUNet forward + backward, on the library
lines, with the derived table and with every level forced onto the operator.

Method (that of tools/texdec_probe.py): every variant of a shape is warmed up, then the variants are timed alternately in
ROUNDS rounds inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds
and the spread (max - min over the rounds).  A shape is admitted to the dispatch table only if the HIP operator's forward +
backward median is below the torch composition's by more than the torch composition's own spread, in both branches
(DESIGN.md section 6a).  Outputs and gradients of the two are compared at the timed size (rel-L2 against the fp32
composition).  The operator's kernels are also timed one by one through the C ABI, with the bytes the algorithm needs and
the rate they give; peak memory of a forward + backward is taken from the allocator each way.  Needs the GPU; there is no
fallback.

Usage: python tools/dispunet_probe.py [--batch 1] [--rounds 7] [--iters 5] [--out profiles/dispunet_probe.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from goliath_amd import _lib, build, dispunet
from goliath_amd._lib import c_float, c_int, fptr, stream_ptr

LEAK = 0.2
CHANNELS = 64
UV_SIZE, INIT_UV_SIZE, DISP_SCALE, POSE_DIMS = 1024, 32, 3.0, 60
HEADS = {"disp": ("tanh", DISP_SCALE, 0.0), "roughness": ("tanh",) + dispunet.ROUGHNESS_HEAD}


def torch_level(xa, xb, weight, bias, act):
    x = F.leaky_relu(xa, 0.2)
    x = F.interpolate(x, size=xb.shape[2:4], mode="bilinear", align_corners=True)
    x = torch.cat([x, xb], dim=1)
    x = F.conv2d(x, weight, None, 1, 1) + bias[None]
    return x if act is None else torch.tanh(x) * act[1] + act[2]


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


def pieces(B, Ca, Cb, Co, Hi, act, xa, xb, weight, bias, g, rounds, iters):
    """The HIP operator's kernels one by one through the C ABI: ms (median over the rounds) and algorithmic MB."""
    code, scale, shift = dispunet._act_args(act)
    dims = (c_int(B), c_int(Ca), c_int(Cb), c_int(Co), c_int(Hi), c_int(Hi), c_int(code), c_float(LEAK), c_float(scale),
            c_float(shift))
    xa, xb, weight, bias = xa.detach(), xb.detach(), weight.detach(), bias.detach()
    y = torch.empty_like(g)
    fn = _lib.load().gol_upcat_conv_bwd_scratch_floats
    fn.restype = ctypes.c_longlong
    scratch = torch.empty(int(fn(*dims[:6])), device=xa.device)
    gxa, gxb, gw, gb = torch.empty_like(xa), torch.empty_like(xb), torch.empty_like(weight), torch.empty_like(bias)
    fwd = lambda: _lib.call("gol_upcat_conv_fwd", *dims, fptr(xa), fptr(xb), fptr(weight), fptr(bias), fptr(y), stream_ptr())

    def bwd(o_xa=None, o_xb=None, o_w=None, o_b=None):
        return lambda: _lib.call("gol_upcat_conv_bwd", *dims, fptr(xa), fptr(xb), fptr(weight), fptr(y if code else None),
                                 fptr(g), fptr(o_xa), fptr(o_xb), fptr(o_w), fptr(o_b), fptr(scratch), stream_ptr())

    n_xa, n_xb, n_w, n_b, n_y = xa.numel(), xb.numel(), weight.numel(), bias.numel(), g.numel()
    n_g = n_y * (2 if code else 1)          # g_y, and y where the tanh is recovered from it
    calls = {"fwd": (fwd, n_xa + n_xb + n_w + n_b + n_y), "bwd_xa": (bwd(o_xa=gxa), n_g + n_w + 2 * n_xa),
             "bwd_xb": (bwd(o_xb=gxb), n_g + n_w + n_xb), "bwd_w": (bwd(o_w=gw), n_xa + n_xb + n_g + n_w),
             "bwd_bias": (bwd(o_b=gb), n_g + n_b)}
    out = {}
    fwd()
    for k, (call, floats) in calls.items():
        call()
        torch.cuda.synchronize()
        ms = statistics.median(timed(call, iters) for _ in range(rounds))
        out[k] = {"ms": ms, "algorithmic_mb": 4 * floats / 1e6, "tb_per_s": 4 * floats / ms / 1e9}
    return out


def probe(branch, level, B, rounds, iters):
    dev = "cuda"
    last = level == 5
    Ca = Cb = CHANNELS
    Co = 1 if last else CHANNELS
    Hi = INIT_UV_SIZE << (level - 1)
    H = 2 * Hi
    act = HEADS[branch] if last else None
    torch.manual_seed(1000 * (branch == "roughness") + level)
    xa = torch.randn(B, Ca, Hi, Hi, device=dev, requires_grad=True)
    xb = torch.randn(B, Cb, H, H, device=dev, requires_grad=True)
    weight = (torch.randn(Co, Ca + Cb, 3, 3, device=dev) / (9.0 * (Ca + Cb)) ** 0.5).requires_grad_(True)
    bias = (0.5 * torch.randn(Co, H, H, device=dev)).requires_grad_(True)
    g = torch.randn(B, Co, H, H, device=dev)
    leaves, names = [xa, xb, weight, bias], ("g_xa", "g_xb", "g_weight", "g_bias")
    ops = {"hip": lambda: dispunet.upcat_conv(xa, xb, weight, bias, LEAK, act),
           "torch": lambda: torch_level(xa, xb, weight, bias, act)}

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
    parity.update({n: rel_l2(p, q) for n, p, q in zip(names, grads["hip"], grads["torch"])})
    del y, grads
    for fn in variants.values():   # warm-up: code objects, the library's algorithm choice, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):        # alternate the variants inside every round
        for k, fn in variants.items():
            times[k].append(timed(fn, iters))
    n_xa, n_xb, n_w, n_b, n_y = xa.numel(), xb.numel(), weight.numel(), bias.numel(), g.numel()
    n_g = n_y * (2 if last else 1)
    bytes_fwd = 4 * (n_xa + n_xb + n_w + n_b + n_y)
    bytes_bwd = 4 * ((n_g + n_w + 2 * n_xa) + (n_g + n_w + n_xb) + (n_xa + n_xb + n_g + n_w) + (n_g + n_b))
    row = {"branch": branch, "level": level, "B": B, "Ca": Ca, "Cb": Cb, "Co": Co, "Hi": Hi, "Wi": Hi, "act": act,
           "gflop_fwd": 2.0 * n_y * 9 * (Ca + Cb) / 1e9, "algorithmic_mb_fwd": bytes_fwd / 1e6,
           "algorithmic_mb_fwd_bwd": (bytes_fwd + bytes_bwd) / 1e6,
           # what the composition writes and reads back on top: the activated, the upsampled and the concatenated tensor
           "activated_mb": 4 * n_xa / 1e6, "upsampled_mb": 16 * n_xa / 1e6, "concatenated_mb": 4 * (4 * n_xa + n_xb) / 1e6,
           "parity_rel_l2": parity}
    for k, v in times.items():
        row[k + "_ms"] = stats(v)
    row["peak_memory_mb_fwd_bwd"] = {name: peak_mb(lambda op=op: fwd_bwd(op)) for name, op in ops.items()}
    t, hp = row["torch_fwd_bwd_ms"], row["hip_fwd_bwd_ms"]
    row["hip_kernels"] = pieces(B, Ca, Cb, Co, Hi, act, xa, xb, weight, bias, g, rounds, iters)
    row["admitted"] = bool(hp["median"] < t["median"] - t["spread"])
    return row


def whole_unet(B, rounds, iters, table):
    """DisplacementUNet forward + backward at the config's sizes: library lines, the derived table, every level forced."""
    torch.manual_seed(7)
    unet = dispunet.DisplacementUNet(UV_SIZE, INIT_UV_SIZE, DISP_SCALE, POSE_DIMS, [CHANNELS] * 6).cuda()
    with torch.no_grad():
        for layers in unet.children():
            for layer in layers:
                layer.bias.normal_(0, 0.1)
    feat_uv = torch.randn(B, 6, UV_SIZE, UV_SIZE, device="cuda")
    pose_cond = torch.randn(B, POSE_DIMS, INIT_UV_SIZE, INIT_UV_SIZE, device="cuda")
    up = torch.randn(2, B, 1, UV_SIZE, UV_SIZE, device="cuda")
    params = list(unet.parameters())
    saved = dict(dispunet.DISPATCH)

    def run(mode):
        os.environ["GOLIATH_FUSED_DISPUNET_ALL"] = "1" if mode == "forced" else "0"
        dispunet.DISPATCH.clear()
        dispunet.DISPATCH.update({} if mode == "library" else table)
        disp, rough, _ = dispunet.forward(unet, feat_uv, pose_cond, op=False if mode == "library" else None)
        grads = torch.autograd.grad((disp * up[0]).sum() + (rough * up[1]).sum(), params)
        return disp.detach(), rough.detach(), grads

    modes = ("library", "dispatch", "forced")
    try:
        ref = run("library")
        parity = {}
        for mode in modes[1:]:
            got = run(mode)
            parity[mode] = {"disp": rel_l2(got[0], ref[0]), "roughness": rel_l2(got[1], ref[1]),
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
        os.environ.pop("GOLIATH_FUSED_DISPUNET_ALL", None)
        dispunet.DISPATCH.clear()
        dispunet.DISPATCH.update(saved)
    return {"B": B, "uv_size": UV_SIZE, "init_uv_size": INIT_UV_SIZE, "channels": CHANNELS, "pose_feat_dim": POSE_DIMS,
            "fwd_bwd_ms": {m: stats(v) for m, v in times.items()}, "peak_memory_mb_fwd_bwd": peak,
            "parity_rel_l2_against_library": parity}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--levels", default="1,2,3,4,5")
    ap.add_argument("--no-unet", action="store_true", help="skip the whole-UNet rows")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "dispunet_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dispunet_probe needs the GPU: there is nothing to measure without one")
    rows = []
    for branch in ("disp", "roughness"):
        for level in map(int, args.levels.split(",")):
            row = probe(branch, level, args.batch, args.rounds, args.iters)
            rows.append(row)
            kernels = " ".join("%s %.3f" % (k, v["ms"]) for k, v in row["hip_kernels"].items())
            print(f"{branch:9s} {row['Ca']}+{row['Cb']}->{row['Co']:2d} @ {row['Hi']:4d}^2  fwd hip {row['hip_fwd_ms']['median']:.3f} / "
                  f"torch {row['torch_fwd_ms']['median']:.3f} ms  fwd+bwd hip {row['hip_fwd_bwd_ms']['median']:.3f} / torch "
                  f"{row['torch_fwd_bwd_ms']['median']:.3f} ms (torch spread {row['torch_fwd_bwd_ms']['spread']:.3f})"
                  f"  peak MB hip {row['peak_memory_mb_fwd_bwd']['hip']:.0f} / torch {row['peak_memory_mb_fwd_bwd']['torch']:.0f}"
                  f"  kernels {kernels}  admitted={row['admitted']}  parity {max(row['parity_rel_l2'].values()):.1e}", flush=True)
            torch.cuda.empty_cache()
    shapes = sorted({(r["Ca"], r["Cb"], r["Co"], r["Hi"], r["Wi"]) for r in rows})
    table = [list(s) for s in shapes if all(r["admitted"] for r in rows if (r["Ca"], r["Cb"], r["Co"], r["Hi"], r["Wi"]) == s)]
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "batch": args.batch,
              "rounds": args.rounds, "iters": args.iters, "leak": LEAK, "levels": rows, "dispatch": table}
    if not args.no_unet:
        result["unet"] = whole_unet(args.batch, args.rounds, args.iters, {tuple(s): True for s in table})
        u = result["unet"]["fwd_bwd_ms"]
        print("whole UNet fwd+bwd ms: " + "  ".join(f"{m} {v['median']:.3f} (spread {v['spread']:.3f})" for m, v in u.items())
              + "  peak MB " + "  ".join(f"{m} {v:.0f}" for m, v in result["unet"]["peak_memory_mb_fwd_bwd"].items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
