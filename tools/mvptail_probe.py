#!/usr/bin/env python
"""Time the fused decoder tail of the MVP hand model (goliath_amd.mvptail.decode_template: gol_mvp_tail_fwd / _bwd) against
what dropin.patch_hand_mvp() runs today for the same lines: the two library last layers (F.conv_transpose2d + bias[None]),
relu(25 x + 100) / relu, and mvpprims.assemble_template(compact=True).

Rows: S = 1024, 64 x 64 primitives of 16 x 16 x 8; B = 1 and B = 4 (the training batch of hand_mvp_example.yml); all
primitives valid and a mask that keeps about half; forward, and forward + backward (all six gradients).

Method (as tools/trunk_probe.py): every variant of a row is warmed up, then the variants are timed alternately in ROUNDS
rounds inside one process (device events around ITERS back-to-back calls); reported are the median over the rounds and
the spread (max - min over the rounds) -- the parent path's own run-to-run spread stands beside every row, and a row
counts as won only if the fused median is below the parent's by more than that spread.  torch.cuda.max_memory_allocated
above the resident leaves is recorded for either path.  Outputs and gradients of the two are compared at the timed size
(rel-L2, under the kink screen of tests/mvptail_cases.py).  The fused forward is also given as traffic on its algorithmic
bytes (x + bias + the written template).  Also recorded: tools/trunk_probe.py's measurement of the two hidden shapes the
hand decoders have and trunk.DISPATCH lacks (64 -> 32 @ 64^2, 32 -> 32 @ 128^2, B = 4).  Needs the GPU; no fallback.

Usage: python tools/mvptail_probe.py [--rounds 7] [--iters 20] [--out profiles/mvptail_probe.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F

import trunk_probe
from goliath_amd import build, mvpprims, mvptail
from goliath_amd._lib import c_float, c_int, fptr, iptr, stream_ptr
from goliath_amd import _lib

TD, TH, TW, NY, NX = 8, 16, 16, 64, 64
PRIMSIZE = (TW, TH, TD)
H = NY * TH // 2
AFFINE = (25.0, 100.0)
HIDDEN = [(64, 32, 64), (32, 32, 128)]   # (Ci, Co, h) of DeconvContentDecoder's hidden layers that trunk.DISPATCH lacks


def parent_path(xr, wr, br, xa, wa, ba, valid):
    """hand_mvp.py:338-340 as the modules run it (library conv + ATen add), :465-472, :427-434, then the one-kernel
    template assembly of the parent commit"""
    B = xa.shape[0]
    rgb = (F.conv_transpose2d(xr, wr, None, 2, 1) + br[None]).view(B, TD, 3, 2 * H, 2 * H)
    rgb = F.relu(25.0 * rgb + 100.0)
    alpha = F.relu((F.conv_transpose2d(xa, wa, None, 2, 1) + ba[None]).view(B, TD, 1, 2 * H, 2 * H))
    return mvpprims.assemble_template(rgb, alpha, PRIMSIZE, valid_prims=valid, compact=True)


def fused_path(xr, wr, br, xa, wa, ba, valid):
    return mvptail.decode_template(xr, wr, br, xa, wa, ba, PRIMSIZE, valid_prims=valid, compact=True, rgb_affine=AFFINE)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v)}


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def pieces(leaves, slot, Kv, g, rounds, iters):
    """The fused operator's ABI calls with one group of outputs each (ms, median): the backward's first pass (template
    layout -> g_pre and the bias gradients) runs in every backward piece."""
    xr, wr, br, xa, wa, ba = (t.detach() for t in leaves)
    B = xa.shape[0]
    dims = (c_int(B), c_int(16), c_int(H), c_int(H), c_int(TD), c_int(TH), c_int(TW), c_int(NY), c_int(NX))
    out = torch.empty(B, Kv, TD, TH, TW, 4, device=xa.device)
    wrt, wat = wr.permute(1, 2, 3, 0).contiguous(), wa.permute(1, 2, 3, 0).contiguous()
    scratch = torch.empty(mvptail._scratch_floats(B, H, H, TD, 4), device=xa.device)
    gx, gw, gb = [torch.empty_like(xr), torch.empty_like(xa)], [torch.empty_like(wr), torch.empty_like(wa)], \
        [torch.empty_like(br), torch.empty_like(ba)]
    none = [None, None]

    def fwd():
        _lib.call("gol_mvp_tail_fwd", *dims, fptr(xr), fptr(wr), fptr(br), fptr(xa), fptr(wa), fptr(ba), iptr(slot), iptr(None),
                  c_int(Kv), c_float(AFFINE[0]), c_float(AFFINE[1]), fptr(out), stream_ptr())

    def bwd(a, b, c):
        return lambda: _lib.call("gol_mvp_tail_bwd", *dims, c_int(4), fptr(xr), fptr(wrt), fptr(xa), fptr(wat), iptr(slot),
                                 iptr(None), c_int(Kv), c_float(AFFINE[0]), fptr(g), fptr(out), fptr(a[0]), fptr(a[1]),
                                 fptr(b[0]), fptr(b[1]), fptr(c[0]), fptr(c[1]), fptr(scratch), stream_ptr())

    calls = {"fwd": fwd, "bwd_gpre_bias": bwd(none, none, gb), "bwd_gpre_x": bwd(gx, none, none),
             "bwd_gpre_w": bwd(none, gw, none), "bwd_all": bwd(gx, gw, gb)}
    res = {}
    for k, call in calls.items():
        call()
        torch.cuda.synchronize()
        res[k] = statistics.median(trunk_probe.timed(call, iters) for _ in range(rounds))
    return res


def probe(B, mask_kind, rounds, iters, with_pieces):
    dev = "cuda"
    torch.manual_seed(7)
    xr, xa = torch.randn(B, 16, H, H, device=dev), torch.randn(B, 16, H, H, device=dev)
    wr, wa = torch.randn(16, 3 * TD, 4, 4, device=dev) / 8.0, torch.randn(16, TD, 4, 4, device=dev) / 8.0
    br = -4.0 + 0.05 * torch.randn(3 * TD, 2 * H, 2 * H, device=dev)
    ba = 0.3 * torch.randn(TD, 2 * H, 2 * H, device=dev)
    leaves = [t.requires_grad_(True) for t in (xr, wr, br, xa, wa, ba)]
    K = NY * NX
    valid = torch.ones(K, dtype=torch.bool, device=dev) if mask_kind == "all" else torch.rand(K, device=dev) < 0.5
    slot, _, Kv = mvpprims.prim_slots(valid, True)
    g = torch.randn(B, Kv, TD, TH, TW, 4, device=dev)
    with torch.no_grad():   # the kink screen of the tests: no upstream gradient where a relu's argument is within rounding of 0
        aff = 25.0 * (F.conv_transpose2d(xr, wr, None, 2, 1) + br[None]).view(B, TD, 3, 2 * H, 2 * H) + 100.0
        pre = (F.conv_transpose2d(xa, wa, None, 2, 1) + ba[None]).view(B, TD, 1, 2 * H, 2 * H)
        keep = mvpprims.assemble_template((aff.abs() >= 1e-3).float(), (pre.abs() >= 1e-4).float(), PRIMSIZE,
                                          valid_prims=valid, compact=True)
        g = g * keep
        screened = 1.0 - float(keep.mean())
        del aff, pre, keep
    ops = {"fused": fused_path, "parent": parent_path}

    def fwd(op):
        with torch.no_grad():
            return op(*leaves, valid)

    def fwd_bwd(op):
        return torch.autograd.grad(op(*leaves, valid), leaves, g)

    y = {n: fwd(op) for n, op in ops.items()}
    parity = {"template": rel_l2(y["fused"], y["parent"])}
    del y
    grads = {n: fwd_bwd(op) for n, op in ops.items()}
    parity.update({k: rel_l2(a, b) for k, a, b in zip(("g_x_rgb", "g_w_rgb", "g_bias_rgb", "g_x_alpha", "g_w_alpha",
                                                       "g_bias_alpha"), grads["fused"], grads["parent"])})
    del grads
    variants = {f"{n}_{kind}": (lambda op=op, run=run: run(op)) for n, op in ops.items()
                for kind, run in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
    peak = {k: peak_mb(fn) for k, fn in variants.items()}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(trunk_probe.timed(fn, iters))
    bytes_fwd = 4 * (2 * B * 16 * H * H + 4 * TD * 4 * H * H + B * Kv * TD * TH * TW * 4)
    row = {"B": B, "mask": mask_kind, "Kv": Kv, "K": K, "S": 2 * H, "primsize": list(PRIMSIZE), "parity_rel_l2": parity, "screened_share": screened,
           "fused_algorithmic_mb_fwd": bytes_fwd / 1e6, "peak_memory_mb": peak}
    for k, v in times.items():
        row[k + "_ms"] = stats(v)
    row["fused_fwd_tb_per_s"] = bytes_fwd / row["fused_fwd_ms"]["median"] / 1e9
    for kind in ("fwd", "fwd_bwd"):
        p, f = row[f"parent_{kind}_ms"], row[f"fused_{kind}_ms"]
        row[f"{kind}_speedup"] = p["median"] / f["median"]
        row[f"{kind}_faster_beyond_parent_spread"] = bool(f["median"] < p["median"] - p["spread"])
    if with_pieces:
        row["fused_abi_calls_ms"] = pieces(leaves, slot, Kv, g, rounds, iters)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "mvptail_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mvptail_probe needs the GPU: there is nothing to measure without one")
    rows = []
    for B in (1, 4):
        for kind in ("all", "half"):
            row = probe(B, kind, args.rounds, args.iters, with_pieces=True)
            rows.append(row)
            print(f"B={B} mask={kind:4s} Kv={row['Kv']:4d}  fwd fused {row['fused_fwd_ms']['median']:.3f} / parent "
                  f"{row['parent_fwd_ms']['median']:.3f} ms (parent spread {row['parent_fwd_ms']['spread']:.3f})  fwd+bwd fused "
                  f"{row['fused_fwd_bwd_ms']['median']:.3f} / parent {row['parent_fwd_bwd_ms']['median']:.3f} ms (spread "
                  f"{row['parent_fwd_bwd_ms']['spread']:.3f})  {row['fused_fwd_tb_per_s']:.2f} TB/s  peak MB "
                  f"{ {k: round(v) for k, v in row['peak_memory_mb'].items()} }  calls "
                  f"{' '.join(f'{k} {v:.3f}' for k, v in row['fused_abi_calls_ms'].items())}  parity "
                  f"{max(row['parity_rel_l2'].values()):.1e}", flush=True)
            torch.cuda.empty_cache()
    hidden = []
    for Ci, Co, h in HIDDEN:
        r = trunk_probe.probe(4, Ci, Co, h, 7, 10)
        hidden.append(r)
        print(f"trunk {Ci}->{Co} @ {h}^2 B=4  fwd+bwd hip {r['hip_fwd_bwd_ms']['median']:.3f} / torch "
              f"{r['torch_fwd_bwd_ms']['median']:.3f} ms (torch spread {r['torch_fwd_bwd_ms']['spread']:.3f}) admitted={r['admitted']}",
              flush=True)
    result = {"device": torch.cuda.get_device_name(0), "source_digest": build.source_digest(), "rounds": args.rounds,
              "iters": args.iters, "rows": rows, "trunk_hidden_shapes_b4": hidden}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
