"""Time the tail of a training iteration (gradient scrub, global-norm clip, Adam step) on the parameter set of bench.py's
e2e workload (decoder.PrimDecoderConvs at slab 1024 plus the albedo tensor), four ways in one process, interleaved:

    a  the reference's literal lines (ca_code/utils/train.py:209-215) + torch.optim.Adam(fused=True)
    b  nan_to_num_ + clip_grad_norm_(foreach=True) + torch.optim.Adam(fused=True)
    c  goliath_amd.optim.Adam(max_norm=1, scrub_nonfinite=True, write_back_grads=True)
    d  the same with write_back_grads=False

Every variant owns its parameters, gradients and state; before each timed step its gradients are refilled from one
master copy (outside the timed span), since a, b and c modify them.  Prints one JSON line; --out writes it to a file too.

    python tools/optim_bench.py [--steps 20] [--warmup 3] [--out profiles/optim_step.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBPS = 6.29      # the measured copy ceiling the byte model is judged against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slab", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from goliath_amd import build, decoder, optim

    dev = torch.device("cuda", 0)
    torch.manual_seed(4321)
    dec = decoder.PrimDecoderConvs(base=args.slab // 128)
    shapes = [tuple(p.shape) for p in dec.parameters()] + [(1, args.slab * args.slab, 3)]
    del dec
    n_params = sum(int(torch.Size(s).numel()) for s in shapes)
    master = [0.01 * torch.randn(s, device=dev) for s in shapes]          # norm >> 1: every variant clips

    def make(kind):
        params = [torch.nn.Parameter(0.1 * torch.randn(s, device=dev)) for s in shapes]
        for p in params:
            p.grad = torch.zeros_like(p)
        if kind in "ab":
            opt = torch.optim.Adam(params, lr=5e-4, fused=True)
        else:
            opt = optim.Adam(params, lr=5e-4, max_norm=1.0, scrub_nonfinite=True, write_back_grads=kind == "c")

        def tail():
            if kind == "a":
                for p in params:
                    p.grad.data[torch.isnan(p.grad.data)] = 0
                    p.grad.data[torch.isinf(p.grad.data)] = 0
                torch.nn.utils.clip_grad_norm_(params, 1.0)
            elif kind == "b":
                for p in params:
                    torch.nan_to_num_(p.grad, nan=0.0, posinf=0.0, neginf=0.0)
                torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
            opt.step()

        return {"grads": [p.grad for p in params], "tail": tail, "gpu_ms": [], "wall_ms": []}

    variants = {k: make(k) for k in "abcd"}
    for it in range(args.warmup + args.steps):
        for v in variants.values():
            torch._foreach_copy_(v["grads"], master)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            v["tail"]()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                v["wall_ms"].append((time.perf_counter() - t0) * 1e3)
                v["gpu_ms"].append(e0.elapsed_time(e1))

    bytes_per_param = {"a": None, "b": None, "c": 36, "d": 32}     # read g | read p g m v, write p m v | write g
    res = {"what": "scrub + clip + Adam step on the e2e decoder's parameter set; ms per step between two events on the "
                   "stream (median / min over the timed steps) and host wall time with a sync at both ends",
           "device": torch.cuda.get_device_name(0), "csrc_sha16": build.source_digest(), "chunk_elems": optim.chunk_elems(),
           "parameters": n_params, "tensors": len(shapes), "largest_tensor": max(int(torch.Size(s).numel()) for s in shapes),
           "steps": args.steps, "warmup": args.warmup, "copy_ceiling_tbps": COPY_CEILING_TBPS, "variants": {}}
    names = {"a": "reference lines + torch fused Adam", "b": "nan_to_num_ + clip_grad_norm_(foreach) + torch fused Adam",
             "c": "goliath_amd.optim.Adam, write_back_grads=True", "d": "goliath_amd.optim.Adam, write_back_grads=False"}
    for k, v in variants.items():
        ms = statistics.median(v["gpu_ms"])
        row = {"name": names[k], "gpu_ms_median": round(ms, 4), "gpu_ms_min": round(min(v["gpu_ms"]), 4),
               "wall_ms_median": round(statistics.median(v["wall_ms"]), 4)}
        if bytes_per_param[k]:
            tbps = n_params * bytes_per_param[k] / (ms * 1e-3) / 1e12
            row.update(bytes_per_parameter=bytes_per_param[k], effective_tbps=round(tbps, 3),
                       fraction_of_copy_ceiling=round(tbps / COPY_CEILING_TBPS, 3))
        res["variants"][k] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
