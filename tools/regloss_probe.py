"""Time forward + backward of the per-Gaussian regularisers at the reference-native size (B x 1,048,576 Gaussians, B = 8
and 1), two ways in one process, interleaved:

    a  the torch composition of the reference's lines (ca_code/loss/__init__.py:560-600, 609-622)
    b  the fused operators of goliath_amd.losses (gol_regloss_*, gol_backlit_*)

per loss and for the four RGCA regularisers (bound_primscale, negcolor, l2_reg, backlit_reg) together.  A pass is the loss
and torch.autograd.grad to its input between two events on the stream; 3 warm-up and 20 timed passes per variant, median
and minimum.  For (b) a second set of passes times every kernel on its own (events around each ABI call) and reports it as a
fraction of the copy ceiling on the algorithmic bytes: forward 4 B per element, backward 8 B; backlit forward 16 B per row,
backward 28 B.  Prints one JSON line; --out writes it to a file too.

    python tools/regloss_probe.py [--steps 20] [--warmup 3] [--out profiles/regloss_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBPS = 6.29      # the measured copy ceiling the byte model is judged against
N = 1 << 20
RGCA = ("bound_primscale", "negcolor", "l2_reg", "backlit_reg")


def torch_losses():
    """The reference's lines, verbatim up to the dictionary lookups."""
    def bound_primscale(p, min_scale=0.1, max_scale=20.0):
        x = p["primscale_preclip"]
        return torch.where(x < min_scale, 1.0 / x.clamp(1e-7, torch.inf),
                           torch.where(x > max_scale, (x - max_scale) ** 2, 0.0)).mean()

    def backlit_reg(p):
        weight = F.relu(-p["cos_weight"]) ** 2
        return (weight * F.relu(p["color_rand"])).sum() / (1.0 + weight.sum())

    def list_l1_reg(p):
        loss = 0
        for term in p["spec_list"]:
            loss += term.abs().mean()
        return loss

    def alphaprior(p):
        alpha = p["alpha"]
        B = alpha.shape[0]
        return torch.mean(torch.log(0.1 + alpha.view(B, -1)) + torch.log(0.1 + 1.0 - alpha.view(B, -1)) - -2.20727)

    return {"bound_primscale": bound_primscale, "negcolor": lambda p: p["diff_color"].clamp(max=0.0).pow(2).mean(),
            "l2_reg": lambda p: p["spec_dnml"].pow(2).mean(), "backlit_reg": backlit_reg, "list_l1_reg": list_l1_reg,
            "alphaprior": alphaprior}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from goliath_amd import _lib, build, losses

    dev = torch.device("cuda", 0)
    ours = {"bound_primscale": losses.bound_primscale, "negcolor": losses.negcolor, "l2_reg": losses.l2_reg,
            "backlit_reg": losses.backlit_reg, "list_l1_reg": lambda p: losses.list_l1_reg(p, key="spec_list"),
            "alphaprior": losses.alphaprior}
    theirs = torch_losses()
    leaf_of = {"bound_primscale": "primscale_preclip", "negcolor": "diff_color", "l2_reg": "spec_dnml",
               "backlit_reg": "color_rand", "list_l1_reg": "spec_list", "alphaprior": "alpha"}
    res = {"what": "forward + backward of the per-Gaussian regularisers, ms between two events on the stream (median / min "
                   "over the timed passes): a = torch composition of the reference's lines, b = goliath_amd.losses; "
                   "kernels = each ABI call of b on its own against the copy ceiling",
           "device": torch.cuda.get_device_name(0), "csrc_sha16": build.source_digest(),
           "chunk_elems": losses.regloss_chunk_elems(), "gaussians": N, "steps": args.steps, "warmup": args.warmup,
           "copy_ceiling_tbps": COPY_CEILING_TBPS, "batches": {}}
    for B in args.batches:
        torch.manual_seed(100 + B)
        g = lambda *s: torch.randn(*s, device=dev)
        preds = {"primscale_preclip": (torch.exp(1.5 * g(B, N, 3)) * 1.0).requires_grad_(True),   # both branches populated
                 "diff_color": g(B, N, 3).requires_grad_(True), "spec_dnml": g(B, N, 3).requires_grad_(True),
                 "color_rand": g(B, N, 3).requires_grad_(True), "cos_weight": torch.rand(B, N, 1, device=dev) * 2 - 1,
                 "alpha": torch.rand(B, 1024, 1024, device=dev).requires_grad_(True)}
        preds["spec_list"] = [preds["spec_dnml"]]
        leaves = lambda name: preds[leaf_of[name]] if name != "list_l1_reg" else preds["spec_dnml"]

        def one(fns, name):
            return torch.autograd.grad(fns[name](preds), leaves(name))

        def four(fns, _name):
            loss = 0.0
            for name in RGCA:
                loss = loss + fns[name](preds)
            return torch.autograd.grad(loss, [leaves(name) for name in RGCA])

        rows = {}
        for name, run in [(n, one) for n in ours] + [("rgca_four_together", four)]:
            t = {"a": [], "b": []}
            for it in range(args.warmup + args.steps):
                for k, fns in (("a", theirs), ("b", ours)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    out = run(fns, name)
                    e1.record()
                    torch.cuda.synchronize()
                    del out
                    if it >= args.warmup:
                        t[k].append(e0.elapsed_time(e1))
            med = {k: statistics.median(v) for k, v in t.items()}
            rows[name] = {"a_ms_median": round(med["a"], 4), "a_ms_min": round(min(t["a"]), 4),
                          "b_ms_median": round(med["b"], 4), "b_ms_min": round(min(t["b"]), 4),
                          "a_over_b": round(med["a"] / med["b"], 3)}
        # (b)'s kernels on their own
        kern = {}
        for name in ours:
            per = {}
            for it in range(args.warmup + args.steps):
                _lib.TIMING = []
                try:
                    one(ours, name)
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        for fn, e0, e1 in _lib.TIMING:
                            per.setdefault(fn, []).append(e0.elapsed_time(e1))
                finally:
                    _lib.TIMING = None
            units = B * N if name == "backlit_reg" else leaves(name).numel()
            for fn, ms in per.items():
                by = {"gol_regloss_fwd": 4, "gol_regloss_bwd": 8, "gol_backlit_fwd": 16, "gol_backlit_bwd": 28}[fn]
                m = statistics.median(ms)
                tbps = units * by / (m * 1e-3) / 1e12
                kern[f"{name}:{fn}"] = {"ms_median": round(m, 4), "ms_min": round(min(ms), 4), "bytes_per_unit": by,
                                        "units": units, "effective_tbps": round(tbps, 3),
                                        "fraction_of_copy_ceiling": round(tbps / COPY_CEILING_TBPS, 3)}
        res["batches"][str(B)] = {"losses": rows, "kernels": kern}
        preds.clear()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
