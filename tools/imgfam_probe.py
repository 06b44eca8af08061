"""Time the image-sized work around the L2 / focus image losses at the reference-native size (B x 3 x 2048 x 1334, B = 8 and
1), two ways in one process, interleaved:

    a  the torch composition of the reference's lines (ca_code/loss/__init__.py:366-386, 496-538,
       ca_code/utils/geom.py:768-794, ca_code/utils/image.py:393-422)
    b  the fused operators of goliath_amd.losses / goliath_amd.imageops (gol_imgloss_*, gol_mask_erode, gol_depth_disc_mask)

for rgb_l2 with mask_erode = 3 and a boolean depth_disc_mask, for rgb_l1_focus + rgb_l1_phys together, and for
depth_discontinuity_mask.  A pass is the loss and torch.autograd.grad to the prediction(s) (the mask operator: the call)
between two events on the stream; 3 warm-up and 20 timed passes per variant, median and minimum.  For (b) a second set of
passes times every kernel on its own (events around each ABI call) and reports it as a fraction of the copy ceiling on the
algorithmic bytes: per element forward 8 + 4 [mask] / C' + 1 [veto] / C (C' = C for a one-channel mask, else 1), backward the
same + 4; depth -> mask 5 B per pixel, the erosion of a float mask 8 B per pixel.  Prints one JSON line; --out writes it to a
file too.

    python tools/imgfam_probe.py [--steps 20] [--warmup 3] [--out profiles/imgfam_probe.json]
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
H, W, C = 2048, 1334, 3


def torch_ops():
    """The reference's lines, verbatim up to the dictionary lookups."""
    def erode(x, ks):
        flip = 1 - x
        w = torch.ones(1, 1, ks, ks, device=x.device)
        return 1 - (F.conv2d(flip, w, padding=ks // 2) > 0).to(dtype=x.dtype)

    def rgb_l2(p, t, mask_erode=3):
        mask = erode(t["image_mask"].to(torch.float32), mask_erode).to(torch.bool)
        mask = mask * ~p["depth_disc_mask"]
        return ((p["rendered_rgb"] - t["image"]) * mask).pow(2).mean()

    def focus(p, t, key):
        mask = t["image_mask"] * ~p["depth_disc_mask"]
        abs_error = ((p[key] - t["image"]) * mask).abs()
        error_weights = torch.exp(abs_error / 255.).detach()
        return (abs_error * error_weights).mean()

    def depth_discontuity_mask(depth, threshold=40.0, pool_ksize=3):
        with torch.no_grad():
            kernel = torch.as_tensor([[[[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]], [[[-1, -2, -1], [0, 0, 0], [1, 2, 1]]]],
                                     dtype=torch.float32, device=depth.device)
            disc = (torch.norm(F.conv2d(depth, kernel, bias=None, padding=1), dim=1) > threshold)[:, None]
            return F.avg_pool2d(disc.float(), pool_ksize, stride=1, padding=pool_ksize // 2) > 0.0

    return {"rgb_l2_erode3": lambda p, t: rgb_l2(p, t),
            "focus_plus_phys": lambda p, t: focus(p, t, "rendered_rgb") + focus(p, t, "rendered_phys_rgb"),
            "depth_discontinuity_mask": lambda p, t: depth_discontuity_mask(p["depth"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from goliath_amd import _lib, build, imageops, losses

    dev = torch.device("cuda", 0)
    ours = {"rgb_l2_erode3": lambda p, t: losses.rgb_l2(p, t, mask_erode=3),
            "focus_plus_phys": lambda p, t: losses.rgb_l1_focus(p, t) + losses.rgb_l1_phys(p, t),
            "depth_discontinuity_mask": lambda p, t: imageops.depth_discontinuity_mask(p["depth"])}
    theirs = torch_ops()
    leaves_of = {"rgb_l2_erode3": ("rendered_rgb",), "focus_plus_phys": ("rendered_rgb", "rendered_phys_rgb"),
                 "depth_discontinuity_mask": ()}
    res = {"what": "forward + backward of the image losses (the mask operator: the call), ms between two events on the stream "
                   "(median / min over the timed passes): a = torch composition of the reference's lines, b = goliath_amd; "
                   "kernels = each ABI call of b on its own against the copy ceiling",
           "device": torch.cuda.get_device_name(0), "csrc_sha16": build.source_digest(),
           "chunk_elems": losses.imgloss_chunk_elems(), "image": [C, H, W], "steps": args.steps, "warmup": args.warmup,
           "copy_ceiling_tbps": COPY_CEILING_TBPS, "batches": {}}
    for B in args.batches:
        torch.manual_seed(100 + B)
        yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        hand = (((yy - H / 2) / (0.4 * H)) ** 2 + ((xx - W / 2) / (0.35 * W)) ** 2 < 1.0)
        depth = torch.where(hand, 600.0 + 0.2 * xx, torch.zeros((), device=dev)).expand(B, 1, H, W).contiguous()
        depth = depth + 2.0 * torch.rand(B, 1, H, W, device=dev) * hand
        preds = {"rendered_rgb": (255 * torch.rand(B, C, H, W, device=dev)).requires_grad_(True),
                 "rendered_phys_rgb": (255 * torch.rand(B, C, H, W, device=dev)).requires_grad_(True),
                 "depth": depth, "depth_disc_mask": imageops.depth_discontinuity_mask(depth)}
        targets = {"image": 255 * torch.rand(B, C, H, W, device=dev), "image_mask": hand.float().expand(B, 1, H, W).contiguous()}

        def run(fns, name):
            out = fns[name](preds, targets)
            if leaves_of[name]:
                return torch.autograd.grad(out, [preds[k] for k in leaves_of[name]])
            return out

        rows = {}
        for name in ours:
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
        # (b)'s kernels on their own; per call the algorithmic bytes of the configuration it runs in
        px, el = B * H * W, B * C * H * W
        fwd_b = 8 * el + 4 * px + 1 * px        # one-channel float mask and byte veto, read once per channel plane in the model
        model = {"rgb_l2_erode3": {"gol_mask_erode": 8 * px, "gol_imgloss_fwd": fwd_b, "gol_imgloss_bwd": fwd_b + 4 * el,
                                   "gol_imgloss_finalize": None},
                 "focus_plus_phys": {"gol_imgloss_fwd": fwd_b, "gol_imgloss_bwd": fwd_b + 4 * el, "gol_imgloss_finalize": None},
                 "depth_discontinuity_mask": {"gol_depth_disc_mask": 5 * px}}
        kern = {}
        for name in ours:
            per = {}
            for it in range(args.warmup + args.steps):
                _lib.TIMING = []
                try:
                    run(ours, name)
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        for fn, e0, e1 in _lib.TIMING:
                            per.setdefault(fn, []).append(e0.elapsed_time(e1))
                finally:
                    _lib.TIMING = None
            for fn, ms in per.items():
                m = statistics.median(ms)
                row = {"ms_median": round(m, 4), "ms_min": round(min(ms), 4), "calls_per_pass": len(ms) // args.steps}
                by = model[name][fn]
                if by is not None:
                    tbps = by / (m * 1e-3) / 1e12
                    row.update(bytes=by, effective_tbps=round(tbps, 3), fraction_of_copy_ceiling=round(tbps / COPY_CEILING_TBPS, 3))
                kern[f"{name}:{fn}"] = row
        res["batches"][str(B)] = {"losses": rows, "kernels": kern}
        preds.clear()
        targets.clear()
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
