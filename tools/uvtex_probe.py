"""uvtex probe: URHand's texture tail on goliath_amd.uvtex against the reference's lines as torch operators, on one GPU.

What is timed is `goliath_amd.urhand.texture_stretch` -- the stretch of AutoEncoder.forward from relight_preds["tex"] to the
four RGBA textures the renderer takes (tex, phys_tex and the two normal-colour textures; urhand.py:721-747, :788-807,
:824-832, :843-847), NOT the whole model -- on a stand-in AutoEncoder (tests/uvtex_standin.py: recorded decoder outputs, a
CalV5-shaped cal in train() mode with a colour, a grey and the identity camera in the batch), with the flag off (torch operators, the parent's path) and on (gol_uvtex_fwd / _bwd,
gol_pack_rgba_*, gol_normal_rgba).  The backward drives seeded cotangents into the tex and phys_tex RGBA textures, as the
two differentiable renders do; gradients reach the decoder's tex, phys_tex and the cal parameters.

Seams: `probe_seams` -- a band of two rows, two columns and the diagonal (5 S texels, 0.5 % of the map) whose texels sample
the point mirrored through the map's centre plus a sub-texel offset, weights in (0.05, 0.95): one-to-one, as the two sides
of a real seam are, so a CSR row holds at most a few entries.  The tests' seams (tests/uvtex_cases.py) instead point 4 S
band texels at ONE destination; one lane walks such a row alone, and the extra row `long_row` times that case (B = 1).

Size: S = 1024; B in {1, 8}; C in {4, 6}; forward alone and forward + backward.  Method: both paths alternate in ONE process
on the same inputs; --warmup untimed passes of each, then --boxes boxes of --reps timed passes each (HIP events around a
box, one synchronise per box); per row the median over the boxes and their spread (max - min).  A row counts as faster only
when the fused median is below the torch median by more than the torch path's own spread; the others are named in
`not_faster`.  Before timing, both float32 paths are compared with the torch lines run in float64 on the same inputs
(relative L2, worst output / worst gradient of each path).

    python tools/uvtex_probe.py [--boxes 7] [--reps 20] [--warmup 3] [--out profiles/uvtex_probe.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import uvtex_standin as standin  # noqa: E402
from goliath_amd import build, urhand  # noqa: E402

S = 1024


class ProbeSeams(torch.nn.Module):
    """SeamSampler-shaped (uvs, weights, resample): see the module docstring."""

    def __init__(self, S):
        super().__init__()
        g = torch.Generator().manual_seed(S)
        rows, cols = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
        uvs = torch.stack([(cols + 0.5) / S, (rows + 0.5) / S], dim=-1).to(torch.float32)
        band = torch.zeros(S, S, dtype=torch.bool)
        band[S // 5] = band[S - S // 3] = True
        band[:, S // 4] = band[:, S - S // 7] = True
        band[torch.arange(S), torch.arange(S)] = True
        n = int(band.sum())
        jit = torch.rand(n, 2, generator=g)
        uvs[band] = torch.stack([(S - 1 - cols[band] + jit[:, 0]) / S, (S - 1 - rows[band] + jit[:, 1]) / S], dim=-1)
        w = torch.zeros(S, S)
        w[band] = 0.05 + 0.9 * torch.rand(n, generator=g)
        self.register_buffer("uvs", uvs)
        self.register_buffer("weights", w.reshape(1, 1, S, S))

    resample = standin._Seams.resample


def make(B, C, long_row=False):
    model = standin.StandInAutoEncoder(S=S, B=B, C=C, seed=B + C, seam_sampler=None if long_row else ProbeSeams(S)).cuda().train()
    batch = standin.StandInAutoEncoder.batch(B, seed=B, device="cuda", cams=("400002", "410011", "400004"))
    g = torch.Generator().manual_seed(1)
    cot = [torch.randn(B, 4, S, S, generator=g).cuda() for _ in range(2)]
    return model, batch, cot


def step(model, batch, cot, fused, backward):
    relight = model.decoder_relight()
    tex_mean = model.tex_mean.repeat(batch["Rt"].shape[0], 1, 1, 1)       # urhand.py:765, part of the parent's cost only
    out = urhand.texture_stretch(model, relight, tex_mean, {"camera": batch["camera_id"], "frame": None}, batch["Rt"], fused)
    if backward:
        model.zero_grad(set_to_none=True)
        torch.autograd.backward([out[2], out[3]], cot)
    return out


def timed(fn, boxes, reps):
    ms = []
    for _ in range(boxes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def rel_l2(a, b):
    return float((a.detach().double() - b.detach().double()).norm() / b.detach().double().norm().clamp_min(1e-300))


def grads_of(model):
    return [model.decoder_relight.tex.grad.clone(), model.decoder_relight.phys_tex.grad.clone(), model.cal.params.grad.clone()]


def parity_vs_float64(model, batch, cot):
    """Worst relative L2 of each float32 path against the torch lines in float64: (outputs, gradients) per path."""
    m64 = copy.deepcopy(model).double()
    b64 = dict(batch, Rt=batch["Rt"].double())
    want = step(m64, b64, [c.double() for c in cot], False, True)
    g_want = grads_of(m64)
    out = {}
    for fused, tag in ((False, "torch"), (True, "fused")):
        got = step(model, batch, cot, fused, True)
        out[tag] = dict(outputs=max(rel_l2(a, b) for a, b in zip(got, want)),
                        gradients=max(rel_l2(a, b) for a, b in zip(grads_of(model), g_want)))
    del m64, want, g_want
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uvtex_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uvtex_probe needs a GPU: a timing taken elsewhere says nothing")
    rows, not_faster = [], []
    for B, C, long_row in [(1, 4, False), (1, 6, False), (8, 4, False), (8, 6, False), (1, 4, True)]:
        model, batch, cot = make(B, C, long_row)
        parity = parity_vs_float64(model, batch, cot)
        for backward in (False, True):
            runs = {f: (lambda f=f: step(model, batch, cot, f, backward)) for f in (False, True)}
            for _ in range(args.warmup):
                for f in (False, True):
                    runs[f]()
            torch.cuda.synchronize()
            ms = {False: [], True: []}
            for _ in range(args.boxes):                              # alternate the two paths box by box
                for f in (False, True):
                    ms[f] += timed(runs[f], 1, args.reps)
            row = dict(B=B, C=C, S=S, seams="long_row" if long_row else "one_to_one", mode="fwd+bwd" if backward else "fwd",
                       parity_vs_float64=parity)
            for f, tag in ((False, "torch"), (True, "fused")):
                row[tag + "_ms_median"] = statistics.median(ms[f])
                row[tag + "_ms_spread"] = max(ms[f]) - min(ms[f])
                row[tag + "_ms_boxes"] = ms[f]
            row["speedup"] = row["torch_ms_median"] / row["fused_ms_median"]
            row["faster_beyond_spread"] = row["fused_ms_median"] < row["torch_ms_median"] - row["torch_ms_spread"]
            if not row["faster_beyond_spread"]:
                not_faster.append(f"B={B} C={C} {row['seams']} {row['mode']}")
            rows.append(row)
            print(f"B={B} C={C} {row['seams']:10s} {row['mode']:8s} torch {row['torch_ms_median']:8.3f} ms (spread "
                  f"{row['torch_ms_spread']:.3f})  fused {row['fused_ms_median']:8.3f} ms (spread {row['fused_ms_spread']:.3f})  "
                  f"x{row['speedup']:.2f}  vs float64: {parity}", flush=True)
        del model, batch, cot
        torch.cuda.empty_cache()
    out = dict(tool="tools/uvtex_probe.py", device=torch.cuda.get_device_name(0), source_digest=build.source_digest(),
               method=f"HIP events, {args.warmup} warm-up passes, {args.boxes} boxes x {args.reps} passes, paths alternating",
               what="texture_stretch: relight_preds['tex'] -> tex / phys_tex / 2 normal RGBA textures; torch = flag off",
               rows=rows, not_faster=not_faster)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
