"""MVP primitive-assembly probe: the PyTorch chain of hand_mvp.AutoEncoder.render + Raymarcher (cat / view / permute /
reshape, then template[:, valid_prims].contiguous()) against goliath_amd.mvpprims.assemble_template (csrc/mvpprims.hip).

Config-5 size: K = 4096 primitives of (16, 16, 8) on a 1024^2 slab, B in {1, 4}, about 70 % of the primitives valid and all
valid.  Medians over --reps passes after --warmup, HIP events, the two versions alternating inside every pass, of the
forward (leaves requiring grad, as in training) and of forward + backward.  The two template kernels and the two transform
kernels are also timed one by one (HIP events around each ABI call); the template kernels are set against their
algorithmic bytes -- (4 TD TH TW 4) (Kv read + Kv written) per view forward, (Kv read + K written) backward -- as a fraction
of 8 TB/s.  The outputs and gradients of the two versions are compared (torch.equal) at the timed size.  Prints one JSON
line and writes it to --out.

    python tools/mvp_prims_probe.py [--reps 7] [--warmup 2] [--out profiles/mvp_prims_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import mvpprims_cases as cases  # noqa: E402
from goliath_amd import _lib, build, mvpprims  # noqa: E402

PRIMSIZE, NY, NX = (16, 16, 8), 64, 64
HBM = 8e12


def _chain(rgb, alpha, valid):
    """The parent path: hand_mvp.py:171-185, then render_raymarcher.py:41-47."""
    TW, TH, TD = PRIMSIZE
    B = rgb.shape[0]
    t = torch.cat([rgb, alpha], 2).view(B, TD, 4, NY, TH, NX, TW).permute(0, 3, 5, 1, 4, 6, 2)
    t = t.reshape(B, NY * NX, TD, TH, TW, 4)
    return t if valid is None else t[:, valid].contiguous()


def _alternating_medians(fns, reps, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: round(statistics.median(v), 3) for k, v in times.items()}


def _entry_times(fn, reps):
    per = {}
    for _ in range(reps):
        _lib.TIMING = []
        try:
            fn()
            torch.cuda.synchronize()
            for name, e0, e1 in _lib.TIMING:
                per.setdefault(name, []).append(e0.elapsed_time(e1))
        finally:
            _lib.TIMING = None
    return {k: round(statistics.median(v), 4) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvp_prims_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mvp_prims_probe needs a GPU: a time taken anywhere else says nothing")
    TW, TH, TD = PRIMSIZE
    K = NY * NX
    prim_bytes = 4 * TD * TH * TW * 4
    g = torch.Generator().manual_seed(0)
    masks = {"70pct": (torch.rand(K, generator=g) < 0.7).cuda(), "all": torch.ones(K, dtype=torch.bool).cuda()}
    rows = []
    for B in (1, 4):
        rgb = torch.randn(B, TD, 3, NY * TH, NX * TW, device="cuda").requires_grad_(True)
        alpha = torch.randn(B, TD, 1, NY * TH, NX * TW, device="cuda").requires_grad_(True)
        for mname, valid in masks.items():
            Kv = mvpprims.prim_slots(valid)[2]
            up = torch.randn(B, Kv, TD, TH, TW, 4, device="cuda")

            def fwd(f):
                return f(rgb, alpha, valid)

            def fwd_bwd(f):
                rgb.grad, alpha.grad = None, None
                f(rgb, alpha, valid).backward(up)

            fused = lambda r, al, v: mvpprims.assemble_template(r, al, PRIMSIZE, valid_prims=v)
            with torch.no_grad():
                same_fwd = torch.equal(_chain(rgb, alpha, valid), fused(rgb, alpha, valid))
            fwd_bwd(_chain)
            ref = (rgb.grad.clone(), alpha.grad.clone())
            fwd_bwd(fused)
            same_bwd = torch.equal(rgb.grad, ref[0]) and torch.equal(alpha.grad, ref[1])
            del ref
            t_fwd = _alternating_medians({"torch": lambda: fwd(_chain), "fused": lambda: fwd(fused)}, a.reps, a.warmup)
            t_fb = _alternating_medians({"torch": lambda: fwd_bwd(_chain), "fused": lambda: fwd_bwd(fused)}, a.reps, a.warmup)
            kt = _entry_times(lambda: fwd_bwd(fused), a.reps)
            nbytes = {"gol_mvp_template_fwd": B * prim_bytes * (Kv + Kv), "gol_mvp_template_bwd": B * prim_bytes * (Kv + K)}
            kern = {n: dict(ms=kt.get(n), bytes=nb, hbm_fraction=round(nb / (kt[n] * 1e-3) / HBM, 3) if kt.get(n) else None)
                    for n, nb in nbytes.items()}
            row = dict(B=B, mask=mname, K=K, Kv=Kv, equal_forward=same_fwd, equal_backward=same_bwd,
                       fwd_ms=t_fwd, fwd_bwd_ms=t_fb, speedup_fwd=round(t_fwd["torch"] / t_fwd["fused"], 2),
                       speedup_fwd_bwd=round(t_fb["torch"] / t_fb["fused"], 2), fused_kernels=kern)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
            rgb.grad, alpha.grad = None, None
    # the transform tail: the PyTorch restatement of hand_mvp.py:410-425 (tests/mvpprims_cases.py: fewer launches than the
    # reference's nine nested stacks) against one launch each way
    tr = {}
    for B in (1, 4):
        q = torch.nn.functional.normalize(torch.randn(B, K, 4, device="cuda"), dim=-1)
        rot = torch.stack([q[..., :3], torch.roll(q[..., :3], 1, -1), torch.roll(q[..., :3], 2, -1)], -2).contiguous()
        pos = torch.randn(B, K, 3, device="cuda")
        d = [torch.randn(B, K, 3, device="cuda").mul_(s).requires_grad_(True) for s in (1e-4, 0.01, 1.0)]

        def torch_tail():
            return cases.transform_tail(pos, rot, d[0], d[1], d[2], 512)

        def fused_tail():
            return mvpprims.prim_transforms(pos, rot, d[0], d[1], d[2], 512)

        def fb(f):
            for t in d:
                t.grad = None
            p, r, s = f()
            (p.sum() + r.sum() + s.sum()).backward()

        t = _alternating_medians({"torch": lambda: fb(torch_tail), "fused": lambda: fb(fused_tail)}, a.reps, a.warmup)
        kt = _entry_times(lambda: fb(fused_tail), a.reps)
        tr[f"B{B}"] = dict(fwd_bwd_ms=t, kernels={k: v for k, v in kt.items() if "primtransf" in k})
    res = dict(probe="mvp_prims", primsize=PRIMSIZE, K=K, reps=a.reps, warmup=a.warmup, hbm_peak=HBM,
               device=torch.cuda.get_device_name(0), source_digest=build.source_digest(), template=rows, transforms=tr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
