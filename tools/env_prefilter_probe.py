"""Env-prefilter probe: device time of the relight pyramid of one environment map (goliath_amd.envprefilter.build_pyramid ->
gol_envprefilter_sg, two launches per prefiltered level) next to the reference's algorithm run as torch operators on the same
GPU.

Timed at 512 x 1024, miplevel 4, 4096 samples per texel: after --warmup builds, --steps builds, each synchronised and taken
by wall clock and between its own HIP event pair; median, minimum, maximum.  `levels`: prefilter_sg of each level alone
(256 x 512, 128 x 256, 64 x 128), the same way, with the samples per second it amounts to.

The torch loop: tests/envprefilter_cases.py's float32 composition (the reference's sequence of ATen calls: rand, erfinv, two
cross, two normalize, atan2, acos, grid_sample per sample; ca_code is not importable where this runs) for the same three
levels, --torch-runs runs (default 1: it takes seconds), synchronised, wall clock.  No time threshold.

Prints one JSON line and writes it to --out (default profiles/env_prefilter_probe.json).

    python tools/env_prefilter_probe.py [--steps 10] [--warmup 3] [--torch-runs 1] [--samples 4096] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import envprefilter_cases as PC  # noqa: E402
from goliath_amd import build, envprefilter  # noqa: E402

SIZE, LEVELS, SIGMA_STEP = (512, 1024), 4, 0.2


def _timed(fn):
    """(wall ms, event-pair ms) of one synchronised run."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)


def _stats(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    runs = [_timed(fn) for _ in range(steps)]
    out = {}
    for name, col in (("wall_ms", [r[0] for r in runs]), ("event_ms", [r[1] for r in runs])):
        out[name] = dict(median=round(statistics.median(col), 4), min=round(min(col), 4), max=round(max(col), 4))
    return out


def _torch_loop(inputs, samples):
    """The reference's loop (envmap.py:310-323) for every level, float32, on the GPU."""
    out = []
    for i, dirs, env in inputs:
        acc = torch.zeros_like(dirs)
        for _ in range(samples):
            x = torch.rand_like(dirs[:, :2])
            acc += PC.lookup(PC.sample_directions(x, dirs, i * SIGMA_STEP), env)
        out.append(acc / float(samples))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-runs", type=int, default=1)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_prefilter_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("env_prefilter_probe needs a GPU: nothing is measured without one")
    image = PC.hdr_map(512, *SIZE).cuda()
    S = a.samples
    with torch.no_grad():
        fused = _stats(lambda: envprefilter.build_pyramid(image, SIGMA_STEP, LEVELS, S, seed=1), a.steps, a.warmup)
        inputs = [(i, d.cuda(), env) for i, d, env in PC.pyramid_inputs(image, LEVELS)]
        levels = []
        for i, dirs, env in inputs:
            row = _stats(lambda: envprefilter.prefilter_sg(i * SIGMA_STEP, dirs, env, S, seed=i), a.steps, a.warmup)
            n = dirs.shape[2] * dirs.shape[3] * S
            row.update(level=i, H=dirs.shape[2], W=dirs.shape[3], samples=n,
                       gsamples_per_s=round(n / (1e6 * row["event_ms"]["median"]), 3))
            levels.append(row)
        loop = [_timed(lambda: _torch_loop(inputs, S))[0] for _ in range(a.torch_runs)]
        # the two agree as estimators: the RMS difference of the coarsest level against the spread of either
        ours = envprefilter.build_pyramid(image, SIGMA_STEP, LEVELS, S, seed=1)
        theirs = _torch_loop(inputs[-1:], S)
        diff = PC.rms_err(ours[-1], theirs[0])
    res = dict(probe="env_prefilter", steps=a.steps, warmup=a.warmup, samples=S, size=list(SIZE), miplevel=LEVELS,
               device=torch.cuda.get_device_name(0), source_digest=build.source_digest(), build_pyramid=fused, levels=levels,
               torch_loop_wall_ms=dict(runs=[round(t, 1) for t in loop], median=round(statistics.median(loop), 1)),
               coarsest_level_rms_difference=diff, coarsest_level_rms=float(theirs[0].double().pow(2).mean().sqrt()))
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
