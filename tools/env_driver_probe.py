"""Env-driver probe: device time of one relight frame's driver work (goliath_amd.envdriver.EnvSpin.frame -> gol_envspin_frame,
three launches) next to the host lines it replaces, and its measured errors next to the bars tests/test_gpu_env_driver.py
holds them to.

Timed at 512 x 1024 for B = 1 and B = 8, `index` a device tensor (the rotations are built on the device as well): the
median over --steps of (a) one call between its own HIP event pair and (b) --burst calls back to back between one event
pair, divided by the burst: what a call costs inside a stream of work.  Both include the Python wrapper (the small tensor
operators of spin_lightrot, six torch.empty).  `frame_lightrot_*`: the same with the rotations given (the kernels and the
allocations only).

Host lines, per VIEW, on this machine's CPU with torch's default thread count (recorded), composed in torch from the
formulas (ca_code is not importable where this runs): the rotated map by a CPU grid_sample of the 3 x 512 x 1024 image
(envmap.py:141-166), np.percentile(image, 90) (light_decorator.py:123) and the antialiased interpolate to 16 x 32
(:128-130); median of --host-runs runs each.  No time threshold.

Errors: the full-size case of tests/golden/env_driver_golden.npz (max abs error of every output vs the float64 composition
on our float32 rotations, bar = 2 x the reference's own float32 error recorded there).

Prints one JSON line and writes it to --out (default profiles/env_driver_probe.json).

    python tools/env_driver_probe.py [--steps 100] [--warmup 20] [--burst 100] [--host-runs 5] [--out FILE]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import envdriver_cases as EC  # noqa: E402
from goliath_amd import build, envdriver  # noqa: E402


def _event_ms(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def _time(fn, steps, warmup, burst):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    single = [_event_ms(fn) for _ in range(steps)]
    bursts = [_event_ms(fn, burst) for _ in range(max(steps // 10, 5))]
    return dict(call_event_pair_median_us=round(1e3 * statistics.median(single), 2),
                call_event_pair_min_us=round(1e3 * min(single), 2),
                call_in_burst_median_us=round(1e3 * statistics.median(bursts), 2), burst=burst)


def _host_lines(image, runs):
    """The per-view host work of light_decorator.py:120-130, composed in torch (float32, CPU)."""
    _, H, W = image.shape
    rot = envdriver.spin_lightrot([7], EC.CYCLE, "cpu")[0]

    def rotate():
        theta, phi = torch.meshgrid((torch.arange(H, dtype=torch.float32) + 0.5) * 3.1415926 / H,
                                    (torch.arange(-W // 2, W // 2, dtype=torch.float32) + 0.5) * 3.1415926 * 2 / W, indexing="ij")
        vec = torch.stack([torch.sin(theta) * torch.sin(phi), torch.cos(theta), torch.sin(theta) * torch.cos(phi)], dim=-1)
        vec = torch.clamp(torch.matmul(vec, rot.T.contiguous()[None]), -1, 1)
        u = (1 / np.pi) * torch.atan2(vec[:, :, 0], vec[:, :, 2])
        v = 2 * (1 / np.pi) * torch.acos(vec[:, :, 1]) - 1.0
        return F.grid_sample(image[None], torch.stack([u, v], -1)[None], padding_mode="border", align_corners=False)[0]

    new_env = rotate()
    arr = image.numpy()

    def med(fn):
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return round(statistics.median(ts), 2)

    return dict(torch_threads=torch.get_num_threads(), runs=runs, rotate_grid_sample_ms=med(rotate),
                percentile_ms=med(lambda: np.percentile(arr, 90)),
                antialiased_interpolate_ms=med(lambda: F.interpolate(new_env[None], (16, 32), mode="bilinear", antialias=True)))


def _errors(image, spin):
    G = np.load(EC.GOLDEN)
    out = {}
    for tag, indices in EC.batches(full=True):
        key = f"full/{tag}"
        fr = spin.frame(index=indices) if indices is not None else spin.frame(lightrot=torch.from_numpy(G[f"{key}/rot"]).cuda())
        want = EC.compose64(image, fr.lightrot.cpu(), G["full/perc90"])
        out[tag] = {k: dict(max_abs_err=EC.max_err(getattr(fr, k), want[k]), err_ref32=float(G[f"{key}/err_ref32/{k}"]),
                            bar=2.0 * float(G[f"{key}/err_ref32/{k}"])) for k in EC.OUTPUTS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--burst", type=int, default=100)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_driver_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("env_driver_probe needs a GPU: nothing is measured without one")
    image = EC.full_image()
    spin = envdriver.EnvSpin(image, EC.ENV_SCALE, cycle=EC.CYCLE, envmap_dist=EC.ENVMAP_DIST)
    timing = []
    for B in (1, 8):
        idx = torch.arange(7, 7 + 13 * B, 13, device="cuda")
        rot = envdriver.spin_lightrot(idx, EC.CYCLE, "cuda")
        row = dict(B=B, H=spin.H, W=spin.W, frame_index=_time(lambda: spin.frame(index=idx), a.steps, a.warmup, a.burst),
                   frame_lightrot=_time(lambda: spin.frame(lightrot=rot), a.steps, a.warmup, a.burst),
                   frame_lightrot_no_envbg=_time(lambda: spin.frame(lightrot=rot, want_envbg=False), a.steps, a.warmup, a.burst))
        timing.append(row)
    res = dict(probe="env_driver", steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               source_digest=build.source_digest(), timing=timing, host_lines_per_view=_host_lines(image, a.host_runs),
               errors=_errors(image, spin))
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
