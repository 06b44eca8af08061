"""Light-SH probe: device time of the fused light entry (goliath_amd.lights.headrel_light_sh -> gol_light_sh_fwd, ONE launch)
and its measured errors next to the bars tests/test_gpu_light_sh.py holds them to.

Timed shapes (deg 8): (B=8, L=512, C=3) a relight-vis batch of env lights; (B=8, L=460, C=1) a training batch padded to the
rig; (B=8, L=1, C=1) the training-only random light.  Per shape: the median over --steps of (a) one call between its own
HIP event pair -- at this size mostly the event pair and the launch -- and (b) --burst calls back to back between one event
pair, divided by the burst: what a call costs inside a stream of work.  Both include the Python wrapper (two torch.empty).
The reference path (dir2sh_torch: one operator chain and one host sync per basis function) is NOT timed here: ca_code is
not importable where this runs.  No time threshold.

Errors: the basis on the two direction sets of tests/golden/light_sh_golden.npz (max abs error vs float64, bar = 2 x the
reference's own float32 error recorded there), the recorded dir2sh_torch calls of tests/golden/rgca_model_golden.npz (bar
3 x), the four light frames (rel-L2 vs the float64 composition, bar 3e-5).

Prints one JSON line and writes it to --out (default profiles/light_sh_probe.json).

    python tools/light_sh_probe.py [--steps 200] [--warmup 20] [--burst 100] [--out FILE]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from goliath_amd import build, lights  # noqa: E402

SHAPES = ((8, 512, 3), (8, 460, 1), (8, 1, 1))
DEG = 8
BAR_FRAME = 3e-5


def _event_ms(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def _time(B, L, C, steps, warmup, burst, gen):
    lp = (torch.randn(B, L, 3, generator=gen) * 1500.0).cuda()
    li = torch.rand(B, L, C, generator=gen).cuda()
    hp = torch.cat([torch.linalg.qr(torch.randn(B, 3, 3, generator=gen))[0], torch.randn(B, 3, 1, generator=gen) * 80.0], 2).cuda()
    fn = lambda: lights.headrel_light_sh(lp, li, hp, DEG)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    single = [_event_ms(fn) for _ in range(steps)]
    bursts = [_event_ms(fn, burst) for _ in range(max(steps // 10, 5))]
    return dict(B=B, L=L, C=C, deg=DEG, call_event_pair_median_us=round(1e3 * statistics.median(single), 2),
                call_event_pair_min_us=round(1e3 * min(single), 2),
                call_in_burst_median_us=round(1e3 * statistics.median(bursts), 2), burst=burst)


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _errors():
    import npz_parts

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    G = np.load(os.path.join(ROOT, "tests", "golden", "light_sh_golden.npz"))
    out = {"basis": {}, "recorded_calls": {}, "frames": {}}
    for name in ("generic", "polar"):
        got = lights.dir2sh(DEG, t(G[f"{name}/dirs"]).cuda()).double().cpu()
        out["basis"][name] = dict(max_abs_err=float((got - t(G[f"{name}/truth"])).abs().max()),
                                  err_ref32=float(G[f"{name}/err_ref32"]), bar=2.0 * float(G[f"{name}/err_ref32"]),
                                  finite=bool(torch.isfinite(got).all()))
    R = npz_parts.load(os.path.join(ROOT, "tests", "golden", "rgca_model_golden.npz"))
    for k in R.files:
        if k.endswith("/dirs") and "/sh" in k:
            want = t(R[k[:-4] + "coeffs"]).double()
            got = lights.dir2sh(DEG, t(R[k]).cuda()).double().cpu()
            out["recorded_calls"][k[:-5]] = dict(max_abs_err=float((got - want).abs().max()),
                                                 bar=3.0 * float(G["generic/err_ref32"]))
    for i in range(4):
        f = {k: t(G[f"frame{i}/{k}"]) for k in ("light_pos", "light_intensity", "head_pose", "headrel_light_pos",
                                                "headrel_light_sh")}
        pos, sh = lights.headrel_light_sh(f["light_pos"].cuda(), f["light_intensity"].cuda(), f["head_pose"].cuda(), DEG)
        out["frames"][f"frame{i}"] = dict(shape=list(f["light_intensity"].shape),
                                          rel_l2_headrel_light_pos=_rel_l2(pos, f["headrel_light_pos"]),
                                          rel_l2_headrel_light_sh=_rel_l2(sh, f["headrel_light_sh"]), bar=BAR_FRAME)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--burst", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_sh_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("light_sh_probe needs a GPU: nothing is measured without one")
    gen = torch.Generator().manual_seed(0)
    res = dict(probe="light_sh", steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               source_digest=build.source_digest(),
               timing=[_time(B, L, C, a.steps, a.warmup, a.burst, gen) for B, L, C in SHAPES], errors=_errors())
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
