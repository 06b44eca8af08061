"""Generate tests/golden/envbg_golden.npz (in parts, tests/npz_parts.py) with the REFERENCE's own functions
(ca_code/utils/envmap.py:169-248, 325-345: pure PyTorch, run on the CPU; imported unchanged through ref_stubs).  Build
container only.  Data only.

Per case of tests/envbg_cases.py (the inputs are rebuilt from their seeds by the test, not stored):
  <case>/out        compose_envmap (compose cases) or envmap_to_image(blurbg=False) (the bicubic case) on the inputs cast to
                    float64, under torch.set_default_dtype(float64) -- the reference builds its pixel grids in the default
                    dtype -- rounded to float32
  <case>/ref32_err  [2] = max |float32 run - float64 run| over the mirror-ball square and over the rest (0 for an empty region)
  strip1/bg, strip1/bg_ref32_err   the blurred, un-clamped envmap_to_image of that case and its float32 error
The generator asserts what the cases are there for: finite outputs, both clamps of the background active, the +-pi seam and a
clamped tap row inside the bicubic case."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import envbg_cases as cases  # noqa: E402
import npz_parts  # noqa: E402
import ref_stubs  # noqa: E402


def run(fn, dtype):
    torch.set_default_dtype(dtype)
    try:
        return fn(dtype)
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    ref_stubs.install()
    import ca_code.utils.envmap as ref

    out = {}
    for name, *_ in cases.CASES:
        c = cases.build(name)
        H, W = c["H"], c["W"]

        def image(dt, blur):
            K = c["K"].to(dt)
            return ref.envmap_to_image(W, H, c["envbg"].to(dt), K[:, :2, 2], K, c["Rt"][:, :3, :3].to(dt), blurbg=blur)

        if c["compose"]:
            fn = lambda dt: ref.compose_envmap(c["render"].to(dt), c["alpha"].to(dt), c["envbg"].to(dt), c["K"].to(dt),
                                               c["Rt"].to(dt))
        else:
            fn = lambda dt: image(dt, False)
        o64, o32 = run(fn, torch.float64), run(fn, torch.float32)
        assert o64.dtype == torch.float64 and o32.dtype == torch.float32
        assert bool(torch.isfinite(o64).all()) and bool(torch.isfinite(o32).all()), name
        ball, rest = cases.regions(c)
        err = (o32.double() - o64).abs().amax(dim=(0, 1))
        e = [float(err[m].max()) if bool(m.any()) else 0.0 for m in (ball, rest)]
        out[f"{name}/out"] = o64.to(torch.float32).numpy()
        out[f"{name}/ref32_err"] = np.asarray(e, dtype=np.float64)
        print(f"{name}: out max {float(o64.abs().max()):.3f}  ref32_err ball {e[0]:.2e} rest {e[1]:.2e}")
        if c["compose"]:
            bg64, bg32 = run(lambda dt: image(dt, True), torch.float64), run(lambda dt: image(dt, True), torch.float32)
            assert bool(torch.isfinite(bg64).all()) and bool(torch.isfinite(bg32).all()), name
            hi, lo = float((bg64 > 1).float().mean()), float((bg64 < 0).float().mean())
            print(f"   bg > 1 on {100 * hi:.2f} %, bg < 0 on {100 * lo:.2f} % of the pixels")
            assert hi >= 5e-4 and lo >= 5e-4, (name, hi, lo)
            if name == cases.BG_CASE:
                out[f"{name}/bg"] = bg64.to(torch.float32).numpy()
                out[f"{name}/bg_ref32_err"] = np.asarray([float((bg32.double() - bg64).abs().max())])
                print(f"   bg ref32_err {float(out[name + '/bg_ref32_err'][0]):.2e}")
        else:
            u, v = cases.pixel_uv(c)
            assert bool((u > 0.98).any()) and bool((u < -0.98).any()), "the +-pi seam is not in the image"
            iy = (v + 1.0) * 0.5 * (c["He"] - 1)
            assert bool((iy < 1.0).any()) or bool((iy > c["He"] - 2.0).any()), "no tap row is clamped at a pole"
    path = os.path.join(HERE, "envbg_golden.npz")
    parts = npz_parts.save(path, out)
    total = sum(os.path.getsize(p) for p in parts)
    assert total < 4 << 20, total
    print("wrote", len(parts), "parts,", total, "bytes")


if __name__ == "__main__":
    main()
