"""Generate tests/golden/envprefilter_golden.npz with the REFERENCE's own `envmap.prefilterEnvmapSG`
(ca_code/utils/envmap.py:305-323, with importance_sample_sg :251-281 and sample_uv :284-302) on the CPU.

The draws are numpy.random.default_rng(seed) float32 arrays (tests/envprefilter_cases.py: draws, pyramid_draws) which the
tests regenerate; for the duration of a call `torch.rand_like` hands them out in iteration order, so the reference's own
lines consume them where they would consume their own.

Per parity case (envprefilter_cases.CASES) `<name>/...`:
    ref            the reference's float32 output [B,3,H,W], whole
    err_ref32      max |reference float32 - float64 composition on the same draws| over the whole output: the reference's
                   own float32 error, the yardstick of the tests
    near_cut       the number of samples with d_z < 0 and 0 < |d_x| < CUT_EPS in float64: such a sample may land on the other
                   border of the map in float32.  Asserted 0 for every case; no texel is excluded from any comparison
    exact_cut      the number of samples with d_z < 0 and d_x == 0.  The hand-made grid holds n = (0,0,-1), whose tangent
                   frame is zero (up x n = 0): every sample of that texel is d = (+-0, 0, -+1) exactly, in float32 as in
                   float64, and the SIGN of the zero picks the border.  These cannot be seeded away; asserted instead: the
                   reference and the composition agree on the whole output to 1e-3 max|map| (one sample on the other
                   border of a noise map moves a texel by about max|map| / S)
    xi_checksum    of the draws
The pyramid case `pyramid/level<i>`: light_decorator.py:64-92 restated without .cuda() (envprefilter_cases.pyramid_inputs),
the prefilter itself the reference's; `pyramid/err_ref32/level<i>` as above.
The statistics case `stat/...` (level_directions(6, 12), a 16 x 32 noise map, sigma 0.4):
    converged      the float64 composition with 2^18 samples per texel (numpy draws, seed 900): its own error is 1 / 32 of
                   an S = 256 run's
    rms_ref/S<S>   the RMS error of the reference (its own rand_like under torch.manual_seed(2000 + k)) against `converged`
                   over the 216 values, meaned over k = 0..7, for S = 64 and S = 1024
The reference is asserted to have produced no NaN anywhere.
Run in the build container only (needs /root/reference):
    python tests/golden/make_envprefilter_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_stubs  # noqa: E402

ref_stubs.install()
import ca_code.utils.envmap as ref_envmap  # noqa: E402

import envprefilter_cases as PC  # noqa: E402


def reference_on_draws(sigma, v, env, xi):
    """envmap.prefilterEnvmapSG(sigma, v, env, len(xi)) with rand_like handing out xi[0], xi[1], ..."""
    it = iter(xi)
    original = torch.rand_like

    def rand_like(t, *a, **k):
        x = next(it)
        assert tuple(x.shape) == tuple(t.shape) and x.dtype == t.dtype
        return x.clone()

    torch.rand_like = rand_like
    try:
        out = ref_envmap.prefilterEnvmapSG(sigma, v, env, len(xi))
    finally:
        torch.rand_like = original
    assert next(it, None) is None
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all()), "the reference produced a NaN"
    return out


def record(out, key, sigma, v, env, xi):
    ref = reference_on_draws(sigma, v, env, xi)
    stats = {}
    want = PC.compose(sigma, v, env, xi, torch.float64, stats)
    err, peak = PC.max_err(ref, want), float(env.abs().max())
    f32 = PC.max_err(PC.compose(sigma, v, env, xi, torch.float32), ref)
    print(f"{key}: err_ref32 {err:.3e} (max|map| {peak:.3g}), float32 composition vs reference {f32:.3e}, "
          f"near_cut {stats['near_cut']}, exact_cut {stats['exact_cut']}", flush=True)
    assert stats["near_cut"] == 0, (key, stats)
    assert err <= 1e-3 * peak, (key, err)
    assert f32 <= err, (key, f32, err)          # what tests/test_envprefilter_api.py asks of the composition
    return ref, err, stats


def main():
    out = {}
    for name in PC.CASES:
        sigma, v, env, xi = PC.case(name)
        ref, err, stats = record(out, name, sigma, v, env, xi)
        out[f"{name}/ref"] = ref.numpy()
        out[f"{name}/err_ref32"] = np.float64(err)
        out[f"{name}/near_cut"], out[f"{name}/exact_cut"] = np.int64(stats["near_cut"]), np.int64(stats["exact_cut"])
        out[f"{name}/xi_checksum"] = np.array(PC.checksum(xi))

    image = PC.pyramid_image()
    for (i, dirs, env), xi in zip(PC.pyramid_inputs(image), PC.pyramid_draws()):
        ref, err, _ = record(out, f"pyramid/level{i}", i * PC.PYR_SIGMA_STEP, dirs, env, xi)
        out[f"pyramid/level{i}"] = ref.numpy()
        out[f"pyramid/err_ref32/level{i}"] = np.float64(err)
    out["pyramid/checksum"] = np.array(PC.checksum(image))

    sigma, v, env = PC.stat_case()
    rng = np.random.default_rng(900)
    total = torch.zeros(v.shape, dtype=torch.float64)
    block = 4096
    for s in range(0, PC.STAT_CONVERGED_S, block):
        xi = torch.from_numpy(rng.random((block, 1, 2, *PC.STAT_GRID), dtype=np.float32))
        total += PC.compose_batched(sigma, v, env, xi) * block
    converged = total / PC.STAT_CONVERGED_S
    out["stat/converged"] = converged.numpy()
    for S in PC.STAT_S:
        rms = []
        for k in range(PC.STAT_SEEDS):
            torch.manual_seed(2000 + k)
            got = ref_envmap.prefilterEnvmapSG(sigma, v, env, S)
            assert bool(torch.isfinite(got).all())
            rms.append(PC.rms_err(got, converged))
        out[f"stat/rms_ref/S{S}"] = np.float64(np.mean(rms))
        print(f"stat S={S}: reference RMS error {np.mean(rms):.4e} (spread {np.std(rms):.2e} over {len(rms)} seeds)", flush=True)
    print("stat: reference error ratio S64 / S1024 = %.3f" % (out["stat/rms_ref/S64"] / out["stat/rms_ref/S1024"]))

    np.savez_compressed(PC.GOLDEN, **out)
    print(PC.GOLDEN, os.path.getsize(PC.GOLDEN), "bytes")
    assert os.path.getsize(PC.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main()
