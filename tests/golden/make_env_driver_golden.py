"""Generate tests/golden/env_driver_golden.npz with the REFERENCE's own relight driver on the CPU:
`EnvSpinDecorator.forward` (ca_code/utils/light_decorator.py:102-164) with what it calls, `envmap.rvec_to_R` and
`envmap.rotate_envmap_mat` (ca_code/utils/envmap.py:20-50, 141-166).

The decorator is made without __init__ (no cv2 load, no SG-prefiltered pyramid: both out of scope), `image` set to the case's
image, `sphvec` as :42-52 build it and a one-level dummy pyramid.  forward() runs unchanged; for the generic rotation
`rvec_to_R` is wrapped for the one call so that forward's own lines see rvec_to_R([0.3, -1.1, 0.7]) instead of the spin.

Cases (tests/envdriver_cases.py): sizes (16,32) (33,70) (40,72) (48,96) with HDR-like noise images u v^4 20 from
numpy.random.default_rng(1000 + H), a smooth trigonometric image at 48 x 96; per image the index batches [0], [7,128,201],
[-5,64] (cycle 256) and the generic rotation.  Recorded per call `<image>/<batch>/...`:
    rot              lightrot [B,3,3] float32 (the reference's)
    envbg, envmap, norm_scale, mip_scale      the reference's float32 outputs; light_intensity is asserted here to be
                     envmap.view(3, -1).t() bit for bit and is not stored twice; envbg at 48 x 96 holds every third row
                     (envdriver_cases.recorded_rows; the file has to stay under 1 MB)
    err_ref32/<out>  max |reference float32 - float64 composition| over the WHOLE output: the reference's own float32 error,
                     the yardstick of the tests
and per image `perc90` (np.percentile(image, 90), float32) and `checksum` (the images are regenerated from their seeds).
The full-size case (512 x 1024, seed 512; indices [7,201] and the generic rotation) records the checksum, perc90, the
rotations and the err_ref32 scalars only.

Asserted for every call: err_ref32 <= 1e-2 max|image| for envbg (a half-texel indexing mistake on the noise image gives an
error of the order of the maximum), over every pixel -- none is excluded.  Sample directions with z < 0 and |x| < 1e-6 in
float64 sit on the atan2 cut, where a sign flips the sample between the two borders of the map; `cut` (the smallest such
|x|) and `near_cut_pixels` are recorded per call.  One call has such pixels: 33 x 70 at index 64, a quarter turn whose
float32 matrix is exactly [[0,0,1],[0,1,0],[-1,0,0]] -- the centres of column 52 (x - W/2 + 0.5 = W/4) have
dx = sin(theta) cos(phi) with phi = 3.1415926 / 2, below pi / 2 by 2.7e-8: the TRUNCATED constant decides the side, the
same way in float32 and float64 (the generator asserts that the reference agrees with the composition there).
Run in the build container only (needs /root/reference):
    python tests/golden/make_env_driver_golden.py
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
import ca_code.utils.light_decorator as LD  # noqa: E402

import envdriver_cases as EC  # noqa: E402


class _Capture(torch.nn.Module):
    def forward(self, **data):
        return data


def decorator(image):
    d = LD.EnvSpinDecorator.__new__(LD.EnvSpinDecorator)
    torch.nn.Module.__init__(d)
    d.mod = _Capture()
    d.envmap_dist, d.env_scale, d.cycle, d.sigma_step, d.miplevel = EC.ENVMAP_DIST, EC.ENV_SCALE, EC.CYCLE, 0.2, 1
    d.image = image
    L = 16                                                                  # light_decorator.py:42-52
    theta, phi = np.meshgrid((np.arange(L, dtype=np.float32) + 0.5) * np.pi / L,
                             (np.arange(-L, L, dtype=np.float32) + 0.5) * np.pi / L, indexing="ij")
    sph = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], axis=0).reshape((3, -1))
    d.register_buffer("sphvec", torch.from_numpy(sph))
    d.register_buffer("mipmap_0", torch.ones(1, 3, 2, 4))
    return d


def run_reference(d, indices):
    """forward() for the index batch, or (indices None) for one view whose rot_mat is the generic rotation."""
    if indices is not None:
        return d(campos=torch.zeros(len(indices), 3), index=list(indices))
    generic = ref_envmap.rvec_to_R(torch.tensor(EC.GENERIC_RVEC))
    original = ref_envmap.rvec_to_R
    ref_envmap.rvec_to_R = lambda rvec: generic
    try:
        return d(campos=torch.zeros(1, 3), index=[0])
    finally:
        ref_envmap.rvec_to_R = original


def record(out, name, image, small):
    _, H, W = image.shape
    d = decorator(image)
    perc90 = np.percentile(image.numpy(), 90)
    assert perc90 > 0
    out[f"{name}/perc90"] = np.float32(perc90)
    out[f"{name}/checksum"] = np.array(EC.checksum(image))
    peak = float(image.max())
    for tag, indices in EC.batches(full=not small):
        data = run_reference(d, indices)
        B = data["lightrot"].shape[0]
        # norm_scale is not in `data` (forward keeps view 0's inside the scaled pyramid: ones * scale is the scale itself)
        got = dict(envbg=data["envbg"], envmap=data["envmap"], light_intensity=data["light_intensity"],
                   norm_scale=norm_scales(d, data["lightrot"]), mip_scale=data["preconv_envmap"][0][0, 0, 0, :1])
        assert torch.equal((2.0 * np.pi * got["norm_scale"][0]).reshape(1), got["mip_scale"])
        assert all(v.dtype == torch.float32 for v in got.values())
        assert torch.equal(got["light_intensity"], got["envmap"].reshape(B, 3, -1).transpose(1, 2))
        want = EC.compose64(image, data["lightrot"], perc90)
        key = f"{name}/{tag}"
        near = want["near_cut"][:, None].expand_as(want["envbg"])
        out[f"{key}/cut"], out[f"{key}/near_cut_pixels"] = np.float64(want["cut"]), np.int64(want["near_cut"].sum())
        if bool(near.any()):   # on the cut: the side must be the same in float32 and float64, or the case proves nothing
            side = EC.max_err(got["envbg"][near] * float(perc90), want["envbg"][near] * float(perc90))
            print(f"{key}: {int(want['near_cut'].sum())} pixels within {EC.CUT_EPS} of the atan2 cut (min |dx| = "
                  f"{want['cut']:.3g}); reference float32 vs float64 there: {side:.3g} (max|image| {peak:.3g})")
            assert side <= 1e-2 * peak, (key, side)
        out[f"{key}/rot"] = data["lightrot"].numpy()
        for k in EC.OUTPUTS:
            err = EC.max_err(got[k], want[k])
            if k == "envbg":
                assert err <= 1e-2 * peak / float(perc90), (key, k, err)
            out[f"{key}/err_ref32/{k}"] = np.float64(err)
        assert EC.max_err(got["envbg"] * float(perc90), want["envbg"] * float(perc90)) <= 1e-2 * peak
        if small:
            out[f"{key}/envbg"] = np.stack([got["envbg"][b][:, EC.recorded_rows(H, W, b)].numpy() for b in range(B)])
            for k in ("envmap", "norm_scale", "mip_scale"):
                out[f"{key}/{k}"] = got[k].numpy()
        print(key, "cut %.2e" % want["cut"],
              " ".join("%s %.2e" % (k, out[f"{key}/err_ref32/{k}"]) for k in EC.OUTPUTS),
              "| envbg err / max|image| = %.2e" % (out[f"{key}/err_ref32/envbg"] * float(perc90) / peak), flush=True)

def norm_scales(d, rots):
    """light_decorator.py:120-139 for each view: the reference's float32 norm_scale (forward keeps only view 0's, inside
    `preconv_envmap`)."""
    import torch.nn.functional as thf

    out = []
    for rot_mat in rots:
        new_env = ref_envmap.rotate_envmap_mat(d.image, rot_mat)
        new_env = thf.interpolate(new_env[None], (16, 32), mode="bilinear", antialias=True)[0]
        new_env_sin = new_env * torch.sin((torch.arange(new_env.shape[1]) + 0.5) * np.pi / new_env.shape[1])[None, :, None]
        out.append(d.env_scale / new_env_sin.sum())
    return torch.stack(out).float()


def main():
    out = {}
    for name, image in EC.images().items():
        record(out, name, image, True)
    record(out, "full", EC.full_image(), False)
    path = EC.GOLDEN
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
