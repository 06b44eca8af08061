"""Generate tests/golden/light_sh_golden.npz with the REFERENCE's own `dir2sh_torch` (ca_code/utils/sh.py:118-127) on the CPU.

Two direction sets, each with the float32 directions, dir2sh_torch(8, .) of them evaluated in float64 (`truth`) and the
scalar err_ref32 = max |dir2sh_torch(8, float32 dirs) - truth|, the reference's own float32 error -- the yardstick of
tests/test_gpu_light_sh.py:
    generic   250 seeded unit directions with |z| <= 0.999, the six axis directions, the zero vector
    polar     60 directions with sin(theta) in [0, 1e-2]: both exact poles, the rest log-spaced from 1e-6 (those below about 2e-4 round to
              z = +-1 in float32: inside the 1e-4 floor band of sh.py:60) at azimuths that walk round the circle, alternating
              hemispheres
Four light-frame cases (`frame{i}/...`): light_pos, light_intensity, head_pose and the composition of
ca_code/models/rgca.py:175-191 (the statements are written out below, every operand in float64, the SH basis the
reference's dir2sh_torch): headrel_light_pos and headrel_light_sh.
    frame0  B=1 L=1    C=3  identity pose
    frame1  B=2 L=3    C=1
    frame2  B=2 L=512  C=3
    frame3  B=3 L=257  C=1  the last 100 lights padded as the dataloader pads (position 0, intensity 0)
The file holds inputs and recorded results only.  Run in the build container only (needs /root/reference):
    python tests/golden/make_light_sh_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, "/root/reference")
import ca_code.utils.sh as ref_sh  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEG = 8


def generic_dirs(g):
    d = []
    while len(d) < 250:
        v = F.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0)
        if abs(float(v[2])) <= 0.999:
            d.append(v)
    axes = torch.cat([torch.eye(3, dtype=torch.float64), -torch.eye(3, dtype=torch.float64)])
    return torch.cat([torch.stack(d), axes, torch.zeros(1, 3, dtype=torch.float64)]).float()


def polar_dirs():
    st = torch.cat([torch.zeros(2, dtype=torch.float64), torch.logspace(-6, -2, 58, dtype=torch.float64)])
    sign = torch.where(torch.arange(60) % 2 == 0, 1.0, -1.0).double()
    phi = torch.arange(60, dtype=torch.float64) * 2.399963229728653   # the golden angle: every azimuth quadrant
    z = sign * torch.sqrt(1.0 - st * st)
    return torch.stack([st * torch.cos(phi), st * torch.sin(phi), z], -1).float()


def record_set(out, name, dirs):
    truth = ref_sh.dir2sh_torch(DEG, dirs.double())
    got32 = ref_sh.dir2sh_torch(DEG, dirs)
    assert got32.dtype == torch.float32 and bool(torch.isfinite(truth).all())
    out[f"{name}/dirs"] = dirs.numpy()
    out[f"{name}/truth"] = truth.numpy()
    out[f"{name}/err_ref32"] = np.float64((got32.double() - truth).abs().max())
    print(name, tuple(dirs.shape), "err_ref32 = %.3e" % out[f"{name}/err_ref32"])


def rotation(g):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    return q if torch.det(q) > 0 else -q


def frame(out, i, B, L, C, g, identity=False, padded=0):
    light_pos = (torch.randn(B, L, 3, generator=g) * 1500.0)
    light_intensity = torch.rand(B, L, C, generator=g) * 2.0
    if padded:
        light_pos[:, L - padded:] = 0.0
        light_intensity[:, L - padded:] = 0.0
    if identity:
        head_pose = torch.eye(4)[:3][None].repeat(B, 1, 1)
    else:
        head_pose = torch.stack([torch.cat([rotation(g), torch.randn(3, 1, generator=g, dtype=torch.float64) * 80.0], 1)
                                 for _ in range(B)]).float()
    # rgca.py:175-191 on the float32 inputs, evaluated in float64
    li = light_intensity.double().expand(-1, -1, 3)
    hp = head_pose.double()
    rot, trans = hp[:, :3, :3], hp[:, :3, 3]
    headrel_light_pos = (light_pos.double() - trans[:, None]) @ rot
    sh_coeffs = ref_sh.dir2sh_torch(DEG, F.normalize(headrel_light_pos, p=2, dim=-1))
    headrel_light_sh = (sh_coeffs[:, :, None] * li[..., None]).sum(dim=1)
    out[f"frame{i}/light_pos"] = light_pos.numpy()
    out[f"frame{i}/light_intensity"] = light_intensity.numpy()
    out[f"frame{i}/head_pose"] = head_pose.numpy()
    out[f"frame{i}/headrel_light_pos"] = headrel_light_pos.numpy()
    out[f"frame{i}/headrel_light_sh"] = headrel_light_sh.numpy()
    out[f"frame{i}/padded"] = np.int64(padded)


def main():
    g = torch.Generator().manual_seed(20240531)
    out = {}
    record_set(out, "generic", generic_dirs(g))
    record_set(out, "polar", polar_dirs())
    frame(out, 0, 1, 1, 3, g, identity=True)
    frame(out, 1, 2, 3, 1, g)
    frame(out, 2, 2, 512, 3, g)
    frame(out, 3, 3, 257, 1, g, padded=100)
    path = os.path.join(HERE, "light_sh_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
