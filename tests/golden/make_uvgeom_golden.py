"""Generate tests/golden/uvgeom_golden.partNN.npz by running the REFERENCE's own `values_to_uv` and `vert_normals`
(/root/reference/ca_code/utils/geom.py:308-346) and `F.normalize` on the CPU, once in float32 and once with the same
vertices in float64, with backward against fixed seeded cotangents.  Build container only (imports ca_code through
tests/golden/ref_stubs.py).  Only numbers are stored.

Topology: tests/urhand_shaped.py:FakeGeo(64, 8) (81 vertices, 128 faces, a 64 x 64 map).  Geometry: a smooth dome of about
160 x 200 x 60 mm plus 1.5 mm of noise, B = 3 views (the tests take B = 1 as the first view: views are independent).
`values` has C = 4 channels (the tests take C = 1, 3 as the leading channels: channels are independent)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import npz_parts  # noqa: E402
import ref_stubs  # noqa: E402

ref_stubs.install()
from ca_code.utils.geom import values_to_uv, vert_normals  # noqa: E402
from urhand_shaped import FakeGeo  # noqa: E402

S, N, B, C = 64, 8, 3, 4


def dome(n):
    t = torch.linspace(-1.0, 1.0, n + 1, dtype=torch.float64)
    v, u = torch.meshgrid(t, t, indexing="ij")
    return torch.stack([80.0 * u, 100.0 * v, -60.0 * (1.0 - 0.5 * (u * u + v * v))], -1).reshape(-1, 3)


def run(dtype, geo, verts, values, cot):
    """The reference's lines in `dtype`: outputs and gradients as float64 numpy arrays of that precision's values."""
    vi = geo.vi.long()
    verts = verts.to(dtype).clone().requires_grad_(True)
    values = values.to(dtype).clone().requires_grad_(True)
    vn = vert_normals(verts, vi)
    (g_verts_vn,) = torch.autograd.grad((vn * cot["g_vn"].to(dtype)).sum(), verts, retain_graph=True)
    uv = values_to_uv(values, geo.index_image, geo.bary_image)
    (g_values,) = torch.autograd.grad((uv * cot["g_uv"].to(dtype)).sum(), values)
    postex = values_to_uv(verts, geo.index_image, geo.bary_image)
    tn_raw = values_to_uv(vn, geo.index_image, geo.bary_image)
    tn = F.normalize(tn_raw, dim=1)
    (g_verts_geo,) = torch.autograd.grad((postex * cot["g_postex"].to(dtype)).sum() + (tn * cot["g_tn"].to(dtype)).sum(),
                                         verts)
    out = dict(vn=vn, uv=uv, postex=postex, tn=tn, g_verts_vn=g_verts_vn, g_values=g_values, g_verts_geo=g_verts_geo)
    return {k: v.detach() for k, v in out.items()}, tn_raw.detach()


def main():
    geo = FakeGeo(S, N)
    V = (N + 1) ** 2
    g = torch.Generator().manual_seed(20240)
    # float32 values everywhere: both precisions see the same inputs
    verts = (dome(N)[None] + 1.5 * torch.randn(B, V, 3, generator=g, dtype=torch.float64)).float()
    values = torch.randn(B, V, C, generator=g)
    cot = {"g_vn": torch.randn(B, V, 3, generator=g), "g_uv": torch.randn(B, C, S, S, generator=g),
           "g_postex": torch.randn(B, 3, S, S, generator=g), "g_tn": torch.randn(B, 3, S, S, generator=g)}
    r32, _ = run(torch.float32, geo, verts, values, cot)
    r64, tn_raw = run(torch.float64, geo, verts, values, cot)
    mask = (geo.index_image != -1).all(-1)
    out = {"vi": geo.vi.numpy().astype(np.int32), "index_image": geo.index_image.numpy().astype(np.int32),
           "bary_image": geo.bary_image.numpy(), "verts": verts.numpy(), "values": values.numpy()}
    out.update({k: v.numpy() for k, v in cot.items()})
    out.update({f"ref32/{k}": v.numpy() for k, v in r32.items()})
    out.update({f"ref64/{k}": v.numpy() for k, v in r64.items()})
    print(f"V = {V}, F = {geo.vi.shape[0]}, covered = {float(mask.float().mean()):.3f}, smallest un-normalised texel normal "
          f"= {float(tn_raw.norm(dim=1)[:, mask].min()):.3f}")
    for k in r32:
        print(f"  {k:12s} max |fp64| = {float(r64[k].abs().max()):.3e}   fp32 - fp64 = "
              f"{float((r32[k].double() - r64[k]).abs().max()):.3e}")
    for name in npz_parts.save(os.path.join(HERE, "uvgeom_golden.npz"), out):
        print(name, os.path.getsize(name))


if __name__ == "__main__":
    main()
