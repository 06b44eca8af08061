"""TEST INFRASTRUCTURE: the topologies and inputs of the uvframes tests (goliath_amd/uvframes.py, csrc/uvframes.hip), as plain
tensors.  Shared by tests/golden/make_uvframes_golden.py (which runs the reference on them) and the tests (which run the
HIP operator on them): nothing here needs the reference.  Every map is 64 x 64, V <= 81, B <= 3.

General cases (the generator asserts that every clamped norm is at least 10 x its clamp on cases 1-4):
  dome      1  FakeGeo(64, 8) with the dome geometry of the uvgeom golden, B = 3
  coarse    2  FakeGeo(64, 2): about 400 texels per triple, every triple spans several 64-texel items
  full      3  one island over the whole map: rows and columns 0 and S-1 are covered (the stencil's zero padding)
  impaint   4  the empty texels of `dome` filled; on some of them vi[face_index_image] is not the index_image triple
  seam      5  some vertices whose v2uv[:, 0] uv is not the uv their faces use; one makes |fin| < 1e-8 with negative sign
Clamp cases (exact zeros in float32 and float64 alike, so both precisions take the same branch):
  clamp_a      mode A: the three vertices of face 40 coincide (t0 raw = 0), cam_pos equals the position of texel (30, 30).
               All coordinates are multiples of 1/4 below 128, so the cross products of the degenerate neighbour faces
               are exactly zero in any arithmetic, fused or not
  clamp_b      mode B: a position map whose normal is (0, 0, -1), face 40 stood up so that its t0 = (0, 0, 1) (n x t0 = 0),
               and an exactly zero 7 x 7 patch of the map (U x V = 0)
"""
import numpy as np
import torch

from urhand_shaped import FakeGeo

S = 64
CASES = ("dome", "coarse", "full", "impaint", "seam")
CLAMP_CASES = ("clamp_a", "clamp_b")
# (run name, mode B?, flip_normal, views): what the golden holds for a case
RUNS = {"dome": (("A0", False, False, 3), ("B1", True, True, 3), ("A1", False, True, 1), ("B0", True, False, 1)),
        "clamp_a": (("A0", False, False, 1),), "clamp_b": (("B1", True, True, 1),)}
DEFAULT_RUNS = (("A0", False, False, 1), ("B1", True, True, 1))
CLAMP_FACE, CLAMP_TEXEL, ZERO_PATCH = 40, (30, 30), (slice(40, 47), slice(20, 27))


class Geo:
    """The buffers of a GeometryModule that the frames read."""

    def __init__(self, src):
        for k in ("vi", "vt", "v2uv", "index_image", "face_index_image", "bary_image"):
            setattr(self, k, getattr(src, k).clone())
        self.uv_size = self.index_image.shape[0]

    def cuda(self):
        for k, v in list(self.__dict__.items()):
            if torch.is_tensor(v):
                setattr(self, k, v.cuda())
        return self


def _full_island(n=6):
    """FakeGeo's grid with the island over [0, 1]^2: every texel is covered."""
    geo = Geo(FakeGeo(S, n))
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    geo.vt = torch.from_numpy(np.stack([jj / n, ii / n], -1).reshape(-1, 2).astype(np.float32))
    vi = geo.vi.numpy()
    c = (np.arange(S) + 0.5) / S * n
    u, v = np.meshgrid(c, c)                      # u along columns, v along rows
    j, i = np.minimum(u.astype(np.int64), n - 1), np.minimum(v.astype(np.int64), n - 1)
    fu, fv = u - j, v - i
    low = fu + fv <= 1.0
    face = 2 * (i * n + j) + np.where(low, 0, 1)
    bary = np.where(low[..., None], np.stack([1 - fu - fv, fu, fv], -1), np.stack([fu + fv - 1, 1 - fu, 1 - fv], -1))
    geo.index_image = torch.from_numpy(vi[face])
    geo.face_index_image = torch.from_numpy(face)
    geo.bary_image = torch.from_numpy(bary.astype(np.float32))
    return geo


def _impainted():
    """`dome`'s images with every empty texel filled: texel (r, c) takes the triple of face (7 r + 3 c) % F and odd
    barycentrics; where r + c is a multiple of 3 its face_index_image names ANOTHER face."""
    geo = Geo(FakeGeo(S, 8))
    F = geo.vi.shape[0]
    empty = (geo.index_image == -1).all(-1)
    r, c = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    face = (7 * r + 3 * c) % F
    other = (face + 1 + (r % 5)) % F
    geo.index_image[empty] = geo.vi[face[empty]]
    geo.face_index_image[empty] = torch.where((r + c) % 3 == 0, other, face)[empty]
    geo.bary_image[empty] = torch.tensor([0.5, 0.3, 0.25])
    return geo


def _seam():
    """`dome` with three vertices whose first uv slot is a duplicate uv elsewhere.  Vertex 12 (row 1, column 3) is corner 2
    of face 6 = (3, 4, 12): its first-slot uv becomes uv(3) + (0.05, -4 ulp), so that vt02 = (0.05, -3e-8), vt01 = (0.1, 0)
    and fin = -3e-9."""
    geo = Geo(FakeGeo(S, 8))
    vt = geo.vt.numpy()
    y = np.float32(vt[3, 1])
    for _ in range(4):
        y = np.nextafter(y, np.float32(-1.0))
    extra = np.array([[vt[3, 0] + np.float32(0.05), y], [0.47, 0.52], [0.33, 0.71]], np.float32)
    geo.vt = torch.from_numpy(np.concatenate([vt, extra]))
    geo.v2uv = torch.cat([geo.v2uv, torch.full_like(geo.v2uv, -1)], 1)      # a second, empty slot
    for k, vert in enumerate((12, 40, 58)):
        geo.v2uv[vert, 1] = geo.v2uv[vert, 0]
        geo.v2uv[vert, 0] = vt.shape[0] + k
    return geo


def geometry(name):
    if name in ("dome", "clamp_a", "clamp_b"):
        return Geo(FakeGeo(S, 8))
    if name == "coarse":
        return Geo(FakeGeo(S, 2))
    return {"full": _full_island, "impaint": _impainted, "seam": _seam}[name]()


def n_views(name):
    return max(r[3] for r in RUNS.get(name, DEFAULT_RUNS))


def _dome(n):
    t = torch.linspace(-1.0, 1.0, n + 1, dtype=torch.float64)
    v, u = torch.meshgrid(t, t, indexing="ij")
    return torch.stack([80.0 * u, 100.0 * v, -60.0 * (1.0 - 0.5 * (u * u + v * v))], -1).reshape(-1, 3)


def _to_uv(geo, values):
    mask = (geo.index_image != -1).any(-1)
    out = (values[:, geo.index_image.clamp(min=0)] * geo.bary_image[None, ..., None]).sum(3)
    return (out * mask[None, ..., None]).permute(0, 3, 1, 2).contiguous()


def inputs(name):
    """float32 tensors: verts[B,V,3], posmap[B,3,S,S] (the vertices' map plus a smooth displacement; noise of a few mm on the
    uncovered texels, which the stencil reads), cam_pos[B,3] and the cotangents g_nml, g_viewout [B,3,S,S], g_frames
    [B,S,S,3,3].  Seeded numpy streams: the golden stores a checksum."""
    geo = geometry(name)
    B = n_views(name)
    rng = np.random.default_rng(20250 + (CASES + CLAMP_CASES).index(name))
    f32 = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    n = int(round(geo.v2uv.shape[0] ** 0.5)) - 1
    verts = (_dome(n)[None] + 1.5 * f32(B, (n + 1) ** 2, 3).double()).float()
    if name == "clamp_a":
        verts = torch.round(verts * 4.0) / 4.0
        a, b, c = geo.vi[CLAMP_FACE].tolist()
        verts[:, b] = verts[:, a]
        verts[:, c] = verts[:, a]
    mask = (geo.index_image != -1).any(-1)
    r, c = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    if name == "clamp_b":
        a, b, c3 = geo.vi[CLAMP_FACE].tolist()
        verts[:, b] = verts[:, a] + torch.tensor([0.0, 0.0, 7.0])
        posmap = torch.stack([1.5 * c, 2.0 * r, torch.zeros_like(r)])[None].repeat(B, 1, 1, 1)
        posmap[:, :, ZERO_PATCH[0], ZERO_PATCH[1]] = 0.0
    else:
        bump = torch.stack([0.8 * torch.sin(r / 5.0), 0.8 * torch.cos(c / 7.0), 1.2 * torch.sin((r + c) / 9.0)])
        posmap = _to_uv(geo, verts) + bump[None] * mask + 3.0 * f32(B, 3, S, S) * ~mask
    cam_pos = torch.tensor([[30.0, -40.0, 700.0]]).repeat(B, 1) + 20.0 * f32(B, 3)
    if name == "clamp_a":
        posmap = torch.round(posmap * 4.0) / 4.0
        cam_pos[0] = posmap[0, :, CLAMP_TEXEL[0], CLAMP_TEXEL[1]]
    out = dict(verts=verts, posmap=posmap.contiguous(), cam_pos=cam_pos, g_nml=f32(B, 3, S, S), g_viewout=f32(B, 3, S, S),
               g_frames=f32(B, S, S, 3, 3))
    return geo, out


def checksum(inp):
    return float(sum(float(v.double().sum()) * (i + 1) for i, v in enumerate(inp.values())))
