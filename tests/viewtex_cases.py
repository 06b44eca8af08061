"""Cases and the numpy float64 oracle of the camera-to-UV view textures (goliath_amd/viewtex.py, csrc/viewtex.hip), shared
by tests/test_viewtex_cpu.py (which pins this oracle to the reference's own geom.py), tests/test_gpu_viewtex.py and
tests/golden/make_viewtex_golden.py.

Oracle, from the stated semantics, in float64 on the float32 inputs:
  * face_vis[b, f] = face f occurs in view b's index image (indices outside [0, F) are ignored);
  * vis[b, texel] = face_index_uv != -1 and face_vis[b, face_index_uv];
  * xyz = sum_k verts[b, idx_k] bary_k; p = K (R xyz + t) with the full 3x3 K; pix = p.xy / p.z; the sample coordinate
    s = pix - 0.5 (what grid_sample's un-normalisation makes of 2 pix / size - 1) clamped to [0, size - 1] and rounded to
    nearest even; p.z == 0 or a non-finite pix gives 0;
  * tex = (index_image_uv[..., 0] != -1 ? rgb : 0) * vis, then * all_c(tex_c <= threshold) when a threshold is given.
Band of a case: texels that are covered and visible in some view whose clamped sample coordinate lies within 1e-3 px of a
rounding boundary (k + 0.5, i.e. pix within 1e-3 of an integer) on either axis in that view -- where fp32 and float64 may
fetch neighbouring pixels.  (A subset of "pix within 1e-3 of an integer in some view": a coordinate that the clamp pins
to the border, or a texel that shows nothing in that view, has no rounding choice to make.)  `alts` holds the texture
under the four forced choices (floor / ceil per axis); inside the band a texel may equal any of them, per view.

Topologies: uvtopo_cases "f" (S = 64, 128 faces, jittered) and "b" (S = 24) after the impaint.  B = 3 views, camera image
20 x 28 (H != W, W no multiple of 64), integer-valued float32 pixels in [0, 255].  View 0 shows every face, view 1's index
image is all -1, view 2 shows a strict subset; K has a skew term; the mesh overflows the image on all four sides; one
vertex of a face that view 2 shows lies behind view 2's camera.  check_fixture asserts all of that on the oracle.
"""
import collections
import functools

import numpy as np

import uvtopo_cases as U

BAND_PX = 1e-3
H, W, B = 20, 28, 3
THRESHOLD = 200.0
Case = collections.namedtuple("Case", ["name", "S", "F", "faces", "index_image_uv", "bary_image_uv", "face_index_uv", "verts",
                                       "image", "index_img", "K", "Rt", "behind"])
Oracle = collections.namedtuple("Oracle", ["tex", "mask", "face_vis", "band", "band_views", "alts", "pix", "cam_z"])


# ---- oracle -----------------------------------------------------------------------------------------------------------------
def face_visibility(index_img, F):
    out = np.zeros((index_img.shape[0], F), bool)
    for b, img in enumerate(index_img):
        ids = np.unique(img[(img >= 0) & (img < F)])
        out[b, ids] = True
    return out


def uv_visibility(face_vis, face_index_uv):
    F = face_vis.shape[1]
    ok = (face_index_uv >= 0) & (face_index_uv < F)
    return ok[None] & face_vis[:, np.clip(face_index_uv, 0, F - 1)]


def project(verts, index_image_uv, bary_image_uv, K, Rt):
    """-> pix[B,S,S,2] and p[B,S,S,3] (p.z = the depth of K p_cam), float64; uncovered texels use vertex 0."""
    nB = K.shape[0]
    v = np.broadcast_to(verts.astype(np.float64), (nB,) + verts.shape[1:])
    idx = np.clip(index_image_uv, 0, None)
    xyz = (v[:, idx] * bary_image_uv.astype(np.float64)[None, ..., None]).sum(-2)                   # [B,S,S,3]
    Rt, K = Rt.astype(np.float64), K.astype(np.float64)
    p_cam = np.einsum("bij,bhwj->bhwi", Rt[:, :3, :3], xyz) + Rt[:, None, None, :3, 3]
    p = np.einsum("bij,bhwj->bhwi", K, p_cam)
    with np.errstate(divide="ignore", invalid="ignore"):
        pix = p[..., :2] / p[..., 2:]
    return pix, p


def compute(verts, image, index_img, K, Rt, index_image_uv, bary_image_uv, face_index_uv, F, threshold=None):
    """The oracle on raw arrays -> Oracle."""
    nB, _, h, w = image.shape
    face_vis = face_visibility(index_img, F)
    vis = uv_visibility(face_vis, face_index_uv)                                                    # [B,S,S]
    covered = index_image_uv[..., 0] != -1
    pix, p = project(verts, index_image_uv, bary_image_uv, K, Rt)
    ok = (p[..., 2] != 0) & np.isfinite(pix).all(-1)
    size = np.array([w, h], np.float64)
    s = np.clip(np.where(ok[..., None], pix, 0.0) - 0.5, 0.0, size - 1.0)
    show = vis & covered[None] & ok

    def fetch(col, row):
        col, row = col.astype(np.int64), row.astype(np.int64)
        rgb = image[np.arange(nB)[:, None, None], :, row, col]                                      # [B,S,S,3]
        tex = np.where(show[..., None], rgb, np.float32(0)).transpose(0, 3, 1, 2)
        if threshold:
            tex = tex * (tex <= np.float32(threshold)).all(1, keepdims=True)
        return np.ascontiguousarray(tex.astype(np.float32))

    tex = fetch(np.rint(s[..., 0]), np.rint(s[..., 1]))
    lo, hi = np.floor(s), np.minimum(np.ceil(s), size - 1.0)
    alts = np.stack([fetch(cx[..., 0], cy[..., 1]) for cx in (lo, hi) for cy in (lo, hi)])
    frac = s - np.floor(s)
    band_views = show & (np.abs(frac - 0.5) < BAND_PX).any(-1)
    return Oracle(tex, vis[:, None], face_vis, band_views.any(0), band_views, alts, pix, p[..., 2])


def in_alts(got, o, where=None):
    """bool [B,S,S]: got[b, :, texel] equals one of the four rounding candidates of view b."""
    hit = (got[None] == o.alts).all(2).any(0)
    return hit if where is None else hit[:, where]


def sequential_sum(start, texs):
    """fp32 `start += tex` for every tex in order."""
    acc = np.array(start, np.float32, copy=True)
    for t in texs:
        acc = (acc + t.astype(np.float32)).astype(np.float32)
    return acc


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def _rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


def _topology(name):
    o = U.oracle(name)
    if name == "f":
        return o.index_image.copy(), o.bary32.copy(), o.face.copy()
    src = U.oracle_nearest(name, 100.0).src
    return U.impaint(o.index_image, src), U.impaint(o.bary32, src), U.impaint(o.face, src)


def _scene(name, topo, seed, broadcast):
    c = U.CASES[topo]
    rng = np.random.default_rng(seed)
    index_image_uv, bary_image_uv, face_index_uv = _topology(topo)
    faces = np.asarray(c.vi, np.int64)
    F, V = faces.shape[0], int(faces.max()) + 1
    # a mesh vertex sits where (one of) its uv vertices sits: a bumpy sheet that overflows the image on every side
    uv = np.zeros((V, 2))
    uv[faces.reshape(-1)] = np.asarray(c.vt, np.float64)[np.asarray(c.vti).reshape(-1)]
    base = np.stack([(uv[:, 0] - 0.5) * 2.6, (uv[:, 1] - 0.5) * 2.2, 0.3 * np.sin(3 * uv[:, 0]) * np.cos(2 * uv[:, 1])], -1)
    nV = 1 if broadcast else B
    verts = np.stack([base + 0.02 * b * rng.standard_normal(base.shape) for b in range(nV)]).astype(np.float32)
    K = np.stack([np.array([[40.0 + 3 * b, 1.5, 14.0 - b], [0, 38.0 - 2 * b, 10.0 + 0.5 * b], [0, 0, 1]]) for b in range(B)])
    Rt = np.stack([np.concatenate([_rot(-0.1 + 0.07 * b, 0.2 - 0.15 * b), [[0.05 * b], [-0.03], [3.0 + 0.2 * b]]], 1)
                   for b in range(B)])
    K, Rt = K.astype(np.float32), Rt.astype(np.float32)
    image = rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)
    # index images: view 0 runs of every face, random faces, holes; view 1 empty; view 2 a strict subset
    n = H * W
    v0 = np.concatenate([np.repeat(np.arange(F), 2), rng.integers(0, F, n)])[:n]
    v0[rng.random(n) < 0.1] = -1
    v0[3], v0[n - 1] = F - 1, 0
    subset = np.sort(rng.choice(F, max(2, (2 * F) // 5), replace=False))
    v2 = subset[rng.integers(0, len(subset), n)]
    v2[rng.random(n) < 0.3] = -1
    index_img = np.stack([v0, np.full(n, -1), v2]).reshape(B, H, W).astype(np.int64)
    # a vertex of a face view 2 shows, pushed far behind view 2's camera (camera z about -40: the face's zero crossing
    # of p.z is a sliver no texel falls into)
    shown = [f for f in subset if (face_index_uv == f).sum() >= 6]
    j = int(faces[shown[len(shown) // 2], 0])
    vb = verts.shape[0] - 1
    R2, t2 = Rt[2, :, :3].astype(np.float64), Rt[2, :, 3].astype(np.float64)
    cam = R2 @ verts[vb, j].astype(np.float64) + t2
    cam[2] = -40.0
    verts[vb, j] = (R2.T @ (cam - t2)).astype(np.float32)
    return Case(name, c.S, F, faces, index_image_uv, bary_image_uv, face_index_uv, verts, image, index_img, K, Rt, j)


@functools.lru_cache(maxsize=None)
def case(name):
    c = {"f": lambda: _scene("f", "f", 11, False), "f_bcast": lambda: _scene("f_bcast", "f", 12, True),
         "b": lambda: _scene("b", "b", 13, False)}[name]()
    for a in c:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


NAMES = ("f", "f_bcast", "b")


@functools.lru_cache(maxsize=None)
def oracle(name, threshold=None):
    c = case(name)
    o = compute(c.verts, c.image, c.index_img, c.K, c.Rt, c.index_image_uv, c.bary_image_uv, c.face_index_uv, c.F, threshold)
    for a in o:
        a.setflags(write=False)
    return o


def check_fixture(name):
    """What the fixtures claim to hold, asserted on the oracle alone.  Returns the band's share of the texels."""
    c, o, ot = case(name), oracle(name), oracle(name, THRESHOLD)
    assert c.image.shape == (B, 3, H, W) and H != W and W % 64 != 0
    assert c.verts.shape[0] == (1 if name.endswith("bcast") else B)
    show = (o.mask[:, 0] & (c.index_image_uv[..., 0] != -1)[None])
    px, py = o.pix[..., 0][show], o.pix[..., 1][show]
    assert (px < 0).any() and (px > W).any() and (py < 0).any() and (py > H).any()      # the clamp, all four sides
    assert (c.K[:, 0, 1] != 0).all()                                                     # skew
    assert (c.index_img[1] == -1).all() and not o.face_vis[1].any() and not o.mask[1].any()
    assert 0 < o.face_vis[2].sum() < o.face_vis[0].sum() and (o.face_vis[0] | ~o.face_vis[2]).all()   # a strict subset
    assert (c.index_img == c.F - 1).any() and (c.index_img == 0).any()
    assert o.face_vis[0, c.F - 1] and o.face_vis[0, 0]
    # a vertex behind view 2's camera on a face view 2 marks visible, and texels of that face that show something
    vb = c.verts.shape[0] - 1
    z = (c.Rt[2, 2, :3].astype(np.float64) @ c.verts[vb, c.behind].astype(np.float64)) + float(c.Rt[2, 2, 3])
    assert z < 0
    fs = [f for f in range(c.F) if c.behind in c.faces[f] and o.face_vis[2, f]]
    assert fs and any(((c.face_index_uv == f) & show[2]).any() for f in fs)
    assert (o.cam_z[2][show[2]] < 0).any()                                               # samples behind the camera are taken
    assert (c.image > THRESHOLD).any() and (c.image < THRESHOLD).any()
    cut = (o.tex != 0).any(1) & (ot.tex == 0).all(1)
    assert cut.any() and (ot.tex != 0).any() and (ot.tex <= THRESHOLD).all()
    if name == "b":   # impainted texels are exercised: texels the plain topology leaves empty show something
        assert (show.any(0) & ~U.oracle("b").valid).any()
    share = o.band.mean()
    assert share <= 0.01, share
    assert np.array_equal(o.band, ot.band)
    return share
