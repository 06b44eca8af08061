"""Generate tests/golden/viewtex_golden.npz with the REFERENCE's own compute_view_texture, compute_uv_visiblity_face and
compute_face_visibility (ca_code/utils/geom.py:834-910) in float32 on the CPU, on the scenes of tests/viewtex_cases.py.

Per case `{name}/...`: the inputs (verts, image, index_img, K, Rt, index_image_uv, bary_image_uv, face_index_uv, faces) and
the reference's outputs tex, mask (without a threshold), tex_thr (intensity_threshold = 200), face_vis and uv_vis.
The file holds inputs and recorded results only.  Run in the build container only (needs /root/reference):
    python tests/golden/make_viewtex_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import viewtex_cases as C  # noqa: E402

REF = "/root/reference"
INPUTS = ("verts", "image", "index_img", "K", "Rt", "index_image_uv", "bary_image_uv", "face_index_uv", "faces")


def reference_geom():
    from goliath_amd import dropin

    dropin.install_pytorch3d_shim()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import ca_code.utils.geom as geom

    return geom


def reference_outputs(geom, c, threshold=None, dtype=torch.float32):
    """(tex, mask) of the reference's compute_view_texture on case c's inputs, the floating ones cast to dtype."""
    t = lambda a: torch.from_numpy(np.array(a))   # noqa: E731
    f = lambda a: t(a).to(dtype)                  # noqa: E731
    verts = f(c.verts).expand(c.image.shape[0], -1, -1)
    return geom.compute_view_texture(verts, t(c.faces), f(c.image), t(c.index_img), None, f(c.K), f(c.Rt),
                                     t(c.index_image_uv), f(c.bary_image_uv), t(c.face_index_uv),
                                     intensity_threshold=threshold, normal_threshold=0.1)


def build():
    geom = reference_geom()
    out = {}
    for name in C.NAMES:
        c = C.case(name)
        for k in INPUTS:
            out[f"{name}/{k}"] = np.array(getattr(c, k))
        tex, mask = reference_outputs(geom, c)
        tex_thr, _ = reference_outputs(geom, c, C.THRESHOLD)
        assert tex.dtype == torch.float32 and mask.dtype == torch.bool
        out[f"{name}/tex"] = tex.numpy()
        out[f"{name}/mask"] = mask.numpy()
        out[f"{name}/tex_thr"] = tex_thr.numpy()
        t = lambda a: torch.from_numpy(np.array(a))   # noqa: E731
        out[f"{name}/face_vis"] = geom.compute_face_visibility(t(c.index_img), t(c.faces)).numpy()
        out[f"{name}/uv_vis"] = geom.compute_uv_visiblity_face(t(c.index_img), t(c.faces), t(c.face_index_uv)).numpy()
    return out


def main():
    out = build()
    path = os.path.join(HERE, "viewtex_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
