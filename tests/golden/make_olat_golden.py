"""Generates tests/golden/olat_golden.npz by running the REFERENCE's own
    ca_code.models.hand_teacher_mvp.OLATRGBDecoder.forward_rgb (hand_teacher_mvp.py:253-494)
in TRAIN mode on the CPU, as an unbound method on the seeded stand-in of tests/urhand_shaped.py, with the stubs of
make_urhand_model_golden.py: compute_raydirs and the with_shadow march through oracle/mvp_oracle.c, drtk.transform restated
in urhand_shaped.py.  Two cases at B = 2, L = 3: iteration = 0 (the shadow warm-up branch, :470-473) and iteration = 5000.
Per case <tag> in ("it0", "it5000"):
    <tag>_unet_input   the captured input of the first encoder layer [B L, 7 Z, S, S]
    <tag>_shadow       the deep-shadow volume [B, L, n_prim_y, n_prim_x, 1, Z, Y, X] as the march returned it
    <tag>_primrgb, _primshadow, _texolat
    <tag>_grad_joint_feat, _grad_enc0_weight, _grad_declast_weight: the gradients of
        loss = sum(primrgb * r1) + sum(texolat * r2),  r1, r2 = randn from torch.Generator().manual_seed(7), in that order
Only numbers go into the file.  Run where the reference tree is available:   python tests/golden/make_olat_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import ref_stubs  # noqa: E402

ref_stubs.install()
for n in ("sgutilslib", "utilslib", "mvpraymarchlib"):
    sys.modules.setdefault(n, types.ModuleType(n))
import ca_code.models.hand_teacher_mvp as T  # noqa: E402
import urhand_shaped as S  # noqa: E402
from oracle import cref  # noqa: E402

T.transform = S.drtk_transform
T.compute_raydirs = lambda vp, vr, f, pp, pc, vol: cref.compute_raydirs(vp, vr, f, pp, pc, vol)
torch.Tensor.cuda = lambda self, *a, **k: self      # forward_rgb calls .cuda() on three linspaces (hand_teacher_mvp.py:379-381)

B, L = 2, 3


class RecordingRaymarcher(S.OracleRaymarcher):
    def __call__(self, *args, **kwargs):
        res = super().__call__(*args, **kwargs)
        self.shadow = res[3].detach().clone()
        return res


out = {}
for tag, iteration in (("it0", 0), ("it5000", 5000)):
    dec = S.ShapedOLATRGBDecoder(RecordingRaymarcher(200.0), 200.0, seed=0).train()
    captured = {}
    dec.enc_layers[0].register_forward_pre_hook(lambda m, a: captured.__setitem__("x", a[0].detach().clone()))
    inp = S.teacher_inputs(B=B, L=L)
    joint_feat = inp["joint_feat"].clone().requires_grad_(True)
    res = T.OLATRGBDecoder.forward_rgb(dec, **{**inp, "joint_feat": joint_feat}, iteration=iteration)
    X, Y, Z = dec.primsize
    out[f"{tag}_unet_input"] = captured["x"].numpy()
    out[f"{tag}_shadow"] = dec.raymarcher.shadow.reshape(B, L, dec.n_prim_y, dec.n_prim_x, 1, Z, Y, X).numpy()
    for k in ("primrgb", "primshadow", "texolat"):
        out[f"{tag}_{k}"] = res[k].detach().numpy()
    g = torch.Generator().manual_seed(7)
    r1 = torch.randn(res["primrgb"].shape, generator=g)
    r2 = torch.randn(res["texolat"].shape, generator=g)
    ((res["primrgb"] * r1).sum() + (res["texolat"] * r2).sum()).backward()
    out[f"{tag}_grad_joint_feat"] = joint_feat.grad.numpy()
    out[f"{tag}_grad_enc0_weight"] = dec.enc_layers[0][0].weight.grad.numpy()
    out[f"{tag}_grad_declast_weight"] = dec.dec_layers[-1][0].weight.grad.numpy()
path = os.path.join(HERE, "olat_golden.npz")
np.savez_compressed(path, **out)
print("written", len(out), "arrays,", os.path.getsize(path), "bytes;",
      {k: tuple(v.shape) for k, v in out.items() if k.startswith("it0")})
