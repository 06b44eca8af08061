"""Generates tests/golden/dispunet_golden.partNN.npz by running the REFERENCE's own
    ca_code.models.urhand.DisplacementUNet   (urhand.py:109-242)
on the CPU in float64: uv_size=64, init_uv_size=2, output_scale=3.0, pose_feat_dim=4, n_enc_dims=[8]*6 (sizes
[2,4,8,16,32,64], 88,082 parameters), seed 0, B = 1.  Parameters and inputs are rounded to float32 before the float64 run, so
they are stored as float32; outputs and parameter gradients (under a seeded random upstream on disp and roughness) are
stored as float64.  Numbers only.  part00: inputs and the state dict; part01: outputs and gradients.
Run in the build container (needs the reference tree):   python tests/golden/make_dispunet_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import ref_stubs  # noqa: E402

ref_stubs.install()
import ca_code.models.urhand as U  # noqa: E402

CONFIG = dict(uv_size=64, init_uv_size=2, output_scale=3.0, pose_feat_dim=4, n_enc_dims=[8] * 6)

torch.manual_seed(0)
unet = U.DisplacementUNet(**CONFIG)
state = {k: v.detach().clone() for k, v in unet.state_dict().items()}
assert all(v.dtype == torch.float32 for v in state.values())
feat_uv = torch.randn(1, 6, 64, 64)
pose_cond = torch.randn(1, 4, 2, 2)
g_disp, g_rough = torch.randn(1, 1, 64, 64), torch.randn(1, 1, 64, 64)

unet = unet.double()
disp, rough, interm = unet(feat_uv.double(), pose_cond.double())
((disp * g_disp.double()).sum() + (rough * g_rough.double()).sum()).backward()
assert sum(q.numel() for q in unet.parameters()) == 88082 and list(unet.sizes) == [2, 4, 8, 16, 32, 64]

part0 = {"feat_uv": feat_uv.numpy(), "pose_cond": pose_cond.numpy(), "g_disp": g_disp.numpy(), "g_roughness": g_rough.numpy()}
part0.update({"state." + k: v.numpy() for k, v in state.items()})
part1 = {"disp": disp.detach().numpy(), "roughness": rough.detach().numpy(), "interm_feat": interm.detach().numpy()}
part1.update({"grad." + k: q.grad.numpy() for k, q in unet.named_parameters()})
assert all(v.dtype == np.float64 for v in part1.values())
for i, part in enumerate((part0, part1)):
    path = os.path.join(HERE, "dispunet_golden.part%02d.npz" % i)
    np.savez_compressed(path, **part)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000
print("tanh saturation: max |disp| / scale = %.3f, roughness in [%.3f, %.3f]"
      % (float(disp.abs().max()) / 3.0, float(rough.min()), float(rough.max())))
