"""Generates tests/golden/featenc_golden.npz by running the REFERENCE's own weight-normalised layers
    proj = la.Conv2dWN(4, 16, 7, 1, 3, bias=False);  feat = la.Conv2dWN(16, 32, 4, 2, 1, bias=False)
    (ca_code/nn/layers.py:470), composed by the lines of FeatEncoderUNet.forward (ca_code/models/urhand.py:100-102):
    x = proj(x); x = feat(x)
on the CPU in float64, seed 0, input [2,4,12,20].  (The reference class itself hard-codes 64 / 192 / ... channels, about
10 M parameters: not a fixture.)  Parameters and the input are rounded to float32 before the float64 run, so they are
stored as float32; y and the four parameter gradients (under a seeded random upstream g_y) are stored as float64.
Numbers only.
Run in the build container (needs the reference tree):   python tests/golden/make_featenc_golden.py
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
import ca_code.nn.layers as la  # noqa: E402

torch.manual_seed(0)
proj = la.Conv2dWN(4, 16, 7, 1, 3, bias=False)
feat = la.Conv2dWN(16, 32, 4, 2, 1, bias=False)
with torch.no_grad():   # magnitudes away from the initial norm, so that weight_g matters
    proj.weight_g.mul_(torch.rand_like(proj.weight_g) + 0.5)
    feat.weight_g.mul_(torch.rand_like(feat.weight_g) + 0.5)
state = {"proj." + k: v.detach().clone() for k, v in proj.state_dict().items()}
state.update({"feat." + k: v.detach().clone() for k, v in feat.state_dict().items()})
assert sorted(state) == ["feat.weight_g", "feat.weight_v", "proj.weight_g", "proj.weight_v"]
assert all(v.dtype == torch.float32 for v in state.values())
x = torch.randn(2, 4, 12, 20)
g_y = torch.randn(2, 32, 6, 10)

proj, feat = proj.double(), feat.double()
h = proj(x.double())           # urhand.py:100
y = feat(h)                    # urhand.py:102, i = 0
(y * g_y.double()).sum().backward()

out = {"x": x.numpy(), "g_y": g_y.numpy(), "y": y.detach().numpy()}
out.update({k: v.numpy() for k, v in state.items()})
for name, mod in (("proj", proj), ("feat", feat)):
    for k, q in mod.named_parameters():
        out["grad.%s.%s" % (name, k)] = q.grad.numpy()
assert tuple(out["y"].shape) == (2, 32, 6, 10) and len(out) == 3 + 4 + 4
assert all(out[k].dtype == np.float64 for k in out if k == "y" or k.startswith("grad."))
path = os.path.join(HERE, "featenc_golden.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1000000
