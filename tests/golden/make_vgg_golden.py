"""Golden vectors of the masked VGG19 feature loss, made by the reference's OWN `VGGLossMasked.forward`
(ca_code/loss/vgg.py:52-88 of the reference tree, imported unchanged through ref_stubs) and autograd.  `Vgg19.__init__` asks
`torchvision.models.vgg.vgg19(pretrained=True)` for its network; torchvision is absent here and nothing may be
downloaded, so the existing torchvision stand-in of ref_stubs.py is given a `vgg19` that returns THIS generator's network:
the same 30-module `features` layout (conv, relu, ..., pool at 4, 9, 18, 27) at reduced widths, with seeded random
weights.  Build container only:  python tests/golden/make_vgg_golden.py  ->  tests/golden/vgg_golden.npz (~280 KB)."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

WIDTHS = (16, 16, 16, 16, 32)
GROUPS = (2, 2, 4, 4, 1)


def make_features(seed):
    torch.manual_seed(seed)
    mods, n_in = [], 3
    for gi, (width, count) in enumerate(zip(WIDTHS, GROUPS)):
        for _ in range(count):
            conv = nn.Conv2d(n_in, width, 3, padding=1)
            with torch.no_grad():
                conv.weight.normal_(0, (2.0 / (9 * n_in)) ** 0.5)
                conv.bias.normal_(0, 0.1)
            mods += [conv, nn.ReLU(inplace=False)]
            n_in = width
        if gi < 4:
            mods.append(nn.MaxPool2d(2, 2))
    assert len(mods) == 30
    return nn.Sequential(*mods)


def main():
    ref_stubs.install()
    features = make_features(7)
    sys.modules["torchvision.models.vgg"].vgg19 = lambda pretrained=True: types.SimpleNamespace(features=features)
    from ca_code.loss.vgg import VGGLossMasked

    torch.manual_seed(8)
    x = torch.rand(2, 3, 34, 45) * 330.0 - 40.0
    y = torch.rand(2, 3, 34, 45) * 330.0 - 40.0
    mask = torch.rand(2, 1, 34, 45)
    mask[:, :, :, :12] = 0.0
    out = {"widths": np.asarray(WIDTHS), "x": x.numpy(), "y": y.numpy(), "mask": mask.numpy()}
    for k, v in features.state_dict().items():
        out[f"features.{k}"] = v.numpy()
    module = VGGLossMasked()
    assert not any(p.requires_grad for p in module.parameters())
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        module = module.to(dtype)
        xs = x.to(dtype).requires_grad_(True)
        loss = module(xs, y.to(dtype), mask.to(dtype))
        g, = torch.autograd.grad(loss, xs)
        out[f"loss{tag}"], out[f"g_x{tag}"] = loss.detach().numpy(), g.numpy()
        factor = module(x.to(dtype), y.to(dtype), 0.5)        # a non-tensor mask is a plain factor
        out[f"loss_factor{tag}"] = factor.detach().numpy()
    path = os.path.join(HERE, "vgg_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; loss", float(out["loss64"]))


if __name__ == "__main__":
    main()
