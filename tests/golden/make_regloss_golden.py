"""Generate tests/golden/regloss_golden.npz with the REFERENCE's own regularisers (ca_code/loss/__init__.py:560-600,
609-622: pure PyTorch, run on the CPU; imported unchanged through ref_stubs) and autograd for the gradients.  Build
container only.

Per case the file holds the float32 inputs, the loss and the input gradient of the reference's function on the inputs cast
to float64 (`loss64`, `grad64`), and the same function on the float32 inputs (`loss32`, `grad32`): the float32-vs-float64
deviation of the reference itself is what tests/test_gpu_regloss.py scales its bound by.  Data only.

Inputs.  Every case starts from its kind's kinks (thresholds, the values next to them on either side, exact zeros, both
signs) followed by random values, shuffled; cases shorter than the kink list keep its head.  Cases of more than 2046
elements tile a palette of 509 values (kinks + random; 509 is prime, so a value meets every lane, float4 slot and chunk
offset) instead of drawing every element: the file stays a few hundred KB, and an element that lands in the wrong place
still shows, since its neighbours within +-508 all differ."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

PALETTE = 509
FULL = 2046          # up to here every element is drawn on its own

UNARY_SHAPES = {"n1": (1,), "n3": (3,), "n4": (4,), "n4095": (4095,), "n4097": (4097,), "n12293": (3 * 4096 + 5,),
                "real": (2, 341, 3)}
BACKLIT_SHAPES = {"one": (1, 1, 3), "rows1023": (2, 1023, 3), "rows1025": (2, 1025, 3), "c1": (2, 700, 1),
                  "c4": (1, 515, 4), "allpos": (1, 300, 3)}
MIN_SCALE, MAX_SCALE = 0.1, 20.0


def _f32(v):
    return np.float32(v)


def _around(v):
    v = _f32(v)
    return [np.nextafter(v, _f32(-np.inf)), v, np.nextafter(v, _f32(np.inf))]


def kinks(kind):
    if kind == "bound_primscale":   # head: one value per branch; then the thresholds, their neighbours, 0, negatives
        return [0.05, 25.0, 1.0, 0.0] + _around(MIN_SCALE) + _around(MAX_SCALE) + _around(1e-7) + [
            -0.5, -1e-9, 1e-8, 3e-5, 19.5, 0.09, 0.11, 400.0]
    if kind == "alphaprior":
        return [0.37, 0.0, 1.0, 0.8, 0.5, 1e-6, 1.0 - 1e-6, 0.05, 0.95]
    if kind == "l2_reg":
        return [1.3, -0.6, 0.0, 1e-4, -30.0]
    return [-0.7, 0.0, 0.4, -1e-3, 0.0, 1e-6, -1e-6, 2.5, -3.0, 0.0]   # negcolor, list_l1_reg: zeros and both signs


def draw(kind, n, g):
    if kind == "bound_primscale":   # log-uniform over [1e-3, 100], a tenth of them negative
        x = torch.exp(torch.empty(n).uniform_(float(np.log(1e-3)), float(np.log(100.0)), generator=g))
        return torch.where(torch.rand(n, generator=g) < 0.1, -x, x)
    if kind == "alphaprior":
        return torch.rand(n, generator=g)
    return torch.randn(n, generator=g)


def sequence(head, rand, n, g):
    """n values: the head of `head` if n is short, else head + random values, shuffled; tiled from a palette if n is large."""
    head = torch.tensor(np.array(head, dtype=np.float32))
    if n <= len(head):
        return head[:n].clone()
    m = n if n <= FULL else PALETTE
    v = torch.cat([head, rand(m - len(head))])
    v = v[torch.randperm(m, generator=g)]
    return v if m == n else v.repeat(-(-n // m))[:n].clone()


def both(fn, make_preds, x):
    """(loss64, grad64, loss32, grad32) of fn(make_preds(leaf)) for leaf = x in float64 and in float32."""
    out = []
    for dt in (torch.float64, torch.float32):
        leaf = x.detach().clone().to(dt).requires_grad_(True)
        loss = fn(make_preds(leaf))
        (grad,) = torch.autograd.grad(loss, leaf)
        out += [loss.detach().numpy(), grad.numpy()]
    return out


def main():
    ref_stubs.install()
    import types

    sys.modules.setdefault("sgutilslib", types.ModuleType("sgutilslib"))
    import ca_code.loss as L

    fns = {"bound_primscale": lambda p: L.loss_bound_primscale(p, min_scale=MIN_SCALE, max_scale=MAX_SCALE),
           "negcolor": L.loss_negcolor, "l2_reg": L.loss_l2_reg, "list_l1_reg": L.loss_list_l1_reg,
           "alphaprior": L.loss_alphaprior}
    keys = {"bound_primscale": "primscale_preclip", "negcolor": "diff_color", "l2_reg": "spec_dnml",
            "list_l1_reg": "spec_dnml", "alphaprior": "alpha"}
    out = {"bound_primscale/params": np.array([MIN_SCALE, MAX_SCALE], dtype=np.float64)}
    for ki, (kind, fn) in enumerate(fns.items()):
        for si, (tag, shape) in enumerate(UNARY_SHAPES.items()):
            g = torch.Generator().manual_seed(1000 * ki + si)
            n = int(np.prod(shape))
            x = sequence(kinks(kind), lambda k: draw(kind, k, g), n, g).reshape(shape)
            wrap = (lambda t: {keys[kind]: [t]}) if kind == "list_l1_reg" else (lambda t: {keys[kind]: t})
            l64, g64, l32, g32 = both(fn, wrap, x)
            pre = f"{kind}/{tag}/"
            out[pre + "x"], out[pre + "loss64"], out[pre + "grad64"] = x.numpy(), l64, g64
            out[pre + "loss32"], out[pre + "grad32"] = l32, g32
    # backlit: rows of (colour[C], cos weight); kink rows first: zeros and both signs in both, then random rows
    for si, (tag, shape) in enumerate(BACKLIT_SHAPES.items()):
        g = torch.Generator().manual_seed(7000 + si)
        C, M = shape[-1], int(np.prod(shape[:-1]))
        head_cw = [-0.6, 0.0, 0.5, -1e-3, -1.0, 0.9, -0.25, 0.0]
        head_col = [[0.5, -0.2, 0.0, 1.5], [0.3, 0.0, -0.1, 0.2], [0.7, 0.1, -0.4, 0.0], [0.0, 0.0, 0.0, 0.0],
                    [-1.0, -2.0, -0.5, -0.1], [1.0, 2.0, 3.0, 4.0], [0.0, 1e-6, -1e-6, 0.5], [0.2, -0.3, 0.4, 0.0]]
        m = M if M * C <= FULL else PALETTE
        k = min(m, len(head_cw))
        cw = torch.cat([torch.tensor(head_cw[:k]), torch.empty(m - k).uniform_(-1.0, 1.0, generator=g)])
        col = torch.cat([torch.tensor(head_col)[:k, :C], torch.randn(m - k, C, generator=g)])
        zero = torch.rand(m - k, C, generator=g) < 0.05
        col[k:][zero] = 0.0
        if m > len(head_cw):
            perm = torch.randperm(m, generator=g)
            cw, col = cw[perm], col[perm]
        if m != M:
            cw, col = cw.repeat(-(-M // m))[:M].clone(), col.repeat(-(-M // m), 1)[:M].clone()
        if tag == "allpos":             # no backlit row at all: the loss is 0 and the denominator exactly 1
            cw = cw.abs() + 0.01
        col, cw = col.reshape(shape), cw.reshape(*shape[:-1], 1)
        l64, g64, l32, g32 = both(L.loss_backlight_reg, lambda t: {"color_rand": t, "cos_weight": cw.to(t.dtype)}, col)
        pre = f"backlit_reg/{tag}/"
        out[pre + "color"], out[pre + "cos_weight"] = col.numpy(), cw.numpy()
        out[pre + "loss64"], out[pre + "grad64"], out[pre + "loss32"], out[pre + "grad32"] = l64, g64, l32, g32
    path = os.path.join(HERE, "regloss_golden.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
