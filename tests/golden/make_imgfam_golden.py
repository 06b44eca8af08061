"""Generate tests/golden/imgfam_golden.npz (in parts, tests/npz_parts.py) with the REFERENCE's own functions
(ca_code/loss/__init__.py:366-445, 496-538, 555-557, ca_code/utils/geom.py:768-794, ca_code/utils/image.py:393-422: pure
PyTorch, run on the CPU; imported unchanged through ref_stubs) and autograd for the gradients.  Build container only.
Data only.

Loss cases.  Per case the float32 inputs, the loss and the gradient w.r.t. the prediction of the reference's function on the
inputs cast to float64 (`loss64`, `grad64`) and of the same function on the float32 inputs (`loss32`, `grad32`).
  loss/<shape>/...          pred, target, mask1, maskc, veto for [B,C,HW] "images" (the kernel's cases), shared by
  loss/<shape>/<kind>/<mask>-<veto>/...  the three kinds (rgb_l1, rgb_l2, rgb_l1_focus) x mask none / [B,1,HW] / [B,C,HW]
                            x veto none / ~10 % set.  (rgb_l1_focus always reads a mask and a depth_disc_mask: "none" hands
                            it ones / all False, the same numbers.)
  pub/<case>/...            the public functions on [2,3,19,23] images, their arguments as in PUBLIC below.
Inputs hold the kinks: pred == target exactly, residuals of both signs next to 0, mask values 0, 1 and fractional, and
|residual| up to 255 (the focus weight reaches e).  Planes of more than 2046 elements tile a palette of 509 joint
(pred, target, mask, veto) entries, rolled by 37 per plane, as make_regloss_golden.py does.

Mask cases.  disc/<HxW>/depth [S,H,W] integer-valued scenes (tests/imgfam_cases.py) and disc/<HxW>/p<pool>t<i> the reference's
boolean output per pool size and threshold; disc/float/... the paraboloid blob; erode/<HxW>/x (float, values 0, 0.5, 1),
erode/<HxW>/f<ks> and b<ks> the reference's output for the float input and for its boolean twin (x == 1)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import imgfam_cases as cases  # noqa: E402
import npz_parts  # noqa: E402
import ref_stubs  # noqa: E402

FULL = 2046
PUB_SHAPE = (2, 3, 19, 23)
PUBLIC = {   # case -> (function, keyword arguments, what the dictionaries hold)
    "rgb_l2_erode3": ("rgb_l2", {"mask_erode": 3}, {"mask": True, "ddisc": "bool"}),
    "rgb_l2_nomask": ("rgb_l2", {}, {"mask": False, "ddisc": None}),
    "psnr": ("psnr", {"data_range": 255.0}, {"mask": True, "ddisc": "bool"}),
    "pose_shadow_l2": ("pose_shadow_l2", {}, {}),
}
for _fn in ("rgb_l1_focus", "rgb_l1_phys"):
    for _sm in (False, True):
        for _blur in (False, True):
            for _dd in ("bool", "float"):
                PUBLIC[f"{_fn}_sm{int(_sm)}_blur{int(_blur)}_{_dd}"] = (
                    _fn, {"self_mask": _sm, "img_blur": _blur, "mask_erode": 3 if _sm == _blur else None}, {"mask": True, "ddisc": _dd})


def palette(m, C, g):
    """m joint entries: pred[C], target[C], mask1, maskc[C], veto -- kinks first, then random, shuffled."""
    t = torch.rand(m, C, generator=g) * 255.0
    r = torch.randn(m, C, generator=g) * 20.0
    tiny = torch.tensor([0.0, 0.0, 1e-6, -1e-6, 1e-3, -1e-3, 255.0, -255.0, 254.5, -0.5, 0.5, 1.0, -1.0, 3e-5, -3e-5, 100.0])
    k = min(m, len(tiny))
    r[:k] = tiny[:k, None]
    big, small = r[:k].abs() >= 254.0, r[:k].abs() < 0.01
    t[:k] = torch.where(big, torch.where(r[:k] > 0, 0.0, 255.0), torch.where(small, 0.0, t[:k].round()))   # pred - target == r
    zero = torch.rand(m, C, generator=g) < 0.05
    zero[:k] = False
    p = t + r                                             # (float32: the residual p - t is whatever rounding left of r)
    p[zero] = t[zero]                                     # pred == target exactly
    u = torch.rand(m, 1 + C, generator=g)
    mk = torch.where(u < 0.25, torch.zeros_like(u), torch.where(u < 0.6, torch.ones_like(u), torch.rand(m, 1 + C, generator=g)))
    mk[:k] = 1.0                                          # the kinks stay visible ...
    mk[:k:5] = 0.5                                        # ... some through a fractional mask
    v = torch.rand(m, generator=g) < 0.1
    v[:k] = False
    perm = torch.randperm(m, generator=g)
    return p[perm], t[perm], mk[perm, :1], mk[perm, 1:], v[perm]


def loss_inputs(B, C, HW, g):
    m = HW if HW <= FULL else cases.PALETTE
    p, t, m1, mc, v = palette(m, C, g)
    out = {k: [] for k in ("pred", "target", "mask1", "maskc", "veto")}
    for b in range(B):
        rows = lambda a, s: torch.roll(a, s, 0).repeat(-(-HW // m), *([1] * (a.dim() - 1)))[:HW]
        out["pred"].append(torch.stack([rows(p[:, c], 37 * (b * C + c)) for c in range(C)]))
        out["target"].append(torch.stack([rows(t[:, c], 37 * (b * C + c)) for c in range(C)]))
        out["maskc"].append(torch.stack([rows(mc[:, c], 37 * (b * C + c)) for c in range(C)]))
        out["mask1"].append(rows(m1[:, 0], 37 * b * C)[None])
        out["veto"].append(rows(v, 37 * b * C)[None])
    return {k: torch.stack(v).contiguous() for k, v in out.items()}


def both(fn, pred):
    """(loss64, grad64, loss32, grad32) of fn(leaf, dtype) for leaf = pred in float64 and in float32."""
    out = []
    for dt in (torch.float64, torch.float32):
        leaf = pred.detach().clone().to(dt).requires_grad_(True)
        loss = fn(leaf, dt)
        (grad,) = torch.autograd.grad(loss, leaf)
        out += [loss.detach().numpy(), grad.numpy()]
    return out


def put(out, pre, res):
    out[pre + "loss64"], out[pre + "grad64"], out[pre + "loss32"], out[pre + "grad32"] = res


def kernel_cases(L, out):
    for si, (B, C) in enumerate(cases.BCS):
        for hi, HW in enumerate(cases.HWS):
            g = torch.Generator().manual_seed(100 * si + hi)
            x = loss_inputs(B, C, HW, g)
            tag = f"loss/{cases.shape_tag(B, C, HW)}/"
            for k, v in x.items():
                out[tag + k] = v.numpy()
            for kind in cases.KINDS:
                for mk in cases.MASKS:
                    for vk in cases.VETOS:
                        mask = {"none": None, "one": x["mask1"], "full": x["maskc"]}[mk]
                        veto = x["veto"] if vk == "veto" else None

                        def fn(leaf, dt):
                            m = None if mask is None else mask.to(dt)
                            if kind == "expw":      # always reads a mask and a depth_disc_mask
                                m = torch.ones(B, 1, HW, dtype=dt) if m is None else m
                                dd = torch.zeros(B, 1, HW, dtype=torch.bool) if veto is None else veto
                                return L.rgb_l1_focus({"rendered_rgb": leaf, "depth_disc_mask": dd},
                                                      {"image": x["target"].to(dt), "image_mask": m})
                            preds, targets = {"rendered_rgb": leaf}, {"image": x["target"].to(dt)}
                            if m is not None:
                                targets["image_mask"] = m
                            if veto is not None:
                                preds["depth_disc_mask"] = veto
                            return (L.rgb_l1 if kind == "abs" else L.rgb_l2)(preds, targets)

                        put(out, f"{tag}{kind}/{mk}-{vk}/", both(fn, x["pred"]))


def public_cases(L, out):
    B, C, H, W = PUB_SHAPE
    for ci, (case, (name, kw, has)) in enumerate(PUBLIC.items()):
        g = torch.Generator().manual_seed(5000 + ci)
        x = loss_inputs(B, C, H * W, g)
        img = lambda a: a.reshape(B, -1, H, W).contiguous()
        pred, target = img(x["pred"]), img(x["target"])
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        blob = (((yy - 9.3) / 8.0) ** 2 + ((xx - 11.6) / 10.0) ** 2 < 1.0).float()[None, None].repeat(B, 1, 1, 1)
        blob[:, :, 9, 11] = 0.0                                       # a hole for the erosion
        blob[1, :, :6] = 1.0                                          # and a part that touches the border
        frac = torch.where(torch.rand(B, 1, H, W, generator=g) < 0.1, img(x["mask1"]).clamp(min=0.25), torch.ones(B, 1, H, W))
        mask2 = torch.roll(blob, (2, -3), (2, 3)) * frac              # rendered_mask: fractional at a tenth of its pixels
        ddisc = img(x["veto"])
        ddisc = ddisc if has.get("ddisc") == "bool" else ddisc.float()
        pre = f"pub/{case}/"
        out[pre + "pred"], out[pre + "target"] = pred.numpy(), target.numpy()
        if name == "pose_shadow_l2":
            res = both(lambda leaf, dt: L.pose_to_shadow_l2_loss({"pose_shadow_map": leaf, "shadow_map": target.to(dt)}), pred)
        else:
            if has["mask"]:
                out[pre + "image_mask"], out[pre + "rendered_mask"] = blob.numpy(), mask2.numpy()
            if has["ddisc"]:
                out[pre + "depth_disc_mask"] = ddisc.numpy()

            def fn(leaf, dt):
                cast = lambda t: t if t.dtype == torch.bool else t.to(dt)
                preds = {"rendered_rgb": leaf, "rendered_rgb_blur": leaf, "rendered_phys_rgb": leaf}
                targets = {"image": target.to(dt)}
                if has["mask"]:
                    targets["image_mask"], preds["rendered_mask"] = blob.to(dt), mask2.to(dt)
                if has["ddisc"]:
                    preds["depth_disc_mask"] = cast(ddisc)
                return getattr(L, name)(preds, targets, **kw)

            res = both(fn, pred)
        put(out, pre, res)


def disc_scenes(H, W, g):
    hot, seam = cases.marks(H, W)
    s = []
    for pts in (hot, seam):
        a = np.zeros((H, W), np.float32)
        for y, x in pts:
            a[y, x] = 512.0
        s.append(a)
    a = np.zeros((H, W), np.float32)
    a[:H // 2 + 1, :W // 2 + 1] = 300.0                               # a plateau on the border: zero padding fires there
    a[H // 2 + 1:, W // 2 + 1:] = 7.0                                 # and one too low to fire
    s.append(a)
    s.append(torch.randint(0, 13, (H, W), generator=g).float().numpy())   # n = gx^2 + gy^2 scattered around 1600
    yy, xx = np.mgrid[0:H, 0:W]
    s.append((5.0 * np.minimum(xx, 100) + (yy % 4 == 0) * (xx % 4 == 0) + 2.0 * (yy % 4 == 2) * (xx % 4 == 2)).astype(np.float32))
    sparse = torch.randint(0, 513, (H, W), generator=g).float() * (torch.rand(H, W, generator=g) < 0.1)
    s.append(sparse.numpy())
    if (H, W) == cases.STEP_SIZE:                                     # straight steps of height 10: n = 1600 exactly
        for k in range(cases.TILE_W + 2):
            s.append((10.0 * (xx >= k)).astype(np.float32))
        for k in range(cases.TILE_H + 2):
            s.append((10.0 * (yy >= k)).astype(np.float32))
    return np.stack(s)


def erode_scenes(H, W, g):
    hot, seam = cases.marks(H, W)
    s = []
    for pts in (hot, seam):
        a = np.ones((H, W), np.float32)
        for i, (y, x) in enumerate(pts):
            a[y, x] = 0.5 if i % 3 == 2 else 0.0
        s.append(a)
    s.append(np.ones((H, W), np.float32))
    u = torch.rand(H, W, generator=g)
    s.append(torch.where(u < 0.01, torch.zeros(H, W), torch.where(u < 0.02, 0.5 * torch.ones(H, W), torch.ones(H, W))).numpy())
    a = np.ones((H, W), np.float32)
    a[H // 2, W // 2] = 0.5                                           # a single half: it vetoes its window
    s.append(a)
    return np.stack(s)


def float_scene():
    """A paraboloid blob on a zero background: the Sobel norm 8 |grad d| = 16 k r crosses 40 along the circle r = 10."""
    H, W = 3 * cases.TILE_H, cases.TILE_W + 16
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r2 = (yy - 23.3183) ** 2 + (xx - 41.7071) ** 2
    return np.maximum(0.0, 64.0 - 0.25 * r2).astype(np.float32)[None]


def mask_cases(geom, image, out):
    for si, (H, W) in enumerate(cases.SIZES):
        g = torch.Generator().manual_seed(9000 + si)
        tag = cases.size_tag(H, W)
        depth = disc_scenes(H, W, g)
        assert depth.min() >= 0 and depth.max() <= 512 and np.array_equal(depth, np.round(depth))
        out[f"disc/{tag}/depth"] = depth
        for pool in cases.POOLS:
            for ti, thr in enumerate(cases.THRESHOLDS):
                ref = geom.depth_discontuity_mask(torch.from_numpy(depth)[:, None], threshold=thr, pool_ksize=pool)
                out[f"disc/{tag}/p{pool}t{ti}"] = ref[:, 0].numpy()
        x = erode_scenes(H, W, g)
        out[f"erode/{tag}/x"] = x
        for ks in cases.ERODE_KS:
            out[f"erode/{tag}/f{ks}"] = image.erode(torch.from_numpy(x)[:, None], ks)[:, 0].numpy()
            out[f"erode/{tag}/b{ks}"] = image.erode(torch.from_numpy(x == 1.0)[:, None], ks)[:, 0].numpy()
    depth = float_scene()
    out["disc/float/depth"] = depth
    for pool in cases.POOLS:
        ref = geom.depth_discontuity_mask(torch.from_numpy(depth)[:, None], pool_ksize=pool)[:, 0].numpy()
        yes, no = cases.decide(depth, pool)
        flagged = ~(yes | no)
        assert ref[yes].all() and not ref[no].any(), "the reference's own float32 output disagrees on a decided pixel"
        assert flagged.mean() <= cases.FLAGGED_CAP, (pool, int(flagged.sum()))
        assert yes.any() and no.any()
        out[f"disc/float/p{pool}"] = ref
        print(f"float scene pool {pool}: {int(yes.sum())} true, {int(no.sum())} false, {int(flagged.sum())} flagged")


def main():
    ref_stubs.install()
    sys.modules.setdefault("sgutilslib", types.ModuleType("sgutilslib"))
    import ca_code.loss as L
    import ca_code.utils.geom as geom
    import ca_code.utils.image as image

    out = {}
    kernel_cases(L, out)
    public_cases(L, out)
    mask_cases(geom, image, out)
    written = npz_parts.save(os.path.join(HERE, "imgfam_golden.npz"), out)
    print(len(out), "arrays,", [(os.path.basename(p), os.path.getsize(p)) for p in written])


if __name__ == "__main__":
    main()
