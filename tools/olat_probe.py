"""olat probe: the MVP teacher's UNet input and OLAT sum on goliath_amd.olat against the torch lines of
goliath_amd.urhand.olat_rgb_decoder_forward_rgb, on one GPU.

Rows, each at the reference's size (S = 1024, 64 x 64 primitives of 16 x 16 x 8 voxels, B = 1) for L = 1 and the
reference's chunk of L = 5 lights:
    features             olat.features against the lines in float32 (tests/olat_cases.features_ref), no_grad
    combine fwd          olat.combine(want_texolat=True, use_shadow=False) against olat_cases.combine_ref, no_grad
    combine fwd+bwd      the same with a backward from cotangents of rgb and texolat ("g_texolat") or of rgb alone ("rgb only")
    forward_rgb train    olat_rgb_decoder_forward_rgb_fused against olat_rgb_decoder_forward_rgb, forward + backward in
                         train() mode on a two-level stand-in UNet (56 -> 16 -> 16 channels, 4 Z out), iteration = 5000.
                         The deep-shadow march is REPLAYED from a stored volume in both paths (it is the same code in both
                         and is not what this change touches), so the row is the work around the march, UNet included.
Each row reports GB/s on its algorithmic bytes (what one fused pass must move): features 28 Z S^2 B L written + 4 Z S^2 B L
read; the combine's from its tensors in the same way (see `combine_bytes`).

Method: both paths alternate in ONE process on the same inputs; --warmup untimed passes of each, then --boxes boxes of
--reps timed passes each (HIP events around a box, one synchronise per box); per row the median over the boxes and their
spread (max - min).  A row counts as faster only when the fused median is below the torch median by more than the torch
path's own spread; the others are named in `not_faster`.

    python tools/olat_probe.py [--boxes 7] [--reps 5] [--warmup 3] [--out profiles/olat_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
from torch import nn  # noqa: E402

import olat_cases as C  # noqa: E402
from goliath_amd import build, olat, urhand  # noqa: E402

S, PRIMSIZE, NP = 1024, (16, 16, 8), 64
X, Y, Z = PRIMSIZE
K = NP * NP
VOLRADIUS = 256.0


class ProbeDecoder(nn.Module):
    """Attribute layout of hand_teacher_mvp.OLATRGBDecoder at the reference's map size, with a two-level UNet."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.primsize, self.n_prim_x, self.n_prim_y, self.uv_size, self.volradius = PRIMSIZE, NP, NP, S, VOLRADIUS
        self.sizes = [S, S // 2]
        act = lambda: nn.LeakyReLU(0.2)
        self.enc_layers = nn.ModuleList([nn.Sequential(nn.Conv2d(7 * Z, 16, 3, padding=1), act()),
                                         nn.Sequential(nn.Conv2d(16, 16, 3, padding=1), act())])
        self.dec_layers = nn.ModuleList([nn.Sequential(nn.Conv2d(16 + 8, 16, 3, padding=1), act()),
                                         nn.Sequential(nn.Conv2d(32, 4 * Z, 3, padding=1))])


def make(L, B=1):
    g = torch.Generator().manual_seed(L)
    ii, jj = torch.meshgrid(torch.arange(float(NP)), torch.arange(float(NP)), indexing="ij")
    centres = torch.stack([(jj - NP / 2) * 3.0, (ii - NP / 2) * 3.0, 20.0 * torch.sin(0.1 * (ii + jj))], -1).reshape(1, K, 3)
    valid = (torch.rand(K, generator=g) > 0.1).float()
    d = dict(primpos=centres + 0.3 * torch.randn(B, K, 3, generator=g), primrot=C._rotations(B, K, g),
             primscale=(VOLRADIUS / 3.0) * (1.0 + 0.1 * torch.rand(B, K, 3, generator=g)), valid_prims=valid,
             light_pos=torch.tensor([150.0, 80.0, 560.0]) + 200.0 * torch.randn(B, L, 3, generator=g),
             campos=torch.tensor([[20.0, -30.0, 650.0]]).repeat(B, 1),
             primalpha=torch.zeros(1),                      # read by the march only, which the probe replays
             light_intensity=0.5 + torch.rand(B, L, 3, generator=g), joint_feat=torch.randn(B, 8, S // 2, S // 2, generator=g))
    d = {k: v.cuda() for k, v in d.items()}
    gg = torch.Generator(device="cuda").manual_seed(L)
    d["shadow"] = torch.rand(B * L, K, Z, Y, X, generator=gg, device="cuda")
    d["tex"] = torch.randn(B * L, 4 * Z, S, S, generator=gg, device="cuda") * 1.5
    d["tex"][:, [c for c in range(4 * Z) if c % 4]] -= 4.0          # colour channels around the relu's kink
    d["cot_rgb"] = torch.randn(B, Z, 3, S, S, generator=gg, device="cuda")
    d["cot_texolat"] = torch.randn(B, L, Z, 3, S, S, generator=gg, device="cuda")
    return d


def combine_bytes(B, L, backward, g_texolat):
    """Algorithmic bytes of one fused pass.  fwd: tex (4 channels) and shadow read, texolat, rgb and primshadow written.
    bwd: tex and g_rgb (and g_texolat) read, g_tex written."""
    vox = Z * S * S
    n = (16 + 4 + 12) * vox * B * L + 2 * 12 * vox * B
    if backward:
        n += (16 + 16 + (12 if g_texolat else 0)) * vox * B * L + 12 * vox * B
    return n


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def rows_for(L, dec):
    B = 1
    d = make(L, B)
    geom = [d[k] for k in C.GEOM_KEYS]
    tail = (PRIMSIZE, NP, NP)
    volume = d["shadow"].reshape(B, L, NP, NP, 1, Z, Y, X)
    urhand.deep_shadow = lambda *a, **k: volume            # both forward_rgb paths look it up in the module

    def features(fused):
        with torch.no_grad():
            if fused:
                return olat.features(*geom, d["shadow"], *tail, VOLRADIUS)
            return C.features_ref(*geom, d["shadow"], *tail, VOLRADIUS, dtype=torch.float32)

    def combine(fused, backward, g_texolat):
        tex = d["tex"].requires_grad_(backward)
        tex.grad = None
        with torch.set_grad_enabled(backward):
            if fused:
                rgb, texolat, ps = olat.combine(tex, d["light_intensity"], d["shadow"], *tail, False, True)
            else:
                rgb, texolat, ps = C.combine_ref(tex, d["light_intensity"], d["shadow"], *tail, False, dtype=torch.float32)
        if backward:
            outs, cots = ([rgb, texolat], [d["cot_rgb"], d["cot_texolat"]]) if g_texolat else ([rgb], [d["cot_rgb"]])
            torch.autograd.backward(outs, cots)
        return rgb

    def model(fused):
        fn = urhand.olat_rgb_decoder_forward_rgb_fused if fused else urhand.olat_rgb_decoder_forward_rgb
        dec.zero_grad(set_to_none=True)
        res = fn(dec, d["campos"], None, None, d["primpos"], d["primrot"], d["primscale"], d["primalpha"], d["valid_prims"],
                 d["joint_feat"], d["light_pos"], d["light_intensity"], iteration=5000)
        torch.autograd.backward([res["primrgb"], res["texolat"]], [d["cot_rgb"], d["cot_texolat"]])
        return res["primrgb"]

    feat_bytes = 32 * Z * S * S * B * L
    work = [("features", features, feat_bytes),
            ("combine fwd", lambda f: combine(f, False, False), combine_bytes(B, L, False, False)),
            ("combine fwd+bwd g_texolat", lambda f: combine(f, True, True), combine_bytes(B, L, True, True)),
            ("combine fwd+bwd rgb only", lambda f: combine(f, True, False), combine_bytes(B, L, True, False)),
            ("forward_rgb train fwd+bwd", model, None)]
    return d, work


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "olat_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("olat_probe needs a GPU: a timing taken elsewhere says nothing")
    dec = ProbeDecoder().cuda().train()
    rows, not_faster = [], []
    for L in (1, 5):
        d, work = rows_for(L, dec)
        for name, fn, nbytes in work:
            agree = float((fn(True).detach().double() - fn(False).detach().double()).norm()
                          / fn(False).detach().double().norm())     # the two paths compute the same thing
            for _ in range(args.warmup):
                for f in (False, True):
                    fn(f)
            torch.cuda.synchronize()
            ms = {False: [], True: []}
            for _ in range(args.boxes):                              # alternate the two paths box by box
                for f in (False, True):
                    ms[f].append(timed(lambda: fn(f), args.reps))
            row = dict(row=name, B=1, L=L, S=S, primsize=list(PRIMSIZE), fused_vs_torch_rel_l2=agree, algorithmic_bytes=nbytes)
            for f, tag in ((False, "torch"), (True, "fused")):
                med = statistics.median(ms[f])
                row[tag + "_ms_median"] = med
                row[tag + "_ms_spread"] = max(ms[f]) - min(ms[f])
                row[tag + "_ms_boxes"] = ms[f]
                if nbytes is not None:
                    row[tag + "_GBps"] = nbytes / (med * 1e-3) / 1e9
            row["speedup"] = row["torch_ms_median"] / row["fused_ms_median"]
            row["faster_beyond_spread"] = row["fused_ms_median"] < row["torch_ms_median"] - row["torch_ms_spread"]
            if not row["faster_beyond_spread"]:
                not_faster.append(f"L={L} {name}")
            rows.append(row)
            print(f"L={L} {name:28s} torch {row['torch_ms_median']:9.3f} ms (spread {row['torch_ms_spread']:.3f})  fused "
                  f"{row['fused_ms_median']:9.3f} ms (spread {row['fused_ms_spread']:.3f})  x{row['speedup']:.2f}  "
                  f"fused GB/s {row.get('fused_GBps', float('nan')):.0f}  agree {agree:.1e}", flush=True)
        del d, work
        torch.cuda.empty_cache()
    out = dict(tool="tools/olat_probe.py", device=torch.cuda.get_device_name(0), source_digest=build.source_digest(),
               method=f"HIP events, {args.warmup} warm-up passes, {args.boxes} boxes x {args.reps} passes, paths alternating",
               what="olat.features / olat.combine / olat_rgb_decoder_forward_rgb_fused against the torch lines of "
                    "olat_rgb_decoder_forward_rgb; forward_rgb rows replay a stored deep-shadow volume in both paths",
               rows=rows, not_faster=not_faster)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
