"""Generate tests/golden/uvtex_golden.partNN.npz (tests/npz_parts.py) by running the REFERENCE's own code on the CPU, as unbound methods on a small
stand-in object that has `tex_std`, `cal` and `decoder_relight.refine_geo`:
    AutoEncoder.forward_tex      /root/reference/ca_code/models/urhand.py:711-748
    a real CalV5 (train() mode: the gradient hook applies)   ca_code/nn/color_cal.py:101-241
    SeamSampler.resample         ca_code/utils/seams.py:21-41
once in float32 and once, on the same float32 inputs, in float64.  Build container only (imports ca_code through
tests/golden/ref_stubs.py):  python tests/golden/make_uvtex_golden.py

Cases, seams and inputs: tests/uvtex_cases.py.  Per case the golden holds
    <case>/{tex, tex_mean, cal_params, uvs, weights, w_rec, w_before}     the float32 inputs (cams as strings)
    <case>/ref64/{before, tex_rec, g_tex, g_cal}    float64: forward_tex's output, the resampled texture, the gradients of
                                                   loss = <w_rec, tex_rec> + <w_before, before> w.r.t. relight_preds["tex"]
                                                   and the cal parameters ([cameras, 6])
    <case>/err32/<tensor>                           the reference's own float32-vs-float64 relative L2 error
    <case>/share_clamped                            share of pre-clamp values below 0 / above 255
Conditions (the case is reseeded until they hold): no pre-clamp float64 value lies within 1e-3 of 0 or 255, so the clamp's
gradient mask is never a tie and nothing has to be excluded from a comparison; more than 3 % of the pre-clamp values lie
below 0 and more than 3 % above 255."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import npz_parts  # noqa: E402
import ref_stubs  # noqa: E402

ref_stubs.install()
from ca_code.models.urhand import AutoEncoder  # noqa: E402
from ca_code.nn.color_cal import CalV5  # noqa: E402
from ca_code.utils.seams import SeamSampler  # noqa: E402
import uvtex_cases as cases  # noqa: E402


def run(dtype, name, inp):
    """The reference's lines in `dtype`: outputs, gradients and the pre-clamp values."""
    c = cases.CASES[name]
    B = c["B"]
    tex = inp["tex"].to(dtype).clone().requires_grad_(True)
    tex_mean = inp["tex_mean"].to(dtype)
    tex_mean = tex_mean.repeat(B, 1, 1, 1) if tex_mean.shape[0] == 1 else tex_mean.clone()   # urhand.py:765
    me = types.SimpleNamespace(tex_std=cases.TEX_STD, decoder_relight=types.SimpleNamespace(refine_geo=False))
    if c["cams"] is not None:
        cal = CalV5(cameras=cases.CAMERAS, identity_camera=cases.IDENTITY).to(dtype)
        with torch.no_grad():
            cal.holder.params.copy_(inp["cal_params"].to(dtype))
        cal.train()
        me.cal = cal
    sampler = SeamSampler(dict(dst_ij=torch.zeros(1, 2, dtype=torch.long), src_ij=torch.zeros(1, 2, dtype=torch.long),
                               uvs=inp["uvs"].to(dtype), weights=inp["weights"].to(dtype)))
    before, _ = AutoEncoder.forward_tex(me, {"tex": tex}, None, None, tex_mean, None, {"camera": c["cams"], "frame": None})
    tex_rec = SeamSampler.resample(sampler, before)
    loss = (tex_rec * inp["w_rec"].to(dtype)).sum() + (before * inp["w_before"].to(dtype)).sum()
    loss.backward()
    out = dict(before=before, tex_rec=tex_rec, g_tex=tex.grad)
    if c["cams"] is not None:
        out["g_cal"] = me.cal.holder.params.grad
    # the pre-clamp values, for the tie condition: the same lines without the clamp
    with torch.no_grad():
        t = tex.detach()
        ng = 1 if c["C"] == 2 else 3
        pre = tex_mean.clamp(0, 255) * t[:, :ng] + t[:, ng:] * cases.TEX_STD
        if c["cams"] is not None:
            me.cal.eval()
            pre = me.cal(pre, me.cal.name_to_idx(c["cams"]))
    return {k: v.detach() for k, v in out.items()}, pre


def main():
    out = {"cameras": np.array(cases.CAMERAS), "identity": np.array(cases.IDENTITY), "tex_std": np.array(cases.TEX_STD)}
    for i, name in enumerate(cases.CASES):
        seed = 100 * (i + 1)
        while True:
            inp = cases.make_inputs(name, seed)
            r64, pre = run(torch.float64, name, inp)
            share = ((pre < 0).double().mean().item(), (pre > 255).double().mean().item())
            no_tie = min((pre - 0.0).abs().min().item(), (pre - 255.0).abs().min().item()) >= 1e-3
            if no_tie and min(share) > 0.03:     # a visible share below 0 and above 255
                break
            seed += 1
        r32, _ = run(torch.float32, name, inp)
        out[f"{name}/seed"] = np.array(seed)
        out[f"{name}/cams"] = np.array(cases.CASES[name]["cams"] or [])
        out[f"{name}/share_clamped"] = np.array(share)
        for k, v in inp.items():
            out[f"{name}/{k}"] = v.numpy()
        for k, v in r64.items():
            out[f"{name}/ref64/{k}"] = v.numpy()
            out[f"{name}/err32/{k}"] = np.array(cases.rel_l2(r32[k].numpy(), v.numpy()))
        print(name, "seed", seed, "clamped below / above: %.3f / %.3f" % share,
              {k: "%.2e" % out[f"{name}/err32/{k}"] for k in r64})
    for path in npz_parts.save(os.path.join(HERE, "uvtex_golden.npz"), out):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
