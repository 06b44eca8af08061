"""Deterministic inputs for the edge-shape parity tests of the URHand relighting row (tests/test_urhand_cases.py guards
them on the CPU; tests/test_gpu_shadow.py and tests/test_gpu_uvlight.py feed them to gol_shadow_pcf and gol_uvlight_*),
and the float32 / float64 results of oracle/urhand_ref.py that the GPU tests are judged by.

Plain helper module: no fixtures, no GPU.  Every builder returns CPU float32 tensors; scenes and oracle results are
computed once per case and dtype and shared (callers must not modify them).
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

TIE_MARGIN = 0.05      # px: no centre-tap coordinate of a shadow case lies nearer than this to a rounding tie k + 0.5


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def rel(a, ref):
    """|a - ref| / |ref| in float64 (what tests/scenes.py:rel_l2 computes, without the parity ledger's bookkeeping)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


# ====================================================================================================== shadow PCF
# (tag: B, L, H, W, dh, dw, nml)    hole = the all-hole rectangle (y0, y1, x0, x1) of every depth image
SHADOW = {
    "native_BL": dict(B=2, L=3, H=19, W=23, dh=40, dw=56, nml=True, hole=(14, 28, 20, 38)),
    "native_BL_nonml": dict(B=2, L=3, H=19, W=23, dh=40, dw=56, nml=False, hole=(14, 28, 20, 38)),
    "tall": dict(B=3, L=1, H=16, W=16, dh=48, dw=20, nml=True, hole=(18, 30, 6, 14)),
}
SHADOW_TAGS = list(SHADOW) + ["dyadic_ties"]
_SCENE_OF = {"native_BL_nonml": "native_BL"}       # the same scene, evaluated without the normal map
OVERDRAW = 6                                        # candidate texels drawn per texel kept


def _rodrigues(w):
    """Rotation matrix of the axis-angle vector w (float64)."""
    th = float(w.norm())
    k = w / max(th, 1e-30)
    Kx = torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def tie_margin(ix, iy):
    """Distance of either unnormalised sample coordinate to the nearest k + 0.5 (where nearest-sampling switches texel)."""
    m = lambda c: ((c - torch.floor(c)) - 0.5).abs()
    return torch.minimum(m(ix), m(iy))


def _candidates(c, gen, n, focal):
    """n texel positions in camera 0's frame (float64 [n,3]), by inverse projection from chosen pixel coordinates: 40 %
    uniform over the map and a 6 px rim around it, 40 % in 3 px bands over the four borders, 14 % inside the all-hole
    rectangle, 6 % inside the map but BEHIND the camera (Z < 0)."""
    dh, dw = c["dh"], c["dw"]
    r = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    kind, side = r(), torch.randint(0, 4, (n,), generator=gen)
    u, v = -6 + (dw + 12) * r(), -6 + (dh + 12) * r()
    band = (kind >= 0.40) & (kind < 0.80)
    bu, bv = r(), r()
    u = torch.where(band & (side == 0), -1.0 + 3 * bu, u)           # u is the pixel coordinate f X / Z + c: the sampled
    u = torch.where(band & (side == 1), dw - 1.0 + 3 * bu, u)       # index is round(u - 1), so u - 1 spans (-2, 1) here
    v = torch.where(band & (side == 2), -1.0 + 3 * bv, v)
    v = torch.where(band & (side == 3), dh - 1.0 + 3 * bv, v)
    y0, y1, x0, x1 = c["hole"]
    inhole = (kind >= 0.80) & (kind < 0.94)
    u = torch.where(inhole, x0 + 2.5 + (x1 - x0 - 3) * bu, u)
    v = torch.where(inhole, y0 + 2.5 + (y1 - y0 - 3) * bv, v)
    behind = kind >= 0.94
    u = torch.where(behind, 3 + (dw - 6) * bu, u)
    v = torch.where(behind, 3 + (dh - 6) * bv, v)
    Z = (690 + 80 * r()) * torch.where(behind, -1.0, 1.0)
    return torch.stack([(u - dw / 2) * Z / focal, (v - dh / 2) * Z / focal, Z], 1)


@functools.lru_cache(maxsize=None)
def shadow_scene(tag):
    """dict(depth [B*L,dh,dw], Rt [B*L,3,4], postex [B,3,H,W], nml [B,3,H,W] or None, focal, B, L, accepted): CPU float32.
    The L cameras of a batch element are camera 0 turned by 4 mrad and moved by a few units, so they see one texel set a
    few pixels apart; `accepted` is the share of candidate texels that passed the tie-margin rule."""
    from oracle import urhand_ref

    if tag == "dyadic_ties":
        return _dyadic_scene()
    c = SHADOW[tag]
    B, L, H, W, dh, dw = (c[k] for k in ("B", "L", "H", "W", "dh", "dw"))
    gen, focal, HW = _gen(_SCENE_OF.get(tag, tag)), 1000.0, c["H"] * c["W"]
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    Rts, cands = [], []
    for b in range(B):
        R0, t0 = _rodrigues(0.4 * rn(3)), 15 * rn(3)
        pc = _candidates(c, gen, OVERDRAW * HW, focal)
        cands.append(((pc - t0) @ R0).float())                                  # R0^T (p_cam - t0), then float32
        for l in range(L):
            Rl = R0 if l == 0 else _rodrigues(0.004 * F.normalize(rn(3), dim=0)) @ R0
            tl = t0 if l == 0 else t0 + 2.5 * rn(3)
            Rts.append(torch.cat([Rl, tl[:, None]], 1))
    Rt = torch.stack(Rts).float()
    depth = 650 + 150 * torch.rand(B * L, dh, dw, generator=gen)
    depth[torch.rand(B * L, dh, dw, generator=gen) < 0.25] = 0.0
    y0, y1, x0, x1 = c["hole"]
    depth[:, y0:y1, x0:x1] = 0.0
    # tie rule, in float64 on the float32 values the kernel will be given: keep the first HW candidates of a batch element
    # that stay TIE_MARGIN away from every k + 0.5 in all of its L cameras
    cand = torch.stack(cands).permute(0, 2, 1)[:, :, None]                      # [B,3,1,N]
    ix, iy, _ = urhand_ref.shadow_pcf_taps(depth, Rt, cand.repeat_interleave(L, 0), focal)
    ok = (tie_margin(ix, iy).view(B, L, -1) >= TIE_MARGIN).all(1)                # [B,N]
    assert int(ok.sum(1).min()) >= HW, (tag, ok.sum(1))
    postex = torch.stack([cand[b, :, 0][:, ok[b]][:, :HW] for b in range(B)]).view(B, 3, H, W).contiguous()
    nml = F.normalize(torch.randn(B, 3, H, W, generator=gen), dim=1) if c["nml"] else None
    return dict(depth=depth, Rt=Rt, postex=postex, nml=nml, focal=focal, B=B, L=L, accepted=float(ok.float().mean()))


def _dyadic_scene():
    """Every coordinate exactly representable: focal 1024, Rt = [I | 0], texels (x, y, 1024) with x, y in {-10, -9.5, ...,
    9.5}, a 16 x 16 map.  The sampled coordinate is x + 7: half of them are exact ties k + 0.5, and the taps reach from
    index -4 to 17.  The map is a ramp (3 per row, 0.4375 per column, so that a tap one texel off changes the result) from
    1000: below Z = 1024 in its upper half; every fifth texel along the diagonals is a hole."""
    ax = torch.arange(-10.0, 10.0, 0.5)
    y, x = torch.meshgrid(ax, ax, indexing="ij")
    postex = torch.stack([x, y, torch.full_like(x, 1024.0)])[None].contiguous()          # [1,3,40,40]
    i, j = torch.meshgrid(torch.arange(16.0), torch.arange(16.0), indexing="ij")
    depth = 1000.0 + 3.0 * i + 0.4375 * j
    depth[(3 * i + j) % 5 == 0] = 0.0
    Rt = torch.cat([torch.eye(3), torch.zeros(3, 1)], 1)[None]
    return dict(depth=depth[None], Rt=Rt, postex=postex, nml=None, focal=1024.0, B=1, L=1, accepted=1.0)


def shadow_oracle_inputs(tag, dtype):
    """(depth, Rt, postex, nml) as oracle/urhand_ref.shadow_pcf takes them: texels and normals repeated per light."""
    s = shadow_scene(tag)
    rep = lambda t: None if t is None else t.repeat_interleave(s["L"], 0).to(dtype)
    return s["depth"].to(dtype), s["Rt"].to(dtype), rep(s["postex"]), rep(s["nml"])


@functools.lru_cache(maxsize=None)
def shadow_oracle(tag, dtype):
    """in_shadow [B*L,1,H,W] of a case by oracle/urhand_ref.shadow_pcf in `dtype`."""
    from oracle import urhand_ref

    with torch.no_grad():
        return urhand_ref.shadow_pcf(*shadow_oracle_inputs(tag, dtype), focal=shadow_scene(tag)["focal"])


@functools.lru_cache(maxsize=None)
def shadow_classes(tag):
    """Per (light camera, texel) [B*L, HW], all from the float64 evaluation of the oracle's own sample coordinates: the tie
    `margin`, camera-space `Z`, and boolean classes of the nine taps -- all_inside / all_outside the map, straddling the
    `left`, `right`, `top`, `bottom` border (a tap beyond that side and a tap inside), `all_holes` (taps inside, every one
    of them a hole: vsum == 0), `mixed` (holes and hits among the inside taps)."""
    from oracle import urhand_ref

    s = shadow_scene(tag)
    depth, Rt, postex, _ = shadow_oracle_inputs(tag, torch.float32)
    ix, iy, Z = urhand_ref.shadow_pcf_taps(depth, Rt, postex, s["focal"])
    BL, (dh, dw) = depth.shape[0], depth.shape[-2:]
    ix, iy, Z = ix.reshape(BL, -1), iy.reshape(BL, -1), Z.reshape(BL, -1)
    off = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)
    rx = torch.round(ix[..., None, None] + off[:, None]).expand(-1, -1, 3, 3).long()     # torch.round: half to even
    ry = torch.round(iy[..., None, None] + off[None, :]).expand(-1, -1, 3, 3).long()
    inside = (rx >= 0) & (rx < dw) & (ry >= 0) & (ry < dh)
    d = depth[torch.arange(BL)[:, None, None, None], ry.clamp(0, dh - 1), rx.clamp(0, dw - 1)]
    hit, hole = inside & (d > 0), inside & (d == 0)
    any_, all_ = (lambda m: m.flatten(2).any(2)), (lambda m: m.flatten(2).all(2))
    return dict(margin=tie_margin(ix, iy), Z=Z, ix=ix, iy=iy, all_inside=all_(inside), all_outside=~any_(inside),
                left=any_(rx < 0) & any_(inside), right=any_(rx >= dw) & any_(inside),
                top=any_(ry < 0) & any_(inside), bottom=any_(ry >= dh) & any_(inside),
                all_holes=any_(inside) & ~any_(hit), mixed=any_(hole) & any_(hit))


# =================================================================================================== UV light loops
# 17 x 31 = 527 texels: two blocks of 256 and a tail of 15; 9 x 29 = 261: one block and 5.  Roughness is lo + (hi - lo) u^k
# with u uniform and k = rough_skew (1 unless given)
UV = {
    "tail_unit": dict(B=3, L=4, H=17, W=31, normals="unit", rough=(0.3, 0.9), powers=(1, 16, 32), shadow=True),
    "tail_nosh": dict(B=3, L=4, H=17, W=31, normals="unit", rough=(0.3, 0.9), powers=(1, 16, 32), shadow=False),
    "nonunit": dict(B=3, L=4, H=17, W=31, normals="nonunit", rough=(0.3, 0.9), powers=(1, 16, 32), shadow=True),
    "highlight": dict(B=2, L=1, H=17, W=31, normals="highlight", rough=(0.3, 0.9), rough_skew=10, powers=(2, 5, 8, 64),
                      shadow=False),
    "p0": dict(B=2, L=3, H=9, W=29, normals="unit", rough=(0.3, 0.9), powers=(), shadow=True),
    "p1": dict(B=2, L=3, H=9, W=29, normals="unit", rough=(0.3, 0.9), powers=(2.5,), shadow=True),
    "lowrough": dict(B=3, L=4, H=17, W=31, normals="unit", rough=(0.05, 0.9), powers=(1, 16, 32), shadow=True),
    "dark": dict(B=2, L=3, H=9, W=29, normals="unit", rough=(0.3, 0.9), powers=(1, 16, 32), shadow=True, dark=True),
}
UV_TAGS = list(UV)
PHONG_KEYS = ("phong/diff", "phong/spec", "phong/g_p_uv", "phong/g_nml")
GGX_KEYS = ("ggx/feat", "ggx/rgb", "ggx/g_p_uv", "ggx/g_nml", "ggx/g_roughness", "ggx/g_tex")
HIGHLIGHT_JITTER = 0.02
HIGHLIGHT_ANGLES = (30.0, 124.0)    # degrees between the view and the light direction, per batch element (see uv_inputs)


@functools.lru_cache(maxsize=None)
def uv_inputs(tag):
    """CPU float32 dict: p_uv, nml [B,3,H,W]; cam_pos [B,3]; light_pos [B,L,3]; light_intensity [B,L,1]; roughness
    [B,1,H,W]; tex_mean [B,3,H,W]; shadow_map [B,L,1,H,W] or None; powers; the upstream weights w_diff, w_spec, w_feat,
    w_rgb of the two backward passes."""
    c = UV[tag]
    B, L, H, W, P = c["B"], c["L"], c["H"], c["W"], len(c["powers"])
    g = _gen(tag)
    rn, ru = (lambda *s: torch.randn(*s, generator=g)), (lambda *s: torch.rand(*s, generator=g))
    p_uv = 40 * rn(B, 3, H, W)
    cam = torch.tensor([20.0, 10.0, -800.0]) + 30 * rn(B, 3)
    lp = F.normalize(rn(B, L, 3), dim=-1) * 1100
    if c["normals"] == "highlight":
        # the one light of each batch element at a chosen angle from the camera, seen from the origin.  With the normal on
        # the half vector h and of length s: n . L = s cos(angle / 2) and reflection . L = s^2 (1 + cos) - cos, so the
        # small angle puts both above 1 for s > 1.  The GGX lobe exceeds 1 only where N . H clamps to 1 (s >= 1) and
        # N . V, N . L are small: specular = F / (4 pi a^2 nom1 nom2), which falls like roughness^-4.  Power 64 overflows
        # float32 in the oracle's backward (0 * inf = NaN) above 2^(128/63) = 4.09, so the lobe has to land in a band
        # only a factor 1.41 wide in roughness.  With roughness uniform on [0.3, 0.9] no angle holds specular > 1 at 10 %
        # of the pairs with under 1 % non-finite (scanned 120 .. 170 degrees: 4.2 % at best, or 11 % with 7 % non-finite).
        # Hence the second angle, at which roughness 0.3 peaks just under 4.09 (measured largest 4.8), and `rough_skew`:
        # roughness = 0.3 + 0.6 u^10 keeps to the case's bounds but is glossy for most texels, with a rough tail
        cdir = F.normalize(cam, dim=-1)
        side = F.normalize(torch.linalg.cross(cdir, rn(B, 3)), dim=-1)
        ang = torch.deg2rad(torch.tensor(HIGHLIGHT_ANGLES))[:, None]
        lp = (1100 * (torch.cos(ang) * cdir + torch.sin(ang) * side))[:, None]
    li = ru(B, L, 1) + 0.05
    if c.get("dark"):
        li = torch.zeros(B, L, 1)
    lo, hi = c["rough"]
    rough = lo + (hi - lo) * ru(B, 1, H, W) ** c.get("rough_skew", 1)
    tex = 255 * ru(B, 3, H, W)
    shm = ru(B, L, 1, H, W) if c["shadow"] else None
    nml = F.normalize(rn(B, 3, H, W), dim=1)
    if c["normals"] == "highlight":
        # half of the texels: the half vector between the view and the (single) light direction, jittered -- the
        # configuration at which reflection . light, n . light and the GGX lobe peak
        v = F.normalize(cam[..., None, None] - p_uv, dim=1)
        l = F.normalize(lp[:, 0][..., None, None] - p_uv, dim=1)
        h = F.normalize(F.normalize(v + l, dim=1) + HIGHLIGHT_JITTER * rn(B, 3, H, W), dim=1)
        nml = torch.where(ru(B, 1, H, W) < 0.5, h, nml)
    if c["normals"] != "unit":
        nml = nml * (0.6 + 0.9 * ru(B, 1, H, W))
    return dict(p_uv=p_uv, nml=nml, cam_pos=cam, light_pos=lp, light_intensity=li, roughness=rough, tex_mean=tex,
                shadow_map=shm, powers=c["powers"], w_diff=rn(B, 1, H, W), w_spec=rn(B, P, 1, H, W),
                w_feat=rn(B, 1 + P, H, W), w_rgb=rn(B, 3, H, W))


def run_uv(mod, inp, to):
    """Forward and backward of mod.phong_features and mod.ggx_features (mod: oracle.urhand_ref or goliath_amd.uvlight) on
    the inputs `inp` mapped through `to` (dtype / device); returns the ten tensors of PHONG_KEYS + GGX_KEYS."""
    t = {k: (to(v) if torch.is_tensor(v) else v) for k, v in inp.items()}
    leaf = {k: t[k].clone().requires_grad_(True) for k in ("p_uv", "nml", "roughness", "tex_mean")}
    fixed = (t["cam_pos"], t["light_pos"], t["light_intensity"])
    out = {}
    d, s = mod.phong_features(leaf["p_uv"], leaf["nml"], *fixed, t["shadow_map"], spec_powers=t["powers"])
    gp, gn = torch.autograd.grad((d * t["w_diff"]).sum() + (s * t["w_spec"]).sum(), (leaf["p_uv"], leaf["nml"]))
    out.update({"phong/diff": d, "phong/spec": s, "phong/g_p_uv": gp, "phong/g_nml": gn})
    f, rgb = mod.ggx_features(leaf["p_uv"], leaf["nml"], *fixed, leaf["roughness"], leaf["tex_mean"], t["shadow_map"],
                              spec_powers=t["powers"])
    gs = torch.autograd.grad((f * t["w_feat"]).sum() + (rgb * t["w_rgb"]).sum(), tuple(leaf.values()))
    out.update({"ggx/feat": f, "ggx/rgb": rgb})
    out.update(dict(zip(("ggx/g_p_uv", "ggx/g_nml", "ggx/g_roughness", "ggx/g_tex"), gs)))
    return {k: v.detach() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def uv_oracle(tag, dtype):
    """The ten tensors of a case by oracle/urhand_ref.py in `dtype`."""
    from oracle import urhand_ref

    return run_uv(urhand_ref, uv_inputs(tag), lambda v: v.to(dtype))


@functools.lru_cache(maxsize=None)
def e_ref64(tag):
    """{tensor: (rel-L2 of the float32 oracle from the float64 oracle over the elements where the float32 oracle is finite,
    share of elements where it is not)} -- torch yields NaN (0 * inf) where spec^31 overflows float32 behind clamp(max=1)."""
    o32, o64 = uv_oracle(tag, torch.float32), uv_oracle(tag, torch.float64)
    res = {}
    for k in PHONG_KEYS + GGX_KEYS:
        ok = torch.isfinite(o32[k])
        res[k] = (rel(o32[k][ok], o64[k][ok]), 1.0 - float(ok.double().mean()) if ok.numel() else 0.0)
    return res


@functools.lru_cache(maxsize=None)
def uv_intermediates(tag):
    """float64 [B,L,H,W]: n . L, reflection . L (the Phong clamps' arguments, oracle/urhand_ref.py:22-27), and V . n
    [B,1,H,W] (the sign GGX flips the normal by, :44)."""
    t = {k: v.double() for k, v in uv_inputs(tag).items() if torch.is_tensor(v)}
    v = F.normalize(t["cam_pos"][..., None, None] - t["p_uv"], dim=1)
    l = F.normalize(t["light_pos"][..., None, None] - t["p_uv"][:, None], dim=2)
    ref = -v - 2.0 * (-v * t["nml"]).sum(1, keepdim=True) * t["nml"]
    return dict(ndl=(t["nml"][:, None] * l).sum(2), rdl=(ref[:, None] * l).sum(2), vdn=(v * t["nml"]).sum(1, keepdim=True))


@functools.lru_cache(maxsize=None)
def ggx_specular(tag):
    """The GGX `specular` term [B,H,W] of a one-light case in float64, taken from the oracle itself: with tex_mean = 0 and
    L = 1, rgb = 4 pi * specular * I * max(n . L, 0) (oracle/urhand_ref.py:68-70).  NaN where n . L <= 0 (not lit)."""
    from oracle import urhand_ref

    t = {k: v.double() for k, v in uv_inputs(tag).items() if torch.is_tensor(v)}
    assert t["light_pos"].shape[1] == 1
    _, rgb = urhand_ref.ggx_features(t["p_uv"], t["nml"], t["cam_pos"], t["light_pos"], t["light_intensity"],
                                     t["roughness"], torch.zeros_like(t["tex_mean"]), None, spec_powers=UV[tag]["powers"])
    cos = uv_intermediates(tag)["ndl"][:, 0].clamp(min=0.0)
    spec = rgb[:, 0] / (4 * math.pi * t["light_intensity"][:, 0, 0, None, None] * cos)
    return torch.where(cos > 0, spec, torch.full_like(spec, float("nan")))
