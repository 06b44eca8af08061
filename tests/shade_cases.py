"""Edge scene of the shading tail (goliath_amd/csrc/shade.hip), its float32 / float64 torch oracles (oracle/shade_ref.py run
in both precisions on the same float32 inputs) and the partition of every (view, Gaussian) into conditioning classes.
Shared by tests/test_shade_cases.py (CPU: is the scene what it claims to be) and tests/test_gpu_shade_edges.py (GPU: HIP
against float64, per class).

The scene: B = 3 views of N = 1064 Gaussians (the GPU tests also run the first 1061: scalar planes, last lane three short)
with seeded draws on both sides of every branch of the kernel -- the softplus threshold and the [0.1, 20] primscale clamp,
the 0.01 sigma floor, every pair of mip levels and the top clamp, env texels below 0 and above 1, a negative light -- and
four constructed blocks of 64 rows whose normals are solved for per view (n ~ view - wanted reflection): `pole`, `seam`,
`aligned` (towards point light 0) and `zero_sh` (the 113 SH planes exactly 0).  The degenerate rows (exact poles, the exact
seam, zero quaternion, zero normal, position == campos, reflection exactly along a light) live in a scene of their own
(degenerate_scene) that is never handed to torch's autograd.  Everything is cached: callers must not write into it."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import shade_ref

B, N, N_ODD = 3, 1064, 1061
NCOL, NMONO = 16, 65
ND = 3 * NCOL + NMONO                     # 113 SH planes
PYRAMID = ((16, 32), (8, 16), (4, 8), (2, 4))
L = 6
N_LIGHTS = (6, 1, 0)
K = 64                                    # rows per constructed block
BLOCKS = dict(pole=(0, K), seam=(K, 2 * K), aligned=(2 * K, 3 * K), zero_sh=(3 * K, 4 * K), dark=(4 * K, 5 * K))
EPS32 = 2.0 ** -23
MIN_CLASS = 30
ENV_CLASSES = ("pole", "seam", "y_clamped", "x_clamped", "top_level", "over_one", "col_clamped", "interior")
SG_CLASSES = ("aligned", "no_light", "one_light", "sharp", "mid", "broad")
FALLBACK_CLASSES = ("sharp", "aligned")   # the only classes whose figures may be held to the oracle's EXPECTED error
ELEMENT_MASKS = ("scale_low", "scale_high", "scale_free", "sigma_floor", "sigma_free", "diff_neg", "diff_pos", "zero_sh")
# what each element mask governs (names of quantities(), below)
GOVERNS = dict(scale_low=("primscale", "g_scale"), scale_high=("primscale", "g_scale"), scale_free=("primscale", "g_scale"),
               sigma_floor=("sigma", "g_rough"), sigma_free=("sigma", "g_rough"),
               diff_neg=("color", "diff_color"), diff_pos=("color", "diff_color"), zero_sh=("g_sh", "color_rand", "diff_color"))
LEAVES = ("f_vnocond", "f_vcond", "postex", "tn", "albedo")
OUT_KEYS = ("color", "opacity", "primpos", "primqvec", "primscale", "primscale_preclip", "sigma", "spec_vis", "spec_nml",
            "spec_dnml", "diff_color", "spec_color", "primnmlbase", "color_rand")
GRAD_KEYS = ("g_sh", "g_pos", "g_quat", "g_scale", "g_opac", "g_rough", "g_vis", "g_dnml", "g_postex", "g_tn")


def unit(u, theta):
    """Direction with equirectangular u = atan2(x, z) / pi and polar angle theta from +y."""
    return torch.stack([torch.sin(theta) * torch.sin(math.pi * u), torch.cos(theta), torch.sin(theta) * torch.cos(math.pi * u)], -1)


@functools.lru_cache(maxsize=None)
def scene():
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    fv = 0.3 * r(B, ND + 12, N, 1)
    fv[:, ND + 7:ND + 10] = -6 + 32 * u(B, 3, N, 1)       # softplus: clamps low below -2.25, high above 20, threshold at 20
    fv[:, ND + 11] = -4 + 8 * u(B, N, 1)                  # sigma floor below -2.30; level 5 sigma over 0.05 .. 27
    fv[:, ND + 10] = 3 * r(B, N, 1)
    fc = 0.3 * r(B, 4, N, 1)
    fc[:, 0] = 3 * r(B, N, 1)
    postex = 60 * r(B, 3, N, 1)
    tn = F.normalize(r(B, 3, N, 1), dim=1)
    alb = 0.2 + 0.6 * u(1, N, 3)
    lsh, lrand = 0.3 * r(B, 3, NCOL + NMONO), 0.3 * r(B, 3, NCOL + NMONO)
    campos = torch.tensor([[30.0, -40.0, -900.0], [-500.0, 100.0, -700.0], [0.0, 0.0, -300.0]])
    mips = [u(B, 3, h, w) * 1.7 - 0.15 for h, w in PYRAMID]
    rot = torch.linalg.qr(r(B, 3, 3))[0].contiguous()
    li = u(B, L, 3)
    li[:, 3] = -li[:, 3]                                   # one negative light: the outer max(col, 0) clamps
    lp = F.normalize(r(B, L, 3), dim=-1) * 1100
    nl = torch.tensor(N_LIGHTS)

    def aim(rows, dirs_env=None, light=None):
        """tn / f_vcond[1:4] of `rows` such that, per view, lightrot x reflection = dirs_env, or the reflection points at
        point light `light` rotated away from it by dirs_env-free offsets (see the caller)."""
        pos = (fv[:, ND:ND + 3, :, 0] + postex[:, :, :, 0]).double()               # [B,3,N]
        view = F.normalize(pos - campos.double()[:, :, None], dim=1)
        for b in range(B):
            if light is None:
                want = rot[b].double().T @ dirs_env.double().T                     # [3,len]
            else:
                to = F.normalize(lp[b, light].double()[:, None] - pos[b][:, rows], dim=0)
                # rotate `to` by the wanted angle about a seeded axis perpendicular to it
                ax = F.normalize(torch.linalg.cross(to, dirs_env["axis"].double().T, dim=0), dim=0)
                a = dirs_env["angle"].double()[None]
                want = to * torch.cos(a) + ax * torch.sin(a)
            tn[b, :, rows, 0] = F.normalize(view[b][:, rows] - want, dim=0).float()
            fc[b, 1:4, rows, 0] = 0.0

    j = lambda n, amp: amp * (2 * u(n) - 1)                                        # seeded jitter: off the texel edges
    th = torch.linspace(2e-3, 0.98 * 2 * math.pi / 16, K // 2)
    th = th * (1 + j(K // 2, 0.01))
    th = torch.cat([th, math.pi - th])
    aim(torch.arange(*BLOCKS["pole"]), unit(torch.linspace(-0.97, 0.97, K) + j(K, 0.01), th))
    uu = 1 - torch.linspace(1e-3, 3 / 32, K // 2) * (1 + j(K // 2, 0.01))
    aim(torch.arange(*BLOCKS["seam"]), unit(torch.cat([uu, -uu]), torch.linspace(0.3, 2.8, K) + j(K, 0.01)))
    aim(torch.arange(*BLOCKS["aligned"]), dict(axis=r(K, 3), angle=torch.linspace(1e-4, 1e-2, K)), light=0)
    fv[:, :ND, BLOCKS["zero_sh"][0]:BLOCKS["zero_sh"][1]] = 0.0
    # `dark`: the random draws alone leave the outer max(col, 0) all but unclamped (a bilinear sample of texels that are
    # negative 9 % of the time is rarely negative).  These rows look, with the sharpest lobe (level 0.05), at the centres of
    # the most negative interior texels of each view's finest level, with a low albedo and a high visibility
    lo, hi = BLOCKS["dark"]
    h0, w0 = PYRAMID[0]
    for b in range(B):
        m = mips[0][b, :, 2:h0 - 2, 3:w0 - 3]
        score = torch.where(m.max(0).values < 0.95, m.min(0).values, torch.ones(()))   # not in `over_one`
        pick = score.flatten().argsort()[:K]
        yy, xx = 2 + pick // (w0 - 6), 3 + pick % (w0 - 6)
        dirs = unit((2 * xx + 1) / w0 - 1 + j(K, 0.04 / w0), ((2 * yy + 1) / h0 + j(K, 0.04 / h0)) * math.pi / 2)
        keep_tn, keep_fc = tn.clone(), fc.clone()
        aim(torch.arange(lo, hi), dirs)
        for o in range(B):                       # aim() writes every view: keep the other views' rows
            if o != b:
                tn[o, :, lo:hi], fc[o, 1:4, lo:hi] = keep_tn[o, :, lo:hi], keep_fc[o, 1:4, lo:hi]
    for b in range(B):
        fc[b, 1:4, lo:hi] = 0.0
    fv[:, ND + 11, lo:hi] = -4.0
    fc[:, 0, lo:hi] = 3.0
    alb[:, lo:hi] = 0.2
    return dict(f_vnocond=fv, f_vcond=fc, postex=postex, tn=tn, albedo=alb, light_sh=lsh, light_sh_rand=lrand, campos=campos,
                mips=mips, rot=rot, light_intensity=li, light_pos=lp, n_lights=nl)


@functools.lru_cache(maxsize=None)
def upstream():
    """Dense seeded upstream gradients of every differentiable output, [B,N,k] float32 (sigma: [B,N])."""
    g = torch.Generator().manual_seed(9)
    return {k: torch.randn(B, N, generator=g) if k == "sigma" else
            torch.randn(B, N, 4 if k == "primqvec" else 1 if k in ("opacity", "spec_vis") else 3, generator=g) for k in OUT_KEYS}


def _sg_eval(dirs, sig, lv, lp, pp, nl, w_type):
    """torch_ref.evaluate_gaussian with the gradient paths of the operation it restates: the reference's autograd node
    returns gradients for the lobe direction, the lobe width and the light values and None for the light and primitive
    positions (sgutils.py:63), so nothing flows into the position through the direction towards a light."""
    from oracle import torch_ref

    return torch_ref.evaluate_gaussian(dirs, sig, lv, lp.detach(), pp.detach(), nl, w_type)


def run_oracle(sc, dt, env, ups, coefs=None, rand=True, grad=True):
    """shade_ref.shade in dtype `dt` on the float32 scene `sc`, backward of sum(out[k] * ups[k]).  Returns (outputs, leaf
    gradients), detached."""
    leaf = {k: sc[k].to(dt).clone().requires_grad_(grad) for k in LEAVES}
    mips = [m.to(dt) for m in sc["mips"]] * (2 if len(sc["mips"]) == 1 else 1)   # one level: the oracle's selection needs
    kw = (dict(envmips=mips, lightrot=sc["rot"].to(dt)) if env else                # two; a lerp of a level with itself is exact
          dict(light_intensity=sc["light_intensity"].to(dt), light_pos=sc["light_pos"].to(dt), n_lights=sc["n_lights"],
               sg_eval=_sg_eval))
    if rand:
        kw["light_sh_rand"] = sc["light_sh_rand"].to(dt)
    out = shade_ref.shade(leaf["f_vnocond"], leaf["f_vcond"], leaf["postex"], leaf["tn"], leaf["albedo"], sc["light_sh"].to(dt),
                          sc["campos"].to(dt), coefs=coefs, **kw)
    if grad:
        sum((out[k] * ups[k].to(dt)).sum() for k in out if k in ups and out[k].requires_grad).backward()
    return ({k: v.detach() for k, v in out.items()},
            {k: torch.zeros_like(v) if v.grad is None else v.grad for k, v in leaf.items()} if grad else None)


def quantities(out, grads, nd=ND):
    """name -> [B,n,k]: the outputs, and the leaf gradients cut into the pieces the classes govern (g_albedo: [1,n,3])."""
    q = {k: (v[..., None] if v.dim() == 2 else v) for k, v in out.items()}
    if grads is not None:
        gv = grads["f_vnocond"].flatten(2).permute(0, 2, 1)
        gc = grads["f_vcond"].flatten(2).permute(0, 2, 1)
        q.update(g_sh=gv[..., :nd], g_pos=gv[..., nd:nd + 3], g_quat=gv[..., nd + 3:nd + 7], g_scale=gv[..., nd + 7:nd + 10],
                 g_opac=gv[..., nd + 10:nd + 11], g_rough=gv[..., nd + 11:nd + 12], g_vis=gc[..., :1], g_dnml=gc[..., 1:],
                 g_postex=grads["postex"].flatten(2).permute(0, 2, 1), g_tn=grads["tn"].flatten(2).permute(0, 2, 1),
                 g_albedo=grads["albedo"].reshape(1, -1, 3))
    return q


def lookup(sc, o64, pyramid=PYRAMID):
    """float64 quantities of the env lookup: uv [B,N,2], polar angle, level, the pixel coordinates (ix, iy) of the two levels
    used, the unclamped env value (recovered from spec_color only where needed by the caller)."""
    view = F.normalize(o64["primpos"] - sc["campos"].double()[:, None], dim=-1)
    n = o64["spec_nml"]
    ref = view - 2 * (view * n).sum(-1, keepdim=True) * n
    rr = torch.einsum("bxy,bny->bnx", sc["rot"].double(), ref)
    u = torch.atan2(rr[..., 0], rr[..., 2]) / math.pi
    theta = torch.atan2((rr[..., 0] ** 2 + rr[..., 2] ** 2).sqrt(), rr[..., 1])
    v = 2 * theta / math.pi - 1
    q = len(pyramid)
    level = 5 * o64["sigma"]
    lam = level.clamp(0, q - 1 - 1e-6) if q > 1 else torch.zeros_like(level)
    d1 = lam.floor().long()
    d2 = (d1 + 1).clamp(max=q - 1)
    hs, ws = torch.tensor([p[0] for p in pyramid]).double(), torch.tensor([p[1] for p in pyramid]).double()
    pix = lambda d, c, sizes: ((c + 1) * sizes[d] - 1) / 2
    return dict(ref=ref, u=u, v=v, theta=theta, level=level, q=q,
                ix=(pix(d1, u, ws), pix(d2, u, ws)), iy=(pix(d1, v, hs), pix(d2, v, hs)), w=(ws[d1], ws[d2]), h=(hs[d1], hs[d2]))


def env_value(sc, lk, mips=None):
    """The unclamped float64 env sample [B,N,3] at the float64 lookup coordinates."""
    mips = [m.double() for m in (mips or sc["mips"])]
    if len(mips) == 1:
        mips = mips * 2
    return shade_ref.mip_sample(mips, torch.stack([lk["u"], lk["v"]], -1), lk["level"])


def _near_int(x, tol):
    return (x - x.round()).abs() < tol


def near_branch(sc, o64, env, lk=None, zero_rows=None, pyramid=PYRAMID):
    """[B,N] bool: float32 and float64 may legitimately take different branches here (float64 quantities only)."""
    fv = sc["f_vnocond"].double().flatten(2).permute(0, 2, 1)
    nd = fv.shape[-1] - 12
    n = fv.shape[1]
    near = torch.zeros(fv.shape[0], n, dtype=torch.bool)
    rel = lambda x, t: (x - t).abs() < 1e-5 * abs(t)
    sp = o64["primscale_preclip"]
    near |= (rel(sp, 0.1) | rel(sp, 20.0) | rel(fv[..., nd + 7:nd + 10], 20.0)).any(-1)
    near |= rel(0.1 * torch.exp(fv[..., nd + 11]), 0.01)
    # diff and the random-light sum against the magnitude of their terms; the zero_sh rows' ties are exact in both precisions
    ncoef = sc["light_sh"].shape[-1]
    ncol = (nd - ncoef) // 2
    sh = torch.cat([fv[..., :3 * ncol].reshape(fv.shape[0], n, 3, ncol),
                    fv[..., 3 * ncol:nd].reshape(fv.shape[0], n, 1, nd - 3 * ncol).expand(-1, -1, 3, -1)], -1)
    tie = torch.zeros_like(near)
    for light in (sc["light_sh"], sc["light_sh_rand"]):
        terms = sh * light.double()[:, None]
        tie |= (terms.sum(-1).abs() < 1e-5 * terms.abs().sum(-1)).any(-1)
    if zero_rows is not None:
        tie[:, zero_rows[0]:zero_rows[1]] = False
    near |= tie
    spec = o64["spec_color"]
    dpos = o64["diff_color"].clamp(min=0)
    near |= ((dpos + spec).abs() < 1e-5 * (dpos + spec.abs())).any(-1) & (spec != 0).any(-1)
    if env:
        for k in (0, 1):
            for pix, size in ((lk["ix"][k], lk["w"][k]), (lk["iy"][k], lk["h"][k])):
                near |= _near_int(pix, 1e-4) & (pix > -0.5) & (pix < size - 0.5)
        near |= lk["u"].abs() > 1 - 1e-5
        near |= _near_int(lk["level"], 1e-5) & (lk["level"] < lk["q"] - 1 + 1e-3)
        near |= ((env_value(sc, lk) - 1).abs() < 1e-5).any(-1)
    else:
        # the +-1 clamp of the lobe's cosine: within float32 rounding of it the float32 cosine IS 1 and acos' = -inf
        # (of every light, the ones past n_lights included: the oracle evaluates them all and multiplies by a mask)
        near |= (light_cosines(sc, o64, lk, active_only=False).abs() > 1 - 1e-7).any(-1)
    return near


def light_cosines(sc, o64, lk, active_only=True):
    """[B,N,L] float64 cosine between the reflection and each light; active_only: 0 for the lights past n_lights."""
    ld = F.normalize(sc["light_pos"].double()[:, None] - o64["primpos"][:, :, None], dim=-1)
    c = (ld * F.normalize(lk["ref"], dim=-1)[:, :, None]).sum(-1)
    active = torch.arange(c.shape[-1])[None, None] < sc["n_lights"][:, None, None]
    return c * active if active_only else c


def _partition(names, cond):
    taken, out = None, {}
    for name in names:
        m = cond[name] if taken is None else cond[name] & ~taken
        out[name] = m
        taken = m if taken is None else taken | m
    return out


def classify(sc, o64, env, lk):
    """name -> [B,N] bool partition (the first class whose condition holds), float64 quantities only."""
    sig = o64["sigma"]
    if env:
        clamped = lambda pix, size: (pix <= 0) | (pix >= size - 1)
        ev = env_value(sc, lk)
        col = o64["diff_color"].clamp(min=0) + ev.clamp(max=1) * o64["spec_vis"]
        cond = dict(pole=(lk["theta"] < 2 * math.pi / 16) | (lk["theta"] > math.pi - 2 * math.pi / 16),
                    seam=lk["u"].abs() > 1 - 3 / 32,
                    y_clamped=clamped(lk["iy"][0], lk["h"][0]) | clamped(lk["iy"][1], lk["h"][1]),
                    x_clamped=clamped(lk["ix"][0], lk["w"][0]) | clamped(lk["ix"][1], lk["w"][1]),
                    top_level=lk["level"] >= lk["q"] - 1, over_one=(ev > 1).any(-1), col_clamped=(col < 0).any(-1),
                    interior=torch.ones_like(sig, dtype=torch.bool))
        return _partition(ENV_CLASSES, cond)
    nl = sc["n_lights"][:, None].expand_as(sig)
    c = light_cosines(sc, o64, lk)
    cond = dict(aligned=(c > math.cos(1.5e-2)).any(-1), no_light=nl == 0, one_light=nl == 1, sharp=sig < 0.03,
                mid=sig < 0.5, broad=torch.ones_like(sig, dtype=torch.bool))
    return _partition(SG_CLASSES, cond)


def element_masks(sc, o64):
    """Element masks for the outputs they govern: [B,N,3] for the scale / diff ones, [B,N,1] otherwise."""
    sp, d = o64["primscale_preclip"], o64["diff_color"]
    floor = (0.1 * torch.exp(sc["f_vnocond"].double()[:, ND + 11].flatten(1)) < 0.01)[..., None]
    zero = torch.zeros(B, N, 1, dtype=torch.bool)
    zero[:, BLOCKS["zero_sh"][0]:BLOCKS["zero_sh"][1]] = True
    return dict(scale_low=sp < 0.1, scale_high=sp > 20.0, scale_free=(sp >= 0.1) & (sp <= 20.0), sigma_floor=floor,
                sigma_free=~floor, diff_neg=d < 0, diff_pos=d > 0, zero_sh=zero)


def class_rel_l2(got, want, mask):
    """rel-L2 of `got` against the float64 `want` over `mask`: [B,n] (whole rows) or of the tensors' own shape."""
    if mask.dim() == want.dim() and mask.shape[-1] != want.shape[-1]:
        mask = mask.expand_as(want)
    d = (got.double() - want)[mask]
    return float(d.norm() / want[mask].norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def reference(env):
    """Everything the CPU side knows about one mode (env map / point lights), computed once and shared (read-only)."""
    sc, ups = scene(), upstream()
    o64, g64 = run_oracle(sc, torch.float64, env, ups)
    o32, g32 = run_oracle(sc, torch.float32, env, ups)
    lk = lookup(sc, o64)
    near = near_branch(sc, o64, env, lk, zero_rows=BLOCKS["zero_sh"])
    return dict(scene=sc, ups=ups, o64=o64, g64=g64, o32=o32, g32=g32, q64=quantities(o64, g64), q32=quantities(o32, g32),
                lookup=lk, near=near, keep=~near, classes=classify(sc, o64, env, lk), elements=element_masks(sc, o64))


def judged(ref, n=N):
    """[(class name, mask, quantity names)] of one mode for the first n Gaussians: the mode's partition on every quantity, the
    element masks on what they govern; near-branch members left out; classes of fewer than MIN_CLASS members dropped."""
    keep = ref["keep"][:, :n]
    items = [(c, m[:, :n] & keep, OUT_KEYS + GRAD_KEYS) for c, m in ref["classes"].items()]
    items += [(c, m[:, :n] & keep[..., None], GOVERNS[c]) for c, m in ref["elements"].items()]
    return [(c, m, qs) for c, m, qs in items if int(m.sum()) >= MIN_CLASS]


@functools.lru_cache(maxsize=None)
def small_scene(n, coefs=(NCOL, NMONO), pyramid=PYRAMID, seed=0):
    """B = 2 views of n Gaussians with the scene's seeded draws and no constructed block, any SH layout and pyramid."""
    ncol, nmono = coefs
    nd, Bs = 3 * ncol + nmono, 2
    g = torch.Generator().manual_seed(100 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    fv = 0.3 * r(Bs, nd + 12, n, 1)
    fv[:, nd + 7:nd + 10] = -6 + 32 * u(Bs, 3, n, 1)
    fv[:, nd + 11] = -4 + 8 * u(Bs, n, 1)
    fc = 0.3 * r(Bs, 4, n, 1)
    fc[:, 0] = 3 * r(Bs, n, 1)
    li = u(Bs, L, 3)
    li[:, 3] = -li[:, 3]
    return dict(f_vnocond=fv, f_vcond=fc, postex=60 * r(Bs, 3, n, 1), tn=F.normalize(r(Bs, 3, n, 1), dim=1),
                albedo=0.2 + 0.6 * u(1, n, 3), light_sh=0.3 * r(Bs, 3, ncol + nmono), light_sh_rand=0.3 * r(Bs, 3, ncol + nmono),
                campos=torch.tensor([[30.0, -40.0, -900.0], [-500.0, 100.0, -700.0]]),
                mips=[u(Bs, 3, h, w) * 1.7 - 0.15 for h, w in pyramid], rot=torch.linalg.qr(r(Bs, 3, 3))[0].contiguous(),
                light_intensity=li, light_pos=F.normalize(r(Bs, L, 3), dim=-1) * 1100, n_lights=torch.tensor([L, 2]))


def small_upstream(sc, seed=9):
    g = torch.Generator().manual_seed(seed)
    Bs, n = sc["f_vnocond"].shape[0], sc["f_vnocond"].shape[2]
    return {k: torch.randn(Bs, n, generator=g) if k == "sigma" else
            torch.randn(Bs, n, 4 if k == "primqvec" else 1 if k in ("opacity", "spec_vis") else 3, generator=g) for k in OUT_KEYS}


@functools.lru_cache(maxsize=None)
def small_reference(n, coefs, pyramid, env, rand, seed=0):
    """Both oracles, their quantities and the near-branch exclusion of one small scene (read-only)."""
    sc = small_scene(n, coefs, pyramid, seed)
    ups = small_upstream(sc)
    nd = 3 * coefs[0] + coefs[1]
    o64, g64 = run_oracle(sc, torch.float64, env, ups, coefs=coefs, rand=rand)
    o32, g32 = run_oracle(sc, torch.float32, env, ups, coefs=coefs, rand=rand)
    lk = lookup(sc, o64, pyramid)
    return dict(scene=sc, ups=ups, q64=quantities(o64, g64, nd), q32=quantities(o32, g32, nd),
                keep=~near_branch(sc, o64, env, lk))


ENSEMBLE = 8


@functools.lru_cache(maxsize=None)
def conditioning(env, only=None):
    """The float32 oracle's rel-L2 against float64 per (class, quantity) as an EXPECTED value: the root mean square over
    ENSEMBLE copies of the scene whose differentiable inputs are moved by at most one float32 rounding (x (1 + eps32 u), u
    uniform in [-1, 1]), each copy judged against the float64 oracle on the same copy (the recipe of
    project_cases.ensemble_rms).  Oracle numbers only.  Returns {(class, quantity): rms}."""
    ref = reference(env)
    ups = ref["ups"] if only is None else {only: ref["ups"][only]}      # `only`: one upstream gradient at a time
    acc = {}
    for k in range(ENSEMBLE):
        g = torch.Generator().manual_seed(1000 + k)
        copy = dict(ref["scene"])
        for name in LEAVES:
            copy[name] = (copy[name] * (1.0 + EPS32 * (2.0 * torch.rand(copy[name].shape, generator=g) - 1.0))).contiguous()
        q32 = quantities(*run_oracle(copy, torch.float32, env, ups))
        o64, g64 = run_oracle(copy, torch.float64, env, ups)
        q64 = quantities(o64, g64)
        # a copy may move a member next to a branch: not arithmetic error
        same = ~near_branch(copy, o64, env, lookup(copy, o64), zero_rows=BLOCKS["zero_sh"])
        for c, m, qs in judged(ref):
            for o in qs:
                mm = m & (same if m.dim() == 2 else same[..., None])
                acc.setdefault((c, o), []).append(class_rel_l2(q32[o], q64[o], mm) ** 2)
    return {key: math.sqrt(sum(v) / len(v)) for key, v in acc.items()}


# ------------------------------------------------------------------------------------------------ degenerate rows
DEG = 16
DEG_ROWS = dict(pole_up=0, pole_down=1, seam=2, seam_far=3, zero_quat=(4, 5), zero_normal=(6, 7), at_camera=(8, 9),
                along_light0=10, along_light1=11)


@functools.lru_cache(maxsize=None)
def degenerate_scene():
    """16 rows per view built from exactly representable numbers: integer camera positions, distances that are powers of
    two, axis-aligned views with the normal ALONG the view (reflection = -view exactly), lightrot = identity or a quarter
    turn about y.  Rows (DEG_ROWS): reflection exactly +y / -y; exactly on the seam (r_x = 0, r_z < 0), twice; all four
    quaternion channels 0; f_vcond[1:4] + tn = 0; position == campos; reflection exactly along light 0 / light 1; fillers."""
    g = torch.Generator().manual_seed(17)
    r = lambda *s: torch.randn(*s, generator=g)
    fv = 0.3 * r(B, ND + 12, DEG, 1)
    fv[:, ND:ND + 3] = 0.0                                                     # position = postex
    fc = 0.3 * r(B, 4, DEG, 1)
    campos = torch.tensor([[32.0, -40.0, -896.0], [-512.0, 96.0, -704.0], [0.0, 0.0, -320.0]])
    postex = campos[:, :, None, None] + 60 * r(B, 3, DEG, 1) + torch.tensor([0.0, 0.0, 800.0])[None, :, None, None]
    tn = F.normalize(r(B, 3, DEG, 1), dim=1)
    x, y, z = torch.eye(3)

    def along(row, view, dist):
        """position = campos + dist * view, normal = view: reflection = -view, exactly."""
        postex[:, :, row, 0] = campos + dist * view
        tn[:, :, row, 0] = view
        fc[:, 1:4, row, 0] = 0.0

    along(0, -y, 512.0)
    along(1, y, 512.0)
    along(2, z, 512.0)
    along(3, z, 1024.0)
    fv[:, ND + 3:ND + 7, 4:6] = 0.0
    fc[:, 1:4, 6:8] = -tn[:, :, 6:8]
    postex[:, :, 8:10, 0] = campos[:, :, None]
    along(10, z, 512.0)
    along(11, -y, 256.0)
    fv[:, ND + 11, :12] = 2.5         # broad lobes: these rows' reflections are along the axes and so are the lights; where
                                      # the exact cosine is 1, acos at a float32 cosine one ulp below is 3.5e-4 rad, not 0
    lp = torch.stack([campos + 512.0 * z - 1024.0 * z, campos - 256.0 * y + 1024.0 * y], 1)   # [B,2,3]
    li = torch.tensor([[0.9, 0.5, 0.7], [0.3, 0.8, 0.6]])[None].repeat(B, 1, 1)
    rot = torch.stack([torch.eye(3), torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]), torch.eye(3)])
    gm = torch.Generator().manual_seed(18)
    return dict(f_vnocond=fv, f_vcond=fc, postex=postex.contiguous(), tn=tn, albedo=0.2 + 0.6 * torch.rand(1, DEG, 3, generator=g),
                light_sh=0.3 * r(B, 3, NCOL + NMONO), light_sh_rand=0.3 * r(B, 3, NCOL + NMONO), campos=campos,
                mips=[torch.rand(B, 3, h, w, generator=gm) * 1.7 - 0.15 for h, w in PYRAMID], rot=rot,
                light_intensity=li, light_pos=lp.contiguous(), n_lights=torch.tensor([2, 2, 1]))


def degenerate_forward(dt, env):
    """Forward of the degenerate rows in dtype `dt` with the polar angle formed as atan2(|r_xz|, r_y) (what acos(r_y) is
    for a unit vector, and finite where acos is not).  No autograd: torch's grid_sample backward must not see these rows."""
    def dir2uv(d):
        u = torch.atan2(d[..., 0], d[..., 2]) / math.pi
        v = 2.0 * torch.atan2((d[..., 0] ** 2 + d[..., 2] ** 2).sqrt(), d[..., 1]) / math.pi - 1.0
        return torch.stack([u, v], -1)

    keep = shade_ref.dir2uv
    shade_ref.dir2uv = dir2uv
    try:
        with torch.no_grad():
            return run_oracle(degenerate_scene(), dt, env, None, grad=False)[0]
    finally:
        shade_ref.dir2uv = keep
