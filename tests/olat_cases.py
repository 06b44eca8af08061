"""Shared by the olat tests: the yardstick and the cases.

The yardstick is the two stretches of goliath_amd/urhand.py's olat_rgb_decoder_forward_rgb that csrc/olat.hip replaces --
the UNet input (its `with torch.no_grad()` block and the cat) and the OLAT sum after the UNet -- restated line for line
with the dtype as a parameter: in float64 it is the reference value, in float32 it is the existing path whose own error
against float64 sizes the bound on the kernels' largest error.  `shadow` is [B L, K, Z, Y, X] everywhere, the march's layout.
"""
import torch
import torch.nn.functional as F

import urhand_shaped as S


def prim_to_uv(shadow, primsize, npx, npy):
    """[B L, K, Z, Y, X] -> [B L, Z, npy Y, npx X]: the permute / reshape of the reference's shadow_feat."""
    X, Y, Z = primsize
    return shadow.reshape(-1, npy, npx, Z, Y, X).permute(0, 3, 1, 4, 2, 5).reshape(-1, Z, npy * Y, npx * X)


def uv_to_prim(shadow_feat, primsize, npx, npy):
    """The inverse of prim_to_uv."""
    X, Y, Z = primsize
    return shadow_feat.reshape(-1, Z, npy, Y, npx, X).permute(0, 2, 4, 1, 3, 5).reshape(-1, npy * npx, Z, Y, X).contiguous()


def features_ref(primpos, primrot, primscale, valid_prims, light_pos, campos, shadow, primsize, npx, npy, volradius,
                 dtype=torch.float64):
    """The UNet input x[B L, 7 Z, S_y, S_x] by the torch lines, computed in `dtype`."""
    primpos, primrot, primscale, valid_prims, light_pos, campos, shadow = (
        t.to(dtype) for t in (primpos, primrot, primscale, valid_prims, light_pos, campos, shadow))
    B, L = light_pos.shape[:2]
    X, Y, Z = primsize
    Sy, Sx = npy * Y, npx * X
    dev = primpos.device
    shadow_feat = prim_to_uv(shadow, primsize, npx, npy)
    grid = torch.stack(torch.meshgrid([torch.linspace(-1.0, 1.0, n, device=dev, dtype=dtype) for n in (Z, Y, X)],
                                      indexing="ij"))
    vox = grid.transpose(1, 3).reshape(3, -1)
    vox = primrot @ (vox[None, None] / primscale[..., None])
    vox = volradius * (primpos[..., None] + vox)
    vox = vox.view(B, npy, npx, 3, Z, Y, X).permute(0, 4, 3, 1, 5, 2, 6)   # B Z C H Y W X
    lvec = F.normalize(light_pos[:, :, None, :, None, None, None, None] - vox[:, None], dim=3)
    vvec = F.normalize(campos[:, None, :, None, None, None, None] - vox, dim=2)
    rot = primrot.reshape(B, npy, npx, 3, 3)
    lvec = torch.einsum("bhwef,blzehywx->blzfhywx", rot, lvec)
    vvec = torch.einsum("bhwef,bzehywx->bzfhywx", rot, vvec)
    vp = valid_prims.reshape(npy, npx)
    lvec = (vp[None, None, None, None, :, None, :, None] * lvec).reshape(B * L, -1, Sy, Sx)
    vvec = (vp[None, None, None, :, None, :, None] * vvec).reshape(B, -1, Sy, Sx)
    vvec = vvec[:, None].expand(-1, L, -1, -1, -1).reshape(B * L, -1, Sy, Sx)
    return torch.cat([lvec, vvec, 1.0 - shadow_feat], dim=1)


def combine_ref(tex, light_intensity, shadow, primsize, npx, npy, use_shadow, dtype=torch.float64):
    """(rgb, texolat, primshadow) by the torch lines after the UNet, computed in `dtype`; differentiable in `tex`."""
    X, Y, Z = primsize
    Sy, Sx = npy * Y, npx * X
    B, L = light_intensity.shape[:2]
    shadow_feat = prim_to_uv(shadow.to(dtype), primsize, npx, npy)
    light_intensity = light_intensity.to(dtype).expand(-1, -1, 3)[:, :, None, :, None, None]
    tex = tex.to(dtype).view(B, L, Z, 4, Sy, Sx)
    if use_shadow:
        shadowolat = shadow_feat.reshape(B, L, Z, 1, Sy, Sx)
    else:
        shadowolat = torch.sigmoid(tex[:, :, :, :1])
    texolat = 25.0 * tex[:, :, :, 1:] + 100.0
    rgb = (shadowolat * F.relu(texolat) * light_intensity).sum(1).view(B, Z, 3, Sy, Sx)
    primshadow = shadow_feat[:, :, None].expand(-1, -1, 3, -1, -1).reshape(B, L, Z, 3, Sy, Sx).sum(1) / L
    return rgb, texolat, primshadow


# ---------------------------------------------------------------------------------------------------------------- cases
GEOM_KEYS = ("primpos", "primrot", "primscale", "valid_prims", "light_pos", "campos")


def _rotations(B, K, g):
    q = F.normalize(torch.randn(B, K, 4, generator=g) * 0.3 + torch.tensor([1.0, 0, 0, 0]), dim=-1)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z),
                        1 - 2 * (x * x + z * z), 2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x),
                        1 - 2 * (x * x + y * y)], -1).reshape(B, K, 3, 3)


def standin_case(B, L, seed=11):
    """(a) the stand-in's shape: 4 x 4 primitives of 4 x 4 x 2 voxels, S = 16, primitive 5 invalid (urhand_shaped)."""
    inp = S.teacher_inputs(B=B, L=L)
    g = torch.Generator().manual_seed(seed + 10 * B + L)
    case = {k: inp[k] for k in GEOM_KEYS}
    case.update(primsize=(4, 4, 2), npx=4, npy=4, volradius=200.0, shadow=torch.rand(B * L, 16, 2, 4, 4, generator=g))
    return case


def odd_case(seed=12):
    """(b) nothing is a multiple of four and nothing is square: 3 x 6 primitives of 2 x 4 x 3 voxels (X, Y, Z), S = 12."""
    B, L, npx, npy = 2, 2, 6, 3
    X, Y, Z = 2, 4, 3
    K = npx * npy
    g = torch.Generator().manual_seed(seed)
    valid = torch.ones(K)
    valid[7] = 0.0
    return dict(primpos=40.0 * torch.randn(B, K, 3, generator=g), primrot=_rotations(B, K, g),
                primscale=(200.0 / 30.0) * (1.0 + 0.3 * torch.rand(B, K, 3, generator=g)), valid_prims=valid,
                light_pos=torch.tensor([[[150.0, 80.0, 560.0], [-220.0, -40.0, 520.0]]]).repeat(B, 1, 1)
                + 4.0 * torch.randn(B, L, 3, generator=g),
                campos=torch.tensor([[20.0, -30.0, 650.0]]).repeat(B, 1) + torch.randn(B, 3, generator=g),
                primsize=(X, Y, Z), npx=npx, npy=npy, volradius=200.0, shadow=torch.rand(B * L, K, Z, Y, X, generator=g))


def degenerate_case(seed=13):
    """(c) identity transforms, so every primitive's voxels lie at volradius * local, and light 1 sits exactly on the voxel
    labelled (0, 0, 0): local = (-1, -1, -1), a position that is exact in every precision.  The float64 yardstick gives the
    zero vector there.  Returns the case and the [B L, 7 Z, S, S] bool mask of the light-direction entries concerned."""
    B, L, npx, npy = 1, 2, 4, 4
    X, Y, Z = 4, 4, 2
    K = npx * npy
    g = torch.Generator().manual_seed(seed)
    vol = 200.0
    case = dict(primpos=torch.zeros(B, K, 3), primrot=torch.eye(3).expand(B, K, 3, 3).contiguous(),
                primscale=torch.ones(B, K, 3), valid_prims=torch.ones(K),
                light_pos=torch.tensor([[[150.0, 80.0, 560.0], [-vol, -vol, -vol]]]),
                campos=torch.tensor([[20.0, -30.0, 650.0]]), primsize=(X, Y, Z), npx=npx, npy=npy, volradius=vol,
                shadow=torch.rand(B * L, K, Z, Y, X, generator=g))
    hit = torch.zeros(B * L, 7 * Z, npy * Y, npx * X, dtype=torch.bool)
    hit[1, 0:3, 0::Y, 0::X] = True          # light 1, z = 0, the light-direction channels, texel (0, 0) of every primitive
    return case, hit


FIXED_KINK = ((0, 1, 0, 0), (0, 2, 3, 5), (0, 3, 7, 2), (-1, 5, 1, 1), (-1, 6, 11, 9))   # (image, channel, row, col)


def combine_case(B, L, primsize=(4, 4, 2), npx=4, npy=4, seed=21):
    """tex[B L, 4 Z, S_y, S_x] around the relu's kink (texolat = 25 t + 100 changes sign at t = -4) with |texolat| >= 1e-3
    everywhere -- the band in which a fused and an unfused multiply-add may disagree about the sign holds no samples --
    except the FIXED_KINK entries, which are exactly -4.0: there texolat is exactly 0 in any arithmetic."""
    X, Y, Z = primsize
    K = npx * npy
    g = torch.Generator().manual_seed(seed + 10 * B + L)
    tex = torch.randn(B * L, 4 * Z, npy * Y, npx * X, generator=g) * 1.5
    colour = torch.ones(4 * Z, dtype=torch.bool)
    colour[0::4] = False                      # channel 4 z is the sigmoid's input
    t = tex[:, colour] - 4.0
    t[(25.0 * t + 100.0).abs() < 1e-3] = -3.9
    tex[:, colour] = t
    kinks = [k for k in FIXED_KINK if k[1] % 4 != 0 and k[1] < 4 * Z and k[2] < npy * Y and k[3] < npx * X]
    for n, c, r, q in kinks:
        tex[n, c, r, q] = -4.0
    return dict(tex=tex, light_intensity=0.5 + torch.rand(B, L, 3, generator=g),
                shadow=torch.rand(B * L, K, Z, Y, X, generator=g), primsize=primsize, npx=npx, npy=npy, kinks=kinks)
