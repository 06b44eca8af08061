"""Make the reference's Python code (`ca_code`, `extensions/*/*.py`) run on libgoliath_hip.so unchanged.

    import goliath_amd.dropin as dropin
    dropin.install()              # before importing ca_code.* / extensions.*
    dropin.patch_rgca()           # optional: fused shading tail + batched, sync-free render
    dropin.patch_light_decorator()  # optional: the env-relight driver hands over ONE shared pyramid (config 2)
    dropin.patch_geometry()       # optional: GeometryModule.to_uv / .vn and the decoder's postex / tn on the uvgeom kernels
    dropin.install_pytorch3d_shim()  # optional, before importing ca_code.*: lets geom / urhand / hand_mvp import without pytorch3d
    dropin.patch_geometry_ctor()  # optional: GeometryModule(...) builds its index / bary / face images (and the impaint) on HIP
    dropin.patch_lbs()            # optional: LinearBlendSkinning / LBSModule.pose on the fused skeleton + skinning kernels
    dropin.patch_relight_vis()    # optional, with patch_rgca(): run_vis_relight's frames from ONE render + the HIP env background
    dropin.patch_sh()             # optional: sh.dir2sh_torch and (with patch_rgca()) the frame's light SH on ONE HIP launch, no host sync
    dropin.patch_env_driver()     # optional: EnvSpinDecorator.forward's per-frame map rotation, light probe and mip scale on the GPU
    dropin.patch_env_prefilter()  # optional: envmap.prefilterEnvmapSG (the pyramid of _set_lightmap) on ONE HIP kernel per level
    dropin.patch_encoder()        # optional: Encoder.forward's texture stack on the fused conv + bias + LeakyReLU operator
    dropin.patch_view_texture()   # optional: geom.compute_view_texture and its two visibility helpers (run_gen_texmean) on two HIP kernels, no host sync
    dropin.set_environment(decorator, image)   # another environment map for a live EnvSpinDecorator, pyramid built on the GPU

`install()` registers the module names the reference imports for its native code:
    gsplat            project_gaussians, rasterize_gaussians   (ca_code/utils/render_gsplat.py:10-11)
    sgutilslib        evaluate_gaussian_fwd/_bwd               (extensions/sgutils/sgutils.py:12-15)
    mvpraymarchlib    compute_aabb, raymarch_forward/_backward (extensions/mvpraymarch/mvpraymarch.py:15-18)
    utilslib          compute_raydirs_forward/_backward        (extensions/utils/utils.py:20-23)
so `run_train.py` / `run_vis_relight.py` need no edit.  `patch_rgca()` additionally swaps the two
Python-level hot spots of ca_code.models.rgca for their fused equivalents (same signatures/returns).
"""
import importlib.machinery
import sys
import types



def install():
    from . import mvp, sg, splat

    gs = types.ModuleType("gsplat")
    gs.project_gaussians = splat.project_gaussians
    gs.rasterize_gaussians = splat.rasterize_gaussians
    gs.__version__ = "0.1.11+goliath_amd"
    sys.modules["gsplat"] = gs
    for name, obj in (("sgutilslib", sg.sgutilslib), ("mvpraymarchlib", mvp.mvpraymarchlib), ("utilslib", mvp.utilslib)):
        m = types.ModuleType(name)
        for attr in dir(obj):
            if not attr.startswith("_"):
                setattr(m, attr, getattr(obj, attr))
        sys.modules[name] = m
    return ["gsplat", "sgutilslib", "mvpraymarchlib", "utilslib"]


def patch_rgca(rgca_module=None):
    """Swap AutoEncoder.render (rgca.py:112-151), AutoEncoder.forward (rgca.py:153-253: the image tail after the render
    becomes one fused pass) and PrimDecoder.forward (rgca.py:466-620) for the batched / fused versions in
    goliath_amd.rgca.  Returns the patched module."""
    from . import rgca as fused

    if rgca_module is None:
        import ca_code.models.rgca as rgca_module
    rgca_module.AutoEncoder.render = fused.autoencoder_render
    rgca_module.AutoEncoder.forward = fused.autoencoder_forward
    rgca_module.PrimDecoder.forward = fused.prim_decoder_forward
    return rgca_module


def patch_encoder(rgca_module=None):
    """Opt in to the fused texture encoder: `Encoder.forward` (rgca.py:310-332) becomes goliath_amd.encoder.encoder_forward,
    which runs the (Conv2dWNUB 4/2/1, LeakyReLU) pairs of `texmod` that goliath_amd.encoder.DISPATCH admits on
    gol_enc_conv_fwd / _bwd and folds `color / 255.0 - 0.5` into the first layer's load when that layer is taken.  CPU
    tensors and shapes that are not admitted take the module path: the reference's own lines, identical results.  Implies
    none of the other patches; idempotent.  Returns the patched module."""
    from . import encoder

    if rgca_module is None:
        import ca_code.models.rgca as rgca_module
    rgca_module.Encoder.forward = encoder.encoder_forward
    return rgca_module


def patch_relight_vis(rgca_module=None):
    """Opt in to the fused relight visualisation: with it (and patch_rgca(), which installs the forward that reads the flag)
    the `envbg` branch of AutoEncoder.forward (rgca.py:232-245, what run_vis_relight.py:110-122 calls under no_grad) makes
    ONE render -- the diffuse / specular breakdown rides as six extra channels over the lit render's tile lists
    (gol_rasterize_nd_fwd) instead of two further project + bin + sort + raster passes -- and composites the env-map
    background and the mirror ball with goliath_amd.envbg (gol_envbg_image / gol_envbg_compose) instead of
    ca_code.utils.envmap.compose_envmap's bicubic grid_sample + 101 x 101 depthwise conv2d.  Forward-only: with grad mode
    on the branch stays the reference's.  Sets a class flag on AutoEncoder; idempotent.  Returns the patched module."""
    from . import rgca as fused

    if rgca_module is None:
        import ca_code.models.rgca as rgca_module
    setattr(rgca_module.AutoEncoder, fused.RELIGHT_VIS_FLAG, True)
    return rgca_module


def patch_sh(sh_module=None, rgca_module=None):
    """Opt in to the fused light path (goliath_amd.lights, csrc/lightsh.hip):
      * `sh_module.dir2sh_torch` (ca_code/utils/sh.py:118-127: (deg+1)^2 functions evaluated one at a time, a device-to-host
        sync each) is replaced by a wrapper that runs lights.dir2sh -- one launch, no sync -- for CUDA float32 directions
        that need no gradient and deg <= 8; CPU tensors, other dtypes, deg > 8 and (with grad mode on) directions that
        require grad go to the original, kept on the wrapper as `.reference`;
      * a class flag on `AutoEncoder` and `PrimDecoder` (goliath_amd.rgca.LIGHT_SH_FLAG): with it the forwards
        patch_rgca() installs take headrel_light_pos / headrel_light_sh from ONE gol_light_sh_fwd and the training-only
        random light from lights.random_light_sh, under the same input conditions; without it they run the reference's
        lines and call whatever `ca_code.utils.sh.dir2sh_torch` is.
    Idempotent (patching twice does not wrap twice).  Returns (sh_module, rgca_module)."""
    from . import lights
    from . import rgca as fused

    if sh_module is None:
        import ca_code.utils.sh as sh_module
    if rgca_module is None:
        import ca_code.models.rgca as rgca_module
    original = sh_module.dir2sh_torch
    if not getattr(original, "_goliath_dir2sh", False):
        import torch

        def dir2sh_torch(deg, dirs):
            if (torch.is_tensor(dirs) and dirs.is_cuda and dirs.dtype == torch.float32 and 0 <= deg <= lights.MAX_DEG
                    and not (torch.is_grad_enabled() and dirs.requires_grad)):
                return lights.dir2sh(deg, dirs)
            return original(deg, dirs)

        dir2sh_torch.reference = original
        dir2sh_torch._goliath_dir2sh = True
        sh_module.dir2sh_torch = dir2sh_torch
    for cls in (rgca_module.AutoEncoder, rgca_module.PrimDecoder):
        setattr(cls, fused.LIGHT_SH_FLAG, True)
    return sh_module, rgca_module


def patch_geometry(geom_module=None):
    """Rebind `GeometryModule.to_uv` and `.vn` (ca_code/utils/geom.py:267-271) to the fused HIP operators of
    goliath_amd.uvgeom (gol_values_to_uv / gol_vert_normals: no boolean-mask gather, no host sync, graph-capturable).  The
    packed topology is built lazily from the module's own `vi` / `index_image` / `bary_image` buffers and rebuilt when
    their device or shape changes.  With it, goliath_amd.rgca.prim_decoder_forward makes one `uv_geometry` call for
    `postex` / `tn`.  Idempotent.  Returns the patched module."""
    from . import uvgeom

    if geom_module is None:
        import ca_code.utils.geom as geom_module
    geom_module.GeometryModule.to_uv = uvgeom.geometry_to_uv
    geom_module.GeometryModule.vn = uvgeom.geometry_vn
    return geom_module


def patch_geometry_ctor(geom_module=None):
    """Rebind `geom.make_uv_face_index` (ca_code/utils/geom.py:31-66: pytorch3d's CUDA rasterize_meshes) and
    `geom.index_image_impaint` (geom.py:145-194: a scikit-learn KD-tree on the host) to goliath_amd.uvtopo
    (gol_mesh_raster on the UV triangles, gol_nearest_valid), so that an unmodified `GeometryModule(...)` and
    `render_index_images(...)` build their index / barycentric / face images without either package; the reference's own
    make_uv_vert_index, make_uv_barys and bary_coords keep running on the face image they are handed.  Like the reference
    the replacements accept the constructor's CPU buffers: the work runs on `device` (default "cuda") and the impainted
    images come back where the inputs were.  Conventions (what is pinned by the reference, what is stated): see
    goliath_amd/uvtopo.py.  Idempotent.  Returns the patched module."""
    from . import uvtopo

    if geom_module is None:
        import ca_code.utils.geom as geom_module

    def make_uv_face_index(vt, vti, uv_shape, flip_uv=True, device=None):
        return uvtopo.uv_face_index(vt, vti, uv_shape, flip_uv=flip_uv, device="cuda" if device is None else device)

    def index_image_impaint(index_image, bary_image=None, distance_threshold=100.0):
        device = None if index_image.is_cuda and (bary_image is None or bary_image.is_cuda) else "cuda"
        return uvtopo.impaint(index_image, bary_image, distance_threshold, device=device)

    geom_module.make_uv_face_index = make_uv_face_index
    geom_module.index_image_impaint = index_image_impaint
    return geom_module


def patch_view_texture(geom_module=None, tex_module=None):
    """Opt in to the fused camera-to-UV unwrap (goliath_amd.viewtex, csrc/viewtex.hip): rebinds
    `geom.compute_face_visibility`, `geom.compute_uv_visiblity_face` and `geom.compute_view_texture`
    (ca_code/utils/geom.py:834-910: two Python loops over the batch with a th.unique and a host sync each, boolean-mask
    gathers and scatters) to wrappers that run viewtex for CUDA inputs with a float32 image / float32 vertices; everything
    else goes to the original, kept on the wrapper as `.reference`.  If `ca_code.utils.tex` is already imported (or is
    passed in) its by-name import `compute_view_texture` and its `get_tex_rl` (tex.py:21-63) are rebound too; this patch
    does not import it (it pulls in drtk and cv2).  Implies no other patch; idempotent.  Returns the patched geom module."""
    from . import viewtex

    if geom_module is None:
        import ca_code.utils.geom as geom_module
    if tex_module is None:
        tex_module = sys.modules.get("ca_code.utils.tex")
    import torch

    def on_gpu(*tensors):
        return all(torch.is_tensor(t) and t.is_cuda for t in tensors)

    def wrap(module, name, make):
        original = getattr(module, name)
        if getattr(original, "_goliath_viewtex", False):
            return original
        fn = make(original)
        fn.__name__ = name
        fn.reference = original
        fn._goliath_viewtex = True
        setattr(module, name, fn)
        return fn

    def make_face_visibility(original):
        def compute_face_visibility(index_img, faces):
            if on_gpu(index_img) and index_img.dtype in (torch.int32, torch.int64):
                return viewtex.face_visibility(index_img, faces.shape[0])
            return original(index_img, faces)
        return compute_face_visibility

    def make_uv_visibility(original):
        def compute_uv_visiblity_face(face_index_image, faces, face_index_uv):
            if on_gpu(face_index_image, face_index_uv) and face_index_image.dtype in (torch.int32, torch.int64):
                return viewtex.uv_visibility(face_index_image, faces.shape[0], face_index_uv)
            return original(face_index_image, faces, face_index_uv)
        return compute_uv_visiblity_face

    def make_view_texture(original):
        def compute_view_texture(verts, faces, image, face_index_image, normal_image, K, Rt, index_image_uv, bary_image_uv,
                                 face_index_uv, intensity_threshold=None, normal_threshold=None):
            if (on_gpu(verts, image, face_index_image, K, Rt, index_image_uv, bary_image_uv, face_index_uv)
                    and image.dtype == torch.float32 and verts.dtype == torch.float32):
                return viewtex.compute_view_texture(verts, faces, image, face_index_image, normal_image, K, Rt,
                                                    index_image_uv, bary_image_uv, face_index_uv,
                                                    intensity_threshold=intensity_threshold,
                                                    normal_threshold=normal_threshold)
            return original(verts, faces, image, face_index_image, normal_image, K, Rt, index_image_uv, bary_image_uv,
                            face_index_uv, intensity_threshold=intensity_threshold, normal_threshold=normal_threshold)
        return compute_view_texture

    def make_get_tex_rl(original):
        def get_tex_rl(rl, image, ply, extrin, intrin, face_index, index_image, bary_image):
            if (on_gpu(image, ply[0], extrin, intrin, face_index, index_image, bary_image)
                    and image.dtype == torch.float32 and ply[0].dtype == torch.float32):
                return viewtex.get_tex_rl(rl, image, ply, extrin, intrin, face_index, index_image, bary_image)
            return original(rl, image, ply, extrin, intrin, face_index, index_image, bary_image)
        return get_tex_rl

    wrap(geom_module, "compute_face_visibility", make_face_visibility)
    wrap(geom_module, "compute_uv_visiblity_face", make_uv_visibility)
    cvt = wrap(geom_module, "compute_view_texture", make_view_texture)
    if tex_module is not None:
        if hasattr(tex_module, "compute_view_texture"):
            tex_module.compute_view_texture = cvt
        if hasattr(tex_module, "get_tex_rl"):
            wrap(tex_module, "get_tex_rl", make_get_tex_rl)
    return geom_module


def _pytorch3d_placeholder(name):
    def placeholder(*args, **kwargs):
        raise RuntimeError(f"pytorch3d.{name} is a placeholder: pytorch3d is not installed.  The UV index images of "
                           "GeometryModule are built without it after goliath_amd.dropin.patch_geometry_ctor(); the "
                           "pytorch3d mesh renderer has no stand-in (use goliath_amd.meshraster.RenderLayer)")

    placeholder.__name__ = placeholder.__qualname__ = name.rsplit(".", 1)[-1]
    return placeholder


def axis_angle_to_matrix(axis_angle):
    """pytorch3d.transforms.axis_angle_to_matrix restated in plain torch: [..., 3] -> [..., 3, 3], Rodrigues' formula
    R = I + (sin t / t) K + ((1 - cos t) / t^2) K^2 with K the cross-product matrix of the vector, t its length (the two
    ratios by their Taylor series below t = 1e-4)."""
    import torch

    t2 = (axis_angle * axis_angle).sum(-1)
    t = t2.sqrt()
    small = t < 1e-4
    ts = torch.where(small, torch.ones_like(t), t)
    a = torch.where(small, 1.0 - t2 / 6.0, ts.sin() / ts)
    b = torch.where(small, 0.5 - t2 / 24.0, (1.0 - ts.cos()) / (ts * ts))
    x, y, z = axis_angle.unbind(-1)
    o = torch.zeros_like(x)
    K = torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(axis_angle.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=axis_angle.dtype, device=axis_angle.device)
    return eye + a[..., None, None] * K + b[..., None, None] * (K @ K)


def euler_angles_to_matrix(euler_angles, convention):
    """pytorch3d.transforms.euler_angles_to_matrix restated: [..., 3] angles in radians and a convention of three letters
    out of "XYZ" -> the product R_c0(a0) R_c1(a1) R_c2(a2) of the elementary right-handed rotations, [..., 3, 3]."""
    import torch

    if len(convention) != 3 or any(c not in "XYZ" for c in convention) or convention[1] in (convention[0], convention[2]):
        raise ValueError(f"invalid convention {convention!r}")

    def axis(letter, angle):
        c, s, o, l = angle.cos(), angle.sin(), torch.zeros_like(angle), torch.ones_like(angle)
        flat = {"X": (l, o, o, o, c, -s, o, s, c), "Y": (c, o, s, o, l, o, -s, o, c), "Z": (c, -s, o, s, c, o, o, o, l)}[letter]
        return torch.stack(flat, -1).reshape(angle.shape + (3, 3))

    m = [axis(c, a) for c, a in zip(convention, euler_angles.unbind(-1))]
    return m[0] @ m[1] @ m[2]


def matrix_to_axis_angle(matrix):
    """pytorch3d.transforms.matrix_to_axis_angle restated: rotation matrices [..., 3, 3] -> axis * angle [..., 3], angle in
    [0, pi].  Through the unit quaternion with the larger of the four candidate components as pivot (stable at every
    angle, pi included), w made non-negative, angle = 2 atan2(|xyz|, w)."""
    import torch

    m = matrix
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    q_abs = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], -1)
    q_abs = q_abs.clamp(min=0.0).sqrt()                       # 2 |w|, 2 |x|, 2 |y|, 2 |z|
    cand = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m[..., 2, 1] - m[..., 1, 2], m[..., 0, 2] - m[..., 2, 0], m[..., 1, 0] - m[..., 0, 1]], -1),
        torch.stack([m[..., 2, 1] - m[..., 1, 2], q_abs[..., 1] ** 2, m[..., 1, 0] + m[..., 0, 1], m[..., 0, 2] + m[..., 2, 0]], -1),
        torch.stack([m[..., 0, 2] - m[..., 2, 0], m[..., 1, 0] + m[..., 0, 1], q_abs[..., 2] ** 2, m[..., 1, 2] + m[..., 2, 1]], -1),
        torch.stack([m[..., 1, 0] - m[..., 0, 1], m[..., 2, 0] + m[..., 0, 2], m[..., 2, 1] + m[..., 1, 2], q_abs[..., 3] ** 2], -1),
    ], -2)                                                    # [..., 4 pivots, 4]: 4 p (w, x, y, z) for pivot p
    pivot = q_abs.argmax(-1)
    q = torch.gather(cand, -2, pivot[..., None, None].expand(pivot.shape + (1, 4)))[..., 0, :]
    q = q / (2.0 * torch.gather(q_abs, -1, pivot[..., None]).clamp(min=0.1))
    q = torch.where(q[..., :1] < 0, -q, q)
    n = q[..., 1:].norm(dim=-1, keepdim=True)
    angle = 2.0 * torch.atan2(n, q[..., :1])
    # angle / |xyz|: 2 / w-ish near 0 (sin(t/2) ~ t/2 -> factor 2)
    factor = torch.where(n < 1e-6, torch.full_like(n, 2.0), angle / n.clamp(min=1e-30))
    return q[..., 1:] * factor


def install_pytorch3d_shim():
    """Where `import pytorch3d` fails, register the least of it that lets `ca_code.utils.geom`, `ca_code.models.urhand`
    and `ca_code.models.hand_mvp` import: `pytorch3d.transforms.axis_angle_to_matrix`, `euler_angles_to_matrix` and
    `matrix_to_axis_angle` (urhand.py:773 calls them every frame) as the plain-torch restatements above; `Meshes`,
    `rasterize_meshes`, `TexturesUV`, `MeshRasterizer`, `RasterizationSettings`, `cameras_from_opencv_projection`,
    `load_ply` and `save_ply` as placeholders whose call raises an error naming patch_geometry_ctor().  Does nothing when
    the real package imports.  Returns the list of module names it registered."""
    try:
        import pytorch3d  # noqa: F401

        return []
    except ImportError:
        pass
    layout = {
        "pytorch3d": {},
        "pytorch3d.structures": {"Meshes": None},
        "pytorch3d.renderer": {"MeshRasterizer": None, "RasterizationSettings": None},
        "pytorch3d.renderer.mesh": {},
        "pytorch3d.renderer.mesh.rasterize_meshes": {"rasterize_meshes": None},
        "pytorch3d.renderer.mesh.textures": {"TexturesUV": None},
        "pytorch3d.utils": {"cameras_from_opencv_projection": None},
        "pytorch3d.io": {"load_ply": None, "save_ply": None},
        "pytorch3d.transforms": {"axis_angle_to_matrix": axis_angle_to_matrix,
                                 "euler_angles_to_matrix": euler_angles_to_matrix,
                                 "matrix_to_axis_angle": matrix_to_axis_angle},
    }
    for name, attrs in layout.items():
        m = types.ModuleType(name)
        m.__path__ = []           # a package: `import pytorch3d.renderer.mesh.textures` walks the chain
        m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)   # importlib.util.find_spec() needs one
        for attr, obj in attrs.items():
            setattr(m, attr, obj if obj is not None else _pytorch3d_placeholder(f"{name[len('pytorch3d.'):]}.{attr}"))
        sys.modules[name] = m
    for name in layout:          # parents carry their children as attributes
        parent, _, child = name.rpartition(".")
        if parent:
            setattr(sys.modules[parent], child, sys.modules[name])
    return list(layout)


def patch_lbs(lbs_module=None):
    """Rebind `LinearBlendSkinning.forward`, `.compute_rigid_transforms`, `.compute_rigid_transforms_matrix` and
    `LBSModule.pose` / `.template_pose` (ca_code/utils/lbs.py:151-169, 308-337, 725-731, 741-745) to the fused HIP operators
    of goliath_amd.lbs (gol_lbs_skeleton_* / gol_lbs_skin_*: no per-joint host sync, two launches forward, at most four
    backward, graph-capturable, bitwise reproducible).  The packed skeleton is built lazily from the module's own buffers
    and rebuilt when their device or shape changes.  Left alone by decision: `unpose` / `unskinning` (body models, out of
    scope per SURVEY section 2) and `compute_root_rigid_transform`.  Idempotent.  Returns the patched module."""
    from . import lbs

    if lbs_module is None:
        import ca_code.utils.lbs as lbs_module
    cls = lbs_module.LinearBlendSkinning
    cls.forward = lbs.lbs_forward
    cls.compute_rigid_transforms = lbs.lbs_compute_rigid_transforms
    cls.compute_rigid_transforms_matrix = lbs.lbs_compute_rigid_transforms_matrix
    lbs_module.LBSModule.pose = lbs.lbs_module_pose
    lbs_module.LBSModule.template_pose = lbs.lbs_module_template_pose
    return lbs_module


def _shared_mipmap(self, bsize, device, scale=1.0):
    """EnvSpinDecorator.mipmap (ca_code/utils/light_decorator.py:96-100) without the B materialised copies: the reference
    expands each registered level over the batch and then multiplies by `scale`, which writes B identical scaled maps (at the
    run_vis_relight size 8 x 10.5 MB).  Here ONE map is scaled (other readers of `preconv_envmap` see the reference's values)
    and the batch axis is a stride-0 view.  `scale` is 2 pi norm_scale[0] of the FRAME (:147-149), so the scaled tensor is a
    new one every step: each level therefore also carries the unscaled registered buffer (on `device`, cached on the
    decorator) and the scale -- goliath_amd.shade packs the footprint records of THAT buffer once per environment (its address
    and version do not change with the spin index) and hands the scale to the kernel (gol_shade_in.mips_scale): 42 MB of
    records for 8 views instead of 335 MB, no re-packing per step; what does run per step is the scaling of the one map."""
    cache = self.__dict__.setdefault("_gol_dev_levels", {})
    out = []
    for i in range(self.miplevel):
        buf = getattr(self, f"mipmap_{i}")
        key = (i, str(device), buf.data_ptr(), buf._version)
        base = cache.get(key)
        if base is None:
            for k in [k for k in cache if k[0] == i and k[1] == str(device)]:
                del cache[k]                         # the buffer was replaced / rewritten: drop the stale device copy
            base = cache[key] = buf.to(device)
        m = (base * scale).expand(bsize, -1, -1, -1)
        # a CUDA tensor (envdriver's mip_scale) stays one: `base * scale` above was a device multiply, and shade hands the
        # tensor's address to the kernel instead of waiting for its value
        m._gol_base, m._gol_scale = base, scale if getattr(scale, "is_cuda", False) else float(scale)
        out.append(m)
    return out


def patch_light_decorator(decorator_module=None):
    """BASELINE config 2's relight driver as a drop-in: `EnvSpinDecorator.mipmap` returns stride-0 batch views of the one
    prefiltered pyramid (see _shared_mipmap); nothing else of the decorator changes.  Returns the patched module."""
    if decorator_module is None:
        import ca_code.utils.light_decorator as decorator_module
    decorator_module.EnvSpinDecorator.mipmap = _shared_mipmap
    return decorator_module


def _env_spin_state(self, device):
    """The decorator's goliath_amd.envdriver.EnvSpin, built lazily from `self.image` and rebuilt when the image (address,
    in-place version), the device or one of the scalars it bakes in changes.  None: this decorator stays on the reference
    (no GPU, or perc90 <= 0 -- the reference then divides by the maximum of every rotated frame, light_decorator.py:125)."""
    import numpy as np

    from . import envdriver

    key = (self.image.data_ptr(), self.image._version, str(device), float(self.env_scale), self.cycle,
           float(self.envmap_dist))
    hit = self.__dict__.get("_gol_env_spin")
    if hit is None or hit[0] != key:
        state = None
        if device.type == "cuda":
            perc90 = np.percentile(self.image.data.cpu().numpy(), 90)
            if perc90 > 0:
                state = envdriver.EnvSpin(self.image, self.env_scale, cycle=self.cycle, envmap_dist=self.envmap_dist,
                                          perc90=perc90, device=device)
        hit = self.__dict__["_gol_env_spin"] = (key, state)
    return hit[1]


def _env_driver_forward(self, reference, **data):
    """EnvSpinDecorator.forward (ca_code/utils/light_decorator.py:102-164) on goliath_amd.envdriver: the same keys, shapes
    and dtypes in `data`, from three launches per frame instead of a CPU grid_sample, a percentile, a CPU interpolate and a
    6 MB upload per view.  `preconv_envmap` comes from self.mipmap with the frame's scale as a DEVICE tensor (with
    patch_light_decorator() the shading kernel reads it from there)."""
    import torch

    device = data["campos"].device
    batch_size = data["campos"].size(0)
    state = _env_spin_state(self, device)
    if state is None:
        return reference(self, **data)
    index = data["index"]
    index = index[:batch_size] if torch.is_tensor(index) else [index[i] for i in range(batch_size)]
    with torch.no_grad():
        fr = state.frame(index=index)
    data["preconv_envmap"] = self.mipmap(batch_size, device, fr.mip_scale)
    data["sigma_step"] = self.sigma_step
    data["envmap"] = fr.envmap
    data["lightrot"] = fr.lightrot
    data["light_intensity"] = fr.light_intensity
    data["light_pos"] = fr.light_pos
    data["envbg"] = fr.envbg
    data["light_type"] = "envmap"
    data["n_lights"] = fr.n_lights
    data["is_fullylit_frame"] = torch.zeros(1, device=device)
    return self.mod(**data)


def patch_env_driver(decorator_module=None):
    """Opt in to the fused relight driver: `EnvSpinDecorator.forward` becomes _env_driver_forward; the original stays on it
    as `.reference` and still serves a decorator whose np.percentile(image, 90) is not positive.  Implies none of the other
    patches and changes no default path; idempotent.  A sync-free loop also needs GOLIATH_CHECK_LIGHTROT=0.
    Returns the patched module."""
    if decorator_module is None:
        import ca_code.utils.light_decorator as decorator_module
    cls = decorator_module.EnvSpinDecorator
    original = cls.forward
    if not getattr(original, "_goliath_env_driver", False):
        def forward(self, **data):
            return _env_driver_forward(self, original, **data)

        forward.reference = original
        forward._goliath_env_driver = True
        cls.forward = forward
    return decorator_module


def patch_env_prefilter(envmap_module=None):
    """Opt in to the fused SG prefilter: `envmap.prefilterEnvmapSG` (ca_code/utils/envmap.py:305-323: num_samples Python
    iterations of two dozen ATen kernels each) becomes a wrapper that sends CUDA float32 inputs which need no gradient to
    goliath_amd.envprefilter.prefilter_sg -- two launches -- with a seed drawn from torch's generator (torch.randint on the
    host: torch.manual_seed makes the result repeatable, as it does the reference's rand_like).  CPU tensors, other dtypes
    and (grad mode on) inputs that require grad go to the original, kept on the wrapper as `.reference`.  The reference's
    own EnvSpinDecorator._set_lightmap (light_decorator.py:64-94) then builds its pyramid in three kernel calls, unchanged.
    Implies none of the other patches; idempotent.  Returns the patched module."""
    if envmap_module is None:
        import ca_code.utils.envmap as envmap_module
    original = envmap_module.prefilterEnvmapSG
    if not getattr(original, "_goliath_env_prefilter", False):
        import torch

        from . import envprefilter

        def prefilterEnvmapSG(sigma, v, env_tex, num_samples=1):
            ok = all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
                     and not (torch.is_grad_enabled() and t.requires_grad) for t in (v, env_tex))
            if not ok:
                return original(sigma, v, env_tex, num_samples)
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())      # a host tensor: no device sync
            return envprefilter.prefilter_sg(sigma, v, env_tex, num_samples, seed=seed)

        prefilterEnvmapSG.reference = original
        prefilterEnvmapSG._goliath_env_prefilter = True
        envmap_module.prefilterEnvmapSG = prefilterEnvmapSG
    return envmap_module


def set_environment(decorator, image, num_samples=4096, seed=0):
    """Give an EnvSpinDecorator another environment map without the reference's loop: `decorator.image` and its `mipmap_i`
    buffers (light_decorator.py:61-62, :93-94) are REPLACED by `image` [3,H,W] (kept on the device it is given on) and the
    pyramid goliath_amd.envprefilter.build_pyramid makes of it on the GPU (the image's, else the old pyramid's, else the
    current one), with the decorator's own sigma_step and miplevel.  New tensors, new addresses: _shared_mipmap and
    _env_spin_state key their caches on the buffers' address and version and drop their stale copies on the next frame.
    Returns the decorator."""
    import torch

    from . import envprefilter

    image = image.detach().to(torch.float32).contiguous()
    dev = image.device
    if dev.type != "cuda":           # a host image: build where the pyramid lives, or on the current GPU
        old = getattr(decorator, "mipmap_0", None)
        dev = old.device if torch.is_tensor(old) and old.is_cuda else torch.device("cuda")
    with torch.no_grad():
        levels = envprefilter.build_pyramid(image.to(dev), sigma_step=decorator.sigma_step, miplevel=decorator.miplevel,
                                            num_samples=num_samples, seed=seed)
    # the reference's forward rotates self.image where it lies (light_decorator.py:120): the new one stays on its device
    decorator.image = image
    for i, level in enumerate(levels):
        name = f"mipmap_{i}"
        if isinstance(decorator, torch.nn.Module) and name not in decorator._buffers:
            decorator.register_buffer(name, level)
        else:
            setattr(decorator, name, level)          # (nn.Module.__setattr__ replaces a registered buffer)
    return decorator


REGULARIZER_LOSSES = ("bound_primscale", "negcolor", "l2_reg", "list_l1_reg", "backlit_reg", "alphaprior", "mask_l1")
IMAGE_LOSSES = ("rgb_l2", "psnr", "rgb_l1_focus", "rgb_l1_phys", "pose_shadow_l2")


def patch_losses(registry_module=None, regularizers=False, images=False, perceptual=None, effnet=None,
                 perceptual_precision="fp32"):
    """Re-register the image losses of the reference's loss registry (ca_code/loss/registry.py:59-79; rgb_l1 and
    rgb_ssim, ca_code/loss/__init__.py:391-411, 478-494) with the fused HIP versions, so a `ModularLoss` built from the
    unchanged config picks them up.  Call after `import ca_code.loss` and before constructing the loss.
    regularizers=True also re-registers the per-Gaussian regularisers and their kin (REGULARIZER_LOSSES,
    ca_code/loss/__init__.py:450-453, 560-600, 609-622) with the gol_regloss_* / gol_backlit_* operators of
    goliath_amd.losses; images=True also re-registers the L2 / focus image losses (IMAGE_LOSSES,
    ca_code/loss/__init__.py:366-386, 415-445, 496-538, 555-557) with the gol_imgloss_* operators.  perceptual= a
    torchvision vgg19 state dict, the path of one or a goliath_amd.perceptual.Vgg19Features also re-registers `vgg`
    (ca_code/loss/perceptual.py:55-58) with goliath_amd.perceptual.VGGLoss over that network (gol_conv3_* where the layer's
    shape is in perceptual.DISPATCH); the weights come from the caller, nothing is downloaded, and the default (None)
    leaves `vgg` untouched; perceptual_precision="bf16x3" (opt-in, passed to perceptual.as_features) runs its wide layers on
    the split-bf16 operator gol_conv3x_* where perceptual.DISPATCH_BF16X3 admits the shape.  effnet= a torchvision efficientnet_b0 state dict, the path of one or a
    goliath_amd.effnet.EffNetB0Features also re-registers `effnet` and `effnet_phys` (ca_code/loss/perceptual.py:61-69; the
    latter with src_key="rendered_phys_rgb") with goliath_amd.effnet.EffNetLoss over ONE shared network
    (gol_mbconv_front_* where the block's shape is in effnet.DISPATCH), without importing ca_code.loss.effnet or
    torchvision; the default (None) leaves both untouched.  With perceptual= and effnet= given, every loss of the hand
    configs has an implementation here; every other entry of the registry stays the reference's."""
    from . import losses

    if registry_module is None:
        import ca_code.loss  # noqa: F401  (registers the reference's own functions first)
        import ca_code.loss.registry as registry_module

    def factory(fn):
        return lambda assets=None, **function_args: registry_module.FnLoss(fn, function_args)

    for name, fn in (("rgb_l1", losses.rgb_l1), ("rgb_ssim", losses.rgb_ssim)):
        registry_module.loss_registry[name] = factory(fn)
    if regularizers:
        for name in REGULARIZER_LOSSES:
            registry_module.loss_registry[name] = factory(getattr(losses, name))
    if images:
        for name in IMAGE_LOSSES:
            registry_module.loss_registry[name] = factory(getattr(losses, name))
    if perceptual is not None:
        from . import perceptual as perceptual_module

        features = perceptual_module.as_features(perceptual, perceptual_precision)
        registry_module.loss_registry["vgg"] = \
            lambda assets=None, **kwargs: perceptual_module.VGGLoss(assets, features=features, **kwargs)
    if effnet is not None:
        from . import effnet as effnet_module

        network = effnet_module.as_features(effnet)
        registry_module.loss_registry["effnet"] = \
            lambda assets=None, **kwargs: effnet_module.EffNetLoss(assets, features=network, **kwargs)
        registry_module.loss_registry["effnet_phys"] = \
            lambda assets=None, **kwargs: effnet_module.EffNetLoss(assets, features=network, src_key="rendered_phys_rgb",
                                                                   **kwargs)
    return registry_module


IMAGE_OP_MODULES = ("ca_code.models.urhand", "ca_code.models.mesh_vae", "ca_code.models.mesh_vae_drivable", "ca_code.loss")


def patch_image_ops(*modules):
    """Rebind the module-level names `depth_discontuity_mask` (ca_code/utils/geom.py:768-794, imported at urhand.py:31,
    mesh_vae.py:31 and mesh_vae_drivable.py:31) and `erode` (ca_code/utils/image.py:411-422, imported at
    ca_code/loss/__init__.py:31) to goliath_amd.imageops in the modules given (default: IMAGE_OP_MODULES, imported here),
    wherever a module carries the name; a module without it is left alone.  Returns the list of (module name, attribute) pairs that were rebound."""
    import importlib

    from . import imageops

    if not modules:
        modules = tuple(importlib.import_module(name) for name in IMAGE_OP_MODULES)
    done = []
    for mod in modules:
        for attr, fn in (("depth_discontuity_mask", imageops.depth_discontinuity_mask), ("erode", imageops.erode)):
            if hasattr(mod, attr):
                setattr(mod, attr, fn)
                done.append((getattr(mod, "__name__", repr(mod)), attr))
    return done


def patch_urhand(urhand_module=None, mesh_render_layer=False, uv_frames=False, texture_decoder=False, texture_tail=False,
                 displacement_unet=False, feat_encoder=False, feat_encoder_precision="fp32",
                 texture_decoder_precision="fp32"):
    """BASELINE config 4 as a drop-in: `ConvTeacherDecoder.forward` (ca_code/models/urhand.py:349-630) with its two light
    loops and both shadow-map evaluations on the HIP kernels (goliath_amd.urhand.conv_teacher_decoder_forward) and the
    stand-alone shadow-map lookup (`get_shadow_map`, imported at urhand.py:44).  The depth images of the light cameras are
    rendered by gol_mesh_raster from the topology (`vi`, `h`, `w`) of the layer the decoder built (`self.rl`,
    urhand.py:336-343) -- the layer object itself is never called.

    The module-level name `RenderLayer` (urhand.py:43) is LEFT ALONE by default: AutoEncoder.__init__ resolves the same name
    for the model's final, differentiable textured render (`self.renderer`, urhand.py:684, called with
    edge_grad=self.training) -- with drtk installed that stays drtk's.  mesh_render_layer=True rebinds it to
    goliath_amd.meshraster.RenderLayer (a stack without drtk): same constructor / forward / output dict, differentiable
    w.r.t. texture and vertices incl. an edge-gradient estimator (round 4) whose conventions are stated and checked against
    a supersampled render, not against drtk (absent: parity unpinned).

    uv_frames=True installs goliath_amd.urhand.conv_teacher_decoder_forward_uv_frames instead: the same forward with the TBN
    frames of both passes (urhand.py:366-392, :467-486), the two normal maps and the view conditioning (:573-578) on the
    fused operator of goliath_amd.uvframes (gol_uvframes_fwd / _bwd: no [B,S,S,3,3] image, no boolean-mask gather, no host
    sync).  Its topology is packed on first use from the decoder's `geo_fn` buffers (vi, vt, v2uv, index_image,
    face_index_image, bary_image) and cached on the decoder.  Opt-in: the default binding is unchanged.  What it gains
    against the lines it replaces, per batch size and direction, is measured by tools/uvframes_probe.py
    (profiles/uvframes_probe.json, DESIGN.md section 8 "uvframes"); a row in which the fused path is not faster beyond the
    parent's own run-to-run spread is named there.

    texture_decoder=True sets `texdec.TEXTURE_DECODER_FLAG` on the decoder class: either forward then runs its two texture
    branches (urhand.py:583-608) through goliath_amd.texdec.texture_branches, which hands a layer -- exact 2x bilinear
    resize + weight-normalised 3x3 convolution + bias / LeakyReLU or gate / gainbias -- to the fused operator
    (gol_upconv_fwd / _bwd: the upsampled tensor never exists in memory) where its shape is in texdec.DISPATCH, and runs
    the reference's three lines everywhere else (plain nn.Conv2d layers, CPU tensors, inputs that are not half the target
    size, shapes that lost the probe).  Opt-in: the default binding clears the flag and is unchanged.  The measured gain per
    layer shape is written by tools/texdec_probe.py to profiles/texdec_probe.json.
    texture_decoder_precision ("fp32" by default, or "bf16x3") is stored next to the flag as
    `texdec.TEXDEC_PRECISION_FLAG` and handed to texture_branches: at "bf16x3" a recognised layer whose shape passes
    texdec.supported_bf16x3 and is in texdec.DISPATCH_BF16X3 runs on the split-bf16 operator (gol_upconvx_*: the same
    fusion on three bf16 MFMAs per product; tools/texdecx_probe.py, profiles/texdecx_probe.json, DESIGN.md section
    6c-sexies); every other layer takes exactly the decision above.  It has no effect without texture_decoder=True; an
    unknown value raises ValueError.

    texture_tail=True rebinds `AutoEncoder.forward` (urhand.py:750-990) to goliath_amd.urhand.autoencoder_forward -- the same
    parameter list, the same `preds` keys -- and sets `uvtex.TEXTURE_TAIL_FLAG` on the class: the stretch from the decoder's
    relight_preds["tex"] to the RGBA textures the renderer takes (gain / bias, CalV5, clamp, seam resample, alpha packing,
    phys_tex packing, the two normal-colour textures: urhand.py:721-747, :788-790, :805-807, :824-832, :843-847) then runs
    on goliath_amd.uvtex (gol_uvtex_fwd / _bwd, gol_pack_rgba_*, gol_normal_rgba: one pass each way, no host sync per view,
    a deterministic seam backward).  The seam tap list is packed on first use from `seam_sampler.uvs` / `.weights` and
    cached on the sampler.  Opt-in: the default leaves `AutoEncoder.forward` untouched (and puts the original back after
    an earlier texture_tail=True).  Measured by tools/uvtex_probe.py (profiles/uvtex_probe.json, DESIGN.md section 8
    "uvtex").

    displacement_unet=True sets `dispunet.DISPLACEMENT_UNET_FLAG` on the decoder class: either forward then runs its
    displacement / roughness UNet (`self.geo_refiner`, urhand.py:461; DisplacementUNet.forward, :200-242) through
    goliath_amd.dispunet.forward, provided the refiner has `enc_layers`, `dec_layers` and `dec_layers_roughness` (any other
    refiner is called as a module, as today).  A decoder level -- LeakyReLU + exact 2x bilinear resize + concat with the
    skip + weight-normalised 3x3 convolution + untied bias, tanh and affine at the last level -- goes to the fused operator
    (gol_upcat_conv_fwd / _bwd: neither the upsampled nor the concatenated tensor exists in memory) where its shape is in
    dispunet.DISPATCH, and runs the reference's lines everywhere else.  Opt-in: the default binding clears the flag and is
    unchanged.  Measured per level and for the whole UNet by tools/dispunet_probe.py (profiles/dispunet_probe.json,
    DESIGN.md section 6c-bis).

    feat_encoder=True sets `featenc.FEATENC_FLAG` on the decoder class: either forward then runs its feature encoder
    (`self.featenc`, urhand.py:302; FeatEncoderUNet.forward, :98-107, called at :585 on `feat_p.detach()`) through
    goliath_amd.featenc.forward, provided it has `proj`, `feat_mod`, `gb_mod` and `enc` (any other encoder is called as a
    module, as today).  The 7x7 projection and the first 4x4 / stride 2 layer -- both weight-normalised, without bias --
    go to the fused operator (gol_featenc_front_fwd / _bwd: the 64-channel tensor between them and its gradient never
    exist in memory) where the shape is in featenc.DISPATCH, and run the reference's two lines everywhere else; every
    later layer runs as the reference's.  Opt-in: the default binding clears the flag and is unchanged.  Measured for the
    pair and for the whole encoder by tools/featenc_probe.py (profiles/featenc_probe.json).
    feat_encoder_precision ("fp32" by default, or "bf16x3") is stored next to the flag as
    `featenc.FEATENC_PRECISION_FLAG` and handed to featenc.forward: at "bf16x3" the bias-free 4x4 / stride 2 layers
    `feat_mod[0..3]` whose shape is in featenc.DISPATCH_BF16X3 run on the split-bf16 operator featenc.conv4s2
    (gol_conv4x_*: forward, input gradient and weight gradient; tools/conv4x_probe.py, profiles/conv4x_probe.json,
    DESIGN.md section 6c-quater).  It has no effect without feat_encoder=True; an unknown value raises ValueError.
    Returns the patched module."""
    from . import dispunet, featenc, meshraster, shadowmap, texdec, urhand, uvtex

    if urhand_module is None:
        import ca_code.models.urhand as urhand_module
    urhand_module.get_shadow_map = shadowmap.get_shadow_map
    if isinstance(mesh_render_layer, str) and mesh_render_layer == "fused":
        import warnings

        warnings.warn("patch_urhand(mesh_render_layer='fused'): the model's final, differentiable render goes through "
                      "goliath_amd.meshraster.FusedRenderLayer (RenderLayer's numbers on fused HIP kernels), whose edge "
                      "gradients are checked against finite differences only -- drtk is absent in this build, so their parity "
                      "with drtk.edge_grad_estimator is UNVERIFIED; meshraster.EDGE_STATS (opt-in: GOLIATH_EDGE_STATS=1) counts "
                      "the discontinuities that receive no gradient", RuntimeWarning, stacklevel=2)
        urhand_module.RenderLayer = meshraster.FusedRenderLayer
    elif mesh_render_layer:
        import warnings

        warnings.warn("patch_urhand(mesh_render_layer=True): the model's final, differentiable render goes through "
                      "goliath_amd.meshraster.RenderLayer, whose edge gradients are checked against finite differences only -- "
                      "drtk is absent in this build, so their parity with drtk.edge_grad_estimator is UNVERIFIED; "
                      "meshraster.EDGE_STATS (opt-in: GOLIATH_EDGE_STATS=1) counts the discontinuities that receive no gradient", RuntimeWarning, stacklevel=2)
        urhand_module.RenderLayer = meshraster.RenderLayer
    urhand_module.ConvTeacherDecoder.forward = (urhand.conv_teacher_decoder_forward_uv_frames if uv_frames
                                                else urhand.conv_teacher_decoder_forward)
    setattr(urhand_module.ConvTeacherDecoder, texdec.TEXTURE_DECODER_FLAG, bool(texture_decoder))
    setattr(urhand_module.ConvTeacherDecoder, texdec.TEXDEC_PRECISION_FLAG, texdec._precision(texture_decoder_precision))
    setattr(urhand_module.ConvTeacherDecoder, dispunet.DISPLACEMENT_UNET_FLAG, bool(displacement_unet))
    setattr(urhand_module.ConvTeacherDecoder, featenc.FEATENC_FLAG, bool(feat_encoder))
    setattr(urhand_module.ConvTeacherDecoder, featenc.FEATENC_PRECISION_FLAG, featenc._precision(feat_encoder_precision))
    ae = urhand_module.AutoEncoder if texture_tail else getattr(urhand_module, "AutoEncoder", None)
    if texture_tail:
        if "_gol_reference_forward" not in ae.__dict__:
            ae._gol_reference_forward = ae.__dict__["forward"]
        ae.forward = urhand.autoencoder_forward
        setattr(ae, uvtex.TEXTURE_TAIL_FLAG, True)
    elif ae is not None and "_gol_reference_forward" in ae.__dict__:   # undo an earlier texture_tail=True
        ae.forward = ae.__dict__["_gol_reference_forward"]
        del ae._gol_reference_forward
        setattr(ae, uvtex.TEXTURE_TAIL_FLAG, False)
    return urhand_module


def patch_hand_teacher(teacher_module=None, olat_fused=False, unet_precision="fp32"):
    """BASELINE config 5's teacher as a drop-in: `OLATRGBDecoder.forward_rgb` (ca_code/models/hand_teacher_mvp.py:253-494)
    with the per-light deep-shadow march on gol_mvp_shadow_march (goliath_amd.urhand.olat_rgb_decoder_forward_rgb).
    olat_fused=True binds urhand.olat_rgb_decoder_forward_rgb_fused instead: the UNet input and the OLAT sum on
    gol_olat_features_fwd / gol_olat_combine_fwd / _bwd as well (goliath_amd.olat); a later call with False restores the default.
    unet_precision ("fp32" by default, or "bf16x3") is stored on the class as `olatunet.UNET_PRECISION_FLAG` and handed to
    goliath_amd.olatunet.forward by the fused forward: at "bf16x3" a UNet level (:444-467: th.cat + Conv2dWNUB 3x3 + untied
    bias + LeakyReLU) whose shape is in olatunet.DISPATCH runs on the split-bf16 operator olatunet.conv3_ub_lrelu
    (gol_conv3ub_*: forward and the gradients to both inputs, the weight and the bias, without the concatenated tensor;
    tools/olatunet_probe.py, profiles/olatunet_probe.json).  It has no effect without
    olat_fused=True; an unknown value raises ValueError.
    The ordinary ray march of the model already runs on the HIP kernels through `install()` (mvpraymarchlib / utilslib)."""
    from . import olatunet, urhand

    unet_precision = olatunet._precision(unet_precision)
    if teacher_module is None:
        import ca_code.models.hand_teacher_mvp as teacher_module
    setattr(teacher_module.OLATRGBDecoder, olatunet.UNET_PRECISION_FLAG, unet_precision)
    teacher_module.OLATRGBDecoder.forward_rgb = (urhand.olat_rgb_decoder_forward_rgb_fused if olat_fused
                                                 else urhand.olat_rgb_decoder_forward_rgb)
    return teacher_module


def patch_hand_mvp(hand_mvp_module=None, full_template=False, fused_tail=False):
    """BASELINE config 5's student as a drop-in: `AutoEncoder.render` (ca_code/models/hand_mvp.py:162-205) assembles the
    compacted primitive template from the decoder slabs with ONE kernel (gol_mvp_template_fwd / _bwd; no full-K copy, no
    per-step nonzero, implicit pixel grid) and `GeomDecoder.forward` (:386-444) forms primpos / primrot / primscale with
    gol_mvp_primtransf_fwd / _bwd (goliath_amd.mvpprims.hand_mvp_render / geom_decoder_forward).  The march itself already
    runs on the HIP kernels.  preds["primrgba"] -- the full-K template only `HandMVPSummary` reads -- is NOT set unless
    full_template=True (then it is written from the same loads, at the price of one more template-sized store).
    fused_tail=True (opt-in; the default leaves everything above as it is): `GeomDecoder.forward` and
    `RGBSlabDecoder.forward` (:457-474) stop in front of their last ConvTranspose2dWNUB(16 -> TD C) and put a
    `mvptail.TailHandle` (activation + layer; `.materialize()` gives the slab) into preds["primalpha"] / ["primrgb"]; `render`
    hands the two to `mvptail.decode_template` (gol_mvp_tail_fwd / _bwd): last layer, bias, 25 x + 100, relu and template in
    one kernel, no [B,24,1024,1024] / [B,8,1024,1024] slab.  A decoder whose last layer is not the fusable one runs its own
    lines, and so does full_template=True.  A later call without fused_tail restores the default.  Returns the patched
    module."""
    from . import mvpprims, mvptail

    if hand_mvp_module is None:
        import ca_code.models.hand_mvp as hand_mvp_module
    setattr(hand_mvp_module.AutoEncoder, mvpprims.FULL_TEMPLATE_FLAG, bool(full_template))
    hand_mvp_module.AutoEncoder.render = mvpprims.hand_mvp_render
    hand_mvp_module.GeomDecoder.forward = mvpprims.geom_decoder_forward
    rgbdec = getattr(hand_mvp_module, "RGBSlabDecoder", None)
    if fused_tail:
        setattr(hand_mvp_module.GeomDecoder, mvptail.FUSED_TAIL_FLAG, True)
        if "_goliath_own_forward" not in vars(rgbdec):
            rgbdec._goliath_own_forward = rgbdec.forward
        rgbdec.forward = mvptail.rgb_decoder_forward
    else:   # the default touches nothing else; after a fused_tail=True call it puts the decoders back
        if mvptail.FUSED_TAIL_FLAG in vars(hand_mvp_module.GeomDecoder):
            setattr(hand_mvp_module.GeomDecoder, mvptail.FUSED_TAIL_FLAG, False)
        if rgbdec is not None and "_goliath_own_forward" in vars(rgbdec):
            rgbdec.forward = rgbdec._goliath_own_forward
    return hand_mvp_module
