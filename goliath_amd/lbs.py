"""Skeleton solve and linear blend skinning on the HIP kernels of csrc/lbs.hip, with gradients.

    Skeleton(...) / Skeleton.from_module(lbs_fn)   the constants, packed once (the only place that syncs the host)
    skeleton_states(skel, poses, scales)           LinearBlendSkinning.compute_rigid_transforms   (lbs.py:151-159) [B,J,8]
    rigid_transforms(skel, poses, scales)          .compute_rigid_transforms_matrix               (lbs.py:161-169) [B,J,3,4]
    pose_vertices(skel, poses, scales, verts_unposed=None, template=None, global_scaling=None, rest_vertices=None)
                                                   LinearBlendSkinning.forward (lbs.py:308-337) between the two elementwise
                                                   lines of LBSModule.pose (lbs.py:725-731)                        [B,V,3]

The reference walks the kinematic chain in a Python loop that reads every joint's parent index from the device (one host
sync per joint) and launches about a dozen small kernels per joint.  Here the forward is two launches and the backward at
most four, on the current stream, without host sync or atomics: a step through them captures as a graph and is bitwise
reproducible.  `poses` is [B,NP] (global and local pose concatenated), `scales` [B,NS] or one row [1,NS] for all views.
Every tensor must be on the GPU: there is no CPU path.
"""
import ctypes

import torch

from . import _lib
from ._lib import c_int, stream_ptr

_F32, _F64, _I32 = torch.float32, torch.float64, torch.int32
ITEM_ENTRIES = 64   # a joint's (vertex, slot) run is reduced in work items of at most this many entries (csrc/lbs.hip)


def _csr(keys, n):
    start = torch.zeros(n + 1, dtype=torch.long, device=keys.device)
    start[1:] = torch.bincount(keys, minlength=n).cumsum(0)
    return start, torch.argsort(keys, stable=True)


class Skeleton:
    """The constant part of the skeleton solve and the skinning, packed for the kernels on one device.

    joint_parents[J] or [J,1] (-1 = root; a parent's index must be smaller than its child's, as the reference's loop
    assumes: ValueError otherwise), joint_offset[J,3], joint_rotation[J,4] (xyzw), bind_state[1,J,8] or [J,8],
    skin_indices / skin_weights [V,K], mesh_vertices[V,3], transform[7J,P], transform_offsets[1,7J] or [7J].
    Attributes (see include/goliath_hip.h): parents, level_start, level_joints, child_start, child_slot, bind_inv,
    transform, transform_t, transform_offsets, joint_offset, joint_rotation, skin_indices, skin_weights, mesh_vertices,
    jv_start, jv_slot, item_start, ji_start; sizes J, V, K, P, L (levels), E (non-zero weights), I (items)."""

    _TENSORS = ("parents", "level_start", "level_joints", "child_start", "child_slot", "bind_inv", "transform",
                "transform_t", "transform_offsets", "joint_offset", "joint_rotation", "skin_indices", "skin_weights",
                "mesh_vertices", "jv_start", "jv_slot", "item_start", "ji_start")

    def __init__(self, joint_parents, joint_offset, joint_rotation, bind_state, skin_indices, skin_weights, mesh_vertices,
                 transform, transform_offsets):
        dev = joint_offset.device
        parents = joint_parents.to(dev).reshape(-1).long()
        J = parents.numel()
        if J < 1 or tuple(joint_offset.shape) != (J, 3) or tuple(joint_rotation.shape) != (J, 4):
            raise ValueError(f"joint_offset must be [{J},3] and joint_rotation [{J},4]")
        if bind_state.numel() != J * 8:
            raise ValueError(f"bind_state must hold [{J},8] numbers, got {tuple(bind_state.shape)}")
        if transform.dim() != 2 or transform.shape[0] != 7 * J or transform_offsets.numel() != 7 * J:
            raise ValueError(f"transform must be [{7 * J},P] and transform_offsets hold {7 * J} numbers")
        if skin_indices.dim() != 2 or skin_indices.shape != skin_weights.shape or \
                tuple(mesh_vertices.shape) != (skin_indices.shape[0], 3):
            raise ValueError("skin_indices and skin_weights must be [V,K] and mesh_vertices [V,3]")
        ids = torch.arange(J, device=dev)
        if bool(((parents >= ids) | (parents < -1)).any()):
            raise ValueError("joint_parents: a parent's index must be smaller than its child's (-1 = root)")
        idx = skin_indices.to(dev).long()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= J):
            raise ValueError(f"skin_indices must lie in [0, {J})")
        # tree levels (roots = 0): parents come first, so one ascending pass settles every depth
        plist = parents.tolist()
        depth = [0] * J
        for j, p in enumerate(plist):
            depth[j] = depth[p] + 1 if p >= 0 else 0
        depth = torch.tensor(depth, dtype=torch.long, device=dev)
        level_start, level_joints = _csr(depth, int(depth.max()) + 1)
        has_parent = (parents >= 0).nonzero().flatten()
        child_start, order = _csr(parents[has_parent], J)
        child_slot = has_parent[order]
        # bind inverse (lbs.py:392-394) in double from the float32 bind state
        bind = bind_state.to(dev).reshape(J, 8).to(_F64)
        q = bind[:, 3:7]
        br = q * q.new_tensor([-1.0, -1.0, -1.0, 1.0]) / (q * q).sum(-1, keepdim=True)
        bs = bind[:, 7:].reciprocal()
        a, v = br[:, :3], -bind[:, :3]
        av = torch.linalg.cross(a, v)
        bt = (v + 2.0 * (av * br[:, 3:] + torch.linalg.cross(a, av))) * bs
        # joint -> (vertex, slot) of the non-zero weights, every joint's run cut into items
        V, K = idx.shape
        w = skin_weights.to(dev).to(_F32)
        used = (w.reshape(-1) != 0).nonzero().flatten()                       # ascending slots
        jv_start, order = _csr(idx.reshape(-1)[used], J)
        jv_slot = used[order]
        counts = jv_start[1:] - jv_start[:-1]
        n_items = (counts + ITEM_ENTRIES - 1) // ITEM_ENTRIES
        ji_start = torch.zeros(J + 1, dtype=torch.long, device=dev)
        ji_start[1:] = n_items.cumsum(0)
        item_joint = torch.repeat_interleave(ids, n_items)
        I = item_joint.numel()
        item_start = torch.empty(I + 1, dtype=torch.long, device=dev)
        item_start[:I] = jv_start[item_joint] + ITEM_ENTRIES * (torch.arange(I, device=dev) - ji_start[item_joint])
        item_start[I] = used.numel()
        t = transform.to(dev).to(_F32)
        self.J, self.V, self.K, self.P = J, V, K, t.shape[1]
        self.L, self.E, self.I = level_start.numel() - 1, used.numel(), I
        self.parents = parents.to(_I32)
        self.level_start, self.level_joints = level_start.to(_I32), level_joints.to(_I32)
        self.child_start, self.child_slot = child_start.to(_I32), child_slot.to(_I32)
        self.bind_inv = torch.cat([bt, br, bs], -1).contiguous()
        self.transform, self.transform_t = t.contiguous(), t.t().contiguous()
        self.transform_offsets = transform_offsets.to(dev).to(_F32).reshape(-1).contiguous()
        self.joint_offset = joint_offset.to(_F32).contiguous()
        self.joint_rotation = joint_rotation.to(dev).to(_F32).contiguous()
        self.skin_indices, self.skin_weights = idx.to(_I32).contiguous(), w.contiguous()
        self.mesh_vertices = mesh_vertices.to(dev).to(_F32).contiguous()
        self.jv_start, self.jv_slot = jv_start.to(_I32), jv_slot.to(_I32)
        self.item_start, self.ji_start = item_start.to(_I32), ji_start.to(_I32)
        self.device = dev

    SOURCES = ("joint_parents", "joint_offset", "joint_rotation", "bind_state", "skin_indices", "skin_weights",
               "mesh_vertices")

    @classmethod
    def from_module(cls, lbs_fn):
        """From a `LinearBlendSkinning`-shaped object: the buffers named in SOURCES plus `param_transform.transform` and
        `param_transform.transform_offsets`."""
        pt = lbs_fn.param_transform
        return cls(*(getattr(lbs_fn, k) for k in cls.SOURCES), pt.transform, pt.transform_offsets)

    def to(self, device):
        device = torch.device(device)
        if device == self.device:
            return self
        new = object.__new__(Skeleton)
        new.__dict__.update(self.__dict__)
        for name in self._TENSORS:
            setattr(new, name, getattr(self, name).to(device))
        new.device = new.parents.device
        return new


# ---- one marshaller per C-ABI entry: keywords = the header's parameter names; a pointer is a GPU tensor (checked), a
# device address or None; stream = the current one ------------------------------------------------------------------------
def _p(x, dtype, name):
    return ctypes.c_void_p(x) if x is None or isinstance(x, int) else _lib.ptr(x, dtype, name)


def _marshal(entry, order, kw):
    """Call `entry` with the header's parameters: `order` = "name:kind ..." in the header's order, kind i = int, f / d / n =
    pointer to float32 / float64 / int32.  A wrong dtype or a non-contiguous tensor is reported under its parameter name."""
    kinds = {"f": _F32, "d": _F64, "n": _I32}
    args = []
    for item in order.split():
        name, kind = item.split(":")
        args.append(c_int(kw[name]) if kind == "i" else _p(kw[name], kinds[kind], name))
    _lib.call(entry, *args, stream_ptr())


_CHAIN = ("B:i J:i NP:i NS:i L:i poses:f scales:f scales_stride:i {}transform_t:f transform_offsets:f joint_offset:f "
          "joint_rotation:f bind_inv:d parents:n level_start:n level_joints:n ")
_SKIN = "mats:f verts:f verts_batched:i template_verts:f global_scaling:f skin_indices:n skin_weights:f "


def _abi_lbs_skeleton_fwd(*, B, J, NP, NS, L, poses, scales, scales_stride, transform_t, transform_offsets, joint_offset,
                          joint_rotation, bind_inv, parents, level_start, level_joints, states, mats):
    _marshal("gol_lbs_skeleton_fwd", _CHAIN.format("") + "states:f mats:f", locals())


def _abi_lbs_skeleton_bwd(*, B, J, NP, NS, L, poses, scales, scales_stride, transform, transform_t, transform_offsets,
                          joint_offset, joint_rotation, bind_inv, parents, level_start, level_joints, child_start,
                          child_slot, g_states, g_mats, g_poses, g_scales):
    _marshal("gol_lbs_skeleton_bwd", _CHAIN.format("transform:f ") + "child_start:n child_slot:n g_states:f g_mats:f "
             "g_poses:f g_scales:f", locals())


def _abi_lbs_skin_fwd(*, B, V, J, K, mats, verts, verts_batched, template_verts, global_scaling, skin_indices,
                      skin_weights, out):
    _marshal("gol_lbs_skin_fwd", "B:i V:i J:i K:i " + _SKIN + "out:f", locals())


def _abi_lbs_skin_bwd(*, B, V, J, K, E, I, mats, verts, verts_batched, template_verts, global_scaling, skin_indices,
                      skin_weights, item_start, jv_slot, ji_start, g_out, item_sums, g_verts, g_mats):
    _marshal("gol_lbs_skin_bwd", "B:i V:i J:i K:i E:i I:i " + _SKIN + "item_start:n jv_slot:n ji_start:n g_out:f "
             "item_sums:d g_verts:f g_mats:f", locals())


def _f32(t):
    return None if t is None else t.detach().to(_F32).contiguous()


def _saved(ctx):
    """The saved tensors; a second backward (buffers freed) raises RuntimeError, as for any autograd node."""
    return ctx.saved_tensors


def _skeleton_kw(skel, poses, scales):
    """The keywords both skeleton entries share.  scales: [B,NS], or one row for all views (stride 0)."""
    B, NP = poses.shape
    return dict(B=B, J=skel.J, NP=NP, NS=scales.shape[1], L=skel.L, poses=poses, scales=scales,
                scales_stride=scales.shape[1] if scales.shape[0] == B and B > 1 else 0, transform_t=skel.transform_t,
                transform_offsets=skel.transform_offsets, joint_offset=skel.joint_offset,
                joint_rotation=skel.joint_rotation, bind_inv=skel.bind_inv, parents=skel.parents,
                level_start=skel.level_start, level_joints=skel.level_joints)


def _scales_rows(scales):
    """scales as the kernels read it: one contiguous float32 row when every view has the same (a [1,NS] tensor or its
    expansion), [B,NS] otherwise."""
    s = scales.detach()
    if s.shape[0] > 1 and s.stride(0) == 0:
        s = s[:1]
    return s.to(_F32).contiguous()


def _skeleton_bwd(skel, poses, scales, n_views, g_states, g_mats, need_poses, need_scales):
    """(g_poses[B,NP] or None, g_scales in the shape of the caller's `scales` or None)."""
    B, NP = poses.shape
    NS = scales.shape[1]
    g_poses = torch.empty(B, NP, dtype=_F32, device=poses.device) if need_poses and NP else None
    g_scales = torch.empty(B, NS, dtype=_F32, device=poses.device) if need_scales and NS else None
    if g_poses is not None or g_scales is not None:
        _abi_lbs_skeleton_bwd(**_skeleton_kw(skel, poses, scales), transform=skel.transform, child_start=skel.child_start,
                              child_slot=skel.child_slot, g_states=g_states, g_mats=g_mats, g_poses=g_poses,
                              g_scales=g_scales)
    if need_poses and g_poses is None:
        g_poses = poses.new_zeros(B, 0)
    if need_scales and g_scales is None:
        g_scales = poses.new_zeros(B, 0)
    if g_scales is not None and n_views == 1 and B > 1:
        g_scales = g_scales.sum(0, keepdim=True)          # one [1,NS] row served every view
    return g_poses, g_scales


class _Skeleton(torch.autograd.Function):
    """which = "states" -> [B,J,8]; "mats" -> [B,J,3,4]."""

    @staticmethod
    def forward(ctx, poses, scales, skel, which):
        p, s = _f32(poses), _scales_rows(scales)
        B = p.shape[0]
        out = torch.empty((B, skel.J, 8) if which == "states" else (B, skel.J, 3, 4), dtype=_F32, device=p.device)
        with _lib.device_guard(p.device):
            _abi_lbs_skeleton_fwd(**_skeleton_kw(skel, p, s), states=out if which == "states" else None,
                                  mats=out if which == "mats" else None)
        ctx.save_for_backward(p, s)
        ctx.skel, ctx.which, ctx.dtypes, ctx.n_views = skel, which, (poses.dtype, scales.dtype), scales.shape[0]
        return out.to(poses.dtype)

    @staticmethod
    def backward(ctx, g_out):
        p, s = _saved(ctx)
        g = _f32(g_out)
        with _lib.device_guard(p.device):
            g_poses, g_scales = _skeleton_bwd(ctx.skel, p, s, ctx.n_views, g if ctx.which == "states" else None,
                                              g if ctx.which == "mats" else None, ctx.needs_input_grad[0],
                                              ctx.needs_input_grad[1])
        return (None if g_poses is None else g_poses.to(ctx.dtypes[0]),
                None if g_scales is None else g_scales.to(ctx.dtypes[1]), None, None)


class _PoseVertices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, poses, scales, verts_unposed, skel, template, global_scaling, rest_vertices):
        p, s = _f32(poses), _scales_rows(scales)
        B = p.shape[0]
        batched = verts_unposed is not None
        verts = _f32(verts_unposed) if batched else rest_vertices
        mats = torch.empty(B, skel.J, 3, 4, dtype=_F32, device=p.device)
        out = torch.empty(B, skel.V, 3, dtype=_F32, device=p.device)
        with _lib.device_guard(p.device):
            _abi_lbs_skeleton_fwd(**_skeleton_kw(skel, p, s), states=None, mats=mats)
            _abi_lbs_skin_fwd(B=B, V=skel.V, J=skel.J, K=skel.K, mats=mats, verts=verts, verts_batched=int(batched),
                              template_verts=template, global_scaling=global_scaling, skin_indices=skel.skin_indices,
                              skin_weights=skel.skin_weights, out=out)
        ctx.save_for_backward(p, s, mats, verts, *(t for t in (template, global_scaling) if t is not None))
        ctx.skel, ctx.batched, ctx.has = skel, batched, (template is not None, global_scaling is not None)
        ctx.dtypes = (poses.dtype, scales.dtype, verts_unposed.dtype if batched else None)
        ctx.n_views = scales.shape[0]
        return out.to(poses.dtype)

    @staticmethod
    def backward(ctx, g_out):
        p, s, mats, verts, *rest = _saved(ctx)
        rest = list(rest)
        template = rest.pop(0) if ctx.has[0] else None
        global_scaling = rest.pop(0) if ctx.has[1] else None
        skel = ctx.skel
        B = p.shape[0]
        need_p, need_s, need_v = ctx.needs_input_grad[:3]
        need_v = need_v and ctx.batched
        need_m = (need_p and p.shape[1] > 0) or (need_s and s.shape[1] > 0)
        g_verts = torch.empty(B, skel.V, 3, dtype=_F32, device=p.device) if need_v else None
        g_mats = torch.empty(B, skel.J, 3, 4, dtype=_F32, device=p.device) if need_m else None
        g_poses = g_scales = None
        with _lib.device_guard(p.device):
            if need_v or need_m:
                item_sums = torch.empty(B, max(skel.I, 1), 12, dtype=_F64, device=p.device) if need_m else None
                _abi_lbs_skin_bwd(B=B, V=skel.V, J=skel.J, K=skel.K, E=skel.E, I=skel.I, mats=mats, verts=verts,
                                  verts_batched=int(ctx.batched), template_verts=template, global_scaling=global_scaling,
                                  skin_indices=skel.skin_indices, skin_weights=skel.skin_weights,
                                  item_start=skel.item_start, jv_slot=skel.jv_slot, ji_start=skel.ji_start,
                                  g_out=_f32(g_out), item_sums=item_sums, g_verts=g_verts, g_mats=g_mats)
            if need_p or need_s:
                g_poses, g_scales = _skeleton_bwd(skel, p, s, ctx.n_views, None, g_mats, need_p, need_s)
        return (None if g_poses is None else g_poses.to(ctx.dtypes[0]),
                None if g_scales is None else g_scales.to(ctx.dtypes[1]),
                None if g_verts is None else g_verts.to(ctx.dtypes[2]), None, None, None, None)


def _check(name, skel, poses, scales):
    if not isinstance(skel, Skeleton):
        raise TypeError(f"{name}: skel must be a Skeleton")
    for label, x in (("poses", poses), ("scales", scales)):
        if not x.is_cuda:
            raise _lib.GoliathHipError(f"{name} needs CUDA(HIP) tensors; there is no CPU path ({label} is on {x.device})")
        if x.device != skel.device:
            raise _lib.GoliathHipError(f"{name}: the skeleton is on {skel.device}, {label} on {x.device} (use skel.to())")
    B = poses.shape[0] if poses.dim() == 2 else 0
    if B < 1 or scales.dim() != 2 or scales.shape[0] not in (1, B) or poses.shape[1] + scales.shape[1] != skel.P:
        raise _lib.GoliathHipError(f"{name}: expected poses [B,NP] and scales [B or 1,NS] with NP + NS = {skel.P}, got "
                                   f"{tuple(poses.shape)} and {tuple(scales.shape)}")


def skeleton_states(skel, poses, scales):
    """poses[B,NP], scales[B or 1,NS] -> skeleton states [B,J,8] (translation, rotation xyzw, scale): the reference's
    solve_skeleton_state(param_transform(cat(poses, scales)), ...) (lbs.py:340-385)."""
    _check("skeleton_states", skel, poses, scales)
    return _Skeleton.apply(poses, scales, skel, "states")


def rigid_transforms(skel, poses, scales):
    """poses[B,NP], scales[B or 1,NS] -> [B,J,3,4]: states_to_matrix(bind_state, states) (lbs.py:161-169, 388-429)."""
    _check("rigid_transforms", skel, poses, scales)
    return _Skeleton.apply(poses, scales, skel, "mats")


def pose_vertices(skel, poses, scales, verts_unposed=None, template=None, global_scaling=None, rest_vertices=None):
    """-> posed vertices [B,V,3] = skinning(verts_unposed + template) * global_scaling (lbs.py:308-337, 725-731).
    verts_unposed[B,V,3]: None = one mesh for every view (lbs.py:331-334): rest_vertices[V,3], by default the skeleton's
    rest mesh.  template[V,3], global_scaling[3] and rest_vertices are constants (no gradient) and may be None.  Gradients
    go to poses, scales and verts_unposed."""
    _check("pose_vertices", skel, poses, scales)
    B = poses.shape[0]
    if verts_unposed is not None and (not verts_unposed.is_cuda or tuple(verts_unposed.shape) != (B, skel.V, 3)):
        raise _lib.GoliathHipError(f"pose_vertices: verts_unposed must be a CUDA tensor [{B},{skel.V},3], got "
                                   f"{tuple(verts_unposed.shape)} on {verts_unposed.device}")
    if template is not None:
        template = _f32(template).expand(skel.V, 3).contiguous()
    if global_scaling is not None:
        global_scaling = _f32(global_scaling).reshape(-1).expand(3).contiguous()
    rest = skel.mesh_vertices if rest_vertices is None else _f32(rest_vertices).expand(skel.V, 3).contiguous()
    return _PoseVertices.apply(poses, scales, verts_unposed, skel, template, global_scaling, rest)


# ---- binding to LinearBlendSkinning / LBSModule-shaped objects (dropin.patch_lbs) ------------------------------------------
def skeleton_of(lbs_fn):
    """The packed skeleton of a module that owns the reference's buffers, built on first use, cached on the module,
    rebuilt when a buffer's device, shape or storage changes."""
    pt = lbs_fn.param_transform
    bufs = tuple(getattr(lbs_fn, k) for k in Skeleton.SOURCES) + (pt.transform, pt.transform_offsets)
    key = tuple((b.device, tuple(b.shape), b.data_ptr(), b._version) for b in bufs)
    cached = lbs_fn.__dict__.get("_gol_skeleton")
    if cached is None or cached[0] != key:
        cached = (key, Skeleton(*bufs))
        lbs_fn.__dict__["_gol_skeleton"] = cached
    return cached[1]


def lbs_forward(self, poses, scales, verts_unposed=None):
    """LinearBlendSkinning.forward (lbs.py:308-337)."""
    return pose_vertices(skeleton_of(self), poses, scales, verts_unposed)


def lbs_compute_rigid_transforms(self, global_pose, local_pose, scale):
    """LinearBlendSkinning.compute_rigid_transforms (lbs.py:151-159)."""
    return skeleton_states(skeleton_of(self), torch.cat([global_pose, local_pose], -1), scale)


def lbs_compute_rigid_transforms_matrix(self, global_pose, local_pose, scale):
    """LinearBlendSkinning.compute_rigid_transforms_matrix (lbs.py:161-169)."""
    return rigid_transforms(skeleton_of(self), torch.cat([global_pose, local_pose], -1), scale)


def lbs_module_pose(self, verts_unposed, motion, template=None):
    """LBSModule.pose (lbs.py:725-731): the template add and the global scaling fused into the skinning."""
    template = self.lbs_template_verts if template is None else template
    if template.dim() != 2:                                  # a template per view: not a constant of the kernel
        verts_unposed, template = verts_unposed + template, None
    return pose_vertices(skeleton_of(self.lbs_fn), motion, self.lbs_scale, verts_unposed, template, self.global_scaling)


def lbs_module_template_pose(self, motion):
    """LBSModule.template_pose (lbs.py:741-745): the template, shared by the views, in the rest mesh's place."""
    return pose_vertices(skeleton_of(self.lbs_fn), motion, self.lbs_scale, None, None, self.global_scaling,
                         rest_vertices=self.lbs_template_verts)
