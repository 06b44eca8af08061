"""Adam / AdamW with the gradient scrub and the global-norm clip fused in, on the HIP kernels of csrc/optim.hip.

    opt = goliath_amd.optim.Adam(params, lr=5e-4, max_norm=1.0, scrub_nonfinite=True)
    loss.backward(); opt.step()

replaces the tail of the reference's training iteration (ca_code/utils/train.py:209-215):

    for p in optim_params:
        p.grad.data[isnan(p.grad.data)] = 0      # a boolean-mask write: one host sync per tensor
        p.grad.data[isinf(p.grad.data)] = 0      # and another
    clip_grad_norm_(optim_params, 1.0)
    optimizer.step()                             # torch.optim.Adam / AdamW

`step()` reads the gradients once for the norm (gol_optim_grad_stats + gol_optim_finalize) and makes one pass over the
parameters, gradients and both moments (gol_optim_adam_step), all tensors at once.  No host sync and, after the first call,
no allocation: the step counters live on the device, so a whole step captures as a graph.  Without `max_norm` and
`scrub_nonfinite` it is a plain Adam step (one pass, no statistics).  `Adam` and `AdamW` take torch's constructor arguments,
and `state_dict()` / `load_state_dict()` are interchangeable with torch.optim.Adam / AdamW in both directions.  Every
parameter must be a contiguous float32 GPU tensor: there is no CPU path.  amsgrad, maximize, tensor learning rates and
closures are not supported and raise.  The norm counts a non-finite gradient entry as 0 (what the scrub makes of it).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GoliathHipError, c_double, c_int, stream_ptr

GROUP_DOUBLES = 8                        # GOL_OPTIM_GROUP_DOUBLES
SCRUB, CLIP, WRITE_BACK = 1, 2, 4        # GOL_OPTIM_*
_COEF = 8                                # floats of per-segment scratch (seg_coef)


def chunk_elems():
    """The kernels' compile-time chunk size, in elements."""
    return int(_lib.load().gol_optim_chunk_elems())


def chunk_tables(numels, chunk):
    """(chunk_seg int32[C], chunk_off int64[C]), CPU tensors: the chunks of `chunk` elements that tile segment 0, then
    segment 1, ... (segment s has numels[s] elements), in order, every element exactly once."""
    n = np.asarray(list(numels), dtype=np.int64)
    per = -(-n // int(chunk))
    seg = np.repeat(np.arange(n.size, dtype=np.int64), per)
    first = np.concatenate([np.zeros(1, np.int64), np.cumsum(per)])[:-1]
    off = (np.arange(seg.size, dtype=np.int64) - first[seg]) * int(chunk)
    return torch.from_numpy(seg.astype(np.int32)), torch.from_numpy(off)


# ---- one marshaller per C-ABI entry: keywords = the header's parameter names; a pointer is a GPU tensor (checked), a device
# address or None; stream = the current one -----------------------------------------------------------------------------------
_KINDS = {"f": torch.float32, "d": torch.float64, "n": torch.int32, "l": torch.int64}


def _marshal(entry, order, kw):
    """`order` = "name:kind ..." in the header's order: i = int, D = double, f / d / n / l = pointer to float32 / float64 /
    int32 / int64."""
    args = []
    for item in order.split():
        name, kind = item.split(":")
        x = kw[name]
        if kind == "i":
            args.append(c_int(x))
        elif kind == "D":
            args.append(c_double(x))
        else:
            args.append(ctypes.c_void_p(x) if x is None or isinstance(x, int) else _lib.ptr(x, _KINDS[kind], name))
    _lib.call(entry, *args, stream_ptr())


def _abi_optim_grad_stats(*, n_chunks, n_seg, chunk_seg, chunk_off, seg_g, seg_numel, partial):
    _marshal("gol_optim_grad_stats", "n_chunks:i n_seg:i chunk_seg:n chunk_off:l seg_g:l seg_numel:l partial:d", locals())


def _abi_optim_finalize(*, n_chunks, partial, max_norm, stats, nonfinite):
    _marshal("gol_optim_finalize", "n_chunks:i partial:d max_norm:D stats:d nonfinite:l", locals())


def _abi_optim_adam_step(*, n_chunks, n_seg, n_groups, chunk_seg, chunk_off, seg_p, seg_g, seg_m, seg_v, seg_step,
                         seg_numel, seg_group, groups, stats, seg_coef, flags):
    _marshal("gol_optim_adam_step", "n_chunks:i n_seg:i n_groups:i chunk_seg:n chunk_off:l seg_p:l seg_g:l seg_m:l seg_v:l "
             "seg_step:l seg_numel:l seg_group:n groups:d stats:d seg_coef:f flags:i", locals())


class _Tables:
    """What one `step()` hands to the kernels, for one set of tensor addresses."""
    __slots__ = ("key", "device", "n_chunks", "n_seg", "chunk_seg", "chunk_off", "seg", "seg_group", "partial", "seg_coef")


class Adam(torch.optim.Adam):
    """torch.optim.Adam's arguments plus, keyword-only: max_norm (None = no clipping; else the gradients are scaled by
    min(1, max_norm / (global norm + 1e-6)) as clip_grad_norm_ does), scrub_nonfinite (NaN and +-Inf gradient entries count
    and act as 0) and write_back_grads (store the scrubbed and clipped gradient into p.grad, as the reference's lines leave
    it; False saves the 4 bytes per parameter).  After a step with max_norm or scrub_nonfinite, `last_grad_norm` (float64),
    `last_clip_coef` (float64) and `last_nonfinite` (int64) are device scalars of that step; they are overwritten in place
    by the next one."""

    _DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 max_norm=None, scrub_nonfinite=False, write_back_grads=True):
        if amsgrad or maximize:
            raise GoliathHipError("goliath_amd.optim: amsgrad and maximize are not supported")
        if isinstance(lr, torch.Tensor):
            raise GoliathHipError("goliath_amd.optim: a tensor lr is not supported")
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError(f"max_norm must be positive or None, got {max_norm}")
        self.max_norm = None if max_norm is None else float(max_norm)
        self.scrub_nonfinite = bool(scrub_nonfinite)
        self.write_back_grads = bool(write_back_grads)
        self._tables = None
        self._steps = None            # float32[number of parameters] on the parameters' device: state[p]["step"] views it
        self._slot = {}               # parameter -> its index in _steps
        self._groups_dev = self._groups_key = None
        self._stats = self._nonfinite = None
        self.last_grad_norm = self.last_clip_coef = self.last_nonfinite = None
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                         foreach=None, capturable=False, differentiable=False, fused=None,
                         decoupled_weight_decay=self._DECOUPLED)

    @staticmethod
    def _check_param(p):
        if p.dtype != torch.float32:
            raise GoliathHipError(f"goliath_amd.optim: parameters must be float32, got {p.dtype}")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            self._check_param(p)
        self._tables = None

    # ---- step counters on the device ------------------------------------------------------------------------------------------
    def _all_params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _bind_steps(self):
        """One float32 counter per parameter in one device array; every existing state's `step` becomes a view of its
        slot (its value kept)."""
        params = self._all_params()
        if self._steps is not None and len(self._slot) == len(params) and all(p in self._slot for p in params):
            return
        dev = params[0].device
        steps = torch.zeros(len(params), dtype=torch.float32, device=dev)
        self._slot = {p: i for i, p in enumerate(params)}
        for p, i in self._slot.items():
            st = self.state.get(p)
            if st and "step" in st:
                steps[i] = torch.as_tensor(st["step"], dtype=torch.float32)
                st["step"] = steps[i]
        self._steps = steps

    def _adopt_state(self):
        """After the state was replaced from outside (load_state_dict): the step counters move into the device array."""
        self._steps, self._slot, self._tables = None, {}, None
        if self._all_params():
            self._bind_steps()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise GoliathHipError("goliath_amd.optim: the loaded param_groups ask for amsgrad or maximize")
        self._adopt_state()

    def state_dict(self):
        """torch.optim.Adam's layout: `step` is a float32 CPU scalar tensor per parameter (one device read for all)."""
        sd = super().state_dict()
        steps = None if self._steps is None else self._steps.detach().cpu()
        index = {}
        for group, packed in zip(self.param_groups, sd["param_groups"]):
            index.update({pid: p for pid, p in zip(packed["params"], group["params"])})
        state = {}
        for pid, st in sd["state"].items():
            st = dict(st)
            p = index.get(pid)
            if "step" in st and steps is not None and p in self._slot:
                st["step"] = steps[self._slot[p]].clone()
            state[pid] = st
        sd["state"] = state
        return sd

    # ---- tables ----------------------------------------------------------------------------------------------------------------
    def _segments(self):
        """[(parameter, group index)] of the parameters that have a gradient (and at least one element), in group order:
        the kernels' segments."""
        return [(p, gi) for gi, group in enumerate(self.param_groups) for p in group["params"]
                if p.grad is not None and p.numel() > 0]

    def _build_tables(self, segs, key):
        dev = segs[0][0].device
        for p, _ in segs:
            g = p.grad
            for label, x in (("a parameter", p), ("a gradient", g)):
                if not x.is_cuda:
                    raise GoliathHipError(f"goliath_amd.optim needs CUDA(HIP) tensors; there is no CPU path ({label} is on "
                                          f"{x.device})")
                if x.device != dev:
                    raise GoliathHipError(f"goliath_amd.optim: all parameters must be on one device ({dev}, {x.device})")
                if x.is_sparse or x.dtype != torch.float32 or not x.is_contiguous():
                    raise GoliathHipError(f"goliath_amd.optim: {label} is not a dense contiguous float32 tensor")
            if g.numel() != p.numel():
                raise GoliathHipError("goliath_amd.optim: a gradient's size differs from its parameter's")
        chunk = chunk_elems()                    # loads the library: GoliathHipError when it is not built
        self._bind_steps()
        rows = []
        for p, _ in segs:
            st = self.state[p]
            if len(st) == 0:                     # torch's lazy state initialisation
                st["step"] = self._steps[self._slot[p]]
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if not (m.is_contiguous() and v.is_contiguous() and m.dtype == v.dtype == torch.float32 and m.device == dev):
                raise GoliathHipError("goliath_amd.optim: exp_avg / exp_avg_sq must be contiguous float32 on the device")
            rows.append((p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), st["step"].data_ptr(), p.numel()))
        t = _Tables()
        t.key, t.device = key, dev
        chunk_seg, chunk_off = chunk_tables([r[5] for r in rows], chunk)
        t.n_seg, t.n_chunks = len(rows), chunk_seg.numel()
        t.chunk_seg, t.chunk_off = chunk_seg.to(dev), chunk_off.to(dev)
        t.seg = torch.tensor(rows, dtype=torch.int64).t().contiguous().to(dev)        # [6, n_seg]
        t.seg_group = torch.tensor([gi for _, gi in segs], dtype=torch.int32).to(dev)
        t.partial = torch.zeros(max(t.n_chunks, 1), 2, dtype=torch.float64, device=dev)
        t.seg_coef = torch.zeros(t.n_seg, _COEF, dtype=torch.float32, device=dev)
        if self._stats is None or self._stats.device != dev:
            self._stats = torch.zeros(2, dtype=torch.float64, device=dev)
            self._nonfinite = torch.zeros(1, dtype=torch.int64, device=dev)
            self.last_grad_norm, self.last_clip_coef = self._stats[0], self._stats[1]
            self.last_nonfinite = self._nonfinite[0]
        return t

    def _group_rows(self):
        rows = []
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise GoliathHipError("goliath_amd.optim: amsgrad and maximize are not supported")
            lr, (b1, b2) = group["lr"], group["betas"]
            if isinstance(lr, torch.Tensor) or isinstance(b1, torch.Tensor) or isinstance(b2, torch.Tensor):
                raise GoliathHipError("goliath_amd.optim: tensor hyper-parameters are not supported")
            rows.append((float(lr), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                         1.0 if group.get("decoupled_weight_decay") else 0.0, 0.0, 0.0))
        return tuple(rows)

    @staticmethod
    def _capturing():
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    @torch.no_grad()
    def step(self, closure=None):
        """Scrub, clip and step, for every parameter that has a gradient.  Returns None."""
        if closure is not None:
            raise GoliathHipError("goliath_amd.optim: step(closure) is not supported")
        segs = self._segments()
        if not segs:
            return None
        key = tuple((p.data_ptr(), p.grad.data_ptr()) for p, _ in segs)
        t = self._tables
        if t is None or t.key != key:
            if self._capturing():
                raise GoliathHipError("goliath_amd.optim: the set or the addresses of the parameter and gradient tensors "
                                      "changed; the tables cannot be rebuilt under stream capture (warm up one step and "
                                      "keep the gradient tensors: zero_grad(set_to_none=False))")
            t = self._tables = self._build_tables(segs, key)
        rows = self._group_rows()
        if rows != self._groups_key or self._groups_dev is None or self._groups_dev.device != t.device:
            if self._capturing():
                raise GoliathHipError("goliath_amd.optim: a hyper-parameter changed under stream capture")
            host = torch.tensor(rows, dtype=torch.float64).reshape(-1, GROUP_DOUBLES).pin_memory()
            if self._groups_dev is None or self._groups_dev.shape != host.shape or self._groups_dev.device != t.device:
                self._groups_dev = torch.empty(host.shape, dtype=torch.float64, device=t.device)
            self._groups_dev.copy_(host, non_blocking=True)
            self._groups_key = rows
        stats = self.max_norm is not None or self.scrub_nonfinite
        flags = (SCRUB if self.scrub_nonfinite else 0) | (CLIP if self.max_norm is not None else 0) | \
                (WRITE_BACK if self.write_back_grads and stats else 0)
        seg = t.seg.data_ptr()
        row = lambda i: seg + 8 * i * t.n_seg
        with _lib.device_guard(t.device):
            if stats:
                _abi_optim_grad_stats(n_chunks=t.n_chunks, n_seg=t.n_seg, chunk_seg=t.chunk_seg, chunk_off=t.chunk_off,
                                      seg_g=row(1), seg_numel=row(5), partial=t.partial)
                _abi_optim_finalize(n_chunks=t.n_chunks, partial=t.partial,
                                    max_norm=float("inf") if self.max_norm is None else self.max_norm, stats=self._stats,
                                    nonfinite=self._nonfinite)
            _abi_optim_adam_step(n_chunks=t.n_chunks, n_seg=t.n_seg, n_groups=len(rows), chunk_seg=t.chunk_seg,
                                 chunk_off=t.chunk_off, seg_p=row(0), seg_g=row(1), seg_m=row(2), seg_v=row(3),
                                 seg_step=row(4), seg_numel=row(5), seg_group=t.seg_group, groups=self._groups_dev,
                                 stats=self._stats if stats else None, seg_coef=t.seg_coef, flags=flags)
        return None


class AdamW(Adam):
    """torch.optim.AdamW's arguments (decoupled weight decay, 0.01 by default) plus the three of `Adam`."""

    _DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_norm=None, scrub_nonfinite=False, write_back_grads=True):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         max_norm=max_norm, scrub_nonfinite=scrub_nonfinite, write_back_grads=write_back_grads)
