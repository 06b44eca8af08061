"""CPU: the host side of goliath_amd/optim.py -- the chunk and segment tables, the C-ABI marshallers against the header,
state_dict interchange with torch.optim.Adam / AdamW, the loud errors, and, where the reference tree exists, the reference's
own `build_optimizer` instantiating the class from a `per_module` config."""
import copy
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
from test_lbs_host import needs_ref  # noqa: E402  (skips where the reference tree is absent)


def _chunk():
    from goliath_amd import build, optim

    build.build()
    return optim.chunk_elems()


def test_chunk_size_is_a_whole_number_of_16_byte_accesses_per_workgroup():
    chunk = _chunk()
    assert chunk > 0 and chunk % (256 * 4) == 0 and chunk <= 32 * 1024


def test_chunk_tables_tile_every_segment_once_in_order():
    from goliath_amd import optim

    chunk = _chunk()
    numels = [1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
    seg, off = optim.chunk_tables(numels, chunk)
    assert seg.dtype == torch.int32 and off.dtype == torch.int64 and seg.shape == off.shape and seg.dim() == 1
    seg, off = seg.tolist(), off.tolist()
    assert seg == sorted(seg) and sorted(set(seg)) == list(range(len(numels)))
    for s, n in enumerate(numels):
        offs = [o for c, o in zip(seg, off) if c == s]
        assert offs == list(range(0, n, chunk)), (s, n, offs)          # in order, no gap, no overlap, nothing past the end
    assert len(seg) == sum(-(-n // chunk) for n in numels)
    # 64-bit offsets: a tensor past 2^31 elements (tables only; nothing of that size is allocated)
    big = (1 << 31) + 5
    seg, off = optim.chunk_tables([3, big], chunk)
    assert off.dtype == torch.int64 and int(off[-1]) == (big - 1) // chunk * chunk > (1 << 31) - 1
    assert seg.numel() == 1 + -(-big // chunk) and int(seg[-1]) == 1
    # an empty list and an empty tensor make no chunk
    assert optim.chunk_tables([], chunk)[0].numel() == 0 and optim.chunk_tables([0, 5], chunk)[0].tolist() == [1]


def test_a_parameter_without_a_gradient_is_no_segment():
    from goliath_amd import optim

    a, b, c, e = (torch.nn.Parameter(torch.zeros(n)) for n in (5, 7, 9, 0))
    opt = optim.Adam([{"params": [a, b], "lr": 5e-4}, {"params": [c, e], "lr": 1e-3}])
    assert opt._segments() == []
    a.grad, c.grad, e.grad = torch.zeros(5), torch.zeros(9), torch.zeros(0)
    segs = opt._segments()
    assert [(id(p), gi) for p, gi in segs] == [(id(a), 0), (id(c), 1)]      # b: no gradient; e: no element


def _header():
    hdr = open(os.path.join(ROOT, "include", "goliath_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


@pytest.mark.parametrize("entry", ["gol_optim_grad_stats", "gol_optim_finalize", "gol_optim_adam_step"])
def test_optim_marshallers_follow_the_header(entry, monkeypatch):
    """The marshaller of an entry passes exactly the parameters goliath_hip.h declares, in its order and with its C types
    (the library sets no argtypes: a miscounted or swapped list would reach a kernel as a garbage pointer)."""
    from goliath_amd import _lib, optim

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(optim, "_abi_" + entry[len("gol_"):])
    sig = inspect.signature(fn).parameters
    assert set(sig) == {n for _, n in params} - {"stream"}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in sig.values())
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1), "float": (ctypes.c_float, i + 0.5),
                      "double": (ctypes.c_double, i + 0.25)}[ctype]
        if name == "stream":
            v = 0xBEEF
        else:
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(optim, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


def test_header_constants_match_the_module():
    from goliath_amd import optim

    defs = dict(re.findall(r"#define\s+(GOL_OPTIM_\w+)\s+(\d+)", _header()))
    assert {k: int(v) for k, v in defs.items()} == {
        "GOL_OPTIM_GROUP_DOUBLES": optim.GROUP_DOUBLES, "GOL_OPTIM_SCRUB": optim.SCRUB, "GOL_OPTIM_CLIP": optim.CLIP,
        "GOL_OPTIM_WRITE_BACK": optim.WRITE_BACK}


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in ((5,), (3, 2), (4,))]


def _groups(ps):
    return [{"params": ps[:1], "lr": 5e-4}, {"params": ps[1:], "lr": 1e-3}]


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_state_dict_round_trip_with_torch(name):
    """Keys and group keys equal torch's; a torch checkpoint loads into ours and ours into torch (CPU state tensors, no
    step of ours is taken; the last parameter never has a gradient, so it has no state on either side)."""
    from goliath_amd import optim

    ours_cls, torch_cls = getattr(optim, name), getattr(torch.optim, name)
    ps = _params()
    ref = torch_cls(_groups(ps), betas=(0.8, 0.99), eps=1e-7, weight_decay=0.02)
    for _ in range(3):
        for p in ps[:2]:
            p.grad = torch.randn_like(p)
        ref.step()
    want = ref.state_dict()
    ours = ours_cls(_groups(ps), max_norm=1.0, scrub_nonfinite=True)
    assert ours.state_dict()["state"] == {}
    assert [set(g) for g in ours.state_dict()["param_groups"]] == [set(g) for g in want["param_groups"]]
    assert set(ours.defaults) == set(ref.defaults)
    ours.load_state_dict(want)
    got = ours.state_dict()
    assert got["param_groups"] == want["param_groups"]
    assert set(got["state"]) == set(want["state"]) == {0, 1}
    for pid, st in want["state"].items():
        assert set(got["state"][pid]) == set(st) == {"step", "exp_avg", "exp_avg_sq"}
        for k, v in st.items():
            g = got["state"][pid][k]
            assert g.dtype == v.dtype and g.device == v.device and g.shape == v.shape and torch.equal(g, v), (pid, k)
    assert float(got["state"][0]["step"]) == 3.0
    # ... and back into a fresh torch optimizer, which then steps exactly as the original does
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    back = torch_cls(_groups(qs))
    back.load_state_dict(copy.deepcopy(got))     # (a checkpoint file is a copy; loading shares the tensors it is given)
    for p, q in zip(ps[:2], qs[:2]):
        q.grad = p.grad.clone()
    ref.step()
    back.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
    assert float(back.state[qs[0]]["step"]) == 4.0


def test_adam_checkpoint_loads_into_adamw_and_back():
    """The rollback reloads whatever `latest.pt` holds: the decay rule travels with the param_groups, as in torch."""
    from goliath_amd import optim

    ps = _params()
    ours = optim.AdamW(_groups(ps))
    ours.load_state_dict(torch.optim.Adam(_groups(ps), weight_decay=0.03).state_dict())
    assert [g["decoupled_weight_decay"] for g in ours.param_groups] == [False, False]
    assert [g["weight_decay"] for g in ours.param_groups] == [0.03, 0.03]
    t = torch.optim.Adam(_groups(ps))
    t.load_state_dict(ours.state_dict())


def test_unsupported_options_raise():
    from goliath_amd import _lib, optim

    p = [torch.nn.Parameter(torch.zeros(4))]
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(_lib.GoliathHipError):
            cls(p, amsgrad=True)
        with pytest.raises(_lib.GoliathHipError):
            cls(p, maximize=True)
        with pytest.raises(_lib.GoliathHipError):
            cls([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
        with pytest.raises(_lib.GoliathHipError):
            cls(p).step(lambda: 0.0)
        with pytest.raises(ValueError):
            cls(p, max_norm=0.0)
    opt = optim.Adam(p)
    sd = torch.optim.Adam(p, amsgrad=True).state_dict()
    with pytest.raises(_lib.GoliathHipError):
        opt.load_state_dict(sd)


def test_step_on_cpu_tensors_raises():
    from goliath_amd import _lib, optim

    p = torch.nn.Parameter(torch.ones(4))
    opt = optim.Adam([p], max_norm=1.0, scrub_nonfinite=True)
    assert opt.step() is None                    # nothing has a gradient: nothing to do, as in torch
    p.grad = torch.ones(4)
    with pytest.raises(_lib.GoliathHipError):
        opt.step()
    assert torch.equal(p, torch.ones(4)) and len(opt.state[p]) == 0


def test_constructor_takes_torchs_arguments():
    from goliath_amd import optim

    for ours, theirs in ((optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW)):
        mine, want = inspect.signature(ours).parameters, inspect.signature(theirs).parameters
        for k in ("params", "lr", "betas", "eps", "weight_decay"):
            assert mine[k].default == want[k].default and mine[k].kind == want[k].kind, k
        assert list(mine)[:5] == list(want)[:5]
        for k, d in (("max_norm", None), ("scrub_nonfinite", False), ("write_back_grads", True)):
            assert mine[k].kind is inspect.Parameter.KEYWORD_ONLY and mine[k].default == d


def test_finish_and_step_finishes_then_steps():
    from goliath_amd import parallel

    log = []

    class Sync:
        def finish(self):
            log.append("finish")

    class Opt:
        def step(self):
            log.append("step")
            return None

    assert parallel.finish_and_step(Sync(), Opt()) is None and log == ["finish", "step"]
    assert parallel.finish_and_step(None, Opt()) is None and log == ["finish", "step", "step"]


@needs_ref
def test_reference_build_optimizer_builds_the_class():
    """`class_name: goliath_amd.optim.Adam` in the reference's optimizer config, with per_module learning rates
    (config/rgca_example.yml:76-77 names torch.optim.Adam there)."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import ref_stubs

    ref_stubs.install()
    from ca_code.utils.module_loader import build_optimizer

    from goliath_amd import optim

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.decoder = torch.nn.Linear(3, 4)
            self.encoder = torch.nn.Linear(4, 2)
            self.unused = torch.nn.Linear(2, 2)

    model = Model()
    for cls in ("Adam", "AdamW"):
        config = ref_stubs.AttrDict({"class_name": f"goliath_amd.optim.{cls}",
                                     "per_module": {"decoder": {"lr": 5e-4}, "encoder": {"lr": 1e-3}},
                                     "max_norm": 1.0, "scrub_nonfinite": True})
        opt = build_optimizer(config, model)
        assert type(opt) is getattr(optim, cls) and isinstance(opt, torch.optim.Optimizer)
        assert [g["lr"] for g in opt.param_groups] == [5e-4, 1e-3]
        assert [len(g["params"]) for g in opt.param_groups] == [2, 2]
        assert opt.max_norm == 1.0 and opt.scrub_nonfinite and opt.write_back_grads
