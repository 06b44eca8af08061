"""GPU: goliath_amd.optim.Adam / AdamW (csrc/optim.hip) against torch's own optimizer.

The reference's optimizer is torch's (config/rgca_example.yml:76-77), run after the literal scrub and clip lines of
ca_code/utils/train.py:209-212, so the yardstick is torch.optim.Adam / AdamW(foreach=False) on the CPU in float64 fed the
same float32 gradients.  The same torch code in float32 on the CPU gives the size of float32 rounding for every statistic;
the HIP result may deviate from float64 by a fixed multiple of that figure (2x for the parameter update, which is dominated
by the rounding of p that both share; 4x for exp_avg, exp_avg_sq, the norm and the written-back gradients: FMA contraction
and an equally valid evaluation order cost a few ulp per step).  Nothing is hard-coded: both sets of figures are measured in
the test and printed; with GOLIATH_PARITY_DIR set they are also written to optim_parity.json in that directory (the
tracked copy is profiles/optim_parity.json).

The scene: two groups (lr 5e-4 / 1e-3); tensors of 1, 63, 64, 65, CHUNK+1, 2 CHUNK+3 and [3,5,7] elements; the gradient of
the CHUNK+1 tensor is a view at element offset 1 of a larger buffer (no 16-byte alignment: the scalar path); one parameter
never has a gradient; 5 steps of 0.01 randn gradients, except step 2 (10 randn: clipped by ~1e-3); at step 3 NaN, +Inf and
-Inf sit at element 0, the last element and elements CHUNK-1 and CHUNK of every tensor that has them.  (At CHUNK = 4096 the
scene has 12,590 elements, so the small gradients have norm ~1.12 and are clipped mildly, by ~0.89, as well.)
"""
import copy
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, BIG_STEP, BAD_STEP = 5, 2, 3          # 1-based
LRS = (5e-4, 1e-3)
CASES = {"adam": ("Adam", 0.0), "adam_l2": ("Adam", 0.01), "adamw": ("AdamW", 0.01)}
NONE, MISALIGNED = 4, 5                      # indices into the scene's tensors


def _chunk():
    from goliath_amd import optim

    return optim.chunk_elems()


def _shapes():
    c = _chunk()
    return [(1,), (63,), (64,), (65,), (10,), (c + 1,), (2 * c + 3,), (3, 5, 7)]


def _group_of(i):
    return 0 if i < 5 else 1


def _bad_positions(n):
    c = _chunk()
    return sorted({0, n - 1} | ({c - 1, c} if n > c else set()))


@pytest.fixture(scope="module")
def scene():
    """Initial parameters and the gradients of every step (float32, CPU); read-only."""
    g = torch.Generator().manual_seed(20240)
    shapes = _shapes()
    p0 = [torch.randn(*s, generator=g) for s in shapes]
    grads, planted = [], 0
    bad = [float("nan"), float("inf"), float("-inf")]
    for step in range(1, STEPS + 1):
        scale = 10.0 if step == BIG_STEP else 0.01
        gs = [scale * torch.randn(*s, generator=g) for s in shapes]
        if step == BAD_STEP:
            k = 0
            for i, x in enumerate(gs):
                if i == NONE:
                    continue
                for pos in _bad_positions(x.numel()):
                    x.view(-1)[pos] = bad[k % 3]
                    k += 1
                    planted += 1
        grads.append(gs)
    return {"p0": p0, "grads": grads, "planted": planted}


def _groups(params):
    return [{"params": [p for i, p in enumerate(params) if _group_of(i) == gi], "lr": LRS[gi]} for gi in (0, 1)]


def _torch_run(scene, case, dtype, steps=STEPS, scrub_clip=True, start=None):
    """The reference's lines on the CPU.  -> dict(p, m, v [per tensor], norms [per step], grads [per step, after the
    scrub and the clip]).  start = (params, optimizer state_dict) to continue from."""
    name, wd = CASES[case]
    params = [torch.nn.Parameter(x.detach().clone().to(dtype)) for x in (scene["p0"] if start is None else start[0])]
    opt = getattr(torch.optim, name)(_groups(params), weight_decay=wd, foreach=False)
    if start is not None:
        opt.load_state_dict(copy.deepcopy(start[1]))
    norms, post = [], []
    for gs in scene["grads"][steps[0]:steps[1]] if isinstance(steps, tuple) else scene["grads"][:steps]:
        live = []
        for i, (p, g) in enumerate(zip(params, gs)):
            if i != NONE:
                p.grad = g.detach().clone().to(dtype)
                live.append(p)
        if scrub_clip:
            for p in live:                                          # train.py:209-212, literally
                p.grad.data[torch.isnan(p.grad.data)] = 0
                p.grad.data[torch.isinf(p.grad.data)] = 0
            norms.append(float(torch.nn.utils.clip_grad_norm_(live, 1.0).double()))
        post.append([None if p.grad is None else p.grad.detach().clone() for p in params])
        opt.step()
    state = lambda k: [opt.state[p][k].detach().clone() if k in opt.state[p] else None for p in params]
    return {"p": [p.detach().clone() for p in params], "m": state("exp_avg"), "v": state("exp_avg_sq"), "norms": norms,
            "grads": post, "opt": opt}


class _Hip:
    """Our optimizer on the scene: parameters on the GPU, every gradient tensor allocated once (the misaligned one as a
    view at offset 1 of `buffer`) and refilled per step."""

    def __init__(self, scene, case, start=None, **kw):
        from goliath_amd import optim

        name, wd = CASES[case]
        self.scene = scene
        self.params = [torch.nn.Parameter(x.detach().clone().float().cuda()) for x in (scene["p0"] if start is None else start[0])]
        n = self.params[MISALIGNED].numel()
        self.buffer = torch.full((n + 2,), 123.0, device="cuda")
        for i, p in enumerate(self.params):
            if i == MISALIGNED:
                p.grad = self.buffer[1:1 + n].view_as(p)
                assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
            elif i != NONE:
                p.grad = torch.zeros_like(p)
        self.opt = getattr(optim, name)(_groups(self.params), weight_decay=wd, **kw)
        if start is not None:
            self.opt.load_state_dict(copy.deepcopy(start[1]))
        self.norms, self.nonfinite = [], []

    def fill(self, step):                    # 0-based
        for i, (p, g) in enumerate(zip(self.params, self.scene["grads"][step])):
            if i != NONE:
                p.grad.copy_(g)

    def run(self, first=0, last=STEPS):
        for s in range(first, last):
            self.fill(s)
            self.opt.step()
            if self.opt.last_grad_norm is not None:
                self.norms.append(float(self.opt.last_grad_norm))
                self.nonfinite.append(int(self.opt.last_nonfinite))
        return self

    def result(self):
        st = lambda k: [self.opt.state[p][k].detach().cpu() if k in self.opt.state[p] else None for p in self.params]
        return {"p": [p.detach().cpu() for p in self.params], "m": st("exp_avg"), "v": st("exp_avg_sq"),
                "norms": list(self.norms)}


def _cat(xs, skip_none=True):
    return torch.cat([x.double().reshape(-1) for i, x in enumerate(xs) if x is not None and i != NONE])


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _figures(run, ref, p0):
    """The four statistics of `run` against the float64 reference."""
    out = {"update": _rel(_cat(run["p"]) - _cat(p0), _cat(ref["p"]) - _cat(p0)),
           "exp_avg": _rel(_cat(run["m"]), _cat(ref["m"])), "exp_avg_sq": _rel(_cat(run["v"]), _cat(ref["v"]))}
    if ref["norms"]:
        out["norm"] = max(abs(a - b) / b for a, b in zip(run["norms"], ref["norms"]))
    return out


BARS = {"update": 2.0, "exp_avg": 4.0, "exp_avg_sq": 4.0, "norm": 4.0, "grads": 4.0}


def _judge(label, hip, f32):
    print(f"{label}: " + ", ".join(f"{k} hip {hip[k]:.3e} / f32 {f32[k]:.3e} (bar {BARS[k]:g}x)" for k in hip))
    for k in hip:
        assert hip[k] <= BARS[k] * f32[k], (label, k, hip[k], f32[k])


_REPORT = {}


def _report(key, hip, f32):
    _REPORT[key] = {"hip_vs_f64": hip, "torch_f32_vs_f64": f32, "bars_x_f32": {k: BARS[k] for k in hip}}
    out = os.environ.get("GOLIATH_PARITY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    from goliath_amd import build

    json.dump({"what": "goliath_amd.optim vs torch on the CPU in float64 after 5 steps of the scene of tests/test_gpu_optim.py; "
                       "the bar of every statistic is a multiple of what torch in float32 on the CPU deviates by",
               "csrc_sha16": build.source_digest(), "chunk_elems": _chunk(), "cases": _REPORT},
              open(os.path.join(out, "optim_parity.json"), "w"), indent=1)


@pytest.fixture(scope="module")
def refs(scene):
    """float64 and float32 torch runs of every case, computed once."""
    return {case: {"f64": _torch_run(scene, case, torch.float64), "f32": _torch_run(scene, case, torch.float32)}
            for case in CASES}


@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_torch_after_five_steps(scene, refs, case):
    ref, f32 = refs[case]["f64"], refs[case]["f32"]
    hip = _Hip(scene, case, max_norm=1.0, scrub_nonfinite=True).run()
    got = hip.result()
    a, b = _figures(got, ref, scene["p0"]), _figures(f32, ref, scene["p0"])
    _report(case, a, b)
    _judge(case, a, b)
    assert len(got["norms"]) == STEPS and ref["norms"][BIG_STEP - 1] > 100.0
    assert hip.nonfinite == [scene["planted"] if s == BAD_STEP else 0 for s in range(1, STEPS + 1)]
    # untouched, bit for bit: the parameter without a gradient (and no state, no step), and the element in front of the
    # misaligned gradient view
    none = hip.params[NONE]
    assert torch.equal(none.detach().cpu(), scene["p0"][NONE]) and none.grad is None and len(hip.opt.state[none]) == 0
    assert "step" not in hip.opt.state[none]
    assert float(hip.buffer[0]) == 123.0 and float(hip.buffer[-1]) == 123.0
    steps = [float(hip.opt.state[p]["step"]) for i, p in enumerate(hip.params) if i != NONE]
    assert steps == [float(STEPS)] * (len(hip.params) - 1)
    assert all(torch.isfinite(p).all() for p in got["p"])


def test_gradient_write_back(scene, refs):
    """After the NaN / Inf step p.grad holds what the reference's lines leave there; with write_back_grads=False it is left
    as it was put in, and the parameters do not depend on the choice."""
    ref, f32 = refs["adam"]["f64"]["grads"][BAD_STEP - 1], refs["adam"]["f32"]["grads"][BAD_STEP - 1]
    on = _Hip(scene, "adam", max_norm=1.0, scrub_nonfinite=True).run(0, BAD_STEP)
    off = _Hip(scene, "adam", max_norm=1.0, scrub_nonfinite=True, write_back_grads=False).run(0, BAD_STEP)
    assert on.nonfinite[-1] == off.nonfinite[-1] == scene["planted"] > 0
    got = [None if p.grad is None else p.grad.detach().cpu() for p in on.params]
    for i, (a, r) in enumerate(zip(got, ref)):
        if i == NONE:
            assert a is None and r is None
            continue
        assert torch.equal(a == 0, r == 0), i                      # exact zeros where the reference has zeros
        for pos in _bad_positions(a.numel()):
            assert float(a.view(-1)[pos]) == 0.0
    hip = {"grads": _rel(_cat(got), _cat(ref))}
    _judge("write-back", hip, {"grads": _rel(_cat(f32), _cat(ref))})
    for i, (p, q) in enumerate(zip(on.params, off.params)):
        assert torch.equal(p.detach(), q.detach()), i              # same parameters either way, bit for bit
        if i != NONE:
            put_in = scene["grads"][BAD_STEP - 1][i]
            kept = q.grad.detach().cpu()
            assert torch.equal(kept.view(torch.int32), put_in.view(torch.int32)), i     # NaNs included
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(on.opt.state[p][k], off.opt.state[q][k])
    assert float(on.buffer[0]) == 123.0 and float(off.buffer[0]) == 123.0


def _single(n, value, **kw):
    from goliath_amd import optim

    p = torch.nn.Parameter(torch.ones(n, device="cuda"))
    p.grad = torch.full((n,), value, device="cuda")
    return p, optim.Adam([p], lr=1e-3, **kw)


def test_edge_norms():
    n = 1000
    p, opt = _single(n, 0.0, max_norm=1.0, scrub_nonfinite=True)
    opt.step()
    assert float(opt.last_grad_norm) == 0.0 and float(opt.last_clip_coef) == 1.0 and int(opt.last_nonfinite) == 0
    assert torch.equal(p.detach(), torch.ones_like(p)) and torch.equal(p.grad, torch.zeros_like(p))
    assert all(torch.isfinite(opt.state[p][k]).all() for k in ("exp_avg", "exp_avg_sq"))
    # a norm just below and just above max_norm: min(1, max_norm / (norm + 1e-6)) is exactly 1 / below 1
    for norm, clipped in ((0.999, False), (1.001, True)):
        value = norm / n ** 0.5
        p, opt = _single(n, value, max_norm=1.0)
        before = p.grad.clone()
        opt.step()
        got, coef = float(opt.last_grad_norm), float(opt.last_clip_coef)
        assert abs(got - norm) < 1e-6 * norm
        if clipped:
            assert coef < 1.0 and abs(coef - 1.0 / (got + 1e-6)) < 1e-15
            assert torch.equal(p.grad, before * torch.tensor(coef).float().cuda())
        else:
            assert coef == 1.0 and torch.equal(p.grad, before)
        assert torch.isfinite(p).all()


def test_plain_mode_is_torchs_adam(scene):
    """max_norm=None, scrub_nonfinite=False: one pass, no statistics, gradients untouched (finite steps only)."""
    sub = dict(scene, grads=[g for s, g in enumerate(scene["grads"], 1) if s != BAD_STEP])
    ref = _torch_run(sub, "adam", torch.float64, steps=4, scrub_clip=False)
    f32 = _torch_run(sub, "adam", torch.float32, steps=4, scrub_clip=False)
    hip = _Hip(sub, "adam").run(0, 4)
    assert hip.opt.last_grad_norm is None or float(hip.opt.last_grad_norm) == 0.0
    a, b = _figures(hip.result(), ref, scene["p0"]), _figures(f32, ref, scene["p0"])
    _report("plain", a, b)
    _judge("plain", a, b)
    for i, (p, g) in enumerate(zip(hip.params, sub["grads"][3])):
        if i != NONE:
            assert torch.equal(p.grad.detach().cpu(), g)
    assert float(hip.buffer[0]) == 123.0


def test_two_runs_are_bit_identical(scene):
    runs = [_Hip(scene, "adamw", max_norm=1.0, scrub_nonfinite=True).run().result() for _ in range(2)]
    assert runs[0]["norms"] == runs[1]["norms"]
    for k in ("p", "m", "v"):
        for a, b in zip(runs[0][k], runs[1][k]):
            assert (a is None and b is None) or torch.equal(a, b), k


def test_checkpoints_interchange_with_torch_on_the_device(scene, refs):
    """Two steps on one side, the state_dict loaded into the other, the third step there: both orders against three float64
    steps, by the same rule as the five-step parity."""
    ref = _torch_run(scene, "adam", torch.float64, steps=3)
    f32 = _torch_run(scene, "adam", torch.float32, steps=3)
    bar = _figures(f32, ref, scene["p0"])
    bar.pop("norm")
    # ours -> torch
    hip = _Hip(scene, "adam", max_norm=1.0, scrub_nonfinite=True).run(0, 2)
    sd = hip.opt.state_dict()
    assert all(st["step"].device.type == "cpu" and float(st["step"]) == 2.0 for st in sd["state"].values())
    cont = _torch_run(scene, "adam", torch.float32, steps=(2, 3), start=(hip.result()["p"], sd))
    a = _figures(cont, dict(ref, norms=[]), scene["p0"])
    _report("hip_then_torch", a, bar)
    _judge("hip -> torch", a, bar)
    assert float(cont["opt"].state[cont["opt"].param_groups[0]["params"][0]]["step"]) == 3.0
    # torch -> ours
    first = _torch_run(scene, "adam", torch.float32, steps=2)
    back = _Hip(scene, "adam", start=(first["p"], first["opt"].state_dict()), max_norm=1.0, scrub_nonfinite=True).run(2, 3)
    a = _figures(back.result(), dict(ref, norms=[]), scene["p0"])
    _report("torch_then_hip", a, bar)
    _judge("torch -> hip", a, bar)
    live = [p for i, p in enumerate(back.params) if i != NONE]
    assert all(float(back.opt.state[p]["step"]) == 3.0 and back.opt.state[p]["step"].is_cuda for p in live)
    assert len(back.opt.state[back.params[NONE]]) == 0


def test_graph_capture_replays_the_step(scene):
    """One captured step (a linear graph on one stream) replayed with new gradient values in the same tensors equals eager
    steps bit for bit; a gradient tensor at a new address cannot be captured: it raises and the capture ends cleanly."""
    from goliath_amd import _lib

    kw = dict(max_norm=1.0, scrub_nonfinite=True)
    eager = _Hip(scene, "adamw", **kw).run(0, 3)
    cap = _Hip(scene, "adamw", **kw).run(0, 1)                   # warm-up: tables, state and scalars exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.opt.step()
    for s in (1, 2):
        cap.fill(s)
        graph.replay()
        cap.norms.append(float(cap.opt.last_grad_norm))
    torch.cuda.synchronize()
    a, b = eager.result(), cap.result()
    assert a["norms"] == b["norms"]
    for k in ("p", "m", "v"):
        for x, y in zip(a[k], b[k]):
            assert (x is None and y is None) or torch.equal(x, y), k
    assert all(float(cap.opt.state[p]["step"]) == 3.0 for i, p in enumerate(cap.params) if i != NONE)
    assert int(cap.opt.last_nonfinite) == scene["planted"]      # the third step is the NaN / Inf one
    # a new gradient tensor: the tables would have to be rebuilt
    moved = cap.params[0]
    moved.grad = torch.zeros_like(moved)
    torch.cuda.synchronize()
    with pytest.raises(_lib.GoliathHipError):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            cap.opt.step()
    assert not torch.cuda.is_current_stream_capturing()
    torch.cuda.synchronize()
    before = moved.detach().clone()
    cap.fill(3)
    cap.opt.step()                                               # eager: rebuilt, runs
    torch.cuda.synchronize()
    assert float(cap.opt.state[moved]["step"]) == 4.0 and not torch.equal(moved.detach(), before)
