"""CPU: goliath_amd.effnet's twins against float64 and against a composition of plain library modules, the state-dict
loader, the loss twin against the reference's lines, the drop-in keyword and the C-ABI marshallers (no GPU needed)."""
import ctypes
import inspect
import os
import re
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import effnet_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gol_mbconv_front_fwd", "gol_mbconv_front_bwd_x"]


@pytest.mark.parametrize("i", range(len(ec.CASES)), ids=ec.IDS)
def test_float32_twin_within_the_bar_of_float64(i):
    """The bar the GPU test holds the kernel to is one the fp32 library lines meet with a wide margin (SiLU is smooth:
    nothing is masked or excluded)."""
    ref = ec.reference(i)
    got = ec.run_twin(i, torch.float32)
    err = [ec.rel(a, b) for a, b in zip(got, ref)]
    print(ec.IDS[i], err)
    B, Ci, Ce, H, W, k, s, _ = ec.CASES[i]
    assert tuple(ref[0].shape) == (B, Ce, ec.out_size(H, k, s), ec.out_size(W, k, s)) and tuple(ref[1].shape) == (B, Ce)
    assert tuple(ref[2].shape) == (B, Ci, H, W) and float(ref[2].abs().max()) > 0
    assert max(err) <= ec.BAR


def _front_padding_the_input(x, w_e, b_e, w_d, b_d, k, stride):
    """The padding bug: zero-pad x, then expand -- the border of e becomes SiLU(b_e) instead of 0."""
    p, Ce = (k - 1) // 2, w_d.shape[0]
    e = F.silu(F.conv2d(F.pad(x, (p, p, p, p)), w_e.reshape(Ce, -1, 1, 1), b_e))
    z = F.conv2d(e, w_d.reshape(Ce, 1, k, k), b_d, stride, 0, 1, Ce)
    return z, F.silu(z).sum((2, 3))


@pytest.mark.parametrize("i", ec.EXPAND, ids=[ec.IDS[i] for i in ec.EXPAND])
def test_cases_see_the_padding_bug(i):
    ref = ec.reference(i)
    bad = ec.run_twin(i, torch.float64, _front_padding_the_input)
    err = [ec.rel(a, b) for a, b in zip(bad, ref)]
    print(ec.IDS[i], err)
    assert bad[0].shape == ref[0].shape
    assert min(err) > 100 * ec.BAR


@pytest.mark.parametrize("shape", [(2, 3, 37, 50), (1, 3, 64, 48)], ids=["2x3x37x50", "1x3x64x48"])
def test_folded_network_equals_the_module_composition(shape):
    from goliath_amd import effnet

    net = ec.module_network(3)
    feats = effnet.EffNetB0Features().load_torchvision_state_dict(net.state_dict())
    image = ec.draw_image(11, shape).double()
    with torch.no_grad():
        want = ec.module_taps(net.double(), image)
        got = feats.forward_torch(image)
    H, W = shape[2:]
    sizes = [(-(-H // 2), -(-W // 2))]
    sizes += [(ec.out_size(sizes[0][0], 3, 2), ec.out_size(sizes[0][1], 3, 2))]
    sizes += [(ec.out_size(sizes[1][0], 5, 2), ec.out_size(sizes[1][1], 5, 2))]
    assert [tuple(t.shape) for t in got] == [(shape[0], c, *hw) for c, hw in zip((16, 24, 40), sizes)]
    err = [ec.rel(a, b) for a, b in zip(got, want)]
    print(err)
    assert all(t.dtype == torch.float64 for t in got) and max(err) <= 1e-12
    # float32 goes through the same fold (computed in float64, then cast)
    err32 = [ec.rel(a, b) for a, b in zip(feats.forward_torch(image.float()), want)]
    assert max(err32) <= 1e-4 and not any(p.requires_grad for p in feats.parameters())


def test_state_dict_keys_and_loader_errors(tmp_path):
    from goliath_amd import effnet

    sd = ec.module_network(5).state_dict()
    feats = effnet.EffNetB0Features()
    keys = [k for k, _ in effnet.expected_entries()]
    assert list(feats.state_dict().keys()) == keys == [k for k in sd if not k.endswith("num_batches_tracked")]
    assert len(keys) == 5 + 4 * 5 + 5 * (5 + 4 + 5)      # stem; 4 expands; depthwise, SE and project of 5 blocks
    assert tuple(feats.state_dict()["features.3.0.block.1.0.weight"].shape) == (144, 1, 5, 5)
    assert tuple(feats.state_dict()["features.1.0.block.1.fc1.weight"].shape) == (8, 32, 1, 1)
    assert tuple(feats.state_dict()["features.3.1.block.2.fc1.weight"].shape) == (10, 240, 1, 1)
    ref = effnet.EffNetB0Features().load_torchvision_state_dict(sd)
    # without the prefix, with later features and the classifier: ignored
    bare = {k[len("features."):]: v for k, v in sd.items()}
    bare.update({"4.0.block.0.0.weight": torch.zeros(3), "classifier.1.weight": torch.zeros(5, 5)})
    other = effnet.EffNetB0Features().load_torchvision_state_dict(bare)
    for k in keys:
        assert torch.equal(ref.state_dict()[k], sd[k]) and torch.equal(other.state_dict()[k], sd[k])
    # a file; the fold is redone after loading
    before = feats.folded()["2.0"][0].clone()
    path = tmp_path / "effnet_b0.pth"
    torch.save(sd, path)
    assert effnet.as_features(feats) is feats and feats.load_torchvision_state_dict(str(path)) is feats
    assert torch.equal(feats.folded()["2.0"][0], ref.folded()["2.0"][0]) and not torch.equal(before, ref.folded()["2.0"][0])
    assert feats.double().folded(torch.float64)["2.0"][0].dtype == torch.float64
    # errors name what is expected
    with pytest.raises(FileNotFoundError, match="efficientnet_b0 state dict"):
        effnet.EffNetB0Features().load_torchvision_state_dict(str(tmp_path / "absent.pth"))
    renamed = {k.replace("features.2.1.block.2.fc1", "features.2.1.block.2.fc_1"): v for k, v in sd.items()}
    with pytest.raises(KeyError, match=r"features\.2\.1\.block\.2\.fc1\.weight.*\(6, 144, 1, 1\).*fc_1"):
        effnet.EffNetB0Features().load_torchvision_state_dict(renamed)
    wrong = dict(sd)
    wrong["features.3.0.block.1.0.weight"] = torch.zeros(144, 1, 3, 3)
    with pytest.raises(ValueError, match=r"features\.3\.0\.block\.1\.0\.weight.*expected \(144, 1, 5, 5\)"):
        effnet.EffNetB0Features().load_torchvision_state_dict(wrong)
    with pytest.raises(TypeError):
        effnet.EffNetB0Features().load_torchvision_state_dict(3)


@pytest.mark.parametrize("masked", [True, False], ids=["tensor-mask", "mask-none"])
def test_loss_twin_equals_the_reference_lines(masked):
    from goliath_amd import effnet

    feats, x, y, mask = ec.loss_case()
    x, y, mask = x.double().requires_grad_(True), y.double(), (mask.double() if masked else None)
    got = effnet.effnet_loss_torch(feats, x, y, mask)
    want = ec.reference_transcription(feats.forward_torch(x), feats.forward_torch(y), mask)
    g_got, = torch.autograd.grad(got, x)
    g_want, = torch.autograd.grad(want, x)
    assert got.dtype == torch.float64 and float(want) > 0 and float(g_want.abs().max()) > 0
    assert ec.rel(got, want) <= 1e-12 and ec.rel(g_got, g_want) <= 1e-12
    assert effnet.EfficientNetLoss(feats).weights == [0.8, 0.1, 0.1]
    assert list(inspect.signature(effnet.EfficientNetLoss.forward).parameters)[1:] == ["x", "y", "mask"]
    assert inspect.signature(effnet.EfficientNetLoss.forward).parameters["mask"].default is None


def _registry():
    entries = dict(rgb_l1="reference", rgb_ssim="reference", vgg="untouched", effnet="untouched", effnet_phys="untouched",
                   learn_blur="untouched")
    return types.SimpleNamespace(loss_registry=entries, FnLoss=lambda fn, args: (fn, args))


def test_patch_losses_keyword():
    from goliath_amd import dropin, effnet

    assert inspect.signature(dropin.patch_losses).parameters["effnet"].default is None
    before = {name for name in ("torchvision", "ca_code.loss.effnet") if name in sys.modules}    # other tests may have shims
    reg = dropin.patch_losses(_registry())
    assert reg.loss_registry["effnet"] == "untouched" and reg.loss_registry["effnet_phys"] == "untouched"
    feats = effnet.EffNetB0Features()
    reg = dropin.patch_losses(_registry(), effnet=feats)
    assert reg.loss_registry["vgg"] == "untouched" and reg.loss_registry["learn_blur"] == "untouched"
    a = reg.loss_registry["effnet"](None, mask_erode=3, dst_key="rgb2")
    b = reg.loss_registry["effnet_phys"](None)
    assert isinstance(a, effnet.EffNetLoss) and isinstance(b, effnet.EffNetLoss)
    assert a.net.ftrs_net is feats and b.net.ftrs_net is feats        # ONE shared network
    assert (a.src_key, a.tgt_key, a.dst_key, a.mask_key, a.mask_erode) == ("rendered_rgb", "image", "rgb2", "image_mask", 3)
    assert (b.src_key, b.tgt_key, b.dst_key, b.mask_key, b.mask_erode) == ("rendered_phys_rgb", "image", None, "image_mask", None)
    # a state dict, shared as well
    reg = dropin.patch_losses(_registry(), effnet=ec.module_network(5).state_dict())
    assert reg.loss_registry["effnet"](None).net.ftrs_net is reg.loss_registry["effnet_phys"](None).net.ftrs_net
    with pytest.raises(FileNotFoundError):
        dropin.patch_losses(_registry(), effnet="/nonexistent/efficientnet_b0.pth")
    with pytest.raises(ValueError):
        effnet.EffNetLoss(None)
    assert {name for name in ("torchvision", "ca_code.loss.effnet") if name in sys.modules} == before


def _header():
    return open(os.path.join(ROOT, "include", "goliath_hip.h")).read()


def test_library_lists_the_new_entries():
    from goliath_amd import _lib

    for name in ENTRIES + ["gol_mbconv_front_tiles"]:
        assert name in _lib.exported_symbols()
        assert re.search(r"\bint\s+" + name + r"\s*\(", _header()), name


@pytest.mark.parametrize("entry", ENTRIES)
def test_marshallers_follow_the_header(entry, monkeypatch):
    """Each marshaller passes exactly the parameters goliath_hip.h declares, in its order and with its C types (the library
    sets no argtypes: a miscounted or swapped list would reach a kernel as a garbage pointer)."""
    from goliath_amd import _lib, effnet

    decl = re.search(r"\bint\s+" + entry + r"\s*\(([^)]*)\)", _header()).group(1)
    params = [re.fullmatch(r"(.*?)\s*\b(\w+)", " ".join(p.split())).groups() for p in decl.split(",")]
    fn = getattr(effnet, "_abi_" + entry[len("gol_"):])
    sig = inspect.signature(fn).parameters
    assert set(sig) == {n for _, n in params} - {"stream"}
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in sig.values())
    kw, want = {}, []
    for i, (ctype, name) in enumerate(params):   # a distinct value per parameter
        if "*" in ctype:
            cls, v = ctypes.c_void_p, 0x10000 * (i + 1)
        else:
            cls, v = {"int": (ctypes.c_int, i + 1)}[ctype]
        v = {"stream": 0xBEEF}.get(name, v)
        if name != "stream":
            kw[name] = v
        want.append((cls, v))
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(effnet, "stream_ptr", lambda: ctypes.c_void_p(0xBEEF))
    fn(**kw)
    assert len(calls) == 1 and calls[0][0] == entry
    args = calls[0][1]
    assert len(args) == len(params)
    for (ctype, name), (cls, v), a in zip(params, want, args):
        assert type(a) is cls and a.value == v, (name, ctype, a)


def test_no_cpu_path_and_no_weight_gradient():
    from goliath_amd import _lib, effnet

    inp = ec.inputs(5)
    args = (inp["w_e"], inp["b_e"], inp["w_d"], inp["b_d"], inp["k"], inp["stride"])
    with pytest.raises(_lib.GoliathHipError, match="CUDA"):     # no CPU path, no quiet fall-back
        effnet.mbconv_front(inp["x"], *args)
    for n in range(4):
        grad = [t.clone().requires_grad_(True) if m == n else t for m, t in enumerate(args[:4])]
        with pytest.raises(_lib.GoliathHipError, match="frozen"):
            effnet.mbconv_front(inp["x"], *grad, inp["k"], inp["stride"])
    with pytest.raises(_lib.GoliathHipError, match="shapes"):
        effnet.mbconv_front(inp["x"], inp["w_e"], inp["b_e"], inp["w_d"][:, :3, :3], inp["b_d"], 5, 2)
    feats = effnet.EffNetB0Features()
    with pytest.raises(_lib.GoliathHipError, match="CUDA"):
        effnet.EfficientNetLoss(feats)(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    assert effnet.supported(16, 96, 1024, 667, 3, 2) and effnet.supported(32, 32, 9, 9, 3, 1, expand=False)
    assert not any(effnet.supported(*a) for a in ((16, 96, 9, 9, 7, 1), (16, 96, 9, 9, 3, 3), (12, 96, 9, 9, 3, 1),
                                                   (16, 24, 9, 9, 3, 1)))
    assert not effnet.supported(16, 32, 9, 9, 3, 1, expand=False)
    z, ssum = effnet.mbconv_front_torch(inp["x"].requires_grad_(False), *args)
    assert tuple(z.shape) == (3, 16, 1, 1) and tuple(ssum.shape) == (3, 16)
