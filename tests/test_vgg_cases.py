"""CPU: the case tables of tests/vgg_cases.py judged on the float64 reference alone -- the share of upstream gradients a
case zeroes near its kinks stays under the cap, the image case reaches both clamp branches, and the seed of the loss
case leaves the fp32 twin on the float64 twin's side of every ReLU and pool decision."""
import pytest
import torch

import vgg_cases as vc


@pytest.mark.parametrize("i", range(len(vc.CASES)), ids=vc.IDS)
def test_zeroed_share_stays_under_the_cap(i):
    """At most 0.2 % of the output elements of any case lose their upstream gradient to a kink (KINK = 1e-4)."""
    ref = vc.reference(i)
    print(vc.IDS[i], "zeroed", ref["zeroed"])
    assert ref["zeroed"] <= vc.ZEROED_CAP
    assert float(ref["g_x"].abs().max()) > 0 and float(ref["out"].abs().max()) > 0
    (_, _, _, H, W), pool, _ = vc.CASES[i]
    assert tuple(ref["out"].shape[2:]) == ((H // 2, W // 2) if pool else (H, W))


def test_image_case_reaches_both_clamp_branches():
    from goliath_amd import perceptual

    x = vc.inputs(0)["x"]
    assert vc.CASES[0][2] and float((x < 0).float().mean()) > 0.05 and float((x > 255).float().mean()) > 0.05
    n = perceptual.normalize(torch.tensor([0.0, 255.0, 300.0, -3.0]).view(1, 1, 4, 1).expand(1, 3, 4, 1))
    mean, std = torch.tensor(perceptual.MEAN), torch.tensor(perceptual.STD)
    assert torch.equal(n[0, :, 1, 0], (1.0 - mean) / std) and torch.equal(n[0, :, 2, 0], n[0, :, 1, 0])
    assert torch.equal(n[0, :, 0, 0], (0.0 - mean) / std) and torch.equal(n[0, :, 3, 0], n[0, :, 0, 0])


def test_pool_positions_follow_torch():
    """The position numbering of the references (0..3 row-major, the first maximum wins) is max_pool2d's."""
    torch.manual_seed(0)
    y = torch.relu(torch.randn(2, 3, 7, 9))
    y[0, 0, :2, :2] = 0.0
    y[0, 1, :2, :2] = 1.5
    win = vc.windows(y)
    p, idx = torch.nn.functional.max_pool2d(y, 2, return_indices=True)
    assert torch.equal(win.max(-1).values, p)
    pos = win.argmax(-1)
    r, c = torch.div(idx, 9, rounding_mode="floor"), idx % 9
    assert torch.equal((r % 2) * 2 + c % 2, pos)
    assert int(pos[0, 0, 0, 0]) == 0 and int(pos[0, 1, 0, 0]) == 0


def best_loss_seed(n=120):
    """How LOSS_SEED was chosen: the seed among 0..n-1 with the widest float64 margin (a few seconds; not a test)."""
    return max((vc.loss_margin(*vc.loss_case(s)), s) for s in range(n))


def test_loss_seed_keeps_fp32_on_the_float64_side():
    """The widest margin among the seeds 0..119 is 6.6e-6 (seed 48), of the order of the fp32 pre-activation error, so a
    fixed absolute margin is no safe assertion at this size.  Asserted instead: at the chosen seed the fp32 twin and the
    float64 twin have identical ReLU masks and pool positions, for prediction and target."""
    feats, x, y, mask = vc.loss_case(vc.LOSS_SEED)
    print("margin", vc.loss_margin(feats, x, y, mask))
    assert float((mask == 0).float().mean()) > 0.2 and float(mask.max()) > 0.9
    for img in (x, y):
        _, _, relu32, pool32 = vc.trace(feats, img, torch.float32)
        _, _, relu64, pool64 = vc.trace(feats, img, torch.float64)
        assert len(relu32) == 13 and len(pool32) == 4
        for a, b in zip(relu32 + pool32, relu64 + pool64):
            assert torch.equal(a, b)
