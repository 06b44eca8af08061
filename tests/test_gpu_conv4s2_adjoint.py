"""GPU: the encoder layer (csrc/encconv.hip) and the trunk layer (csrc/trunk.hip) are each other's adjoint.

With leak = 1 (every LeakyReLU mask is 1), zero bias and the identity input affine, `encoder.conv_ub_lrelu` with a weight
tensor Wt[Co,Ci,4,4] is a linear map A : [B,Ci,H,W] -> [B,Co,H/2,W/2], and `trunk.convt_ub_lrelu` reading the SAME memory
as [Ci_trunk = Co, Co_trunk = Ci, 4, 4] is its transpose.  So the input gradient of one is the forward of the other: the
quad-form GEMM serves trunk's forward and the encoder's input gradient, the row gather the encoder's forward and trunk's
input gradient (csrc/gol_conv4s2.h).

Bound: each side is asserted within 1e-5 rel-L2 of float64 (test_gpu_trunk.py, test_gpu_encoder.py), so by the triangle
inequality the two sides are within 2e-5 of each other."""
import pytest
import torch

from scenes import rel_l2

pytestmark = pytest.mark.gpu

# (B, Ci_enc, Co_enc, H, W)
SHAPES = [
    (2, 16, 16, 2, 2),     # every window and every quad is on a border: the narrow paths
    (3, 32, 48, 10, 14),   # odd batch; a ragged 32-channel group on the Co side; pixel tiles that wrap rows
    (1, 64, 32, 34, 66),   # several workgroups; odd output width 33
]
BOUND = 2e-5


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_encoder_and_trunk_are_adjoints(shape):
    from goliath_amd import encoder, trunk

    B, Ci, Co, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    Wt = (torch.randn(Co, Ci, 4, 4, generator=gen) / (4.0 * Ci ** 0.5)).cuda()
    x = torch.randn(B, Ci, H, W, generator=gen).cuda()             # fine grid
    g = torch.randn(B, Co, H // 2, W // 2, generator=gen).cuda()   # coarse grid
    zero_fine = torch.zeros(Ci, H, W, device="cuda")
    zero_coarse = torch.zeros(Co, H // 2, W // 2, device="cuda")

    # A x and A^T g from the encoder
    xe = x.clone().requires_grad_(True)
    enc_fwd = encoder.conv_ub_lrelu(xe, Wt, zero_coarse, 1.0, 1.0, 0.0)
    (enc_gx,) = torch.autograd.grad(enc_fwd, xe, g)
    # A^T g and A x from the trunk
    gt = g.clone().requires_grad_(True)
    trunk_fwd = trunk.convt_ub_lrelu(gt, Wt, zero_fine, 1.0)
    (trunk_gx,) = torch.autograd.grad(trunk_fwd, gt, x)

    assert enc_fwd.shape == trunk_gx.shape == g.shape and trunk_fwd.shape == enc_gx.shape == x.shape
    assert float(enc_fwd.detach().norm()) > 0 and float(trunk_fwd.detach().norm()) > 0
    err = {"enc g_x vs trunk fwd": rel_l2(enc_gx, trunk_fwd), "trunk g_x vs enc fwd": rel_l2(trunk_gx, enc_fwd)}
    print(shape, err)
    for name, v in err.items():
        assert v <= BOUND, (shape, name, v)
