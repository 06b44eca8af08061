"""CPU: the edge scene of the shading tail (tests/shade_cases.py) is what it claims to be -- every class is populated, the
near-branch exclusion stays under its caps, both oracles are finite where HIP will be judged, and the zero_sh block realises
the clamp tie of color_rand.  Prints the float32-oracle-vs-float64 table per (class, quantity): the yardstick of
tests/test_gpu_shade_edges.py."""
import pytest
import torch

import shade_cases as sc


@pytest.mark.parametrize("env", [True, False])
def test_every_class_is_populated_and_the_exclusion_is_capped(env):
    ref = sc.reference(env)
    keep, total = ref["keep"], sc.B * sc.N
    assert int((~keep).sum()) <= 0.01 * total, int((~keep).sum())
    names = sc.ENV_CLASSES if env else sc.SG_CLASSES
    seen = torch.zeros(sc.B, sc.N, dtype=torch.int32)
    for c in names:
        m = ref["classes"][c]
        seen += m
        n, out = int((m & keep).sum()), int((m & ~keep).sum())
        print(f"SHADE_CLASS {'env' if env else 'sg'} {c:>12s} n={n:5d} excluded={out}")
        assert n >= sc.MIN_CLASS, (c, n)
        assert out <= 0.1 * int(m.sum()), (c, out, int(m.sum()))
    assert bool((seen == 1).all())                                   # a partition
    for c in sc.ELEMENT_MASKS:
        m = ref["elements"][c]
        n, out = int((m & keep[..., None]).sum()), int((m & ~keep[..., None]).sum())
        print(f"SHADE_CLASS {'env' if env else 'sg'} {c:>12s} n={n:5d} excluded={out}")
        assert n >= sc.MIN_CLASS and out <= 0.1 * int(m.sum()), (c, n, out)
    for n_run in (sc.N, sc.N_ODD):
        assert {c for c, _, _ in sc.judged(ref, n_run)} == set(names) | set(sc.ELEMENT_MASKS)
    # the constructed blocks land in the classes they were built for
    blk = lambda name: slice(*sc.BLOCKS[name])
    if env:
        assert bool(ref["classes"]["pole"][:, blk("pole")].all())
        assert int(ref["classes"]["seam"][:, blk("seam")].sum()) >= 0.9 * sc.B * sc.K
        assert float(ref["lookup"]["theta"][:, blk("pole")].min()) < 3e-3
    else:
        assert int(ref["classes"]["aligned"][:2, blk("aligned")].sum()) == 2 * sc.K


@pytest.mark.parametrize("env", [True, False])
def test_oracles_are_finite_where_judged_and_their_error_table(env):
    ref = sc.reference(env)
    print()
    for c, m, qs in sc.judged(ref):
        for o in qs:
            want, got = ref["q64"][o], ref["q32"][o]
            mm = m if m.dim() == 2 else m.expand_as(want) if m.shape[-1] != want.shape[-1] else m
            assert bool(torch.isfinite(want[mm]).all()), (c, o)
            assert bool(torch.isfinite(got[mm]).all()), (c, o)
            print(f"SHADE_ORACLE {'env' if env else 'sg'} {c:>12s} {o:>17s} n={int(m.sum()):5d} oracle32={sc.class_rel_l2(got, want, m):.2e}")


def test_zero_sh_block_realises_the_clamp_tie():
    """torch's clamp(min=0) passes the gradient where its input is >= 0: with color_rand as the only upstream gradient the
    SH planes of the zero_sh block receive u_rand x light_sh_rand, which is not zero."""
    s, ups = sc.scene(), sc.upstream()
    lo, hi = sc.BLOCKS["zero_sh"]
    out, g = sc.run_oracle(s, torch.float64, False, {"color_rand": ups["color_rand"]})
    assert not bool(out["color_rand"][:, lo:hi].any()) and not bool(out["diff_color"][:, lo:hi].any())
    got = sc.quantities(out, g)["g_sh"][:, lo:hi]                                  # [B,K,113]
    u, lr = ups["color_rand"][:, lo:hi].double(), s["light_sh_rand"].double()     # [B,K,3], [B,3,81]
    want = torch.cat([(u[..., None] * lr[:, None, :, :sc.NCOL]).flatten(2), torch.einsum("bkc,bcm->bkm", u, lr[:, :, sc.NCOL:])], -1)
    assert float(want.abs().min()) > 0
    assert torch.allclose(got, want, rtol=1e-14, atol=0)
