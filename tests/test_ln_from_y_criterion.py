"""functional.ln_from_y_ok: which (gamma, beta) let FusedLayerNorm rebuild x_hat = (y - beta) /
gamma from the forward's output in its backward. Pure function of the two tensors; CPU."""
import torch

from dna_amd import functional as DF

R, GMIN = DF.LN_FROM_Y_MAX_RATIO, DF.LN_FROM_Y_MIN_GAMMA


def _ok(gamma, beta, **kw):
    return DF.ln_from_y_ok(torch.tensor(gamma, dtype=torch.float32),
                           torch.tensor(beta, dtype=torch.float32), **kw)


def test_well_conditioned_and_negative_gamma():
    g = torch.Generator().manual_seed(0)
    gamma = 1 + 0.1 * torch.randn(768, generator=g)
    beta = 0.1 * torch.randn(768, generator=g)
    assert DF.ln_from_y_ok(gamma, beta)
    assert DF.ln_from_y_ok(-gamma, -beta)  # signs do not matter, only magnitudes
    assert _ok([1.0, -1.0, 0.5], [0.0, 3.0, -2.0])


def test_zero_gamma_fails_whatever_beta():
    assert not _ok([1.0, 0.0, 1.0], [0.0, 0.0, 0.0])
    assert not _ok([1.0, -0.0, 1.0], [0.0, 0.0, 0.0])
    assert not _ok([0.0], [1.0])


def test_tiny_gamma_passes_only_with_beta_as_tiny():
    # the x_hat error is 2^-24 (|beta| / |gamma| + |x_hat|): a tiny gamma alone does no harm
    assert _ok([1e-6, -1e-6, 1.0], [0.0, 1e-5, 0.1])
    assert not _ok([1e-6, 1.0], [1.0, 0.0])
    assert not _ok([1.0, -1e-2], [0.0, 1.0])  # ratio 100
    assert _ok([1.0, -1e-1], [0.0, 1.0])      # ratio 10
    assert not _ok([GMIN / 2], [0.0])         # below the floor: 1 / gamma, y leave fp32's range
    assert _ok([GMIN], [0.0])


def test_large_beta():
    assert not _ok([1.0, 1.0], [0.0, 17.0])
    assert _ok([1.0, 1.0], [0.0, 15.0])
    assert not _ok([1.0], [float("inf")])
    assert not _ok([1.0], [float("nan")])
    assert not _ok([float("nan")], [0.0])


def test_boundary_is_inclusive():
    assert R == 16.0
    assert _ok([0.25, -2.0], [4.0, -32.0])  # exactly R, exact in fp32
    assert not _ok([0.25], [4.0 + 2.0 ** -21])
    assert not _ok([2.0], [32.0 + 2.0 ** -18])


def test_margin_and_shrink_move_the_threshold_inwards():
    # margin m: |gamma| may fall and |beta| may rise by m with the verdict still right
    assert _ok([1.0], [8.0], margin=0.25)             # 8.25 <= 16 * 0.75
    assert not _ok([1.0], [12.0], margin=0.25)        # 12.25 > 12
    assert not _ok([0.2], [0.0], margin=0.25)         # gamma could reach 0
    assert _ok([1.0], [15.0], shrink=0.05)            # 15 <= 16 * 0.95
    assert not _ok([1.0], [15.5], shrink=0.05)
    # whatever passes with a margin passes every perturbation inside it
    g = torch.Generator().manual_seed(1)
    gamma = torch.randn(4096, generator=g)
    beta = 4 * torch.randn(4096, generator=g)
    m = 0.05
    keep = torch.tensor([DF.ln_from_y_ok(gamma[i:i + 1], beta[i:i + 1], margin=m)
                         for i in range(gamma.numel())])
    assert 0 < keep.sum() < keep.numel()
    for _ in range(4):
        dg = (2 * torch.rand(4096, generator=g) - 1) * m
        db = (2 * torch.rand(4096, generator=g) - 1) * m
        assert DF.ln_from_y_ok((gamma + dg)[keep], (beta + db)[keep])
