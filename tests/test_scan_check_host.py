"""CPU: the selective-scan plan query at its thresholds, and the checker of
tests/test_gpu_selective_scan_paths.py checked itself (tests/scan_check.py): the threaded oracle
split equals the unsplit call, and the long-memory inputs make chunk carries visible -- a
reference that forgets everything older than one chunk, or whose carries are zero, is rejected
in EVERY row by the same assertion the GPU tests use, at no less than 10x the fp32 bound."""
import numpy as np
import pytest
import torch

from tests import scan_check as SC


# ---------------------------------------------------------------- dna_selective_scan_plan

def _plan(b, d, l, n):
    p = SC.plan(b, d, l, n)
    return p["chunked"], p["k"], p["nch"], p["carry_par"]


@pytest.mark.parametrize("shape,want", [
    # chunk-parallel kernels need dim % 8 == 0
    ((2, 8, 4104, 16), (True, 1, 9, False)), ((2, 5, 4104, 16), (False, 0, 0, False)),
    ((2, 12, 4104, 16), (False, 0, 0, False)), ((2, 16, 4104, 16), (True, 1, 9, False)),
    # nch = ceil(len / 512)
    ((1, 8, 512, 4), (True, 1, 1, False)), ((1, 8, 513, 4), (True, 1, 2, False)),
    # k channels per wave: dim % 8k == 0 and batch * nch * dim / 8k >= 2048 blocks
    ((1, 16 * 2048, 512, 16), (True, 2, 1, False)), ((1, 16 * 2047, 512, 16), (True, 1, 1, False)),
    ((8, 2064, 520, 16), (True, 2, 2, False)), ((8, 2032, 520, 16), (True, 1, 2, False)),
    ((16, 2080, 520, 8), (True, 4, 2, False)), ((16, 2016, 520, 8), (True, 2, 2, False)),
    ((16, 4096, 520, 4), (True, 8, 2, False)), ((16, 4032, 520, 4), (True, 4, 2, False)),
    ((16, 4096, 517, 4), (True, 8, 2, False)),
    # 2064 blocks at k = 4 too, but 2064 % 32 != 0: divisibility decides
    ((16, 2064, 520, 16), (True, 2, 2, False)),
    # carry kernel: carry_blk_kernel while nch * (N + 1) + 512 floats fit 64 KB
    ((1, 8, 933 * 512, 16), (True, 1, 933, False)), ((1, 8, 933 * 512 + 1, 16), (True, 1, 934, True)),
    ((1, 8, 478216, 16), (True, 1, 935, True)),
    ((1, 8, 1763 * 512, 8), (True, 1, 1763, False)), ((1, 8, 1763 * 512 + 1, 8), (True, 1, 1764, True)),
    ((1, 8, 3174 * 512, 4), (True, 1, 3174, False)), ((1, 8, 1625096, 4), (True, 1, 3175, True)),
    # the per > 1 shapes of carry_blk_kernel
    ((1, 8, 8712, 16), (True, 1, 18, False)), ((1, 8, 33288, 4), (True, 1, 66, False)),
    # the per-channel kernels have no carry kernel, whatever the length
    ((1, 5, 1625096, 4), (False, 0, 0, False)),
])
def test_plan_query_at_the_thresholds(shape, want):
    assert _plan(*shape) == want


def test_plan_query_matches_the_states_buffer_and_rejects_bad_shapes():
    from dna_amd import _native as N
    for b, d, l, n in [(2, 8, 4104, 16), (1, 8, 33288, 4), (16, 4096, 517, 4)]:
        nch = SC.plan(b, d, l, n)["nch"]
        assert N.lib().dna_selective_scan_states(b, d, l, n) == b * d * nch * (2 * n + 1)
    for bad in [(0, 8, 512, 16), (1, 0, 512, 16), (1, 8, 0, 16), (1, 8, 512, 5), (1, 8, 512, 32)]:
        with pytest.raises(N.NativeError):
            SC.plan(*bad)
    # every output pointer is optional
    assert N.lib().dna_selective_scan_plan(2, 8, 4104, 16, None, None, None, None) == 0


# ---------------------------------------------------------------- the oracle split

@pytest.mark.parametrize("shape,kw", [((3, 7, 700, 8), {}), ((2, 16, 1030, 4), {}),
                                      ((1, 5, 600, 16), {"softplus": False, "bias": False})])
def test_threaded_oracle_split_equals_the_unsplit_call(shape, kw):
    inp = SC.long_memory_inputs(*shape, seed=5, **kw)
    sp = kw.get("softplus", True)
    whole, split = SC.oracle(inp, sp, threads=1), SC.oracle(inp, sp, threads=16)
    assert set(whole) == set(split) and "out" in whole and "A" in whole
    assert ("delta_bias" in whole) == (inp["delta_bias"] is not None)
    for k in whole:
        scale = max(1.0, float(np.abs(whole[k]).max()))
        assert np.abs(whole[k] - split[k]).max() <= 1e-12 * scale, k


def test_optional_arguments_reach_the_oracle():
    inp = SC.long_memory_inputs(2, 8, 300, 4, seed=6)
    full = SC.oracle(inp)
    for drop in ("D", "z"):
        less = SC.oracle({**inp, drop: None})
        assert drop not in less and np.abs(less["out"] - full["out"]).max() > 1e-3


def test_long_memory_inputs_are_in_the_slow_band():
    for kw in ({}, {"bias": False}, {"softplus": False}, {"softplus": False, "bias": False}):
        inp = SC.long_memory_inputs(2, 16, 2048, 16, seed=7, **kw)
        eff = inp["delta"].double()
        if inp["delta_bias"] is not None:
            eff = eff + inp["delta_bias"].double()[None, :, None]
        if kw.get("softplus", True):
            eff = torch.nn.functional.softplus(eff)
        per_chunk = eff.reshape(2, 16, 4, 512).sum(-1)
        # state 0 (A ~ -1) keeps e^-0.4 .. e^-3.5 of itself over one chunk
        assert 0.4 < float(per_chunk.min()) and float(per_chunk.max()) < 3.5, kw
        assert float(eff.min()) > 0


# ---------------------------------------------------------------- the row-wise assertion

def test_row_error_sees_a_fault_in_one_small_row():
    ref = np.ones((2, 4, 64))
    ref[1, 2] *= 1e-4                     # a channel four orders below the tensor's maximum
    got = ref.copy()
    got[1, 2, 5] *= 1.01                  # 1 % off in that row: 1e-6 of the global maximum
    with pytest.raises(AssertionError, match=r"row \(1, 2\)"):
        SC.assert_close("out", got, ref)
    SC.assert_close("out", ref * (1 + 5e-5), ref)
    got = ref.copy()
    got[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match=r"row \(0, 0\)"):
        SC.assert_close("out", got, ref)


def test_bf16_bound_is_per_element():
    ref = np.ones((1, 1, 8))
    ref[0, 0, 1:] = 1e-2
    small_off = ref.copy()
    small_off[0, 0, 3] += 3e-4            # 3 % of a small element, 3e-4 of the row maximum
    with pytest.raises(AssertionError):
        SC.assert_close("out", small_off, ref, torch.bfloat16)
    SC.assert_close("out", ref * (1 + 2.0 ** -9), ref, torch.bfloat16)
    # last_state, dA, dD, ddelta_bias are written in fp32 and keep the fp32 bound in a bf16 run
    with pytest.raises(AssertionError):
        SC.assert_close("A", np.ones((2, 4)) * (1 + 2.0 ** -9), np.ones((2, 4)), torch.bfloat16)


# ---------------------------------------------------------------- mutants

# every multi-chunk shape of the GPU file whose oracle is cheap (the k > 1 and carry_par shapes
# cost seconds per oracle call; their inputs come from the same generator)
_SHAPES = SC.PER_CHANNEL + SC.MATRIX + SC.CARRY_BLK_PER + SC.OPTIONAL
# remembering one chunk can only be told from the truth two chunks on: shapes of three chunks
# whose third is a few positions long carry that difference in those few positions alone
_LONG = [s for s in _SHAPES if s[2] >= 4 * SC.CHUNK]


@pytest.fixture(scope="module")
def truth():
    cache = {}

    def get(shape):
        if shape not in cache:
            inp = SC.long_memory_inputs(*shape, SC.seed_for(*shape))
            cache[shape] = (inp, SC.oracle(inp))
        return cache[shape]
    return get


def _rejected(name, mutant, ref, factor):
    with pytest.raises(AssertionError):
        SC.assert_close(name, mutant, ref)
    r = SC.row_ratios(name, mutant, ref)
    assert r.min() >= factor, f"{name}: some row rejects the mutant at only {r.min():.3g}x the bound"
    # and the bf16 bound, though wider, still rejects it in every row
    assert SC.row_ratios(name, mutant, ref, torch.bfloat16).min() > 1.0
    return float(r.min())


@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_zero_carry_mutant_is_rejected_in_every_row(truth, shape):
    inp, ref = truth(shape)
    _rejected("out", SC.windowed(inp, True, "out", 0, 0), ref["out"], 10)
    _rejected("u", SC.windowed(inp, True, "u", 0, 0), ref["u"], 10)


@pytest.mark.parametrize("shape", _LONG, ids=lambda s: "x".join(map(str, s)))
def test_one_chunk_memory_mutant_is_rejected_in_every_row(truth, shape):
    inp, ref = truth(shape)
    # forward: restarted from a zero state at the start of the previous chunk
    _rejected("out", SC.windowed(inp, True, "out", 1, 0), ref["out"], 10)
    # backward: the adjoint chain remembers the next chunk only
    _rejected("u", SC.windowed(inp, True, "u", 0, 1), ref["u"], 10)


def test_old_inputs_make_carries_invisible():
    """The draw of tests/test_gpu_selective_scan.py (steps near 0.3, A = -exp(0.5 randn)): the
    same one-chunk-memory mutant is indistinguishable from the truth, which is why those tests
    cannot see a wrong carry."""
    b, d, l, n = 2, 16, 1300, 16
    g = torch.Generator().manual_seed(l + n)
    inp = {"u": torch.randn(b, d, l, generator=g),
           "delta": torch.randn(b, d, l, generator=g) * 0.5 - 1.0,
           "A": -torch.exp(torch.randn(d, n, generator=g) * 0.5),
           "B": torch.randn(b, n, l, generator=g), "C": torch.randn(b, n, l, generator=g),
           "D": torch.randn(d, generator=g), "z": torch.randn(b, d, l, generator=g),
           "delta_bias": torch.randn(d, generator=g) * 0.1, "dout": None}
    ref = SC.oracle(inp)
    mutant = SC.windowed(inp, True, "out", 1, 0)
    assert SC.row_ratios("out", mutant, ref["out"]).max() < 1e-6
