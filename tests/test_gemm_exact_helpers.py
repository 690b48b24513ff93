"""CPU: the host-side logic of tests/test_gpu_gemm_exact.py on CPU tensors -- the integer operand
builder, the exactness precondition, the zero-tolerance reference, the localising failure
messages on deliberately corrupted copies, and the restated dispatch condition of the shape
lists (every K-step count, ragged row tiles, N off the tile, more than two units per workgroup)."""
import pytest
import torch

import test_gpu_gemm_exact as E


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def test_int_operand_range_and_row_scale():
    g = _gen()
    t = E._int_operand(64, 96, 255, g)
    assert t.dtype == torch.bfloat16 and t.shape == (64, 96)
    d = t.double()
    assert bool((d == d.round()).all()) and float(d.abs().max()) == 255.0  # all 8 bits in use
    rexp = torch.randint(-8, 9, (64,), generator=g)
    s = E._int_operand(64, 96, 2, g, rexp).double() * E._pow2(-rexp)[:, None]
    assert bool((s == s.round()).all()) and float(s.abs().max()) == 2.0


def test_exact_ref_matches_integer_arithmetic_and_rounds_once():
    g = _gen(1)
    a = E._int_operand(37, 200, 255, g).double()
    b = E._int_operand(200, 24, 2, g).double()
    bias = torch.randint(-64, 65, (24,), generator=g).double()
    want = a.long() @ b.long() + bias.long()
    f = E._exact_ref(a, b, bias, torch.float32)
    assert f.dtype == torch.float32 and torch.equal(f.long(), want)
    h = E._exact_ref(a, b, bias, torch.bfloat16)
    assert h.dtype == torch.bfloat16 and torch.equal(h, want.float().bfloat16())
    assert not torch.equal(h.double(), want.double())  # sums past 8 bits: the rounding is exercised
    rexp = torch.randint(-8, 9, (37,), generator=g)
    hs = E._exact_ref(a, b, None, torch.bfloat16, rexp)
    assert torch.equal(hs.double(), (a.long() @ b.long()).float().bfloat16().double()
                       * E._pow2(rexp)[:, None])


def test_exact_ref_rejects_inexact_inputs():
    a = torch.full((2, 70000), 255.0, dtype=torch.float64)
    b = torch.full((70000, 2), 2.0, dtype=torch.float64)
    with pytest.raises(AssertionError, match="2\\^24"):
        E._exact_ref(a, b, None, torch.bfloat16)  # 70000 * 255 * 2 > 2^24
    with pytest.raises(AssertionError, match="2\\^24"):
        E._exact_ref(a[:, :32896], b[:32896], torch.tensor([257.0, 0.0]).double(), torch.float32)
    E._exact_ref(a[:, :32896], b[:32896], None, torch.float32)  # 32896 * 510 = 2^24 - 256: allowed
    with pytest.raises(AssertionError, match="integers"):
        E._exact_ref(torch.full((2, 4), 0.5).double(), b[:4], None, torch.float32)
    with pytest.raises(AssertionError, match="row scale"):
        E._exact_ref(a[:, :8], b[:8], torch.zeros(2).double(), torch.bfloat16, torch.zeros(2).long())


def test_assert_same_localises_a_corrupted_copy():
    want = torch.arange(600 * 520, dtype=torch.float32).reshape(600, 520).bfloat16()
    E._assert_same(want.clone(), want)
    got = want.clone()
    got[300:316, 400:416] = -1.0  # one 16 x 16 sub-tile of tile (1, 1), quadrant (0, 1)
    got[599, 3] = float("nan")    # tile (2, 0), quadrant (0, 0)
    with pytest.raises(AssertionError) as e:
        E._assert_same(got, want, what="probe")
    msg = str(e.value)
    assert msg.startswith("probe: 257 of 312000 elements wrong; first at (300, 400)")
    assert "rows [300, 599] x cols [3, 415]" in msg
    assert "in 2 (tile, quadrant)" in msg
    assert "tile (1, 1) quadrant (0, 1)" in msg and "tile (2, 0) quadrant (0, 0)" in msg
    assert "got -1.0, want" in msg
    assert "tile (1, 3) quadrant (0, 0)" in E._diff_report(got, want, tile=(256, 128))  # 128-column units


def test_assert_within_localises_and_fails_on_nan():
    g = _gen(2)
    a, b = torch.randn(300, 64, generator=g).double(), torch.randn(64, 264, generator=g).double()
    bias = torch.randn(264, generator=g).double()
    ref, bound = E._bf16_bound(a, b, bias, 64)
    assert torch.equal(ref, a @ b + bias) and bool((bound > 0).all())
    got = ref.float().bfloat16()
    E._assert_within(got, ref, bound)  # a correctly rounded result is inside the bound
    bad = got.clone()
    bad[257, 260] = (ref[257, 260] * (1 + 2.0 ** -6) + 1e-3).float().bfloat16()  # 4x the rounding
    with pytest.raises(AssertionError, match=r"1 of 79200 elements wrong; first at \(257, 260\).*"
                                             r"tile \(1, 1\) quadrant \(0, 0\).*> bound"):
        E._assert_within(bad, ref, bound)
    bad = got.clone()
    bad[0, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"first at \(0, 0\)"):
        E._assert_within(bad, ref, bound)
    r32, b32 = E._f32_bound(a.t(), a, 300)
    E._assert_within((a.t() @ a).float(), r32, b32)


def test_shape_lists_reach_the_paths_they_name():
    assert all(E._fwd_path(Nn, K) == "p2" for _, Nn, K in E.FWD_P2)
    assert all(E._fwd_path(Nn, K) == "p0" for _, Nn, K in E.FWD_P0)
    assert all(E._fwd_path(Nn, K) == "np" for _, Nn, K in E.FWD_NP)
    assert E._fwd_path(8448, 128) == "np" and E._fwd_path(128, 192, wide=256) == "p0"
    assert {K // 64 for _, _, K in E.FWD_P2} == {2, 4} and {K // 64 for _, _, K in E.FWD_P0} == {3, 5}
    assert {K // 64 for _, _, K in E.FWD_NP} == {1, 3}
    assert {Nn // 64 for _, Nn, _ in E.DGRAD} >= {1, 2, 3, 12}
    for shapes in (E.FWD_P2, E.FWD_P0, E.FWD_NP, E.DGRAD):
        assert any(M % 256 for M, _, _ in shapes)          # a ragged last row tile
    assert any(Nn % 256 for _, Nn, _ in E.FWD_NP) and any(K % 256 for _, _, K in E.DGRAD)
    # 17 row tiles (17 % 8 != 0) x 32 column tiles > 2 x 256 workgroups on the MI355X
    assert (E.MANY_M + 255) // 256 == 17 and E.MANY_N <= 8192
    assert 17 * (E.MANY_N // 256) > 2 * 256
    # dna_linear_wgrad_p: odd and even K-step counts, T off the 64-row step, the smallest legal T
    steps = {(T + 63) // 64 for T in E.WGRAD_P_T}
    assert min(E.WGRAD_P_T) == 128 and {2, 3, 4} <= steps and any(T % 64 for T in E.WGRAD_P_T)
