"""CPU: the checker of tests/test_gpu_fftconv_paths.py checked itself (tests/fft_check.py), at
L = 64 and L = 4,096, causal and bidirectional: the plain fp32 FFT passes its own bound, the bf16
rounding of the oracle passes the bf16 bound, and every planted error -- one element moved by 1e-5
of its row maximum, one row scaled by 1 + 2e-6, the two rows of a pair swapped, du read at offset 0
instead of pad_before, bf16 truncation instead of rounding -- is rejected by the same assertion
the GPU tests use, with a message that names the tensor and the row. Also the plan query at every
size and the derivation constants of the dbias bound."""
import numpy as np
import pytest
import torch

from oracle import hyena_ref as H
from tests import fft_check as FC

B, D = 3, 3
LENS = (64, 4096)


@pytest.fixture(scope="module")
def truth():
    cache = {}

    def get(L, bi, dtype=torch.float32):
        key = (L, bi, dtype)
        if key not in cache:
            cache[key] = FC.reference(B, D, L, bi, dtype)
        return cache[key]
    return get


def _cases():
    return [(L, bi) for L in LENS for bi in (False, True)]


@pytest.mark.parametrize("L,bi", _cases())
def test_ref32_passes_its_own_bound_and_is_a_few_ulp(truth, L, bi):
    inp, ref, e32 = truth(L, bi)
    r32 = FC.ref32(inp, bi)
    report, failures = FC.check_all(r32, ref, e32)
    assert not failures, failures
    for n in FC.ROW_AXES:
        assert report[n] == pytest.approx(e32[n])
        # a plain fp32 FFT of this formula: a few 2^-24 of the row maximum, at every size -- so
        # 4 x e32 stays near 1e-6, the regression the bound is there to catch
        assert 2.0 ** -25 < e32[n] < 5e-7, (n, e32[n])
    # its plain fp32 sum of B*L products also stays inside the bound derived for the kernel's order
    assert report["dbias"] <= e32["dbias"][0]


@pytest.mark.parametrize("L,bi", _cases())
def test_one_element_moved_is_rejected(truth, L, bi):
    _, ref, e32 = truth(L, bi)
    for name, idx, row in (("out", (2, 1, L - 1), r"row \(2, 1\)"), ("du", (0, 2, 0), r"row \(0, 2\)"),
                           ("dk", (1, L // 2), r"row \(1,\)")):
        got = ref[name].copy()
        got[idx] += 1e-5 * np.abs(ref[name][idx[:-1]]).max()
        with pytest.raises(AssertionError, match=rf"^{name}: {row}"):
            FC.assert_close(name, got, ref[name], e32[name])
        # also in a bf16 run for dk (an fp32 output); out / du there allow 2^-8 |ref| per element
        if name == "dk":
            with pytest.raises(AssertionError, match=rf"^dk: {row}"):
                FC.assert_close(name, got, ref[name], e32[name], torch.bfloat16)


@pytest.mark.parametrize("L,bi", _cases())
def test_one_row_scaled_is_rejected(truth, L, bi):
    _, ref, e32 = truth(L, bi)
    for name, row, pat in (("out", (1, 2), r"row \(1, 2\)"), ("du", (2, 0), r"row \(2, 0\)"),
                           ("dk", (2,), r"row \(2,\)")):
        got = ref[name].copy()
        got[row] *= 1 + 2e-6
        with pytest.raises(AssertionError, match=rf"^{name}: {pat}"):
            FC.assert_close(name, got, ref[name], e32[name])
    got = ref["dbias"].copy()
    got[1] += 1e-5 * e32["dbias"][1][1]   # 1e-5 of sum |dy u|: ~170 x 2^-24
    with pytest.raises(AssertionError, match=r"^dbias: row \(1,\)"):
        FC.assert_close("dbias", got, ref["dbias"], e32["dbias"])


@pytest.mark.parametrize("L,bi", _cases())
def test_swapped_pair_is_rejected(truth, L, bi):
    _, ref, e32 = truth(L, bi)
    for name in ("out", "du"):
        got = ref[name].copy()
        got[[0, 1]] = got[[1, 0]]          # batches 0 and 1 share one complex sequence
        with pytest.raises(AssertionError, match=rf"^{name}: row \((0|1), \d\)"):
            FC.assert_close(name, got, ref[name], e32[name])
    got = ref["dk"].copy()
    got[[0, 1]] = got[[1, 0]]              # channels 0 and 1 of the filter pair
    with pytest.raises(AssertionError, match=r"^dk: row \((0|1),\)"):
        FC.assert_close("dk", got, ref["dk"], e32["dk"])


@pytest.mark.parametrize("L", LENS)
def test_du_read_at_offset_zero_is_rejected(truth, L):
    inp, ref, e32 = truth(L, True)
    a = {k: v.numpy().astype(np.float64) for k, v in inp.items()}
    N, pb = 2 * L, H.pad_before(L, True)
    assert pb == L // 2
    kf = np.fft.rfft(a["k"], n=N) / N
    dut = np.fft.irfft(np.fft.rfft(a["dy"], n=N) * np.conj(kf), n=N, norm="forward")
    right = dut[..., pb:pb + L] + a["dy"] * a["bias"]
    assert np.abs(right - ref["du"]).max() < 1e-12
    with pytest.raises(AssertionError, match=r"^du: row \(\d, \d\)"):
        FC.assert_close("du", dut[..., :L] + a["dy"] * a["bias"], ref["du"], e32["du"])


def _truncate_bf16(x):
    bits = np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return bits.view(np.float32)


@pytest.mark.parametrize("L,bi", _cases())
def test_bf16_rounding_passes_and_truncation_fails(truth, L, bi):
    _, ref, e32 = truth(L, bi, torch.bfloat16)
    for name in ("out", "du"):
        rn = torch.from_numpy(ref[name]).to(torch.bfloat16).double().numpy()
        FC.assert_close(name, rn, ref[name], e32[name], torch.bfloat16)
        with pytest.raises(AssertionError, match=rf"^{name}: row \(\d, \d\)"):
            FC.assert_close(name, _truncate_bf16(ref[name]), ref[name], e32[name], torch.bfloat16)
        # and the fp32 bound rejects a bf16-rounded tensor outright
        with pytest.raises(AssertionError):
            FC.assert_close(name, rn, ref[name], e32[name])


def test_inputs_are_order_one_in_every_row_and_channel():
    inp = FC.inputs(B, D, 4096, False, 7)
    for n in ("u", "dy", "k"):
        m = inp[n].abs().amax(-1)
        assert float(m.min()) > 1.0 and float(m.max()) < 8.0, n
    assert inp["bias"].shape == (D, 1) and all(v.dtype == torch.float32 for v in inp.values())
    r = FC.rounded(inp, torch.bfloat16)
    assert torch.equal(r["u"], inp["u"].bfloat16().float()) and torch.equal(r["k"], inp["k"])


def test_dbias_terms_follow_the_kernel_constants():
    # per = ceil(B L / 32); n_t = VE ceil(ceil(per / VE) / 512), largest over VE = 1, 4, 8
    assert FC.dbias_terms(1, 64) == 8 + 44            # per = 2: one 8-wide load per thread
    assert FC.dbias_terms(3, 4096) == 8 + 44          # per = 384
    assert FC.dbias_terms(3, 131072) == 24 + 44       # per = 12288 = 3 * 4096
    assert FC.dbias_terms(3, 65536) == 16 + 44        # per = 6144


# ---------------------------------------------------------------- dna_fftconv_plan

# L -> logN, logM1, logM2, fixed_ln, col_group, row_group, rowbwd_group: N = 2L = M1 * M2 with
# M2 = min(N / 2, 512); 8192 points per block in the column and row passes (groups of
# min(8192 / M1, M2) columns, min(8192 / M2, M1) rows), 4096 in the backward's row pass
_PLAN = {
    64: (7, 1, 6, 0, 6, 1, 1), 128: (8, 1, 7, 0, 7, 1, 1), 256: (9, 1, 8, 0, 8, 1, 1),
    512: (10, 1, 9, 0, 9, 1, 1), 1024: (11, 2, 9, 0, 9, 2, 2), 2048: (12, 3, 9, 0, 9, 3, 3),
    4096: (13, 4, 9, 0, 9, 4, 3), 8192: (14, 5, 9, 0, 8, 4, 3), 16384: (15, 6, 9, 0, 7, 4, 3),
    32768: (16, 7, 9, 16, 6, 4, 3), 65536: (17, 8, 9, 17, 5, 4, 3), 131072: (18, 9, 9, 18, 4, 4, 3),
}


@pytest.mark.parametrize("L", sorted(_PLAN))
def test_plan_query_at_every_size(L, monkeypatch):
    monkeypatch.delenv("DNA_FFT_GENERIC", raising=False)
    p = FC.plan(L)
    assert tuple(p[k] for k in FC.PLAN_KEYS) == _PLAN[L]
    assert p["logM1"] + p["logM2"] == p["logN"] and (1 << p["logN"]) == 2 * L
    from dna_amd import _native as N
    assert N.lib().dna_fftconv_kspec_elems(L) == 2 << p["logN"]


@pytest.mark.parametrize("L", [0, -64, 32, 63, 96, 262144])
def test_plan_query_refuses_unsupported_lengths(L):
    from dna_amd import _native as N
    with pytest.raises(N.NativeError, match="dna_fftconv_plan"):
        FC.plan(L)
    assert N.lib().dna_fftconv_plan(64, None) != 0
    assert N.lib().dna_abi_version() == 1 and N.lib().dna_abi_revision() >= 9
