"""GPU: every dispatch path of dna_amd/csrc/selective_scan.hip against the float64 C oracle, on
long-memory inputs (tests/scan_check.py: a chunk's output depends on many chunks before it, so a
wrong chunk carry is visible), forward with last_state and the backward of every input, with the
error taken per row. Each case asserts through dna_selective_scan_plan that its shape takes the
path it is named for.

Bounds (scan_check.assert_close): fp32 -- 1e-4 of the row maximum for out / last_state, 1e-3 for
every gradient; bf16 -- against the oracle on the bf16-rounded inputs, per element
2^-8 |ref| + the fp32 bound x row maximum for what is written in bf16, the fp32 bound for dA, dD,
ddelta_bias and last_state. The measured figures are in DESIGN.md ("Selective scan: dispatch
paths under test")."""
import pytest
import torch

from tests import scan_check as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
_DT = {F32: "fp32", BF16: "bf16"}
_refs = {}


def _reference(shape, dtype, softplus=True, D=True, z=True, bias=True):
    """(inputs as the run sees them, float64 reference); small cases are kept for the tests that
    share them."""
    key = (shape, dtype, softplus, D, z, bias)
    if key in _refs:
        return _refs[key]
    inp = SC.long_memory_inputs(*shape, SC.seed_for(*shape), softplus=softplus, bias=bias)
    if not D:
        inp["D"] = None
    if not z:
        inp["z"] = None
    inp = SC.rounded(inp, dtype)
    ref = SC.oracle(inp, softplus)
    if inp["u"].numel() * shape[3] <= 1 << 21:
        _refs[key] = (inp, ref)
    return inp, ref


def _dev(t, dtype, misalign):
    """t on the device as a leaf; misalign: a contiguous view that starts one element into a
    larger storage (so .contiguous() keeps it and its pointer is not 16-B aligned)."""
    if t is None:
        return None
    if misalign:
        store = torch.empty(t.numel() + 8, device=DEV, dtype=dtype)
        v = store[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
    else:
        v = t.to(DEV, dtype)
        assert v.data_ptr() % 16 == 0
    return v.requires_grad_(True)


def _check(shape, dtype, softplus=True, D=True, z=True, bias=True, misalign=False, label=""):
    from dna_amd.mamba import selective_scan_fn
    inp, ref = _reference(shape, dtype, softplus, D, z, bias)
    t = {k: _dev(inp[k], dtype, misalign) for k in ("u", "delta", "B", "C", "z")}
    t.update({k: _dev(inp[k], F32, False) for k in ("A", "D", "delta_bias")})
    out, last = selective_scan_fn(t["u"], t["delta"], t["A"], t["B"], t["C"], D=t["D"], z=t["z"],
                                  delta_bias=t["delta_bias"], delta_softplus=softplus,
                                  return_last_state=True)
    assert out.dtype == dtype and last.dtype == F32
    out.backward(inp["dout"].to(DEV, dtype))
    torch.cuda.synchronize()
    got = {"out": out.detach(), "last_state": last}
    for k, v in t.items():
        if v is not None:
            assert v.grad is not None and v.grad.dtype == v.dtype, k
            got[k] = v.grad
    assert set(got) == set(ref)
    report, failures = {}, []
    for k in ref:
        try:
            SC.assert_close(k, got[k].float().cpu().numpy(), ref[k], dtype, report=report)
        except AssertionError as e:
            failures.append(str(e))
    # every figure before any assertion: worst row, in units of the row maximum for tensors under
    # the fp32 bound, of the per-element allowance (times the bound) for bf16-written ones
    fwd = max(report[k] for k in SC.FORWARD)
    grad = max(v for k, v in report.items() if k not in SC.FORWARD)
    print(f"SCANPATH {label} {'x'.join(map(str, shape))} {_DT[dtype]} fwd {fwd:.2e} grad {grad:.2e} "
          + " ".join(f"{k}={v:.1e}" for k, v in report.items()))
    assert not failures, "\n".join(failures)


def _ids(v):
    return _DT.get(v) or ("x".join(map(str, v)) if isinstance(v, tuple) else str(v))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
@pytest.mark.parametrize("shape", SC.PER_CHANNEL, ids=_ids)
def test_per_channel_kernels(shape, dtype):
    """fwd_kernel / bwd_kernel (dim % 8 != 0) over several chunks."""
    assert not SC.plan(*shape)["chunked"]
    _check(shape, dtype, label="per_channel")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
@pytest.mark.parametrize("shape", SC.MATRIX, ids=_ids)
def test_chunked_k1_matrix(shape, dtype):
    """sum / carry_blk / chunk kernels at one channel per wave: N in {4, 8, 16} (the three state
    loops of chunk_bwd_kernel) x VEC (len 4104) / not VEC (len 4099)."""
    p = SC.plan(*shape)
    assert p["chunked"] and p["k"] == 1 and p["nch"] == 9 and not p["carry_par"]
    _check(shape, dtype, label="k1_vec" if shape[2] % 8 == 0 else "k1_novec")


@pytest.mark.parametrize("shape,nch", list(zip(SC.CARRY_BLK_PER, (18, 66))), ids=_ids)
def test_carry_blk_several_chunks_per_segment(shape, nch):
    """carry_blk_kernel with more chunks than chain segments (256 / N): per > 1."""
    p = SC.plan(*shape)
    assert p["chunked"] and p["nch"] == nch and not p["carry_par"]
    assert nch > 256 // shape[3]
    _check(shape, F32, label="carry_blk_per")


@pytest.mark.parametrize("k,shape,dtype", [(k, s, F32) for k, s in SC.K_WAVE] +
                         [(8, SC.K_WAVE[2][1], BF16)], ids=_ids)
def test_channels_per_wave(k, shape, dtype):
    """k = 2, 4, 8 channels per wave: the j loops of all four chunk kernels, their prefetch of
    channel j + 1 and the dB / dC accumulators carried across j in LDS."""
    p = SC.plan(*shape)
    assert p["chunked"] and p["k"] == k and p["nch"] == 2 and not p["carry_par"]
    _check(shape, dtype, label=f"k{k}")


@pytest.mark.parametrize("shape,dtype", [(s, F32) for s in SC.CARRY_PAR] + [(SC.CARRY_PAR[0], BF16)],
                         ids=_ids)
def test_carry_par_kernel(shape, dtype):
    """carry_par_kernel: more chunks than carry_blk_kernel can hold in LDS."""
    p = SC.plan(*shape)
    assert p["chunked"] and p["carry_par"] and p["k"] == 1
    _check(shape, dtype, label="carry_par")


_OPTIONS = {"no_D": dict(D=False), "no_z": dict(z=False), "no_delta_bias": dict(bias=False),
            "no_softplus": dict(softplus=False),
            "none_of_them": dict(D=False, z=False, bias=False, softplus=False)}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
@pytest.mark.parametrize("opt", list(_OPTIONS))
@pytest.mark.parametrize("shape", SC.OPTIONAL, ids=_ids)
def test_optional_arguments(shape, opt, dtype):
    """D / z / delta_bias absent and delta_softplus off, one at a time and together, on the
    chunked VEC kernels (dim 8: `a.z ? a.z : a.u`, lane_param) and the per-channel ones (dim 5)."""
    assert SC.plan(*shape)["chunked"] == (shape[1] % 8 == 0) and shape[2] % 8 == 0
    _check(shape, dtype, label=opt, **_OPTIONS[opt])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
def test_rows_of_whole_vectors_at_an_unaligned_base(dtype):
    """len % 8 == 0 but u, delta, z, B, C start one element off a 16-B boundary: the host must
    choose the scalar row I/O and stagef its element-wise fallback; same bounds as aligned."""
    shape = SC.OPTIONAL[0]
    assert SC.plan(*shape)["chunked"] and shape[2] % 8 == 0
    _check(shape, dtype, misalign=True, label="misaligned")
