"""Packed (variable-length) ALiBi attention, csrc/attention_varlen.hip, against an fp64 torch
restatement that is dense per sequence and takes its bias from the tokens' columns. GPU only.

Bounds are those of tests/test_gpu_kernels.py for the padded kernel: forward maximum absolute
error below 2e-5 (fp32) / 3e-2 (bf16) on N(0, 1) inputs, backward below 1e-4 / 6e-2 times
max(|reference gradient|, 1). The reference sees the inputs the kernel sees (bf16-rounded in
bf16), in float64. Every row of dqkv is compared, on a NaN-prefilled buffer: an unwritten row fails.
"""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 64
FWD_TOL = {torch.float32: 2e-5, torch.bfloat16: 3e-2}
BWD_TOL = {torch.float32: 1e-4, torch.bfloat16: 6e-2}
DTYPES = [torch.float32, torch.bfloat16]

# heads, lengths
CASES = {
    # length 1, a sub-tile, an exact tile, a tile plus one, several tiles with a ragged tail,
    # and an unaligned end of the buffer (T = 530)
    "A": (2, [1, 7, 63, 64, 65, 130, 200]),
    "B": (12, [72, 72, 40, 72, 7]),  # the fine-tuning fixture batch
    "C1": (1, [300, 5]),
    "C2": (1, [5, 300]),
    "D": (3, [1]),
}


def _index(lens, positions=None):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    pos = None if positions is None else torch.tensor(positions, dtype=torch.int32, device=DEV)
    return SimpleNamespace(cu_seqlens=torch.tensor(cu, dtype=torch.int32, device=DEV),
                           positions=pos, batch=len(lens), max_seqlen=max(lens), total=cu[-1],
                           sq_sum=sum(n * n for n in lens), lens=list(lens))


def _slopes(H):
    from dna_amd.config import alibi_slopes
    return torch.tensor(alibi_slopes(H), dtype=torch.float32, device=DEV)


def _inputs(T, H, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(T, 3 * H * D, generator=g).to(DEV).to(dtype)
    dout = torch.randn(T, H * D, generator=g).to(DEV).to(dtype)
    return qkv, dout


def _reference(qkv, dout, idx, H):
    """-> (out [T, H*D], lse [H, T], dqkv [T, 3*H*D]) in float64."""
    x = qkv.double().clone().requires_grad_(True)
    slopes = _slopes(H).double()
    outs, lses, r0 = [], [], 0
    for n in idx.lens:
        rows = x[r0:r0 + n].view(n, 3, H, D)
        q, k, v = (rows[:, t].transpose(0, 1) for t in range(3))  # [H, n, D]
        pos = (torch.arange(n, device=DEV) if idx.positions is None
               else idx.positions[r0:r0 + n]).double()
        bias = -slopes[:, None, None] * (pos[:, None] - pos[None, :]).abs()
        s = q @ k.transpose(-1, -2) / math.sqrt(D) + bias
        lses.append(torch.logsumexp(s, -1))
        outs.append((torch.softmax(s, -1) @ v).transpose(0, 1).reshape(n, H * D))
        r0 += n
    out = torch.cat(outs)
    out.backward(dout.double())
    return out.detach(), torch.cat(lses, 1).detach(), x.grad


def _raw(qkv, dout, idx, H, out=None, dqkv=None):
    """The C entry points as they are -> (out, lse, dqkv); out / dqkv may be caller buffers."""
    from dna_amd import _native as N
    T, dt = idx.total, 1 if qkv.dtype == torch.bfloat16 else 0
    slopes = _slopes(H)
    if out is None:
        out = torch.full((T, H * D), float("nan"), device=DEV, dtype=qkv.dtype)
    if dqkv is None:
        dqkv = torch.full((T, 3 * H * D), float("nan"), device=DEV, dtype=qkv.dtype)
    lse = torch.full((H, T), float("nan"), device=DEV)
    pos = None if idx.positions is None else idx.positions.data_ptr()
    scale = 1.0 / math.sqrt(D)
    N.call("dna_attn_varlen_fwd", qkv.data_ptr(), idx.cu_seqlens.data_ptr(), pos,
           slopes.data_ptr(), idx.batch, T, idx.max_seqlen, H, D, dt, scale, out.data_ptr(),
           lse.data_ptr(), N.stream_ptr())
    ws = torch.empty(N.lib().dna_attn_varlen_bwd_workspace(idx.batch, T, idx.max_seqlen, H),
                     device=DEV, dtype=torch.uint8)
    N.call("dna_attn_varlen_bwd", qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
           idx.cu_seqlens.data_ptr(), pos, slopes.data_ptr(), idx.batch, T, idx.max_seqlen, H, D,
           dt, scale, dqkv.data_ptr(), ws.data_ptr(), N.stream_ptr())
    return out, lse, dqkv


_CACHE = {}


def _case(name, dtype):
    """Inputs, index and the fp64 reference of one case, computed once and left unchanged."""
    key = (name, dtype)
    if key not in _CACHE:
        H, lens = CASES[name]
        idx = _index(lens)
        qkv, dout = _inputs(idx.total, H, dtype, seed=sorted(CASES).index(name))
        _CACHE[key] = (H, idx, qkv, dout, _reference(qkv, dout, idx, H))
    return _CACHE[key]


def _check(tag, dtype, got, ref):
    out, lse, dqkv = got
    rout, rlse, rgrad = ref
    e_out = (out.double() - rout).abs().max().item()
    e_lse = (lse.double() - rlse).abs().max().item()
    gscale = max(rgrad.abs().max().item(), 1.0)
    e_grad = (dqkv.double() - rgrad).abs().max().item()
    print(f"{tag} {dtype}: out err {e_out:.3e}, lse err {e_lse:.3e}, dqkv err {e_grad:.3e} "
          f"(scale {gscale:.3f})")
    assert e_out < FWD_TOL[dtype], e_out  # NaN (an unwritten row) fails every comparison
    assert e_lse < FWD_TOL[dtype], e_lse
    assert e_grad < BWD_TOL[dtype] * gscale, (e_grad, gscale)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_and_backward_vs_fp64(name, dtype):
    from dna_amd import functional as DF
    H, idx, qkv, dout, ref = _case(name, dtype)
    x = qkv.clone().requires_grad_(True)
    out = DF.alibi_attention_varlen(x, idx, _slopes(H), H)
    assert out.shape == (idx.total, H * D) and out.dtype == dtype
    out.backward(dout)
    # the lse comes from the C entry point (the autograd function keeps its own)
    _, lse, dqkv = _raw(qkv, dout, idx, H)
    assert torch.equal(dqkv, x.grad)
    _check(name, dtype, (out.detach(), lse, x.grad), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_positions_shift_is_exact_and_gaps_count(dtype):
    H, idx, qkv, dout, _ = _case("A", dtype)
    col = torch.cat([torch.arange(n) for n in idx.lens])
    a = _raw(qkv, dout, idx, H)
    b = _raw(qkv, dout, _index(idx.lens, (col + 11).tolist()), H)
    for x, y in zip(a, b):  # |i - j| of a shifted row is the same float: bit-identical
        assert torch.equal(x, y)
    # a [PAD] inside a row is no shift: the kernel takes the columns it is given
    H = 2
    gap = _index([6, 3], [0, 1, 2, 9, 10, 40, 0, 1, 2])
    qkv, dout = _inputs(9, H, dtype, seed=21)
    got = _raw(qkv, dout, gap, H)
    _check("gaps", dtype, got, _reference(qkv, dout, gap, H))
    plain = _raw(qkv, dout, _index([6, 3]), H)
    assert not torch.equal(got[0][:6], plain[0][:6])
    assert torch.equal(got[0][6:], plain[0][6:])  # the second sequence has no gap


@pytest.mark.parametrize("dtype", DTYPES)
def test_neighbouring_memory_is_neither_read_nor_written(dtype):
    """qkv, out, dout and dqkv are the first T rows of buffers 256 rows longer. The input tails
    hold NaN, the output tails a sentinel: the results are bit-identical to a run on exact-size
    buffers and the output tails keep the sentinel."""
    H, idx, qkv, dout, _ = _case("A", dtype)
    T = idx.total
    want = _raw(qkv, dout, idx, H)

    def longer(t, fill):
        big = torch.full((T + 256, t.shape[1]), fill, device=DEV, dtype=dtype)
        big[:T] = t
        return big

    bq, bd = longer(qkv, float("nan")), longer(dout, float("nan"))
    bo = torch.full((T + 256, H * D), 7.0, device=DEV, dtype=dtype)
    bg = torch.full((T + 256, 3 * H * D), 7.0, device=DEV, dtype=dtype)
    bo[:T] = float("nan")
    bg[:T] = float("nan")
    out, lse, dqkv = _raw(bq[:T], bd[:T], idx, H, out=bo[:T], dqkv=bg[:T])
    assert out.data_ptr() == bo.data_ptr() and dqkv.data_ptr() == bg.data_ptr()
    assert torch.equal(out, want[0]) and torch.equal(lse, want[1]) and torch.equal(dqkv, want[2])
    assert bool((bo[T:] == 7.0).all()) and bool((bg[T:] == 7.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_agrees_with_the_padded_kernel(name, dtype):
    """The same sequences right-padded through DF.alibi_attention: valid rows agree within the
    bounds both kernels are held to against the same reference."""
    from dna_amd import functional as DF
    H, idx, qkv, dout, ref = _case(name, dtype)
    b, S = idx.batch, (idx.max_seqlen + 63) // 64 * 64
    rows = torch.cat([n * S + torch.arange(L) for n, L in enumerate(idx.lens)]).to(DEV)
    pq = torch.zeros(b * S, 3 * H * D, device=DEV, dtype=dtype)
    pd = torch.zeros(b * S, H * D, device=DEV, dtype=dtype)
    pq[rows], pd[rows] = qkv, dout
    kv = torch.zeros(b * S, dtype=torch.uint8, device=DEV)
    kv[rows] = 1
    x = pq.clone().requires_grad_(True)
    out = DF.alibi_attention(x, kv, _slopes(H), b, S, H)
    out.backward(pd)
    got = _raw(qkv, dout, idx, H)
    e_out = (out.detach()[rows].double() - got[0].double()).abs().max().item()
    e_grad = (x.grad[rows].double() - got[2].double()).abs().max().item()
    gscale = max(ref[2].abs().max().item(), 1.0)
    print(f"{name} {dtype}: packed vs padded out {e_out:.3e}, dqkv {e_grad:.3e} (scale {gscale:.3f})")
    assert e_out < FWD_TOL[dtype], e_out
    assert e_grad < BWD_TOL[dtype] * gscale, (e_grad, gscale)


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_is_deterministic(dtype):
    H, idx, qkv, dout, _ = _case("A", dtype)
    a, b = _raw(qkv, dout, idx, H), _raw(qkv, dout, idx, H)
    for x, y in zip(a, b):
        assert not torch.isnan(x).any() and torch.equal(x, y)


def test_torch_ops_match_the_c_entry_points():
    import dna_amd.ops  # noqa: F401  (registers torch.ops.dna_amd.*)
    H, idx, qkv, dout, _ = _case("B", torch.bfloat16)
    want = _raw(qkv, dout, idx, H)
    out, lse, dqkv = torch.empty_like(want[0]), torch.empty_like(want[1]), torch.empty_like(want[2])
    scale = 1.0 / math.sqrt(D)
    torch.ops.dna_amd.attn_varlen_fwd(qkv, idx.cu_seqlens, None, _slopes(H), idx.max_seqlen, H,
                                      scale, out, lse)
    torch.ops.dna_amd.attn_varlen_bwd(qkv, out, dout, lse, idx.cu_seqlens, None, _slopes(H),
                                      idx.max_seqlen, H, scale, dqkv)
    assert torch.equal(out, want[0]) and torch.equal(lse, want[1]) and torch.equal(dqkv, want[2])
    with pytest.raises(RuntimeError, match="int32|dtype"):
        torch.ops.dna_amd.attn_varlen_fwd(qkv, idx.cu_seqlens.long(), None, _slopes(H),
                                          idx.max_seqlen, H, scale, out, lse)
