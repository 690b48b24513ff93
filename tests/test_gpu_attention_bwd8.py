"""The 8-wave fused attention backward (two waves per SIMD, S = 256 / 512) through
dna_attn_bwd_var, against fp32 PyTorch and against the 4-wave kernel on identical inputs. GPU only.

Shapes: the smallest at which the 8-wave kernel can go wrong -- S = 512 (two key blocks per wave)
with a pad tail of 37 keys that splits a 32-key block, S = 512 with several (batch, head)
workgroups, S = 256 (one key block per wave). Every case with and without the fused
bias-gradient partial rows."""
import functools
import math

import pytest
import torch

from oracle import bert_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(512, 1, 1, ((0, 512 - 37),)), (512, 2, 3, ((0, 400),)), (256, 2, 2, ((1, 200),))]


def _ref_attention(qkv, key_valid, H, b, S):
    """fp32 PyTorch attention with the reference bias (bert_layers.py:167-178, :421-448)."""
    T, three_hd = qkv.shape
    D = three_hd // (3 * H)
    x = qkv.float().view(b, S, 3, H, D)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    bias = bert_ref.attention_bias(key_valid.view(b, S).bool().cpu(), H).to(qkv.device)
    s = q @ k.transpose(-1, -2) / math.sqrt(D) + bias
    p = torch.softmax(s, -1)
    return (p @ v).transpose(1, 2).reshape(T, H * D)


@functools.lru_cache(maxsize=None)
def _inputs(S, b, H, pads):
    """Inputs, the kernel forward (out, lse) and the fp32 reference gradient, once per case."""
    from dna_amd import _native as N
    from dna_amd.config import alibi_slopes
    g = torch.Generator(device="cpu").manual_seed(11)
    qkv = torch.randn(b * S, 3 * H * 64, generator=g).to(DEV).bfloat16()
    valid = torch.ones(b, S, dtype=torch.uint8)
    for r, n in pads:
        valid[r, n:] = 0
    kv = valid.reshape(-1).to(DEV)
    slopes = torch.tensor(alibi_slopes(H), device=DEV)
    T = b * S
    out = torch.empty(T, H * 64, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(b, H, S, device=DEV)
    N.call("dna_attn_fwd", qkv.data_ptr(), kv.data_ptr(), slopes.data_ptr(), b, S, H, 64, N.BF16,
           1 / math.sqrt(64), out.data_ptr(), lse.data_ptr(), N.stream_ptr())
    # pad rows get no gradient
    dout = (torch.randn(T, H * 64, generator=g).to(DEV) * kv[:, None].float()).bfloat16()
    q2 = qkv.float().clone().requires_grad_(True)
    _ref_attention(q2, kv, H, b, S).backward(dout.float())
    return dict(qkv=qkv, kv=kv, slopes=slopes, out=out, lse=lse, dout=dout,
                ref=q2.grad.view(T, 3, H * 64))


def _launch(S, b, H, pads, nw, with_part):
    from dna_amd import _native as N
    x = _inputs(S, b, H, pads)
    dqkv = torch.full_like(x["qkv"], float("nan"))
    rows = N.lib().dna_attn_dbias_part_rows(b, S)
    part = torch.full((rows, 3 * H * 64), float("nan"), device=DEV) if with_part else None
    delta = torch.empty(b * H * S, device=DEV)
    N.call("dna_attn_bwd_var", x["qkv"].data_ptr(), x["out"].data_ptr(), x["dout"].data_ptr(),
           x["lse"].data_ptr(), x["kv"].data_ptr(), x["slopes"].data_ptr(), b, S, H, 64, N.BF16,
           1 / math.sqrt(64), dqkv.data_ptr(), delta.data_ptr(), N.ptr(part), nw, N.stream_ptr())
    return dqkv, part


@functools.lru_cache(maxsize=None)
def _run(S, b, H, pads, nw, with_part):
    return _launch(S, b, H, pads, nw, with_part)


def _bf16_ord(t):
    """bf16 bit patterns as integers that order like the values (ulp distance = difference)."""
    i = t.view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("with_part", [False, True])
@pytest.mark.parametrize("nw", [8, 4])
@pytest.mark.parametrize("S,b,H,pads", CASES)
def test_bwd_var_vs_fp32(S, b, H, pads, nw, with_part):
    x = _inputs(S, b, H, pads)
    dqkv, _ = _run(S, b, H, pads, nw, with_part)
    gv = x["ref"]
    hv = dqkv.float().view(b * S, 3, H * 64)
    valid = x["kv"].bool()
    scale = gv[valid].abs().max().item()
    err = (hv - gv)[valid].abs().max().item()
    print(f"S={S} b={b} H={H} nw={nw} part={with_part}: err {err:.4g} scale {scale:.4g}")
    assert err < 6e-2 * max(scale, 1.0), (err, scale)
    # pad rows: gradients must be exactly zero (they never reach the loss)
    assert (~valid).any() and hv[~valid].abs().max().item() == 0.0


@pytest.mark.parametrize("with_part", [False, True])
@pytest.mark.parametrize("S,b,H,pads", CASES)
def test_bwd8_vs_bwd4(S, b, H, pads, with_part):
    """dK, dV and the bias-gradient partial rows: bit-identical (the per-key sums over the query
    slices and the column sums keep their order). dQ sums four key-quarter partials instead of
    two key-half ones before the bf16 rounding: its error against fp32 may not exceed the 4-wave
    kernel's by more than 5 %."""
    x = _inputs(S, b, H, pads)
    d8, p8 = _run(S, b, H, pads, 8, with_part)
    d4, p4 = _run(S, b, H, pads, 4, with_part)
    v8, v4 = d8.view(b * S, 3, H * 64), d4.view(b * S, 3, H * 64)
    assert torch.equal(v8[:, 1], v4[:, 1]), "dK"
    assert torch.equal(v8[:, 2], v4[:, 2]), "dV"
    if with_part:
        assert torch.isfinite(p8).all() and torch.equal(p8, p4), "dbias_part"
    valid = x["kv"].bool()
    ref = x["ref"][:, 0][valid]
    e8 = (v8[:, 0].float()[valid] - ref).abs().max().item()
    e4 = (v4[:, 0].float()[valid] - ref).abs().max().item()
    ne = (v8[:, 0] != v4[:, 0]).float().mean().item()
    ulps = (_bf16_ord(v8[:, 0].contiguous()) - _bf16_ord(v4[:, 0].contiguous())).abs().max().item()
    print(f"S={S} b={b} H={H} part={with_part}: dQ err nw8 {e8:.6g} nw4 {e4:.6g}; "
          f"{100 * ne:.3f} % of dQ elements differ, at most {ulps} bf16 ulp")
    assert e8 <= 1.05 * e4, (e8, e4)


@pytest.mark.parametrize("S,b,H,pads", CASES)
def test_bwd8_deterministic(S, b, H, pads):
    """Two runs on NaN-prefilled outputs: every element written, bit-identical."""
    d1, p1 = _run(S, b, H, pads, 8, True)
    d2, p2 = _launch(S, b, H, pads, 8, True)
    assert torch.isfinite(d1.float()).all() and torch.isfinite(p1).all()
    assert torch.equal(d1, d2) and torch.equal(p1, p2)
    ref = d1.float().sum(0)  # the partial rows sum to dqkv's column sums (fp32 vs rounded bf16)
    assert (p1.sum(0) - ref).abs().max().item() < 1e-2 * ref.abs().max().item() + 1e-3


def test_bwd_var_rejects_unsupported():
    """No quiet fall-back: a variant that does not exist for the shape is an error."""
    from dna_amd import _native as N
    S, b, H, pads = CASES[2]
    x = _inputs(S, b, H, pads)
    z = x["qkv"].data_ptr()
    for nw, seqlen in ((8, 128), (6, 256)):
        st = N.lib().dna_attn_bwd_var(z, z, z, z, None, z, 1, seqlen, 1, 64, N.BF16, 0.125, z, z, None,
                                      nw, N.stream_ptr())
        assert st != 0
