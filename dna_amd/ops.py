"""The hot-path HIP kernels as PyTorch operators: `torch.ops.dna_amd.<op>` (SURVEY §8(b) kernel
boundary).

Each op wraps one C-ABI entry point of include/dna_amd.h, runs on the current torch HIP stream,
writes into caller-allocated outputs (declared as mutated arguments), and raises a Python
exception on dtype / shape / contiguity / device errors -- the checks the reference's Triton slot
asserts (flash_attn_triton.py:849-855) -- instead of letting a kernel read out of bounds.

    torch.ops.dna_amd.attn_fwd(qkv, key_valid, slopes, b, S, H, scale, out, lse)
    torch.ops.dna_amd.attn_bwd(qkv, out, dout, lse, key_valid, slopes, b, S, H, scale, dqkv)
    torch.ops.dna_amd.attn_varlen_fwd(qkv, cu_seqlens, positions, slopes, max_seqlen, H, scale, out,
                                      lse)                        packed rows, per-sequence keys
    torch.ops.dna_amd.attn_varlen_bwd(qkv, out, dout, lse, cu_seqlens, positions, slopes,
                                      max_seqlen, H, scale, dqkv)
    torch.ops.dna_amd.linear_fwd(x, w, bias, y)                   y = x w^T (+ bias), bf16 MFMA
    torch.ops.dna_amd.geglu_fwd(g, p, seed, offset, a, fac)       a = dropout(gelu(g1) g2),
                                                                  fac = backward factors
    torch.ops.dna_amd.geglu_bwd(da, fac, dg)                      dg = da * fac
    torch.ops.dna_amd.xent_fwd(logits, target, loss, lse)         per-row CE
    torch.ops.dna_amd.transpose_bf16(src, dst)
    torch.ops.dna_amd.cls_head_fwd(x, wp, bp, wc, bc, p, seed, offset, t, a, logits)
    torch.ops.dna_amd.cls_loss(logits, labels, problem_type, loss, dlogits, pred)
    torch.ops.dna_amd.cls_head_bwd(dlogits, x, t, a, wp, wc, p, seed, offset, dwc, dbc, dwp, dbp,
                                   dx, accumulate)
    torch.ops.dna_amd.pool_head_fwd(x1, x2, flip2, mirror2, start, count, w, bias, pooled, logits)
    torch.ops.dna_amd.pool_head_bwd(dlogits, pooled, w, start, count, dx1, dx2, flip2, mirror2, dw,
                                    dbias, accumulate)
    torch.ops.dna_amd.pool_head_wide_fwd(x1, x2, flip2, mirror2, start, count, w, bias, pooled,
                                         logits, labels, problem, loss, dlogits)   up to 1024 labels
    torch.ops.dna_amd.pool_head_wide_bwd(... as pool_head_bwd)
    torch.ops.dna_amd.lm_head_fwd(h, w, labels, denom, loss, count, coef)
    torch.ops.dna_amd.lm_head_bwd(coef, h, w, labels, count, upstream, denom, dh, dw, accumulate)
    torch.ops.dna_amd.lm_head_rc_fwd(h, w, cm, labels, denom, loss, count, coef)   h [T, 2 D]
    torch.ops.dna_amd.lm_head_rc_bwd(coef, h, w, cm, labels, count, upstream, denom, dh, dw,
                                     accumulate)
    torch.ops.dna_amd.dconv_fwd(x, w_taps, bias, dilation, epilogue, act, g, res, out, z_out,
                                res_out)                          dilated Conv1d + gated epilogues
    torch.ops.dna_amd.dconv_bwd_elem(dfeat, drc, z_h, g, z_g, forget, dz_h, dz_g)
    torch.ops.dna_amd.dconv_wgrad(dz, x, dilation, dw, dbias, accumulate)
    torch.ops.dna_amd.onehot_conv_fwd(input_ids, w, bias, complement, act, out)
    torch.ops.dna_amd.onehot_conv_bwd(input_ids, w, bias, dout, complement, act, dw, dbias,
                                      accumulate)
and the reference's FlashAttention kernel slot with its own signature (flash_attn_triton.py:
1077-1130, called at bert_layers.py:188/192 as flash_attn_qkvpacked_func(qkv, bias)), autograd
included:

    out = dna_amd.ops.flash_attn_qkvpacked_func(qkv[b,S,3,H,D], bias=None, causal=False,
                                                softmax_scale=None)
    out, lse = torch.ops.dna_amd.flash_attn_qkvpacked(qkv, bias, causal, softmax_scale)
with the reference's bias forms ("vector" [., ., 1, S] / "matrix" [., ., S, S], batch / head
broadcast, fp32 or the qkv dtype), fp16 and bf16, any S, head_dim <= 128 (csrc/flash_slot.hip).
The model itself runs the fast path, where the ALiBi + key-pad bias enters as (slopes,
key_valid) instead of a materialised [b,H,S,S] tensor: bias[h,i,j] = -slopes[h]*|i-j| +
(key j pad ? -10000 : 0), exactly what bert_layers.py:421-448 builds:

    out = dna_amd.ops.alibi_attn_qkvpacked_func(qkv, slopes, key_valid, softmax_scale)
The model's own autograd Functions (dna_amd.functional) call the C ABI directly (no per-call
dispatcher overhead on the ~300 launches of a step).
"""
import math

import torch

from . import _native as N

_DT = {torch.float32: N.F32, torch.bfloat16: N.BF16}


def _check(cond, msg):
    if not cond:
        raise RuntimeError(f"dna_amd: {msg}")


def _cuda_contig(name, t, dtypes=None):
    _check(t.is_cuda, f"{name} must be on the GPU (no CPU fallback), got {t.device}")
    _check(t.is_contiguous(), f"{name} must be contiguous")
    if dtypes is not None:
        _check(t.dtype in dtypes, f"{name} dtype {t.dtype} not in {dtypes}")


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------- attention
@torch.library.custom_op("dna_amd::attn_fwd", mutates_args=("out", "lse"))
def attn_fwd(qkv: torch.Tensor, key_valid: torch.Tensor | None, slopes: torch.Tensor, b: int,
             S: int, H: int, scale: float, out: torch.Tensor, lse: torch.Tensor) -> None:
    _cuda_contig("qkv", qkv, (torch.bfloat16, torch.float32))
    _check(qkv.dim() == 2 and qkv.shape[0] == b * S and qkv.shape[1] % (3 * H) == 0,
           f"qkv must be [b*S, 3*H*D], got {tuple(qkv.shape)}")
    D = qkv.shape[1] // (3 * H)
    _cuda_contig("out", out, (qkv.dtype,))
    _check(tuple(out.shape) == (b * S, H * D), "out must be [b*S, H*D]")
    _cuda_contig("lse", lse, (torch.float32,))
    _check(lse.numel() == b * H * S, "lse must hold b*H*S floats")
    _cuda_contig("slopes", slopes, (torch.float32,))
    if key_valid is not None:
        _cuda_contig("key_valid", key_valid, (torch.uint8, torch.bool))
        _check(key_valid.numel() == b * S, "key_valid must hold b*S entries")
    N.call("dna_attn_fwd", qkv.data_ptr(), _p(key_valid), slopes.data_ptr(), b, S, H, D,
           _DT[qkv.dtype], scale, out.data_ptr(), lse.data_ptr(), N.stream_ptr())


@torch.library.custom_op("dna_amd::attn_bwd", mutates_args=("dqkv",))
def attn_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor,
             key_valid: torch.Tensor | None, slopes: torch.Tensor, b: int, S: int, H: int,
             scale: float, dqkv: torch.Tensor) -> None:
    for n, t in (("qkv", qkv), ("out", out), ("dout", dout), ("dqkv", dqkv)):
        _cuda_contig(n, t, (qkv.dtype,))
    _cuda_contig("lse", lse, (torch.float32,))
    _check(dqkv.shape == qkv.shape and dout.shape == out.shape, "dqkv / dout shapes")
    D = qkv.shape[1] // (3 * H)
    delta = torch.empty(b * H * S, device=qkv.device, dtype=torch.float32)
    N.call("dna_attn_bwd", qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
           _p(key_valid), slopes.data_ptr(), b, S, H, D, _DT[qkv.dtype], scale, dqkv.data_ptr(),
           delta.data_ptr(), N.stream_ptr())


def _check_varlen(qkv, cu_seqlens, positions, slopes, max_seqlen, H):
    _cuda_contig("qkv", qkv, (torch.bfloat16, torch.float32))
    _check(qkv.dim() == 2 and qkv.shape[0] > 0 and qkv.shape[1] % (3 * H) == 0,
           f"qkv must be [T, 3*H*D], got {tuple(qkv.shape)}")
    _cuda_contig("cu_seqlens", cu_seqlens, (torch.int32,))
    _check(cu_seqlens.dim() == 1 and cu_seqlens.numel() >= 2, "cu_seqlens must be [nseq + 1]")
    if positions is not None:
        _cuda_contig("positions", positions, (torch.int32,))
        _check(positions.numel() == qkv.shape[0], "positions must hold T entries")
    _cuda_contig("slopes", slopes, (torch.float32,))
    _check(slopes.numel() == H, "slopes must hold H entries")
    _check(max_seqlen > 0, "max_seqlen must be positive")
    return qkv.shape[0], qkv.shape[1] // (3 * H), cu_seqlens.numel() - 1


@torch.library.custom_op("dna_amd::attn_varlen_fwd", mutates_args=("out", "lse"))
def attn_varlen_fwd(qkv: torch.Tensor, cu_seqlens: torch.Tensor, positions: torch.Tensor | None,
                    slopes: torch.Tensor, max_seqlen: int, H: int, scale: float,
                    out: torch.Tensor, lse: torch.Tensor) -> None:
    """Packed ALiBi attention (csrc/attention_varlen.hip): rows cu_seqlens[n] .. cu_seqlens[n+1]-1
    of qkv [T, 3*H*D] are sequence n; out [T, H*D], lse [H, T] fp32."""
    T, D, nseq = _check_varlen(qkv, cu_seqlens, positions, slopes, max_seqlen, H)
    _cuda_contig("out", out, (qkv.dtype,))
    _check(tuple(out.shape) == (T, H * D), "out must be [T, H*D]")
    _cuda_contig("lse", lse, (torch.float32,))
    _check(lse.numel() == H * T, "lse must hold H*T floats")
    N.call("dna_attn_varlen_fwd", qkv.data_ptr(), cu_seqlens.data_ptr(), _p(positions),
           slopes.data_ptr(), nseq, T, max_seqlen, H, D, _DT[qkv.dtype], scale, out.data_ptr(),
           lse.data_ptr(), N.stream_ptr())


@torch.library.custom_op("dna_amd::attn_varlen_bwd", mutates_args=("dqkv",))
def attn_varlen_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor,
                    cu_seqlens: torch.Tensor, positions: torch.Tensor | None, slopes: torch.Tensor,
                    max_seqlen: int, H: int, scale: float, dqkv: torch.Tensor) -> None:
    T, D, nseq = _check_varlen(qkv, cu_seqlens, positions, slopes, max_seqlen, H)
    for n, t in (("out", out), ("dout", dout), ("dqkv", dqkv)):
        _cuda_contig(n, t, (qkv.dtype,))
    _cuda_contig("lse", lse, (torch.float32,))
    _check(dqkv.shape == qkv.shape and dout.shape == out.shape and
           tuple(out.shape) == (T, H * D) and lse.numel() == H * T, "dqkv / dout / out / lse shapes")
    ws = torch.empty(N.lib().dna_attn_varlen_bwd_workspace(nseq, T, max_seqlen, H),
                     device=qkv.device, dtype=torch.uint8)
    N.call("dna_attn_varlen_bwd", qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
           cu_seqlens.data_ptr(), _p(positions), slopes.data_ptr(), nseq, T, max_seqlen, H, D,
           _DT[qkv.dtype], scale, dqkv.data_ptr(), ws.data_ptr(), N.stream_ptr())


@torch.library.custom_op("dna_amd::alibi_attn_qkvpacked", mutates_args=())
def alibi_attn_qkvpacked(qkv: torch.Tensor, slopes: torch.Tensor, key_valid: torch.Tensor | None,
                         softmax_scale: float | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """The model's fast path: the ALiBi + key-pad bias of bert_layers.py:421-448 from (slopes,
    key_valid), never materialised. -> (out [b, S, H, D], lse [b, H, S] fp32 natural log)."""
    _check(qkv.dim() == 5 and qkv.shape[2] == 3, f"qkv must be [b, S, 3, H, D], got {tuple(qkv.shape)}")
    b, S, _, H, D = qkv.shape
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    packed = qkv.contiguous().view(b * S, 3 * H * D)
    out = torch.empty(b * S, H * D, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(b, H, S, device=qkv.device, dtype=torch.float32)
    kv = None if key_valid is None else key_valid.to(torch.uint8).contiguous()
    attn_fwd(packed, kv, slopes.float().contiguous(), b, S, H, scale, out, lse)
    return out.view(b, S, H, D), lse


@alibi_attn_qkvpacked.register_fake
def _(qkv, slopes, key_valid, softmax_scale=None):
    b, S, _, H, D = qkv.shape
    return qkv.new_empty(b, S, H, D), qkv.new_empty(b, H, S, dtype=torch.float32)


def _alibi_setup(ctx, inputs, output):
    qkv, slopes, key_valid, softmax_scale = inputs
    out, lse = output
    ctx.save_for_backward(qkv, slopes, key_valid if key_valid is not None else torch.empty(0),
                          out, lse)
    ctx.has_kv = key_valid is not None
    ctx.scale = softmax_scale


def _alibi_backward(ctx, dout, dlse):
    qkv, slopes, key_valid, out, lse = ctx.saved_tensors
    b, S, _, H, D = qkv.shape
    scale = ctx.scale if ctx.scale is not None else 1.0 / math.sqrt(D)
    packed = qkv.contiguous().view(b * S, 3 * H * D)
    kv = key_valid.to(torch.uint8).contiguous() if ctx.has_kv else None
    dqkv = torch.empty_like(packed)
    attn_bwd(packed, out.contiguous().view(b * S, H * D), dout.contiguous().view(b * S, H * D),
             lse, kv, slopes.float().contiguous(), b, S, H, scale, dqkv)
    return dqkv.view(qkv.shape), None, None, None


alibi_attn_qkvpacked.register_autograd(_alibi_backward, setup_context=_alibi_setup)


def alibi_attn_qkvpacked_func(qkv, slopes, key_valid=None, softmax_scale=None):
    """The fast path: out of alibi_attn_qkvpacked (bias = -slopes[h]*|i-j| + pad*-10000)."""
    return torch.ops.dna_amd.alibi_attn_qkvpacked(qkv, slopes, key_valid, softmax_scale)[0]


# ------------------------------------------------------------------- generic FlashAttention slot
_FDT = {torch.bfloat16: N.BF16, torch.float16: N.F16, torch.float32: N.F32}


def _bias_args(bias, b, H, S, qkv_dtype):
    """The reference's bias handling (flash_attn_triton.py:780-807): 4-D, fp32 or the qkv dtype,
    last dims (1, S) "vector" or (S, S) "matrix", first dims broadcastable to (b, H) -- broadcast
    as stride 0 here instead of repeat copies. -> (bias, dtype code, type, sb, sh, sq)."""
    if bias is None:
        return None, N.F32, 0, 0, 0, 0
    _check(bias.dtype in (qkv_dtype, torch.float32), f"bias dtype {bias.dtype} must be fp32 or {qkv_dtype}")
    _check(bias.is_cuda, "bias must be on the GPU")
    _check(bias.dim() == 4, f"bias must be 4-D, got {bias.dim()}-D")
    if bias.stride(-1) != 1:
        bias = bias.contiguous()
    if tuple(bias.shape[2:]) == (1, S):
        btype = 1
    elif tuple(bias.shape[2:]) == (S, S):
        btype = 2
    else:
        raise RuntimeError("Last 2 dimensions of bias must be (1, seqlen_k) or (seqlen_q, seqlen_k)")
    _check(bias.shape[0] in (1, b) and bias.shape[1] in (1, H),
           f"First 2 dimensions of bias must be broadcastible to (batch, nheads) = ({b}, {H}). "
           f"Bias has shape: {tuple(bias.shape)}")
    sb = bias.stride(0) if bias.shape[0] == b and b > 1 else 0
    sh = bias.stride(1) if bias.shape[1] == H and H > 1 else 0
    sq = bias.stride(2) if btype == 2 else 0
    return bias, _FDT[bias.dtype], btype, sb, sh, sq


def _pad_head(t, Dp):
    D = t.shape[-1]
    return t if D == Dp else torch.nn.functional.pad(t, (0, Dp - D))


def _kernel_dim(D):
    _check(D <= 128, "FlashAttention only support head dimensions up to 128")
    return 32 if D <= 32 else (64 if D <= 64 else 128)


@torch.library.custom_op("dna_amd::flash_attn_qkvpacked", mutates_args=())
def flash_attn_qkvpacked(qkv: torch.Tensor, bias: torch.Tensor | None = None, causal: bool = False,
                         softmax_scale: float | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """_flash_attn_forward over packed qkv [b, S, 3, H, D] (flash_attn_triton.py:767-860)
    -> (out [b, S, H, D], lse [b, H, ceil(S/128)*128] fp32 natural log)."""
    _check(qkv.dim() == 5 and qkv.shape[2] == 3, f"qkv must be [b, S, 3, H, D], got {tuple(qkv.shape)}")
    _check(qkv.dtype in (torch.float16, torch.bfloat16), "Only support fp16 and bf16")
    _check(qkv.is_cuda, "qkv must be on the GPU (no CPU fallback)")
    b, S, _, H, D = qkv.shape
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    Dp = _kernel_dim(D)
    x = _pad_head(qkv, Dp).contiguous()
    bias, bdt, btype, sb, sh, sq = _bias_args(bias, b, H, S, qkv.dtype)
    out = torch.empty(b, S, H, Dp, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(b, H, N.lib().dna_flash_lse_rows(S), device=qkv.device, dtype=torch.float32)
    N.call("dna_flash_fwd", x.data_ptr(), _FDT[qkv.dtype], _p(bias), bdt, btype, sb, sh, sq, b, S, H,
           Dp, int(bool(causal)), scale, out.data_ptr(), lse.data_ptr(), N.stream_ptr())
    return (out if Dp == D else out[..., :D].contiguous()), lse


@flash_attn_qkvpacked.register_fake
def _(qkv, bias=None, causal=False, softmax_scale=None):
    b, S, _, H, D = qkv.shape
    return qkv.new_empty(b, S, H, D), qkv.new_empty(b, H, (S + 127) // 128 * 128, dtype=torch.float32)


def _flash_setup(ctx, inputs, output):
    qkv, bias, causal, softmax_scale = inputs
    out, lse = output
    ctx.save_for_backward(qkv, bias if bias is not None else torch.empty(0), out, lse)
    ctx.has_bias = bias is not None
    ctx.causal = bool(causal)
    ctx.scale = softmax_scale


def _flash_backward(ctx, dout, dlse):
    qkv, bias, out, lse = ctx.saved_tensors
    # flash_attn_triton.py:1109-1110
    _check(not (ctx.has_bias and ctx.needs_input_grad[1]),
           "FlashAttention does not support bias gradient yet")
    b, S, _, H, D = qkv.shape
    scale = ctx.scale if ctx.scale is not None else 1.0 / math.sqrt(D)
    Dp = _kernel_dim(D)
    x = _pad_head(qkv, Dp).contiguous()
    o = _pad_head(out, Dp).contiguous()
    g = _pad_head(dout, Dp).contiguous()
    bias, bdt, btype, sb, sh, sq = _bias_args(bias if ctx.has_bias else None, b, H, S, qkv.dtype)
    delta = torch.empty_like(lse)
    dqkv = torch.empty_like(x)
    N.call("dna_flash_bwd", x.data_ptr(), _FDT[qkv.dtype], _p(bias), bdt, btype, sb, sh, sq,
           o.data_ptr(), g.data_ptr(), lse.data_ptr(), b, S, H, Dp, int(ctx.causal), scale,
           delta.data_ptr(), dqkv.data_ptr(), N.stream_ptr())
    return (dqkv if Dp == D else dqkv[..., :D].contiguous()), None, None, None


flash_attn_qkvpacked.register_autograd(_flash_backward, setup_context=_flash_setup)


def flash_attn_qkvpacked_func(qkv, bias=None, causal=False, softmax_scale=None):
    """Drop-in for flash_attn_qkvpacked_func (flash_attn_triton.py:1077-1130, the reference's
    _FlashAttnQKVPackedFunc.apply): same positional signature and semantics -- qkv [b, S, 3, H, D]
    fp16 / bf16, bias broadcastible to (b, H, S, S) as "vector" [., ., 1, S] or "matrix"
    [., ., S, S] (fp32 or qkv dtype), causal, softmax_scale (default 1/sqrt(D)); returns
    out [b, S, H, D]; the backward gives dqkv (no bias gradient, as the reference)."""
    return torch.ops.dna_amd.flash_attn_qkvpacked(qkv, bias, bool(causal), softmax_scale)[0]


# ------------------------------------------------------------------------------- GEMM
@torch.library.custom_op("dna_amd::linear_fwd", mutates_args=("y",))
def linear_fwd(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, y: torch.Tensor) -> None:
    _cuda_contig("x", x, (torch.bfloat16,))
    _cuda_contig("w", w, (torch.bfloat16,))
    _cuda_contig("y", y, (torch.bfloat16,))
    M, K = x.shape
    Nn = w.shape[0]
    _check(w.shape[1] == K and tuple(y.shape) == (M, Nn), "shapes: x[M,K], w[N,K], y[M,N]")
    _check(K % 64 == 0 and Nn % 8 == 0, f"K % 64 and N % 8 required (K={K}, N={Nn})")
    if bias is not None:
        _cuda_contig("bias", bias, (torch.float32,))
        _check(bias.numel() == Nn, "bias must hold N floats")
    N.call("dna_linear_fwd", x.data_ptr(), w.data_ptr(), _p(bias), M, Nn, K, y.data_ptr(),
           N.stream_ptr())


@torch.library.custom_op("dna_amd::transpose_bf16", mutates_args=("dst",))
def transpose_bf16(src: torch.Tensor, dst: torch.Tensor) -> None:
    _cuda_contig("src", src, (torch.bfloat16,))
    _cuda_contig("dst", dst, (torch.bfloat16,))
    r, c = src.shape
    _check(tuple(dst.shape) == (c, r), "dst must be src transposed")
    N.call("dna_transpose_bf16", src.data_ptr(), r, c, dst.data_ptr(), N.stream_ptr())


@torch.library.custom_op("dna_amd::geglu_linear_fwd", mutates_args=("fac", "a"))
def geglu_linear_fwd(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, p: float,
                     seed: int, offset: int, fac: torch.Tensor, a: torch.Tensor) -> None:
    """g = x . w^T (+ bias), a = dropout(gelu(g[:, :F]) * g[:, F:]) and fac = the backward
    factors of geglu_fwd in one launch (gated_layers + GeGLU, bert_layers.py:292-296; g itself is
    not stored); same bits as linear_fwd + geglu_fwd."""
    _cuda_contig("x", x, (torch.bfloat16,))
    _cuda_contig("w", w, (torch.bfloat16,))
    _cuda_contig("fac", fac, (torch.bfloat16,))
    _cuda_contig("a", a, (torch.bfloat16,))
    M, K = x.shape
    F2 = w.shape[0]
    _check(w.shape[1] == K and tuple(fac.shape) == (M, F2) and tuple(a.shape) == (M, F2 // 2),
           "shapes: x[M,K], w[2F,K], fac[M,2F], a[M,F]")
    _check(K % 64 == 0 and F2 % 256 == 0, f"K % 64 and 2F % 256 required (K={K}, 2F={F2})")
    if bias is not None:
        _cuda_contig("bias", bias, (torch.float32,))
        _check(bias.numel() == F2, "bias must hold 2F floats")
    N.call("dna_geglu_linear_fwd", x.data_ptr(), w.data_ptr(), _p(bias), M, F2 // 2, K, float(p),
           seed, offset, fac.data_ptr(), a.data_ptr(), N.stream_ptr())


@torch.library.custom_op("dna_amd::geglu_linear_dgrad", mutates_args=("dg",))
def geglu_linear_dgrad(dy: torch.Tensor, wt: torch.Tensor, fac: torch.Tensor,
                       dg: torch.Tensor) -> None:
    """dg = geglu_bwd(dy . wt^T, fac) in one launch: wo's data gradient (wt = wo^T, [F, hidden])
    with the GeGLU backward in the epilogue (bert_layers.py:292-297); == linear_fwd + geglu_bwd."""
    _cuda_contig("dy", dy, (torch.bfloat16,))
    _cuda_contig("wt", wt, (torch.bfloat16,))
    _cuda_contig("fac", fac, (torch.bfloat16,))
    _cuda_contig("dg", dg, (torch.bfloat16,))
    M, H = dy.shape
    F = wt.shape[0]
    _check(wt.shape[1] == H and tuple(fac.shape) == (M, 2 * F) and dg.shape == fac.shape,
           "shapes: dy[M,H], wt[F,H], fac / dg[M,2F]")
    _check(H % 128 == 0 and H >= 256 and F % 256 == 0,
           f"hidden % 128, hidden >= 256 and F % 256 required (H={H}, F={F})")
    N.call("dna_geglu_linear_dgrad_p", dy.data_ptr(), wt.data_ptr(), fac.data_ptr(), M, F, H,
           dg.data_ptr(), N.stream_ptr())


# ------------------------------------------------------------------------------- elementwise
@torch.library.custom_op("dna_amd::geglu_fwd", mutates_args=("a", "fac"))
def geglu_fwd(g: torch.Tensor, p: float, seed: int, offset: int, a: torch.Tensor,
              fac: torch.Tensor) -> None:
    """a = dropout(gelu(g[:, :F]) * g[:, F:]); fac [rows, 2F] = the backward factors
    [d a / d g1 | d a / d g2] with the dropout folded in, for geglu_bwd (may be g itself)."""
    _cuda_contig("g", g, (torch.bfloat16, torch.float32))
    _cuda_contig("a", a, (g.dtype,))
    n, f2 = g.shape
    _check(tuple(a.shape) == (n, f2 // 2), "a must be [rows, F] for g [rows, 2F]")
    _cuda_contig("fac", fac, (g.dtype,))
    _check(fac.shape == g.shape, "fac must be shaped like g")
    N.call("dna_geglu_fwd", g.data_ptr(), _DT[g.dtype], n, f2 // 2, p, seed, offset, a.data_ptr(),
           fac.data_ptr(), N.stream_ptr())


@torch.library.custom_op("dna_amd::geglu_bwd", mutates_args=("dg",))
def geglu_bwd(da: torch.Tensor, fac: torch.Tensor, dg: torch.Tensor) -> None:
    """dg = [da * fac1 | da * fac2] (fac from geglu_fwd / geglu_linear_fwd)."""
    _cuda_contig("fac", fac, (torch.bfloat16, torch.float32))
    _cuda_contig("da", da, (fac.dtype,))
    _cuda_contig("dg", dg, (fac.dtype,))
    n, f2 = fac.shape
    _check(tuple(da.shape) == (n, f2 // 2) and dg.shape == fac.shape, "da [rows, F], dg like fac")
    N.call("dna_geglu_bwd", da.data_ptr(), fac.data_ptr(), _DT[fac.dtype], n, f2 // 2,
           dg.data_ptr(), N.stream_ptr())


@torch.library.custom_op("dna_amd::xent_fwd", mutates_args=("loss", "lse"))
def xent_fwd(logits: torch.Tensor, target: torch.Tensor, loss: torch.Tensor,
             lse: torch.Tensor) -> None:
    _cuda_contig("logits", logits, (torch.bfloat16, torch.float32))
    _cuda_contig("target", target, (torch.int64,))
    M, V = logits.shape
    _check(target.numel() == M and loss.numel() == M and lse.numel() == M, "row counts")
    N.call("dna_xent_fwd", logits.data_ptr(), _DT[logits.dtype], target.data_ptr(), M, V,
           loss.data_ptr(), lse.data_ptr(), N.stream_ptr())


# ------------------------------------------------------------------------------- cls head
def _cls_x(x):
    _check(x.is_cuda, f"x must be on the GPU (no CPU fallback), got {x.device}")
    _check(x.dtype in _DT, f"x dtype {x.dtype} not in {tuple(_DT)}")
    _check(x.dim() == 2 and x.stride(1) == 1 and (x.shape[0] == 1 or x.stride(0) >= x.shape[1]),
           "x must be [B, H] rows with unit column stride")
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


@torch.library.custom_op("dna_amd::cls_head_fwd", mutates_args=("t", "a", "logits"))
def cls_head_fwd(x: torch.Tensor, wp: torch.Tensor, bp: torch.Tensor, wc: torch.Tensor,
                 bc: torch.Tensor, p: float, seed: int, offset: int, t: torch.Tensor,
                 a: torch.Tensor, logits: torch.Tensor) -> None:
    """t = tanh(x wp^T + bp), a = dropout(t; p, seed, offset), logits = a wc^T + bc (fp32
    parameters; x fp32 or bf16 rows, a strided row view is read in place)."""
    stride = _cls_x(x)
    B, H = x.shape
    C = wc.shape[0]
    for n, w, shape in (("wp", wp, (H, H)), ("bp", bp, (H,)), ("wc", wc, (C, H)), ("bc", bc, (C,)),
                        ("t", t, (B, H)), ("a", a, (B, H)), ("logits", logits, (B, C))):
        _cuda_contig(n, w, (torch.float32,))
        _check(tuple(w.shape) == shape, f"{n} must be {shape}, got {tuple(w.shape)}")
    nws = N.lib().dna_cls_head_fwd_workspace(B, H, C)
    ws = torch.empty(max(nws // 4, 4), device=x.device, dtype=torch.float32)
    N.call("dna_cls_head_fwd", x.data_ptr(), _DT[x.dtype], stride, wp.data_ptr(), bp.data_ptr(),
           wc.data_ptr(), bc.data_ptr(), B, H, C, float(p), seed, offset, t.data_ptr(),
           a.data_ptr(), logits.data_ptr(), None, 0, None, None, None, ws.data_ptr(),
           ws.numel() * 4, N.stream_ptr())


@torch.library.custom_op("dna_amd::cls_loss", mutates_args=("loss", "dlogits", "pred"))
def cls_loss(logits: torch.Tensor, labels: torch.Tensor, problem_type: int, loss: torch.Tensor,
             dlogits: torch.Tensor, pred: torch.Tensor | None) -> None:
    """problem_type 0 regression (MSE), 1 single-label (mean CE, int64 labels [B]; pred = argmax),
    2 multi-label (BCE with logits); fp32 labels [B, C] for 0 and 2. loss: one float, dlogits:
    d loss / d logits."""
    _cuda_contig("logits", logits, (torch.float32,))
    B, C = logits.shape
    _cuda_contig("labels", labels, (torch.int64,) if problem_type == 1 else (torch.float32,))
    _check(labels.numel() == (B if problem_type == 1 else B * C), "label count")
    _cuda_contig("loss", loss, (torch.float32,))
    _cuda_contig("dlogits", dlogits, (torch.float32,))
    _check(loss.numel() == 1 and dlogits.shape == logits.shape, "loss [1], dlogits like logits")
    if pred is not None:
        _cuda_contig("pred", pred, (torch.int64,))
        _check(pred.numel() == B, "pred must hold B entries")
    N.call("dna_cls_loss", logits.data_ptr(), labels.data_ptr(), problem_type, B, C,
           loss.data_ptr(), dlogits.data_ptr(), _p(pred), N.stream_ptr())


@torch.library.custom_op("dna_amd::cls_head_bwd",
                         mutates_args=("dwc", "dbc", "dwp", "dbp", "dx"))
def cls_head_bwd(dlogits: torch.Tensor, x: torch.Tensor, t: torch.Tensor, a: torch.Tensor,
                 wp: torch.Tensor, wc: torch.Tensor, p: float, seed: int, offset: int,
                 dwc: torch.Tensor, dbc: torch.Tensor, dwp: torch.Tensor, dbp: torch.Tensor,
                 dx: torch.Tensor, accumulate: bool) -> None:
    """Backward of cls_head_fwd from dlogits: dwc, dbc, dwp, dbp (accumulate: added into the
    buffers) and dx [B, H] fp32."""
    stride = _cls_x(x)
    B, H = x.shape
    C = wc.shape[0]
    for n, w, shape in (("dlogits", dlogits, (B, C)), ("t", t, (B, H)), ("a", a, (B, H)),
                        ("wp", wp, (H, H)), ("wc", wc, (C, H)), ("dwc", dwc, (C, H)),
                        ("dbc", dbc, (C,)), ("dwp", dwp, (H, H)), ("dbp", dbp, (H,)),
                        ("dx", dx, (B, H))):
        _cuda_contig(n, w, (torch.float32,))
        _check(tuple(w.shape) == shape, f"{n} must be {shape}, got {tuple(w.shape)}")
    nws = N.lib().dna_cls_head_bwd_workspace(B, H, C)
    ws = torch.empty(max(nws // 4, 4), device=x.device, dtype=torch.float32)
    N.call("dna_cls_head_bwd", dlogits.data_ptr(), None, x.data_ptr(), _DT[x.dtype], stride,
           t.data_ptr(), a.data_ptr(), wp.data_ptr(), wc.data_ptr(), B, H, C, float(p), seed,
           offset, dwc.data_ptr(), dbc.data_ptr(), dwp.data_ptr(), dbp.data_ptr(), dx.data_ptr(),
           int(accumulate), ws.data_ptr(), ws.numel() * 4, N.stream_ptr())

# ------------------------------------------------------------------------------- pool head
def _pool_x(name, x):
    _check(x.is_cuda, f"{name} must be on the GPU (no CPU fallback), got {x.device}")
    _check(x.dtype in _DT, f"{name} dtype {x.dtype} not in {tuple(_DT)}")
    _check(x.dim() == 3 and x.numel() > 0, f"{name} must be a non-empty [B, L, D]")
    B, L, D = x.shape
    s = x.stride(1) if L > 1 else (x.stride(0) if B > 1 else D)
    _check(x.stride(2) == 1 and s >= D and (B == 1 or L == 1 or x.stride(0) == L * s),
           f"{name} must have unit channel stride and batch stride L * position stride")
    return s


def _pool_win(name, t, B):
    if t is not None:
        _cuda_contig(name, t, (torch.int32,))
        _check(t.dim() == 1 and t.numel() == B, f"{name} must be int32 [{B}]")


@torch.library.custom_op("dna_amd::pool_head_fwd", mutates_args=("pooled", "logits"))
def pool_head_fwd(x1: torch.Tensor, x2: torch.Tensor | None, flip2: bool, mirror2: bool,
                  start: torch.Tensor | None, count: torch.Tensor | None, w: torch.Tensor,
                  bias: torch.Tensor | None, pooled: torch.Tensor, logits: torch.Tensor) -> None:
    """pooled = mean over the window [start, start + count) of x1 (averaged with the same over x2,
    its channels reversed when flip2, its window mirrored along L when mirror2), logits =
    pooled w^T (+ bias). x1, x2 [B, L, D] fp32 or
    bf16 views with unit channel stride, read in place."""
    s1 = _pool_x("x1", x1)
    B, L, D = x1.shape
    s2 = 0
    if x2 is not None:
        s2 = _pool_x("x2", x2)
        _check(x2.shape == x1.shape and x2.dtype == x1.dtype, "x2 must match x1")
    C = w.shape[0]
    for n, t, shape in (("w", w, (C, D)), ("bias", bias, (C,)), ("pooled", pooled, (B, D)),
                        ("logits", logits, (B, C))):
        if t is None:
            continue
        _cuda_contig(n, t, (torch.float32,))
        _check(tuple(t.shape) == shape, f"{n} must be {shape}, got {tuple(t.shape)}")
    _pool_win("start", start, B)
    _pool_win("count", count, B)
    nws = N.lib().dna_pool_head_fwd_workspace(B, L, D)
    ws = torch.empty(max(nws // 4, 4), device=x1.device, dtype=torch.float32)
    N.call("dna_pool_head_fwd", x1.data_ptr(), s1, _p(x2), s2, int(flip2) | (int(mirror2) << 1),
           _DT[x1.dtype],
           _p(start), _p(count), w.data_ptr(), _p(bias), B, L, D, C, pooled.data_ptr(),
           logits.data_ptr(), None, 0, None, None, None, ws.data_ptr(), ws.numel() * 4,
           N.stream_ptr())


@torch.library.custom_op("dna_amd::pool_head_bwd", mutates_args=("dx1", "dx2", "dw", "dbias"))
def pool_head_bwd(dlogits: torch.Tensor, pooled: torch.Tensor, w: torch.Tensor,
                  start: torch.Tensor | None, count: torch.Tensor | None, dx1: torch.Tensor,
                  dx2: torch.Tensor | None, flip2: bool, mirror2: bool, dw: torch.Tensor,
                  dbias: torch.Tensor | None, accumulate: bool) -> None:
    """Backward of pool_head_fwd from dlogits: dw, dbias (accumulate: added into the buffers) and
    dx1 / dx2 [B, L, D] (views with unit channel stride), every element written."""
    s1 = _pool_x("dx1", dx1)
    B, L, D = dx1.shape
    s2 = 0
    if dx2 is not None:
        s2 = _pool_x("dx2", dx2)
        _check(dx2.shape == dx1.shape and dx2.dtype == dx1.dtype, "dx2 must match dx1")
    C = w.shape[0]
    for n, t, shape in (("dlogits", dlogits, (B, C)), ("pooled", pooled, (B, D)), ("w", w, (C, D)),
                        ("dw", dw, (C, D)), ("dbias", dbias, (C,))):
        if t is None:
            continue
        _cuda_contig(n, t, (torch.float32,))
        _check(tuple(t.shape) == shape, f"{n} must be {shape}, got {tuple(t.shape)}")
    _pool_win("start", start, B)
    _pool_win("count", count, B)
    nws = N.lib().dna_pool_head_bwd_workspace(B, L, D)
    ws = torch.empty(max(nws // 4, 4), device=dx1.device, dtype=torch.float32)
    N.call("dna_pool_head_bwd", dlogits.data_ptr(), None, pooled.data_ptr(), w.data_ptr(),
           _p(start), _p(count), B, L, D, C, _DT[dx1.dtype], dx1.data_ptr(), s1, _p(dx2), s2,
           int(flip2) | (int(mirror2) << 1), dw.data_ptr(), _p(dbias), int(accumulate), ws.data_ptr(), ws.numel() * 4,
           N.stream_ptr())


@torch.library.custom_op("dna_amd::pool_head_wide_fwd",
                         mutates_args=("pooled", "logits", "loss", "dlogits"))
def pool_head_wide_fwd(x1: torch.Tensor, x2: torch.Tensor | None, flip2: bool, mirror2: bool,
                       start: torch.Tensor | None, count: torch.Tensor | None, w: torch.Tensor,
                       bias: torch.Tensor | None, pooled: torch.Tensor, logits: torch.Tensor,
                       labels: torch.Tensor | None, problem: int, loss: torch.Tensor | None,
                       dlogits: torch.Tensor | None) -> None:
    """pool_head_fwd for up to 1024 labels (the wide kernels of csrc/pool_head.hip). labels fp32
    [B, C] with problem = the dna_cls_problem value of regression or multi-label: loss [1] and
    dlogits [B, C] are written too; labels None: pooled and logits only."""
    s1 = _pool_x("x1", x1)
    B, L, D = x1.shape
    s2 = 0
    if x2 is not None:
        s2 = _pool_x("x2", x2)
        _check(x2.shape == x1.shape and x2.dtype == x1.dtype, "x2 must match x1")
    C = w.shape[0]
    for n, t, shape in (("w", w, (C, D)), ("bias", bias, (C,)), ("pooled", pooled, (B, D)),
                        ("logits", logits, (B, C)), ("labels", labels, (B, C)), ("loss", loss, (1,)),
                        ("dlogits", dlogits, (B, C))):
        if t is None:
            continue
        _cuda_contig(n, t, (torch.float32,))
        _check(tuple(t.shape) == shape, f"{n} must be {shape}, got {tuple(t.shape)}")
    _check(labels is None or (loss is not None and dlogits is not None),
           "labels need loss and dlogits")
    _pool_win("start", start, B)
    _pool_win("count", count, B)
    nws = N.lib().dna_pool_head_wide_fwd_workspace(B, L, D, C)
    ws = torch.empty(max(nws // 4, 4), device=x1.device, dtype=torch.float32)
    N.call("dna_pool_head_wide_fwd", x1.data_ptr(), s1, _p(x2), s2,
           int(flip2) | (int(mirror2) << 1), _DT[x1.dtype], _p(start), _p(count), w.data_ptr(),
           _p(bias), B, L, D, C, pooled.data_ptr(), logits.data_ptr(), _p(labels), int(problem),
           _p(loss), _p(dlogits), ws.data_ptr(), ws.numel() * 4, N.stream_ptr())


@torch.library.custom_op("dna_amd::pool_head_wide_bwd",
                         mutates_args=("dx1", "dx2", "dw", "dbias"))
def pool_head_wide_bwd(dlogits: torch.Tensor, pooled: torch.Tensor, w: torch.Tensor,
                       start: torch.Tensor | None, count: torch.Tensor | None, dx1: torch.Tensor,
                       dx2: torch.Tensor | None, flip2: bool, mirror2: bool, dw: torch.Tensor,
                       dbias: torch.Tensor | None, accumulate: bool) -> None:
    """pool_head_bwd for up to 1024 labels: the same arguments and results."""
    s1 = _pool_x("dx1", dx1)
    B, L, D = dx1.shape
    s2 = 0
    if dx2 is not None:
        s2 = _pool_x("dx2", dx2)
        _check(dx2.shape == dx1.shape and dx2.dtype == dx1.dtype, "dx2 must match dx1")
    C = w.shape[0]
    for n, t, shape in (("dlogits", dlogits, (B, C)), ("pooled", pooled, (B, D)), ("w", w, (C, D)),
                        ("dw", dw, (C, D)), ("dbias", dbias, (C,))):
        if t is None:
            continue
        _cuda_contig(n, t, (torch.float32,))
        _check(tuple(t.shape) == shape, f"{n} must be {shape}, got {tuple(t.shape)}")
    _pool_win("start", start, B)
    _pool_win("count", count, B)
    nws = N.lib().dna_pool_head_wide_bwd_workspace(B, L, D, C)
    ws = torch.empty(max(nws // 4, 4), device=dx1.device, dtype=torch.float32)
    N.call("dna_pool_head_wide_bwd", dlogits.data_ptr(), None, pooled.data_ptr(), w.data_ptr(),
           _p(start), _p(count), B, L, D, C, _DT[dx1.dtype], dx1.data_ptr(), s1, _p(dx2), s2,
           int(flip2) | (int(mirror2) << 1), dw.data_ptr(), _p(dbias), int(accumulate),
           ws.data_ptr(), ws.numel() * 4, N.stream_ptr())


def _lm_rows(name, x):
    _check(x.is_cuda, f"{name} must be on the GPU (no CPU fallback), got {x.device}")
    _check(x.dtype in _DT, f"{name} dtype {x.dtype} not in {tuple(_DT)}")
    _check(x.dim() == 2 and x.numel() > 0, f"{name} must be a non-empty [T, D]")
    T, D = x.shape
    _check(x.stride(1) == 1 and (T == 1 or x.stride(0) >= D),
           f"{name} must have unit column stride and a row stride >= D")
    return x.stride(0) if T > 1 else D


def _lm_common(w, labels, count, T, D):
    V = w.shape[0]
    _cuda_contig("w", w, tuple(_DT))
    _check(tuple(w.shape) == (V, D) and 1 <= V <= 64, f"w must be [V <= 64, {D}], got {tuple(w.shape)}")
    _cuda_contig("labels", labels, (torch.int64,))
    _check(labels.numel() == T, f"labels must be int64 [{T}]")
    _cuda_contig("count", count, (torch.int64,))
    _check(count.numel() == 1, "count must hold one int64")
    return V


@torch.library.custom_op("dna_amd::lm_head_fwd", mutates_args=("loss", "count", "coef"))
def lm_head_fwd(h: torch.Tensor, w: torch.Tensor, labels: torch.Tensor, denom: float,
                loss: torch.Tensor, count: torch.Tensor, coef: torch.Tensor | None) -> None:
    """Masked cross entropy of h w^T over the rows with 0 <= labels < V, no logits tensor:
    loss[0] = the sum, loss[1] = sum / (denom > 0 ? denom : count) (0 when count == 0), count = the
    kept rows, coef [T, V] = softmax - onehot on kept rows (the other rows are not written)."""
    hs = _lm_rows("h", h)
    T, D = h.shape
    V = _lm_common(w, labels, count, T, D)
    _cuda_contig("loss", loss, (torch.float32,))
    _check(loss.numel() == 2, "loss must hold two fp32 values (sum, mean)")
    if coef is not None:
        _cuda_contig("coef", coef, (torch.float32,))
        _check(tuple(coef.shape) == (T, V), f"coef must be [{T}, {V}]")
    nws = N.lib().dna_lm_head_fwd_workspace(T)
    ws = torch.empty(max(nws // 8, 2), device=h.device, dtype=torch.float64)
    N.call("dna_lm_head_fwd", h.data_ptr(), hs, _DT[h.dtype], w.data_ptr(), _DT[w.dtype],
           labels.data_ptr(), T, D, V, float(denom), loss.data_ptr(), count.data_ptr(),
           loss.data_ptr() + 4, _p(coef), ws.data_ptr(), ws.numel() * 8, N.stream_ptr())


@torch.library.custom_op("dna_amd::lm_head_bwd", mutates_args=("dh", "dw"))
def lm_head_bwd(coef: torch.Tensor, h: torch.Tensor, w: torch.Tensor, labels: torch.Tensor,
                count: torch.Tensor, upstream: torch.Tensor | None, denom: float,
                dh: torch.Tensor, dw: torch.Tensor, accumulate: bool) -> None:
    """Backward of lm_head_fwd: dh [T, D] in h's dtype (a view with unit column stride; every
    element written, zeros on ignored rows) and dw [V, D] fp32 (accumulate: added into it), both
    times upstream[0] / (denom > 0 ? denom : count)."""
    hs = _lm_rows("h", h)
    ds = _lm_rows("dh", dh)
    T, D = h.shape
    V = _lm_common(w, labels, count, T, D)
    _check(dh.shape == h.shape and dh.dtype == h.dtype, "dh must match h")
    for n, t, shape in (("coef", coef, (T, V)), ("dw", dw, (V, D))):
        _cuda_contig(n, t, (torch.float32,))
        _check(tuple(t.shape) == shape, f"{n} must be {shape}, got {tuple(t.shape)}")
    if upstream is not None:
        _cuda_contig("upstream", upstream, (torch.float32,))
        _check(upstream.numel() == 1, "upstream must hold one fp32 value")
    nws = N.lib().dna_lm_head_bwd_workspace(T, D, V)
    ws = torch.empty(max(nws // 4, 4), device=h.device, dtype=torch.float32)
    N.call("dna_lm_head_bwd", coef.data_ptr(), h.data_ptr(), hs, _DT[h.dtype], w.data_ptr(),
           _DT[w.dtype], labels.data_ptr(), count.data_ptr(), _p(upstream), float(denom), T, D, V,
           dh.data_ptr(), ds, dw.data_ptr(), int(accumulate), ws.data_ptr(), ws.numel() * 4,
           N.stream_ptr())


def _lm_rc_common(h, w, cm):
    """The RC head's shapes: h [T, 2 D] for w [V, D], cm [V] int64 -> (T, D)."""
    T, D2 = h.shape
    D = w.shape[-1] if w.dim() == 2 else 0
    _check(D > 0 and D2 == 2 * D, f"h must have 2 * D = {2 * D} columns for w [V, {D}], got {D2}")
    _cuda_contig("cm", cm, (torch.int64,))
    _check(cm.numel() == w.shape[0], f"cm must be int64 [{w.shape[0]}]")
    return T, D


@torch.library.custom_op("dna_amd::lm_head_rc_fwd", mutates_args=("loss", "count", "coef"))
def lm_head_rc_fwd(h: torch.Tensor, w: torch.Tensor, cm: torch.Tensor, labels: torch.Tensor,
                   denom: float, loss: torch.Tensor, count: torch.Tensor,
                   coef: torch.Tensor | None) -> None:
    """lm_head_fwd for the RC-equivariant head: h [T, 2 D], w [V, D], cm [V] int64 (entries in
    [0, V), validated by the caller), logit_v = h[:, :D] w[v] + flip(h[:, D:]) w[cm[v]]."""
    hs = _lm_rows("h", h)
    T, D = _lm_rc_common(h, w, cm)
    V = _lm_common(w, labels, count, T, D)
    _cuda_contig("loss", loss, (torch.float32,))
    _check(loss.numel() == 2, "loss must hold two fp32 values (sum, mean)")
    if coef is not None:
        _cuda_contig("coef", coef, (torch.float32,))
        _check(tuple(coef.shape) == (T, V), f"coef must be [{T}, {V}]")
    nws = N.lib().dna_lm_head_rc_fwd_workspace(T, D, V)
    ws = torch.empty(nws // 8 + 2, device=h.device, dtype=torch.float64)
    N.call("dna_lm_head_rc_fwd", h.data_ptr(), hs, _DT[h.dtype], w.data_ptr(), _DT[w.dtype],
           cm.data_ptr(), labels.data_ptr(), T, D, V, float(denom), loss.data_ptr(),
           count.data_ptr(), loss.data_ptr() + 4, _p(coef), ws.data_ptr(), ws.numel() * 8,
           N.stream_ptr())


@torch.library.custom_op("dna_amd::lm_head_rc_bwd", mutates_args=("dh", "dw"))
def lm_head_rc_bwd(coef: torch.Tensor, h: torch.Tensor, w: torch.Tensor, cm: torch.Tensor,
                   labels: torch.Tensor, count: torch.Tensor, upstream: torch.Tensor | None,
                   denom: float, dh: torch.Tensor, dw: torch.Tensor, accumulate: bool) -> None:
    """Backward of lm_head_rc_fwd: dh [T, 2 D] as lm_head_bwd writes it, and dw [V, D] fp32 with
    the gradient of the gathered rows w[cm] folded back in a fixed order (accumulate: added)."""
    hs = _lm_rows("h", h)
    ds = _lm_rows("dh", dh)
    T, D = _lm_rc_common(h, w, cm)
    V = _lm_common(w, labels, count, T, D)
    _check(dh.shape == h.shape and dh.dtype == h.dtype, "dh must match h")
    for n, t, shape in (("coef", coef, (T, V)), ("dw", dw, (V, D))):
        _cuda_contig(n, t, (torch.float32,))
        _check(tuple(t.shape) == shape, f"{n} must be {shape}, got {tuple(t.shape)}")
    if upstream is not None:
        _cuda_contig("upstream", upstream, (torch.float32,))
        _check(upstream.numel() == 1, "upstream must hold one fp32 value")
    nws = N.lib().dna_lm_head_rc_bwd_workspace(T, D, V)
    ws = torch.empty(nws // 4 + 4, device=h.device, dtype=torch.float32)
    N.call("dna_lm_head_rc_bwd", coef.data_ptr(), h.data_ptr(), hs, _DT[h.dtype], w.data_ptr(),
           _DT[w.dtype], cm.data_ptr(), labels.data_ptr(), count.data_ptr(), _p(upstream),
           float(denom), T, D, V, dh.data_ptr(), ds, dw.data_ptr(), int(accumulate),
           ws.data_ptr(), ws.numel() * 4, N.stream_ptr())


# ------------------------------------------------------------------------------- dilated conv
_DCONV_EPI = {"plain": N.DCONV_PLAIN, "gate": N.DCONV_GATE, "main_mul": N.DCONV_MAIN_MUL,
              "main_add": N.DCONV_MAIN_ADD}
_DCONV_ACT = {"none": N.ACT_NONE, "gelu": N.ACT_GELU, "sigmoid": N.ACT_SIGMOID,
              "relu": N.ACT_RELU}  # relu: onehot_conv_* only (dna_dconv_fwd refuses it)


def _dconv_x(name, t, like=None):
    _cuda_contig(name, t, (torch.bfloat16, torch.float32))
    _check(t.dim() == 3, f"{name} must be [B, L, C], got {tuple(t.shape)}")
    if like is not None:
        _check(t.shape == like.shape and t.dtype == like.dtype, f"{name} must match x")
    return t.shape


def _dconv_res(name, t, x):
    _cuda_contig(name, t, (torch.float32,))
    _check(t.shape == x.shape, f"{name} must be fp32 {tuple(x.shape)}")


@torch.library.custom_op("dna_amd::dconv_fwd", mutates_args=("out", "z_out", "res_out"))
def dconv_fwd(x: torch.Tensor, w_taps: torch.Tensor, bias: torch.Tensor | None, dilation: int,
              epilogue: str, act: str, g: torch.Tensor | None, res: torch.Tensor | None,
              out: torch.Tensor | None, z_out: torch.Tensor | None,
              res_out: torch.Tensor | None) -> None:
    """The dilated convolution of x [B, L, C] with the tap-major weight w_taps [K, C, C] and one
    of the epilogues plain | gate | main_mul | main_add (dna_dconv_fwd, include/dna_amd.h)."""
    B, L, C = _dconv_x("x", x)
    _cuda_contig("w_taps", w_taps, (x.dtype,))
    _check(w_taps.dim() == 3 and tuple(w_taps.shape[1:]) == (C, C),
           f"w_taps must be [K, {C}, {C}] in x's dtype, got {tuple(w_taps.shape)}")
    _check(epilogue in _DCONV_EPI and act in _DCONV_ACT, f"epilogue {epilogue!r} / act {act!r}")
    if bias is not None:
        _cuda_contig("bias", bias, (torch.float32,))
        _check(bias.numel() == C, "bias must hold C floats")
    for n, t in (("g", g), ("out", out), ("z_out", z_out)):
        if t is not None:
            _dconv_x(n, t, x)
    for n, t in (("res", res), ("res_out", res_out)):
        if t is not None:
            _dconv_res(n, t, x)
    N.call("dna_dconv_fwd", x.data_ptr(), _DT[x.dtype], w_taps.data_ptr(), _p(bias), B, L, C,
           w_taps.shape[0], int(dilation), _DCONV_EPI[epilogue], _DCONV_ACT[act], _p(g), _p(res),
           _p(out), _p(z_out), _p(res_out), N.stream_ptr())


@torch.library.custom_op("dna_amd::dconv_bwd_elem", mutates_args=("dz_h", "dz_g"))
def dconv_bwd_elem(dfeat: torch.Tensor, drc: torch.Tensor | None, z_h: torch.Tensor,
                   g: torch.Tensor | None, z_g: torch.Tensor | None, forget: bool,
                   dz_h: torch.Tensor, dz_g: torch.Tensor) -> None:
    """dz_h, dz_g of one gated layer from the gradients of its two new residual streams."""
    _dconv_x("z_h", z_h)
    _dconv_res("dfeat", dfeat, z_h)
    if drc is not None:
        _dconv_res("drc", drc, z_h)
    for n, t in (("g", g), ("z_g", z_g), ("dz_h", dz_h), ("dz_g", dz_g)):
        if t is not None:
            _dconv_x(n, t, z_h)
    _check((g if forget else z_g) is not None, "forget needs g, otherwise z_g")
    N.call("dna_dconv_bwd_elem", dfeat.data_ptr(), _p(drc), z_h.data_ptr(), _p(g), _p(z_g),
           _DT[z_h.dtype], z_h.numel(), int(forget), dz_h.data_ptr(), dz_g.data_ptr(),
           N.stream_ptr())


@torch.library.custom_op("dna_amd::dconv_wgrad", mutates_args=("dw", "dbias"))
def dconv_wgrad(dz: torch.Tensor, x: torch.Tensor, dilation: int, dw: torch.Tensor,
                dbias: torch.Tensor | None, accumulate: bool) -> None:
    """dw [C, C, K] (+)= the weight gradient, dbias [C] (+)= sum dz, both fp32, deterministic."""
    B, L, C = _dconv_x("x", x)
    _dconv_x("dz", dz, x)
    _cuda_contig("dw", dw, (torch.float32,))
    _check(dw.dim() == 3 and tuple(dw.shape[:2]) == (C, C), f"dw must be [{C}, {C}, K]")
    if dbias is not None:
        _cuda_contig("dbias", dbias, (torch.float32,))
        _check(dbias.numel() == C, "dbias must hold C floats")
    K = dw.shape[2]
    nws = N.lib().dna_dconv_wgrad_workspace(B, L, C, K)
    ws = torch.empty(max(nws, 16) // 4, device=x.device, dtype=torch.float32)
    N.call("dna_dconv_wgrad", dz.data_ptr(), x.data_ptr(), _DT[x.dtype], B, L, C, K, int(dilation),
           dw.data_ptr(), _p(dbias), int(accumulate), ws.data_ptr(), ws.numel() * 4,
           N.stream_ptr())


def _onehot_args(ids, w, bias):
    _cuda_contig("input_ids", ids, (torch.int64,))
    _check(ids.dim() == 2, "input_ids must be [B, L]")
    _cuda_contig("w", w, (torch.float32,))
    _check(w.dim() == 3, "w must be [C, V, KW]")
    if bias is not None:
        _cuda_contig("bias", bias, (torch.float32,))
        _check(bias.numel() == w.shape[0], "bias must hold C floats")
    return ids.shape[0], ids.shape[1], w.shape[0], w.shape[1], w.shape[2]


@torch.library.custom_op("dna_amd::onehot_conv_fwd", mutates_args=("out",))
def onehot_conv_fwd(input_ids: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None,
                    complement: bool, act: str, out: torch.Tensor) -> None:
    """out [B, L, C] fp32 = act(Conv1d(V, C, KW)(one_hot(ids))) as a table lookup."""
    B, L, C, V, KW = _onehot_args(input_ids, w, bias)
    _cuda_contig("out", out, (torch.float32,))
    _check(tuple(out.shape) == (B, L, C), f"out must be {(B, L, C)}")
    N.call("dna_onehot_conv_fwd", input_ids.data_ptr(), w.data_ptr(), _p(bias), B, L, C, V, KW,
           int(complement), _DCONV_ACT[act], out.data_ptr(), N.stream_ptr())


@torch.library.custom_op("dna_amd::onehot_conv_bwd", mutates_args=("dw", "dbias"))
def onehot_conv_bwd(input_ids: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None,
                    dout: torch.Tensor, complement: bool, act: str, dw: torch.Tensor,
                    dbias: torch.Tensor | None, accumulate: bool) -> None:
    """dw [C, V, KW] and dbias [C] (+)= the gradients of onehot_conv_fwd, deterministic."""
    B, L, C, V, KW = _onehot_args(input_ids, w, bias)
    _cuda_contig("dout", dout, (torch.float32,))
    _check(tuple(dout.shape) == (B, L, C), f"dout must be {(B, L, C)}")
    _cuda_contig("dw", dw, (torch.float32,))
    _check(dw.shape == w.shape, "dw must match w")
    if dbias is not None:
        _cuda_contig("dbias", dbias, (torch.float32,))
        _check(dbias.numel() == C, "dbias must hold C floats")
    nws = N.lib().dna_onehot_conv_bwd_workspace(B, L, C, V, KW)
    ws = torch.empty(max(nws, 16) // 4, device=dout.device, dtype=torch.float32)
    N.call("dna_onehot_conv_bwd", input_ids.data_ptr(), w.data_ptr(), _p(bias), dout.data_ptr(),
           B, L, C, V, KW, int(complement), _DCONV_ACT[act], dw.data_ptr(), _p(dbias),
           int(accumulate), ws.data_ptr(), ws.numel() * 4, N.stream_ptr())


OPS = ("attn_fwd", "attn_bwd", "attn_varlen_fwd", "attn_varlen_bwd", "alibi_attn_qkvpacked",
       "flash_attn_qkvpacked", "linear_fwd", "transpose_bf16", "geglu_linear_fwd", "geglu_linear_dgrad",
       "geglu_fwd", "geglu_bwd", "xent_fwd", "cls_head_fwd", "cls_loss", "cls_head_bwd", "pool_head_fwd",
       "pool_head_bwd", "pool_head_wide_fwd", "pool_head_wide_bwd", "lm_head_fwd", "lm_head_bwd",
       "lm_head_rc_fwd", "lm_head_rc_bwd", "dconv_fwd", "dconv_bwd_elem", "dconv_wgrad",
       "onehot_conv_fwd", "onehot_conv_bwd")
