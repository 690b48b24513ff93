"""Autograd Functions over the dna_amd C ABI (HIP kernels on the current torch stream).

Each Function is one fused HIP op with a hand-written backward; the forward, data-gradient and
weight-gradient GEMMs run the MFMA kernels of csrc/gemm.hip (hipBLASLt through torch only for
shapes those kernels do not take, or as the DNA_GEMM_IMPL / DNA_WGRAD_IMPL=torch A/B arm).
No CPU fallback: every op raises if the native library is missing or a tensor is not on a GPU.
"""
import math
import os
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N
from .flat import raw_writes

_DT = {torch.float32: N.F32, torch.bfloat16: N.BF16}


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"dna_amd: unsupported dtype {t.dtype} (fp32 / bf16 only)")


def _gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("dna_amd ops run on the GPU only (no CPU fallback); "
                               f"got a tensor on {t.device}")


def _p(t):
    return None if t is None else t.data_ptr()


class LibraryFallbackError(RuntimeError):
    """A projection left the hand-written kernels for a torch/hipBLASLt GEMM under
    DNA_STRICT_NATIVE=1 (bench.py sets it: the timed step must stay native)."""


_FALLBACK_SEEN = set()


def library_fallback(what, *shapes):
    """Called wherever a projection is about to run on torch.mm / addmm / bmm instead of the
    hand-written MFMA kernels (shapes the kernels do not take, or the DNA_GEMM_IMPL /
    DNA_WGRAD_IMPL=torch A/B arms). DNA_STRICT_NATIVE=1 turns it into an error; otherwise each
    (site, shapes) pair is counted once in `_FALLBACK_SEEN` (tests and bench read it)."""
    key = (what,) + tuple(tuple(s) for s in shapes)
    if os.environ.get("DNA_STRICT_NATIVE", "0") == "1":
        raise LibraryFallbackError(f"dna_amd: {what} {shapes} would run on a library GEMM "
                                   "(DNA_STRICT_NATIVE=1)")
    _FALLBACK_SEEN.add(key)


class OpTimer:
    """Optional HIP-event timing of ops on the stream they launch on (bench.py roofline).
    Disabled (None) by default: zero overhead on the product path."""
    active = None

    def __init__(self):
        self.pending = []  # (name, units, start_event, end_event)

    def __enter__(self):
        OpTimer.active = self
        return self

    def __exit__(self, *exc):
        OpTimer.active = None

    def summary(self):
        """{name: (launches, mean_ms, units_per_launch, kind)} after a device synchronize;
        kind "flop" (MFMA-bound: algorithmic FLOPs) or "byte" (HBM-bound: algorithmic bytes)."""
        acc = {}
        for name, units, kind, a, b in self.pending:
            n, t, u, _ = acc.get(name, (0, 0.0, 0.0, kind))
            acc[name] = (n + 1, t + a.elapsed_time(b), u + units, kind)
        return {k: (n, t / n, u / n, kind) for k, (n, t, u, kind) in acc.items()}


class _timed:
    __slots__ = ("name", "units", "kind", "t", "a")

    def __init__(self, name, units, kind="flop"):
        self.name, self.units, self.kind, self.t = name, units, kind, OpTimer.active

    def __enter__(self):
        if self.t is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.t is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            self.t.pending.append((self.name, self.units, self.kind, self.a, b))


class DropoutRNG:
    """Counter-based dropout stream: every dropout site draws (seed, offset) and advances the
    offset by the number of Philox4x32 groups it consumes, so backward regenerates the mask.
    MLMTrainer derives the seed from train.seed and the rank; checkpoints keep (seed, offset)."""

    def __init__(self, seed=2222):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.offset = 0

    def take(self, n_elements):
        off = self.offset
        self.offset += (int(n_elements) + 3) // 4 + 1
        return self.seed, off


# ----------------------------------------------------------------------------------- embeddings
class EmbeddingLN(torch.autograd.Function):
    """dropout(LN(E[ids] + type_row)) -> (y fp32, y_bf16|None)   (bert_layers.py:62-107)."""

    @staticmethod
    def forward(ctx, ids, E, tt, gamma, beta, eps, p, seed, off, want_f32, want_bf16):
        _gpu(ids, E, tt, gamma, beta)
        ctx.set_materialize_grads(False)
        T, (V, d) = ids.numel(), E.shape
        y = torch.empty(T, d, device=E.device, dtype=torch.float32) if want_f32 else None
        yb = torch.empty(T, d, device=E.device, dtype=torch.bfloat16) if want_bf16 else None
        mean = torch.empty(T, device=E.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        ids = ids.contiguous()
        N.call("dna_embed_ln_fwd", ids.data_ptr(), E.data_ptr(), tt[0].data_ptr(),
               gamma.data_ptr(), beta.data_ptr(), T, d, V, eps, p, seed, off, _p(y), _p(yb),
               mean.data_ptr(), rstd.data_ptr(), N.stream_ptr())
        ctx.save_for_backward(ids, E, tt, gamma, mean, rstd)
        ctx.cfg = (eps, p, seed, off)
        return y, yb

    @staticmethod
    def backward(ctx, dy, dyb):
        ids, E, tt, gamma, mean, rstd = ctx.saved_tensors
        _, p, seed, off = ctx.cfg
        T, (V, d) = ids.numel(), E.shape
        dtt = torch.zeros_like(tt)
        dg = torch.empty_like(gamma)
        db = torch.empty_like(gamma)
        nws = N.lib().dna_ln_bwd_workspace(T, d)
        ws = torch.empty(max(nws, 16), device=E.device, dtype=torch.uint8)
        dy = None if dy is None else dy.contiguous()
        dyb = None if dyb is None else dyb.contiguous()
        # per-token row gradients, then an id-sorted segmented sum into the table (frequent
        # tokens would otherwise serialise thousands of atomic row adds on one row)
        drows = torch.empty(T, d, device=E.device, dtype=torch.float32)
        N.call("dna_embed_ln_bwd_rows", _p(dy), _p(dyb), ids.data_ptr(), E.data_ptr(),
               tt[0].data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), T, d, V,
               p, seed, off, drows.data_ptr(), dtt[0].data_ptr(), dg.data_ptr(), db.data_ptr(),
               ws.data_ptr(), nws, N.stream_ptr())
        sorted_ids, perm = torch.sort(ids, stable=True)  # fixed summation order run to run
        dE = torch.zeros_like(E)
        nsw = N.lib().dna_embed_grad_segsum_workspace(T, d)
        sw = torch.empty(max(nsw // 4, 4), device=E.device, dtype=torch.float32)
        N.call("dna_embed_grad_segsum", drows.data_ptr(), sorted_ids.data_ptr(), perm.data_ptr(),
               T, d, V, 0, dE.data_ptr(), sw.data_ptr(), nsw, N.stream_ptr())
        # the tied decoder's weight gradient may still be adding into E.grad on the wgrad side
        # stream; AccumulateGrad adds dE into the same buffer on this stream next
        join_side_stream()
        return None, dE, dtt, dg, db, None, None, None, None, None, None


class EmbeddingFn(torch.autograd.Function):
    """E[ids] with the table gradient of dna_embed_grad_segsum (ids sorted once, rows summed per
    run of equal ids in a fixed order: deterministic, no atomics) instead of torch's
    embedding_dense_backward -- with a 16-symbol character vocabulary every id owns thousands of
    rows, which that path serialises (0.65 ms per HyenaDNA step at L = 65,536)."""

    @staticmethod
    def forward(ctx, ids, E, padding_idx):
        _gpu(ids, E)
        ctx.save_for_backward(ids)
        ctx.cfg = (E.shape, padding_idx)
        return F.embedding(ids, E, padding_idx)

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        (V, d), pad = ctx.cfg
        flat = ids.reshape(-1).contiguous()
        T = flat.numel()
        drows = dy.reshape(T, d).float().contiguous()
        sorted_ids, perm = torch.sort(flat, stable=True)
        dE = torch.zeros(V, d, device=dy.device, dtype=torch.float32)
        nsw = N.lib().dna_embed_grad_segsum_workspace(T, d)
        sw = torch.empty(max(nsw // 4, 4), device=dy.device, dtype=torch.float32)
        N.call("dna_embed_grad_segsum", drows.data_ptr(), sorted_ids.data_ptr(), perm.data_ptr(),
               T, d, V, -1 if pad is None else pad, dE.data_ptr(), sw.data_ptr(), nsw,
               N.stream_ptr())
        join_side_stream()  # a tied head's weight gradient may be on the wgrad side stream
        return None, dE, None


def embedding(ids, weight, padding_idx=None):
    """F.embedding(ids, weight, padding_idx) with EmbeddingFn's backward for fp32 CUDA tables of
    width 64k <= 1024 (torch's otherwise)."""
    V, d = weight.shape
    if (ids.is_cuda and weight.dtype == torch.float32 and d % 64 == 0 and d <= 1024
            and ids.dtype in (torch.int64, torch.int32) and torch.is_grad_enabled()
            and weight.requires_grad):
        if padding_idx is not None and padding_idx < 0:
            padding_idx += V
        return EmbeddingFn.apply(ids.long(), weight, padding_idx)
    return F.embedding(ids, weight, padding_idx)


class HipEmbedding(nn.Embedding):
    """nn.Embedding (same parameter / state_dict) whose table gradient is the deterministic
    segmented sum (functional.embedding); max_norm / scale_grad_by_freq / sparse keep torch's."""

    def forward(self, ids):
        if self.max_norm is not None or self.scale_grad_by_freq or self.sparse:
            return super().forward(ids)
        return embedding(ids, self.weight, self.padding_idx)


def strided_gemm(A, sa, B, sb, C, sc, M, Nc, K, batch, splits=1, out_f32=None, bias_n=None,
                 accumulate=False):
    """C[z][m][n] = sum_k A(m, k) B(k, n) (+ bias_n[n], fp32) on dna_gemm_bf16_strided /
    dna_gemm_f32_strided (z = batch * splits + split). sa = (sam, sak, saz), sb = (sbk, sbn, sbz),
    sc = (ldc, scz); strides in elements. accumulate (bf16 operands, splits == 1): C += A B in the
    epilogue."""
    bn = None if bias_n is None else bias_n.data_ptr()
    if A.dtype == torch.bfloat16:
        assert B.dtype == torch.bfloat16
        f32 = C.dtype == torch.float32 if out_f32 is None else out_f32
        N.call("dna_gemm_bf16_strided", A.data_ptr(), *sa, B.data_ptr(), *sb, C.data_ptr(), *sc,
               int(f32) | (2 if accumulate else 0), None, bn, M, Nc, K, batch, splits,
               N.stream_ptr())
    else:
        if accumulate:
            raise NotImplementedError("strided_gemm: accumulate needs bf16 operands")
        assert A.dtype == B.dtype == C.dtype == torch.float32
        N.call("dna_gemm_f32_strided", A.data_ptr(), *sa, B.data_ptr(), *sb, C.data_ptr(), *sc,
               bn, M, Nc, K, batch, splits, N.stream_ptr())


class StridedLinear(torch.autograd.Function):
    """y[L, N] = x[L, K] . w[N, K]^T + b on the strided MFMA GEMM (dna_gemm_bf16_strided /
    dna_gemm_f32_strided) for skinny projections over many tokens (the HyenaDNA implicit-filter
    MLP, the char-vocabulary LM heads): the weight gradient's L-long contraction runs as fp32
    split-K slices summed once by dna_sum_slices_accum (rounded once, as one GEMM with fp32
    accumulation would), the bias gradient as an fp32 column sum. x / w / b in one dtype."""

    @staticmethod
    def forward(ctx, x, w, b):
        _gpu(x, w, b)
        L, K = x.shape
        Nn = w.shape[0]
        x = x.contiguous()
        w = w.contiguous()
        y = torch.empty(L, Nn, device=x.device, dtype=x.dtype)
        bf = None if b is None else b.float().contiguous()
        with _timed("strided_linear", (L * (K + Nn)) * x.element_size(), "byte"):
            strided_gemm(x, (K, 1, 0), w, (1, K, 0), y, (Nn, 0), L, Nn, K, 1, bias_n=bf)
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        L, K = x.shape
        Nn = w.shape[0]
        dy = dy.contiguous().to(x.dtype)
        dx = None
        if ctx.needs_input_grad[0]:  # dx[L, K] = dy[L, N] . w[N, K]
            dx = torch.empty(L, K, device=x.device, dtype=x.dtype)
            strided_gemm(dy, (Nn, 1, 0), w, (K, 1, 0), dx, (K, 0), L, K, Nn, 1)
        s = int(N.lib().dna_gemm_strided_splits(Nn, K, L, 1))
        part = torch.empty(s, Nn, K, device=x.device, dtype=torch.float32)
        if x.dtype == torch.bfloat16:  # dW[N, K] = sum_l dy[l, n] x[l, k]
            strided_gemm(dy, (1, Nn, 0), x, (K, 1, 0), part, (K, Nn * K), Nn, K, L, 1, s,
                            out_f32=True)
        else:
            strided_gemm(dy, (1, Nn, 0), x, (K, 1, 0), part, (K, Nn * K), Nn, K, L, 1, s)
        dw = torch.empty(Nn, K, device=x.device, dtype=torch.float32)
        N.call("dna_sum_slices", part.data_ptr(), s, Nn * K, dw.data_ptr(), N.stream_ptr())
        db = dy.float().sum(0).to(dy.dtype) if ctx.has_b else None
        return dx, dw.to(w.dtype), db


def strided_linear(x, weight, bias=None):
    """F.linear(x, weight, bias) with nn.Linear's dtype flow (under autocast x, W and b in the
    autocast dtype, output in it, bias added inside the product) on StridedLinear; x [..., K]."""
    w, b = weight, bias
    if torch.is_autocast_enabled(x.device.type):
        dt = torch.get_autocast_dtype(x.device.type)
        x, w, b = x.to(dt), w.to(dt), (b.to(dt) if b is not None else None)
    else:
        b = b.to(x.dtype) if b is not None else None
        w = w.to(x.dtype)
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise NotImplementedError(f"strided_linear in {x.dtype}")
    lead = x.shape[:-1]
    with torch.autocast(x.device.type, enabled=False):
        y = StridedLinear.apply(x.reshape(-1, x.shape[-1]), w, b)
    return y.reshape(*lead, w.shape[0])


# ----------------------------------------------------------------------------------- fused LN
_PARAM_DIRECT = os.environ.get("DNA_PARAM_GRAD_DIRECT", "1") != "0"  # 0: AccumulateGrad (A/B)


def _param_grads_direct(params):
    """Every parameter of the tuple (None entries skipped) is FlatParams-owned with direct
    gradients on (dna_amd.flat.enable_direct_grad) and holds its fp32 .grad view: the kernel may
    then add its gradient there itself. Only for loss.backward() into those buffers."""
    ps = [q for q in params if q is not None]
    return _PARAM_DIRECT and bool(ps) and all(getattr(q, "_dna_direct", False) and q.grad is not None
                            and q.grad.dtype == torch.float32 and q.grad.is_contiguous()
                            for q in ps)


def _notify_direct(*params):
    """After a kernel has added its gradients straight into the .grad views of these parameters
    (None entries skipped): tell whoever counts their contributions (ddp.GradBucketReducer)."""
    for q in params:
        notify = getattr(q, "_dna_notify", None) if q is not None else None
        if notify is not None:
            notify(q)


class FusedLayerNorm(torch.autograd.Function):
    """LN(dropout(act(x + bias)) + residual) -> (y fp32|None, y_bf16|None).

    BertSelfOutput (bert_layers.py:209-214), GeGLU-MLP tail (:298-300), head transform
    (:524-528, act=gelu, eps=1e-12)."""

    @staticmethod
    def forward(ctx, x, bias, residual, gamma, beta, eps, act, p, seed, off, want_f32, want_bf16):
        _gpu(x, bias, residual, gamma, beta)
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        n, d = x.shape
        y = torch.empty(n, d, device=x.device, dtype=torch.float32) if want_f32 else None
        yb = torch.empty(n, d, device=x.device, dtype=torch.bfloat16) if want_bf16 else None
        mean = torch.empty(n, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        residual = None if residual is None else residual.contiguous()
        es = x.element_size()
        nbytes = n * (d * (es + (4 if residual is not None else 0) + (4 if want_f32 else 0)
                           + (2 if want_bf16 else 0)) + 8)
        with _timed("ln_fwd", nbytes, "byte"):
            N.call("dna_ln_fwd", x.data_ptr(), _dt(x), _p(bias), act, p, seed, off, _p(residual),
                   gamma.data_ptr(), beta.data_ptr(), n, d, eps, _p(y), _p(yb), mean.data_ptr(),
                   rstd.data_ptr(), N.stream_ptr())
        # backward from the fp32 output (x_hat = (y - beta) / gamma, dna_ln_bwd_from_y): one fp32
        # row read instead of x + the residual, and neither is kept alive for the backward --
        # where (gamma, beta) leave it as accurate as the recomputation from x (ln_from_y_ok)
        ctx.from_y = (y is not None and act == N.ACT_NONE and _LN_BWD_FROM_Y
                      and any(ctx.needs_input_grad[:5]) and _ln_from_y_verdict(gamma, beta))
        if ctx.from_y:
            ctx.save_for_backward(y, bias, gamma, beta, rstd)
            ctx.shape = (n, d, x.dtype, residual is not None)
            # the parameters themselves (their .grad / FlatParams flags), for _param_grads_direct
            ctx.params = (bias, gamma, beta)
        else:
            ctx.save_for_backward(x, bias, residual, gamma, mean, rstd)
        ctx.cfg = (act, p, seed, off)
        return y, yb

    @staticmethod
    def backward(ctx, dy, dyb):
        if ctx.from_y:
            return FusedLayerNorm._backward_from_y(ctx, dy, dyb)
        x, bias, residual, gamma, mean, rstd = ctx.saved_tensors
        act, p, seed, off = ctx.cfg
        n, d = x.shape
        dx = torch.empty_like(x)
        dres = torch.empty(n, d, device=x.device, dtype=torch.float32) if residual is not None else None
        dg = torch.empty_like(gamma)
        db = torch.empty_like(gamma)
        dbias = torch.empty_like(bias) if bias is not None else None
        nws = N.lib().dna_ln_bwd_workspace(n, d)
        ws = torch.empty(max(nws, 16), device=x.device, dtype=torch.uint8)
        dy = None if dy is None else dy.contiguous()
        dyb = None if dyb is None else dyb.contiguous()
        es = x.element_size()
        # reads dy / dy_bf16, x, residual; writes dx and (with a residual) d(residual) fp32
        nbytes = n * (d * ((4 if dy is not None else 0) + (2 if dyb is not None else 0) + 2 * es
                           + (8 if residual is not None else 0)) + 8)
        with _timed("ln_bwd", nbytes, "byte"):
            N.call("dna_ln_bwd", _p(dy), _p(dyb), x.data_ptr(), _dt(x), _p(bias), act, p, seed,
                   off, _p(residual), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), n, d,
                   _p(dres), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), _p(dbias), ws.data_ptr(),
                   nws, N.stream_ptr())
        return dx, dbias, dres, dg, db, None, None, None, None, None, None, None

    @staticmethod
    def _backward_from_y(ctx, dy, dyb):
        y, bias, gamma, beta, rstd = ctx.saved_tensors
        act, p, seed, off = ctx.cfg
        n, d, xdt, has_res = ctx.shape
        dx = torch.empty(n, d, device=y.device, dtype=xdt)
        dres = torch.empty(n, d, device=y.device, dtype=torch.float32) if has_res else None
        direct = _param_grads_direct(ctx.params)
        if direct:
            # dgamma / dbeta / dbias added straight into the flat fp32 gradient (dna_amd.flat)
            # by the partial-sum pass, instead of three AccumulateGrad adds
            pb, pg, pbe = ctx.params
            dg, db, dbias = pg.grad, pbe.grad, (pb.grad if pb is not None else None)
        else:
            dg = torch.empty_like(gamma)
            db = torch.empty_like(gamma)
            dbias = torch.empty_like(bias) if bias is not None else None
        nws = N.lib().dna_ln_bwd_workspace(n, d)
        ws = torch.empty(max(nws, 16), device=y.device, dtype=torch.uint8)
        dy = None if dy is None else dy.contiguous()
        dyb = None if dyb is None else dyb.contiguous()
        es = dx.element_size()
        # reads dy / dy_bf16 and y; writes dx and (with a residual) d(residual) fp32
        nbytes = n * (d * ((4 if dy is not None else 0) + (2 if dyb is not None else 0) + 4 + es
                           + (4 if has_res else 0)) + 4)
        with _timed("ln_bwd", nbytes, "byte"):
            N.call("dna_ln_bwd_from_y_acc" if direct else "dna_ln_bwd_from_y", _p(dy), _p(dyb),
                   y.data_ptr(), _dt(dx), p, seed, off, gamma.data_ptr(), beta.data_ptr(),
                   rstd.data_ptr(), n, d, _p(dres), dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                   _p(dbias), ws.data_ptr(), nws, N.stream_ptr())
        if direct:
            _notify_direct(*ctx.params)
            return dx, None, dres, None, None, None, None, None, None, None, None, None
        return dx, dbias, dres, dg, db, None, None, None, None, None, None, None


# DNA_LN_BWD_FROM_Y=0: the LayerNorm backward recomputes x_hat from x (+ bias, dropout) + the
# residual instead of from the fp32 output (A/B switch)
_LN_BWD_FROM_Y = os.environ.get("DNA_LN_BWD_FROM_Y", "1") != "0"

# Which (gamma, beta) may take the from-y backward. The forward's fp32 y carries a rounding of
# 2^-24 |y| <= 2^-24 (|beta_k| + |gamma_k| |x_hat|); (y - beta) / gamma turns it into an x_hat
# error of about 2^-24 (|beta_k| / |gamma_k| + |x_hat|), against 2^-24 |x_hat| for the
# recomputation from x. So the from-y path is as accurate only while max_k |beta_k| / |gamma_k|
# is small, and it needs every |gamma_k| > 0 (2^-64: y and 1 / gamma stay normal fp32 numbers).
# Measured on the MI355X against fp64 (tests/test_gpu_layernorm_fp64.py (c): 1000 rows, 128 and
# 768 columns, four columns at gamma = +-t, two of them with beta = 1; error of dgamma relative
# to fp32 torch's error, 1.4e-7, over the four shapes; the recompute path stays at 1 to 2.5):
#   |beta / gamma| = 10 (t = 1e-1): 1.2 .. 2.6      100 (t = 1e-2): 6.7 .. 12.5
#   1e3: 44 .. 99       1e4: 335 .. 1010       1e6: 6.5e4 .. 2.6e5       gamma = 0: 3e6 .. 6e6
# The tests allow 8. The error grows linearly in the ratio (about 0.11 per unit at worst), which
# puts 16 at 3.3 or less: inside the bound with room to spare, 100 is outside it.
LN_FROM_Y_MAX_RATIO = 16.0
LN_FROM_Y_MIN_GAMMA = 2.0 ** -64


def ln_from_y_ok(gamma, beta, margin=0.0, shrink=0.0):
    """Whether a LayerNorm with these parameters may take the from-y backward: every column has
    g = |gamma| (1 - shrink) - margin >= LN_FROM_Y_MIN_GAMMA and |beta| + margin <=
    LN_FROM_Y_MAX_RATIO * g (NaN fails). margin / shrink: absolute / relative distance the
    parameters may still move with the verdict standing (LNFromYGuard); 0 for the values as they
    are. Pure function of the two tensors, on any device (one host read of the result)."""
    g = gamma.detach().float().abs() * (1.0 - shrink) - margin
    b = beta.detach().float().abs() + margin
    return bool(((g >= LN_FROM_Y_MIN_GAMMA) & (b <= LN_FROM_Y_MAX_RATIO * g)).all())


def _ln_from_y_verdict(gamma, beta):
    """ln_from_y_ok(gamma, beta), cached on gamma as (ok, beta, gamma._version, beta._version,
    last raw-write count it holds for). A hit costs no device work. A miss -- the first forward
    of a pair, a direct caller's fresh tensors, an in-place change torch saw (load_state_dict), a
    fused AdamW step with no LNFromYGuard refreshing the entry -- computes it with a host
    synchronisation. The trainers keep the entries of their LayerNorms fresh (LNFromYGuard)."""
    now = raw_writes()
    c = getattr(gamma, "_dna_ln_verdict", None)
    if (c is not None and c[1] is beta and c[2] == gamma._version and c[3] == beta._version
            and c[4] >= now):
        return c[0]
    ok = ln_from_y_ok(gamma, beta)
    gamma._dna_ln_verdict = (ok, beta, gamma._version, beta._version, now)
    return ok


class LNFromYGuard:
    """Keeps the from-y verdicts of a FlatParams' LayerNorms fresh without a host synchronisation
    in the training step. The fused AdamW step rewrites gamma and beta through raw pointers, so a
    cached verdict would go stale unseen. After each optimizer step `launch()` runs one small
    kernel over every (gamma, beta) pair a FusedLayerNorm has seen (dna_ln_from_y_check) and
    copies the verdicts to pinned host memory, with an event; `poll()`, at the start of a step,
    takes over whatever has arrived without blocking.

    A verdict is computed MAX_AGE optimizer steps inside the accuracy threshold: AdamW moves a
    parameter by at most lr * max(1, (1 - b1) / sqrt(1 - b2)) <= 3.2 lr per step (b = (0.9,
    0.999)) plus lr * weight_decay * |p| of decay, so with margin = MAX_AGE * 3.2 * lr and
    shrink = MAX_AGE * lr * weight_decay a verdict stays right for MAX_AGE steps and a stale one
    cannot be wrong. poll() blocks only when the newest verdict taken over is older than that --
    the host more than MAX_AGE steps ahead of the device."""

    MAX_AGE = 16

    def __init__(self, flat, opt):
        self.flat, self.opt = flat, opt
        self._pending = []  # (event, host verdicts, pairs with their versions, raw-write count)
        self._free = []     # pinned host buffers to reuse
        self._key, self._dev = None, None
        self._good_until = -1

    def _pairs(self):
        out = []
        for g in self.flat.params:
            c = getattr(g, "_dna_ln_verdict", None)
            if c is not None and id(c[1]) in self.flat._index:
                out.append((g, c[1]))
        return out

    def launch(self):
        """After the optimizer step, on its stream."""
        pairs = self._pairs()
        if not pairs or not self.flat.flat.is_cuda:
            return
        dev = self.flat.flat.device
        key = tuple((id(g), id(b)) for g, b in pairs)
        if key != self._key:
            goff = [self.flat.slice_of(g)[0] for g, _ in pairs]
            boff = [self.flat.slice_of(b)[0] for _, b in pairs]
            cols = [g.numel() for g, _ in pairs]
            self._dev = (torch.tensor(goff, dtype=torch.int64, device=dev),
                         torch.tensor(boff, dtype=torch.int64, device=dev),
                         torch.tensor(cols, dtype=torch.int32, device=dev),
                         torch.empty(len(pairs), dtype=torch.int32, device=dev))
            self._key, self._free = key, []
        goff, boff, cols, ok = self._dev
        g0 = self.opt.param_groups[0]
        lr = max(float(g0["lr"]), float(g0.get("initial_lr", 0.0)))
        b1, b2 = g0["betas"]
        per_step = max(3.2, (1.0 - b1) / math.sqrt(1.0 - b2))
        N.call("dna_ln_from_y_check", self.flat.flat.data_ptr(), goff.data_ptr(), boff.data_ptr(),
               cols.data_ptr(), len(pairs), LN_FROM_Y_MAX_RATIO, LN_FROM_Y_MIN_GAMMA,
               self.MAX_AGE * per_step * lr, self.MAX_AGE * lr * float(g0["weight_decay"]),
               ok.data_ptr(), N.stream_ptr(dev))
        host = self._free.pop() if self._free else torch.empty(len(pairs), dtype=torch.int32,
                                                               pin_memory=True)
        host.copy_(ok, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((ev, host, [(g, b, g._version, b._version) for g, b in pairs],
                              raw_writes()))

    def _take(self, item):
        _, host, pairs, at = item
        for (g, b, gv, bv), ok in zip(pairs, host.tolist()):
            if g._version == gv and b._version == bv:  # else: changed since, the forward recomputes
                g._dna_ln_verdict = (bool(ok), b, gv, bv, at + self.MAX_AGE)
        self._good_until = at + self.MAX_AGE
        if len(host) == len(self._key or ()):
            self._free.append(host)

    def poll(self):
        """Before a step's forward: take over every finished check; wait for one only if the
        verdicts held have run out."""
        now = raw_writes()
        while self._pending and self._pending[0][0].query():
            self._take(self._pending.pop(0))
        if self._good_until >= now:
            return
        for i, item in enumerate(self._pending):
            if item[3] + self.MAX_AGE >= now:
                item[0].synchronize()
                for it in self._pending[:i + 1]:
                    self._take(it)
                del self._pending[:i + 1]
                return


class AddLayerNorm(torch.autograd.Function):
    """Pre-norm residual add + LN: (x, residual fp32) -> (sum = x + residual fp32, LN(sum) fp32
    or bf16) in one pass (dna_add_ln_fwd); beta None = RMSNorm (mamba_ssm's fused add + RMSNorm
    of the Caduceus Blocks). The flash_attn Block's `residual = dropout(x) +
    residual; norm(residual)` with residual_in_fp32 and dropout p = 0 (HyenaDNA's Blocks,
    long_conv_lm.py:205-267): same fp32 sum, same LN. The backward adds the gradient of `sum`
    from the residual stream to the LN's input gradient in the same kernel (dna_add_ln_bwd), so
    the add node, autograd's gradient accumulation and the cast of x's gradient are gone."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps, want_bf16):
        _gpu(x, residual, gamma, beta)
        ctx.set_materialize_grads(False)
        x, residual = x.contiguous(), residual.contiguous()
        n, d = x.shape
        rms = beta is None  # RMSNorm (AddRMSNorm)
        s = torch.empty(n, d, device=x.device, dtype=torch.float32)
        y = torch.empty(n, d, device=x.device, dtype=torch.bfloat16 if want_bf16 else torch.float32)
        mean = None if rms else torch.empty(n, device=x.device, dtype=torch.float32)
        rstd = torch.empty(n, device=x.device, dtype=torch.float32)
        nbytes = n * (d * (x.element_size() + 8 + y.element_size()) + 8)
        with _timed("ln_fwd", nbytes, "byte"):
            N.call("dna_add_ln_fwd", x.data_ptr(), _dt(x), residual.data_ptr(), gamma.data_ptr(),
                   _p(beta), n, d, eps, int(rms), s.data_ptr(),
                   None if want_bf16 else y.data_ptr(), y.data_ptr() if want_bf16 else None,
                   _p(mean), rstd.data_ptr(), N.stream_ptr())
        ctx.save_for_backward(x, residual, gamma, mean, rstd)
        ctx.rms = rms
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        x, residual, gamma, mean, rstd = ctx.saved_tensors
        rms = ctx.rms
        n, d = x.shape
        dx = torch.empty_like(x)
        dres = torch.empty(n, d, device=x.device, dtype=torch.float32)
        dg = torch.empty_like(gamma)
        db = None if rms else torch.empty_like(gamma)
        nws = N.lib().dna_ln_bwd_workspace(n, d)
        ws = torch.empty(max(nws, 16), device=x.device, dtype=torch.uint8)
        dy = None if dy is None else dy.contiguous()
        ds = None if ds is None else ds.contiguous().float()
        dyf = dy if (dy is not None and dy.dtype == torch.float32) else None
        dyb = dy if (dy is not None and dy.dtype == torch.bfloat16) else None
        nbytes = n * (d * ((4 if dyf is not None else 0) + (2 if dyb is not None else 0)
                           + (4 if ds is not None else 0) + 2 * x.element_size() + 8) + 8)
        with _timed("ln_bwd", nbytes, "byte"):
            N.call("dna_add_ln_bwd", _p(dyf), _p(dyb), _p(ds), x.data_ptr(), _dt(x),
                   residual.data_ptr(), gamma.data_ptr(), _p(mean), rstd.data_ptr(), n, d, int(rms),
                   dres.data_ptr(), dx.data_ptr(), dg.data_ptr(), _p(db), ws.data_ptr(),
                   nws, N.stream_ptr())
        return dx, dres, dg, db, None, None


class RMSNormFn(torch.autograd.Function):
    """x * rsqrt(mean(x^2) + eps) * gamma -> (y fp32|None, y_bf16|None): mamba_ssm's RMSNorm
    as the Caduceus Blocks / norm_f apply it (modeling_caduceus.py:25-65, :214-216)."""

    @staticmethod
    def forward(ctx, x, gamma, eps, want_f32, want_bf16):
        _gpu(x, gamma)
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        n, d = x.shape
        y = torch.empty(n, d, device=x.device, dtype=torch.float32) if want_f32 else None
        yb = torch.empty(n, d, device=x.device, dtype=torch.bfloat16) if want_bf16 else None
        rstd = torch.empty(n, device=x.device, dtype=torch.float32)
        nbytes = n * (d * (x.element_size() + (4 if want_f32 else 0) + (2 if want_bf16 else 0)) + 4)
        with _timed("rms_fwd", nbytes, "byte"):
            N.call("dna_rms_fwd", x.data_ptr(), _dt(x), gamma.data_ptr(), n, d, eps, _p(y), _p(yb),
                   rstd.data_ptr(), N.stream_ptr())
        ctx.save_for_backward(x, gamma, rstd)
        return y, yb

    @staticmethod
    def backward(ctx, dy, dyb):
        x, gamma, rstd = ctx.saved_tensors
        n, d = x.shape
        dx = torch.empty_like(x)
        dg = torch.empty_like(gamma)
        nws = N.lib().dna_ln_bwd_workspace(n, d)
        ws = torch.empty(max(nws, 16), device=x.device, dtype=torch.uint8)
        dy = None if dy is None else dy.contiguous()
        dyb = None if dyb is None else dyb.contiguous()
        nbytes = n * (d * ((4 if dy is not None else 0) + (2 if dyb is not None else 0)
                           + 2 * x.element_size()) + 4)
        with _timed("rms_bwd", nbytes, "byte"):
            N.call("dna_rms_bwd", _p(dy), _p(dyb), x.data_ptr(), _dt(x), gamma.data_ptr(),
                   rstd.data_ptr(), n, d, dx.data_ptr(), dg.data_ptr(), ws.data_ptr(), nws,
                   N.stream_ptr())
        return dx, dg, None, None, None


# ----------------------------------------------------------------------------------- attention
class AlibiAttention(torch.autograd.Function):
    """softmax(q k^T * scale - slope_h |i-j| + pad_bias) v on packed qkv [T, 3*H*D]."""

    @staticmethod
    def forward(ctx, qkv, key_valid, slopes, b, S, H, scale, bias_grad=False):
        _gpu(qkv, key_valid, slopes)
        qkv = qkv.contiguous()
        T = qkv.shape[0]
        D = qkv.shape[1] // (3 * H)
        out = torch.empty(T, H * D, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(b, H, S, device=qkv.device, dtype=torch.float32)
        with _timed("attn_fwd", 4.0 * b * H * S * S * D):
            N.call("dna_attn_fwd", qkv.data_ptr(), _p(key_valid), slopes.data_ptr(), b, S, H, D,
                   _dt(qkv), scale, out.data_ptr(), lse.data_ptr(), N.stream_ptr())
        ctx.save_for_backward(qkv, out, lse, key_valid, slopes)
        ctx.cfg = (b, S, H, D, scale)
        ctx.bias_grad = bias_grad and qkv.dtype == torch.bfloat16
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, key_valid, slopes = ctx.saved_tensors
        b, S, H, D, scale = ctx.cfg
        dqkv = torch.empty_like(qkv)
        delta = torch.empty(b * H * S, device=qkv.device, dtype=torch.float32)
        dout = dout.contiguous()
        part = None
        if ctx.bias_grad:  # column sums of dqkv (the packed projection's bias gradient), fused
            rows = N.lib().dna_attn_dbias_part_rows(b, S)
            part = torch.empty(rows, qkv.shape[1], device=qkv.device, dtype=torch.float32)
        with _timed("attn_bwd", 10.0 * b * H * S * S * D):
            N.call("dna_attn_bwd_ex", qkv.data_ptr(), out.data_ptr(), dout.data_ptr(),
                   lse.data_ptr(), _p(key_valid), slopes.data_ptr(), b, S, H, D, _dt(qkv), scale,
                   dqkv.data_ptr(), delta.data_ptr(), _p(part), N.stream_ptr())
        if part is not None:
            colsum = torch.empty(qkv.shape[1], device=qkv.device, dtype=torch.float32)
            N.call("dna_colsum_f32", part.data_ptr(), part.shape[0], part.shape[1],
                   colsum.data_ptr(), 0, N.stream_ptr())
            # picked up by Linear.backward of the projection that produced qkv (same tensor
            # object: nothing sits between the two nodes), instead of a dy.sum(0) pass
            dqkv._dna_colsum = colsum
        return dqkv, None, None, None, None, None, None, None


def alibi_attention(qkv, key_valid, slopes, b, S, H, scale=None, bias_grad=False):
    """bias_grad: also produce the column sums of dqkv in backward (bf16 path), for the bias of
    the linear layer that made qkv (see Linear.backward)."""
    D = qkv.shape[1] // (3 * H)
    return AlibiAttention.apply(qkv, key_valid, slopes, b, S, H,
                                scale if scale is not None else 1.0 / math.sqrt(D), bias_grad)


class AlibiAttentionVarlen(torch.autograd.Function):
    """AlibiAttention on an unpadded batch: qkv [T, 3*H*D] holds the real tokens only, sequence n
    owns rows cu_seqlens[n] .. cu_seqlens[n+1]-1 and attends within itself; the ALiBi distance is
    taken between `positions` (each token's column in the padded rectangle)."""

    @staticmethod
    def forward(ctx, qkv, cu_seqlens, positions, slopes, nseq, max_seqlen, sq_sum, H, scale):
        _gpu(qkv, cu_seqlens, positions, slopes)
        qkv = qkv.contiguous()
        T = qkv.shape[0]
        D = qkv.shape[1] // (3 * H)
        out = torch.empty(T, H * D, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(H, T, device=qkv.device, dtype=torch.float32)
        with _timed("attn_varlen_fwd", 4.0 * H * sq_sum * D):
            N.call("dna_attn_varlen_fwd", qkv.data_ptr(), cu_seqlens.data_ptr(), _p(positions),
                   slopes.data_ptr(), nseq, T, max_seqlen, H, D, _dt(qkv), scale, out.data_ptr(),
                   lse.data_ptr(), N.stream_ptr())
        ctx.save_for_backward(qkv, out, lse, cu_seqlens, positions, slopes)
        ctx.cfg = (nseq, max_seqlen, sq_sum, H, D, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, cu_seqlens, positions, slopes = ctx.saved_tensors
        nseq, max_seqlen, sq_sum, H, D, scale = ctx.cfg
        T = qkv.shape[0]
        dqkv = torch.empty_like(qkv)
        nws = N.lib().dna_attn_varlen_bwd_workspace(nseq, T, max_seqlen, H)
        ws = torch.empty(nws, device=qkv.device, dtype=torch.uint8)
        dout = dout.contiguous()
        with _timed("attn_varlen_bwd", 10.0 * H * sq_sum * D):
            N.call("dna_attn_varlen_bwd", qkv.data_ptr(), out.data_ptr(), dout.data_ptr(),
                   lse.data_ptr(), cu_seqlens.data_ptr(), _p(positions), slopes.data_ptr(), nseq, T,
                   max_seqlen, H, D, _dt(qkv), scale, dqkv.data_ptr(), ws.data_ptr(),
                   N.stream_ptr())
        return dqkv, None, None, None, None, None, None, None, None


def _check_varlen_index(T, cu_seqlens, positions, nseq):
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.numel() != nseq + 1 or \
            not cu_seqlens.is_contiguous():
        raise ValueError(f"cu_seqlens must be contiguous int32 [{nseq + 1}], got "
                         f"{cu_seqlens.dtype} {tuple(cu_seqlens.shape)}")
    if positions is not None and (positions.dtype != torch.int32 or positions.numel() != T
                                  or not positions.is_contiguous()):
        raise ValueError(f"positions must be contiguous int32 [{T}], got {positions.dtype} "
                         f"{tuple(positions.shape)}")


def alibi_attention_varlen(qkv, packed, slopes, H, scale=None):
    """Packed attention on the T = packed.total real tokens of a batch. `packed`: a PackedIndex
    (dna_amd.bert_layers) already on qkv's device, or anything with its cu_seqlens / positions /
    batch / max_seqlen / total (and optionally sq_sum, the sum of squared lengths, for the op
    timer's FLOP count -- a host int, so nothing here waits for the device)."""
    T = qkv.shape[0]
    D = qkv.shape[1] // (3 * H)
    if packed.total != T:
        raise ValueError(f"alibi_attention_varlen: qkv has {T} rows, the index {packed.total}")
    _check_varlen_index(T, packed.cu_seqlens, packed.positions, packed.batch)
    sq_sum = getattr(packed, "sq_sum", None)
    if sq_sum is None:
        sq_sum = packed.batch * packed.max_seqlen ** 2
    return AlibiAttentionVarlen.apply(qkv, packed.cu_seqlens, packed.positions, slopes,
                                      packed.batch, packed.max_seqlen, sq_sum, H,
                                      scale if scale is not None else 1.0 / math.sqrt(D))


# ----------------------------------------------------------------------------------- GeGLU
def _geglu_forward(g, p, seed, off):
    """(a, fac): the GeGLU output and the backward factors fac = [d a / d g1 | d a / d g2]
    (dropout folded in; csrc/common.h geglu_fwd_fac), so the backward is dg = da * fac. From
    the gated_layers epilogue, which wrote fac in g's place (Linear, geglu=...), or the separate
    pass (dna_geglu_fwd; fac in a new buffer, g is left as it is)."""
    pre = getattr(g, "_dna_geglu", None)
    if pre is not None and pre[1] == (p, seed, off):
        a = pre[0]  # computed in the producing GEMM's epilogue (Linear, geglu=...)
        del g._dna_geglu
        return a, g
    g = g.contiguous()
    n, F2 = g.shape
    a = torch.empty(n, F2 // 2, device=g.device, dtype=g.dtype)
    fac = torch.empty_like(g)
    with _timed("geglu_fwd", n * F2 // 2 * 5 * g.element_size(), "byte"):
        N.call("dna_geglu_fwd", g.data_ptr(), _dt(g), n, F2 // 2, p, seed, off, a.data_ptr(),
               fac.data_ptr(), N.stream_ptr())
    return a, fac


class GeGLU(torch.autograd.Function):
    """dropout(gelu(g[:, :F]) * g[:, F:])   (bert_layers.py:292-296)."""

    @staticmethod
    def forward(ctx, g, p, seed, off):
        _gpu(g)
        a, fac = _geglu_forward(g, p, seed, off)
        ctx.save_for_backward(fac)
        return a

    @staticmethod
    def backward(ctx, da):
        (fac,) = ctx.saved_tensors
        n, F2 = fac.shape
        dg = torch.empty_like(fac)
        da = da.contiguous()
        with _timed("geglu_bwd", n * F2 // 2 * 5 * fac.element_size(), "byte"):
            N.call("dna_geglu_bwd", da.data_ptr(), fac.data_ptr(), _dt(fac), n, F2 // 2,
                   dg.data_ptr(), N.stream_ptr())
        return dg, None, None, None


# ----------------------------------------------------------------------------------- loss
class MaskedCrossEntropy(torch.autograd.Function):
    """sum_r CE(logits[r], target[r]) / denom  (fp32 math on bf16 or fp32 logits)."""

    @staticmethod
    def forward(ctx, logits, target, denom):
        _gpu(logits, target)
        logits = logits.contiguous()
        M, V = logits.shape
        loss = torch.empty(M, device=logits.device, dtype=torch.float32)
        lse = torch.empty_like(loss)
        target = target.contiguous()
        N.call("dna_xent_fwd", logits.data_ptr(), _dt(logits), target.data_ptr(), M, V,
               loss.data_ptr(), lse.data_ptr(), N.stream_ptr())
        ctx.save_for_backward(logits, target, lse)
        ctx.denom = float(denom)
        return loss.sum() / ctx.denom

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse = ctx.saved_tensors
        M, V = logits.shape
        dl = torch.empty_like(logits)
        dloss = dloss.detach().to(torch.float32).contiguous().reshape(1)
        N.call("dna_xent_bwd", logits.data_ptr(), _dt(logits), target.data_ptr(), lse.data_ptr(),
               dloss.data_ptr(), 1.0 / ctx.denom, M, V, dl.data_ptr(), N.stream_ptr())
        return dl, None, None


LM_HEAD_MAX_VOCAB = 64  # csrc/lm_head.hip: a lane per vocabulary entry


class MaskedLMHead(torch.autograd.Function):
    """Tied LM head + masked cross entropy on csrc/lm_head.hip, for vocabularies of at most 64
    entries (the HyenaDNA character tokenizer), without a logits tensor:

        logits = h w^T (fp32);  loss = sum_{r: labels[r] >= 0} CE(logits[r], labels[r]) / count
        -> (loss scalar fp32, count scalar int64: the kept rows, on the device)

    h [T, D] fp32 or bf16; a view with unit column stride and a row stride >= D is read in place;
    rows with a negative label are never read. w [V, D]: the fp32 master parameter; under a
    bf16 h its bf16 shadow (`_dna_lp`, kept by the trainer) is what the kernels read. labels [T]
    int64 (a label >= V is treated as ignored by the kernel and never indexes w; callers
    validate labels where they are built, on the host). denom > 0 replaces count as the divisor.
    count == 0 gives loss 0 and zero gradients (the reference's mean over an empty selection is
    NaN). The upstream gradient stays on the device. dh comes back in h's dtype, every element
    written by the kernel; dw is added straight into the flat gradient with FlatParams direct
    gradients (the tied embedding adds its own share there too), else returned.

    cm [V] int64 on the device (Caduceus' RCPSLMHead.complement_map, its entries validated on the
    host where the module builds it): the RC-equivariant head. h is then [T, 2 D] and
    logits = h[:, :D] w^T + flip(h[:, D:]) w[cm]^T; dw folds the gathered rows' gradient back in a
    fixed order (dna_lm_head_rc_*).

    bias [V] fp32 (with cm None only): an untied, biased head (the CNN's out_linear),
    logits = h w^T + bias on dna_lm_head_bias_*; its gradient goes where dw goes."""

    @staticmethod
    def forward(ctx, h, w, labels, denom, cm=None, bias=None):
        _gpu(h, w, labels)
        ctx.set_materialize_grads(False)
        if bias is not None and cm is not None:
            raise ValueError("dna_amd: the RC-equivariant lm head (complement_map) takes no bias")
        if h.dim() != 2 or h.numel() == 0:
            raise ValueError(f"dna_amd: lm head input must be a non-empty [T, D], got {tuple(h.shape)}")
        T, Dh = h.shape
        D = Dh if cm is None else Dh // 2
        if cm is not None and (Dh % 2 or w.dim() != 2 or w.shape[1] != D):
            raise ValueError(f"dna_amd: RC lm head input must have 2 * D columns for a weight "
                             f"[V, D], got h {tuple(h.shape)}, weight {tuple(w.shape)}")
        if h.stride(1) != 1 or (T > 1 and h.stride(0) < Dh):
            h = h.contiguous()
        hs = h.stride(0) if T > 1 else Dh
        V = w.shape[0]
        if w.dtype != torch.float32 or not w.is_contiguous() or tuple(w.shape) != (V, D):
            raise TypeError(f"dna_amd: lm head weight must be contiguous fp32 [V, {D}], got "
                            f"{w.dtype} {tuple(w.shape)}")
        if not 1 <= V <= LM_HEAD_MAX_VOCAB:
            raise ValueError(f"dna_amd: lm head takes 1 <= V <= {LM_HEAD_MAX_VOCAB}, got {V}")
        if labels.dtype != torch.int64 or labels.numel() != T:
            raise TypeError(f"dna_amd: lm head labels must be int64 [{T}], got {labels.dtype} "
                            f"{tuple(labels.shape)}")
        if bias is not None:
            _gpu(bias)
            if bias.dtype != torch.float32 or not bias.is_contiguous() or tuple(bias.shape) != (V,):
                raise TypeError(f"dna_amd: lm head bias must be contiguous fp32 [{V}], got "
                                f"{bias.dtype} {tuple(bias.shape)}")
        if cm is not None:
            _gpu(cm)
            if cm.dtype != torch.int64 or cm.numel() != V:
                raise TypeError(f"dna_amd: lm head complement map must be int64 [{V}], got "
                                f"{cm.dtype} {tuple(cm.shape)}")
            cm = cm.reshape(-1).contiguous()
        labels = labels.reshape(-1).contiguous()
        lp = getattr(w, "_dna_lp", None)
        wk = lp if (h.dtype == torch.bfloat16 and lp is not None) else w
        dev = h.device
        need_bwd = (ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or
                    (bias is not None and ctx.needs_input_grad[5]))
        out = torch.empty(2, device=dev, dtype=torch.float32)  # loss_sum, loss
        count = torch.empty((), device=dev, dtype=torch.int64)
        coef = torch.empty(T, V, device=dev, dtype=torch.float32) if need_bwd else None
        dn = 0.0 if denom is None else float(denom)
        if bias is not None:
            nws = N.lib().dna_lm_head_fwd_workspace(T)
            ws = torch.empty(max(nws // 8, 2), device=dev, dtype=torch.float64)
            with _timed("lm_head_bias_fwd", float(T) * D * h.element_size(), kind="byte"):
                N.call("dna_lm_head_bias_fwd", h.data_ptr(), hs, _dt(h), wk.data_ptr(), _dt(wk),
                       bias.data_ptr(), labels.data_ptr(), T, D, V, dn, out.data_ptr(),
                       count.data_ptr(), out[1:].data_ptr(), _p(coef), ws.data_ptr(),
                       ws.numel() * 8, N.stream_ptr())
        elif cm is None:
            nws = N.lib().dna_lm_head_fwd_workspace(T)
            ws = torch.empty(max(nws // 8, 2), device=dev, dtype=torch.float64)
            with _timed("lm_head_fwd", float(T) * D * h.element_size(), kind="byte"):
                N.call("dna_lm_head_fwd", h.data_ptr(), hs, _dt(h), wk.data_ptr(), _dt(wk),
                       labels.data_ptr(), T, D, V, dn, out.data_ptr(), count.data_ptr(),
                       out[1:].data_ptr(), _p(coef), ws.data_ptr(), ws.numel() * 8, N.stream_ptr())
        else:
            nws = N.lib().dna_lm_head_rc_fwd_workspace(T, D, V)
            ws = torch.empty(nws // 8 + 2, device=dev, dtype=torch.float64)
            with _timed("lm_head_rc_fwd", float(T) * Dh * h.element_size(), kind="byte"):
                N.call("dna_lm_head_rc_fwd", h.data_ptr(), hs, _dt(h), wk.data_ptr(), _dt(wk),
                       cm.data_ptr(), labels.data_ptr(), T, D, V, dn, out.data_ptr(),
                       count.data_ptr(), out[1:].data_ptr(), _p(coef), ws.data_ptr(),
                       ws.numel() * 8, N.stream_ptr())
        ctx.save_for_backward(h, wk, labels, count, coef, cm)
        ctx.param = w
        ctx.bias = bias
        ctx.cfg = (hs, dn)
        ctx.mark_non_differentiable(count)
        return out[1], count

    @staticmethod
    def backward(ctx, dloss, dcount):
        h, wk, labels, count, coef, cm = ctx.saved_tensors
        if dloss is None or coef is None:
            return None, None, None, None, None, None
        hs, dn = ctx.cfg
        T, Dh = h.shape
        V, D = wk.shape
        dev = h.device
        up = dloss.detach().to(torch.float32).reshape(1).contiguous()
        w, b = ctx.param, ctx.bias
        direct = _param_grads_direct((w, b))
        dw = db = None
        if direct:
            dw, db = w.grad, None if b is None else b.grad
        elif ctx.needs_input_grad[1] or (b is not None and ctx.needs_input_grad[5]):
            dw = torch.empty(V, D, device=dev, dtype=torch.float32)
            db = None if b is None else torch.empty(V, device=dev, dtype=torch.float32)
        dh = torch.empty(T, Dh, device=dev, dtype=h.dtype) if ctx.needs_input_grad[0] else None
        if b is not None:
            nws = N.lib().dna_lm_head_bias_bwd_workspace(T, D, V) if dw is not None else 0
            ws = torch.empty(max(nws // 4, 4), device=dev, dtype=torch.float32)
            with _timed("lm_head_bias_bwd", float(T) * D * h.element_size(), kind="byte"):
                N.call("dna_lm_head_bias_bwd", coef.data_ptr(), h.data_ptr(), hs, _dt(h),
                       wk.data_ptr(), _dt(wk), labels.data_ptr(), count.data_ptr(), up.data_ptr(),
                       dn, T, D, V, _p(dh), D, _p(dw), _p(db), int(direct), ws.data_ptr(),
                       ws.numel() * 4, N.stream_ptr())
        elif cm is None:
            nws = N.lib().dna_lm_head_bwd_workspace(T, D, V) if dw is not None else 0
            ws = torch.empty(max(nws // 4, 4), device=dev, dtype=torch.float32)
            with _timed("lm_head_bwd", float(T) * D * h.element_size(), kind="byte"):
                N.call("dna_lm_head_bwd", coef.data_ptr(), h.data_ptr(), hs, _dt(h), wk.data_ptr(),
                       _dt(wk), labels.data_ptr(), count.data_ptr(), up.data_ptr(), dn, T, D, V,
                       _p(dh), D, _p(dw), int(direct), ws.data_ptr(), ws.numel() * 4,
                       N.stream_ptr())
        else:
            nws = N.lib().dna_lm_head_rc_bwd_workspace(T, D, V)
            ws = torch.empty(nws // 4 + 4, device=dev, dtype=torch.float32)
            with _timed("lm_head_rc_bwd", float(T) * Dh * h.element_size(), kind="byte"):
                N.call("dna_lm_head_rc_bwd", coef.data_ptr(), h.data_ptr(), hs, _dt(h),
                       wk.data_ptr(), _dt(wk), cm.data_ptr(), labels.data_ptr(), count.data_ptr(),
                       up.data_ptr(), dn, T, D, V, _p(dh), Dh, _p(dw), int(direct), ws.data_ptr(),
                       ws.numel() * 4, N.stream_ptr())
        if direct:
            _notify_direct(w, b)
            return dh, None, None, None, None, None
        return dh, dw, None, None, None, db


def masked_lm_head(h, weight, labels, denom=None, complement_map=None, bias=None):
    """MaskedLMHead outside autocast (the kernels take h in its own dtype, so the result is the
    same with and without it). h [..., D], labels [...] -> (loss, count). complement_map [V]
    (int64, on the device): the RC-equivariant head; h then has 2 * D columns. bias [V] fp32: the
    biased head (complement_map None only)."""
    if bias is not None and complement_map is not None:
        raise ValueError("dna_amd: the RC-equivariant lm head (complement_map) takes no bias")
    with torch.autocast("cuda", enabled=False):
        return MaskedLMHead.apply(h.reshape(-1, h.shape[-1]), weight, labels.reshape(-1), denom,
                                  complement_map, bias)


# ----------------------------------------------------------------------------------- cls head
CLS_PROBLEMS = {"regression": N.CLS_REGRESSION, "single_label_classification": N.CLS_SINGLE_LABEL,
                "multi_label_classification": N.CLS_MULTI_LABEL}


def _cls_rows(x):
    """x as B rows of H with unit column stride (a strided row view is read in place)."""
    if x.dim() != 2:
        raise ValueError(f"dna_amd: cls head input must be [B, H], got {tuple(x.shape)}")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else x.shape[1])


def _cls_labels(labels, problem, B, C):
    if problem == N.CLS_SINGLE_LABEL:
        labels = labels.reshape(-1).to(torch.int64).contiguous()
        if labels.numel() != B:
            raise ValueError(f"dna_amd: {labels.numel()} labels for a batch of {B}")
        return labels
    labels = labels.to(torch.float32).reshape(-1).contiguous()
    if labels.numel() != B * C:
        raise ValueError(f"dna_amd: {labels.numel()} label values for logits [{B}, {C}]")
    return labels


def _f32_param(name, t, shape):
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise TypeError(f"dna_amd: cls head {name} must be contiguous fp32 {tuple(shape)}, got "
                        f"{t.dtype} {tuple(t.shape)}")


def _loss_outputs(labels, problem, logits):
    """What the loss of a classification head reads and writes -> (labels as the kernel takes
    them, loss [1], dlogits [B, C], pred [B] int64 | None: single-label only); all None without
    labels."""
    if labels is None:
        return None, None, None, None
    B, C = logits.shape
    labels = _cls_labels(labels, problem, B, C)
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    dl = torch.empty_like(logits)
    pred = None
    if problem == N.CLS_SINGLE_LABEL:
        pred = torch.empty(B, device=logits.device, dtype=torch.int64)
    return labels, loss, dl, pred


def _logits_grad(dl, dlogits, dloss):
    """What a classification head's backward starts from: dl, the dlogits its loss kernel stored
    in the forward (None without labels), the incoming gradient of the logits and that of the
    loss -> (g [B, C] fp32, up): the backward kernels take g * up[0], up None meaning 1, so the
    loss's scalar gradient stays on the device. None: no gradient came in."""
    if dl is not None and dloss is not None:
        if dlogits is None:  # the usual case: only the loss was used
            return dl, dloss.detach().to(torch.float32).reshape(1).contiguous()
        return (dl * dloss + dlogits).contiguous(), None
    if dlogits is not None:
        return dlogits.to(torch.float32).contiguous(), None
    return None


class ClsHead(torch.autograd.Function):
    """BertPooler + dropout + classifier (+ loss) of BertForSequenceClassification (reference
    bert_layers.py:495-510, :969-998) on csrc/cls_head.hip:

        t = tanh(x Wp^T + bp);  a = dropout(t; p, seed, off);  logits = a Wc^T + bc
        -> (logits [B, C] fp32, loss scalar | None, pred [B] int64 | None)

    x [B, H] fp32 or bf16, rows may be strided (the [CLS] rows of a [b*S, H] activation read in
    place); the weights are the fp32 master parameters in both precisions. labels None: logits
    only. Forward 2 launches (the loss rides in the second), backward 2; with FlatParams direct
    gradients the four parameter gradients are added straight into the flat buffer."""

    @staticmethod
    def forward(ctx, x, wp, bp, wc, bc, p, seed, off, labels, problem):
        _gpu(x, wp, bp, wc, bc, labels)
        ctx.set_materialize_grads(False)
        x, stride = _cls_rows(x)
        B, H = x.shape
        C = wc.shape[0]
        _f32_param("pooler weight", wp, (H, H))
        _f32_param("pooler bias", bp, (H,))
        _f32_param("classifier weight", wc, (C, H))
        _f32_param("classifier bias", bc, (C,))
        dev = x.device
        t = torch.empty(B, H, device=dev, dtype=torch.float32)
        a = torch.empty_like(t)
        logits = torch.empty(B, C, device=dev, dtype=torch.float32)
        labels, loss, dl, pred = _loss_outputs(labels, problem, logits)
        nws = N.lib().dna_cls_head_fwd_workspace(B, H, C)
        ws = torch.empty(max(nws // 4, 4), device=dev, dtype=torch.float32)
        with _timed("cls_head_fwd", 2.0 * B * H * (H + C)):
            N.call("dna_cls_head_fwd", x.data_ptr(), _dt(x), stride, wp.data_ptr(), bp.data_ptr(),
                   wc.data_ptr(), bc.data_ptr(), B, H, C, float(p), seed, off, t.data_ptr(),
                   a.data_ptr(), logits.data_ptr(), _p(labels), problem, _p(loss), _p(dl), _p(pred),
                   ws.data_ptr(), ws.numel() * 4, N.stream_ptr())
        ctx.save_for_backward(x, wp, wc, t, a, dl)
        ctx.params = (wp, bp, wc, bc)
        ctx.cfg = (stride, float(p), seed, off)
        if pred is not None:
            ctx.mark_non_differentiable(pred)
        return logits, (None if loss is None else loss.reshape(())), pred

    @staticmethod
    def backward(ctx, dlogits, dloss, dpred):
        x, wp, wc, t, a, dl = ctx.saved_tensors
        stride, p, seed, off = ctx.cfg
        g_up = _logits_grad(dl, dlogits, dloss)
        if g_up is None:
            return (None,) * 10
        g, up = g_up
        B, H = x.shape
        C = wc.shape[0]
        dev = x.device
        pwp, pbp, pwc, pbc = ctx.params
        direct = _param_grads_direct(ctx.params)
        if direct:
            dwp, dbp, dwc, dbc = pwp.grad, pbp.grad, pwc.grad, pbc.grad
        else:
            dwp, dbp = torch.empty_like(wp), torch.empty(H, device=dev, dtype=torch.float32)
            dwc, dbc = torch.empty_like(wc), torch.empty(C, device=dev, dtype=torch.float32)
        dx = torch.empty(B, H, device=dev, dtype=torch.float32)
        nws = N.lib().dna_cls_head_bwd_workspace(B, H, C)
        ws = torch.empty(max(nws // 4, 4), device=dev, dtype=torch.float32)
        with _timed("cls_head_bwd", 4.0 * B * H * (H + C)):
            N.call("dna_cls_head_bwd", g.data_ptr(), _p(up), x.data_ptr(), _dt(x), stride,
                   t.data_ptr(), a.data_ptr(), wp.data_ptr(), wc.data_ptr(), B, H, C, p, seed, off,
                   dwc.data_ptr(), dbc.data_ptr(), dwp.data_ptr(), dbp.data_ptr(), dx.data_ptr(),
                   int(direct), ws.data_ptr(), ws.numel() * 4, N.stream_ptr())
        dx = dx if x.dtype == torch.float32 else dx.to(x.dtype)
        if direct:
            _notify_direct(*ctx.params)
            return (dx,) + (None,) * 9
        return dx, dwp, dbp, dwc, dbc, None, None, None, None, None


_POOLER_WARNED = False


def pooler(x, wp, bp):
    """tanh(x wp^T + bp) [B, H] fp32 (BertPooler, reference bert_layers.py:495-510) from the head
    kernel's first stage, for embedding extraction. The result carries no autograd graph
    (training goes through ClsHead, which has the backward); where one would have been recorded
    -- grad mode on and an input that requires grad -- a warning says so, once."""
    if torch.is_grad_enabled() and (x.requires_grad or wp.requires_grad or bp.requires_grad):
        global _POOLER_WARNED
        if not _POOLER_WARNED:
            _POOLER_WARNED = True
            warnings.warn("dna_amd: BertModel's pooled_output is computed without an autograd "
                          "graph (embedding extraction); train the pooler through "
                          "BertForSequenceClassification", stacklevel=2)
    _gpu(x, wp, bp)
    x, stride = _cls_rows(x)
    B, H = x.shape
    _f32_param("pooler weight", wp, (H, H))
    _f32_param("pooler bias", bp, (H,))
    t = torch.empty(B, H, device=x.device, dtype=torch.float32)
    a = torch.empty_like(t)
    wc = torch.zeros(1, H, device=x.device, dtype=torch.float32)  # a one-label classifier of zeros
    logits = torch.empty(B, 1, device=x.device, dtype=torch.float32)
    nws = N.lib().dna_cls_head_fwd_workspace(B, H, 1)
    ws = torch.empty(max(nws // 4, 4), device=x.device, dtype=torch.float32)
    N.call("dna_cls_head_fwd", x.data_ptr(), _dt(x), stride, wp.data_ptr(), bp.data_ptr(),
           wc.data_ptr(), wc.data_ptr(), B, H, 1, 0.0, 0, 0, t.data_ptr(), a.data_ptr(),
           logits.data_ptr(), None, 0, None, None, None, ws.data_ptr(), ws.numel() * 4,
           N.stream_ptr())
    return t


def cls_head(x, wp, bp, wc, bc, p=0.0, rng=None, labels=None, problem_type=None):
    """ClsHead with the dropout draw: rng.take(B * H) only when p > 0. problem_type: a
    CLS_PROBLEMS name (needed with labels). -> (logits, loss | None, pred | None)."""
    seed, off = rng.take(x.shape[0] * x.shape[1]) if p > 0 else (0, 0)
    problem = CLS_PROBLEMS[problem_type] if labels is not None else N.CLS_SINGLE_LABEL
    return ClsHead.apply(x, wp, bp, wc, bc, float(p), seed, off, labels, problem)


# ----------------------------------------------------------------------------------- pool head
def _pool_rows(name, x):
    """x [B, L, W] as the pool-head kernels read it: unit channel stride, one position stride,
    batch stride L * position stride (a strided view such as a channel slice is read in place;
    anything else is copied). -> (x, position stride in elements)"""
    if x.dim() != 3:
        raise ValueError(f"dna_amd: pool head {name} must be [B, L, D], got {tuple(x.shape)}")
    B, L, W = x.shape
    if B == 0 or L == 0 or W == 0:
        raise ValueError(f"dna_amd: pool head {name} is empty: {tuple(x.shape)}")
    s = x.stride(1) if L > 1 else (x.stride(0) if B > 1 else W)
    if x.stride(2) != 1 or s < W or (B > 1 and L > 1 and x.stride(0) != L * s):
        x = x.contiguous()
        s = W
    return x, s


def _pool_window(name, t, B):
    if t is None:
        return None
    if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != B:
        raise TypeError(f"dna_amd: pool head {name} must be int32 [{B}], got {t.dtype} "
                        f"{tuple(t.shape)}")
    _gpu(t)
    return t.contiguous()


# The head's kernels by label count: up to POOL_NARROW_LABELS the narrow ones (any problem type),
# up to POOL_WIDE_LABELS the wide ones (regression, multi-label); C alone decides.
POOL_NARROW_LABELS, POOL_WIDE_LABELS = 64, 1024


class PoolHead(torch.autograd.Function):
    """Windowed mean over L + linear (+ loss) on csrc/pool_head.hip, the head of the HyenaDNA
    SequenceDecoder (pool / first / last) and of CaduceusForSequenceClassification:

        pooled = mean_{l in [start, start + count)} x[:, l]       (+ the same over x2, halved)
        logits = pooled w^T (+ bias)
        -> (logits [B, C] fp32, loss scalar | None, pred [B] int64 | None)

    x [B, L, D] fp32 or bf16; a view with unit channel stride is read in place. rcps: x is
    [B, L, 2D] and its halves are the two inputs, the second with its channels reversed (one
    [B, L, 2D] gradient comes back). x2: a second [B, L, D] input (flip2: channels reversed).
    mirror2: the second input's window is [L - start - count, L - start), the same positions of
    its sequence flip. start / count: int32 [B] on the device or None (0 / L - start). w [C, D], bias [C] | None: the
    fp32 master parameters in both precisions. Forward 2 launches + the loss's, backward 2; with
    FlatParams direct gradients dw / dbias are added straight into the flat buffer. C > 64 (to
    1024; regression and multi-label only) runs the wide kernels: forward 3 launches + 2 for the
    loss, backward 2; a larger C is a ValueError."""

    @staticmethod
    def forward(ctx, x, x2, w, bias, start, count, rcps, flip2, mirror2, labels, problem):
        _gpu(x, x2, w, bias, start, count, labels)
        ctx.set_materialize_grads(False)
        if rcps and x2 is not None:
            raise ValueError("dna_amd: pool head takes rcps or x2, not both")
        x, s1 = _pool_rows("x", x)
        B, L, W = x.shape
        s2 = 0
        if rcps:
            if W % 2:
                raise ValueError(f"dna_amd: rcps pool head needs an even width, got {W}")
            D, flip2 = W // 2, True
            xa, xb, s2 = x[..., :D], x[..., D:], s1
        elif x2 is not None:
            x2, s2 = _pool_rows("x2", x2)
            if x2.shape != x.shape or x2.dtype != x.dtype:
                raise ValueError(f"dna_amd: pool head x2 {x2.dtype} {tuple(x2.shape)} does not "
                                 f"match x {x.dtype} {tuple(x.shape)}")
            D, xa, xb = W, x, x2
        else:
            D, xa, xb, flip2, mirror2 = W, x, None, False, False
        flags = int(bool(flip2)) | (int(bool(mirror2)) << 1)
        C = w.shape[0]
        if C > POOL_WIDE_LABELS:
            raise ValueError(f"dna_amd: pool head has {C} labels; at most {POOL_WIDE_LABELS} are "
                             "built")
        if C > POOL_NARROW_LABELS and labels is not None and problem == N.CLS_SINGLE_LABEL:
            raise ValueError(f"dna_amd: a single_label_classification pool head takes at most "
                             f"{POOL_NARROW_LABELS} labels, got {C} (regression and "
                             f"multi_label_classification go up to {POOL_WIDE_LABELS})")
        if w.dtype != torch.float32 or not w.is_contiguous() or tuple(w.shape) != (C, D):
            raise TypeError(f"dna_amd: pool head weight must be contiguous fp32 [C, {D}], got "
                            f"{w.dtype} {tuple(w.shape)}")
        if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()
                                 or tuple(bias.shape) != (C,)):
            raise TypeError(f"dna_amd: pool head bias must be contiguous fp32 [{C}], got "
                            f"{bias.dtype} {tuple(bias.shape)}")
        dev = x.device
        start = _pool_window("start", start, B)
        count = _pool_window("count", count, B)
        pooled = torch.empty(B, D, device=dev, dtype=torch.float32)
        logits = torch.empty(B, C, device=dev, dtype=torch.float32)
        labels, loss, dl, pred = _loss_outputs(labels, problem, logits)
        nin = 1 if xb is None else 2
        head = (xa.data_ptr(), s1, _p(xb), s2, flags, _dt(x), _p(start), _p(count), w.data_ptr(),
                _p(bias), B, L, D, C, pooled.data_ptr(), logits.data_ptr(), _p(labels), problem,
                _p(loss), _p(dl))
        with _timed("pool_head_fwd", float(nin) * B * L * D * x.element_size(), kind="byte"):
            if C <= POOL_NARROW_LABELS:
                nws = N.lib().dna_pool_head_fwd_workspace(B, L, D)
                ws = torch.empty(max(nws // 4, 4), device=dev, dtype=torch.float32)
                N.call("dna_pool_head_fwd", *head, _p(pred), ws.data_ptr(), ws.numel() * 4,
                       N.stream_ptr())
            else:
                nws = N.lib().dna_pool_head_wide_fwd_workspace(B, L, D, C)
                ws = torch.empty(max(nws // 4, 4), device=dev, dtype=torch.float32)
                N.call("dna_pool_head_wide_fwd", *head, ws.data_ptr(), ws.numel() * 4,
                       N.stream_ptr())
        ctx.save_for_backward(w, pooled, dl, start, count)
        ctx.params = (w, bias)
        ctx.cfg = (tuple(x.shape), x.dtype, D, bool(rcps), xb is not None, flags)
        if pred is not None:
            ctx.mark_non_differentiable(pred)
        return logits, (None if loss is None else loss.reshape(())), pred

    @staticmethod
    def backward(ctx, dlogits, dloss, dpred):
        w, pooled, dl, start, count = ctx.saved_tensors
        shape, dtype, D, rcps, two, flags = ctx.cfg
        g_up = _logits_grad(dl, dlogits, dloss)
        if g_up is None:
            return (None,) * 11
        g, up = g_up
        B, L, W = shape
        C = w.shape[0]
        dev = w.device
        pw, pb = ctx.params
        direct = _param_grads_direct(ctx.params)
        if direct:
            dw, db = pw.grad, (None if pb is None else pb.grad)
        else:
            dw = torch.empty_like(w)
            db = None if pb is None else torch.empty(C, device=dev, dtype=torch.float32)
        # dx is contiguous whatever x's strides were (autograd takes any layout); a frozen backbone
        # needs none, and then the broadcast pass is not launched
        need_dx = ctx.needs_input_grad[0] or (two and not rcps and ctx.needs_input_grad[1])
        dx = dx2 = da = dbuf = None
        if need_dx:
            dx = torch.empty(B, L, W, device=dev, dtype=dtype)
            if rcps:
                da, dbuf = dx[..., :D], dx[..., D:]
            elif two:
                dx2 = torch.empty(B, L, W, device=dev, dtype=dtype)
                da, dbuf = dx, dx2
            else:
                da = dx
        wide = C > POOL_NARROW_LABELS
        nws = (N.lib().dna_pool_head_wide_bwd_workspace(B, L, D, C) if wide
               else N.lib().dna_pool_head_bwd_workspace(B, L, D))
        ws = torch.empty(max(nws // 4, 4), device=dev, dtype=torch.float32)
        nout = (2 if two else 1) if need_dx else 0
        es = 2 if dtype == torch.bfloat16 else 4
        with _timed("pool_head_bwd", float(nout) * B * L * D * es, kind="byte"):
            N.call("dna_pool_head_wide_bwd" if wide else "dna_pool_head_bwd",
                   g.data_ptr(), _p(up), pooled.data_ptr(), w.data_ptr(),
                   _p(start), _p(count), B, L, D, C, _DT[dtype], _p(da), W, _p(dbuf), W,
                   flags, dw.data_ptr(), _p(db), int(direct), ws.data_ptr(), ws.numel() * 4,
                   N.stream_ptr())
        if direct:
            _notify_direct(*ctx.params)
            return (dx, dx2) + (None,) * 9
        return dx, dx2, dw, db, None, None, None, None, None, None, None


def pool_head(x, w, bias=None, x2=None, rcps=False, flip2=False, mirror2=False, start=None,
              count=None, labels=None, problem_type=None):
    """PoolHead outside autocast (the kernels take x in its own dtype and the fp32 parameters, so
    the result is the same with and without it). problem_type: a CLS_PROBLEMS name (needed with
    labels). -> (logits, loss | None, pred | None)."""
    problem = CLS_PROBLEMS[problem_type] if labels is not None else N.CLS_SINGLE_LABEL
    with torch.autocast("cuda", enabled=False):
        return PoolHead.apply(x, x2, w, bias, start, count, bool(rcps), bool(flip2), bool(mirror2),
                              labels, problem)


# ----------------------------------------------------------------------------------- GEMM
def _gemm_impl():
    """"hip" (default): forward and data-gradient GEMMs on csrc/gemm.hip; "torch": hipBLASLt
    through torch.mm (A/B switch, DNA_GEMM_IMPL)."""
    return os.environ.get("DNA_GEMM_IMPL", "hip")


def _hip_gemm_ok(x, w_lp, n_out, k_red):
    return (x.dtype == torch.bfloat16 and w_lp.dtype == torch.bfloat16 and x.is_cuda
            and k_red % 64 == 0 and n_out % 8 == 0 and _gemm_impl() == "hip")


def _f32_gemm_ok(x, w):
    """fp32 parity mode: exact-fp32 MFMA kernels (csrc/gemm_f32.hip) for every projection."""
    return (x.dtype == torch.float32 and w.dtype == torch.float32 and x.is_cuda
            and _gemm_impl() == "hip")


def _hip_linear_f32(x, w, bias):
    """y[M, N] = x[M, K] . w[N, K]^T (+ b), fp32 in / fp32 out (dna_linear_fwd_f32)."""
    x, w = x.contiguous(), w.contiguous()
    M, K = x.shape
    Nn = w.shape[0]
    y = torch.empty(M, Nn, device=x.device, dtype=torch.float32)
    b = None if bias is None else bias.float().contiguous()
    N.call("dna_linear_fwd_f32", x.data_ptr(), w.data_ptr(), _p(b), M, Nn, K, y.data_ptr(),
           N.stream_ptr())
    return y


def _hip_dgrad_f32(dy, w):
    """dx[M, K] = dy[M, N] . w[N, K], fp32 (dna_linear_dgrad_f32)."""
    dy, w = dy.contiguous(), w.contiguous()
    M, Nn = dy.shape
    K = w.shape[1]
    dx = torch.empty(M, K, device=dy.device, dtype=torch.float32)
    N.call("dna_linear_dgrad_f32", dy.data_ptr(), w.data_ptr(), M, Nn, K, dx.data_ptr(),
           N.stream_ptr())
    return dx


def _hip_wgrad_f32_parts(dy, x):
    """fp32 split-K partials [s, m, n] of dy^T x (dna_linear_wgrad_f32)."""
    dy, x = dy.contiguous(), x.contiguous()
    rows, m = dy.shape
    n = x.shape[1]
    s = N.lib().dna_linear_wgrad_f32_splits(rows, m, n)
    parts = torch.empty(s, m, n, device=dy.device, dtype=torch.float32)
    N.call("dna_linear_wgrad_f32", dy.data_ptr(), x.data_ptr(), rows, m, n, s, parts.data_ptr(),
           N.stream_ptr())
    return parts, s


def _geglu_fused_ok(x, w_lp):
    F2, K = w_lp.shape
    return (os.environ.get("DNA_GEGLU_FUSED", "1") != "0" and _hip_gemm_ok(x, w_lp, F2, K)
            and F2 % 256 == 0 and K >= 128)


def _hip_geglu_linear(x, w_nk, p, seed, off):
    """fac[M, 2F] (the GeGLU backward factors of g = x . w^T, in g's place) and
    a[M, F] = dropout(gelu(g1) g2) in one launch (dna_geglu_linear_fwd)."""
    x = x.contiguous()
    M, K = x.shape
    F2 = w_nk.shape[0]
    fac = torch.empty(M, F2, device=x.device, dtype=torch.bfloat16)
    a = torch.empty(M, F2 // 2, device=x.device, dtype=torch.bfloat16)
    N.call("dna_geglu_linear_fwd", x.data_ptr(), w_nk.data_ptr(), None, M, F2 // 2, K, float(p),
           seed, off, fac.data_ptr(), a.data_ptr(), N.stream_ptr())
    return fac, a


def _gelu_fc1_ok(x, w_lp):
    """dna_linear_gelu_fwd applies (the persistent kernel's lean body: N % 256, N <= 8192,
    K % 128); DNA_GELU_FC1_FUSED=0: torch's separate GELU pass (A/B)."""
    Nn, K = w_lp.shape
    return (os.environ.get("DNA_GELU_FC1_FUSED", "1") != "0" and _hip_gemm_ok(x, w_lp, Nn, K)
            and Nn % 256 == 0 and Nn <= 8192 and K % 128 == 0 and Nn * K * 2 < 2 ** 31)


def _hip_linear_gelu(x, w_nk, bias):
    """h = x . w_nk^T (+ fp32 bias) and act = bf16(gelu_tanh(h)) from one launch
    (dna_linear_gelu_fwd)."""
    x = x.contiguous()
    M, K = x.shape
    Nn = w_nk.shape[0]
    h = torch.empty(M, Nn, device=x.device, dtype=torch.bfloat16)
    act = torch.empty_like(h)
    N.call("dna_linear_gelu_fwd", x.data_ptr(), w_nk.data_ptr(), _p(bias), M, Nn, K, h.data_ptr(),
           act.data_ptr(), N.stream_ptr())
    return h, act


def _hip_linear(x, w_nk, bias):
    """y[M, N] = x[M, K] . w_nk[N, K]^T (+ fp32 bias): the persistent MFMA GEMM (dna_linear_fwd)."""
    x = x.contiguous()
    M, K = x.shape
    Nn = w_nk.shape[0]
    y = torch.empty(M, Nn, device=x.device, dtype=torch.bfloat16)
    N.call("dna_linear_fwd", x.data_ptr(), w_nk.data_ptr(), _p(bias), M, Nn, K, y.data_ptr(),
           N.stream_ptr())
    return y


def bias_grad(dy, bias=None):
    """fp32 sum over rows of dy [rows, cols] (a Linear's bias gradient): bf16 CUDA gradients
    with cols % 64 == 0 on the native two-stage column sum (dna_colsum_bf16, deterministic);
    everything else torch's sum."""
    rows, cols = dy.shape
    if (dy.dtype == torch.bfloat16 and dy.is_cuda and cols % 64 == 0 and rows >= 1
            and dy.is_contiguous() and dy.data_ptr() % 16 == 0):
        # bias: the parameter; under FlatParams direct gradients the column sum is added straight
        # into its fp32 .grad view (the kernel's accumulate mode) and None is returned -- no
        # AccumulateGrad add launch per bias and step (DNA_BIAS_GRAD_DIRECT=0: returned, A/B)
        direct = (bias is not None and os.environ.get("DNA_BIAS_GRAD_DIRECT", "1") != "0"
                  and _param_grads_direct((bias,)) and bias.grad.numel() == cols)
        out = bias.grad if direct else torch.empty(cols, device=dy.device, dtype=torch.float32)
        nws = N.lib().dna_colsum_bf16_workspace(rows, cols)
        ws = torch.empty(nws, device=dy.device, dtype=torch.uint8)
        with _timed("colsum", rows * cols * 2, "byte"):
            N.call("dna_colsum_bf16", dy.data_ptr(), rows, cols, out.data_ptr(), int(direct),
                   ws.data_ptr(), nws, N.stream_ptr())
        if direct:
            _notify_direct(bias)
            return None
        return out
    return dy.sum(0, dtype=torch.float32)


class GeluLinear(torch.autograd.Function):
    """o = gelu_tanh(h) . w^T + b as one autograd node (the flash_attn Mlp's act + fc2 in the
    HyenaDNA Blocks, activation F.gelu(approximate="tanh")): forward = torch's GELU kernel then the
    persistent GEMM; backward = fc2's data gradient with the GELU backward in its epilogue
    (dna_gelu_linear_dgrad_p: dh = bf16(dy . w) * gelu'(h), the intermediate da never stored),
    weight gradient from a = gelu(h), bias gradient by the native column sum."""

    @staticmethod
    def forward(ctx, h, w, b, w_lp, w_lpt, act=None):
        _gpu(h)
        h = h.contiguous()
        # act: gelu(h) from fc1's GEMM epilogue (dna_linear_gelu_fwd), else torch's GELU pass
        a = act if act is not None else F.gelu(h, approximate="tanh")
        flops = 2.0 * h.shape[0] * w_lp.shape[0] * w_lp.shape[1]
        with _timed("gemm_hip", flops):
            o = _hip_linear(a, w_lp, None if b is None else b.float())
        ctx.save_for_backward(h, a, w_lpt)
        ctx.weight = w
        ctx.bias = b
        ctx.has_b = b is not None
        return o

    @staticmethod
    def backward(ctx, do):
        h, a, w_lpt = ctx.saved_tensors
        do = do.contiguous()
        M, F_ = h.shape
        Nn = do.shape[1]
        flops = 2.0 * M * Nn * F_
        dh = torch.empty_like(h)
        with _timed("gemm_gelu_bwd", flops):
            N.call("dna_gelu_linear_dgrad_p", do.data_ptr(), w_lpt.data_ptr(), h.data_ptr(), M, F_,
                   Nn, dh.data_ptr(), N.stream_ptr())
        dw = _weight_grad(ctx.weight, do, a, flops)
        db = bias_grad(do, ctx.bias) if ctx.has_b else None
        return dh, dw, db, None, None, None


def gelu_linear_ok(h, w):
    """GeluLinear applies: bf16 CUDA activations, the persistent kernel's shapes (fc2's output
    and input widths % 256: the forward is then the same GEMM hip_linear runs), the hand-written
    GEMM path enabled."""
    Nn, F_ = w.shape
    return (h.is_cuda and h.dtype == torch.bfloat16 and Nn % 256 == 0
            and F_ % 256 == 0 and _gemm_impl() == "hip"
            and os.environ.get("DNA_GELU_BWD_FUSED", "1") != "0")


def gelu_linear(h, w, b, act=None):
    """F.linear(F.gelu(h, approximate="tanh"), w, b) under bf16 autocast (GeluLinear); act:
    gelu(h) already computed by fc1's epilogue (hyena.hip_linear(..., gelu=True))."""
    lead, F_ = h.shape[:-1], h.shape[-1]
    w_lp = w.to(torch.bfloat16)
    y = GeluLinear.apply(h.reshape(-1, F_), w, b, w_lp, w_lp.t().contiguous(),
                         None if act is None else act.reshape(-1, F_))
    return y.view(*lead, w.shape[0])


class Linear(torch.autograd.Function):
    """y = x @ w_lp^T (+ b): forward and dgrad on the compute dtype copy `w_lp` of the fp32
    master weight `w` -- bf16: the hand-written MFMA kernel (csrc/gemm.hip), the data gradient
    on the transposed copy `w_lpt` (dx = dy . w = dy . (w^T)^T, both operands K-major); the
    weight gradient in fp32 from the token-major MFMA kernel (dna_linear_wgrad_p chunk partials
    folded into the flat gradient by dna_sum_slices_accum)."""

    @staticmethod
    def forward(ctx, x, w, w_lp, b, w_lpt, geglu=None, gelu=False):
        ctx.save_for_backward(x, w_lp, w_lpt)
        ctx.weight = w
        ctx.bias = b
        ctx.has_b = b is not None
        flops = 2.0 * x.shape[0] * w_lp.shape[0] * w_lp.shape[1]
        if geglu is not None and b is None and _geglu_fused_ok(x, w_lp):
            # g = x . w^T and a = dropout(gelu(g1) g2) in one launch (the GeGLU epilogue of the
            # persistent GEMM). The tensor returned in g's place holds the GeGLU backward factors
            # (g itself is never stored); `a` rides on it for the GeGLU node that follows, which
            # must be its only consumer (bit-identical to the separate dna_geglu_fwd pass, which
            # then does not run)
            with _timed("gemm_geglu", flops):
                g, a = _hip_geglu_linear(x, w_lp, *geglu)
            g._dna_geglu = (a, tuple(geglu))
            return g
        if gelu and _gelu_fc1_ok(x, w_lp):
            # h and gelu_tanh(h) from one launch; gelu(h) rides on h for the GeluLinear node
            # that follows (it carries the GELU backward: this node's gradient stays dh)
            with _timed("gemm_gelu", flops):
                h, act = _hip_linear_gelu(x, w_lp, b if (b is None or b.dtype == torch.float32) else b.float())
            h._dna_gelu = act
            return h
        if _hip_gemm_ok(x, w_lp, w_lp.shape[0], w_lp.shape[1]):
            with _timed("gemm_hip", flops):
                return _hip_linear(x, w_lp, b if (b is None or b.dtype == torch.float32) else b.float())
        if _f32_gemm_ok(x, w_lp):
            with _timed("gemm_f32", flops):
                return _hip_linear_f32(x, w_lp, b)
        library_fallback("linear forward", x.shape, w_lp.shape)
        with _timed("gemm", flops):
            if b is not None:
                return torch.addmm(b.to(x.dtype), x, w_lp.t())
            return torch.mm(x, w_lp.t())

    @staticmethod
    def backward(ctx, dy):
        x, w_lp, w_lpt = ctx.saved_tensors
        colsum = getattr(dy, "_dna_colsum", None)
        dy = dy.contiguous()
        if colsum is not None:
            dy._dna_colsum = colsum
        flops = 2.0 * x.shape[0] * w_lp.shape[0] * w_lp.shape[1]
        dx = None
        if ctx.needs_input_grad[0]:
            if w_lpt is not None and _hip_gemm_ok(dy, w_lpt, w_lpt.shape[0], w_lpt.shape[1]):
                with _timed("gemm_hip", flops):
                    dx = _hip_linear(dy, w_lpt, None)
            elif _f32_gemm_ok(dy, w_lp):
                with _timed("gemm_f32", flops):
                    dx = _hip_dgrad_f32(dy, w_lp)
            else:
                library_fallback("linear data gradient", dy.shape, w_lp.shape)
                with _timed("gemm", flops):
                    dx = torch.mm(dy, w_lp)
        dw = _weight_grad(ctx.weight, dy, x, flops)
        db = None
        if ctx.has_b:
            db = getattr(dy, "_dna_colsum", None)  # fused upstream (AlibiAttention.backward)
            if db is None:
                db = bias_grad(dy, ctx.bias)
        return dx, dw, None, db, None, None, None


# ------------------------------------------------------------------ weight-gradient side stream
# The weight gradient of a projection is off the backward's critical path: with a side stream
# (DNA_WGRAD_STREAM=1) it runs beside the next memory-bound kernels of the backward (GeGLU /
# LayerNorm backward). Measured at the bench shape (interleaved A/B): +1.0-1.2 % step throughput
# -- the GEMM blocks hold the CUs and the LayerNorm backward beside them stretches 0.30 -> 1.08 ms
# per launch -- so it is off by default (the per-kernel timings then stay clean).
_SIDE = {}


def _side_stream():
    if os.environ.get("DNA_WGRAD_STREAM", "0") != "1":
        return None
    dev = torch.cuda.current_device()
    st = _SIDE.get(dev)
    if st is None:
        st = _SIDE[dev] = torch.cuda.Stream(device=dev)
    return st


_JOIN_QUEUED = [False]
_KEEP = []  # dy / x of side-stream wgrads, released once the current stream has joined


def join_side_stream():
    """Make the current stream wait for every weight gradient queued on the side stream. Queued
    automatically at the end of every backward that used it (autograd engine callback), so
    whatever reads the gradients after backward() -- all-reduce, clipping, optimizer, tests --
    sees them complete; the gradient-bucket reducer also calls it before each collective."""
    _JOIN_QUEUED[0] = False
    st = _SIDE.get(torch.cuda.current_device()) if torch.cuda.is_available() else None
    if st is not None:
        torch.cuda.current_stream().wait_stream(st)
    # safe to release now: later users of these blocks run on the current stream, behind the join
    _KEEP.clear()


def _queue_join():
    if not _JOIN_QUEUED[0]:
        _JOIN_QUEUED[0] = True
        torch.autograd.Variable._execution_engine.queue_callback(join_side_stream)


def wgrad_splits(rows, m, n, target_tiles=512, max_splits=None):
    """Split-K factor for dW = dY^T X: the contraction runs over all `rows` tokens while the
    output has only (m/256)*(n/256) tiles (9..72 for DNABERT-2), far fewer than 256 CUs.
    Smallest power of two giving >= target_tiles tiles, capped at 64 (measured at b=256: Wqkv
    545 us at s=32 vs 635-738 at s=16; Wg best at 8, Wwo at 16, Wo flat from 16 to 64)."""
    if max_splits is None:
        max_splits = int(os.environ.get("DNA_WGRAD_MAX_SPLITS", 64))
    tiles = max(1, (m // 256) * (n // 256))
    s = 1
    while s < max_splits and tiles * s < target_tiles:
        s *= 2
    while s > 1 and (rows % s or rows // s < 256):
        s //= 2
    return s


def _hip_wgrad_ok(dy, x):
    """The persistent token-major weight-gradient kernel (dna_linear_wgrad_p) for every bf16
    projection with 256-multiple sides -- all of DNABERT-2's. At the bench shapes (T = 262,144)
    it is 1-22 % faster than hipBLASLt's split-K batched GEMM (0.40-0.43 of the bf16 peak vs
    0.34-0.42; profiles/r03/wgrad_ab*.jsonl). DNA_WGRAD_IMPL=torch is the A/B arm."""
    rows, m = dy.shape
    n = x.shape[1]
    # the kernel needs two 64-row K-steps per split: a handful of rows (the MLM head's masked rows
    # of a tiny micro-batch, or none) goes to the torch split-K path
    return (dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dy.is_cuda
            and rows >= 128 and m % 256 == 0 and n % 256 == 0 and _gemm_impl() == "hip"
            and os.environ.get("DNA_WGRAD_IMPL", "hip") == "hip")


def _small_wgrad_ok(dy, x):
    """A handful of rows (the [CLS] rows of a fine-tuning batch in the last layer, the masked rows
    of a tiny micro-batch): below dna_linear_wgrad_p's two 64-row K-steps per split, so dW runs
    on the strided MFMA GEMM (dna_gemm_bf16_strided, fp32 out, any shape) instead of a library
    GEMM."""
    return (dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dy.is_cuda
            and 1 <= dy.shape[0] < 128 and _gemm_impl() == "hip"
            and os.environ.get("DNA_WGRAD_IMPL", "hip") == "hip")


def _small_wgrad(dy, x, out, accumulate):
    """out[m, n] (+)= dy[rows, m]^T x[rows, n], fp32 out, one launch."""
    dy, x = dy.contiguous(), x.contiguous()
    rows, m = dy.shape
    n = x.shape[1]
    strided_gemm(dy, (1, m, 0), x, (n, 1, 0), out, (n, 0), m, n, rows, 1, out_f32=True,
                 accumulate=accumulate)


def _hip_wgrad_parts(dy, x):
    """fp32 split-K partials [s, m, n] of dy^T x from the persistent MFMA kernel (token-major
    operands read in place; s chosen by the library to fill the grid)."""
    dy, x = dy.contiguous(), x.contiguous()
    rows, m = dy.shape
    n = x.shape[1]
    s = N.lib().dna_linear_wgrad_p_splits(rows, m, n)
    parts = torch.empty(s, m, n, device=dy.device, dtype=torch.float32)
    N.call("dna_linear_wgrad_p", dy.data_ptr(), x.data_ptr(), rows, m, n, s, parts.data_ptr(),
           N.stream_ptr())
    return parts, s


def wgrad(dy, x):
    """fp32 dW [m, n] = dy[rows, m]^T x[rows, n] (split-K partials + fp32 sum for bf16; the
    exact-fp32 MFMA kernel's slices for fp32)."""
    if _f32_gemm_ok(x, dy):
        parts, s = _hip_wgrad_f32_parts(dy, x)
        out = torch.empty(parts.shape[1:], device=dy.device, dtype=torch.float32)
        N.call("dna_sum_slices", parts.data_ptr(), s, out.numel(), out.data_ptr(), N.stream_ptr())
        return out
    if x.dtype == torch.float32:
        library_fallback("weight gradient", dy.shape, x.shape)
        return torch.mm(dy.t(), x)
    if _hip_wgrad_ok(dy, x):
        parts, s = _hip_wgrad_parts(dy, x)
        out = torch.empty(parts.shape[1:], device=dy.device, dtype=torch.float32)
        N.call("dna_sum_slices", parts.data_ptr(), s, out.numel(), out.data_ptr(), N.stream_ptr())
        return out
    if _small_wgrad_ok(dy, x):
        out = torch.empty(dy.shape[1], x.shape[1], device=dy.device, dtype=torch.float32)
        _small_wgrad(dy, x, out, False)
        return out
    library_fallback("weight gradient", dy.shape, x.shape)
    rows, m = dy.shape
    n = x.shape[1]
    s = wgrad_splits(rows, m, n)
    if s == 1:
        return torch.mm(dy.t(), x, out_dtype=torch.float32)
    a = dy.view(s, rows // s, m).transpose(1, 2)
    b = x.view(s, rows // s, n)
    return torch.bmm(a, b, out_dtype=torch.float32).sum(0)


def wgrad_accumulate(dy, x, grad):
    """grad[m, n] += dy^T x: split-K partials (the persistent MFMA kernel; hipBLASLt batched GEMM
    for shapes it does not take, or with DNA_WGRAD_IMPL=torch) folded in by one native pass."""
    rows, m = dy.shape
    n = x.shape[1]
    assert grad.is_contiguous() and grad.dtype == torch.float32 and grad.shape == (m, n)
    if _hip_wgrad_ok(dy, x):
        parts, s = _hip_wgrad_parts(dy, x)
        N.call("dna_sum_slices_accum", parts.data_ptr(), s, m * n, grad.data_ptr(), N.stream_ptr())
        return
    if _small_wgrad_ok(dy, x):
        _small_wgrad(dy, x, grad, True)
        return
    library_fallback("weight gradient", dy.shape, x.shape)
    s = wgrad_splits(rows, m, n)
    if s == 1:
        parts = torch.mm(dy.t(), x, out_dtype=torch.float32)
    else:
        parts = torch.bmm(dy.view(s, rows // s, m).transpose(1, 2), x.view(s, rows // s, n),
                          out_dtype=torch.float32)
    N.call("dna_sum_slices_accum", parts.data_ptr(), s, m * n, grad.data_ptr(), N.stream_ptr())


def _weight_grad(w, dy, x, flops):
    """dW = dy^T x of the projection with fp32 master weight w: straight into the flat gradient
    buffer when a FlatParams owns w (None returned, bucket reducer notified), else returned."""
    direct = (getattr(w, "_dna_direct", False) and w.grad is not None and x.dtype != torch.float32
              and (_hip_wgrad_ok(dy, x) or _small_wgrad_ok(dy, x)))
    side = _side_stream() if direct else None
    if side is not None:
        # wgrad beside the rest of the backward; dy / x must outlive it on the side stream
        side.wait_stream(torch.cuda.current_stream())
        _KEEP.append((dy, x))  # (record_stream instead made the allocator thrash)
        with torch.cuda.stream(side), _timed("gemm_wgrad", flops):
            wgrad_accumulate(dy, x, w.grad)
        _queue_join()
        _notify_direct(w)
        return None
    with _timed("gemm_wgrad", flops):
        if direct:
            # write straight into the flat fp32 gradient buffer (dna_amd.flat) and tell the
            # gradient-bucket reducer, instead of returning dW to AccumulateGrad
            wgrad_accumulate(dy, x, w.grad)
            _notify_direct(w)
            return None
        return wgrad(dy, x)


def geglu_out_fused_ok(g, w_lp, w_lpt):
    """GeGLUOut applies: bf16 path, the transposed wo copy present, kernel-legal shapes
    (hidden % 128, F % 256), DNA_GEGLU_BWD_FUSED not 0."""
    if w_lpt is None or os.environ.get("DNA_GEGLU_BWD_FUSED", "1") == "0":
        return False
    Nh, F = w_lp.shape
    return (g.dtype == torch.bfloat16 and _hip_gemm_ok(g, w_lp, Nh, F) and w_lpt.shape == (F, Nh)
            and g.shape[1] == 2 * F and Nh % 128 == 0 and F % 256 == 0)


class GeGLUOut(torch.autograd.Function):
    """o = dropout(gelu(g[:, :F]) * g[:, F:]) . wo^T  (bert_layers.py:292-297, the bias going to
    the LayerNorm that follows) as ONE autograd node, so its backward runs the data gradient of
    wo and the GeGLU backward in one launch (dna_geglu_linear_dgrad_p: dg straight from dy, da
    never in memory) beside wo's weight gradient. Forward: the GeGLU output `a` from the
    gated_layers epilogue (Linear, geglu=...) or the separate pass, then the persistent GEMM."""

    @staticmethod
    def forward(ctx, g, p, seed, off, w, w_lp, w_lpt):
        _gpu(g)
        g = g.contiguous()
        # the same `a` (fused epilogue or dna_geglu_fwd) and the backward factors
        a, fac = _geglu_forward(g, p, seed, off)
        n, F2 = g.shape
        flops = 2.0 * n * w_lp.shape[0] * w_lp.shape[1]
        with _timed("gemm_hip", flops):
            o = _hip_linear(a, w_lp, None)
        ctx.save_for_backward(fac, a, w_lpt)
        ctx.weight = w
        return o

    @staticmethod
    def backward(ctx, dy):
        fac, a, w_lpt = ctx.saved_tensors
        dy = dy.contiguous()
        n, F2 = fac.shape
        Nh = dy.shape[1]
        flops = 2.0 * n * Nh * (F2 // 2)
        dg = torch.empty_like(fac)
        with _timed("gemm_geglu_bwd", flops):
            N.call("dna_geglu_linear_dgrad_p", dy.data_ptr(), w_lpt.data_ptr(), fac.data_ptr(), n,
                   F2 // 2, Nh, dg.data_ptr(), N.stream_ptr())
        dw = _weight_grad(ctx.weight, dy, a, flops)
        return dg, None, None, None, dw, None, None


def geglu_out(g, p, seed, off, w, w_lp, w_lpt):
    return GeGLUOut.apply(g, p, seed, off, w, w_lp, w_lpt)


def linear(x, w, w_lp, b=None, w_lpt=None, geglu=None):
    """geglu=(p, seed, offset): the output feeds GeGLU.apply(y, p, seed, offset) next -- fuse
    that GeGLU forward into the GEMM epilogue when the shapes allow (DNA_GEGLU_FUSED=0: never)."""
    return Linear.apply(x, w, w_lp if w_lp is not None else w, b, w_lpt, geglu)


# ----------------------------------------------------------------------------------- dilated conv
def conv_impl():
    """"hip" (default): the dilated convolutions on csrc/dilated_conv.hip; "torch": F.conv1d
    (MIOpen), for measurement only (DNA_CONV_IMPL; counted as a library fallback, so
    DNA_STRICT_NATIVE=1 refuses it)."""
    return os.environ.get("DNA_CONV_IMPL", "hip")


def _shadow(w, dt):
    """The parameter in the compute dtype: the trainer's persistent bf16 copy (`_dna_lp`) while it
    still stands for the parameter -- the trainer stamps the parameter's version on it whenever it
    re-derives the copy, and an in-place change outside the fused AdamW step (load_state_dict, a
    manual edit) moves the version on -- else a cast of the parameter itself."""
    lp = getattr(w, "_dna_lp", None)
    if (dt == torch.bfloat16 and lp is not None
            and getattr(w, "_dna_lp_version", None) == w._version):
        return lp
    return w.detach().to(dt)


def conv_taps(w, dt):
    """Conv1d weight [co, ci, K] -> the kernel's tap-major [K, co, ci] in the compute dtype."""
    return _shadow(w, dt).permute(2, 0, 1).contiguous()


def conv_taps_dgrad(w, dt):
    """The data gradient's weight: taps reversed, W transposed -> [K, ci, co]."""
    return _shadow(w, dt).flip(2).permute(2, 1, 0).contiguous()


def _dconv(x, w_taps, bias, dilation, epilogue, act, g=None, res=None, out=None, z=None,
           res_out=None):
    B, L, C = x.shape
    K = w_taps.shape[0]
    with _timed("dconv", 2.0 * B * L * C * C * K):
        N.call("dna_dconv_fwd", x.data_ptr(), _dt(x), w_taps.data_ptr(), _p(bias), B, L, C, K,
               int(dilation), epilogue, act, _p(g), _p(res), _p(out), _p(z), _p(res_out),
               N.stream_ptr())


def _dconv_wgrad(dz, x, w, b, dilation):
    """(dW, db) of one Conv1d(C, C, K), or (None, None) after adding them straight into the flat
    gradient when a FlatParams trainer owns both parameters."""
    B, L, C = x.shape
    K = w.shape[2]
    direct = _param_grads_direct((w, b)) and tuple(w.grad.shape) == tuple(w.shape)
    dw = w.grad if direct else torch.empty(C, C, K, device=x.device, dtype=torch.float32)
    db = None if b is None else (b.grad if direct else torch.empty(C, device=x.device,
                                                                   dtype=torch.float32))
    nws = N.lib().dna_dconv_wgrad_workspace(B, L, C, K)
    ws = torch.empty(nws, device=x.device, dtype=torch.uint8)
    with _timed("dconv_wgrad", 2.0 * B * L * C * C * K):
        N.call("dna_dconv_wgrad", dz.data_ptr(), x.data_ptr(), _dt(x), B, L, C, K, int(dilation),
               dw.data_ptr(), _p(db), int(direct), ws.data_ptr(), nws, N.stream_ptr())
    if direct:
        _notify_direct(w, b)
        return None, None
    return dw, db


class GatedDilatedConv(torch.autograd.Function):
    """One layer of the reference's CNNModel in mode "dilation" (denoise.py:469-484) after its two
    LayerNorms, as one node:
        g = act_g(gates[i](rc_norm)),  h = gelu(convs[i](h_norm))       act_g: sigmoid | gelu
        feat_new = h * g + feat (forget) | h + g + feat,   rc_new = g + rc
    h_norm, rc_norm [B, L, C] channels-last in the compute dtype (bf16 under bf16 autocast, else
    fp32); feat, rc, feat_new, rc_new fp32 (the residual streams stay fp32). Two launches of
    dna_dconv_fwd, the combine in their epilogues; saved for the backward: the two inputs, z_h,
    g and (GELU gate) z_g. Backward: one elementwise kernel (dz_h, dz_g), the two data gradients
    through the same convolution kernel, the weight and bias gradients from split partials
    (deterministic), written straight into the flat gradient where a trainer owns the parameters."""

    @staticmethod
    def forward(ctx, h_norm, rc_norm, feat, rc, conv_w, conv_b, gate_w, gate_b, dilation, forget):
        _gpu(h_norm, rc_norm, feat, rc, conv_w, gate_w)
        B, L, C = h_norm.shape
        # every conv of this model maps C to C, so h always has feat's shape (the reference's
        # `else: feat = h` branch cannot be reached)
        assert conv_w.shape[:2] == (C, C) and gate_w.shape == conv_w.shape, \
            "GatedDilatedConv: Conv1d(C, C, K) only"
        assert rc_norm.shape == h_norm.shape == feat.shape == rc.shape
        dt = h_norm.dtype
        x_h, x_g = h_norm.contiguous(), rc_norm.to(dt).contiguous()
        feat, rc = feat.float().contiguous(), rc.float().contiguous()
        forget = bool(forget)
        g = torch.empty_like(x_g)
        z_g = None if forget else torch.empty_like(x_g)
        rc_new, feat_new = torch.empty_like(rc), torch.empty_like(feat)
        z_h = torch.empty_like(x_h)
        _dconv(x_g, conv_taps(gate_w, dt), gate_b, dilation, N.DCONV_GATE,
               N.ACT_SIGMOID if forget else N.ACT_GELU, res=rc, out=g, z=z_g, res_out=rc_new)
        _dconv(x_h, conv_taps(conv_w, dt), conv_b, dilation,
               N.DCONV_MAIN_MUL if forget else N.DCONV_MAIN_ADD, N.ACT_GELU, g=g, res=feat, z=z_h,
               res_out=feat_new)
        ctx.save_for_backward(x_h, x_g, z_h, g, z_g)
        ctx.params = (conv_w, conv_b, gate_w, gate_b)
        ctx.cfg = (int(dilation), forget)
        ctx.set_materialize_grads(False)
        return feat_new, rc_new

    @staticmethod
    def backward(ctx, dfeat, drc):
        x_h, x_g, z_h, g, z_g = ctx.saved_tensors
        conv_w, conv_b, gate_w, gate_b = ctx.params
        dilation, forget = ctx.cfg
        if dfeat is None:
            dfeat = torch.zeros(x_h.shape, device=x_h.device, dtype=torch.float32)
        dfeat = dfeat.float().contiguous()
        drc = None if drc is None else drc.float().contiguous()
        dz_h, dz_g = torch.empty_like(z_h), torch.empty_like(z_h)
        N.call("dna_dconv_bwd_elem", dfeat.data_ptr(), _p(drc), z_h.data_ptr(), g.data_ptr(),
               _p(z_g), _dt(z_h), z_h.numel(), int(forget), dz_h.data_ptr(), dz_g.data_ptr(),
               N.stream_ptr())
        dt = x_h.dtype
        dx_h = dx_g = None
        if ctx.needs_input_grad[0]:
            dx_h = torch.empty_like(x_h)
            _dconv(dz_h, conv_taps_dgrad(conv_w, dt), None, dilation, N.DCONV_PLAIN, N.ACT_NONE,
                   out=dx_h)
        if ctx.needs_input_grad[1]:
            dx_g = torch.empty_like(x_g)
            _dconv(dz_g, conv_taps_dgrad(gate_w, dt), None, dilation, N.DCONV_PLAIN, N.ACT_NONE,
                   out=dx_g)
        dwc, dbc = _dconv_wgrad(dz_h, x_h, conv_w, conv_b, dilation)
        dwg, dbg = _dconv_wgrad(dz_g, x_g, gate_w, gate_b, dilation)
        return dx_h, dx_g, dfeat, drc, dwc, dbc, dwg, dbg, None, None


class OneHotConv(torch.autograd.Function):
    """act(Conv1d(V, C, KW, padding (KW - 1) / 2)(one_hot(ids))) -> [B, L, C] fp32 as a table
    lookup (dna_onehot_conv_fwd); complement: on 3 - id for id < 4 (N stays). The backward
    recomputes z and sums the [C, V, KW] gradient from per-block partials in a fixed order."""

    @staticmethod
    def forward(ctx, ids, w, b, complement, act=N.ACT_GELU):
        _gpu(ids, w, b)
        if act not in (N.ACT_GELU, N.ACT_RELU):
            raise ValueError(f"dna_amd: onehot_conv act must be ACT_GELU or ACT_RELU, got {act}")
        ids = ids.to(torch.int64).contiguous()
        B, L = ids.shape
        C, V, KW = w.shape
        w32, b32 = w.detach().float().contiguous(), None if b is None else b.detach().float().contiguous()
        out = torch.empty(B, L, C, device=ids.device, dtype=torch.float32)
        N.call("dna_onehot_conv_fwd", ids.data_ptr(), w32.data_ptr(), _p(b32), B, L, C, V, KW,
               int(bool(complement)), int(act), out.data_ptr(), N.stream_ptr())
        ctx.save_for_backward(ids)
        ctx.params = (w, b)
        ctx.complement = bool(complement)
        ctx.act = int(act)
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        w, b = ctx.params
        B, L = ids.shape
        C, V, KW = w.shape
        dout = dout.float().contiguous()
        direct = _param_grads_direct((w, b)) and tuple(w.grad.shape) == tuple(w.shape)
        dw = w.grad if direct else torch.empty(C, V, KW, device=ids.device, dtype=torch.float32)
        db = None if b is None else (b.grad if direct else torch.empty(C, device=ids.device,
                                                                       dtype=torch.float32))
        w32, b32 = w.detach().float().contiguous(), None if b is None else b.detach().float().contiguous()
        nws = N.lib().dna_onehot_conv_bwd_workspace(B, L, C, V, KW)
        ws = torch.empty(nws, device=ids.device, dtype=torch.uint8)
        N.call("dna_onehot_conv_bwd", ids.data_ptr(), w32.data_ptr(), _p(b32), dout.data_ptr(), B,
               L, C, V, KW, int(ctx.complement), ctx.act, dw.data_ptr(), _p(db), int(direct),
               ws.data_ptr(), nws, N.stream_ptr())
        if direct:
            _notify_direct(w, b)
            return None, None, None, None, None
        return None, dw, db, None, None


def onehot_conv(ids, weight, bias, complement=False, act=N.ACT_GELU):
    """act: N.ACT_GELU (the fine-tuning forward) | N.ACT_RELU (the pretraining forward's `linear`)."""
    return OneHotConv.apply(ids, weight, bias, complement, act)
