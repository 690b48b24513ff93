"""The wide pooling-head kernels alone (csrc/pool_head.hip, dna_pool_head_wide_*: up to 1024
labels, regression and multi-label) against float64 torch.

Tolerance: the rule of tests/test_gpu_pool_head.py, verbatim. Every output is compared with the
same computation in float64 on the same operands (bf16 inputs are rounded to bf16 first, then
upcast). The yardstick per tensor is the largest of
  - the error of CPU fp32 torch (mean -> F.linear -> loss, with autograd) against float64,
  - the error of the reference's own form of the pool in fp32 (torch.cumsum(x, -2) / arange,
    indexed at the window's end) carried through the same head,
  - the floor 2^-24 max|ref| (half an fp32 ulp of the tensor's largest value),
and the kernel may be at most 4x that. bf16 dx is compared after rounding the float64 reference
to bf16 and may differ by one bf16 ulp. Where the wide op runs a shape the narrow op also takes,
the two agree within the sum of their two bounds.

Measured on MI355X, kernel max-abs error against float64 / the yardstick, over every case below:
  pooled      0 .. 2.4e-7 / 2.9e-8 .. 2.4e-7        ratio 0.00 .. 1.42 (largest: RCPS in place, fp32)
  logits      1.5e-8 .. 1.9e-7 / 3.3e-8 .. 1.0e-6   ratio 0.13 .. 0.59
  loss        1.5e-10 .. 6.9e-8 / 4.2e-8 .. 1.9e-7  ratio 0.00 .. 0.76
  dx (fp32)   3.2e-13 .. 1.5e-8 / 1.9e-12 .. 4.1e-8 ratio 0.06 .. 1.00
  dx (bf16)   equal to the bf16-rounded float64 reference except 9 .. 21 of ~200,000 elements one
              bf16 ulp off at (130, 7, 256, 1024) and (1025, 3, 64, 257)
  dW          4.0e-12 .. 1.2e-7 / 6.7e-12 .. 7.3e-8 ratio 0.11 .. 1.77 (largest: (2, 16, 8, 1))
  dbias       1.4e-11 .. 7.8e-8 / 3.4e-11 .. 9.9e-8 ratio 0.14 .. 1.00
The bound of 4 was never closer than 1.77: logits, gs = dlogits W and dW accumulate in double, so
what is left is the pool's fp32 sums (shared with the narrow head) and one rounding per output.
"""
import pytest
import torch

import dna_amd.ops  # noqa: F401  (registers torch.ops.dna_amd.*)
from test_gpu_pool_head import DEV, _bf16_ulp, _labels, _operands, _reference, _run, _windows

gpu = pytest.mark.gpu
REG, MULTI, SINGLE = "regression", "multi_label_classification", "single_label_classification"
PROBLEMS = [REG, MULTI]
# (B, L, D, C): the first wide C, one row, one position | VEC = 1, C no multiple of the tile,
# DeepSEA's C | the largest C | more rows than a workgroup has threads, C just over 256
WIDE_SHAPES = [(1, 1, 8, 65), (3, 130, 118, 919), (130, 7, 256, 1024), (1025, 3, 64, 257)]
DIRECT_SHAPES = [(2, 1026, 128, 3), (2, 16, 8, 1)]
dtypes = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def _bounds(x, w, bias, layout, start, count, labels, problem, **kw):
    """-> (float64 reference, {tensor: 4 x yardstick}) by test_gpu_pool_head's rule."""
    args = (x, w, bias, layout, start, count, labels, problem)
    ref = _reference(*args, torch.float64, **kw)
    cpu = _reference(*args, torch.float32, **kw)
    cum = _reference(*args, torch.float32, form="cumsum", **kw)
    bound = {}
    for k, r in ref.items():
        floor = float(r.abs().max()) * 2.0 ** -24
        bound[k] = 4 * max(float((cpu[k] - r).abs().max()), float((cum[k] - r).abs().max()), floor)
    return ref, bound


def _compare(got, ref, bound, dtype, tag):
    bad = {}
    for k, r in ref.items():
        g = got[k].detach().cpu()
        assert bool(torch.isfinite(g.float()).all()), (tag, k, "non-finite")
        if k == "dx" and dtype == torch.bfloat16:
            rb = r.to(torch.bfloat16).float()
            diff = (g.float() - rb).abs()
            over = (diff - _bf16_ulp(rb)).max().item()
            print(f"{tag} dx(bf16): {int((diff > 0).sum())} of {diff.numel()} elements one ulp off"
                  f", worst |diff| - ulp = {over:.3e}")
            if over > 0:
                bad[k] = over
            continue
        err = float((g.double().reshape(r.shape) - r).abs().max())
        yard = bound[k] / 4
        print(f"{tag} {k}: kernel {err:.3e} yardstick {yard:.3e} ratio {err / yard:.2f}")
        if not err <= bound[k]:
            bad[k] = (err, yard)
    assert not bad, (tag, bad)


def _check(got, x, w, bias, layout, start, count, labels, problem, dtype, tag, **kw):
    ref, bound = _bounds(x, w, bias, layout, start, count, labels, problem, **kw)
    _compare(got, ref, bound, dtype, tag)
    return ref, bound


def _raw(name, *args):
    from dna_amd import _native as N
    N.call(name, *args, N.stream_ptr())


@gpu
def test_argument_errors():
    """Run first, with valid pointers: every refusal names its field and launches nothing."""
    from dna_amd import _native as N
    B, L, D = 2, 16, 8
    x = torch.zeros(B * L * D, device=DEV)
    w = torch.zeros(1025 * D, device=DEV)
    pooled, logits = torch.zeros(B * D, device=DEV), torch.zeros(B * 1025, device=DEV)
    labels, dl, loss = torch.zeros(B * 1025, device=DEV), torch.zeros(B * 1025, device=DEV), \
        torch.zeros(1, device=DEV)
    ws = torch.zeros(1 << 16, device=DEV)

    def fwd(C, problem=N.CLS_MULTI_LABEL, ws_bytes=ws.numel() * 4):
        _raw("dna_pool_head_wide_fwd", x.data_ptr(), D, None, 0, 0, N.F32, None, None,
             w.data_ptr(), None, B, L, D, C, pooled.data_ptr(), logits.data_ptr(),
             labels.data_ptr(), problem, loss.data_ptr(), dl.data_ptr(), ws.data_ptr(), ws_bytes)

    def bwd(C, ws_bytes=ws.numel() * 4):
        dx, dw = torch.zeros(B * L * D, device=DEV), torch.zeros(1025 * D, device=DEV)
        _raw("dna_pool_head_wide_bwd", dl.data_ptr(), None, pooled.data_ptr(), w.data_ptr(), None,
             None, B, L, D, C, N.F32, dx.data_ptr(), D, None, 0, 0, dw.data_ptr(), None, 0,
             ws.data_ptr(), ws_bytes)

    fwd(65)
    bwd(65)
    for C in (0, 1025):
        with pytest.raises(N.NativeError, match="labels"):
            fwd(C)
        with pytest.raises(N.NativeError, match="labels"):
            bwd(C)
    with pytest.raises(N.NativeError, match="problem type single_label"):
        fwd(65, problem=N.CLS_SINGLE_LABEL)
    need = N.lib().dna_pool_head_wide_fwd_workspace(B, L, D, 65)
    assert need == N.lib().dna_pool_head_fwd_workspace(B, L, D) + 8  # one loss workgroup's sum
    with pytest.raises(N.NativeError, match="workspace"):
        fwd(65, ws_bytes=need - 8)
    with pytest.raises(N.NativeError, match="workspace"):
        bwd(65, ws_bytes=N.lib().dna_pool_head_wide_bwd_workspace(B, L, D, 65) - 4)
    torch.cuda.synchronize()


@gpu
@dtypes
@pytest.mark.parametrize("problem", PROBLEMS)
@pytest.mark.parametrize("B,L,D,C", WIDE_SHAPES)
def test_forward_backward_vs_float64(B, L, D, C, problem, dtype):
    x, w, bias = _operands(B, L, D, D, C, dtype)
    labels = _labels(problem, B, C)
    got = _run(x, w, bias, "single", None, None, labels, problem, dtype)
    assert got["pred"] is None
    _check(got, x, w, bias, "single", None, None, labels, problem, dtype,
           f"[{B},{L},{D},{C}] {problem} {dtype}")


def _wide_op(x, w, bias, labels, problem, dtype):
    """Forward with loss + backward through torch.ops.dna_amd.pool_head_wide_*."""
    from dna_amd import functional as DF
    o = torch.ops.dna_amd
    B, L, D = x.shape
    C = w.shape[0]
    xd, wd = x.to(DEV).to(dtype), w.to(DEV)
    bd = None if bias is None else bias.to(DEV)
    pooled, logits = torch.empty(B, D, device=DEV), torch.empty(B, C, device=DEV)
    loss, dl = torch.empty(1, device=DEV), torch.empty(B, C, device=DEV)
    o.pool_head_wide_fwd(xd, None, False, False, None, None, wd, bd, pooled, logits,
                         labels.to(DEV).float().reshape(B, C).contiguous(),
                         DF.CLS_PROBLEMS[problem], loss, dl)
    dx = torch.full((B, L, D), float("nan"), device=DEV, dtype=dtype)
    dw = torch.empty(C, D, device=DEV)
    db = None if bias is None else torch.empty(C, device=DEV)
    o.pool_head_wide_bwd(dl, pooled, wd, None, None, dx, None, False, False, dw, db, False)
    out = dict(pooled=pooled, logits=logits, loss=loss, dx=dx, dw=dw)
    if db is not None:
        out["dbias"] = db
    return out


@gpu
@dtypes
@pytest.mark.parametrize("problem", PROBLEMS)
@pytest.mark.parametrize("B,L,D,C", DIRECT_SHAPES)
def test_wide_op_on_narrow_shapes_agrees_with_narrow_op(B, L, D, C, problem, dtype):
    x, w, bias = _operands(B, L, D, D, C, dtype, seed=3)
    labels = _labels(problem, B, C).reshape(B, C)
    wide = _wide_op(x, w, bias, labels, problem, dtype)
    tag = f"direct [{B},{L},{D},{C}] {problem} {dtype}"
    ref, bound = _check(wide, x, w, bias, "single", None, None, labels, problem, dtype, tag)
    narrow = _run(x, w, bias, "single", None, None, labels, problem, dtype)
    for k in ref:
        a, b = wide[k].detach().float().cpu(), narrow[k].detach().float().cpu().reshape(wide[k].shape)
        if k == "dx" and dtype == torch.bfloat16:  # each within one ulp of the same value
            assert float(((a - b).abs() - 2 * _bf16_ulp(ref[k].to(torch.bfloat16).float())).max()) <= 0
        else:
            assert float((a.double() - b.double()).abs().max()) <= 2 * bound[k], (tag, k)


VARIANT = (3, 130, 118, 919)


@gpu
@dtypes
@pytest.mark.parametrize("problem", PROBLEMS)
def test_no_bias_windows_and_upstream(problem, dtype):
    """No bias; a prefix, a middle and an empty window; the loss's gradient 0.25 from upstream."""
    B, L, D, C = VARIANT
    x, w, _ = _operands(B, L, D, D, C, dtype, seed=4, bias=False)
    labels = _labels(problem, B, C)
    start, count = [0, 17, 5], [130, 50, 0]
    got = _run(x, w, None, "single", start, count, labels, problem, dtype, upstream=0.25)
    _check(got, x, w, None, "single", start, count, labels, problem, dtype,
           f"windows {problem} {dtype}", upstream=0.25)
    dx = got["dx"].float().cpu()
    st, cn = _windows(B, L, start, count)
    for b in range(B):
        outside = torch.cat([dx[b, :st[b]], dx[b, st[b] + cn[b]:]])
        assert outside.numel() == 0 or outside.abs().max().item() == 0
    assert got["pooled"][2].abs().max().item() == 0 and dx[2].abs().max().item() == 0


@gpu
@dtypes
@pytest.mark.parametrize("layout", ["rcps", "rcps_mirror"])
def test_rcps_halves_in_place(layout, dtype):
    """x [2, 67, 2 x 64] read in place as two halves, the second flipped (and its window
    mirrored); the one [B, L, 2D] dx is checked whole."""
    B, L, D, C = 2, 67, 64, 130
    x, w, bias = _operands(B, L, 2 * D, D, C, dtype, seed=5)
    labels = _labels(MULTI, B, C)
    start, count = ([0, 7], [67, 30]) if layout == "rcps_mirror" else (None, [67, 30])
    got = _run(x, w, bias, layout, start, count, labels, MULTI, dtype)
    assert got["dx"].shape == (B, L, 2 * D)
    _check(got, x, w, bias, layout, start, count, labels, MULTI, dtype, f"{layout} {dtype}")


def _raw_bwd(dl, up, pooled, w, B, L, D, C, dx, dw, db, accumulate):
    from dna_amd import _native as N
    ws = torch.empty(max(N.lib().dna_pool_head_wide_bwd_workspace(B, L, D, C) // 4, 4), device=DEV)
    _raw("dna_pool_head_wide_bwd", dl.data_ptr(), None if up is None else up.data_ptr(),
         pooled.data_ptr(), w.data_ptr(), None, None, B, L, D, C, N.F32,
         None if dx is None else dx.data_ptr(), D, None, 0, 0, dw.data_ptr(), db.data_ptr(),
         int(accumulate), ws.data_ptr(), ws.numel() * 4)
    torch.cuda.synchronize()


@gpu
def test_upstream_accumulates_into_nonzero_buffers_and_frozen_backbone():
    """upstream = 0.25 added into non-zero dW / dbias is one fp32 add of the plain call's value;
    dx, handed over full of NaN, is written whole and never accumulated; without dx1 (a frozen
    backbone) the parameter gradients are the same bits."""
    B, L, D, C = VARIANT
    g = torch.Generator().manual_seed(11)
    dl = (torch.randn(B, C, generator=g) / (B * C)).to(DEV)
    pooled, w = torch.randn(B, D, generator=g).to(DEV), torch.randn(C, D, generator=g).to(DEV)
    up = torch.tensor([0.25], device=DEV)
    plain = [torch.empty(C, D, device=DEV), torch.empty(C, device=DEV)]
    dx0 = torch.full((B, L, D), float("nan"), device=DEV)
    _raw_bwd(dl, up, pooled, w, B, L, D, C, dx0, *plain, False)
    init = [torch.randn(C, D, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)]
    accd = [t.clone() for t in init]
    dx1 = torch.full((B, L, D), float("nan"), device=DEV)
    _raw_bwd(dl, up, pooled, w, B, L, D, C, dx1, *accd, True)
    frozen = [torch.empty(C, D, device=DEV), torch.empty(C, device=DEV)]
    _raw_bwd(dl, up, pooled, w, B, L, D, C, None, *frozen, False)
    for p, a, i, f in zip(plain, accd, init, frozen):
        assert torch.equal(a, i + p) and torch.equal(f, p)
    assert not bool(torch.isnan(dx0).any()) and torch.equal(dx0, dx1)
    dl64, w64, p64 = dl.double().cpu(), w.double().cpu(), pooled.double().cpu()
    for got, ref in ((plain[0], 0.25 * dl64.T @ p64), (plain[1], 0.25 * dl64.sum(0)),
                     (dx0[:, 0], 0.25 * dl64 @ w64 / L)):
        # one rounding of a double sum: half an fp32 ulp of the value, the rule's floor
        assert float((got.double().cpu() - ref).abs().max()) <= 4 * 2.0 ** -24 * float(ref.abs().max())


@gpu
def test_bit_identical_from_run_to_run():
    B, L, D, C = VARIANT
    x, w, bias = _operands(B, L, D, D, C, torch.bfloat16, seed=8)
    labels = _labels(MULTI, B, C)
    runs = [_run(x, w, bias, "single", None, [130, 50, 1], labels, MULTI, torch.bfloat16)
            for _ in range(2)]
    for k in ("pooled", "logits", "loss", "dx", "dw", "dbias"):
        assert torch.equal(runs[0][k], runs[1][k]), k


@gpu
def test_dispatch_by_label_count(monkeypatch):
    """C alone picks the kernels: 64 the narrow ones, 65 the wide ones, 1025 is refused."""
    from dna_amd import _native as N
    from dna_amd import functional as DF
    called = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    x = torch.randn(2, 16, 8, device=DEV, requires_grad=True)
    for C, wide in ((64, False), (65, True)):
        called.clear()
        w = torch.randn(C, 8, device=DEV, requires_grad=True)
        labels = (torch.rand(2, C, device=DEV) < 0.4).float()
        _, loss, _ = DF.pool_head(x, w, labels=labels, problem_type=MULTI)
        loss.backward()
        names = [n for n in called if "pool_head" in n]
        assert names == (["dna_pool_head_wide_fwd", "dna_pool_head_wide_bwd"] if wide else
                         ["dna_pool_head_fwd", "dna_pool_head_bwd"]), names
    w = torch.randn(1025, 8, device=DEV)
    with pytest.raises(ValueError, match="1024"):
        DF.pool_head(x, w)
    with pytest.raises(ValueError, match="single_label"):
        DF.pool_head(x, torch.randn(65, 8, device=DEV), labels=torch.zeros(2, dtype=torch.int64,
                                                                           device=DEV),
                     problem_type=SINGLE)
    torch.cuda.synchronize()


def test_registry_has_the_wide_ops_and_they_reject_cpu_tensors():
    from dna_amd import ops
    o = torch.ops.dna_amd
    for name in ("pool_head_wide_fwd", "pool_head_wide_bwd"):
        assert name in ops.OPS and hasattr(o, name)
    x, w = torch.zeros(2, 16, 8), torch.zeros(70, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        o.pool_head_wide_fwd(x, None, False, False, None, None, w, None, torch.zeros(2, 8),
                             torch.zeros(2, 70), None, 0, None, None)
    with pytest.raises(RuntimeError, match="GPU"):
        o.pool_head_wide_bwd(torch.zeros(2, 70), torch.zeros(2, 8), w, None, None, x, None, False,
                             False, torch.zeros(70, 8), None, False)
