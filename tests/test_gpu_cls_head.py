"""The classification-head kernels alone (csrc/cls_head.hip) against float64 torch.

Tolerance. Every output is compared with the same computation in float64 on the same fp32
operands. The yardstick is CPU fp32 torch (F.linear / tanh / cross_entropy and its autograd) on
those operands: its max-abs error against float64 is measured per tensor, and the kernel is
allowed 4x that (a different summation order). An error below half an fp32 ulp of the tensor's
largest value cannot be told from rounding the result to fp32 at all, so the yardstick is floored
there (2^-24 max|ref|): it matters for the one-element tensors (the loss, dbc at C = 1), where the
CPU result is at times the correctly rounded one and its error against float64 is zero.

Measured on MI355X, kernel max-abs error against float64 / the CPU fp32 yardstick:
  t, a        1.2e-7 .. 4.4e-7 / 3.1e-7 .. 1.5e-6   ratio 0.29 .. 0.50 (lanes split the sum over H)
  logits      8.9e-8 .. 4.9e-7 / 6.6e-8 .. 9.1e-7   ratio 0.54 .. 1.36
  loss        2.4e-8 .. 1.6e-7 / 4.5e-8 .. 1.4e-7   ratio 0.47 .. 1.93 (largest: B = 1, one row)
  dx          3.7e-10 .. 4.6e-8 / 6.8e-10 .. 7.9e-8 ratio 0.36 .. 0.58
  dWp, dbp    2.2e-9 .. 1.3e-7 / 3.2e-9 .. 1.0e-7   ratio 0.47 .. 1.69
  dWc, dbc    1.0e-8 .. 3.4e-7 / 1.3e-8 .. 5.9e-7   ratio 0.43 .. 1.60
  loss kernel alone (three problem types): loss 8.3e-9 .. 1.5e-7, dlogits 5.6e-10 .. 1.9e-8,
  ratio 0.09 .. 1.52. The bound of 4 was never closer than 1.93.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dna_amd.ops  # noqa: F401  (registers torch.ops.dna_amd.*)

gpu = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 128, 1), (5, 128, 3), (33, 768, 2), (64, 768, 9)]
KS = float(np.float32(1) / (np.float32(1) - np.float32(0.1)))  # the kernel's fp32 1 / (1 - p)


def _operands(B, H, C, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * B + C)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).float()
    return dict(x=r(B, H), wp=r(H, H, scale=H ** -0.5), bp=r(H, scale=0.1),
                wc=r(C, H, scale=H ** -0.5), bc=r(C, scale=0.1))


def _labels(problem, B, C, seed=0):
    g = torch.Generator().manual_seed(seed + 7)
    if problem == "single_label_classification":
        return torch.randint(0, C, (B,), generator=g)
    if problem == "regression":
        return torch.randn(B, C, generator=g)
    return (torch.rand(B, C, generator=g) < 0.4).float()


def _torch_loss(logits, labels, problem):
    if problem == "regression":
        return F.mse_loss(logits, labels.to(logits.dtype))
    if problem == "single_label_classification":
        return F.cross_entropy(logits, labels)
    return F.binary_cross_entropy_with_logits(logits, labels.to(logits.dtype))


def _reference(ops, labels, problem, dtype, mask=None, upstream=1.0):
    """The head in torch on the CPU in `dtype`; mask: explicit dropout keep mask (scale KS)."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in ops.items()}
    t = torch.tanh(F.linear(p["x"], p["wp"], p["bp"]))
    a = t if mask is None else t * (mask.to(dtype) * KS)
    logits = F.linear(a, p["wc"], p["bc"])
    loss = _torch_loss(logits, labels, problem)
    (loss * upstream).backward()
    out = dict(t=t, a=a, logits=logits, loss=loss.reshape(1), dx=p["x"].grad, dwp=p["wp"].grad,
               dbp=p["bp"].grad, dwc=p["wc"].grad, dbc=p["bc"].grad)
    return {k: v.detach().double() for k, v in out.items()}


def _check(got, ops, labels, problem, mask=None, upstream=1.0, tag=""):
    ref = _reference(ops, labels, problem, torch.float64, mask, upstream)
    cpu = _reference(ops, labels, problem, torch.float32, mask, upstream)
    ratios = {}
    for k, r in ref.items():
        floor = float(r.abs().max()) * 2.0 ** -24
        yard = max(float((cpu[k] - r).abs().max()), floor)
        err = float((got[k].detach().double().cpu().reshape(r.shape) - r).abs().max())
        ratios[k] = (err, yard)
        print(f"{tag} {k}: kernel {err:.3e} cpu-fp32 {yard:.3e} ratio {err / yard:.2f}")
    bad = {k: v for k, v in ratios.items() if not v[0] <= 4 * v[1]}
    assert not bad, bad


def _run_head(ops, labels, problem, p=0.0, seed=0, off=0, x_dev=None):
    """DF.ClsHead forward + loss.backward() on the GPU; returns the outputs and gradients."""
    from dna_amd import functional as DF
    prm = {k: v.to(DEV).requires_grad_(True) for k, v in ops.items() if k != "x"}
    x = ops["x"].to(DEV).requires_grad_(True) if x_dev is None else x_dev
    logits, loss, pred = DF.ClsHead.apply(x, prm["wp"], prm["bp"], prm["wc"], prm["bc"], p, seed,
                                          off, labels.to(DEV), DF.CLS_PROBLEMS[problem])
    return x, prm, logits, loss, pred


def _saved(loss):
    """t and a of the forward (the Function's saved tensors)."""
    fn = loss.grad_fn
    while fn is not None and type(fn).__name__ != "ClsHeadBackward":
        fn = fn.next_functions[0][0]
    return fn.saved_tensors[3], fn.saved_tensors[4]


@gpu
@pytest.mark.parametrize("B,H,C", SHAPES)
def test_forward_backward_vs_float64(B, H, C):
    problem = "regression" if C == 1 else "single_label_classification"
    ops = _operands(B, H, C)
    labels = _labels(problem, B, C)
    x, prm, logits, loss, pred = _run_head(ops, labels, problem)
    t, a = _saved(loss)
    loss.backward()
    got = dict(t=t, a=a, logits=logits, loss=loss.reshape(1), dx=x.grad, dwp=prm["wp"].grad,
               dbp=prm["bp"].grad, dwc=prm["wc"].grad, dbc=prm["bc"].grad)
    _check(got, ops, labels, problem, tag=f"[{B},{H},{C}]")
    if pred is not None:
        assert torch.equal(pred.cpu(), logits.detach().cpu().argmax(-1))


@gpu
def test_bf16_strided_rows_read_in_place():
    B, H, C = 33, 768, 2
    problem = "single_label_classification"
    ops = _operands(B, H, C, seed=3)
    buf = torch.randn(3 * B, H, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    ops["x"] = buf[1::3].float()
    labels = _labels(problem, B, C)
    big = buf.to(DEV).requires_grad_(True)
    xv = big[1::3]
    assert xv.stride(0) == 3 * H and not xv.is_contiguous()
    x, prm, logits, loss, pred = _run_head(ops, labels, problem, x_dev=xv)
    t, a = _saved(loss)
    loss.backward()
    dx = big.grad[1::3].float()
    assert big.grad[0::3].abs().max().item() == 0 and big.grad[2::3].abs().max().item() == 0
    got = dict(t=t, a=a, logits=logits, loss=loss.reshape(1), dwp=prm["wp"].grad,
               dbp=prm["bp"].grad, dwc=prm["wc"].grad, dbc=prm["bc"].grad)
    ref = _reference(ops, labels, problem, torch.float64)
    cpu = _reference(ops, labels, problem, torch.float32)
    for k, v in got.items():
        yard = max(float((cpu[k] - ref[k]).abs().max()), float(ref[k].abs().max()) * 2.0 ** -24)
        err = float((v.detach().double().cpu().reshape(ref[k].shape) - ref[k]).abs().max())
        assert err <= 4 * yard, (k, err, yard)
    # dx leaves the kernel in fp32 and is rounded to x's bf16 once
    err = float((dx.double().cpu() - ref["dx"]).abs().max())
    assert err <= float(ref["dx"].abs().max()) * 2.0 ** -8, err


@gpu
def test_accumulate_into_nonzero_buffers():
    B, H, C = 5, 128, 3
    ops = _operands(B, H, C, seed=9)
    labels = _labels("single_label_classification", B, C).to(DEV)
    d = {k: v.to(DEV) for k, v in ops.items()}
    t, a = torch.empty(B, H, device=DEV), torch.empty(B, H, device=DEV)
    logits, loss = torch.empty(B, C, device=DEV), torch.empty(1, device=DEV)
    dl, pred = torch.empty(B, C, device=DEV), torch.empty(B, device=DEV, dtype=torch.int64)
    o = torch.ops.dna_amd
    o.cls_head_fwd(d["x"], d["wp"], d["bp"], d["wc"], d["bc"], 0.0, 0, 0, t, a, logits)
    o.cls_loss(logits, labels, 1, loss, dl, pred)
    outs = []
    for acc in (False, True):
        g = torch.Generator().manual_seed(11)
        bufs = [torch.randn(*s, generator=g).to(DEV) for s in ((C, H), (C,), (H, H), (H,))]
        init = [b.clone() for b in bufs]
        dx = torch.full((B, H), 7.0, device=DEV)
        o.cls_head_bwd(dl, d["x"], t, a, d["wp"], d["wc"], 0.0, 0, 0, *bufs, dx, acc)
        outs.append((bufs, init, dx))
    (plain, _, dx0), (accd, init, dx1) = outs
    for g0, g1, i in zip(plain, accd, init):
        assert torch.equal(g1, i + g0)  # one fp32 add of the same sum
    assert torch.equal(dx0, dx1)  # dx is always written, never accumulated


@gpu
def test_dropout_mask_rate_determinism_and_backward():
    from dna_amd import functional as DF
    B, H, C, p = 64, 768, 2, 0.1
    problem = "single_label_classification"
    ops = _operands(B, H, C, seed=4)
    labels = _labels(problem, B, C)
    x, prm, logits, loss, _ = _run_head(ops, labels, problem, p=p, seed=1234, off=77)
    t, a = _saved(loss)
    kept = a != 0
    scaled = t * np.float32(KS)
    assert torch.equal(torch.where(kept, a, scaled), scaled)  # a is 0 or t / (1 - p)
    assert int((t == 0).sum()) == 0
    rate = kept.float().mean().item()
    assert abs(rate - 0.9) < 0.007, rate  # 5 sigma of 49,152 draws
    # same (seed, offset): same bits; another offset: another mask
    _, _, logits2, loss2, _ = _run_head(ops, labels, problem, p=p, seed=1234, off=77)
    assert torch.equal(_saved(loss2)[1], a) and torch.equal(logits2, logits)
    _, _, _, loss3, _ = _run_head(ops, labels, problem, p=p, seed=1234, off=78)
    assert not torch.equal(_saved(loss3)[1] != 0, kept)
    # DropoutRNG convention: B * H elements take (B * H + 3) // 4 + 1 Philox groups
    rng = DF.DropoutRNG(5)
    DF.cls_head(x.detach(), *(prm[k].detach() for k in ("wp", "bp", "wc", "bc")), p=p, rng=rng)
    assert rng.offset == (B * H + 3) // 4 + 1
    DF.cls_head(x.detach(), *(prm[k].detach() for k in ("wp", "bp", "wc", "bc")), p=0.0, rng=rng)
    assert rng.offset == (B * H + 3) // 4 + 1  # no draw at p = 0
    loss.backward()
    got = dict(t=t, a=a, logits=logits, loss=loss.reshape(1), dx=x.grad, dwp=prm["wp"].grad,
               dbp=prm["bp"].grad, dwc=prm["wc"].grad, dbc=prm["bc"].grad)
    _check(got, ops, labels, problem, mask=kept.cpu(), tag="[dropout]")


@gpu
@pytest.mark.parametrize("problem,C", [("regression", 1), ("regression", 3),
                                       ("single_label_classification", 9),
                                       ("multi_label_classification", 4)])
def test_loss_three_problem_types(problem, C):
    B = 37
    g = torch.Generator().manual_seed(C)
    logits = (torch.randn(B, C, generator=g) * 3).float()
    labels = _labels(problem, B, C)
    if problem == "single_label_classification":
        logits[4, 2] = logits[4, 6] = logits[4].max() + 1  # a tie: argmax is the lowest index
        logits[9, :] = 0.5
    code = {"regression": 0, "single_label_classification": 1, "multi_label_classification": 2}
    lab = labels.to(DEV) if code[problem] == 1 else labels.float().reshape(B, C).to(DEV)
    loss, dl = torch.empty(1, device=DEV), torch.empty(B, C, device=DEV)
    pred = torch.empty(B, device=DEV, dtype=torch.int64) if code[problem] == 1 else None
    torch.ops.dna_amd.cls_loss(logits.to(DEV), lab, code[problem], loss, dl, pred)
    res = {}
    for dt in (torch.float64, torch.float32):
        lg = logits.to(dt).requires_grad_(True)
        lv = _torch_loss(lg.squeeze() if (problem == "regression" and C == 1) else lg,
                         labels.squeeze() if (problem == "regression" and C == 1) else labels,
                         problem)
        lv.backward()
        res[dt] = (lv.detach().double().reshape(1), lg.grad.double())
    for k, got in ((0, loss), (1, dl)):
        ref, cpu = res[torch.float64][k], res[torch.float32][k]
        yard = max(float((cpu - ref).abs().max()), float(ref.abs().max()) * 2.0 ** -24)
        err = float((got.double().cpu() - ref).abs().max())
        print(f"{problem} C={C} {'loss' if k == 0 else 'dlogits'}: {err:.3e} vs {yard:.3e}")
        assert err <= 4 * yard, (k, err, yard)
    if pred is not None:
        assert torch.equal(pred.cpu(), logits.argmax(-1))
        assert pred[4].item() == 2 and pred[9].item() == 0


@gpu
@pytest.mark.parametrize("B,H,C", [(4, 100, 3), (4, 128, 0), (4, 128, 65)])
def test_argument_errors(B, H, C):
    from dna_amd import _native as N
    z = lambda *s: torch.zeros(*s, device=DEV)
    t, a, logits = z(B, H), z(B, H), z(B, max(C, 1))
    args = (z(B, H).data_ptr(), N.F32, H, z(H, H).data_ptr(), z(H).data_ptr(),
            z(max(C, 1), H).data_ptr(), z(max(C, 1)).data_ptr(), B, H, C, 0.0, 0, 0, t.data_ptr(),
            a.data_ptr(), logits.data_ptr(), None, 1, None, None, None, z(1 << 16).data_ptr(),
            4 << 16, N.stream_ptr())
    with pytest.raises(N.NativeError, match="dna_cls_head_fwd"):
        N.call("dna_cls_head_fwd", *args)
    torch.cuda.synchronize()  # nothing was launched, nothing to fail here
    with pytest.raises(N.NativeError, match="dna_cls_loss" if H % 64 == 0 else "dna_cls_head_bwd"):
        if H % 64 == 0:
            N.call("dna_cls_loss", logits.data_ptr(), z(B).long().data_ptr(), 1, B, C,
                   z(1).data_ptr(), logits.data_ptr(), None, N.stream_ptr())
        else:
            N.call("dna_cls_head_bwd", logits.data_ptr(), None, t.data_ptr(), N.F32, H,
                   t.data_ptr(), a.data_ptr(), z(H, H).data_ptr(), z(C, H).data_ptr(), B, H, C, 0.0,
                   0, 0, z(C, H).data_ptr(), z(C).data_ptr(), z(H, H).data_ptr(), z(H).data_ptr(),
                   z(B, H).data_ptr(), 0, z(1 << 16).data_ptr(), 4 << 16, N.stream_ptr())


@gpu
def test_batch_beyond_the_grid_is_an_argument_error():
    """B above DNA_CLS_MAX_BATCH (8 rows per workgroup x 65,535 grid rows) is refused before any
    launch; the small buffers passed here are never touched."""
    from dna_amd import _native as N
    B, H, C = 8 * 65535 + 1, 128, 3
    z = lambda *s: torch.zeros(*s, device=DEV)
    t, w = z(8, H), z(H, H)
    with pytest.raises(N.NativeError, match=r"batch must be in \[1, 524280\]"):
        N.call("dna_cls_head_fwd", t.data_ptr(), N.F32, H, w.data_ptr(), t.data_ptr(),
               w.data_ptr(), t.data_ptr(), B, H, C, 0.0, 0, 0, t.data_ptr(), t.data_ptr(),
               t.data_ptr(), None, 1, None, None, None, w.data_ptr(), 1 << 40, N.stream_ptr())
    with pytest.raises(N.NativeError, match=r"batch must be in \[1, 524280\]"):
        N.call("dna_cls_head_bwd", t.data_ptr(), None, t.data_ptr(), N.F32, H, t.data_ptr(),
               t.data_ptr(), w.data_ptr(), w.data_ptr(), B, H, C, 0.0, 0, 0, w.data_ptr(),
               t.data_ptr(), w.data_ptr(), t.data_ptr(), t.data_ptr(), 0, w.data_ptr(), 1 << 40,
               N.stream_ptr())
    torch.cuda.synchronize()


@gpu
def test_registry_ops_match_autograd_function():
    B, H, C, p, seed, off = 5, 128, 3, 0.1, 99, 3
    problem = "single_label_classification"
    ops = _operands(B, H, C, seed=2)
    labels = _labels(problem, B, C)
    x, prm, logits, loss, pred = _run_head(ops, labels, problem, p=p, seed=seed, off=off)
    t, a = _saved(loss)
    loss.backward()
    d = {k: v.to(DEV) for k, v in ops.items()}
    o = torch.ops.dna_amd
    t2, a2 = torch.empty_like(t), torch.empty_like(a)
    lg2, ls2, dl2 = torch.empty_like(logits), torch.empty(1, device=DEV), torch.empty_like(logits)
    pr2 = torch.empty_like(pred)
    o.cls_head_fwd(d["x"], d["wp"], d["bp"], d["wc"], d["bc"], p, seed, off, t2, a2, lg2)
    o.cls_loss(lg2, labels.to(DEV), 1, ls2, dl2, pr2)
    g = [torch.empty(C, H, device=DEV), torch.empty(C, device=DEV), torch.empty(H, H, device=DEV),
         torch.empty(H, device=DEV), torch.empty(B, H, device=DEV)]
    o.cls_head_bwd(dl2, d["x"], t2, a2, d["wp"], d["wc"], p, seed, off, *g, False)
    for u, v in ((t2, t), (a2, a), (lg2, logits), (ls2, loss.reshape(1)), (pr2, pred),
                 (g[0], prm["wc"].grad), (g[1], prm["bc"].grad), (g[2], prm["wp"].grad),
                 (g[3], prm["bp"].grad), (g[4], x.grad)):
        assert torch.equal(u, v.detach())


def test_registry_ops_reject_cpu_tensors():
    from dna_amd import functional as DF, ops
    for name in ("cls_head_fwd", "cls_loss", "cls_head_bwd"):
        assert name in ops.OPS and hasattr(torch.ops.dna_amd, name)
    B, H, C = 2, 64, 3
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(RuntimeError, match="GPU"):
        torch.ops.dna_amd.cls_head_fwd(z(B, H), z(H, H), z(H), z(C, H), z(C), 0.0, 0, 0, z(B, H),
                                       z(B, H), z(B, C))
    with pytest.raises(RuntimeError, match="GPU"):
        torch.ops.dna_amd.cls_loss(z(B, C), z(B).long(), 1, z(1), z(B, C), None)
    with pytest.raises(RuntimeError, match="GPU"):
        torch.ops.dna_amd.cls_head_bwd(z(B, C), z(B, H), z(B, H), z(B, H), z(H, H), z(C, H), 0.0,
                                       0, 0, z(C, H), z(C), z(H, H), z(H), z(B, H), False)
    with pytest.raises(RuntimeError, match="GPU"):
        DF.ClsHead.apply(z(B, H), z(H, H), z(H), z(C, H), z(C), 0.0, 0, 0, None, 1)
