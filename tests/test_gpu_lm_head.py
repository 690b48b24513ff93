"""The small-vocabulary masked-LM head kernels alone (csrc/lm_head.hip) against float64 torch.

Every case runs torch.ops.dna_amd.lm_head_fwd / lm_head_bwd on h [T, D], the tied W [V, D] and
labels [T] (-100 = ignored), twice: plain (upstream 1, dW written) and with an upstream scalar
of 0.25 accumulating into a non-zero dW. dh is handed over full of NaN. The reference is float64
torch on the same inputs (bf16 inputs upcast, W as given).

Tolerance: no fitted constants. For the loss, dh and dW, with err = max |x - fp64|,

    err_new <= 2 * err_old + floor

err_old is the error of the path the head replaces, on the same inputs: hip_linear (fp32 inputs:
the fp32 GEMM; bf16: under bf16 autocast) -> .float() -> F.cross_entropy -> autograd. The factor 2
is the project's margin for "no worse than the path it replaces" (test_gpu_model.py,
test_bf16_train_step_vs_reference_fixture). floor is the worst-case bound of fp32 summation,
u = 2^-24, a length-n sum of terms t_i carrying at most 2 n u sum|t_i| (all evaluated in fp64):

    logit     e_rv = 2 D u sum_d |h_rd W_vd|;  E_r = max_v e_rv
    loss_r    lse is 1-Lipschitz in the logits (max norm): 2 E_r, + 8 u (|lse_r| + |logit_ry|)
              for exp / log / the subtractions;  loss: the mean of these over the kept rows
              + 2 u |loss| (the fp32 roundings of the sum and of the quotient)
    coef_rv   = p_rv - [v = y_r]:  d p_v = p_v (d l_v - sum_w p_w d l_w), so
              eps_rv = 2 E_r p_rv + 8 u max(p_rv, |coef_rv|)
    dh_rd     = s sum_v coef_rv W_vd (s = g / count), a length-V sum:
              |s| (sum_v eps_rv |W_vd| + 2 V u sum_v |coef_rv W_vd|) + 2 u |dh_rd|
              + one output rounding: 2^-9 |dh_rd| in bf16, u |dh_rd| in fp32
    dW_vd     = s sum_r coef_rv h_rd over the K kept rows:
              |s| (sum_r eps_rv |h_rd| + 2 K u sum_r |coef_rv h_rd|) + 2 u |dW_vd|
              + u |dW0_vd + dW_vd| for the add under accumulate
count is exact, ignored rows of dh are exact zeros, two runs agree bit for bit.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24

SHAPES = [(1, 8, 5), (67, 64, 12), (257, 100, 16), (300, 256, 16), (130, 1024, 64), (64, 256, 1)]
PATTERNS = ["none_ignored", "kept15", "first_only", "last_only", "all_ignored"]


def _labels(T, V, pattern, g):
    y = torch.randint(0, V, (T,), generator=g)
    keep = torch.zeros(T, dtype=torch.bool)
    if pattern == "none_ignored":
        keep[:] = True
    elif pattern == "kept15":
        keep = torch.rand(T, generator=g) < 0.15
        keep[T // 2] = True  # never empty, also at T = 1
    elif pattern == "first_only":
        keep[0] = True
    elif pattern == "last_only":
        keep[-1] = True
    return torch.where(keep, y, torch.full_like(y, -100))


def _inputs(T, D, V, pattern, hdt, wdt):
    g = torch.Generator().manual_seed(T * 1009 + D * 31 + V + len(pattern))
    h = (torch.randn(T, D, generator=g) * 1.5).to(hdt)
    w = (torch.randn(V, D, generator=g) * (2.0 / D ** 0.5)).to(wdt)
    dw0 = torch.randn(V, D, generator=g)
    return h, w, _labels(T, V, pattern, g), dw0


def _reference(h, w, labels, up, dw0, out_bf16):
    """float64 values and the fp32 summation floors of the module docstring."""
    h64, w64 = h.double(), w.double()
    T, D = h64.shape
    V = w64.shape[0]
    keep = labels >= 0
    K = int(keep.sum())
    r = {"count": K}
    if K == 0:
        z = torch.zeros
        r.update(loss=0.0, dh=z(T, D, dtype=torch.float64), dw=z(V, D, dtype=torch.float64),
                 f_loss=0.0, f_dh=0.0, f_dw=0.0, f_dw_acc=0.0)
        return r
    hk, yk = h64[keep], labels[keep]
    logits = hk @ w64.t()
    E = (2 * D * U * (hk.abs() @ w64.abs().t())).max(1).values  # [K]
    lse = torch.logsumexp(logits, 1)
    ly = logits.gather(1, yk[:, None])[:, 0]
    loss = float((lse - ly).sum() / K)
    p = torch.softmax(logits, 1)
    coef = p.clone()
    coef[torch.arange(K), yk] -= 1.0
    s = up / K
    dh = torch.zeros(T, D, dtype=torch.float64)
    dh[keep] = s * (coef @ w64)
    dw = s * (coef.t() @ hk)
    eps = 2 * E[:, None] * p + 8 * U * torch.maximum(p, coef.abs())
    r.update(loss=loss, dh=dh, dw=dw)
    r["f_loss"] = float((2 * E + 8 * U * (lse.abs() + ly.abs())).sum() / K + 2 * U * abs(loss))
    f_dh = abs(s) * (eps @ w64.abs() + 2 * V * U * (coef.abs() @ w64.abs())) \
        + (2 * U + (2.0 ** -9 if out_bf16 else U)) * dh[keep].abs()
    r["f_dh"] = float(f_dh.max())
    f_dw = abs(s) * (eps.t() @ hk.abs() + 2 * K * U * (coef.abs().t() @ hk.abs())) + 2 * U * dw.abs()
    r["f_dw"] = float(f_dw.max())
    r["f_dw_acc"] = float((f_dw + U * (dw0.double() + dw).abs()).max())
    return r


_OLD = {}


def _old_path(key, h, w, labels, up):
    """The path the head replaces, once per input set: (loss, dh, dW) for upstream `up`."""
    k = key + (up,)
    if k not in _OLD:
        from dna_amd.hyena import hip_linear
        hd = h.to(DEV).contiguous().requires_grad_(True)
        wd = w.to(DEV).float().contiguous().requires_grad_(True)  # a bf16 W upcasts exactly
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=h.dtype == torch.bfloat16):
            logits = hip_linear(hd, wd)
        n = max(int((labels >= 0).sum()), 1)
        loss = F.cross_entropy(logits.float(), labels.to(DEV), ignore_index=-100,
                               reduction="sum") / n
        (loss * up).backward()
        _OLD[k] = (float(loss.detach()), hd.grad.double().cpu(), wd.grad.double().cpu())
    return _OLD[k]


def _layout(t, layout, fill=float("nan")):
    """A [T, D] device tensor holding t in the given layout (+ the buffer it lives in)."""
    T, D = t.shape
    if layout == "contiguous":
        buf = t.to(DEV).contiguous()
        return buf, buf
    if layout == "strided":  # a column slice of a wider tensor: row stride D + 16
        buf = torch.full((T, D + 16), fill, dtype=t.dtype, device=DEV)
        v = buf[:, :D]
    else:  # "offset": the base pointer one element off every vector alignment
        buf = torch.full((T * D + 1,), fill, dtype=t.dtype, device=DEV)
        v = buf[1:].view(T, D)
    v.copy_(t)
    return v, buf


def _run(h, w, labels, layout, up=None, dw0=None, denom=0.0):
    """fwd + bwd through the registered ops -> dict of host tensors."""
    from dna_amd import ops  # noqa: F401  (registers torch.ops.dna_amd.*)
    o = torch.ops.dna_amd
    T, D = h.shape
    V = w.shape[0]
    hv, _ = _layout(h, layout, fill=0.0)
    wd, ld = w.to(DEV).contiguous(), labels.to(DEV)
    loss = torch.full((2,), float("nan"), device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    coef = torch.zeros(T, V, device=DEV)
    o.lm_head_fwd(hv, wd, ld, denom, loss, count, coef)
    dhv, dhbuf = _layout(torch.full((T, D), float("nan"), dtype=h.dtype), layout)
    dw = torch.full((V, D), float("nan"), device=DEV) if dw0 is None else dw0.to(DEV).clone()
    upt = None if up is None else torch.tensor([up], device=DEV)
    o.lm_head_bwd(coef, hv, wd, ld, count, upt, denom, dhv, dw, dw0 is not None)
    torch.cuda.synchronize()
    return {"loss_sum": loss[0].cpu(), "loss": loss[1].cpu(), "count": int(count.cpu()),
            "coef": coef.cpu(), "dh": dhv.cpu(), "dhbuf": dhbuf.cpu(), "dw": dw.cpu()}


def _check(T, D, V, pattern, hdt, wdt, layout):
    h, w, labels, dw0 = _inputs(T, D, V, pattern, hdt, wdt)
    key = (T, D, V, pattern, hdt, wdt)
    keep = labels >= 0
    bf = hdt == torch.bfloat16
    for up, acc in ((None, None), (0.25, dw0)):
        g = 1.0 if up is None else up
        ref = _reference(h, w, labels, g, dw0, bf)
        got = _run(h, w, labels, layout, up=up, dw0=acc)
        again = _run(h, w, labels, layout, up=up, dw0=acc)
        for k in ("loss_sum", "loss", "dh", "dw"):
            assert torch.equal(got[k], again[k]), f"{k} differs between two runs"
        assert torch.equal(got["coef"][keep], again["coef"][keep])
        assert got["count"] == ref["count"] == again["count"]
        dh = got["dh"].double()
        assert torch.isfinite(dh).all(), "dh has elements the kernel did not write"
        assert (dh[~keep] == 0).all(), "ignored rows of dh must be exact zeros"
        if layout == "strided":  # nothing outside the D columns was touched
            assert torch.isnan(got["dhbuf"][:, D:]).all()
        if layout == "offset":
            assert torch.isnan(got["dhbuf"][0])
        if ref["count"] == 0:
            assert float(got["loss"]) == 0.0 and float(got["loss_sum"]) == 0.0
            assert (dh == 0).all()
            if acc is None:
                assert (got["dw"] == 0).all()
            else:
                assert torch.equal(got["dw"], dw0), "dW must stay as it was under accumulate"
            continue
        old_loss, old_dh, old_dw = _old_path(key, h, w, labels, g)
        dw_ref = ref["dw"] if acc is None else dw0.double() + ref["dw"]
        old_dw = old_dw if acc is None else (dw0 + old_dw.float()).double()
        errs = {
            "loss": (abs(float(got["loss"]) - ref["loss"]), abs(old_loss - ref["loss"]), ref["f_loss"]),
            "dh": (float((dh - ref["dh"]).abs().max()), float((old_dh - ref["dh"]).abs().max()),
                   ref["f_dh"]),
            "dw": (float((got["dw"].double() - dw_ref).abs().max()),
                   float((old_dw - dw_ref).abs().max()),
                   ref["f_dw"] if acc is None else ref["f_dw_acc"]),
        }
        print(f"lm_head T={T} D={D} V={V} {pattern} h={hdt} w={wdt} {layout} up={g}: " +
              ", ".join(f"{k} new {a:.3e} old {b:.3e} floor {c:.3e}" for k, (a, b, c) in errs.items()))
        for k, (new, old, floor) in errs.items():
            assert new <= 2 * old + floor, (k, new, old, floor)
        # loss_sum / count is the loss
        assert abs(float(got["loss_sum"]) / ref["count"] - ref["loss"]) <= \
            2 * errs["loss"][1] + ref["f_loss"] + 2 * U * abs(ref["loss"])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lm_head_fp32_vs_float64(shape, pattern):
    _check(*shape, pattern, torch.float32, torch.float32, "contiguous")


@pytest.mark.parametrize("pattern", ["kept15", "none_ignored"])
@pytest.mark.parametrize("hdt,wdt", [(torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16),
                                     (torch.float32, torch.bfloat16)],
                         ids=["h_bf16-w_fp32", "h_bf16-w_bf16", "h_fp32-w_bf16"])
def test_lm_head_dtypes_300x256x16(hdt, wdt, pattern):
    _check(300, 256, 16, pattern, hdt, wdt, "contiguous")


@pytest.mark.parametrize("shape", [(130, 1024, 64), (67, 64, 12)], ids=lambda s: "x".join(map(str, s)))
def test_lm_head_bf16_other_shapes(shape):
    _check(*shape, "kept15", torch.bfloat16, torch.bfloat16, "contiguous")


@pytest.mark.parametrize("layout", ["strided", "offset"])
@pytest.mark.parametrize("shape,hdt", [((300, 256, 16), torch.float32), ((300, 256, 16), torch.bfloat16),
                                       ((257, 100, 16), torch.float32), ((130, 1024, 64), torch.bfloat16),
                                       ((1, 8, 5), torch.float32)],
                         ids=["300x256x16-fp32", "300x256x16-bf16", "257x100x16-fp32",
                              "130x1024x64-bf16", "1x8x5-fp32"])
def test_lm_head_layouts(shape, hdt, layout):
    """Row stride > D keeps the vector path (the stride is a vector multiple); a base pointer one
    element off falls back to element accesses (at D = 1024 also out of the register path)."""
    _check(*shape, "kept15", hdt, torch.float32, layout)


def test_lm_head_denominator_argument():
    """denom > 0 replaces count as the divisor of the loss and of both gradients."""
    h, w, labels, _ = _inputs(67, 64, 12, "kept15", torch.float32, torch.float32)
    a = _run(h, w, labels, "contiguous")
    K = a["count"]
    b = _run(h, w, labels, "contiguous", denom=float(2 * K))
    assert b["count"] == K and torch.equal(a["loss_sum"], b["loss_sum"])
    assert float(b["loss"]) == pytest.approx(float(a["loss"]) / 2, rel=1e-6)
    torch.testing.assert_close(b["dh"], a["dh"] / 2, rtol=1e-6, atol=0)
    torch.testing.assert_close(b["dw"], a["dw"] / 2, rtol=1e-6, atol=1e-12)


def test_masked_lm_head_autograd_matches_the_ops():
    """functional.masked_lm_head: the autograd Function gives the ops' numbers (upstream 0.25 as
    a device scalar through loss * 0.25), reads a strided view in place, returns count on the
    device, and with nothing kept gives loss 0 and zero gradients."""
    from dna_amd import functional as DF
    h, w, labels, _ = _inputs(300, 256, 16, "kept15", torch.bfloat16, torch.float32)
    want = _run(h, w, labels, "contiguous", up=0.25)
    wide = torch.zeros(300, 272, dtype=torch.bfloat16, device=DEV)
    wide[:, :256] = h.to(DEV)
    hv = wide[:, :256].detach().requires_grad_(True)
    wp = torch.nn.Parameter(w.to(DEV))
    loss, count = DF.masked_lm_head(hv.view(3, 100, 256), wp, labels.to(DEV).view(3, 100))
    assert type(loss.grad_fn).__name__ == "MaskedLMHeadBackward"
    assert count.is_cuda and count.dtype == torch.int64 and int(count) == want["count"]
    (loss * 0.25).backward()
    assert torch.equal(loss.detach().cpu(), want["loss"])
    assert torch.equal(hv.grad.cpu(), want["dh"]) and hv.grad.dtype == torch.bfloat16
    assert torch.equal(wp.grad.cpu(), want["dw"])
    hv.grad = wp.grad = None
    loss, count = DF.masked_lm_head(hv, wp, torch.full((300,), -100, device=DEV))
    loss.backward()
    assert float(loss) == 0.0 and int(count) == 0
    assert (hv.grad == 0).all() and (wp.grad == 0).all()


def test_lm_head_argument_errors():
    from dna_amd import functional as DF
    from dna_amd import ops  # noqa: F401
    o = torch.ops.dna_amd
    h = torch.zeros(4, 8, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="V <= 64"):
        DF.masked_lm_head(h, torch.zeros(65, 8, device=DEV), lab)
    with pytest.raises(RuntimeError, match="GPU only"):
        DF.masked_lm_head(h.cpu(), torch.zeros(5, 8), lab.cpu())
    with pytest.raises(TypeError, match="int64"):
        DF.masked_lm_head(h, torch.zeros(5, 8, device=DEV), lab.int())
    with pytest.raises(RuntimeError, match="unit column stride"):
        o.lm_head_fwd(torch.zeros(8, 4, device=DEV).t(), torch.zeros(5, 8, device=DEV), lab, 0.0,
                      torch.zeros(2, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), None)
