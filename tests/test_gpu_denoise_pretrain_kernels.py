"""The two kernels denoise_cnn pretraining adds, alone, against float64 torch.

Biased small-vocabulary head (csrc/lm_head.hip, dna_lm_head_bias_fwd / _bwd): h [T, D], an untied
W [V, D], bias [V] fp32, labels [T] (-100 = ignored). T 257; D 64 (vector path), 200 (vector path,
a ragged last 64-lane chunk), 67 (element path); V 5 and 64; h in fp32, in bf16 and as a strided
view; about 15 % of the rows kept. Every case runs twice (bit-identical) in two modes: plain
(upstream 1, dW and db written over NaN) and accumulate (an upstream scalar of 0.25, added into
non-zero dW and db). The bound is tests/test_gpu_lm_head.py's, for the loss, dh, dW and db:

    err_new <= 2 * err_old + floor

err_old: hip_linear (with the bias) -> .float() -> F.cross_entropy -> autograd on the same inputs.
floor: that file's fp32 summation bounds with the bias as one more term of the logit's sum,

    e_rv = 2 (D + 1) u (sum_d |h_rd W_vd| + |b_v|)

and db as dW's bound with h = 1: |s| (sum_r eps_rv + 2 K u sum_r |coef_rv|) + 2 u |db_v|
(+ u |db0_v + db_v| under accumulate).

One-hot input layer with ReLU (csrc/dilated_conv.hip, dna_onehot_conv_* with DNA_ACT_RELU):
B 2, L 37, C 64, KW 9, complement on and off, against float64 conv1d + relu under the bounds
tests/test_gpu_dilated_conv.py applies to the GELU layer (an exact pass on an integer table; real
weights: the forward within 1e-6 (1 + |z|) + 2^-22 |out| + z's summation error, the gradients
within 4x torch's own fp32 error plus that file's slack). ReLU's derivative is a step, which that
slack (it rests on |gelu''| < 1.2) does not cover: where |z| is within its summation error of 0
the derivative may differ from the truth's by 1, so |dout| at those positions is added.
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_lm_head import U, _labels, _layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 257


# ----------------------------------------------------------------------------------- the head
def _inputs(D, V, hdt, pattern="kept15"):
    g = torch.Generator().manual_seed(D * 31 + V)
    h = (torch.randn(T, D, generator=g) * 1.5).to(hdt)
    w = torch.randn(V, D, generator=g) * (2.0 / D ** 0.5)
    b = torch.randn(V, generator=g)
    dw0, db0 = torch.randn(V, D, generator=g), torch.randn(V, generator=g)
    return h, w, b, _labels(T, V, pattern, g), dw0, db0


def _reference(h, w, b, labels, up, dw0, db0, out_bf16):
    """float64 values and the fp32 summation floors of the module docstring."""
    h64, w64, b64 = h.double(), w.double(), b.double()
    D, V = h64.shape[1], w64.shape[0]
    keep = labels >= 0
    K = int(keep.sum())
    hk, yk = h64[keep], labels[keep]
    logits = hk @ w64.t() + b64
    E = (2 * (D + 1) * U * (hk.abs() @ w64.abs().t() + b64.abs())).max(1).values  # [K]
    lse = torch.logsumexp(logits, 1)
    ly = logits.gather(1, yk[:, None])[:, 0]
    loss = float((lse - ly).sum() / K)
    p = torch.softmax(logits, 1)
    coef = p.clone()
    coef[torch.arange(K), yk] -= 1.0
    s = up / K
    dh = torch.zeros(T, D, dtype=torch.float64)
    dh[keep] = s * (coef @ w64)
    dw, db = s * (coef.t() @ hk), s * coef.sum(0)
    eps = 2 * E[:, None] * p + 8 * U * torch.maximum(p, coef.abs())
    r = {"count": K, "loss": loss, "dh": dh, "dw": dw, "db": db}
    r["f_loss"] = float((2 * E + 8 * U * (lse.abs() + ly.abs())).sum() / K + 2 * U * abs(loss))
    f_dh = abs(s) * (eps @ w64.abs() + 2 * V * U * (coef.abs() @ w64.abs())) \
        + (2 * U + (2.0 ** -9 if out_bf16 else U)) * dh[keep].abs()
    r["f_dh"] = float(f_dh.max())
    f_dw = abs(s) * (eps.t() @ hk.abs() + 2 * K * U * (coef.abs().t() @ hk.abs())) + 2 * U * dw.abs()
    f_db = abs(s) * (eps.sum(0) + 2 * K * U * coef.abs().sum(0)) + 2 * U * db.abs()
    r["f_dw"], r["f_db"] = float(f_dw.max()), float(f_db.max())
    r["f_dw_acc"] = float((f_dw + U * (dw0.double() + dw).abs()).max())
    r["f_db_acc"] = float((f_db + U * (db0.double() + db).abs()).max())
    return r


def _old_path(h, w, b, labels, up):
    """The path the head replaces: (loss, dh, dW, db) for upstream `up`."""
    from dna_amd.hyena import hip_linear
    hd = h.to(DEV).contiguous().requires_grad_(True)
    wd, bd = (t.to(DEV).contiguous().requires_grad_(True) for t in (w, b))
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=h.dtype == torch.bfloat16):
        logits = hip_linear(hd, wd, bd)
    n = max(int((labels >= 0).sum()), 1)
    loss = F.cross_entropy(logits.float(), labels.to(DEV), ignore_index=-100, reduction="sum") / n
    (loss * up).backward()
    return (float(loss.detach()), hd.grad.double().cpu(), wd.grad.double().cpu(),
            bd.grad.double().cpu())


def _run(h, w, b, labels, layout="contiguous", up=None, dw0=None, db0=None, entry="bias"):
    """fwd + bwd through the C ABI -> dict of host tensors. entry "bias": dna_lm_head_bias_*
    (b None: a null bias pointer and no dbias); "plain": dna_lm_head_* (no bias argument)."""
    from dna_amd import _native as N
    D, V = h.shape[1], w.shape[0]
    dt = N.BF16 if h.dtype == torch.bfloat16 else N.F32
    ptr = lambda t: None if t is None else t.data_ptr()
    hv, _ = _layout(h, layout, fill=0.0)
    hs = hv.stride(0)
    wd, ld = w.to(DEV).contiguous(), labels.to(DEV)
    bd = None if b is None else b.to(DEV).contiguous()
    loss = torch.full((2,), float("nan"), device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    coef = torch.zeros(T, V, device=DEV)
    ws = torch.empty(max(N.lib().dna_lm_head_fwd_workspace(T) // 8, 2), device=DEV,
                     dtype=torch.float64)
    head = (hv.data_ptr(), hs, dt, wd.data_ptr(), N.F32)
    tail = (ld.data_ptr(), T, D, V, 0.0, loss.data_ptr(), count.data_ptr(), loss.data_ptr() + 4,
            coef.data_ptr(), ws.data_ptr(), ws.numel() * 8, N.stream_ptr())
    if entry == "bias":
        N.call("dna_lm_head_bias_fwd", *head, ptr(bd), *tail)
    else:
        N.call("dna_lm_head_fwd", *head, *tail)
    dhv, dhbuf = _layout(torch.full((T, D), float("nan"), dtype=h.dtype), layout)
    acc = dw0 is not None
    dw = dw0.to(DEV).clone() if acc else torch.full((V, D), float("nan"), device=DEV)
    db = None if b is None else (db0.to(DEV).clone() if acc
                                 else torch.full((V,), float("nan"), device=DEV))
    upt = None if up is None else torch.tensor([up], device=DEV)
    nws = (N.lib().dna_lm_head_bias_bwd_workspace if entry == "bias"
           else N.lib().dna_lm_head_bwd_workspace)(T, D, V)
    ws2 = torch.empty(max(nws // 4, 4), device=DEV, dtype=torch.float32)
    head = (coef.data_ptr(), hv.data_ptr(), hs, dt, wd.data_ptr(), N.F32, ld.data_ptr(),
            count.data_ptr(), ptr(upt), 0.0, T, D, V, dhv.data_ptr(), dhv.stride(0), dw.data_ptr())
    tail = (int(acc), ws2.data_ptr(), ws2.numel() * 4, N.stream_ptr())
    if entry == "bias":
        N.call("dna_lm_head_bias_bwd", *head, ptr(db), *tail)
    else:
        N.call("dna_lm_head_bwd", *head, *tail)
    torch.cuda.synchronize()
    return {"loss_sum": loss[0].cpu(), "loss": loss[1].cpu(), "count": int(count.cpu()),
            "coef": coef.cpu(), "dh": dhv.cpu(), "dhbuf": dhbuf.cpu(), "dw": dw.cpu(),
            "db": None if db is None else db.cpu()}


@pytest.mark.parametrize("kind", ["fp32", "bf16", "strided"])
@pytest.mark.parametrize("V", [5, 64])
@pytest.mark.parametrize("D", [64, 200, 67])
def test_biased_head_vs_float64(D, V, kind):
    hdt = torch.bfloat16 if kind == "bf16" else torch.float32
    layout = "strided" if kind == "strided" else "contiguous"
    h, w, b, labels, dw0, db0 = _inputs(D, V, hdt)
    keep = labels >= 0
    assert 20 <= int(keep.sum()) <= 60  # about 15 % of 257
    for up, acc in ((None, False), (0.25, True)):
        g = 1.0 if up is None else up
        ref = _reference(h, w, b, labels, g, dw0, db0, hdt == torch.bfloat16)
        kw = dict(up=up, dw0=dw0 if acc else None, db0=db0 if acc else None)
        got = _run(h, w, b, labels, layout, **kw)
        again = _run(h, w, b, labels, layout, **kw)
        for k in ("loss_sum", "loss", "dh", "dw", "db"):
            assert torch.equal(got[k], again[k]), f"{k} differs between two runs"
        assert torch.equal(got["coef"][keep], again["coef"][keep])
        assert got["count"] == ref["count"]
        dh = got["dh"].double()
        assert torch.isfinite(dh).all(), "dh has elements the kernel did not write"
        assert (dh[~keep] == 0).all(), "ignored rows of dh must be exact zeros"
        assert torch.isfinite(got["dw"]).all() and torch.isfinite(got["db"]).all()
        if layout == "strided":  # nothing outside the D columns was touched
            assert torch.isnan(got["dhbuf"][:, D:]).all()
        old_loss, old_dh, old_dw, old_db = _old_path(h, w, b, labels, g)
        dw_ref, db_ref = ref["dw"], ref["db"]
        if acc:
            dw_ref, db_ref = dw0.double() + dw_ref, db0.double() + db_ref
            old_dw, old_db = (dw0 + old_dw.float()).double(), (db0 + old_db.float()).double()
        errs = {
            "loss": (abs(float(got["loss"]) - ref["loss"]), abs(old_loss - ref["loss"]), ref["f_loss"]),
            "dh": (float((dh - ref["dh"]).abs().max()), float((old_dh - ref["dh"]).abs().max()),
                   ref["f_dh"]),
            "dw": (float((got["dw"].double() - dw_ref).abs().max()),
                   float((old_dw - dw_ref).abs().max()), ref["f_dw_acc" if acc else "f_dw"]),
            "db": (float((got["db"].double() - db_ref).abs().max()),
                   float((old_db - db_ref).abs().max()), ref["f_db_acc" if acc else "f_db"]),
        }
        print(f"lm_head_bias D={D} V={V} {kind} up={g}: " +
              ", ".join(f"{k} new {a:.3e} old {o:.3e} floor {c:.3e}" for k, (a, o, c) in errs.items()))
        for k, (new, old, floor) in errs.items():
            assert new <= 2 * old + floor, (k, new, old, floor)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "strided"])
@pytest.mark.parametrize("D,V", [(64, 5), (200, 64), (67, 5)])
def test_null_bias_is_the_existing_entry_point_bit_for_bit(D, V, kind):
    hdt = torch.bfloat16 if kind == "bf16" else torch.float32
    layout = "strided" if kind == "strided" else "contiguous"
    h, w, _, labels, dw0, _ = _inputs(D, V, hdt)
    for kw in (dict(), dict(up=0.25, dw0=dw0)):
        a = _run(h, w, None, labels, layout, entry="bias", **kw)
        b = _run(h, w, None, labels, layout, entry="plain", **kw)
        assert a["count"] == b["count"] > 0
        for k in ("loss_sum", "loss", "coef", "dh", "dw"):
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("D,V", [(64, 5), (67, 64)])
def test_no_kept_row_gives_zero_everywhere(D, V):
    h, w, b, _, dw0, db0 = _inputs(D, V, torch.float32)
    labels = torch.full((T,), -100, dtype=torch.int64)
    got = _run(h, w, b, labels)
    assert got["count"] == 0 and float(got["loss"]) == 0.0 and float(got["loss_sum"]) == 0.0
    assert (got["dh"] == 0).all() and (got["dw"] == 0).all() and (got["db"] == 0).all()
    got = _run(h, w, b, labels, up=0.25, dw0=dw0, db0=db0)
    assert (got["dh"] == 0).all()
    assert torch.equal(got["dw"], dw0) and torch.equal(got["db"], db0)  # unchanged under accumulate


def test_masked_lm_head_with_a_bias_gives_the_kernels_numbers():
    """functional.masked_lm_head(bias=): the C ABI's numbers through autograd (upstream 0.25 as a
    device scalar), a strided view read in place, the bias gradient next to dW."""
    from dna_amd import functional as DF
    D, V = 200, 5
    h, w, b, labels, _, _ = _inputs(D, V, torch.bfloat16)
    want = _run(h, w, b, labels, up=0.25)
    wide = torch.zeros(T, D + 16, dtype=torch.bfloat16, device=DEV)
    wide[:, :D] = h.to(DEV)
    hv = wide[:, :D].detach().requires_grad_(True)
    wp, bp = torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(b.to(DEV))
    loss, count = DF.masked_lm_head(hv, wp, labels.to(DEV), bias=bp)
    assert type(loss.grad_fn).__name__ == "MaskedLMHeadBackward" and int(count) == want["count"]
    (loss * 0.25).backward()
    assert torch.equal(loss.detach().cpu(), want["loss"])
    assert torch.equal(hv.grad.cpu(), want["dh"]) and hv.grad.dtype == torch.bfloat16
    assert torch.equal(wp.grad.cpu(), want["dw"]) and torch.equal(bp.grad.cpu(), want["db"])
    with pytest.raises(ValueError, match="no bias"):
        DF.masked_lm_head(torch.zeros(T, 2 * D, device=DEV), wp, labels.to(DEV),
                          complement_map=torch.arange(V, device=DEV), bias=bp)
    # without a bias the existing path is taken, unchanged
    plain = _run(h, w, None, labels, entry="plain")
    loss, _ = DF.masked_lm_head(hv, wp, labels.to(DEV))
    assert torch.equal(loss.detach().cpu(), plain["loss"])


# --------------------------------------------------------------------------- the one-hot layer
def _onehot_truth(ids, w, b, dout, complement, dtype=torch.float64):
    V, KW = w.shape[1], w.shape[2]
    if complement:
        ids = torch.where(ids == 4, ids, 3 - ids)
    w, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (w, b))
    z = F.conv1d(F.one_hot(ids, V).to(dtype).transpose(1, 2), w, b, padding=(KW - 1) // 2)
    z = z.transpose(1, 2)
    out = F.relu(z)
    out.backward(dout.to(dtype))
    return out.detach(), w.grad, b.grad, z.detach()


@pytest.mark.parametrize("complement", [False, True], ids=["ids", "complement"])
def test_onehot_input_layer_relu(complement):
    from dna_amd import functional as DF
    from dna_amd import ops  # noqa: F401  (registers torch.ops.dna_amd.*)
    O = torch.ops.dna_amd
    B, L, C, V, KW = 2, 37, 64, 5, 9
    g0 = torch.Generator().manual_seed(6)
    ids = torch.randint(0, 4, (B, L), generator=g0)
    ids[0, :6] = 4
    ids[1, 15:19] = 4
    ids[1, -3:] = 4
    # exact: an integer table gives integer z, so ReLU and its gradient are exact, bit for bit;
    # z = 0 occurs and takes derivative 0
    w = torch.randint(-3, 4, (C, V, KW), generator=g0).float()
    b = torch.randint(-2, 3, (C,), generator=g0).float()
    dout = torch.randint(-1, 2, (B, L, C), generator=g0).float()
    out, dw, db = (torch.empty(s, device=DEV) for s in ((B, L, C), (C, V, KW), (C,)))
    O.onehot_conv_fwd(ids.to(DEV), w.to(DEV), b.to(DEV), complement, "relu", out)
    O.onehot_conv_bwd(ids.to(DEV), w.to(DEV), b.to(DEV), dout.to(DEV), complement, "relu", dw, db,
                      False)
    t_out, t_dw, t_db, z = _onehot_truth(ids, w, b, dout, complement)
    assert int((z == 0).sum()) > 0 and int((z < 0).sum()) > 0 and int((z > 0).sum()) > 0
    assert torch.equal(out.cpu().double(), t_out)
    assert torch.equal(dw.cpu().double(), t_dw) and torch.equal(db.cpu().double(), t_db)
    # real weights. z is an fp32 sum of KW + 1 terms: at most (KW + 1) 2^-24 of the sum of their
    # magnitudes off (the GELU test's zerr and forward bound; relu is 1-Lipschitz)
    w, b = torch.randn(C, V, KW, generator=g0) / 3, torch.randn(C, generator=g0)
    dout = torch.randn(B, L, C, generator=g0)
    O.onehot_conv_fwd(ids.to(DEV), w.to(DEV), b.to(DEV), complement, "relu", out)
    O.onehot_conv_bwd(ids.to(DEV), w.to(DEV), b.to(DEV), dout.to(DEV), complement, "relu", dw, db,
                      False)
    t_out, t_dw, t_db, z = _onehot_truth(ids, w, b, dout, complement)
    c_out, c_dw, c_db, _ = _onehot_truth(ids, w, b, dout, complement, torch.float32)
    zerr = (KW + 1) * 2.0 ** -24 * float(KW * w.abs().max() + b.abs().max())
    bound = 1e-6 * (1 + z.abs()) + 2.0 ** -22 * t_out.abs() + zerr
    assert float(((out.cpu().double() - t_out).abs() - bound).max()) <= 0
    assert (out.cpu()[z < -zerr] == 0).all()
    # the GELU test's slack, plus |dout| wherever |z| <= zerr (the step may fall on either side)
    slack = ((1e-6 * float((1 + z.abs()).max()) + 1.2 * zerr)
             * float(dout.abs().sum(dim=(0, 1)).max()))
    near = (z.abs() <= zerr).double()
    slack += float((near * dout.double().abs()).sum(dim=(0, 1)).max())
    for got, cpu, t in ((dw, c_dw, t_dw), (db, c_db, t_db)):
        ours, torchs = float((got.cpu().double() - t).abs().max()), float((cpu.double() - t).abs().max())
        print(f"onehot relu complement={complement}: ours {ours:.3e} torch fp32 {torchs:.3e} "
              f"slack {slack:.3e}")
        assert ours <= 4 * torchs + slack, (ours, torchs, slack)
    # accumulate adds to what is there
    dw2, db2 = dw.clone(), db.clone()
    O.onehot_conv_bwd(ids.to(DEV), w.to(DEV), b.to(DEV), dout.to(DEV), complement, "relu", dw2, db2,
                      True)
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)
    # functional.onehot_conv(act=): the same numbers through autograd; GELU stays the default
    wp, bp = torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(b.to(DEV))
    y = DF.onehot_conv(ids.to(DEV), wp, bp, complement, act=DF.N.ACT_RELU)
    y.backward(dout.to(DEV))
    assert torch.equal(y.detach(), out) and torch.equal(wp.grad, dw) and torch.equal(bp.grad, db)
    O.onehot_conv_fwd(ids.to(DEV), w.to(DEV), b.to(DEV), complement, "gelu", out)
    assert torch.equal(DF.onehot_conv(ids.to(DEV), wp, bp, complement).detach(), out)
