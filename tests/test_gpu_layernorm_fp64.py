"""LayerNorm family (csrc/layernorm.hip) against torch fp64 autograd, on every dispatch path.

Reference: fp64 autograd of LN(dropout(act(x + bias)) + residual) * gamma + beta on the same input
values (bf16 inputs upcast exactly), the output gradient dy (fp32) + dy_bf16 (upcast) summed as
the kernels sum it. The dropout mask is read back from a separate dna_ln_fwd call on x = 1
(`_keep_mask`), so forward, both backward paths and the reference are tied to one mask.

Metric: err = max|a - ref64| / max(max|ref64|, 1e-30) per output. The same graph in fp32 torch on
the device gives err_torch32. fp32 outputs must satisfy err_kernel <= K * err_torch32; bf16
outputs |a - ref64| <= 2^-8 |ref64| + K * err_torch32 * max|ref64| elementwise (one bf16 ulp: a
value at fp32 noise level may flip the rounding). No additive floor is used.

K: the smallest power of two that is at least twice the largest err_kernel / err_torch32 seen on
the MI355X over every well-conditioned case (gamma = 1 +- 0.1) of this file, and never more than
8: a ratio above 4 is a finding to explain or a bug to fix, not something to absorb. Measured table (largest ratio per entry point and output over all cases of (a), (b), (d)):

    entry point                 y     dx    dres  dgamma dbeta dbias / dtype_row
    dna_ln_fwd                  1.27
    dna_ln_bwd                        1.87  2.30  2.06   2.25  2.07
    dna_ln_bwd_from_y                 1.87  2.30  1.95   2.25  2.25
    dna_ln_bwd_from_y_acc             1.20        2.01   2.47  1.57
    dna_add_ln_fwd / _bwd       1.10  1.00  1.00  2.19   2.12
    dna_rms_fwd / _bwd          1.17  1.28        1.18
    dna_embed_ln_fwd/_bwd_rows  1.85  1.65 (drows) 2.13  1.90  1.44
    FlatParams direct (d)                         1.19   1.46  1.00
    FlatParams, zero gamma (d)                    1.40   1.46  1.22

(err_torch32 itself is at most 2.9e-7, and 0 once -- dbeta of three rows of bf16 gradients, where
the kernel's error is 0 too.) Largest ratio 2.47 (dbeta of the accumulating
entry point at 4099 x 256): twice that is 4.94, so K = 8. Every ratio is below 4. The cases (c)
measure, on the path FusedLayerNorm takes for them, at most y 1.00, dbias 1.30, dres 1.19,
dgamma 2.55 (t = 1e-1, the one t whose |beta / gamma| = 10 still takes the from-y kernel;
2.27 for every other t), dbeta 1.44; every bf16 output is inside its elementwise bound.

The same K holds for the ill-conditioned cases (c): FusedLayerNorm takes the from-y backward only
where functional.ln_from_y_ok(gamma, beta) says that it is as accurate as the recompute path.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = 8
SEED, OFF = 0x5DEECE66D, 1234567  # non-zero seed, offset % 4 == 3
_p = lambda t: None if t is None else t.data_ptr()


def _big(cols):
    """Rows past which bwd_kernel's grid-stride loop takes a second row: 4 * bwd_blocks()."""
    return 4096 if cols < 768 else 2048


def _err(a, ref):
    return (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


class _Report:
    """Collects (output, err_kernel, err_torch32), prints every figure, then asserts the bounds."""

    def __init__(self, tag):
        self.tag, self.rows, self.bad = tag, [], []

    def add(self, name, a, r64, r32):
        assert a.shape == r64.shape, (name, a.shape, r64.shape)
        et = _err(r32, r64)
        ek = _err(a, r64)
        if a.dtype == torch.bfloat16:
            d = (a.double() - r64).abs()
            lim = 2.0 ** -8 * r64.abs() + K * et * r64.abs().max()
            ok = bool((d <= lim).all().item())  # NaN compares false
            print(f"BF16  {self.tag} {name}: err {ek:.3e} torch32 {et:.3e} "
                  f"worst excess {(d - lim).max().item():.3e}")
        else:
            ratio = ek / et if et > 0 else (0.0 if ek == 0 else float("inf"))
            ok = ek <= K * et
            print(f"RATIO {self.tag} {name}: kernel {ek:.3e} torch32 {et:.3e} ratio {ratio:.2f}")
        if not ok:
            self.bad.append((name, ek, et))

    def finish(self):
        assert not self.bad, (self.tag, self.bad)


_MASKS = {}


def _keep_mask(rows, cols, p, seed=SEED, off=OFF):
    """The dropout keep mask of (seed, off, row, col, cols) from dna_ln_fwd on x = 1: kept
    elements (1 / (1 - p)) lie above the row mean, dropped ones (0) below. In a row with nothing
    dropped every value is the same (the fp32 row mean may miss it by an ulp, so `all equal`
    rather than `all zero` is tested): that row is all-kept. Shared, never modified."""
    if p == 0.0:
        return None
    key = (rows, cols, p, seed, off)
    if key not in _MASKS:
        from dna_amd import _native as N
        x = torch.ones(rows, cols, device=DEV)
        gm, bt = torch.ones(cols, device=DEV), torch.zeros(cols, device=DEV)
        y = torch.full((rows, cols), float("nan"), device=DEV)
        mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        N.call("dna_ln_fwd", x.data_ptr(), N.F32, None, 0, p, seed, off, None, gm.data_ptr(),
               bt.data_ptr(), rows, cols, 1e-5, y.data_ptr(), None, mean.data_ptr(),
               rstd.data_ptr(), N.stream_ptr())
        assert torch.isfinite(y).all()
        same = (y.max(1).values == y.min(1).values)[:, None]
        keep = (y > 0) | same
        rate = keep.double().mean().item()
        sigma = (0.09 / (rows * cols)) ** 0.5
        assert abs(rate - (1 - p)) <= 5 * sigma, (rate, sigma)
        _MASKS[key] = keep
    return _MASKS[key]


def _kscale(p):
    return 1.0 / (1.0 - float(np.float32(p)))


def _gsum(dt, dy, dyb):
    """dy (fp32) + dy_bf16 upcast, summed in `dt` (fp32: as the kernels do it)."""
    parts = [t.to(dt) for t in (dy, dyb) if t is not None]
    return parts[0] if len(parts) == 1 else parts[0] + parts[1]


def _ln_graph(dt, x, bias, res, gm, bt, eps, act, keep, p, gouts):
    """LN(dropout(act(x + bias)) + residual) * gamma + beta in `dt` with torch autograd ->
    (y, [{dx, dbias, dres, dgamma, dbeta} per output gradient (dy, dy_bf16) of gouts])."""
    L = {k: (None if v is None else v.detach().to(dt).requires_grad_(True))
         for k, v in dict(dx=x, dbias=bias, dres=res, dgamma=gm, dbeta=bt).items()}
    u = L["dx"] if bias is None else L["dx"] + L["dbias"]
    if act == 1:
        u = F.gelu(u)
    if keep is not None:
        u = u * (keep.to(dt) * _kscale(p))
    if res is not None:
        u = u + L["dres"]
    y = F.layer_norm(u, (x.shape[1],), L["dgamma"], L["dbeta"], eps)
    names = [k for k, v in L.items() if v is not None]
    grads = []
    for dy, dyb in gouts:
        g = torch.autograd.grad(y, [L[k] for k in names], _gsum(dt, dy, dyb), retain_graph=True)
        grads.append(dict(zip(names, g)))
    return y.detach(), grads


def _rand_gouts(n, shape, gsel, g):
    out = []
    for _ in range(n):
        dy = torch.randn(*shape, device=DEV, generator=g) if gsel in ("f32", "both") else None
        dyb = (torch.randn(*shape, device=DEV, generator=g).bfloat16()
               if gsel in ("bf16", "both") else None)
        out.append((dy, dyb))
    return out


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


# ------------------------------------------------------------------ (a) raw entry points
def _raw_cases():
    cases = []
    both = (torch.bfloat16, torch.float32)
    for cols in (64, 192, 256, 1024):  # the widths without a rows sweep
        for xdt in both:
            cases.append((333, cols, xdt, True, True, "both", 0.0, 0, True))
            cases.append((_big(cols) + 3, cols, xdt, True, True, "both", 0.1, 0, True))
    for cols in (128, 512, 768):
        for xdt in both:
            for rows in (1, 3, 5, 449, _big(cols) + 3):
                cases.append((rows, cols, xdt, True, True, "both", 0.1, 0, True))
        # bias / residual / gradient inputs / dropout, one at a time and together
        opts = [(False, True, "both", 0.0), (True, False, "both", 0.1), (True, True, "f32", 0.1),
                (True, True, "bf16", 0.0), (False, False, "bf16", 0.1), (True, True, "f32", 0.0)]
        for i, (ub, ur, gsel, p) in enumerate(opts):
            cases.append((333, cols, both[i % 2], ub, ur, gsel, p, 0, True))
    for xdt in both:  # gelu: recompute-from-x backward only
        cases.append((333, 768, xdt, True, False, "both", 0.0, 1, True))
    cases.append((333, 128, torch.bfloat16, True, True, "both", 0.1, 1, True))
    cases.append((449, 512, torch.bfloat16, True, True, "both", 0.1, 0, False))  # dresidual NULL
    return cases


def _case_id(c):
    rows, cols, xdt, ub, ur, gsel, p, act, dres = c
    return (f"{rows}x{cols}-{'bf16' if xdt == torch.bfloat16 else 'f32'}-b{int(ub)}r{int(ur)}-"
            f"g{gsel}-p{p}-a{act}-d{int(dres)}")


@pytest.mark.parametrize("case", _raw_cases(), ids=_case_id)
def test_ln_raw_entry_points_vs_fp64(case):
    """dna_ln_fwd, dna_ln_bwd, dna_ln_bwd_from_y and dna_ln_bwd_from_y_acc on one input set: every
    output against fp64 under the K bound, outputs pre-filled with NaN (overwritten, every element
    written), the zero pattern of dx of both backward paths equal to the dropout mask, and the
    accumulating entry point called twice on top of a random pre-fill."""
    from dna_amd import _native as N
    rows, cols, xdt, use_bias, use_res, gsel, p, act, want_dres = case
    eps = 1e-12
    g = torch.Generator(device=DEV).manual_seed(rows * 131 + cols + int(10 * p) + act)
    x = torch.randn(rows, cols, device=DEV, generator=g).to(xdt)
    bias = 0.1 * torch.randn(cols, device=DEV, generator=g) if use_bias else None
    res = torch.randn(rows, cols, device=DEV, generator=g) if use_res else None
    gm = 1 + 0.1 * torch.randn(cols, device=DEV, generator=g)
    bt = 0.1 * torch.randn(cols, device=DEV, generator=g)
    gouts = _rand_gouts(2, (rows, cols), gsel, g)
    keep = _keep_mask(rows, cols, p)
    y64, g64 = _ln_graph(torch.float64, x, bias, res, gm, bt, eps, act, keep, p, gouts)
    y32, g32 = _ln_graph(torch.float32, x, bias, res, gm, bt, eps, act, keep, p, gouts)
    rep = _Report(_case_id(case))
    st = N.stream_ptr()
    xd = N.BF16 if xdt == torch.bfloat16 else N.F32

    y, yb = _nan(rows, cols), _nan(rows, cols, dtype=torch.bfloat16)
    mean, rstd = _nan(rows), _nan(rows)
    N.call("dna_ln_fwd", x.data_ptr(), xd, _p(bias), act, p, SEED, OFF, _p(res), gm.data_ptr(),
           bt.data_ptr(), rows, cols, eps, y.data_ptr(), yb.data_ptr(), mean.data_ptr(),
           rstd.data_ptr(), st)
    rep.add("fwd.y", y, y64, y32)
    rep.add("fwd.y_bf16", yb, y64, y32)

    nws = N.lib().dna_ln_bwd_workspace(rows, cols)
    ws = torch.empty(max(nws, 16), device=DEV, dtype=torch.uint8)
    dy, dyb = gouts[0]

    def outputs(fill):
        o = dict(dx=fill(rows, cols).to(xdt), dgamma=fill(cols), dbeta=fill(cols))
        o["dres"] = fill(rows, cols) if (use_res and want_dres) else None
        o["dbias"] = fill(cols) if use_bias else None
        return o

    def check(path, o, ref64, ref32):
        for k, v in o.items():
            if v is not None:
                rep.add(f"{path}.{k}", v, ref64[k], ref32[k])
        if keep is not None:
            assert torch.equal(o["dx"] == 0, ~keep), f"{path}: dx zero pattern != dropout mask"

    o = outputs(_nan)
    N.call("dna_ln_bwd", _p(dy), _p(dyb), x.data_ptr(), xd, _p(bias), act, p, SEED, OFF, _p(res),
           gm.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, cols, _p(o["dres"]),
           o["dx"].data_ptr(), o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), _p(o["dbias"]),
           ws.data_ptr(), nws, st)
    check("bwd_x", o, g64[0], g32[0])

    if act == 0:
        def from_y(name, o, dy, dyb):
            N.call(name, _p(dy), _p(dyb), y.data_ptr(), xd, p, SEED, OFF, gm.data_ptr(),
                   bt.data_ptr(), rstd.data_ptr(), rows, cols, _p(o["dres"]), o["dx"].data_ptr(),
                   o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), _p(o["dbias"]), ws.data_ptr(),
                   nws, st)

        oy = outputs(_nan)
        from_y("dna_ln_bwd_from_y", oy, dy, dyb)
        check("bwd_y", oy, g64[0], g32[0])

        # the accumulating entry point: pre-fill + gradient of call 1 + gradient of call 2
        oa = outputs(lambda *s: torch.randn(*s, device=DEV, generator=g))
        pre = {k: oa[k].clone() for k in ("dgamma", "dbeta", "dbias") if oa[k] is not None}
        from_y("dna_ln_bwd_from_y_acc", oa, dy, dyb)
        assert torch.equal(oa["dx"], oy["dx"])  # dx / dresidual are written, not accumulated
        if oa["dres"] is not None:
            assert torch.equal(oa["dres"], oy["dres"])
        from_y("dna_ln_bwd_from_y_acc", oa, *gouts[1])
        for k, v in pre.items():
            rep.add(f"bwd_y_acc.{k}", oa[k], v.double() + g64[0][k] + g64[1][k],
                    v + g32[0][k] + g32[1][k])
        rep.add("bwd_y_acc.dx", oa["dx"], g64[1]["dx"], g32[1]["dx"])
    rep.finish()


# ------------------------------------------------------------------ (b) the other row-loop users
def _norm(dt, s, gm, bt, eps, rms):
    if rms:
        return s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + eps) * gm
    return F.layer_norm(s, (s.shape[1],), gm, bt, eps)


def _add_ln_graph(dt, x, res, gm, bt, eps, rms, ds, gout):
    L = {k: (None if v is None else v.detach().to(dt).requires_grad_(True))
         for k, v in dict(dx=x, dres=res, dgamma=gm, dbeta=None if rms else bt).items()}
    s = L["dx"] if res is None else L["dx"] + L["dres"]
    y = _norm(dt, s, L["dgamma"], L["dbeta"], eps, rms)
    names = [k for k, v in L.items() if v is not None]
    outs, gs = [y], [_gsum(dt, *gout)]
    if ds is not None:
        outs.append(s)
        gs.append(ds.to(dt))
    grads = dict(zip(names, torch.autograd.grad(outs, [L[k] for k in names], gs)))
    return s.detach(), y.detach(), grads


@pytest.mark.parametrize("xdt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rms", [0, 1])
@pytest.mark.parametrize("rows_big", [False, True], ids=["r3", "rbig"])
@pytest.mark.parametrize("cols", [256, 768])
def test_add_ln_vs_fp64(cols, rows_big, rms, xdt):
    """dna_add_ln_fwd / dna_add_ln_bwd (LayerNorm and RMSNorm, with the sum's own gradient) at
    fewer rows than one block's waves and at a second row per wave."""
    from dna_amd import _native as N
    rows = _big(cols) + 3 if rows_big else 3
    eps = 1e-5
    g = torch.Generator(device=DEV).manual_seed(rows + cols + rms)
    x = torch.randn(rows, cols, device=DEV, generator=g).to(xdt)
    res = torch.randn(rows, cols, device=DEV, generator=g)
    gm = 1 + 0.1 * torch.randn(cols, device=DEV, generator=g)
    bt = 0.1 * torch.randn(cols, device=DEV, generator=g)
    ds = torch.randn(rows, cols, device=DEV, generator=g)
    bf = xdt == torch.bfloat16
    gout = _rand_gouts(1, (rows, cols), "bf16" if bf else "f32", g)[0]
    s64, y64, g64 = _add_ln_graph(torch.float64, x, res, gm, bt, eps, rms, ds, gout)
    s32, y32, g32 = _add_ln_graph(torch.float32, x, res, gm, bt, eps, rms, ds, gout)
    rep = _Report(f"add_ln-{rows}x{cols}-rms{rms}-{'bf16' if bf else 'f32'}")
    st = N.stream_ptr()
    xd = N.BF16 if bf else N.F32
    s = _nan(rows, cols)
    y = _nan(rows, cols, dtype=xdt)
    mean, rstd = _nan(rows), _nan(rows)
    N.call("dna_add_ln_fwd", x.data_ptr(), xd, res.data_ptr(), gm.data_ptr(),
           None if rms else bt.data_ptr(), rows, cols, eps, rms, s.data_ptr(),
           None if bf else y.data_ptr(), y.data_ptr() if bf else None,
           None if rms else mean.data_ptr(), rstd.data_ptr(), st)
    assert torch.equal(s, s32)  # the fp32 sum is torch's x + residual bit for bit
    rep.add("fwd.y", y, y64, y32)
    nws = N.lib().dna_ln_bwd_workspace(rows, cols)
    ws = torch.empty(max(nws, 16), device=DEV, dtype=torch.uint8)
    o = dict(dx=_nan(rows, cols).to(xdt), dres=_nan(rows, cols), dgamma=_nan(cols))
    if not rms:
        o["dbeta"] = _nan(cols)
    N.call("dna_add_ln_bwd", _p(gout[0]), _p(gout[1]), ds.data_ptr(), x.data_ptr(), xd,
           res.data_ptr(), gm.data_ptr(), None if rms else mean.data_ptr(), rstd.data_ptr(), rows,
           cols, rms, o["dres"].data_ptr(), o["dx"].data_ptr(), o["dgamma"].data_ptr(),
           _p(o.get("dbeta")), ws.data_ptr(), nws, st)
    for k, v in o.items():
        rep.add(f"bwd.{k}", v, g64[k], g32[k])
    rep.finish()


@pytest.mark.parametrize("xdt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows_big", [False, True], ids=["r3", "rbig"])
@pytest.mark.parametrize("cols", [256, 768])
def test_rms_bwd_vs_fp64(cols, rows_big, xdt):
    from dna_amd import _native as N
    rows = _big(cols) + 3 if rows_big else 3
    eps = 1e-5
    g = torch.Generator(device=DEV).manual_seed(rows + cols + 7)
    x = torch.randn(rows, cols, device=DEV, generator=g).to(xdt)
    gm = 1 + 0.1 * torch.randn(cols, device=DEV, generator=g)
    gout = _rand_gouts(1, (rows, cols), "both", g)[0]
    _, y64, g64 = _add_ln_graph(torch.float64, x, None, gm, None, eps, 1, None, gout)
    _, y32, g32 = _add_ln_graph(torch.float32, x, None, gm, None, eps, 1, None, gout)
    bf = xdt == torch.bfloat16
    rep = _Report(f"rms-{rows}x{cols}-{'bf16' if bf else 'f32'}")
    st = N.stream_ptr()
    xd = N.BF16 if bf else N.F32
    y, yb, rstd = _nan(rows, cols), _nan(rows, cols, dtype=torch.bfloat16), _nan(rows)
    N.call("dna_rms_fwd", x.data_ptr(), xd, gm.data_ptr(), rows, cols, eps, y.data_ptr(),
           yb.data_ptr(), rstd.data_ptr(), st)
    rep.add("fwd.y", y, y64, y32)
    rep.add("fwd.y_bf16", yb, y64, y32)
    nws = N.lib().dna_ln_bwd_workspace(rows, cols)
    ws = torch.empty(max(nws, 16), device=DEV, dtype=torch.uint8)
    dx, dg = _nan(rows, cols).to(xdt), _nan(cols)
    N.call("dna_rms_bwd", _p(gout[0]), _p(gout[1]), x.data_ptr(), xd, gm.data_ptr(),
           rstd.data_ptr(), rows, cols, dx.data_ptr(), dg.data_ptr(), ws.data_ptr(), nws, st)
    rep.add("bwd.dx", dx, g64["dx"], g32["dx"])
    rep.add("bwd.dgamma", dg, g64["dgamma"], g32["dgamma"])
    rep.finish()


def _embed_graph(dt, ids, E, tt, gm, bt, eps, keep, p, gout):
    rows_in = E[ids].detach().to(dt).requires_grad_(True)  # the gathered rows: drows' variable
    L = dict(drows=rows_in, dtype_row=tt.detach().to(dt).requires_grad_(True),
             dgamma=gm.detach().to(dt).requires_grad_(True),
             dbeta=bt.detach().to(dt).requires_grad_(True))
    y = F.layer_norm(L["drows"] + L["dtype_row"], (E.shape[1],), L["dgamma"], L["dbeta"], eps)
    if keep is not None:
        y = y * (keep.to(dt) * _kscale(p))
    names = list(L)
    grads = dict(zip(names, torch.autograd.grad(y, [L[k] for k in names], _gsum(dt, *gout))))
    return y.detach(), grads


@pytest.mark.parametrize("cols,rows_big,p", [(256, False, 0.0), (256, True, 0.1), (768, False, 0.0),
                                             (768, True, 0.0)])
def test_embed_ln_bwd_rows_vs_fp64(cols, rows_big, p):
    """dna_embed_ln_fwd / dna_embed_ln_bwd_rows with repeated ids (7-row table)."""
    from dna_amd import _native as N
    rows = _big(cols) + 3 if rows_big else 3
    V, eps = 7, 1e-12
    g = torch.Generator(device=DEV).manual_seed(rows + cols + 11)
    ids = torch.randint(0, V, (rows,), device=DEV, generator=g)
    if not rows_big:
        ids[2] = ids[0]
    E = torch.randn(V, cols, device=DEV, generator=g)
    tt = 0.1 * torch.randn(cols, device=DEV, generator=g)
    gm = 1 + 0.1 * torch.randn(cols, device=DEV, generator=g)
    bt = 0.1 * torch.randn(cols, device=DEV, generator=g)
    gout = _rand_gouts(1, (rows, cols), "both", g)[0]
    keep = _keep_mask(rows, cols, p)
    y64, g64 = _embed_graph(torch.float64, ids, E, tt, gm, bt, eps, keep, p, gout)
    y32, g32 = _embed_graph(torch.float32, ids, E, tt, gm, bt, eps, keep, p, gout)
    rep = _Report(f"embed-{rows}x{cols}-p{p}")
    st = N.stream_ptr()
    y, yb = _nan(rows, cols), _nan(rows, cols, dtype=torch.bfloat16)
    mean, rstd = _nan(rows), _nan(rows)
    N.call("dna_embed_ln_fwd", ids.data_ptr(), E.data_ptr(), tt.data_ptr(), gm.data_ptr(),
           bt.data_ptr(), rows, cols, V, eps, p, SEED, OFF, y.data_ptr(), yb.data_ptr(),
           mean.data_ptr(), rstd.data_ptr(), st)
    rep.add("fwd.y", y, y64, y32)
    rep.add("fwd.y_bf16", yb, y64, y32)
    if keep is not None:
        assert torch.equal(y == 0, ~keep)
    nws = N.lib().dna_ln_bwd_workspace(rows, cols)
    ws = torch.empty(max(nws, 16), device=DEV, dtype=torch.uint8)
    o = dict(drows=_nan(rows, cols), dtype_row=_nan(cols), dgamma=_nan(cols), dbeta=_nan(cols))
    N.call("dna_embed_ln_bwd_rows", _p(gout[0]), _p(gout[1]), ids.data_ptr(), E.data_ptr(),
           tt.data_ptr(), gm.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, cols, V, p, SEED,
           OFF, o["drows"].data_ptr(), o["dtype_row"].data_ptr(), o["dgamma"].data_ptr(),
           o["dbeta"].data_ptr(), ws.data_ptr(), nws, st)
    for k, v in o.items():
        rep.add(f"bwd.{k}", v, g64[k], g32[k])
    rep.finish()


# ------------------------------------------------------------------ (c) zero / tiny gamma
def _tiny_gamma(cols, t, g):
    gm = 1 + 0.1 * torch.randn(cols, device=DEV, generator=g)
    bt = 0.1 * torch.randn(cols, device=DEV, generator=g)
    idx = torch.tensor([3, 64, cols - 1, 17], device=DEV)
    gm[idx] = torch.tensor([t, -t, t, t], device=DEV)
    bt[idx[:2]] = 1.0
    return gm, bt, idx


@pytest.mark.parametrize("t", [0.0, 1e-6, 1e-4, 1e-3, 1e-2, 1e-1])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("cols", [128, 768])
def test_fused_layernorm_zero_and_tiny_gamma(cols, p, t):
    """FusedLayerNorm.apply (the public path) with four gamma entries at (t, -t, t, t), beta = 1 in
    two of them: the output and every gradient stay within the K bound of the well-conditioned
    cases -- in particular dgamma of a zero-gamma column is the fp64 value (O(sqrt(rows))), not 0.

    Before FusedLayerNorm chose its backward by ln_from_y_ok, t = 0 and t = 1e-6 failed:
    err (and err / err_torch32) over the four shapes, from-y backward for every gamma:
      t = 0:    dgamma 4.8e-1 .. 8.8e-1 (3.4e6 .. 6.4e6), dres 4.0e-2 .. 1.2e-1, dbias 1.4e-3 ..
                5.4e-2, bf16 dx up to 0.68 (absolute) past its bound; dgamma of the four columns = 0
      t = 1e-6: dgamma 8.9e-3 .. 3.2e-2 (6.5e4 .. 2.6e5), dres 1.2e-3 .. 2.5e-3, dbias 4.5e-4 ..
                6.0e-4
    and with smaller excess up to t = 1e-2: dgamma 335 .. 1010 (1e-4), 44 .. 99 (1e-3), 6.7 .. 12.5
    (1e-2) times err_torch32."""
    from dna_amd import functional as DF
    rows, eps = 1000, 1e-12
    g = torch.Generator(device=DEV).manual_seed(cols + int(10 * p) + 3)
    x = torch.randn(rows, cols, device=DEV, generator=g).bfloat16()
    bias = 0.1 * torch.randn(cols, device=DEV, generator=g)
    res = torch.randn(rows, cols, device=DEV, generator=g)
    gm, bt, idx = _tiny_gamma(cols, t, g)
    gouts = _rand_gouts(1, (rows, cols), "both", g)
    keep = _keep_mask(rows, cols, p)
    y64, (g64,) = _ln_graph(torch.float64, x, bias, res, gm, bt, eps, 0, keep, p, gouts)
    y32, (g32,) = _ln_graph(torch.float32, x, bias, res, gm, bt, eps, 0, keep, p, gouts)
    names = ("dx", "dbias", "dres", "dgamma", "dbeta")
    leaves = [v.clone().requires_grad_(True) for v in (x, bias, res, gm, bt)]
    y, yb = DF.FusedLayerNorm.apply(*leaves, eps, 0, p, SEED, OFF, True, True)
    torch.autograd.backward([y, yb], list(gouts[0]))
    rep = _Report(f"tiny-{cols}-p{p}-t{t:g}")
    rep.add("y", y.detach(), y64, y32)
    rep.add("y_bf16", yb.detach(), y64, y32)
    for k, leaf in zip(names, leaves):
        rep.add(k, leaf.grad, g64[k], g32[k])
    print(f"DGAMMA tiny-{cols}-p{p}-t{t:g}: kernel {leaves[3].grad[idx].tolist()} "
          f"fp64 {g64['dgamma'][idx].tolist()}")
    assert g64["dgamma"][idx].abs().max().item() > rows ** 0.5 / 4  # far from 0 on these inputs
    if keep is not None:
        assert torch.equal(leaves[0].grad == 0, ~keep)
    rep.finish()


# ------------------------------------------------------------------ (d) direct-gradient route
class _LNBlock(torch.nn.Module):
    def __init__(self, cols):
        super().__init__()
        self.bias = torch.nn.Parameter(torch.zeros(cols))
        self.LayerNorm = torch.nn.LayerNorm(cols, eps=1e-12)

    def forward(self, x, res, p):
        from dna_amd import functional as DF
        return DF.FusedLayerNorm.apply(x, self.bias, res, self.LayerNorm.weight,
                                       self.LayerNorm.bias, 1e-12, 0, p, SEED, OFF, True, True)


@pytest.mark.parametrize("zero_gamma", [False, True], ids=["wellcond", "zerogamma"])
@pytest.mark.parametrize("cols", [128, 768])
def test_direct_grad_two_backwards_vs_fp64(cols, zero_gamma, monkeypatch):
    """bias / LayerNorm.weight / LayerNorm.bias owned by FlatParams with direct gradients on: two
    backward passes without zeroing leave the sum of the two fp64 gradients in the flat .grad.
    gamma = 1 +- 0.1 takes dna_ln_bwd_from_y_acc; a zero gamma entry must not take the from-y
    kernel and must still accumulate (through AccumulateGrad)."""
    from dna_amd import _native as N
    from dna_amd.flat import FlatParams
    rows, p, eps = 1000, 0.1, 1e-12
    g = torch.Generator(device=DEV).manual_seed(cols + 5)
    blk = _LNBlock(cols).to(DEV)
    gm, bt, idx = _tiny_gamma(cols, 0.0, g) if zero_gamma else (
        1 + 0.1 * torch.randn(cols, device=DEV, generator=g),
        0.1 * torch.randn(cols, device=DEV, generator=g), None)
    bias = 0.1 * torch.randn(cols, device=DEV, generator=g)
    with torch.no_grad():
        blk.bias.copy_(bias)
        blk.LayerNorm.weight.copy_(gm)
        blk.LayerNorm.bias.copy_(bt)
    flat = FlatParams(blk, DEV, shadow_dtype=None)
    flat.enable_direct_grad(True)
    flat.zero_grad()
    called = []
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    keep = _keep_mask(rows, cols, p)
    tot64 = tot32 = None
    for _ in range(2):
        x = torch.randn(rows, cols, device=DEV, generator=g).bfloat16()
        res = torch.randn(rows, cols, device=DEV, generator=g)
        gouts = _rand_gouts(1, (rows, cols), "both", g)
        _, (g64,) = _ln_graph(torch.float64, x, bias, res, gm, bt, eps, 0, keep, p, gouts)
        _, (g32,) = _ln_graph(torch.float32, x, bias, res, gm, bt, eps, 0, keep, p, gouts)
        tot64 = g64 if tot64 is None else {k: tot64[k] + g64[k] for k in g64}
        tot32 = g32 if tot32 is None else {k: tot32[k] + g32[k] for k in g32}
        y, yb = blk(x, res, p)
        torch.autograd.backward([y, yb], list(gouts[0]))
    bwd = [c for c in called if c.startswith("dna_ln_bwd") and not c.endswith("workspace")]
    assert bwd == (["dna_ln_bwd"] * 2 if zero_gamma else ["dna_ln_bwd_from_y_acc"] * 2), bwd
    rep = _Report(f"direct-{cols}-zero{int(zero_gamma)}")
    for k, prm in (("dbias", blk.bias), ("dgamma", blk.LayerNorm.weight),
                   ("dbeta", blk.LayerNorm.bias)):
        o, n, shape = flat.slice_of(prm)
        assert prm.grad.data_ptr() == flat.grad[o:o + n].data_ptr()
        rep.add(k, flat.grad[o:o + n].view(shape), tot64[k], tot32[k])
    rep.finish()


def test_guard_sees_parameter_writes_torch_does_not():
    """The fused AdamW step rewrites gamma / beta through raw pointers (no `_version` change).
    Without a guard the cached verdict expires with the write and the next forward recomputes it;
    with one (the trainers), the verdict arrives from the device check -- computed with the
    margin of MAX_AGE optimizer steps, so a pair close to the threshold already leaves the
    from-y path while ln_from_y_ok itself still passes."""
    from dna_amd import _native as N
    from dna_amd import functional as DF
    from dna_amd.flat import FlatParams, note_raw_write
    from dna_amd.optim import FusedAdamW
    cols, rows = 128, 8
    blk = _LNBlock(cols).to(DEV)
    flat = FlatParams(blk, DEV, shadow_dtype=None)
    opt = FusedAdamW(flat, lr=1e-3, weight_decay=0.0)
    gamma, beta = blk.LayerNorm.weight, blk.LayerNorm.bias
    go = flat.slice_of(gamma)[0]
    x = torch.randn(rows, cols, device=DEV).requires_grad_(True)

    def from_y():
        y, _ = blk(x, None, 0.0)
        return y.grad_fn.from_y

    assert from_y() and gamma._dna_ln_verdict[0]
    v = gamma._version
    flat.flat[go + 5] = 0.0  # as the optimizer kernel would: no version change on the parameter
    note_raw_write()
    assert gamma._version == v and gamma[5].item() == 0.0
    assert not from_y()  # expired entry -> recomputed
    flat.flat[go + 5] = 1.0
    note_raw_write()
    assert from_y()

    guard = DF.LNFromYGuard(flat, opt)
    margin = guard.MAX_AGE * 3.2 * 1e-3
    for val, want in ((1.0, True), (0.0, False), (margin / 2, False), (-1.0, True)):
        flat.flat[go + 5] = val
        flat.flat[flat.slice_of(beta)[0] + 5] = 0.0
        note_raw_write()
        guard.launch()
        torch.cuda.synchronize()
        guard.poll()
        ok, b, gv, bv, until = gamma._dna_ln_verdict
        assert ok is want and b is beta and until >= guard.MAX_AGE, (val, gamma._dna_ln_verdict)
        assert from_y() is want
        assert not guard._pending
    assert DF.ln_from_y_ok(torch.tensor([margin / 2]), torch.tensor([0.0]))
    # an in-place change torch does see invalidates the entry at once
    with torch.no_grad():
        gamma[7] = 0.0
    assert not from_y()


def test_trainer_keeps_verdicts_fresh_without_host_sync(monkeypatch):
    """MLMTrainer steps in the steady state: no host synchronisation (torch's sync debug mode set
    to raise), one dna_ln_from_y_check per optimizer step, every encoder LayerNorm on the
    accumulating from-y kernel with a verdict that is still valid; after a gamma entry is
    zeroed behind torch's back the next checks move that LayerNorm, and only it, to dna_ln_bwd."""
    import collections
    from dna_amd import _native as N
    from dna_amd.bert_layers import BertForMaskedLM
    from dna_amd.flat import note_raw_write, raw_writes
    from dna_amd.trainer import DeviceBatch, MLMTrainer
    cfg = dict(vocab_size=4096, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
               intermediate_size=512, hyena_framework=True)
    dev = torch.device(DEV, 0)
    torch.manual_seed(0)
    tr = MLMTrainer(BertForMaskedLM(cfg, precision="bf16"), dev, lr=1e-3, weight_decay=1e-5)
    g = torch.Generator().manual_seed(1)
    batches = []
    for _ in range(2):
        target = torch.randint(5, 4096, (4, 128), generator=g)
        mask = torch.rand(4, 128, generator=g) < 0.15
        mask[:, 1] = True
        batches.append(DeviceBatch.from_host(torch.where(mask, torch.full_like(target, 4), target),
                                             mask, torch.where(mask, target, torch.full_like(target, -100)),
                                             target, dev))
    for i in range(3):
        tr.step(batches[i % 2])
    cnt = collections.Counter()
    real = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: (cnt.update([name]), real(name, *a))[1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(4):
            tr.step(batches[i % 2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    lns = [p for p in tr.flat.params if hasattr(p, "_dna_ln_verdict")]
    assert len(lns) == 4  # 2 layers x (attention output, MLP); the head's (gelu) never asks
    assert cnt["dna_ln_from_y_check"] == 4
    assert cnt["dna_ln_bwd_from_y_acc"] == 4 * 4 and cnt["dna_ln_bwd"] == 4  # head: gelu, from x
    assert all(p._dna_ln_verdict[0] and p._dna_ln_verdict[4] >= raw_writes() for p in lns)
    victim = tr.model.bert.encoder.layer[0].attention.output.LayerNorm.weight
    assert any(p is victim for p in lns)
    tr.flat.flat[tr.flat.slice_of(victim)[0] + 3] = 0.0
    note_raw_write()
    for i in range(3):
        tr.step(batches[i % 2])
        torch.cuda.synchronize()
    cnt.clear()
    tr.step(batches[0])
    assert [p._dna_ln_verdict[0] for p in lns] == [p is not victim for p in lns]
    assert cnt["dna_ln_bwd_from_y_acc"] == 3 and cnt["dna_ln_bwd"] == 2
