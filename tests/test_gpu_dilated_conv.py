"""The dilated-convolution kernels alone (csrc/dilated_conv.hip: dna_dconv_fwd, dna_dconv_bwd_elem,
dna_dconv_wgrad, dna_onehot_conv_*) through torch.ops.dna_amd.*. The truth is F.conv1d in float64
on the CPU, computed once per shape.

Shapes (B, L, C, K, d): (3, 96, 64, 9, 64) -- every tap but the centre one is empty (4 * 64 > L);
(2, 200, 128, 5, 9) -- two channel tiles, a ragged second row tile; (2, 65, 64, 9, 1) -- one row
past a 64-row boundary, taps that cross the sequence boundary inside a tile; (1, 33, 128, 3, 27) --
L below one tile, taps that reach one side only; (2, 130, 64, 7, 4) -- two rows past the 128-row
block tile.

Bounds.
  exact       x, W, dz in {-1, 0, 1}, bias an integer in [-2, 2]: every output is an integer of
              magnitude <= 256 (asserted on the truth), so bf16 and fp32 both hold it exactly and
              the kernels must return the truth bit for bit, whatever their summation order.
  real bf16   operands rounded to bf16 before the truth is taken; what differs is fp32
              accumulation and one output rounding: |ours - truth| <= 2^-7 |truth| + 1e-3 rms.
  real fp32   at most 4x the error of torch's own fp32 CPU conv1d against the same truth, plus
              1e-6 rms (the 4 allows for the other summation order). The measured ratios are
              printed (pytest -s) and recorded in DESIGN.md.
  epilogues   GELU is common.h's erf form (|erf error| < 6e-7 in fp32, so |gelu error| and
              |gelu' error| < 1e-6 (1 + |z|)); against fp32 torch on the same stored z and g an
              output may be off by that times the factor it is multiplied with, plus the rounding
              of the output (one bf16 ulp = 2^-8; fp32: up to four roundings, 2^-21 relative).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import dna_amd.ops  # noqa: F401  (registers torch.ops.dna_amd.*)
from dna_amd import functional as DF

pytestmark = pytest.mark.gpu
DEV = "cuda"
O = torch.ops.dna_amd
SHAPES = [(3, 96, 64, 9, 64), (2, 200, 128, 5, 9), (2, 65, 64, 9, 1), (1, 33, 128, 3, 27),
          (2, 130, 64, 7, 4)]
shapes = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
dtypes = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def _conv(x, w, b, d):
    """F.conv1d, "same", on channels-last x [B, L, C] with w [co, ci, K] in x's dtype."""
    K = w.shape[2]
    return F.conv1d(x.transpose(1, 2), w, b, padding=(K - 1) // 2 * d, dilation=d).transpose(1, 2)


def _truth(x, w, b, dz, d, dtype=torch.float64):
    """(z, dx, dw, db) of the convolution in `dtype` on the CPU, by autograd."""
    x, w, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    z = _conv(x, w, b, d)
    z.backward(dz.to(dtype))
    return z.detach(), x.grad, w.grad, b.grad


def _ints(shape, gen, lo=-1, hi=1):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """Operands (fp32 on the CPU) and the float64 truth of one shape; kind: exact | real | bf16
    (real operands rounded to bf16)."""
    B, L, C, K, d = shape
    g = torch.Generator().manual_seed(sum(shape) + len(kind))
    if kind == "exact":
        x, w, dz = _ints((B, L, C), g), _ints((C, C, K), g), _ints((B, L, C), g)
        b = _ints((C,), g, -2, 2)
    else:
        x = torch.randn(B, L, C, generator=g)
        w = torch.randn(C, C, K, generator=g) / (C * K) ** 0.5
        dz = torch.randn(B, L, C, generator=g)
        b = torch.randn(C, generator=g)
        if kind == "bf16":
            x, w, dz = (t.bfloat16().float() for t in (x, w, dz))
    return (x, w, b, dz), _truth(x, w, b, dz, d)


def _run(x, w, b, dz, d, dtype):
    """The four results of the kernels on the GPU: z (act none), dx, dw, db."""
    xd, dzd = x.to(DEV, dtype), dz.to(DEV, dtype)
    wd, bd = w.to(DEV), b.to(DEV)
    z, dx = torch.empty_like(xd), torch.empty_like(xd)
    O.dconv_fwd(xd, DF.conv_taps(wd, dtype), bd, d, "plain", "none", None, None, z, None, None)
    O.dconv_fwd(dzd, DF.conv_taps_dgrad(wd, dtype), None, d, "plain", "none", None, None, dx, None,
                None)
    dw, db = torch.empty_like(wd), torch.empty_like(bd)
    O.dconv_wgrad(dzd, xd, d, dw, db, False)
    torch.cuda.synchronize()
    return z.float().cpu(), dx.float().cpu(), dw.cpu(), db.cpu()


@shapes
@dtypes
def test_exact_integer_operands(shape, dtype):
    ops, truth = _case(shape, "exact")
    for name, t in zip(("z", "dx"), truth):
        assert float(t.abs().max()) <= 256 and bool((t == t.round()).all()), name
    got = _run(*ops, shape[4], dtype)
    for name, o, t in zip(("z", "dx", "dw", "db"), got, truth):
        assert torch.equal(o.double(), t), (name, float((o.double() - t).abs().max()))


@shapes
def test_real_valued_bf16(shape):
    ops, truth = _case(shape, "bf16")
    got = _run(*ops, shape[4], torch.bfloat16)
    for name, o, t in zip(("z", "dx", "dw", "db"), got, truth):
        rms = float(t.pow(2).mean().sqrt())
        excess = (o.double() - t).abs() - (2.0 ** -7 * t.abs() + 1e-3 * rms)
        print(f"bf16 {shape} {name}: max err {float((o.double() - t).abs().max()):.3e}, rms {rms:.3e}")
        assert float(excess.max()) <= 0, (name, float(excess.max()))


@shapes
def test_real_valued_fp32_vs_torch_fp32(shape):
    ops, truth = _case(shape, "real")
    cpu32 = _truth(*ops, shape[4], dtype=torch.float32)
    got = _run(*ops, shape[4], torch.float32)
    for name, o, c, t in zip(("z", "dx", "dw", "db"), got, cpu32, truth):
        rms = float(t.pow(2).mean().sqrt())
        ours, torchs = float((o.double() - t).abs().max()), float((c.double() - t).abs().max())
        print(f"fp32 {shape} {name}: ours {ours:.3e}, torch fp32 {torchs:.3e}, "
              f"ratio {ours / max(torchs, 1e-30):.2f}")
        assert ours <= 4 * torchs + 1e-6 * rms, (name, ours, torchs)


def _gelu_bound(z, factor, out_ulp, ref):
    return 1e-6 * (1 + z.abs()) * factor + out_ulp * ref.abs() + 1e-12


@dtypes
@pytest.mark.parametrize("forget", [True, False], ids=["forget", "add"])
def test_epilogues_and_their_backward(forget, dtype):
    B, L, C, K, d = 2, 65, 64, 9, 4
    g0 = torch.Generator().manual_seed(11)
    x_h, x_g = (torch.randn(B, L, C, generator=g0).to(DEV, dtype) for _ in range(2))
    w_h, w_g = ((torch.randn(C, C, K, generator=g0) * 2 / (C * K) ** 0.5).to(DEV) for _ in range(2))
    b_h, b_g = (torch.randn(C, generator=g0).to(DEV) for _ in range(2))
    feat, rc, df, drc = (torch.randn(B, L, C, generator=g0).to(DEV) for _ in range(4))
    # output rounding: one bf16 ulp, or the four fp32 roundings of the longest expression
    ulp = 2.0 ** -21 if dtype == torch.float32 else 2.0 ** -8
    g, z_g, z_h = (torch.empty_like(x_g) for _ in range(3))
    rc_new, feat_new = torch.empty_like(rc), torch.empty_like(feat)
    O.dconv_fwd(x_g, DF.conv_taps(w_g, dtype), b_g, d, "gate", "sigmoid" if forget else "gelu",
                None, rc, g, z_g, rc_new)
    O.dconv_fwd(x_h, DF.conv_taps(w_h, dtype), b_h, d, "main_mul" if forget else "main_add", "gelu",
                g, feat, None, z_h, feat_new)
    # z itself: the plain convolution, rounded to the activation dtype
    for z, x, w, b in ((z_g, x_g, w_g, b_g), (z_h, x_h, w_h, b_h)):
        ref = _conv(x.double().cpu(), w.to(dtype).double().cpu(), b.double().cpu(), d)
        err = (z.double().cpu() - ref).abs()
        assert float((err - (2 * ulp * ref.abs() + 1e-5)).max()) <= 0
    # the combine, in fp32 torch on the stored z and g
    zg32, zh32, g32 = z_g.float(), z_h.float(), g.float()
    g_ref = torch.sigmoid(zg32) if forget else F.gelu(zg32)
    one = torch.ones_like(g32)
    assert float(((g32 - g_ref).abs() - _gelu_bound(zg32, one, ulp, g_ref)).max()) <= 0
    assert torch.equal(rc_new, g32 + rc)
    h_ref = F.gelu(zh32)
    f_ref = h_ref * g32 + feat if forget else h_ref + g32 + feat
    fac = g32.abs() if forget else one
    assert float(((feat_new - f_ref).abs() - _gelu_bound(zh32, fac, 2.0 ** -22, f_ref)).max()) <= 0
    # the elementwise backward against autograd on the same z (the sigmoid's factor from the
    # stored g, as the kernel takes it)
    dz_h, dz_g = torch.empty_like(z_h), torch.empty_like(z_h)
    O.dconv_bwd_elem(df, drc, z_h, g if forget else None, None if forget else z_g, forget, dz_h,
                     dz_g)
    zh_l, zg_l = zh32.clone().requires_grad_(True), zg32.clone().requires_grad_(True)
    h = F.gelu(zh_l)
    if forget:
        (h * g32 * df).sum().backward()
        rh = zh_l.grad
        rg = (df * h.detach() + drc) * g32 * (1 - g32)
        fh, fg = (df * g32).abs(), (df.abs() * (1 + zh32.abs()) + drc.abs())
    else:
        # g's two consumers as one upstream df + drc (the kernel's own fp32 add): summing two
        # separately rounded products instead would put the reference's cancellation error,
        # 2^-24 |df gelu'|, against a bound that scales with |df + drc|
        (h * df + F.gelu(zg_l) * (df + drc)).sum().backward()
        rh, rg = zh_l.grad, zg_l.grad
        fh, fg = df.abs(), (df + drc).abs()
    assert float(((dz_h.float() - rh).abs() - _gelu_bound(zh32, fh, ulp, rh)).max()) <= 0
    assert float(((dz_g.float() - rg).abs() - _gelu_bound(zg32, fg, ulp, rg)).max()) <= 0
    # drc = NULL is drc = 0
    a, b2 = torch.empty_like(z_h), torch.empty_like(z_h)
    c, d2 = torch.empty_like(z_h), torch.empty_like(z_h)
    O.dconv_bwd_elem(df, None, z_h, g if forget else None, None if forget else z_g, forget, a, b2)
    O.dconv_bwd_elem(df, torch.zeros_like(drc), z_h, g if forget else None,
                     None if forget else z_g, forget, c, d2)
    assert torch.equal(a, c) and torch.equal(b2, d2)


def _onehot_truth(ids, w, b, dout, complement, act, dtype=torch.float64):
    V, KW = w.shape[1], w.shape[2]
    if complement:
        ids = torch.where(ids == 4, ids, 3 - ids)
    w, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (w, b))
    z = F.conv1d(F.one_hot(ids, V).to(dtype).transpose(1, 2), w, b, padding=(KW - 1) // 2)
    z = z.transpose(1, 2)
    out = F.gelu(z) if act == "gelu" else z
    out.backward(dout.to(dtype))
    return out.detach(), w.grad, b.grad, z.detach()


@pytest.mark.parametrize("complement", [False, True], ids=["ids", "complement"])
def test_onehot_input_layer(complement):
    B, L, C, V, KW = 3, 37, 128, 5, 9
    g0 = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 4, (B, L), generator=g0)
    ids[0, :6] = 4
    ids[1, 15:19] = 4
    ids[2, -3:] = 4
    # exact: integer table, no activation -> integers, bit for bit, forward and backward
    w, b = _ints((C, V, KW), g0, -3, 3), _ints((C,), g0, -2, 2)
    dout = _ints((B, L, C), g0)
    out, dw, db = (torch.empty(s, device=DEV) for s in ((B, L, C), (C, V, KW), (C,)))
    O.onehot_conv_fwd(ids.to(DEV), w.to(DEV), b.to(DEV), complement, "none", out)
    O.onehot_conv_bwd(ids.to(DEV), w.to(DEV), b.to(DEV), dout.to(DEV), complement, "none", dw, db,
                      False)
    t_out, t_dw, t_db, _ = _onehot_truth(ids, w, b, dout, complement, "none")
    assert torch.equal(out.cpu().double(), t_out)
    assert torch.equal(dw.cpu().double(), t_dw) and torch.equal(db.cpu().double(), t_db)
    assert float(t_dw[:, 4].abs().sum()) > 0  # the N rows reach the table's N column
    # GELU: forward within the erf form's error, gradients within that error summed over the rows
    w, b = torch.randn(C, V, KW, generator=g0) / 3, torch.randn(C, generator=g0)
    dout = torch.randn(B, L, C, generator=g0)
    O.onehot_conv_fwd(ids.to(DEV), w.to(DEV), b.to(DEV), complement, "gelu", out)
    O.onehot_conv_bwd(ids.to(DEV), w.to(DEV), b.to(DEV), dout.to(DEV), complement, "gelu", dw, db,
                      False)
    t_out, t_dw, t_db, z = _onehot_truth(ids, w, b, dout, complement, "gelu")
    c_out, c_dw, c_db, _ = _onehot_truth(ids, w, b, dout, complement, "gelu", torch.float32)
    # z is an fp32 sum of KW + 1 terms: at most (KW + 1) 2^-24 of the sum of their magnitudes off
    zerr = (KW + 1) * 2.0 ** -24 * float(KW * w.abs().max() + b.abs().max())
    bound = 1e-6 * (1 + z.abs()) + 2.0 ** -22 * t_out.abs() + zerr
    assert float(((out.cpu().double() - t_out).abs() - bound).max()) <= 0
    # |gelu''| < 1.2, so a gradient element is off by at most (1e-6 (1 + |z|) + 1.2 zerr) |dout|
    slack = ((1e-6 * float((1 + z.abs()).max()) + 1.2 * zerr)
             * float(dout.abs().sum(dim=(0, 1)).max()))
    for got, cpu, t in ((dw, c_dw, t_dw), (db, c_db, t_db)):
        ours, torchs = float((got.cpu().double() - t).abs().max()), float((cpu.double() - t).abs().max())
        assert ours <= 4 * torchs + slack, (ours, torchs, slack)
    # accumulate adds to what is there
    dw2, db2 = dw.clone(), db.clone()
    O.onehot_conv_bwd(ids.to(DEV), w.to(DEV), b.to(DEV), dout.to(DEV), complement, "gelu", dw2, db2,
                      True)
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)


@dtypes
def test_backward_is_deterministic_and_accumulates(dtype):
    shape = (2, 200, 128, 5, 9)
    (x, w, b, dz), _ = _case(shape, "bf16")
    a = _run(x, w, b, dz, shape[4], dtype)
    c = _run(x, w, b, dz, shape[4], dtype)
    for name, p, q in zip(("z", "dx", "dw", "db"), a, c):
        assert torch.equal(p, q), name
    xd, dzd = x.to(DEV, dtype), dz.to(DEV, dtype)
    dw, db = a[2].to(DEV).clone(), a[3].to(DEV).clone()
    O.dconv_wgrad(dzd, xd, shape[4], dw, db, True)
    assert torch.equal(dw.cpu(), a[2] + a[2]) and torch.equal(db.cpu(), a[3] + a[3])


def test_bad_arguments_raise_and_launch_nothing():
    x = torch.zeros(1, 8, 96, device=DEV)  # C = 96: no multiple of 64
    with pytest.raises(RuntimeError, match="unsupported"):
        O.dconv_fwd(x, torch.zeros(3, 96, 96, device=DEV), None, 1, "plain", "none", None, None,
                    torch.empty_like(x), None, None)
    x = torch.zeros(1, 8, 64, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):  # even K
        O.dconv_fwd(x, torch.zeros(4, 64, 64, device=DEV), None, 1, "plain", "none", None, None,
                    torch.empty_like(x), None, None)
    with pytest.raises(RuntimeError, match="GPU"):
        O.dconv_fwd(x.cpu(), torch.zeros(3, 64, 64), None, 1, "plain", "none", None, None,
                    torch.empty(1, 8, 64), None, None)
