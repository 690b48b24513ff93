"""GPU: every default dispatch path of the bf16 MFMA GEMMs of csrc/gemm.hip against a reference
with no tolerance.

A bf16 GEMM with fp32 accumulation is exact -- for any summation order and any MFMA-internal
format -- while every partial sum is an integer below 2^24 (times a power of two). With integer
operands the expected bf16 output is round-to-nearest-even(exact sum + bias), which is what the
epilogues' (bf16)float does, so the tests assert torch.equal against an fp64 product: any wrong
element is a kernel or launcher bug, never noise. Two operand classes per shape ("a_wide": A in
[-255, 255] fills all 8 significant bits of bf16 and B in [-2, 2]; "b_wide": swapped) catch a
path that loses low mantissa bits of one operand; permutation / one-hot probes carry arbitrary
normal bf16 bit patterns through the same kernels; a per-element fp64 bound (derived, not
measured) covers realistic randn data. Every output is the head of a NaN-filled buffer and every
operand the head of a NaN-filled parent: rows past the logical end must be neither read into the
result nor written.

Dispatch (read from the launchers at the end of gemm.hip; unless a test says so no DNA_GEMM_*
switch is set, so this is what the defaults reach -- _fwd_path restates the condition and every
forward test asserts the path its shape list is named for):
  dna_linear_fwd / dna_geglu_linear_fwd   persistent gemmp_kernel<EPI, SCH> iff N % 256 == 0
      (GeGLU: any F % 128), N (2F) <= 8192, K >= 128 and the weight < 2 GB; body SCH = 2 iff
      K / 64 is even, else the older SCH = 0 body; otherwise gemm_kernel<true, true, EPI>
  dna_linear_dgrad / dna_geglu_linear_dgrad   always gemm_kernel<true, false, EPI>
  dna_linear_wgrad                            always gemm_kernel<false, false, EPI_F32>
  dna_geglu_linear_dgrad_p / dna_gelu_linear_dgrad_p   always gemmp_kernel<EPI, 2>
  dna_linear_wgrad_p                          wgradp_kernel<2> (K-step pairs); wgradp_kernel<0>
      only where a chunk of whole pairs would pass 2^31 bytes
DNA_GEMM_SCHED=0 (read per call) puts the SCH = 0 bodies of gemmp_kernel and wgradp_kernel where
the defaults take SCH = 2: the "sched0" / sched="0" arms run them under the same exact checks.
"""
import pytest
import torch

from dna_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


# ------------------------------------------------------------------ helpers (device-agnostic)
def _pow2(exp, device="cpu"):
    """fp64 2**exp for an integer tensor, by ldexp on the host: exact (a device pow need not be)."""
    e = exp.cpu().to(torch.int64)
    return torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e).to(device)


def _int_operand(rows, cols, amax, gen, row_exp=None):
    """bf16 [rows, cols] of random integers in [-amax, amax] (amax <= 256: exact in bf16); row r
    scaled by 2**row_exp[r] when given (exact, exercises the exponent field)."""
    assert amax <= 256
    t = torch.randint(-amax, amax + 1, (rows, cols), generator=gen).double()
    if row_exp is not None:
        t = t * _pow2(row_exp)[:, None]
    out = t.bfloat16()
    assert torch.equal(out.double(), t)
    return out


def _exact_ref(a64, b64, bias64, out_dtype, row_exp=None):
    """The exact result of a64 [M, K] @ b64 [K, N] + bias64 [N] for integer-valued fp64 operands
    (a64 WITHOUT its row scale). bf16 output: the sum goes .float() (exact: an integer below
    2^24), then the output rows' scale 2**row_exp, then .bfloat16() -- one round-to-nearest-even,
    as the epilogue's (bf16)float. The scale follows the bias add; 2^e (P + b) equals the operation
    under test, 2^e P + b, only without a bias, so the two are never combined."""
    K = a64.shape[-1]
    assert a64.dtype == b64.dtype == torch.float64 and b64.shape[0] == K
    for t in (a64, b64) + (() if bias64 is None else (bias64,)):
        assert bool((t == t.round()).all()), "exact reference: operands must be integers"
    amax = float(a64.abs().max()) if a64.numel() else 0.0
    bmax = float(b64.abs().max()) if b64.numel() else 0.0
    cmax = float(bias64.abs().max()) if bias64 is not None and bias64.numel() else 0.0
    assert K * amax * bmax + cmax <= 2 ** 24, \
        f"exact reference: K * max|a| * max|b| + max|bias| = {K * amax * bmax + cmax:.0f} > 2^24"
    assert bias64 is None or row_exp is None, "exact reference: a row scale with a bias"
    ref = a64 @ b64
    if bias64 is not None:
        ref = ref + bias64
    f = ref.float()
    assert torch.equal(f.double(), ref)
    if out_dtype == torch.float32:
        assert row_exp is None
        return f
    assert out_dtype == torch.bfloat16
    if row_exp is not None:
        f = f * _pow2(row_exp, f.device).float()[:, None]
    return f.bfloat16()


def _locate(bad, tile):
    """Where the True elements of the 2-D mask `bad` are: count, first index, bounding box, and the
    (row // tile, col // tile) tiles with the 128 x 128-style quadrant (tile halves) inside."""
    idx = bad.nonzero()
    r, c = idx[:, 0], idx[:, 1]
    tm, tn = tile
    key = torch.stack([r // tm, c // tn, (r % tm) // (tm // 2), (c % tn) // (tn // 2)], 1)
    tiles = torch.unique(key, dim=0).tolist()
    shown = ", ".join(f"tile ({a}, {b}) quadrant ({q}, {p})" for a, b, q, p in tiles[:24])
    more = f" ... and {len(tiles) - 24} more" if len(tiles) > 24 else ""
    first = (int(r[0]), int(c[0]))
    return first, (f"{idx.shape[0]} of {bad.numel()} elements wrong; first at {first}; "
                   f"bounding box rows [{int(r.min())}, {int(r.max())}] x cols "
                   f"[{int(c.min())}, {int(c.max())}]; in {len(tiles)} (tile, quadrant) of "
                   f"{tm} x {tn} tiles: {shown}{more}")


def _diff_report(got, want, tile=(256, 256)):
    """None when got equals want everywhere, else the localising message."""
    assert got.shape == want.shape and got.dtype == want.dtype and got.dim() == 2
    if torch.equal(got, want):
        return None
    first, where = _locate(~(got == want), tile)
    return f"{where}; got {got[first].item()!r}, want {want[first].item()!r}"


def _assert_same(got, want, tile=(256, 256), what=""):
    msg = _diff_report(got, want, tile)
    assert msg is None, f"{what}: {msg}"


def _bound_report(got, ref64, bound, tile=(256, 256)):
    """None when |got - ref64| <= bound everywhere (a NaN fails), else the localising message."""
    assert got.shape == ref64.shape == bound.shape and got.dim() == 2
    err = (got.double() - ref64).abs()
    bad = ~(err <= bound)
    if not bool(bad.any()):
        return None
    first, where = _locate(bad, tile)
    return (f"{where}; got {got[first].item()!r}, fp64 {ref64[first].item()!r}, error "
            f"{err[first].item():.3e} > bound {bound[first].item():.3e}")


def _assert_within(got, ref64, bound, tile=(256, 256), what=""):
    msg = _bound_report(got, ref64, bound, tile)
    assert msg is None, f"{what}: {msg}"


def _bf16_bound(a64, b64, bias64, K):
    """|got - ref| <= 2^-8 |ref| + (K + 2) 2^-23 S, S = sum_k |a_k| |b_k| + |bias|: the worst
    rounding of one bf16 store, plus the worst error of a K-term fp32 summation in any order (with
    a factor 2 of slack for truncating accumulators)."""
    ref = a64 @ b64
    S = a64.abs() @ b64.abs()
    if bias64 is not None:
        ref, S = ref + bias64, S + bias64.abs()
    return ref, 2.0 ** -8 * ref.abs() + (K + 2) * 2.0 ** -23 * S


def _f32_bound(a64, b64, T):
    return a64 @ b64, (T + 2) * 2.0 ** -23 * (a64.abs() @ b64.abs())


def _fwd_path(Nn, K, wide=None, sched=None):
    """The launcher's choice for dna_linear_fwd (wide = 2F for dna_geglu_linear_fwd, which has no
    N % 256 condition): 'p2' / 'p0' = persistent gemmp_kernel with the SCH = 2 / SCH = 0 body,
    'np' = gemm_kernel. sched = the value of DNA_GEMM_SCHED (None: unset, which means 2)."""
    assert sched in (None, "0", "2")
    rows = Nn if wide is None else wide
    ok = rows <= 8192 and K >= 128 and rows * K * 2 < 2 ** 31 and (wide is not None or Nn % 256 == 0)
    return "np" if not ok else ("p2" if sched != "0" and (K // 64) % 2 == 0 else "p0")


# ------------------------------------------------------------------ device plumbing
def _call(name, *args):
    N.call(name, *args, N.stream_ptr())


def _head(t, extra=256):
    """t on the device as the head of a NaN-filled parent: an exact-size operand whose
    neighbouring rows poison any result that reads them."""
    parent = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), NAN, device=DEV, dtype=t.dtype)
    parent[:t.shape[0]] = t.to(DEV)
    return parent[:t.shape[0]]


def _out(rows, cols, dtype, extra=64):
    return torch.full((rows + extra, cols), NAN, device=DEV, dtype=dtype)


def _written(buf, rows, what):
    """The first `rows` rows of a NaN-filled output buffer, after checking that nothing past them
    was touched."""
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[rows:]).all()), f"{what}: wrote past row {rows}"
    return buf[:rows]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _fwd(x, w, b):
    (M, K), Nn = x.shape, w.shape[0]
    buf = _out(M, Nn, torch.bfloat16)
    _call("dna_linear_fwd", x.data_ptr(), w.data_ptr(), _ptr(b), M, Nn, K, buf.data_ptr())
    return _written(buf, M, "dna_linear_fwd")


def _dgrad(dy, w):
    (M, Nn), K = dy.shape, w.shape[1]
    buf = _out(M, K, torch.bfloat16)
    _call("dna_linear_dgrad", dy.data_ptr(), w.data_ptr(), M, Nn, K, buf.data_ptr())
    return _written(buf, M, "dna_linear_dgrad")


def _wgrad(name, dy, x, splits):
    """fp32 partials [splits, N, K] of dy^T x from dna_linear_wgrad / dna_linear_wgrad_p, cut from
    a NaN-filled buffer: no NaN may remain in a slice, nothing after the last slice may change."""
    (T, Nn), K = dy.shape, x.shape[1]
    buf = torch.full((splits + 1, Nn, K), NAN, device=DEV)
    _call(name, dy.data_ptr(), x.data_ptr(), T, Nn, K, splits, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[splits]).all()), f"{name}: wrote past slice {splits}"
    for s in range(splits):
        assert not bool(torch.isnan(buf[s]).any()), f"{name}: slice {s} of {splits} not fully written"
    return buf[:splits]


def _gen(*ints):
    seed = 0
    for v in ints:
        seed = (seed * 1000003 + int(v) + 1) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(seed)


CLASSES = {"a_wide": (255, 2), "b_wide": (2, 255)}
M_SMALL = (1, 255, 257)
# more than two units per workgroup: 17 row tiles (17 % GM = 8 != 0, ragged last tile) x 32
# column tiles = 544 units on a grid of CUs & ~7 (256 on the MI355X)
MANY_M, MANY_N = 16 * 256 + 3, 8192
FWD_P2 = [(M, 256, K) for K in (128, 256) for M in M_SMALL] + [(MANY_M, MANY_N, 128)]
FWD_P0 = [(M, 256, K) for K in (192, 320) for M in M_SMALL] + [(MANY_M, MANY_N, 192)]
FWD_NP = ([(M, 256, 64) for M in (1, 257, 600)] +
          [(M, Nn, K) for Nn in (8, 264, 1000) for K in (64, 192) for M in (1, 257, 600)])
FWD_ALL = [(p, s) for p, shapes in (("p2", FWD_P2), ("p0", FWD_P0), ("np", FWD_NP)) for s in shapes]
FWD_IDS = [f"{p}-{M}x{Nn}x{K}" for p, (M, Nn, K) in FWD_ALL]
# the exact test also runs the SCH = 0 body at even K / 64, where only DNA_GEMM_SCHED=0 reaches it
FWD_EXACT = FWD_ALL + [("sched0", s) for s in FWD_P2]
FWD_EXACT_IDS = [f"{p}-{M}x{Nn}x{K}" for p, (M, Nn, K) in FWD_EXACT]
# (M, N, K): dx[M, K] = dy[M, N] . w[N, K], N / 64 K-steps = 1, 3, 12, 1 and (added) 2
DGRAD = [(1, 64, 8), (257, 192, 264), (600, 768, 1000), (300, 64, 256), (129, 128, 72)]
WGRAD_NK = [(8, 8), (264, 136), (256, 256)]
WGRAD_P_NK = [(256, 256), (512, 256)]
WGRAD_P_T = (128, 129, 191, 192, 193, 640, 1000)


def _check_path(path, M, Nn, K, sched=None):
    assert _fwd_path(Nn, K, sched=sched) == path
    if M == MANY_M:
        G = torch.cuda.get_device_properties(0).multi_processor_count & ~7
        U = ((M + 255) // 256) * (Nn // 256)
        assert U > 2 * G, f"{U} units on {G} workgroups: no workgroup runs a third unit"


# ------------------------------------------------------------------ 2. exact root kernels
@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("path,shape", FWD_EXACT, ids=FWD_EXACT_IDS)
def test_linear_fwd_exact(path, shape, bias, cls, monkeypatch):
    """dna_linear_fwd on integer operands equals bf16(exact sum + bias) everywhere; without a
    bias the rows of x carry random scales 2^-8 .. 2^8. The "sched0" arm sets DNA_GEMM_SCHED=0:
    the SCH = 0 body on the even-K/64 shapes."""
    M, Nn, K = shape
    if path == "sched0":
        monkeypatch.setenv("DNA_GEMM_SCHED", "0")
        _check_path("p0", M, Nn, K, sched="0")
    else:
        _check_path(path, M, Nn, K)
    g = _gen(M, Nn, K, bias, cls == "b_wide")
    amax, bmax = CLASSES[cls]
    rexp = None if bias else torch.randint(-8, 9, (M,), generator=g)
    x = _int_operand(M, K, amax, g, rexp)
    w = _int_operand(Nn, K, bmax, g)
    b = torch.randint(-64, 65, (Nn,), generator=g).float() if bias else None
    xd, wd, bd = _head(x), _head(w), (None if b is None else b.to(DEV))
    got = _fwd(xd, wd, bd)
    a64 = xd.double() if rexp is None else xd.double() * _pow2(-rexp, DEV)[:, None]
    want = _exact_ref(a64, wd.double().t(), None if bd is None else bd.double(), torch.bfloat16, rexp)
    _assert_same(got, want, what=f"dna_linear_fwd {path} M={M} N={Nn} K={K} {cls}")


@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("M,Nn,K", DGRAD)
def test_linear_dgrad_exact(M, Nn, K, cls):
    """dna_linear_dgrad (gemm_kernel<true, false, EPI_BF16>, w read n-contiguous) on integer
    operands, dy's rows scaled by 2^-8 .. 2^8."""
    g = _gen(M, Nn, K, cls == "b_wide", 1)
    amax, bmax = CLASSES[cls]
    rexp = torch.randint(-8, 9, (M,), generator=g)
    dy, w = _head(_int_operand(M, Nn, amax, g, rexp)), _head(_int_operand(Nn, K, bmax, g))
    got = _dgrad(dy, w)
    a64 = dy.double() * _pow2(-rexp, DEV)[:, None]
    want = _exact_ref(a64, w.double(), None, torch.bfloat16, rexp)
    _assert_same(got, want, what=f"dna_linear_dgrad M={M} N={Nn} K={K} {cls}")


@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("steps", [1, 2, 3, 5])
@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("Nn,K", WGRAD_NK)
def test_linear_wgrad_exact(Nn, K, splits, steps, cls):
    """dna_linear_wgrad (gemm_kernel<false, false, EPI_F32>): the fp32 split-K partials of
    dy^T x over M = 64 * splits * steps rows sum to the exact integer result."""
    M = 64 * splits * steps
    g = _gen(Nn, K, splits, steps, cls == "b_wide", 2)
    amax, bmax = CLASSES[cls]
    dy, x = _head(_int_operand(M, Nn, amax, g)), _head(_int_operand(M, K, bmax, g))
    parts = _wgrad("dna_linear_wgrad", dy, x, splits)
    want = _exact_ref(dy.double().t(), x.double(), None, torch.float32)
    _assert_same(parts.sum(0), want, what=f"dna_linear_wgrad M={M} N={Nn} K={K} splits={splits} {cls}")


def _wgrad_p_splits(T, Nn, K):
    auto = int(N.lib().dna_linear_wgrad_p_splits(T, Nn, K))
    return sorted({auto} | {s for s in (1, 2, 3) if ((T + 63) // 64) // s >= 2})


def _set_sched(monkeypatch, sched):
    """sched "2" is the default (variable unset); "0" selects the un-paired SCH = 0 bodies."""
    assert sched in ("0", "2")
    if sched == "0":
        monkeypatch.setenv("DNA_GEMM_SCHED", "0")
    else:
        monkeypatch.delenv("DNA_GEMM_SCHED", raising=False)


def _sched_cases(*axes):
    """parametrize arguments: the product of `axes` (first axis fastest) under sched "2" and "0".
    The default keeps the plain id, the other arm appends -sched0."""
    cases = [()]
    for ax in reversed(axes):
        cases = [(v if isinstance(v, tuple) else (v,)) + c for c in cases for v in ax]
    vals = [c + (s,) for s in ("2", "0") for c in cases]
    ids = ["-".join(map(str, c)) + ("" if s == "2" else "-sched0") for s in ("2", "0") for c in cases]
    return dict(argvalues=vals, ids=ids)


@pytest.mark.parametrize("Nn,K,T,cls,sched", **_sched_cases(WGRAD_P_NK, WGRAD_P_T, list(CLASSES)))
def test_linear_wgrad_p_exact(Nn, K, T, cls, sched, monkeypatch):
    """dna_linear_wgrad_p (sched "2": wgradp_kernel<2> in K-step pairs; "0": wgradp_kernel<0>, by
    default reached only past 2^31-byte chunks): odd and even step counts, T no multiple
    of 64, the smallest legal T, the library's chunk count and forced ones; the token rows past T
    that the pair kernel's last step covers lie in NaN-filled memory and must read as zeros."""
    _set_sched(monkeypatch, sched)
    g = _gen(Nn, K, T, cls == "b_wide", 3)
    amax, bmax = CLASSES[cls]
    dy, x = _head(_int_operand(T, Nn, amax, g)), _head(_int_operand(T, K, bmax, g))
    want = _exact_ref(dy.double().t(), x.double(), None, torch.float32)
    for s in _wgrad_p_splits(T, Nn, K):
        parts = _wgrad("dna_linear_wgrad_p", dy, x, s)
        _assert_same(parts.sum(0), want, what=f"dna_linear_wgrad_p T={T} N={Nn} K={K} splits={s} {cls}")


# ------------------------------------------------------------------ 3. permutation probes
def _normal_bf16(rows, cols, gen):
    """Arbitrary normal finite bf16: exponents uniform in [-100, 100], random 7-bit mantissas and
    signs (no inf / NaN / subnormal)."""
    e = torch.randint(-100, 101, (rows, cols), generator=gen) + 127
    m = torch.randint(0, 128, (rows, cols), generator=gen)
    s = torch.randint(0, 2, (rows, cols), generator=gen)
    bits = (s << 15) | (e << 7) | m
    bits = torch.where(bits >= 1 << 15, bits - (1 << 16), bits).to(torch.int16)
    t = bits.view(torch.bfloat16)
    assert bool(torch.isfinite(t.float()).all()) and float(t.float().abs().min()) >= 2.0 ** -101
    return t


def _one_hot(rows, cols, gen):
    hot = torch.randint(0, cols, (rows,), generator=gen)
    t = torch.zeros(rows, cols)
    t[torch.arange(rows), hot] = 1.0
    return t.bfloat16(), hot


def _perm_matrix(n, gen):
    """P[i, perm[i]] = 1."""
    perm = torch.randperm(n, generator=gen)
    t = torch.zeros(n, n)
    t[torch.arange(n), perm] = 1.0
    return t.bfloat16(), perm


@pytest.mark.parametrize("NK", [128, 192, 256])
def test_linear_fwd_dgrad_permutation_probes(NK):
    """Bit patterns beyond small integers, M = 300, no bias. Probe 1: w a permutation matrix, the
    other operand arbitrary normal bf16 -- the output is that operand with its columns permuted,
    bit for bit. Probe 2: the activation rows one-hot, w arbitrary -- the output rows are rows
    (forward: columns of w^T) of w."""
    M = 300
    g = _gen(NK, 4)
    x = _normal_bf16(M, NK, g)
    P, perm = _perm_matrix(NK, g)
    w = _normal_bf16(NK, NK, g)
    H, hot = _one_hot(M, NK, g)
    xd, Pd, wd, Hd = _head(x), _head(P), _head(w), _head(H)
    # forward y = x . w^T: y[m, n] = sum_k x[m, k] P[n, k] = x[m, perm[n]]
    _assert_same(_fwd(xd, Pd, None), xd[:, perm.to(DEV)], what=f"fwd permutation N=K={NK}")
    # y[m, n] = sum_k H[m, k] w[n, k] = w[n, hot[m]]
    _assert_same(_fwd(Hd, wd, None), wd[:, hot.to(DEV)].t().contiguous(), what=f"fwd one-hot N=K={NK}")
    # data gradient dx = dy . w: dx[m, perm[n]] = dy[m, n]
    want = torch.empty_like(xd)
    want[:, perm.to(DEV)] = xd
    _assert_same(_dgrad(xd, Pd), want, what=f"dgrad permutation N=K={NK}")
    # dx[m, k] = sum_n H[m, n] w[n, k] = w[hot[m], k]
    _assert_same(_dgrad(Hd, wd), wd[hot.to(DEV)], what=f"dgrad one-hot N=K={NK}")


@pytest.mark.parametrize("name,NK", [("dna_linear_wgrad", 128), ("dna_linear_wgrad", 192),
                                     ("dna_linear_wgrad", 256), ("dna_linear_wgrad_p", 256)])
def test_linear_wgrad_permutation_probes(name, NK):
    """The weight-gradient kernels with T = N = K tokens: dy a permutation matrix makes
    dW[perm[t], :] = x[t, :] (fp32 of arbitrary normal bf16 values, exact), x one makes
    dW[:, perm[t]] = dy[t, :]."""
    g = _gen(NK, 5, name.endswith("_p"))
    v = _normal_bf16(NK, NK, g)
    P, perm = _perm_matrix(NK, g)
    vd, Pd = _head(v), _head(P)
    want = torch.empty(NK, NK, device=DEV)
    want[perm.to(DEV)] = vd.float()
    _assert_same(_wgrad(name, Pd, vd, 1).sum(0), want, what=f"{name} dy permutation {NK}")
    want = torch.empty(NK, NK, device=DEV)
    want[:, perm.to(DEV)] = vd.float().t()
    _assert_same(_wgrad(name, vd, Pd, 1).sum(0), want, what=f"{name} x permutation {NK}")


# ------------------------------------------------------------------ 4. per-element fp64 bound
@pytest.mark.parametrize("path,shape", FWD_ALL, ids=FWD_IDS)
def test_linear_fwd_randn_elementwise(path, shape):
    """dna_linear_fwd on randn x, 0.05 randn w and a randn bias: every element within the derived
    bound of _bf16_bound of the fp64 result."""
    M, Nn, K = shape
    _check_path(path, M, Nn, K)
    g = _gen(M, Nn, K, 6)
    x = _head(torch.randn(M, K, generator=g).bfloat16())
    w = _head((torch.randn(Nn, K, generator=g) * 0.05).bfloat16())
    b = torch.randn(Nn, generator=g).to(DEV)
    got = _fwd(x, w, b)
    ref, bound = _bf16_bound(x.double(), w.double().t(), b.double(), K)
    _assert_within(got, ref, bound, what=f"dna_linear_fwd {path} M={M} N={Nn} K={K}")


@pytest.mark.parametrize("M,Nn,K", DGRAD)
def test_linear_dgrad_randn_elementwise(M, Nn, K):
    g = _gen(M, Nn, K, 7)
    dy = _head(torch.randn(M, Nn, generator=g).bfloat16())
    w = _head((torch.randn(Nn, K, generator=g) * 0.05).bfloat16())
    got = _dgrad(dy, w)
    ref, bound = _bf16_bound(dy.double(), w.double(), None, Nn)
    _assert_within(got, ref, bound, what=f"dna_linear_dgrad M={M} N={Nn} K={K}")


@pytest.mark.parametrize("steps", [1, 2, 3, 5])
@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("Nn,K", WGRAD_NK)
def test_linear_wgrad_randn_elementwise(Nn, K, splits, steps):
    """fp32 partials: the fp64 sum of the slices within (T + 2) 2^-23 sum_t |dy_t| |x_t|."""
    M = 64 * splits * steps
    g = _gen(Nn, K, splits, steps, 8)
    dy = _head(torch.randn(M, Nn, generator=g).bfloat16())
    x = _head(torch.randn(M, K, generator=g).bfloat16())
    parts = _wgrad("dna_linear_wgrad", dy, x, splits)
    ref, bound = _f32_bound(dy.double().t(), x.double(), M)
    _assert_within(parts.double().sum(0), ref, bound,
                   what=f"dna_linear_wgrad M={M} N={Nn} K={K} splits={splits}")


@pytest.mark.parametrize("Nn,K,T,sched", **_sched_cases(WGRAD_P_NK, WGRAD_P_T))
def test_linear_wgrad_p_randn_elementwise(Nn, K, T, sched, monkeypatch):
    _set_sched(monkeypatch, sched)
    g = _gen(Nn, K, T, 9)
    dy = _head(torch.randn(T, Nn, generator=g).bfloat16())
    x = _head(torch.randn(T, K, generator=g).bfloat16())
    ref, bound = _f32_bound(dy.double().t(), x.double(), T)
    for s in _wgrad_p_splits(T, Nn, K):
        parts = _wgrad("dna_linear_wgrad_p", dy, x, s)
        _assert_within(parts.double().sum(0), ref, bound,
                       what=f"dna_linear_wgrad_p T={T} N={Nn} K={K} splits={s}")


# ------------------------------------------------------------------ 5. fused epilogues
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M", [1, 300])
@pytest.mark.parametrize("path,K,F", [("p0", 192, 128), ("p0", 192, 384), ("np", 64, 128),
                                      ("p2", 128, 128)])
def test_geglu_linear_fwd_equals_unfused(path, K, F, M, p):
    """dna_geglu_linear_fwd on the odd-K/64 persistent body, the non-persistent kernel and KT = 2
    equals dna_linear_fwd + dna_geglu_fwd bit for bit (same Philox mask), and writes no row past
    M; with test_linear_fwd_exact the unfused pair is anchored to an exact root."""
    from test_gpu_kernels import _geglu_factors_match
    assert _fwd_path(F, K, wide=2 * F) == path
    g0 = _gen(K, F, M, 10)
    x = _head(torch.randn(M, K, generator=g0).bfloat16())
    wg = _head((torch.randn(2 * F, K, generator=g0) * 0.05).bfloat16())
    bg = (torch.randn(2 * F, generator=g0) * 0.1).to(DEV)
    fbuf, abuf = _out(M, 2 * F, torch.bfloat16), _out(M, F, torch.bfloat16)
    _call("dna_geglu_linear_fwd", x.data_ptr(), wg.data_ptr(), bg.data_ptr(), M, F, K, p, 11, 5,
          fbuf.data_ptr(), abuf.data_ptr())
    fac, a = _written(fbuf, M, "geglu fac"), _written(abuf, M, "geglu a")
    gl = _fwd(x, wg, bg)
    a2, fac2 = torch.empty_like(a), torch.empty_like(fac)
    _call("dna_geglu_fwd", gl.data_ptr(), 1, M, F, p, 11, 5, a2.data_ptr(), fac2.data_ptr())
    _assert_same(a, a2, tile=(256, 128), what=f"geglu fwd a {path} M={M} K={K} F={F} p={p}")
    _assert_same(fac, fac2, tile=(256, 128), what=f"geglu fwd fac {path} M={M} K={K} F={F} p={p}")
    _geglu_factors_match(gl, a, fac, p)


@pytest.mark.parametrize("M", [1, 300])
@pytest.mark.parametrize("F", [8, 136])
@pytest.mark.parametrize("H", [64, 192])
def test_geglu_linear_dgrad_equals_unfused(H, F, M):
    """dna_geglu_linear_dgrad (gemm_kernel<true, false, EPI_GEGLU_BWD>) equals dna_linear_dgrad +
    dna_geglu_bwd bit for bit at one and three K-steps and F off the tile."""
    from test_gpu_kernels import _random_factors
    g0 = _gen(H, F, M, 11)
    dy = _head(torch.randn(M, H, generator=g0).bfloat16())
    wo = _head((torch.randn(H, F, generator=g0) * 0.05).bfloat16())
    fac = _head(_random_factors(M, F, g0))
    buf = _out(M, 2 * F, torch.bfloat16)
    _call("dna_geglu_linear_dgrad", dy.data_ptr(), wo.data_ptr(), fac.data_ptr(), M, F, H,
          buf.data_ptr())
    dg = _written(buf, M, "dna_geglu_linear_dgrad")
    da = _dgrad(dy, wo)
    dg2 = torch.empty_like(dg)
    _call("dna_geglu_bwd", da.data_ptr(), fac.data_ptr(), 1, M, F, dg2.data_ptr())
    _assert_same(dg, dg2, what=f"dna_geglu_linear_dgrad M={M} H={H} F={F}")


@pytest.mark.parametrize("M", [1, 257])
def test_geglu_linear_dgrad_p_kt2_equals_pair(M):
    """dna_geglu_linear_dgrad_p at two K-steps (hidden = 128, F = 256) equals dna_linear_fwd on the
    transposed weight + dna_geglu_bwd bit for bit and writes nothing past M."""
    from test_gpu_kernels import _geglu_dgrad_pair, _random_factors
    F, H = 256, 128
    gen = _gen(M, 12)
    dy = _head(torch.randn(M, H, generator=gen).bfloat16())
    wt = _head((torch.randn(F, H, generator=gen) * 0.05).bfloat16())
    fac = _head(_random_factors(M, F, gen))
    buf = _out(M, 2 * F, torch.bfloat16)
    _call("dna_geglu_linear_dgrad_p", dy.data_ptr(), wt.data_ptr(), fac.data_ptr(), M, F, H,
          buf.data_ptr())
    dg = _written(buf, M, "dna_geglu_linear_dgrad_p")
    _assert_same(dg, _geglu_dgrad_pair(dy, wt, fac, M, F, H), what=f"dna_geglu_linear_dgrad_p M={M}")


@pytest.mark.parametrize("M", [1, 257])
def test_gelu_linear_dgrad_p_kt2_vs_unfused(M):
    """functional.GeluLinear's backward at two K-steps (fc2 [128, 256]: dna_gelu_linear_dgrad_p,
    hidden = 128, F = 256) against its unfused form -- da = dy . w through dna_linear_fwd on the
    transposed weight copy (exact-anchored above), then torch's tanh-GELU backward of the bf16 da
    -- within bf16 rounding (the criterion of test_gelu_linear_fused_bwd_vs_separate); the raw
    kernel gives the node's dh bit for bit and writes no row past M."""
    from dna_amd import functional as DF
    F, Nn = 256, 128
    g = _gen(M, 13)
    h = (torch.randn(M, F, generator=g) * 2).to(DEV).bfloat16()
    w = (torch.randn(Nn, F, generator=g) / F ** 0.5).to(DEV)
    b = torch.randn(Nn, generator=g).to(DEV) * 0.1
    do = torch.randn(M, Nn, generator=g).to(DEV).bfloat16()
    hh = h.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        o = DF.gelu_linear(hh, w.clone().requires_grad_(True), b.clone().requires_grad_(True))
    o.backward(do)
    dh1 = hh.grad
    assert dh1.dtype == torch.bfloat16 and torch.isfinite(dh1.float()).all()
    hd, wt = _head(h), _head(w.bfloat16().t().contiguous())
    buf = _out(M, F, torch.bfloat16)
    _call("dna_gelu_linear_dgrad_p", do.data_ptr(), wt.data_ptr(), hd.data_ptr(), M, F, Nn,
          buf.data_ptr())
    _assert_same(_written(buf, M, "dna_gelu_linear_dgrad_p"), dh1, what=f"dna_gelu_linear_dgrad_p M={M}")
    da = _fwd(_head(do), wt, None)
    h32 = h.float().requires_grad_(True)
    torch.nn.functional.gelu(h32, approximate="tanh").backward(da.float())
    dh2 = h32.grad
    err = (dh1.float() - dh2).abs().max().item()
    assert err <= 1e-2 * dh2.abs().max().item(), err
