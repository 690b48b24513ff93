"""Shared checker of the FFT long-convolution tests (a plain helper module, not a conftest).

Four parts:
  * inputs: u, dy ~ N(0,1), k = N(0,1) * exp(-linspace(0, 3, L)), bias ~ N(0,1), every row and
    channel O(1). (The kernels pack two batch rows, and two filter channels, into one complex
    sequence: rounding error at the larger one's scale legitimately reaches the smaller one, so
    rows of widely different scales would measure the packing, not a fault. The GPU tests
    measure that cross-talk on its own.)
  * oracle64: the float64 numpy restatement (oracle/hyena_ref.py), out / du / dk / dbias.
  * ref32: the same four results in float32 with torch.fft on the CPU (rfft at n = 2L, the same
    padding and pad_before, norm="forward"). Its own worst-row error against oracle64, e32, is
    the yardstick of the bounds: what a plain fp32 FFT of this formula loses. The kernel under
    test never is.
  * row_figures / assert_close: max_t |got - ref64| / max_t |ref64| of every row -- (b, d) for
    out and du, d for dk -- over every t < L, the worst row reported.

Bounds.
  fp32: a row stays within F32_FACTOR x e32 of its maximum. The kernels' twiddles are products of
    two rounded table values where pocketfft's are one rounding from exact, and they fold 1/N and
    the bias tap into the filter spectrum: a small multiple of e32 is expected, an order of
    magnitude is not -- 4 x ~2.5e-7 = 1e-6 is the twiddle-recurrence regression DESIGN.md
    records. The project's older 2e-5 stays as an outer cap on the same figure.
  bf16: u and dy are rounded to bf16 before the oracle sees them; out and du, written in bf16,
    get per element 2^-8 |ref| (one rounding to nearest) + the fp32 bound x row maximum; dk and
    dbias are fp32 outputs and keep the fp32 bounds.
  dbias: from dbias_kernel's summation order, see dbias_terms.
No GPU code here: tests/test_fft_check_host.py runs all of it on the CPU.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from oracle import hyena_ref as H

F32_FACTOR = 4.0      # x e32
OUTER_CAP = 2e-5      # tests/test_gpu_hyena.py's bound, here per row
BF16_REL = 2.0 ** -8  # one rounding to nearest of a bf16 value (8 significant bits)
U24 = 2.0 ** -24      # unit roundoff of fp32

# name -> axes the row maximum is taken over
ROW_AXES = {"out": (2,), "du": (2,), "dk": (1,)}
NAMES = ("out", "du", "dk", "dbias")
BF16_WRITTEN = ("out", "du")
PLAN_KEYS = ("logN", "logM1", "logM2", "fixed_ln", "col_group", "row_group", "rowbwd_group")


def plan(L):
    """dna_fftconv_plan: the geometry and instantiation the library takes for L, as a dict of
    PLAN_KEYS (the three groups as log2). Host code only."""
    from dna_amd import _native as N
    out = (ctypes.c_int * len(PLAN_KEYS))(*([-1] * len(PLAN_KEYS)))
    N.call("dna_fftconv_plan", L, ctypes.cast(out, ctypes.c_void_p))
    return dict(zip(PLAN_KEYS, (int(v) for v in out)))


def seed_for(B, D, L, bidirectional):
    return 1000003 * D + 7919 * B + 2 * L + int(bool(bidirectional))


def inputs(B, D, L, bidirectional, seed):
    """fp32 CPU tensors u, dy [B, D, L], k [D, L], bias [D, 1] (bidirectional only enters the
    caller's seed: the draw is the same for both directions)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    u, dy = rn(B, D, L), rn(B, D, L)
    k = rn(D, L) * torch.exp(-torch.linspace(0, 3, L))[None]
    return {"u": u, "dy": dy, "k": k.contiguous(), "bias": rn(D, 1)}


def rounded(inp, dtype):
    """The inputs as a run in `dtype` sees them: u and dy rounded to it (k, bias stay fp32)."""
    if dtype == torch.float32:
        return dict(inp)
    return {k: (v.to(dtype).float() if k in ("u", "dy") else v) for k, v in inp.items()}


def oracle64(inp, bidirectional):
    """float64 reference: out, du [B, D, L], dk [D, L], dbias [D] (numpy)."""
    a = {k: v.detach().cpu().numpy() for k, v in inp.items()}
    out = H.fftconv_fwd(a["u"], a["k"], a["bias"], bidirectional)
    du, dk, db = H.fftconv_bwd(a["dy"], a["u"], a["k"], a["bias"], bidirectional)
    return {"out": out, "du": du, "dk": dk, "dbias": db.reshape(-1)}


def ref32(inp, bidirectional):
    """The formula of oracle/hyena_ref.py in float32 with torch.fft on the CPU."""
    u, dy, k, bias = (inp[n].detach().cpu().float() for n in ("u", "dy", "k", "bias"))
    L = u.shape[-1]
    N = 2 * L
    pb = H.pad_before(L, bidirectional)
    kf = torch.fft.rfft(k, n=N) / N
    uf = torch.fft.rfft(F.pad(u, (pb, N - L - pb)), n=N)
    dyf = torch.fft.rfft(dy, n=N)
    out = torch.fft.irfft(uf * kf, n=N, norm="forward")[..., :L] + u * bias
    du = torch.fft.irfft(dyf * kf.conj(), n=N, norm="forward")[..., pb:pb + L] + dy * bias
    dk = (torch.fft.irfft(dyf * uf.conj(), n=N, norm="forward")[..., :L] / N).sum(0)
    dbias = (dy * u).sum((0, 2))
    assert out.dtype == du.dtype == dk.dtype == dbias.dtype == torch.float32
    return {"out": out.numpy(), "du": du.numpy(), "dk": dk.numpy(), "dbias": dbias.numpy()}


def row_figures(name, got, ref):
    """Per row: max_t |got - ref| / max_t |ref|, every t < L (a non-finite element counts as
    infinite; a row whose reference is all zero has no scale and any error there is infinite)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    axes = ROW_AXES[name]
    err = np.abs(got - ref)
    err[~np.isfinite(err)] = np.inf
    return err.max(axis=axes) / (np.abs(ref).max(axis=axes) + 1e-300)


# dbias_kernel's launch constants (dna_amd/csrc/fftconv.hip): NTH threads per block, DB_CHUNKS
# blocks per channel, 64-lane waves
_DB_NTH, _DB_CHUNKS, _DB_WAVE = 512, 32, 64


def dbias_terms(B, L):
    """m such that |dbias - exact| <= gamma_m * sum |dy u| per channel, gamma_m = m u / (1 - m u),
    u = 2^-24, from dbias_kernel's summation order. A sum evaluated in any fixed order obeys
    |err| <= gamma_h * sum |terms| with h the largest number of roundings on the path of one term
    to the result (Higham, Accuracy and Stability of Numerical Algorithms, 4.2). One term's path:
      * its product (1 rounding; none for bf16 operands, whose product is exact in fp32) and the
        thread's running sum `s +=` over its n_t elements (n_t - 1 further additions, the first
        into 0 being exact): n_t. A chunk holds per = ceil(B L / 32) elements (rounded up to the
        vector width VE = 4 / 8 on the 16-byte paths); a thread takes VE consecutive ones every
        512 VE, so n_t <= VE * ceil(ceil(per / VE) / 512), the largest over VE = 1, 4, 8;
      * wave_sum, a butterfly of log2(64) = 6 additions;
      * the sum of the 8 waves' results in order (the first into 0 exact): 7;
      * dbias_final, the sum of the 32 chunks in order: 31.
    Zero-filled tail elements add nothing. m = n_t + 44."""
    per = -(-B * L // _DB_CHUNKS)
    n_t = max(ve * -(-(-(-per // ve)) // _DB_NTH) for ve in (1, 4, 8))
    return n_t + 6 + (_DB_NTH // _DB_WAVE - 1) + (_DB_CHUNKS - 1)


def reference(B, D, L, bidirectional, dtype=torch.float32, seed=None):
    """(inputs as a run in `dtype` sees them, float64 reference, e32) of one case. e32 maps out /
    du / dk to ref32's worst-row figure and "dbias" to (m, sum |dy u| per channel)."""
    seed = seed_for(B, D, L, bidirectional) if seed is None else seed
    inp = rounded(inputs(B, D, L, bidirectional, seed), dtype)
    return (inp,) + reference_of(inp, bidirectional)


def reference_of(inp, bidirectional):
    ref = oracle64(inp, bidirectional)
    r32 = ref32(inp, bidirectional)
    e32 = {n: float(row_figures(n, r32[n], ref[n]).max()) for n in ROW_AXES}
    B, _, L = inp["u"].shape
    e32["dbias"] = (dbias_terms(B, L),
                    (inp["dy"].double() * inp["u"].double()).abs().sum((0, 2)).numpy())
    return ref, e32


def fp32_bound(e32, factor=F32_FACTOR):
    return min(factor * e32, OUTER_CAP)


def assert_close(name, got, ref64, e32, dtype=torch.float32, report=None, factor=F32_FACTOR):
    """Every row of `got` within its bound of `ref64`; the message names the tensor and the worst
    row. `e32` is ref32's worst-row figure for this case and tensor (for dbias: the pair from
    reference()). `report`, a dict, receives name -> the worst row's figure before anything
    asserts: max |err| / row maximum for an fp32 output, the largest share of its per-element
    allowance that an element uses for a bf16-written one, and |err| / (2^-24 sum |dy u|) for
    dbias (to be read against m)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if name == "dbias":
        m, abssum = e32
        err = np.abs(got - ref)
        err[~np.isfinite(err)] = np.inf
        units = err / (U24 * abssum + 1e-300)
        worst = int(np.argmax(units))
        if report is not None:
            report[name] = float(units[worst])
        allowed = m / (1.0 - m * U24)
        assert units[worst] <= allowed, (
            f"dbias: row ({worst},) of {units.shape} is off by {units[worst]:.3g} x 2^-24 sum|dy u|, "
            f"over the {m} roundings of dbias_kernel's summation order")
        return
    bound = fp32_bound(e32, factor)
    axes = ROW_AXES[name]
    aref = np.abs(ref)
    allow = aref.max(axis=axes, keepdims=True) * bound + 1e-300
    rel = BF16_REL if (dtype == torch.bfloat16 and name in BF16_WRITTEN) else 0.0
    if rel:
        allow = allow + rel * aref
    err = np.abs(got - ref)
    err[~np.isfinite(err)] = np.inf
    r = np.atleast_1d((err / allow).max(axis=axes))
    worst = np.unravel_index(int(np.argmax(r)), r.shape)
    if report is not None:
        report[name] = float(r[worst]) * (1.0 if rel else bound)
    assert r[worst] <= 1.0, (
        f"{name}: row {tuple(int(i) for i in worst)} of {r.shape} is {r[worst]:.3g}x its bound "
        f"(row bound {bound:.3g} = min({factor:g} x e32 {e32:.3g}, {OUTER_CAP:g}), per-element "
        f"relative allowance {rel:g}, {int((r > 1).sum())} rows over)")


def check_all(got, ref64, e32, dtype=torch.float32, factor=None):
    """assert_close on every tensor in `got`, all figures collected first: (report, failures).
    `factor`: name -> multiple of e32 for the tensors that do not take F32_FACTOR."""
    report, failures = {}, []
    for name in NAMES:
        if name not in got:
            continue
        try:
            assert_close(name, got[name], ref64[name], e32[name], dtype, report,
                         (factor or {}).get(name, F32_FACTOR))
        except AssertionError as e:
            failures.append(str(e))
    return report, failures


def line(label, shape, bidirectional, dtype, report, e32):
    """FFTPATH <label> BxDxL bi=.. dtype fwd .. du .. dk .. dbias ..: each figure with its ratio
    to e32 (bf16-written: the share of the allowance used; dbias: its error in units of
    2^-24 sum |dy u| over the m it may reach)."""
    dt = {torch.float32: "fp32", torch.bfloat16: "bf16"}[dtype]
    parts = []
    for name, tag in zip(NAMES, ("fwd", "du", "dk", "dbias")):
        if name not in report:
            parts.append(f"{tag} -")
        elif name == "dbias":
            parts.append(f"{tag} {report[name]:.2f}u/{e32[name][0]}u")
        elif dtype == torch.bfloat16 and name in BF16_WRITTEN:
            parts.append(f"{tag} {report[name]:.3f} of its allowance (e32 {e32[name]:.2e})")
        else:
            parts.append(f"{tag} {report[name]:.2e} ({report[name] / e32[name]:.2f}x e32 {e32[name]:.2e})")
    return (f"FFTPATH {label} {'x'.join(map(str, shape))} bi={int(bool(bidirectional))} {dt} "
            + " ".join(parts))
