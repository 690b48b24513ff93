"""Shared checker of the selective-scan tests (a plain helper module, not a conftest).

Three parts:
  * long_memory_inputs: inputs in Mamba's production regime -- per-channel steps of 1e-3 .. 3e-3
    and A = -(n+1), so state 0 decays by about e^-1 over a 512-position chunk and a chunk's
    output depends on many chunks before it. (The older scan tests draw steps near 0.3: a chunk
    then decays the state by e^-150 and every chunk carry is numerically invisible.)
  * oracle: the float64 C restatement (oracle/selective_scan_c.py), forward and backward, split
    over (batch row, channel slice) jobs in a thread pool (ctypes releases the GIL).
  * row_ratios / assert_close: the error of every (b, d) row, (b, n) row or d row against that
    row's own maximum, so that a fault confined to one small channel or state row cannot hide
    behind the tensor's global maximum.
No GPU code here: tests/test_scan_check_host.py runs all of it on the CPU.
"""
import ctypes
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

CHUNK = 512  # positions per chunk of the kernels under test (mutants below cut at its multiples)

# name -> axes the row maximum is taken over (None: the whole tensor is one row)
ROW_AXES = {"out": (2,), "last_state": (2,), "u": (2,), "delta": (2,), "z": (2,),
            "B": (2,), "C": (2,), "A": (1,), "D": None, "delta_bias": None}
FORWARD = ("out", "last_state")
# the project's fp32 bounds (tests/test_gpu_selective_scan.py), here applied per row
FP32_BOUND = {name: (1e-4 if name in FORWARD else 1e-3) for name in ROW_AXES}
# tensors the kernels (or SelectiveScan.backward's cast) round to bf16 in a bf16 run; the rest
# (last_state, dA, dD, ddelta_bias) stay fp32 and keep the fp32 bound
BF16_WRITTEN = ("out", "u", "delta", "z", "B", "C")
# per-element relative allowance of a bf16-written tensor. bf16 keeps 8 significant bits, so one
# rounding to nearest is up to 2^-8 relative (just above a power of two): this term is exactly
# one rounding, and the margin of a bf16 run is the fp32 bound x row maximum added to it
BF16_REL = 2.0 ** -8
ROUNDED_INPUTS = ("u", "delta", "B", "C", "z", "dout")


def plan(b, d, l, n):
    """dna_selective_scan_plan: the dispatch the library takes for a shape, as a dict with
    chunked (bool), k, nch, carry_par (bool). Host code only."""
    from dna_amd import _native as N
    vals = [ctypes.c_int(-1) for _ in range(4)]
    N.call("dna_selective_scan_plan", b, d, l, n, *(ctypes.byref(v) for v in vals))
    chunked, k, nch, carry_par = (v.value for v in vals)
    return {"chunked": bool(chunked), "k": k, "nch": nch, "carry_par": bool(carry_par)}


def _softplus_inv(dt):
    return torch.log(torch.expm1(dt))


def long_memory_inputs(b, d, l, n, seed, softplus=True, bias=True):
    """fp32 CPU tensors u, delta, A, B, C, D, z, delta_bias, dout whose effective step
    softplus(delta + delta_bias) is dt[d] * exp(0.5 randn), dt log-uniform in [1e-3, 3e-3].
    (At dt = 4e-3 a channel forgets two chunks down to about 1e-2 of its row maximum, which is
    10x the gradient bound: too close for the mutants of tests/test_scan_check_host.py.)

    bias=False folds softplus^-1(dt) into delta (delta_bias is then None). softplus=False is the
    delta_softplus=False variant: delta is the already-positive step itself, and delta_bias, when
    wanted, a further 0.25 dt."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    dt = torch.exp(torch.rand(d, generator=g, dtype=torch.float64) * math.log(3.0) + math.log(1e-3))
    shift = _softplus_inv(dt)  # float64 [d]
    noise = 0.5 * rn(b, d, l)
    if softplus:
        delta = noise if bias else (noise.double() + shift[None, :, None]).float()
        delta_bias = shift.float() if bias else None
    else:
        delta = torch.nn.functional.softplus(noise.double() + shift[None, :, None]).float()
        delta_bias = (0.25 * dt).float() if bias else None
    A = (-(torch.arange(n, dtype=torch.float32) + 1.0)[None, :] * torch.exp(0.1 * rn(d, n)))
    return {"u": rn(b, d, l), "delta": delta, "A": A.contiguous(), "B": rn(b, n, l),
            "C": rn(b, n, l), "D": 0.1 * rn(d), "z": rn(b, d, l), "delta_bias": delta_bias,
            "dout": rn(b, d, l)}


def rounded(inp, dtype):
    """The inputs as a run in `dtype` sees them: u, delta, B, C, z, dout rounded to it."""
    if dtype == torch.float32:
        return dict(inp)
    return {k: (v.to(dtype).float() if (v is not None and k in ROUNDED_INPUTS) else v)
            for k, v in inp.items()}


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _jobs(b, d, threads):
    """(batch row, channel slice) jobs: enough of them to keep `threads` workers busy."""
    per_row = min(d, max(1, -(-2 * threads // b)))
    edges = np.linspace(0, d, per_row + 1).astype(int)
    return [(bi, int(edges[i]), int(edges[i + 1])) for bi in range(b) for i in range(per_row)
            if edges[i + 1] > edges[i]]


def oracle(inp, softplus=True, threads=16, backward=True):
    """float64 reference of forward (out, last_state) and, with dout, every gradient (keys u,
    delta, A, B, C and D, z, delta_bias when given) as a dict of numpy arrays. threads=1 is the
    unsplit call."""
    from oracle.selective_scan_c import scan_bwd, scan_fwd
    a = {k: _np(v) for k, v in inp.items()}
    b, d, l = a["u"].shape
    n = a["A"].shape[1]
    backward = backward and a.get("dout") is not None
    threads = max(1, min(threads, 16, os.cpu_count() or 1))
    jobs = [(0, 0, d)] if threads == 1 else _jobs(b, d, threads)
    rows = 1 if threads == 1 else None

    def run(job):
        bi, d0, d1 = job
        bs = slice(0, b) if rows else slice(bi, bi + 1)
        ds = slice(d0, d1)
        opt = lambda k, s: None if a.get(k) is None else a[k][s]
        kw = dict(D=opt("D", ds), z=opt("z", (bs, ds)), delta_bias=opt("delta_bias", ds),
                  delta_softplus=softplus)
        args = (a["u"][bs, ds], a["delta"][bs, ds], a["A"][ds], a["B"][bs], a["C"][bs])
        out, last = scan_fwd(*args, **kw)
        g = scan_bwd(*args, a["dout"][bs, ds], **kw) if backward else {}
        return out, last, g

    with ThreadPoolExecutor(max_workers=min(threads, len(jobs))) as pool:
        results = list(pool.map(run, jobs))
    ref = {"out": np.empty((b, d, l)), "last_state": np.empty((b, d, n))}
    if backward:
        for k in ("u", "delta") + (("z",) if a.get("z") is not None else ()):
            ref[k] = np.empty((b, d, l))
        ref["A"] = np.zeros((d, n))
        ref["B"], ref["C"] = np.zeros((b, n, l)), np.zeros((b, n, l))
        for k in ("D", "delta_bias"):
            if a.get(k) is not None:
                ref[k] = np.zeros(d)
    for (bi, d0, d1), (out, last, g) in zip(jobs, results):
        bs = slice(0, b) if rows else slice(bi, bi + 1)
        ref["out"][bs, d0:d1], ref["last_state"][bs, d0:d1] = out, last
        for k, v in g.items():
            if k in ("u", "delta", "z"):
                ref[k][bs, d0:d1] = v
            elif k in ("B", "C"):
                ref[k][bs] += v       # summed over the channel slices of a batch row
            else:
                ref[k][d0:d1] += v    # A, D, delta_bias: summed over the batch rows
    return ref


def windowed(inp, softplus, name, before, after):
    """A reference with a short memory, chunk by chunk: chunk [s, e) is evaluated on the window
    [s - before*CHUNK, e + after*CHUNK) alone (zero state at the window's left end, zero adjoint
    at its right end) and restricted to [s, e). `name` is "out" or a gradient key.
    (before, after) = (1, 0) forgets everything older than the previous chunk; (0, 0) is a kernel
    whose chunk carries are all zero; (0, 1) is a backward that remembers one chunk."""
    l = inp["u"].shape[2]
    parts = []
    for s in range(0, l, CHUNK):
        e = min(s + CHUNK, l)
        w0, w1 = max(0, s - before * CHUNK), min(l, e + after * CHUNK)
        win = {k: (v[..., w0:w1].contiguous() if (v is not None and v.dim() == 3) else v)
               for k, v in inp.items()}
        ref = oracle(win, softplus, threads=1, backward=name != "out")
        parts.append(ref[name][..., s - w0:e - w0])
    return np.concatenate(parts, axis=-1)


def bounds_for(name, dtype, fp32_bound=None):
    """(row bound, per-element relative allowance) of tensor `name` in a run in `dtype`."""
    fb = (fp32_bound or {}).get(name, FP32_BOUND[name])
    rel = BF16_REL if (dtype == torch.bfloat16 and name in BF16_WRITTEN) else 0.0
    return fb, rel


def row_ratios(name, got, ref, dtype=torch.float32, fp32_bound=None):
    """Per row: max over the row of |err| / (rel * |ref| + bound * max over the row of |ref|).
    A row passes at <= 1. With rel = 0 (every fp32 tensor) this is the row's max |err| over its
    max |ref|, in units of the bound."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bound, rel = bounds_for(name, dtype, fp32_bound)
    axes = ROW_AXES[name]
    if axes is None:
        axes = tuple(range(ref.ndim))
    aref = np.abs(ref)
    rowmax = aref.max(axis=axes, keepdims=True)
    allow = rowmax * bound + 1e-300
    if rel:
        allow = allow + rel * aref
    err = np.abs(got - ref)
    err[~np.isfinite(err)] = np.inf
    return (err / allow).max(axis=axes)


def assert_close(name, got, ref, dtype=torch.float32, fp32_bound=None, report=None):
    """Every row of `got` within its bound of `ref`; the message names the worst row. `report`,
    a dict, collects name -> worst ratio * bound (the worst row error for an fp32 tensor)."""
    r = np.atleast_1d(row_ratios(name, got, ref, dtype, fp32_bound))
    worst = np.unravel_index(int(np.argmax(r)), r.shape)
    bound, rel = bounds_for(name, dtype, fp32_bound)
    if report is not None:
        report[name] = float(r[worst]) * bound
    assert r[worst] <= 1.0, (
        f"{name}: row {tuple(int(i) for i in worst)} of {r.shape} is {r[worst]:.3g}x its bound "
        f"(row bound {bound:g}, per-element relative allowance {rel:g}, "
        f"{int((r > 1).sum())} rows over)")


def seed_for(b, d, l, n):
    return 1000003 * n + 7919 * d + 31 * b + l


# The shapes of tests/test_gpu_selective_scan_paths.py, by the path each is there for (the GPU
# tests assert the path through plan(); tests/test_scan_check_host.py pins plan() at the
# thresholds and checks that the inputs of the affordable ones reject short-memory mutants).
PER_CHANNEL = [(2, 5, 4104, 16), (1, 3, 1547, 8), (1, 6, 1030, 4)]
MATRIX = [(2, 8, l, n) for n in (4, 8, 16) for l in (4104, 4099)]   # VEC / not VEC
CARRY_BLK_PER = [(1, 8, 8712, 16), (1, 8, 33288, 4)]                # nch = 18, 66
K_WAVE = [(2, (8, 2064, 520, 16)), (4, (16, 2080, 520, 8)), (8, (16, 4096, 520, 4)),
          (8, (16, 4096, 517, 4))]
CARRY_PAR = [(1, 8, 478216, 16), (1, 8, 1625096, 4)]                # nch = 935, 3175
OPTIONAL = [(2, 8, 1032, 16), (2, 5, 1032, 16)]
