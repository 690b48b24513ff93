"""GPU: every dispatch path of dna_amd/csrc/fftconv.hip against the float64 oracle
(oracle/hyena_ref.py), forward and the backward of u, k and bias, with the error taken per row
(tests/fft_check.py). Each case asserts through dna_fftconv_plan that its length takes the
geometry or instantiation it is named for.

Bounds (fft_check.assert_close): fp32 -- every row within 4 x e32 of its maximum, e32 being what
a plain fp32 torch.fft evaluation of the same formula loses on the same inputs (never above the
older 2e-5); bf16 -- against the oracle on the bf16-rounded inputs, per element 2^-8 |ref| + the
fp32 bound x row maximum for out and du, the fp32 bound for dk; dbias -- the rounding bound of
dbias_kernel's summation order (fft_check.dbias_terms). The measured figures are in DESIGN.md
("FFT long convolution: dispatch paths under test")."""
import math

import numpy as np
import pytest
import torch

from tests import fft_check as FC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
_DT = {F32: "fp32", BF16: "bf16"}
_DNA = {F32: 0, BF16: 1}
_refs = {}
GRADS = ("du", "dk", "dbias")


def _ids(v):
    return _DT.get(v) or ("x".join(map(str, v)) if isinstance(v, tuple) else str(v))


def _reference(B, D, L, bi, dtype):
    """(inputs as the run sees them, float64 reference, e32), computed once per case."""
    key = (B, D, L, bi, dtype)
    if key not in _refs:
        _refs[key] = FC.reference(B, D, L, bi, dtype)
    return _refs[key]


def _expect_plan(L):
    """The geometry a length is there for: M1 = 2 up to L = 512, M2 = 512 from there on, the
    compile-time instantiations at the top three sizes and the generic kernels below."""
    p = FC.plan(L)
    assert (1 << p["logN"]) == 2 * L
    assert (p["logM1"] == 1) == (L <= 512)
    assert (p["logM2"] == 9) == (L >= 512)
    assert p["fixed_ln"] == {32768: 16, 65536: 17, 131072: 18}.get(L, 0)
    return p


def _verify(label, inp, ref, e32, bi, dtype, got):
    report, failures = FC.check_all(got, ref, e32, dtype)
    print(FC.line(label, tuple(inp["u"].shape), bi, dtype, report, e32))
    assert not failures, "\n".join(failures)
    return report


# ---------------------------------------------------------------- through the wrapper

def _wrapper(inp, bi, dtype, need=("u", "k", "bias")):
    """dna_amd.hyena.fftconv forward + backward with requires_grad on `need`: out and the
    gradients it produced (the others must be None)."""
    from dna_amd.hyena import fftconv
    u = inp["u"].to(DEV, dtype).requires_grad_("u" in need)
    k = inp["k"].to(DEV).requires_grad_("k" in need)
    bias = inp["bias"].to(DEV).requires_grad_("bias" in need)
    assert u.data_ptr() % 16 == 0
    y = fftconv(u, k, bias, bidirectional=bi)
    assert y.shape == u.shape and y.dtype == dtype
    y.backward(inp["dy"].to(DEV, dtype))
    torch.cuda.synchronize()
    got = {"out": y.detach().float().cpu().numpy()}
    for name, t, key in (("u", u, "du"), ("k", k, "dk"), ("bias", bias, "dbias")):
        if name in need:
            assert t.grad is not None and t.grad.dtype == t.dtype and t.grad.shape == t.shape, name
            got[key] = t.grad.float().cpu().numpy().reshape(ref_shape(inp, key))
        else:
            assert t.grad is None, f"{name} got a gradient nobody asked for"
    return got


def ref_shape(inp, key):
    B, D, L = inp["u"].shape
    return {"du": (B, D, L), "dk": (D, L), "dbias": (D,)}[key]


@pytest.mark.parametrize("bi", [False, True], ids=["causal", "bidir"])
@pytest.mark.parametrize("L", [1 << e for e in range(6, 18)])
def test_every_size_fp32(L, bi):
    """(a) L = 2^6 .. 2^17, B = 3 (one full pair + one unpaired row), D = 3 (one filter pair + one
    unpaired channel), every gradient."""
    p = _expect_plan(L)
    inp, ref, e32 = _reference(3, 3, L, bi, F32)
    got = _wrapper(inp, bi, F32)
    _verify(f"size logN={p['logN']} M1=2^{p['logM1']} M2=2^{p['logM2']} ln={p['fixed_ln']}",
            inp, ref, e32, bi, F32, got)


@pytest.mark.parametrize("bi", [False, True], ids=["causal", "bidir"])
@pytest.mark.parametrize("L", [64, 512, 2048, 32768, 65536, 131072])
def test_bf16_forward_and_backward(L, bi):
    """(b) bf16 u / dy / y / du: the 8-wide 16-byte loads and stores of the fixed-size kernels and
    of dbias_kernel<bf16>, and the generic kernels' bf16 element path."""
    p = _expect_plan(L)
    inp, ref, e32 = _reference(3, 3, L, bi, BF16)
    got = _wrapper(inp, bi, BF16)
    _verify(f"bf16 logN={p['logN']} ln={p['fixed_ln']}", inp, ref, e32, bi, BF16, got)


_SUBSETS = {"u_only": ("u",), "k_only": ("k",), "k_bias": ("k", "bias"), "u_bias": ("u", "bias")}


@pytest.mark.parametrize("need", list(_SUBSETS))
@pytest.mark.parametrize("L", [1024, 65536])
def test_gradient_subsets(L, need):
    """(d) u only: no saved spectrum, row_bwd_kernel<false,true>; k only: <true,false>; with and
    without dbias. Gradients not asked for are None."""
    _expect_plan(L)
    bi = True
    inp, ref, e32 = _reference(3, 3, L, bi, F32)
    full = _wrapper(inp, bi, F32)
    got = _wrapper(inp, bi, F32, _SUBSETS[need])
    assert set(got) == {"out"} | {{"u": "du", "k": "dk", "bias": "dbias"}[n] for n in _SUBSETS[need]}
    same = {n: bool(np.array_equal(got[n], full[n])) for n in got}
    print(f"FFTPATH subset {need} L={L} bit-identical to the all-gradients run: {same}")
    _verify(f"subset {need}", inp, ref, e32, bi, F32, got)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
@pytest.mark.parametrize("L", [64, 1024])
@pytest.mark.parametrize("B,D", [(1, 1), (1, 2), (2, 1), (5, 2), (6, 3)])
def test_batch_and_channel_edges(B, D, L, dtype):
    """(f) B = 1: every pair unpaired; B = 5, 6: BP = 3 turns of row_bwd_kernel's pair loop with
    and without an unpaired tail; D = 1: the filter has no second channel (has_b false)."""
    _expect_plan(L)
    for bi in (False, True):
        inp, ref, e32 = _reference(B, D, L, bi, dtype)
        _verify(f"edge BP={(B + 1) // 2}", inp, ref, e32, bi, dtype, _wrapper(inp, bi, dtype))


# ---------------------------------------------------------------- the C entry points directly

_SENT32, _SENT16, _SENT8 = 0x5A5AA5A5, 0x5A5A, 0xA5
_INT = {4: torch.int32, 2: torch.int16, 1: torch.uint8}
_SENT = {4: _SENT32, 2: _SENT16, 1: _SENT8}


class _Buf:
    """A contiguous view `v` of `shape` that starts `lead` elements into a larger storage with
    `tail` elements after it. Outputs: the whole storage holds a sentinel bit pattern and the
    view NaN; inputs: the view holds the values and everything around it NaN."""

    def __init__(self, shape, dtype, lead=0, tail=0, values=None):
        n = math.prod(shape)
        self.store = torch.empty(lead + n + tail, device=DEV, dtype=dtype)
        self.bits = self.store.view(_INT[self.store.element_size()])
        self.lo, self.hi = lead, lead + n
        self.v = self.store[lead:lead + n].view(shape)
        if values is None:
            self.bits.fill_(_SENT[self.store.element_size()])
            if dtype != torch.uint8:
                self.v.fill_(float("nan"))
        else:
            self.store.fill_(float("nan"))
            self.v.copy_(values)
        assert self.v.is_contiguous()

    def ptr(self):
        return self.v.data_ptr()

    def outside_intact(self):
        s = _SENT[self.store.element_size()]
        return bool((self.bits[:self.lo] == s).all() and (self.bits[self.hi:] == s).all())


def _direct(inp, dtype, bi, lead=0, tail=0, save_spec=True, grads=GRADS):
    """dna_fftconv_filter, _fwd, _bwd on buffers of our making. lead: u, dy, y, du, dk start that
    many elements into their storages; tail: every buffer is the head of a storage that much
    longer (outputs: sentinel, inputs: NaN), the workspace exactly dna_fftconv_workspace bytes of
    one. Returns (float32 CPU results, the buffers)."""
    from dna_amd import _native as N
    lib = N.lib()
    B, D, L = inp["u"].shape
    nk, wsz = lib.dna_fftconv_kspec_elems(L), lib.dna_fftconv_workspace(B, D, L)
    assert nk == 4 * L and wsz > 0
    P = (B + 1) // 2 * D
    b = {"u": _Buf((B, D, L), dtype, lead, tail, inp["u"]), "dy": _Buf((B, D, L), dtype, lead, tail, inp["dy"]),
         "k": _Buf((D, L), F32, 0, tail, inp["k"]), "bias": _Buf((D,), F32, 0, tail, inp["bias"].reshape(-1)),
         "out": _Buf((B, D, L), dtype, lead, tail), "kspec": _Buf((D, nk), F32, 0, tail),
         "ws": _Buf((wsz,), torch.uint8, 0, tail)}
    if save_spec:
        b["uspec"] = _Buf((P, nk), F32, 0, tail)
    if "du" in grads:
        b["du"] = _Buf((B, D, L), dtype, lead, tail)
    if "dk" in grads:
        b["dk"] = _Buf((D, L), F32, lead, tail)
    if "dbias" in grads:
        b["dbias"] = _Buf((D,), F32, 0, tail)
    for name in ("u", "dy", "out", "du", "dk"):
        if name in b:
            assert (b[name].ptr() % 16 != 0) == (lead != 0), name
    p = lambda name: b[name].ptr() if name in b else None
    s = N.stream_ptr()
    N.call("dna_fftconv_filter", p("k"), p("bias"), D, L, int(bi), p("kspec"), p("ws"), wsz, s)
    N.call("dna_fftconv_fwd", p("u"), _DNA[dtype], p("kspec"), B, D, L, int(bi), p("out"), p("uspec"),
           p("ws"), wsz, s)
    N.call("dna_fftconv_bwd", p("dy"), p("u"), _DNA[dtype], p("kspec"), p("uspec"), B, D, L, int(bi),
           p("du"), p("dk"), p("dbias"), p("ws"), wsz, s)
    torch.cuda.synchronize()
    got = {n: b[n].v.float().cpu().numpy() for n in ("out",) + tuple(grads)}
    return got, b


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
@pytest.mark.parametrize("L", [32768, 65536, 131072])
def test_misaligned_tensors_at_the_fixed_sizes(L, dtype):
    """(c) u, dy, y, du, dk one element off a 16-byte boundary: the scalar fall-backs inside
    col_fwd_kernel, col_inv_kernel (both output modes) and dbias_kernel of the LN > 0 kernels.
    The same values reach the same LDS slots, so y, du, dk are bit-identical to the aligned run."""
    assert _expect_plan(L)["fixed_ln"] > 0
    bi = True
    inp, ref, e32 = _reference(3, 3, L, bi, dtype)
    aligned, _ = _direct(inp, dtype, bi, lead=0)
    off, _ = _direct(inp, dtype, bi, lead=1, tail=7)
    _verify("aligned direct", inp, ref, e32, bi, dtype, aligned)
    _verify("misaligned", inp, ref, e32, bi, dtype, off)
    same = {n: bool(np.array_equal(aligned[n], off[n])) for n in aligned}
    print(f"FFTPATH misaligned L={L} {_DT[dtype]} bit-identical to the aligned run: {same}")
    assert same["out"] and same["du"] and same["dk"], same


@pytest.mark.parametrize("L", [1024, 65536])
def test_dk_without_a_saved_spectrum(L):
    """(e) uspec = NULL and dk wanted: dna_fftconv_bwd recomputes the input spectrum (column pass
    + ROW_SPEC) into its workspace."""
    _expect_plan(L)
    bi = True
    inp, ref, e32 = _reference(3, 3, L, bi, F32)
    saved, _ = _direct(inp, F32, bi)
    recomputed, _ = _direct(inp, F32, bi, save_spec=False)
    same = {n: bool(np.array_equal(saved[n], recomputed[n])) for n in saved}
    print(f"FFTPATH no_uspec L={L} bit-identical to the saved-spectrum run: {same}")
    _verify("no_uspec", inp, ref, e32, bi, F32, recomputed)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_ids)
@pytest.mark.parametrize("L", [64, 4096, 65536])
def test_nothing_outside_the_outputs_is_touched(L, dtype):
    """(g) every output is the head of a larger buffer whose tail holds a sentinel, the workspace
    is exactly dna_fftconv_workspace bytes of one, the inputs' tails hold NaN: every output
    element is written and finite, every sentinel intact (the missing partner row of the odd
    batch, the workspace's end, uspec and kspec), the results those of exact-size buffers, and
    a second run bit-identical (no atomics)."""
    _expect_plan(L)
    bi = True
    inp, ref, e32 = _reference(3, 3, L, bi, dtype)
    exact, _ = _direct(inp, dtype, bi)
    runs = [_direct(inp, dtype, bi, tail=4099) for _ in range(2)]
    for got, bufs in runs:
        for name, buf in bufs.items():
            if name in ("u", "dy", "k", "bias"):
                continue
            assert buf.outside_intact(), f"{name}: written outside its {buf.hi - buf.lo} elements"
            if name != "ws":
                assert bool(torch.isfinite(buf.v).all()), f"{name}: unwritten or non-finite elements"
        for name in got:
            assert np.array_equal(got[name], exact[name]), f"{name} differs from the exact-size run"
    for name in ("out", "du", "dk", "dbias", "kspec", "uspec"):
        assert torch.equal(runs[0][1][name].v, runs[1][1][name].v), f"{name}: two runs differ"
    _verify("guarded", inp, ref, e32, bi, dtype, runs[0][0])


# ---------------------------------------------------------------- cross-talk of the packing

def _zero_row_figure(got, ref, zero, partner):
    """max |got[zero]| over max |ref[partner]|: what reaches a row whose exact result is zero
    from the row it shares a complex sequence with."""
    assert not np.any(ref[zero])
    return float(np.abs(got[zero]).max() / np.abs(ref[partner]).max())


def test_cross_talk_of_the_batch_pair():
    """(h) batch rows 0 and 1 are the real and imaginary part of one sequence. With row 1 (u and
    dy) all zero its out and du are exactly zero in the oracle; the kernel leaves rounding error
    of row 0 there -- no more than the fp32 bound times row 0's maximum. That describes the
    design; it is not zero."""
    B, D, L, bi = 2, 2, 4096, True
    inp = FC.inputs(B, D, L, bi, FC.seed_for(B, D, L, bi))
    inp["u"][1] = 0
    inp["dy"][1] = 0
    ref, e32 = FC.reference_of(inp, bi)
    got = _wrapper(inp, bi, F32)
    for name in ("out", "du"):
        fig = max(_zero_row_figure(got[name], ref[name], (1, d), (0, d)) for d in range(D))
        print(f"FFTPATH crosstalk batch {name} {fig:.2e} ({fig / e32[name]:.2f}x e32 {e32[name]:.2e})")
        assert fig <= FC.fp32_bound(e32[name]), (name, fig, e32[name])
        FC.assert_close(name, got[name][:1], ref[name][:1], e32[name])
    FC.assert_close("dk", got["dk"], ref["dk"], e32["dk"])
    FC.assert_close("dbias", got["dbias"], ref["dbias"], e32["dbias"])


def test_cross_talk_of_the_filter_pair():
    """(h) filter channels 0 and 1 are transformed as one complex sequence and separated in the
    spectrum. With k[1] and bias[1] zero, channel 1's out (and du) is exactly zero in the oracle;
    the kernel's is the separation's rounding residue of channel 0's spectrum -- within the fp32
    bound times channel 0's row maximum."""
    B, D, L, bi = 2, 2, 4096, True
    inp = FC.inputs(B, D, L, bi, FC.seed_for(B, D, L, bi))
    inp["k"][1] = 0
    inp["bias"][1] = 0
    ref, e32 = FC.reference_of(inp, bi)
    got = _wrapper(inp, bi, F32)
    for name in ("out", "du"):
        fig = max(_zero_row_figure(got[name], ref[name], (b, 1), (b, 0)) for b in range(B))
        print(f"FFTPATH crosstalk filter {name} {fig:.2e} ({fig / e32[name]:.2f}x e32 {e32[name]:.2e})")
        assert fig <= FC.fp32_bound(e32[name]), (name, fig, e32[name])
        FC.assert_close(name, got[name][:, :1], ref[name][:, :1], e32[name])
    FC.assert_close("dk", got["dk"], ref["dk"], e32["dk"])
    FC.assert_close("dbias", got["dbias"], ref["dbias"], e32["dbias"])


# ---------------------------------------------------------------- refusals

def _refused(why, name, *args):
    from dna_amd import _native as N
    status = getattr(N.lib(), name)(*args)
    assert status != 0, f"{name} accepted what it must refuse"
    assert name in N.last_error() and why in N.last_error(), N.last_error()


def _calls(b, B, D, L, dtype, wsz, null=None, short=None):
    """The three calls' argument lists on buffers b; `null` names the call whose first pointer is
    NULL, `short` the call whose workspace is one byte under what it needs."""
    from dna_amd import _native as N
    p = lambda n: b[n].ptr()
    s = N.stream_ptr()
    ws = wsz
    if short:
        NN, P = 2 * L, (B + 1) // 2 * D
        # complex64 spectra: filter ceil(D/2), fwd P, bwd 2P + D and 32 dbias partials per channel
        need = {"filter": (D + 1) // 2 * NN * 8, "fwd": P * NN * 8,
                "bwd": (2 * P + D) * NN * 8 + D * 32 * 4}
        assert max(need.values()) <= wsz
        ws = need[short] - 1
    first = lambda c, n: None if null == c else p(n)
    return {
        "filter": ("dna_fftconv_filter", first("filter", "k"), p("bias"), D, L, 1, p("kspec"), p("ws"),
                   ws, s),
        "fwd": ("dna_fftconv_fwd", first("fwd", "u"), _DNA[dtype], p("kspec"), B, D, L, 1, p("out"),
                p("uspec"), p("ws"), ws, s),
        "bwd": ("dna_fftconv_bwd", first("bwd", "dy"), p("u"), _DNA[dtype], p("kspec"), p("uspec"), B, D, L,
                1, p("du"), p("dk"), p("dbias"), p("ws"), ws, s),
    }


def test_refusals_leave_the_outputs_untouched():
    """(i) unsupported lengths, a null pointer and a workspace one byte short: a non-zero status,
    the error string set, and NaN-prefilled outputs (and the workspace) as they were."""
    from dna_amd import _native as N
    lib = N.lib()
    B, D, dtype = 3, 3, F32
    L0 = 1024
    wsz = lib.dna_fftconv_workspace(B, D, L0)
    # buffers large enough for L0 (the refused lengths never get as far as using them)
    inp = FC.inputs(B, D, L0, True, 11)
    P = (B + 1) // 2 * D
    b = {"u": _Buf((B, D, L0), dtype, values=inp["u"]), "dy": _Buf((B, D, L0), dtype, values=inp["dy"]),
         "k": _Buf((D, L0), F32, values=inp["k"]), "bias": _Buf((D,), F32, values=inp["bias"].reshape(-1)),
         "ws": _Buf((wsz,), torch.uint8)}
    outs = ("out", "du", "dk", "dbias", "kspec", "uspec")
    shapes = {"out": (B, D, L0), "du": (B, D, L0), "dk": (D, L0), "dbias": (D,), "kspec": (D, 4 * L0),
              "uspec": (P, 4 * L0)}
    for n in outs:
        b[n] = _Buf(shapes[n], F32)
    before = {n: b[n].bits.clone() for n in outs + ("ws",)}

    def untouched(which):
        torch.cuda.synchronize()
        for n in which:
            assert torch.equal(b[n].bits, before[n]), f"{n} was written by a refused call"

    for L in (63, 96, 262144):
        assert lib.dna_fftconv_workspace(B, D, L) == 0 and lib.dna_fftconv_kspec_elems(L) == 0
        for args in _calls(b, B, D, L, dtype, wsz).values():
            _refused("must be a power of 2", *args)
        untouched(outs + ("ws",))
    for c in ("filter", "fwd", "bwd"):
        _refused("null pointer", *_calls(b, B, D, L0, dtype, wsz, null=c)[c])
        _refused("workspace too small", *_calls(b, B, D, L0, dtype, wsz, short=c)[c])
    untouched(outs + ("ws",))
    assert lib.dna_fftconv_workspace(0, D, L0) == 0 and lib.dna_fftconv_workspace(B, 0, L0) == 0
    # and the same buffers, unrefused, work: the refusals above were not an artefact of the set-up
    for c in ("filter", "fwd", "bwd"):
        name, *args = _calls(b, B, D, L0, dtype, wsz)[c]
        N.call(name, *args)
    torch.cuda.synchronize()
    ref, e32 = FC.reference_of(inp, True)
    got = {n: b[n].v.float().cpu().numpy() for n in ("out", "du", "dk", "dbias")}
    _verify("after refusals", inp, ref, e32, True, dtype, got)
