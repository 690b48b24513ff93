"""Host side of the packed (unpadded) DNABERT-2 path: PackedIndex against a plain numpy
restatement, the C ABI's new symbols and their argument checks (nothing is launched), the
collate function's unpad mode and finetune.py's dataset.unpad flag. No GPU."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 3


def _restate(ids, pad=PAD):
    """unpad_input's bookkeeping, spelled out with loops."""
    b, S = ids.shape
    indices, positions, cu, row_of = [], [], [0], -np.ones(b * S, dtype=np.int64)
    for n in range(b):
        for s in range(S):
            if ids[n, s] != pad:
                row_of[n * S + s] = len(indices)
                indices.append(n * S + s)
                positions.append(s)
        cu.append(len(indices))
    lens = np.diff(cu)
    return dict(indices=np.array(indices, dtype=np.int64), cu_seqlens=np.array(cu, dtype=np.int32),
                positions=np.array(positions, dtype=np.int32), row_of=row_of,
                max_seqlen=int(lens.max()), total=len(indices), batch=b, seqlen=S,
                first_valid=bool((ids[:, 0] != pad).all()), sq_sum=int((lens.astype(np.int64) ** 2).sum()))


def _batches():
    g = np.random.default_rng(0)
    right = g.integers(5, 4096, (4, 19))
    for r, n in enumerate((19, 1, 7, 12)):
        right[r, n:] = PAD
    left = g.integers(5, 4096, (3, 16))
    for r, n in enumerate((16, 3, 9)):
        left[r, : 16 - n] = PAD
    interior = g.integers(5, 4096, (3, 21))
    interior[0, 4:9] = PAD
    interior[1, 20] = PAD
    interior[2, [1, 3, 5, 18]] = PAD
    return {"right": right, "left": left, "interior": interior}


@pytest.mark.parametrize("kind", ["right", "left", "interior"])
def test_packed_index_matches_numpy_restatement(kind):
    from dna_amd.bert_layers import PackedIndex
    ids = _batches()[kind]
    want = _restate(ids)
    got = PackedIndex.build(torch.as_tensor(ids), PAD)
    for k in ("indices", "cu_seqlens", "positions", "row_of"):
        t = getattr(got, k)
        assert t.dtype == torch.as_tensor(want[k]).dtype, (k, t.dtype)
        assert np.array_equal(t.numpy(), want[k]), k
    for k in ("max_seqlen", "total", "batch", "seqlen", "first_valid", "sq_sum"):
        assert getattr(got, k) == want[k] and type(getattr(got, k)) is type(want[k]), k
    assert got.first_valid == (kind != "left")
    moved = got.to("cpu", non_blocking=True)
    assert torch.equal(moved.indices, got.indices) and moved.total == got.total
    if kind == "left":
        with pytest.raises(ValueError, match="starts with"):
            got.cls_rows()
    else:
        assert got.cls_rows().tolist() == want["cu_seqlens"][:-1].tolist()


def test_packed_index_rejects_an_all_pad_row():
    from dna_amd.bert_layers import PackedIndex
    ids = torch.as_tensor(_batches()["right"]).clone()
    ids[2] = PAD
    with pytest.raises(ValueError, match="row 2"):
        PackedIndex.build(ids, PAD)


def test_packed_index_of_the_fixture_batch():
    from dna_amd.bert_layers import PackedIndex
    z = np.load(os.path.join(GOLDEN, "cls_tiny.npz"))
    ids = torch.as_tensor(z["input_ids"].astype(np.int64))
    p = PackedIndex.build(ids, PAD)
    assert p.total == 263 and p.cu_seqlens.tolist() == [0, 72, 144, 184, 256, 263]
    assert p.max_seqlen == 72 and p.batch == 5 and p.seqlen == ids.shape[1] and p.first_valid


def test_attn_varlen_abi_entries():
    """The three symbols are exported and declared; bad arguments return DNA_ERR_INVALID /
    DNA_ERR_UNSUPPORTED and set dna_last_error before anything touches a GPU (host buffers stand
    in for device memory: every call here must return before a launch)."""
    from dna_amd import _native as N
    L = N.lib()
    for sym in ("dna_attn_varlen_fwd", "dna_attn_varlen_bwd", "dna_attn_varlen_bwd_workspace"):
        assert hasattr(L, sym) and sym in N.declared_symbols() and sym in N._SIGS, sym
    assert L.dna_abi_version() == 1 and L.dna_abi_revision() >= 3
    assert L.dna_attn_varlen_bwd_workspace(5, 263, 72, 12) == 12 * 263 * 4
    for bad in ((0, 263, 72, 12), (5, 0, 72, 12), (5, 263, 0, 12), (5, 263, 72, 0)):
        assert L.dna_attn_varlen_bwd_workspace(*bad) == 0
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def fwd(qkv=p, cu=p, pos=None, sl=p, nseq=2, T=10, ms=8, H=2, D=64, dt=N.BF16, out=p, lse=p):
        return L.dna_attn_varlen_fwd(qkv, cu, pos, sl, nseq, T, ms, H, D, dt, 0.125, out, lse, None)

    def bwd(qkv=p, out=p, dout=p, lse=p, cu=p, pos=None, sl=p, nseq=2, T=10, ms=8, H=2, D=64,
            dt=N.F32, dqkv=p, ws=p):
        return L.dna_attn_varlen_bwd(qkv, out, dout, lse, cu, pos, sl, nseq, T, ms, H, D, dt, 0.125,
                                     dqkv, ws, None)

    invalid = [(lambda: fwd(qkv=None), "null"), (lambda: fwd(cu=None), "null"),
               (lambda: fwd(sl=None), "null"), (lambda: fwd(out=None), "null"),
               (lambda: fwd(lse=None), "null"), (lambda: fwd(nseq=0), "bad shape"),
               (lambda: fwd(T=0), "bad shape"), (lambda: fwd(ms=-1), "bad shape"),
               (lambda: fwd(H=0), "bad shape"), (lambda: fwd(dt=N.F16), "dtype"),
               (lambda: bwd(qkv=None), "null"), (lambda: bwd(out=None), "null"),
               (lambda: bwd(dout=None), "null"), (lambda: bwd(lse=None), "null"),
               (lambda: bwd(cu=None), "null"), (lambda: bwd(sl=None), "null"),
               (lambda: bwd(dqkv=None), "null"), (lambda: bwd(ws=None), "workspace"),
               (lambda: bwd(nseq=-3), "bad shape"), (lambda: bwd(T=0), "bad shape"),
               (lambda: bwd(dt=7), "dtype")]
    for call, word in invalid:
        assert call() == 1, word  # DNA_ERR_INVALID
        assert word in N.last_error(), (word, N.last_error())
    for call in (lambda: fwd(D=32), lambda: fwd(D=128), lambda: bwd(D=96)):
        assert call() == 3  # DNA_ERR_UNSUPPORTED
        assert "head_dim" in N.last_error()


def test_varlen_op_has_no_cpu_fallback():
    from dna_amd import functional as DF
    from dna_amd.bert_layers import PackedIndex
    import dna_amd.ops as ops
    ids = torch.as_tensor(_batches()["right"])
    p = PackedIndex.build(ids, PAD)
    qkv = torch.zeros(p.total, 3 * 2 * 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        DF.alibi_attention_varlen(qkv, p, torch.ones(2), 2)
    with pytest.raises(ValueError, match="rows"):
        DF.alibi_attention_varlen(qkv[:-1], p, torch.ones(2), 2)
    for name in ("attn_varlen_fwd", "attn_varlen_bwd"):
        assert name in ops.OPS and hasattr(torch.ops.dna_amd, name)
    with pytest.raises(RuntimeError, match="GPU"):
        torch.ops.dna_amd.attn_varlen_fwd(qkv, p.cu_seqlens, p.positions, torch.ones(2), p.max_seqlen,
                                          2, 0.125, torch.zeros(p.total, 128),
                                          torch.zeros(2, p.total))


class _Tok:
    pad_token_id = PAD


def test_collate_unpad_keeps_the_batch_maximum():
    from dna_amd.bert_layers import PackedIndex
    from dna_amd.finetune_data import SequenceClassificationCSV
    ds = SequenceClassificationCSV.__new__(SequenceClassificationCSV)
    ds.tokenizer = _Tok()
    g = torch.Generator().manual_seed(0)
    items = [(torch.randint(5, 4096, (n,), generator=g), torch.tensor(n % 2)) for n in (17, 70, 3)]
    ids, labels = ds.collate(items)
    assert tuple(ids.shape) == (3, 128) and labels.tolist() == [1, 0, 1]  # as before: rounded to 64
    ids_u, labels_u, packed = ds.collate(items, unpad=True)
    assert tuple(ids_u.shape) == (3, 70) and torch.equal(labels_u, labels)
    assert torch.equal(ids_u, ids[:, :70])
    assert isinstance(packed, PackedIndex) and packed.total == 90 and packed.max_seqlen == 70
    assert packed.cu_seqlens.tolist() == [0, 17, 87, 90] and packed.first_valid
    assert torch.equal(ids_u.reshape(-1)[packed.indices], torch.cat([i for i, _ in items]))


def test_finetune_dry_run_prints_the_unpad_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--dry-run",
                        "model.config.num_hidden_layers=1", "dataset.unpad=true"],
                       capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["unpad"] is True
    # in process: dataset.unpad=false prints false; the committed experiment does not set the
    # key, and its dry run prints what it always printed
    import io
    import finetune as FT
    from dna_amd.compose import compose
    for extra, want in ((["dataset.unpad=false"], False), ([], None)):
        cfg = compose(os.path.join(ROOT, "configs"), "config",
                      ["experiment=" + FT.EXPERIMENT, "model.config.num_hidden_layers=1"] + extra)
        out = io.StringIO()
        FT.finetune(cfg, dry_run=True, out=out)
        assert json.loads(out.getvalue()).get("unpad") is want
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  ["experiment=hyena/genomic_benchmark_hyena", "dataset.unpad=true"])
    with pytest.raises(ValueError, match="no packed path"):
        FT.finetune(cfg, dry_run=True, out=io.StringIO())
