"""BertForSequenceClassification / BertModel on the HIP path against the reference fixtures
(tests/golden/cls_tiny*.npz, written by tests/golden/make_cls_golden.py) and the trainer around
them (GPU only).

Bounds: fp32 mode is held to the project's fp32 parity bound (logits / activations within 1e-3,
loss within 1e-4, gradients within 2e-3 relative, as tests/test_gpu_model.py); bf16 mode to twice
the reference's own bf16-autocast deviation from its fp32 logits (stored in the fixture) + 5e-3.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle.hashinit import hash_tensor
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEADS = {"c3": (3, "single_label_classification"), "c1": (1, "regression"),
         "c4": (4, "multi_label_classification")}


def _cfg(z, **kw):
    L, d, H, Fd = json.loads(z["config"].tobytes().decode())
    cfg = dict(vocab_size=4096, hidden_size=d, num_hidden_layers=L, num_attention_heads=H,
               intermediate_size=Fd, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0,
               layer_norm_eps=1e-12, max_position_embeddings=512, type_vocab_size=2,
               pad_token_id=0, alibi_starting_size=512, hidden_act="gelu", initializer_range=0.02)
    cfg.update(kw)
    return cfg


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "cls_tiny.npz"))


def _hash_init(m):
    sd = {k: torch.from_numpy(hash_tensor(k, tuple(v.shape))) for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    return m


def _model(z, tag, precision):
    from dna_amd.bert_layers import BertForSequenceClassification
    C, problem = HEADS[tag]
    m = BertForSequenceClassification(_cfg(z, num_labels=C, problem_type=problem),
                                      precision=precision)
    return _hash_init(m).to(DEV).eval()


def _ids(z):
    return torch.as_tensor(z["input_ids"].astype(np.int64), device=DEV)


def _labels(z, tag):
    return torch.as_tensor(z[f"{tag}/labels"], device=DEV)


def test_state_dict_keys_are_the_reference_s(gold):
    m = _model(gold, "c3", "fp32")
    keys = set(m.state_dict())
    assert {"bert.pooler.dense.weight", "bert.pooler.dense.bias", "classifier.weight",
            "classifier.bias"} <= keys
    assert not [k for k in keys if k.startswith("cls.")]
    grads = {k[len("c3/grad/"):] for k in gold.files if k.startswith("c3/grad/")}
    for i in range(2):
        zl = np.load(os.path.join(GOLDEN, f"cls_tiny_grad_c3_l{i}.npz"))
        grads |= {k[len("grad/"):] for k in zl.files}
    assert {n for n, _ in m.named_parameters()} == grads
    # W^T copies for the encoder projections only: the head kernel reads pooler / classifier
    flagged = {n for n, p in m.named_parameters() if getattr(p, "_dna_transpose", False)}
    assert flagged and all(n.startswith("bert.encoder.") for n in flagged)


@pytest.mark.parametrize("tag", ["c3", "c1", "c4"])
def test_fp32_forward_loss_and_gradients_vs_reference(gold, tag):
    m = _model(gold, tag, "fp32")
    out = m(input_ids=_ids(gold), labels=_labels(gold, tag))
    err = np.abs(out.logits.detach().cpu().numpy() - gold[f"{tag}/logits"]).max()
    print(f"{tag}: logits err {err:.3e}, loss {out.loss.item():.6f} vs {float(gold[f'{tag}/loss']):.6f}")
    assert err < 1e-3, err
    assert abs(out.loss.item() - float(gold[f"{tag}/loss"])) < 1e-4
    out.loss.backward()
    ref = {k[len(tag) + 6:]: gold[k] for k in gold.files if k.startswith(f"{tag}/grad/")}
    for i in range(2):
        zl = np.load(os.path.join(GOLDEN, f"cls_tiny_grad_{tag}_l{i}.npz"))
        ref.update({k[len("grad/"):]: zl[k] for k in zl.files})
    worst = 0.0
    for n, p in m.named_parameters():
        g = p.grad.detach().cpu().numpy().astype(np.float64)
        r = ref[n].astype(np.float64)
        rel = np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-12)
        worst = max(worst, rel)
        assert rel < 2e-3, (n, rel)
    print(f"{tag}: worst gradient relative L2 error {worst:.3e}")


def test_fp32_bert_model_outputs_vs_reference(gold):
    from dna_amd.bert_layers import BertModel
    m = BertModel(_cfg(gold), add_pooling_layer=True, precision="fp32")
    sd = {k: torch.from_numpy(hash_tensor("bert." + k, tuple(v.shape)))
          for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    ids = _ids(gold)
    with torch.no_grad():
        seq, pooled = m(ids, attention_mask=(ids != 3).long())
    assert seq.shape == gold["sequence_output"].shape and seq.dtype == torch.float32
    assert np.abs(seq.cpu().numpy() - gold["sequence_output"]).max() < 1e-3
    assert np.abs(pooled.cpu().numpy() - gold["pooled_output"]).max() < 1e-3
    assert seq[ids == 3].abs().max().item() == 0.0  # pad positions exactly zero
    with pytest.raises(NotImplementedError, match="attention_mask must equal"):
        m(ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(NotImplementedError, match="token_type_ids other than 0"):
        m(ids, token_type_ids=torch.ones_like(ids))
    none = BertModel(_cfg(gold), add_pooling_layer=False, precision="fp32").to(DEV).eval()
    with torch.no_grad():
        assert none(ids)[1] is None


@pytest.mark.parametrize("tag", ["c3", "c1", "c4"])
def test_bf16_logits_within_reference_autocast_deviation(gold, tag):
    m = _model(gold, tag, "bf16")
    with torch.no_grad():
        out = m(input_ids=_ids(gold))
    assert out.loss is None
    ref = gold[f"{tag}/logits"]
    tol = 2 * np.abs(gold[f"{tag}/logits_bf16"] - ref).max() + 5e-3
    err = np.abs(out.logits.cpu().numpy() - ref).max()
    print(f"{tag}: bf16 logits err {err:.3e} (tolerance {tol:.3e})")
    assert err < tol, (err, tol)


def test_cls_only_last_layer_equals_full_last_layer(gold):
    m = _model(gold, "c3", "fp32")
    with torch.no_grad():
        sub, _, _ = m.cls_logits(_ids(gold))
        full, _, _ = m.cls_logits(_ids(gold), full_last_layer=True)
    # the kernels' tiling keeps a row's sums the same whichever rows run beside it: bit-equal
    assert torch.equal(sub, full), ((sub - full).abs().max() / full.abs().max()).item()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_internal_padding_is_inert(gold, precision):
    """S = 72 (bf16: padded to 128 inside) and S = 64 give the same logits for the rows whose
    tokens fit in 64 (rows 2 and 4 of the fixture batch: 40 and 7 tokens)."""
    m = _model(gold, "c3", precision)
    ids = _ids(gold)[[2, 4]]
    assert bool((ids[:, 64:] == 3).all())
    with torch.no_grad():
        a = m(input_ids=ids).logits
        b = m(input_ids=ids[:, :64].contiguous()).logits
        c = m(input_ids=torch.nn.functional.pad(ids, (0, 56), value=3)).logits
    # the same logits, bit for bit, in both precisions: a [PAD] key's probability underflows to
    # exactly 0, and the keys of a row's first 64-key tile are summed in the same order whether
    # or not further (all-pad) tiles follow
    assert torch.equal(a, b), ((a - b).abs().max() / a.abs().max()).item()
    if precision == "bf16":  # 72 runs as 128 inside
        assert torch.equal(a, c)
    # BertModel's sliced sequence output keeps its shape and its zero pad rows
    from dna_amd.bert_layers import BertModel
    bm = BertModel(_cfg(gold), add_pooling_layer=True, precision=precision).to(DEV).eval()
    with torch.no_grad():
        seq, pooled = bm(_ids(gold))
    assert seq.shape == (5, 72, 128) and pooled.shape == (5, 128)
    assert seq[_ids(gold) == 3].abs().max().item() == 0.0


def test_mlm_logits_bit_identical_to_parent_commit():
    """mlm_logits after the shared-encoder refactor == a stored run of the parent commit
    (tests/golden/mlm_logits_parent.npz: model_tiny.npz inputs, hash-initialised weights; fp32
    eval, bf16 eval and bf16 training mode with the default dropout stream; bf16 stored as bits)."""
    from dna_amd.bert_layers import BertForMaskedLM, MLMIndex
    z = np.load(os.path.join(GOLDEN, "model_tiny.npz"))
    want = np.load(os.path.join(GOLDEN, "mlm_logits_parent.npz"))
    cfg = _cfg(z, hyena_framework=True)
    ids = torch.as_tensor(z["masked_ids"].astype(np.int64), device=DEV)
    labels = torch.as_tensor(z["labels"].astype(np.int64), device=DEV)
    idx = MLMIndex.build(ids, labels)
    for key in ("fp32_eval", "bf16_eval", "bf16_train"):
        prec, mode = key.split("_")
        m = BertForMaskedLM(cfg, precision=prec)
        sd = {k: torch.from_numpy(hash_tensor(
            k if k != "cls.predictions.decoder.weight" else
            "bert.embeddings.word_embeddings.weight", tuple(v.shape)))
            for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV).train(mode == "train")
        with torch.no_grad():
            lg = m.mlm_logits(ids, idx)
        got = (lg.view(torch.int16) if prec == "bf16" else lg).cpu().numpy()
        assert got.dtype == want[key].dtype and np.array_equal(got, want[key]), key


def _tiny_mlm_checkpoint(tmp_path, cfg):
    import train
    from dna_amd.bert_layers import BertForMaskedLM
    from dna_amd.trainer import MLMTrainer
    torch.manual_seed(3)
    tr = MLMTrainer(BertForMaskedLM(cfg), DEV)
    path = str(tmp_path / "mlm.ckpt")
    train.save_checkpoint(path, tr, epoch=0)
    return path, tr.model


def test_load_backbone_from_mlm_checkpoint(gold, tmp_path):
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.trainer import load_backbone
    cfg = _cfg(gold, num_labels=3)
    path, mlm = _tiny_mlm_checkpoint(tmp_path, cfg)
    m = BertForSequenceClassification(cfg)
    missing, unexpected = load_backbone(m, path)
    assert sorted(missing) == ["bert.pooler.dense.bias", "bert.pooler.dense.weight",
                               "classifier.bias", "classifier.weight"]
    assert unexpected and all(k.startswith("cls.") for k in unexpected)
    assert sorted(unexpected) == sorted(k for k in mlm.state_dict() if k.startswith("cls."))
    src = mlm.state_dict()
    for k, v in m.state_dict().items():
        if k.startswith("bert.") and "pooler" not in k:
            assert torch.equal(v.cpu(), src[k].cpu()), k
    # from_composer: a bare state dict with the `model.` prefix, loaded non-strictly
    bare = str(tmp_path / "bare.pt")
    torch.save({"model." + k: v.cpu() for k, v in mlm.state_dict().items()}, bare)
    m2 = BertForSequenceClassification.from_composer(bare, config=cfg)
    assert sorted(m2.missing_keys) == sorted(missing)
    assert torch.equal(m2.bert.embeddings.word_embeddings.weight,
                       src["bert.embeddings.word_embeddings.weight"].cpu())


def test_small_row_weight_gradient_is_native_and_right(monkeypatch):
    """dW of a projection over a handful of rows (the [CLS] rows in the last layer) runs on the
    strided MFMA GEMM, plain and accumulating; bf16 operands, fp32 sums: compared with float64."""
    from dna_amd import functional as DF
    monkeypatch.setenv("DNA_STRICT_NATIVE", "1")
    g = torch.Generator().manual_seed(1)
    for rows, m_, n_ in ((5, 256, 512), (32, 768, 768), (1, 128, 384)):
        dy = torch.randn(rows, m_, generator=g).to(torch.bfloat16).to(DEV)
        x = torch.randn(rows, n_, generator=g).to(torch.bfloat16).to(DEV)
        ref = dy.double().t() @ x.double()
        out = DF.wgrad(dy, x)
        base = torch.randn(m_, n_, generator=g).to(DEV)
        acc = base.clone()
        DF.wgrad_accumulate(dy, x, acc)
        tol = 1e-5 * rows ** 0.5 * float(ref.abs().max())
        assert float((out.double() - ref).abs().max()) <= tol
        # + one fp32 rounding of base + dW
        assert float((acc.double() - base.double() - ref).abs().max()) <= \
            tol + 2.0 ** -23 * float((base.double() + ref).abs().max())


def _strict_cfg():
    # every projection side a multiple of 256: the shapes the hand-written bf16 kernels take
    return dict(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                intermediate_size=512, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0,
                layer_norm_eps=1e-12, type_vocab_size=2, pad_token_id=0, num_labels=3)


def test_trainer_step_stays_native_under_strict(gold, monkeypatch):
    from dna_amd import functional as DF
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.trainer import ClsTrainer
    monkeypatch.setenv("DNA_STRICT_NATIVE", "1")
    monkeypatch.setattr(DF, "_FALLBACK_SEEN", set())
    torch.manual_seed(0)
    tr = ClsTrainer(BertForSequenceClassification(_strict_cfg()), DEV, lr=1e-4, seed=1)
    ids = _ids(gold)
    assert tuple(ids.shape) == (5, 72)
    before = tr.flat.flat.clone()
    loss = tr.step(ids, _labels(gold, "c3"))
    assert torch.isfinite(loss).item() and not DF._FALLBACK_SEEN
    assert tr.last_pred.shape == (5,) and tr.last_logits.shape == (5, 3)
    assert not torch.equal(before, tr.flat.flat)
    for n, p in tr.model.named_parameters():  # every parameter got a gradient
        if "token_type" not in n:
            assert p.grad.abs().max().item() > 0, n
    assert tr.rng_state()["offset"] > 0


def test_overfits_sixteen_sequences(gold):
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.trainer import ClsTrainer
    torch.manual_seed(0)
    cfg = _cfg(gold, num_labels=2, hidden_dropout_prob=0.0)
    tr = ClsTrainer(BertForSequenceClassification(cfg), DEV, lr=1e-3, weight_decay=0.0)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(5, 4096, (16, 64), generator=g)
    ids[:, 0] = 1
    ids[::3, 40:] = 3
    labels = (torch.arange(16) % 2).to(DEV)
    ids = ids.to(DEV)
    losses = [tr.step(ids, labels).item() for _ in range(30)]
    print("overfit losses", [round(v, 4) for v in losses[::5]], losses[-1])
    assert losses[-1] < 0.5 * losses[0], losses


def test_confusion_matrix_accumulates_without_host_sync():
    """ConfusionMatrix.update on device tensors reads nothing back: under torch's sync debug
    mode ("error": any synchronising call raises) the per-batch updates go through, and the
    counts equal the host computation."""
    from dna_amd.tasks import ConfusionMatrix
    C = 5
    g = torch.Generator().manual_seed(0)
    y = torch.randint(0, C, (4, 64), generator=g)
    pred = torch.randint(0, C, (4, 64), generator=g)
    yd, pd = y.to(DEV), pred.to(DEV)
    cm = ConfusionMatrix(C)
    cm.update(pd[0], yd[0])  # the first update moves the matrix to the device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(1, 4):
            cm.update(pd[i], yd[i])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = torch.zeros(C, C, dtype=torch.int64)
    for t, p in zip(y.reshape(-1).tolist(), pred.reshape(-1).tolist()):
        want[t, p] += 1
    assert cm.counts.is_cuda and torch.equal(cm.counts.cpu(), want)
    host = ConfusionMatrix(C)
    host.update(pred, y)
    assert cm.compute() == host.compute()


def test_bert_model_pooled_output_in_grad_mode_has_no_graph(gold):
    """eval() without no_grad(): the stand-alone pooler returns the same values, without an
    autograd graph, and says so in a warning instead of raising."""
    import warnings
    from dna_amd import functional as DF
    from dna_amd.bert_layers import BertModel
    m = BertModel(_cfg(gold), add_pooling_layer=True, precision="fp32").to(DEV).eval()
    ids = _ids(gold)
    with torch.no_grad():
        _, want = m(ids)
    DF._POOLER_WARNED = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        seq, pooled = m(ids)
    assert any("without an autograd graph" in str(x.message) for x in w)
    assert not pooled.requires_grad and seq.requires_grad and torch.equal(pooled, want)
