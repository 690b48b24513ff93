"""The packed (unpadded) encoder path of BertForSequenceClassification / BertModel /
BertForMaskedLM and the trainer around it, against the reference fixtures of
tests/test_gpu_seq_classification.py (tests/golden/cls_tiny*.npz: tiny config, hash-initialised
weights, eval mode). GPU only.

Bounds are that file's: fp32 logits / activations within 1e-3, loss within 1e-4, every parameter
gradient within 2e-3 relative L2; bf16 logits within twice the reference's own bf16-autocast
deviation + 5e-3. Where the padded and the packed path of one model are compared, the bound is
the fp32 parity bound 1e-3.

A row that starts with [PAD] has no [CLS] row in the packed layout (cls_logits raises), so the
left-padded copy of the fixture batch is compared on BertModel's sequence output and on the
masked-LM logits, whose rows are valid tokens; the copy that keeps [CLS] in column 0 and
right-aligns the rest, and the copy with [PAD] inserted inside the rows, are compared on the
classification logits.
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
PAD = 3
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


def _hash_init(m, prefix=""):
    sd = {k: torch.from_numpy(hash_tensor(prefix + k, tuple(v.shape)))
          for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    return m


def _model(z, tag, precision):
    from dna_amd.bert_layers import BertForSequenceClassification
    C, problem = HEADS[tag]
    m = BertForSequenceClassification(_cfg(z, num_labels=C, problem_type=problem),
                                      precision=precision)
    return _hash_init(m).to(DEV).eval()


def _host_ids(z):
    return torch.as_tensor(z["input_ids"].astype(np.int64))


def _packed(ids_host):
    """The index as the collate function builds it: on the host, then moved."""
    from dna_amd.bert_layers import PackedIndex
    return PackedIndex.build(ids_host, PAD).to(DEV, non_blocking=True)


def _labels(z, tag):
    return torch.as_tensor(z[f"{tag}/labels"], device=DEV)


@pytest.mark.parametrize("tag", ["c3", "c1", "c4"])
def test_fp32_packed_forward_loss_and_gradients_vs_reference(gold, tag):
    m = _model(gold, tag, "fp32")
    ids = _host_ids(gold)
    out = m(input_ids=ids.to(DEV), labels=_labels(gold, tag), packed=_packed(ids))
    err = np.abs(out.logits.detach().cpu().numpy() - gold[f"{tag}/logits"]).max()
    print(f"{tag}: packed logits err {err:.3e}, loss {out.loss.item():.6f} vs "
          f"{float(gold[f'{tag}/loss']):.6f}")
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
    print(f"{tag}: packed worst gradient relative L2 error {worst:.3e}")


@pytest.mark.parametrize("tag", ["c3", "c1", "c4"])
def test_bf16_packed_logits_within_reference_autocast_deviation(gold, tag):
    m = _model(gold, tag, "bf16")
    ids = _host_ids(gold)
    with torch.no_grad():
        logits, loss, _ = m.cls_logits(ids.to(DEV), packed=_packed(ids))
        full, _, _ = m.cls_logits(ids.to(DEV), full_last_layer=True, packed=_packed(ids))
    assert loss is None
    ref = gold[f"{tag}/logits"]
    tol = 2 * np.abs(gold[f"{tag}/logits_bf16"] - ref).max() + 5e-3
    err = np.abs(logits.cpu().numpy() - ref).max()
    err_full = np.abs(full.cpu().numpy() - ref).max()
    print(f"{tag}: packed bf16 logits err {err:.3e}, full last layer {err_full:.3e} "
          f"(tolerance {tol:.3e})")
    assert err < tol, (err, tol)
    assert err_full < tol, (err_full, tol)


def _bert_model(gold, precision="fp32"):
    from dna_amd.bert_layers import BertModel
    m = BertModel(_cfg(gold), add_pooling_layer=True, precision=precision)
    return _hash_init(m, "bert.").to(DEV).eval()


def test_fp32_packed_bert_model_outputs_vs_reference(gold):
    m = _bert_model(gold)
    ids = _host_ids(gold)
    d = ids.to(DEV)
    with torch.no_grad():
        seq, pooled = m(d, attention_mask=(d != PAD).long(), packed=_packed(ids))
    assert seq.shape == gold["sequence_output"].shape and seq.dtype == torch.float32
    e_seq = np.abs(seq.cpu().numpy() - gold["sequence_output"]).max()
    e_pool = np.abs(pooled.cpu().numpy() - gold["pooled_output"]).max()
    print(f"packed BertModel: sequence err {e_seq:.3e}, pooled err {e_pool:.3e}")
    assert e_seq < 1e-3 and e_pool < 1e-3
    assert seq[d == PAD].abs().max().item() == 0.0  # pad positions exactly zero
    with pytest.raises(ValueError, match="PackedIndex of a"):
        m(d[:, :64].contiguous(), packed=_packed(ids))


def _left_padded(ids):
    out = torch.full_like(ids, PAD)
    for r in range(ids.shape[0]):
        tok = ids[r][ids[r] != PAD]
        out[r, ids.shape[1] - tok.numel():] = tok
    return out


def _cls_then_right_aligned(ids):
    out = _left_padded(ids)
    for r in range(ids.shape[0]):
        n = int((ids[r] != PAD).sum())
        if n < ids.shape[1]:
            out[r, ids.shape[1] - n] = PAD
            out[r, 0] = ids[r, 0]
    return out


def _interior_padded(ids):
    """[PAD] inserted inside the rows: 5 after column 3 and 1 after column 20 (rows long enough)."""
    b, S = ids.shape
    out = torch.full((b, S + 6), PAD, dtype=ids.dtype)
    for r in range(b):
        tok = ids[r][ids[r] != PAD]
        n = tok.numel()
        out[r, :min(n, 4)] = tok[:4]
        if n > 4:
            rest = tok[4:]
            k = min(rest.numel(), 17)
            out[r, 9:9 + k] = rest[:k]
            if rest.numel() > 17:
                out[r, 27:27 + rest.numel() - 17] = rest[17:]
    return out


def test_fp32_left_and_interior_padded_batches_agree_with_the_padded_path(gold):
    ids = _host_ids(gold)
    m = _model(gold, "c3", "fp32")
    for name, variant in (("cls + right-aligned", _cls_then_right_aligned(ids)),
                          ("interior", _interior_padded(ids))):
        assert int((variant != PAD).sum()) == 263 and bool((variant[:, 0] != PAD).all())
        assert not torch.equal(variant[:, :ids.shape[1]], ids)
        d = variant.to(DEV)
        with torch.no_grad():
            want, _, _ = m.cls_logits(d)
            got, _, _ = m.cls_logits(d, packed=_packed(variant))
        err = (got - want).abs().max().item()
        print(f"{name}: packed vs padded logits {err:.3e}")
        assert err < 1e-3, (name, err)
    # rows that start with [PAD]: no [CLS] row to read, but the encoder itself is the same
    left = _left_padded(ids)
    bm = _bert_model(gold)
    d = left.to(DEV)
    with torch.no_grad():
        want, _ = bm(d)
        p = _packed(left)
        x32, _ = bm.encode(d, packed=p)
    assert not p.first_valid and x32.shape == (263, 128)
    err = (want.view(-1, 128)[p.indices] - x32).abs().max().item()
    print(f"left-padded: packed vs padded sequence output {err:.3e}")
    assert err < 1e-3, err
    with pytest.raises(ValueError, match="starts with"):
        m.cls_logits(d, packed=p)
    with pytest.raises(ValueError, match="starts with"):
        bm(d, packed=p)


def test_fp32_packed_mlm_logits_agree_with_the_padded_path():
    from dna_amd.bert_layers import BertForMaskedLM, MLMIndex
    z = np.load(os.path.join(GOLDEN, "model_tiny.npz"))
    m = BertForMaskedLM(_cfg(z, hyena_framework=True), precision="fp32")
    sd = {k: torch.from_numpy(hash_tensor(
        k if k != "cls.predictions.decoder.weight" else "bert.embeddings.word_embeddings.weight",
        tuple(v.shape))) for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    ids = torch.as_tensor(z["masked_ids"].astype(np.int64))
    labels = torch.as_tensor(z["labels"].astype(np.int64))
    assert int((ids != PAD).sum()) < ids.numel()  # the fixture has a padded row
    # as stored (right-padded) and as the pretraining corpus pads (on the left)
    shift = ids.shape[1] - (ids != PAD).sum(1)
    left_ids = torch.stack([torch.roll(r, int(s)) for r, s in zip(ids, shift)])
    left_labels = torch.stack([torch.roll(r, int(s)) for r, s in zip(labels, shift)])
    for name, i, l in (("right", ids, labels), ("left", left_ids, left_labels)):
        idx = MLMIndex.build(i, l).to(DEV)
        d = i.to(DEV)
        with torch.no_grad():
            want = m.mlm_logits(d, idx)
            got = m.mlm_logits(d, idx, packed=_packed(i))
            loss_w, _ = m.mlm_loss(d, l.to(DEV) > 0, idx)
            loss_g, _ = m.mlm_loss(d, l.to(DEV) > 0, idx, packed=_packed(i))
        err = (got - want).abs().max().item()
        print(f"mlm {name}-padded: packed vs padded logits {err:.3e}, loss "
              f"{loss_g.item():.6f} vs {loss_w.item():.6f}")
        assert got.shape == want.shape and err < 1e-3, (name, err)
        assert abs(loss_g.item() - loss_w.item()) < 1e-4
    want = z["logits_rows"]
    with torch.no_grad():
        got = m.mlm_logits(ids.to(DEV), MLMIndex.build(ids, labels).to(DEV), packed=_packed(ids))
    assert np.abs(got.cpu().numpy() - want).max() < 1e-3  # and the reference's own rows


def _strict_cfg():
    # every projection side a multiple of 256: the shapes the hand-written bf16 kernels take
    return dict(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                intermediate_size=512, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0,
                layer_norm_eps=1e-12, type_vocab_size=2, pad_token_id=0, num_labels=3)


def test_packed_trainer_step_stays_native_under_strict(gold, monkeypatch):
    from dna_amd import functional as DF
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.trainer import ClsTrainer
    monkeypatch.setenv("DNA_STRICT_NATIVE", "1")
    monkeypatch.setattr(DF, "_FALLBACK_SEEN", set())
    torch.manual_seed(0)
    tr = ClsTrainer(BertForSequenceClassification(_strict_cfg()), DEV, lr=1e-4, seed=1)
    ids = _host_ids(gold)
    packed = _packed(ids)
    assert packed.total == 263
    before = tr.flat.flat.clone()
    loss = tr.step(ids.to(DEV), _labels(gold, "c3"), packed=packed)
    assert torch.isfinite(loss).item() and not DF._FALLBACK_SEEN
    assert tr.last_pred.shape == (5,) and tr.last_logits.shape == (5, 3)
    assert not torch.equal(before, tr.flat.flat)
    for n, p in tr.model.named_parameters():  # every parameter got a gradient
        if "token_type" not in n:
            assert p.grad.abs().max().item() > 0, n
    assert tr.rng_state()["offset"] > 0
    logits, ev_loss, pred = tr.evaluate(ids.to(DEV), _labels(gold, "c3"), packed=packed)
    assert logits.shape == (5, 3) and torch.isfinite(ev_loss).item() and tr.model.training


def test_packed_overfits_sixteen_sequences_of_unequal_length(gold):
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.trainer import ClsTrainer
    torch.manual_seed(0)
    cfg = _cfg(gold, num_labels=2, hidden_dropout_prob=0.0)
    tr = ClsTrainer(BertForSequenceClassification(cfg), DEV, lr=1e-3, weight_decay=0.0)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(5, 4096, (16, 64), generator=g)
    ids[:, 0] = 1
    for r in range(16):  # 4, 8, .. 64 tokens
        ids[r, 4 * (r + 1):] = PAD
    packed = _packed(ids)
    assert packed.total == sum(4 * (r + 1) for r in range(16))
    labels = (torch.arange(16) % 2).to(DEV)
    ids = ids.to(DEV)
    losses = [tr.step(ids, labels, packed=packed).item() for _ in range(30)]
    print("packed overfit losses", [round(v, 4) for v in losses[::5]], losses[-1])
    assert losses[-1] < 0.5 * losses[0], losses


def test_pooling_head_trainer_rejects_a_packed_index():
    """SeqClsTrainer's models have no packed path: the unknown argument is refused by name."""
    from dna_amd.trainer import _ClsSteps

    class NoPacked:
        def cls_logits(self, input_ids, labels=None):
            raise AssertionError("not reached")

    steps = _ClsSteps.__new__(_ClsSteps)
    with pytest.raises(TypeError, match="packed"):
        steps._cls_loss(NoPacked(), (None, None, object()))
