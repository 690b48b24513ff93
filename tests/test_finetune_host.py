"""Host side of fine-tuning (no GPU): the epoch-level metric, the GUE CSV dataset and the
finetune.py command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("C,seed", [(2, 0), (3, 1), (9, 2)])
def test_confusion_matrix_equals_sklearn(C, seed):
    from sklearn.metrics import accuracy_score, f1_score, matthews_corrcoef
    from dna_amd.tasks import ConfusionMatrix
    rng = np.random.default_rng(seed)
    n = 257
    y = rng.integers(0, C, n)
    pred = np.where(rng.random(n) < 0.6, y, rng.integers(0, C, n))
    if C > 2:  # a class that never occurs, neither as a label nor as a prediction
        y[y == C - 1] = 0
        pred[pred == C - 1] = 1
    cm = ConfusionMatrix(C)
    for i in range(0, n, 50):  # accumulated over batches, computed once
        cm.update(torch.as_tensor(pred[i:i + 50]), torch.as_tensor(y[i:i + 50]))
    got = cm.compute()
    assert int(cm.counts.sum()) == n and cm.counts.dtype == torch.int64
    assert got["accuracy"] == pytest.approx(accuracy_score(y, pred), abs=1e-12)
    assert got["mcc"] == pytest.approx(matthews_corrcoef(y, pred), abs=1e-12)
    assert got["f1_macro"] == pytest.approx(f1_score(y, pred, average="macro"), abs=1e-12)


def test_confusion_matrix_predicted_but_never_true_class():
    from sklearn.metrics import f1_score, matthews_corrcoef
    from dna_amd.tasks import ConfusionMatrix
    y = np.array([0, 0, 1, 1, 0, 1, 0])
    pred = np.array([0, 2, 1, 1, 0, 2, 1])  # class 2 is predicted, never true: F1 0, counted
    cm = ConfusionMatrix(3)
    cm.update(torch.as_tensor(pred), torch.as_tensor(y))
    got = cm.compute()
    assert got["f1_macro"] == pytest.approx(f1_score(y, pred, average="macro"), abs=1e-12)
    assert got["mcc"] == pytest.approx(matthews_corrcoef(y, pred), abs=1e-12)


def _write_gue(tmp_path, header):
    rng = np.random.default_rng(0)
    rows = [("".join(rng.choice(list("ACGT"), int(n))), int(rng.integers(0, 3)))
            for n in (30, 500, 70, 1200, 12, 200)]
    for split in ("train", "dev", "test"):
        with open(tmp_path / f"{split}.csv", "w") as f:
            if header:
                f.write("sequence,label\n")
            for s, l in rows:
                f.write(f"{s},{l}\n")
    return rows


@pytest.mark.parametrize("header", [True, False])
def test_csv_dataset_tokens_truncation_and_collate(tmp_path, header):
    from dna_amd.finetune_data import SequenceClassificationCSV
    from dna_amd.tokenizer import DNABertTokenizer
    rows = _write_gue(tmp_path, header)
    tok = DNABertTokenizer()
    ds = SequenceClassificationCSV(str(tmp_path), "train", max_length=100, tokenizer=tok)
    assert len(ds) == len(rows) and ds.num_labels == max(l for _, l in rows) + 1
    long_rows = 0
    for (seq, label), (ids, lab) in zip(rows, ds):
        raw = tok.encode_raw(seq)
        assert ids[0].item() == 1 and ids[-1].item() == 2  # [CLS] ... [SEP]
        assert ids[1:-1].tolist() == raw[:98] and len(ids) <= 100 and lab.item() == label
        long_rows += len(raw) > 98
    assert long_rows >= 2  # truncation was exercised
    ids, labels = ds.collate([ds[i] for i in range(len(ds))])
    assert ids.shape == (len(rows), 128) and ids.dtype == torch.int64  # 100 -> 128
    assert labels.tolist() == [l for _, l in rows]
    for r in range(len(rows)):
        n = len(ds[r][0])
        assert torch.equal(ids[r, :n], ds[r][0]) and bool((ids[r, n:] == 3).all())
    short, _ = ds.collate([ds[0], ds[4]])
    assert short.shape[1] == 64
    with pytest.raises(FileNotFoundError):
        SequenceClassificationCSV(str(tmp_path / "nope"), "train")


def test_finetune_dry_run_composes_the_experiment():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--dry-run",
                        "model.config.num_hidden_layers=1", "model.config.num_labels=9",
                        "optimizer.lr=1e-4"],
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    last = json.loads(r.stdout.strip().splitlines()[-1])
    assert last["dry_run"] is True and last["model"] == "dnabert2_cls" and last["num_labels"] == 9
    assert last["monitor"] == "val/mcc" and last["mode"] == "max"
    assert last["optimizer"]["_name_"] == "adamw" and last["optimizer"]["lr"] == 1e-4
    assert last["scheduler"]["warmup_t"] == 50
    cfg = json.loads(r.stdout[: r.stdout.rindex('{"dry_run"')])
    assert cfg["dataset"]["_name_"] == "gue_csv" and cfg["trainer"]["precision"] == "bf16"
    assert cfg["callbacks"]["model_checkpoint"]["monitor"] == "val/mcc"


def test_finetune_refuses_problem_types_it_has_no_metrics_for():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--dry-run",
                        "model.config.num_hidden_layers=1", "model.config.problem_type=regression"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "single_label_classification" in r.stderr


def test_sequence_classification_modules_import_without_gpu():
    from dna_amd.bert_layers import BertForSequenceClassification, BertModel
    from dna_amd.config import BertConfig
    from dna_amd.trainer import ClsTrainer, load_backbone  # noqa: F401
    cfg = dict(vocab_size=64, hidden_size=64, num_hidden_layers=1, num_attention_heads=1,
               intermediate_size=64, num_labels=1, classifier_dropout=0.3)
    m = BertForSequenceClassification(cfg)
    assert m.num_labels == 1 and m.classifier_dropout == 0.3
    assert BertForSequenceClassification(dict(cfg, classifier_dropout=None)).classifier_dropout == \
        BertConfig().hidden_dropout_prob
    assert m._problem_type(torch.zeros(2)) == "regression"
    m3 = BertForSequenceClassification(dict(cfg, num_labels=3))
    assert m3._problem_type(torch.zeros(2, dtype=torch.long)) == "single_label_classification"
    m4 = BertForSequenceClassification(dict(cfg, num_labels=4))
    assert m4._problem_type(torch.zeros(2, 4)) == "multi_label_classification"
    assert BertModel(cfg, add_pooling_layer=True).pooler is not None
    with pytest.raises(RuntimeError, match="GPU"):
        m3(input_ids=torch.ones(2, 64, dtype=torch.long))
