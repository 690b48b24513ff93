"""Regression and multi-label fine-tuning off the GPU: the DeepSTARR / DeepSEA loaders on tiny
files, PearsonR and MultilabelAUROC against brute force and the reference's recorded values
(tests/golden/regression_tasks.npz, written by make_regression_golden.py from the reference's own
functions), the loss-name table, and finetune.py --dry-run of the three experiments."""
import gzip
import io
import json
import os
import random

import numpy as np
import pytest
import torch

from dna_amd import tasks
from dna_amd.finetune_data import (DEEPSEA_LABELS, DeepSEACsv, DeepSTARRFolder,
                                   string_reverse_complement)
from dna_amd.tokenizer import CharacterTokenizer

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "regression_tasks.npz"))
ML = int(GOLD["max_length"])


def _tok():
    return CharacterTokenizer(["A", "C", "G", "T", "N"], ML + 2, padding_side="left")


def _write_deepstarr(folder, name, seqs, table):
    with open(os.path.join(folder, f"Sequences_{name}.fa"), "w") as f:
        for i, s in enumerate(seqs):
            f.write(f">seq{i}\n{s}\n")
    with open(os.path.join(folder, f"Sequences_activity_{name}.txt"), "w") as f:
        f.write("Dev_log2_enrichment\tother\tHk_log2_enrichment\n")
        for r in table:
            f.write("\t".join(repr(float(v)) for v in r) + "\n")


def _write_deepsea(folder, name, seqs, labels):
    with gzip.open(os.path.join(folder, f"{name}.csv.gz"), "wt") as f:
        for s, row in zip(seqs, labels):
            f.write(s + "," + ",".join(str(int(v)) for v in row) + "\n")


@pytest.fixture()
def deepstarr_dir(tmp_path):
    seqs, table = [str(s) for s in GOLD["deepstarr_seqs"]], GOLD["deepstarr_table"]
    _write_deepstarr(tmp_path, "Train", seqs, table)
    _write_deepstarr(tmp_path, "Val", seqs[:2], table[:2])
    _write_deepstarr(tmp_path, "Test", seqs[2:], table[2:])
    return tmp_path


@pytest.fixture()
def deepsea_dir(tmp_path):
    seqs, labels = [str(s) for s in GOLD["deepsea_seqs"]], GOLD["deepsea_labels"]
    _write_deepsea(tmp_path, "train", seqs, labels)
    _write_deepsea(tmp_path, "valid", seqs[:1], labels[:1])
    _write_deepsea(tmp_path, "test", seqs[1:], labels[1:])
    return tmp_path


# ------------------------------------------------------------------------------------ loaders
def test_deepstarr_items_match_the_reference_dataset(deepstarr_dir):
    ds = DeepSTARRFolder(deepstarr_dir, "train", ML, tokenizer=_tok())
    assert len(ds) == 5 and ds.num_labels == 2 and ds.d_output == 2
    ids, tgt = ds.collate([ds[i] for i in range(len(ds))])
    assert ids.dtype == torch.int64 and tgt.dtype == torch.float32
    assert np.array_equal(ids.numpy(), GOLD["deepstarr_ids"])       # left padding, truncation
    assert np.array_equal(tgt.numpy(), GOLD["deepstarr_targets"])   # the two columns, by name
    assert np.array_equal(tgt.numpy(), GOLD["deepstarr_table"][:, [0, 2]])
    pad = ds.pad_token_id
    assert (ids[3, :-1] == pad).all() and ids[3, -1] != pad          # a 1-base sequence
    assert (ids[2] != pad).all()                                     # 20 bases cut to 12


def test_deepstarr_split_names_and_errors(deepstarr_dir, tmp_path):
    sizes = {"train": 5, "val": 2, "valid": 2, "Val": 2, "test": 3, "Test": 3}
    for split, n in sizes.items():
        assert len(DeepSTARRFolder(deepstarr_dir, split, ML)) == n
    with pytest.raises(ValueError, match="dev"):
        DeepSTARRFolder(deepstarr_dir, "dev", ML)
    with pytest.raises(NotImplementedError, match="use_tokenizer"):
        DeepSTARRFolder(deepstarr_dir, "train", ML, use_tokenizer=False)
    os.remove(os.path.join(deepstarr_dir, "Sequences_activity_Test.txt"))
    with pytest.raises(FileNotFoundError, match="Sequences_activity_Test.txt"):
        DeepSTARRFolder(deepstarr_dir, "test", ML)
    # a count mismatch, and the reference's FASTA rule: reading stops at the first empty line
    with open(os.path.join(deepstarr_dir, "Sequences_Val.fa"), "w") as f:
        f.write(">a\nACGT\n\n>b\nGGCC\n")
    with pytest.raises(ValueError, match="1 sequences.*2 rows"):
        DeepSTARRFolder(deepstarr_dir, "val", ML)
    with open(os.path.join(deepstarr_dir, "Sequences_activity_Val.txt"), "w") as f:
        f.write("Dev_log2_enrichment\tHk\n1.0\t2.0\n")
    with pytest.raises(ValueError, match="Hk_log2_enrichment"):
        DeepSTARRFolder(deepstarr_dir, "val", ML)


def test_deepsea_items_match_the_reference_dataset(deepsea_dir):
    ds = DeepSEACsv(deepsea_dir, "train", ML, tokenizer=_tok())
    assert len(ds) == 4 and ds.num_labels == DEEPSEA_LABELS == 919
    assert ds.labels.dtype == torch.uint8 and tuple(ds.labels.shape) == (4, 919)
    ids, tgt = ds.collate([ds[i] for i in range(len(ds))])
    assert tgt.dtype == torch.float32 and tuple(tgt.shape) == (4, 919)
    assert np.array_equal(ids.numpy(), GOLD["deepsea_ids"])
    assert np.array_equal(tgt.numpy(), GOLD["deepsea_targets"])


def test_deepsea_split_names_max_rows_and_errors(deepsea_dir, tmp_path):
    for split, n in {"train": 4, "val": 1, "valid": 1, "test": 3, "Test": 3}.items():
        assert len(DeepSEACsv(deepsea_dir, split, ML)) == n
    assert len(DeepSEACsv(deepsea_dir, "train", ML, max_rows=3)) == 3
    assert len(DeepSEACsv(deepsea_dir, "train", ML, max_rows=None)) == 4
    import inspect
    assert inspect.signature(DeepSEACsv).parameters["max_rows"].default == 40000
    with pytest.raises(ValueError, match="dev"):
        DeepSEACsv(deepsea_dir, "dev", ML)
    os.remove(os.path.join(deepsea_dir, "valid.csv.gz"))
    with pytest.raises(FileNotFoundError, match="valid.csv.gz"):
        DeepSEACsv(deepsea_dir, "val", ML)
    _write_deepsea(deepsea_dir, "valid", ["ACGT"], [[0, 1, 0]])
    with pytest.raises(ValueError, match="4 columns"):
        DeepSEACsv(deepsea_dir, "val", ML)


@pytest.mark.parametrize("which", ["deepstarr", "deepsea"])
def test_rc_aug_return_mask_and_eos(which, deepstarr_dir, deepsea_dir):
    def make(**kw):
        if which == "deepstarr":
            return DeepSTARRFolder(deepstarr_dir, "train", ML, **kw)
        return DeepSEACsv(deepsea_dir, "train", ML, **kw)

    plain = make()
    seqs = plain.all_seqs
    aug = make(rc_aug=True, rng=random.Random(5))
    draws = random.Random(5)
    for rep in range(3):
        for i in range(len(aug)):
            flipped = draws.random() < 0.5
            want = plain._item(string_reverse_complement(seqs[i]) if flipped else seqs[i], None)[0]
            ids, target = aug[i]  # one access, one draw
            assert torch.equal(ids, want)
            assert torch.equal(target, plain[i][1])  # the targets do not depend on the strand
    masked = make(return_mask=True)
    for i in range(len(masked)):
        ids, _, mask = masked[i]
        assert mask.dtype == torch.bool and torch.equal(mask, ids != masked.pad_token_id)
        assert int(mask.sum()) == min(len(seqs[i]), ML)
        assert not mask[: ML - int(mask.sum())].any()  # the padding is on the left
    eos = make(add_eos=True)
    sep = eos.tokenizer.sep_token_id
    for i in range(len(eos)):
        assert eos[i][0][-1].item() == sep and eos[i][0].numel() == ML
    assert len(masked.collate([masked[0], masked[1]])) == 3


# ------------------------------------------------------------------------------------ metrics
def test_pearson_matches_the_reference_and_corrcoef():
    outs, y = torch.tensor(GOLD["mse_outs"]), torch.tensor(GOLD["mse_y"])
    m = tasks.PearsonR()
    m.update(outs, y)
    got = m.compute()
    assert set(got) == {"pearsonr_dev", "pearsonr_hk", "pearsonr_mean"}
    for k in got:  # scipy on fp32 arrays, as the reference calls it
        assert abs(got[k] - float(GOLD["mse_" + k])) <= 2e-6, k
    for c, k in enumerate(("pearsonr_dev", "pearsonr_hk")):
        ref = torch.corrcoef(torch.stack([outs[:, c].double(), y[:, c].double()]))[0, 1].item()
        assert abs(got[k] - ref) <= 1e-12
    assert abs(got["pearsonr_mean"] - (got["pearsonr_dev"] + got["pearsonr_hk"]) / 2) <= 1e-15
    batched = tasks.PearsonR(names=("dev", "hk"))
    at = 0
    for n in (1, 9, 2, 11, 3, 7, 4):
        batched.update(outs[at:at + n], y[at:at + n].reshape(-1))  # targets in any shape
        at += n
    assert at == 37
    for k, v in batched.compute().items():
        assert abs(v - got[k]) <= 1e-12
    constant = tasks.PearsonR(names=("a",))
    constant.update(torch.ones(5, 1), torch.arange(5.0).reshape(5, 1))
    assert constant.compute()["pearsonr_a"] == 0.0


def _auc_pairs(x, y):
    """Brute force over all (positive, negative) pairs in float64; a tie counts 1/2."""
    pos, neg = x[y > 0.5].double(), x[y <= 0.5].double()
    d = pos[:, None] - neg[None, :]
    return ((d > 0).double().sum() + 0.5 * (d == 0).double().sum()).item() / (len(pos) * len(neg))


def _auroc_cases():
    g = torch.Generator().manual_seed(31)
    y = (torch.rand(64, 919, generator=g) < 0.4).float()
    x = torch.randn(64, 919, generator=g) + 0.7 * y
    ties = torch.randint(-2, 3, (64, 919), generator=g).float()  # five distinct values
    return {"random": (x, y), "ties": (ties, y)}


@pytest.mark.parametrize("case", ["random", "ties"])
def test_auroc_matches_pair_counting(case):
    x, y = _auroc_cases()[case]
    assert bool(((y.sum(0) > 0) & (y.sum(0) < 64)).all())  # no constant column: nothing skipped
    m = tasks.MultilabelAUROC(919)
    for lo, hi in ((0, 10), (10, 11), (11, 64)):
        m.update(x[lo:hi], y[lo:hi])
    assert m.labels[0].dtype == torch.uint8
    got = m.compute()
    assert got["roc_labels_skipped"] == 0
    ref = np.mean([_auc_pairs(x[:, c], y[:, c]) for c in range(919)])
    assert abs(got["roc"] - ref) <= 1e-12
    sk = pytest.importorskip("sklearn.metrics")
    assert abs(got["roc"] - sk.roc_auc_score(y.numpy(), x.double().numpy(), average="macro")) <= 1e-12


def test_auroc_skips_a_constant_label():
    x, y = _auroc_cases()["random"]
    x, y = x[:, :5].clone(), y[:, :5].clone()
    y[:, 2] = 1.0
    m = tasks.MultilabelAUROC(5)
    m.update(x, y)
    got = m.compute()
    assert got["roc_labels_skipped"] == 1
    ref = np.mean([_auc_pairs(x[:, c], y[:, c]) for c in (0, 1, 3, 4)])
    assert abs(got["roc"] - ref) <= 1e-12


# ------------------------------------------------------------------------- losses and configs
def test_loss_name_table():
    assert tasks.pool_loss("regression", "mse", 2) == ("regression", 1.0)
    assert tasks.pool_loss("regression", "customMSE", 2) == ("regression", 2.0)
    assert tasks.pool_loss("regression", "customMSE", 5) == ("regression", 5.0)
    assert tasks.pool_loss("regression", None, 2) == ("regression", 1.0)
    for name in ("binary_cross_entropy", "deepsea_loss"):
        assert tasks.pool_loss("multilabel_classification", name, 919) == (
            "multi_label_classification", 1.0)
    assert tasks.pool_loss("sequence_classification", None, 2) == (
        "single_label_classification", 1.0)
    with pytest.raises(ValueError, match="huber"):
        tasks.pool_loss("regression", "huber", 2)
    with pytest.raises(ValueError, match="ranking"):
        tasks.pool_loss("ranking", "mse", 2)
    with pytest.raises(ValueError, match="deepsea_loss"):
        tasks.pool_loss("regression", "deepsea_loss", 2)


def test_reference_losses_are_the_heads_loss_times_the_scale():
    """customMSE = C x the mean over B x C (what the head computes); deepsea_loss = BCE with
    logits, the mean over B x C."""
    import torch.nn.functional as F
    outs, y = torch.tensor(GOLD["mse_outs"]).double(), torch.tensor(GOLD["mse_y"]).double()
    _, scale = tasks.pool_loss("regression", "customMSE", 2)
    assert abs(scale * F.mse_loss(outs, y).item() - float(GOLD["mse_customMSE"])) <= 1e-6
    lg, lab = torch.tensor(GOLD["bce_logits"]).double(), torch.tensor(GOLD["bce_y"]).double()
    _, scale = tasks.pool_loss("multilabel_classification", "deepsea_loss", 919)
    assert abs(scale * F.binary_cross_entropy_with_logits(lg, lab).item()
               - float(GOLD["bce_deepsea_loss"])) <= 1e-6


def _dry_run(*overrides):
    import finetune as FT
    from dna_amd.compose import compose
    cfg = compose(os.path.join(os.path.dirname(HERE), "configs"), "config", list(overrides))
    out = io.StringIO()
    FT.finetune(cfg, dry_run=True, out=out)
    return json.loads(out.getvalue())


@pytest.mark.parametrize("experiment,num_labels,monitor,problem,scale,dataset", [
    ("hyena/deepstarr_hyena", 2, "test/pearsonr_mean", "regression", 2.0, "deepstarr"),
    ("hyena/deepsea_hyena", 919, "test/roc", "multi_label_classification", 1.0, "deepsea"),
    ("caduceus/deepstarr_caduceus", 2, "test/pearsonr_mean", "regression", 2.0, "deepstarr"),
])
def test_dry_run_builds_the_new_experiments(experiment, num_labels, monitor, problem, scale,
                                            dataset):
    info = _dry_run("experiment=" + experiment)
    assert info["num_labels"] == num_labels and info["monitor"] == monitor
    assert info["problem_type"] == problem and info["loss_scale"] == scale
    assert info["dataset"] == dataset and info["mode"] == "max"
    assert "t_initial" in info["scheduler"]


def test_dry_run_names_an_unknown_task_or_loss():
    with pytest.raises(ValueError, match="ranking"):
        _dry_run("experiment=hyena/deepstarr_hyena", "task._name_=ranking")
    with pytest.raises(ValueError, match="huber"):
        _dry_run("experiment=hyena/deepstarr_hyena", "task.loss=huber")
    with pytest.raises(ValueError, match="imagenet"):
        _dry_run("experiment=hyena/deepstarr_hyena", "dataset._name_=imagenet")


def test_evaluator_follows_the_problem_type():
    import finetune as FT
    m, on_logits = FT._metric("regression", 2)
    assert isinstance(m, tasks.PearsonR) and m.names == ("dev", "hk") and on_logits
    m, on_logits = FT._metric("multi_label_classification", 919)
    assert isinstance(m, tasks.MultilabelAUROC) and on_logits
    m, on_logits = FT._metric("single_label_classification", 3)
    assert isinstance(m, tasks.ConfusionMatrix) and not on_logits
