"""finetune.main on a toy Nucleotide Transformer folder: the NT experiments end to end with the
splits resident on the device, and the first step's loss against the item-by-item path's (the
forward sees identical ids, so it is the same number)."""
import functools
import io
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _toy_folder(root, name="toy"):
    """64 train and 32 test sequences of at most 40 bp: label 0 is A/C-rich, label 1 G/T-rich."""
    rng = np.random.default_rng(7)
    os.makedirs(os.path.join(root, name))
    for split, n in (("train", 64), ("test", 32)):
        with open(os.path.join(root, name, f"{name}_{split}.fasta"), "w") as f:
            for i in range(n):
                label = i % 2
                rich = "GT" if label else "AC"
                seq = "".join(rng.choice(list(rich)) if rng.random() < 0.85 else
                              rng.choice(list("ACGTN")) for _ in range(40 - int(rng.integers(0, 9))))
                f.write(f">{split}_{i}|{label}\n{seq[:25]}\n{seq[25:]}\n")


def _run(monkeypatch, tmp_path, experiment, resident, *extra):
    import finetune as FT
    out = io.StringIO()
    monkeypatch.setattr(FT, "finetune", functools.partial(FT.finetune, out=out))
    ckpt = os.path.join(str(tmp_path), f"ck_{experiment.split('/')[0]}_{resident}")
    metrics = FT.main([f"experiment={experiment}", f"dataset.dest_path={tmp_path}",
                       "dataset.dataset_name=toy", "dataset.max_length=40", "dataset.d_output=2",
                       "dataset.train_len=64", "dataset.metric=mcc", "dataset.batch_size=16",
                       "dataset.eval_batch_size=16", "trainer.max_epochs=1",
                       "trainer.log_every_n_steps=1", f"dataset.resident={resident}",
                       f"callbacks.model_checkpoint.dirpath={ckpt}", *extra])
    return [json.loads(l) for l in out.getvalue().splitlines()], metrics, ckpt


@pytest.mark.parametrize("experiment,extra", [
    ("denoise/nt_denoise", ()), ("hyena/nt_hyena", ("model.layer.l_max=40",))])
def test_nt_experiment_resident_then_item_by_item(monkeypatch, tmp_path, experiment, extra):
    _toy_folder(str(tmp_path))
    events, metrics, ckpt = _run(monkeypatch, tmp_path, experiment, "true", *extra)
    kinds = [e["event"] for e in events]
    assert kinds[0] == "start" and kinds.count("train") == 4 and kinds[-1] == "eval"
    assert events[0] == {"event": "start", "train": 64, "dev": 32, "test": 32, "num_labels": 2,
                         "batch_size": 16}
    for k in ("val/mcc", "test/mcc", "val/loss", "test/loss"):
        assert math.isfinite(metrics[k]), (k, metrics[k])
    assert metrics["val/mcc"] == metrics["test/mcc"]  # both are the test file
    assert os.path.exists(os.path.join(ckpt, "last.ckpt"))
    steps = [e for e in events if e["event"] == "train"]
    assert all(math.isfinite(e["trainer/loss"]) for e in steps)
    # the cosine schedule of a 4-step run: warmup_t = 0.04 steps, so step 1 is on the cosine
    want_lr = 1e-4 + (1e-3 - 1e-4) * 0.5 * (1 + math.cos(math.pi * 1 / 4))
    assert steps[0]["lr"] == pytest.approx(want_lr, rel=1e-9)
    # the same seed on the item-by-item path: the first forward reads the same ids
    events2, _, _ = _run(monkeypatch, tmp_path, experiment, "false", "train.max_steps=1", *extra)
    first = [e for e in events2 if e["event"] == "train"][0]
    assert first["trainer/loss"] == steps[0]["trainer/loss"]
