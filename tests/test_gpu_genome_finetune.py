"""finetune.main on synthetic genomes: the species and chromatin-profile experiments end to end,
with the genome resident on the device and item by item (the first forward sees identical ids on
both paths, so its loss is the same number)."""
import functools
import io
import json
import math
import os
import random
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import genome_fixtures as GF  # noqa: E402

pytestmark = pytest.mark.gpu

SPECIES = ["mouse", "hippo"]


def _species_genomes(root):
    """Chromosomes of 1,500-2,500 bp; mouse is A/C-rich and hippo G/T-rich."""
    from dna_amd.finetune_data import SPECIES_SPLITS
    rng = random.Random(5)
    for spec, rich in zip(SPECIES, ("AC", "GT")):
        os.makedirs(os.path.join(root, spec))
        for split in ("train", "valid", "test"):
            for chrom in SPECIES_SPLITS[spec][split]:
                seq = "".join(rng.choice(rich) if rng.random() < 0.8 else rng.choice("ACGTNacgt")
                              for _ in range(rng.randint(1500, 2500)))
                with open(os.path.join(root, spec, f"chr{chrom}.fna"), "w") as f:
                    f.write(f">chr{chrom}\n" + "\n".join(seq[i:i + 80]
                                                         for i in range(0, len(seq), 80)) + "\n")


def _run(monkeypatch, ckpt, *overrides):
    import finetune as FT
    out = io.StringIO()
    monkeypatch.setattr(FT, "finetune", functools.partial(FT.finetune, out=out))
    metrics = FT.main([*overrides, "trainer.max_epochs=1", "trainer.log_every_n_steps=1",
                       f"callbacks.model_checkpoint.dirpath={ckpt}"])
    return [json.loads(l) for l in out.getvalue().splitlines()], metrics


def test_species_resident_then_item_by_item(monkeypatch, tmp_path):
    root = str(tmp_path / "genomes")
    os.makedirs(root)
    _species_genomes(root)
    common = ["experiment=hyena/species_hyena", f"dataset.species_dir={root}",
              f"dataset.species=[{','.join(SPECIES)}]", "dataset.max_length=256",
              "model.layer.l_max=258", "dataset.total_size=16", "dataset.batch_size=4",
              "dataset.eval_batch_size=8"]
    runs = {}
    for resident in ("true", "false"):
        ckpt = str(tmp_path / f"ck_{resident}")
        events, metrics = _run(monkeypatch, ckpt, *common, f"dataset.resident={resident}")
        kinds = [e["event"] for e in events]
        assert kinds[0] == "start" and kinds.count("train") == 4 and kinds[-1] == "eval"
        assert events[0] == {"event": "start", "train": 16, "dev": 16, "test": 16,
                             "num_labels": 2, "batch_size": 4}
        assert all(math.isfinite(e["trainer/loss"]) for e in events if e["event"] == "train")
        for split in ("val", "test"):
            assert math.isfinite(metrics[f"{split}/loss"])
            for k in ("accuracy_per_class", "precision_per_class", "recall_per_class"):
                assert len(metrics[f"{split}/{k}"]) == 2, k
                assert all(0.0 <= v <= 1.0 for v in metrics[f"{split}/{k}"])
        assert json.loads(json.dumps(events[-1]))["val/recall_per_class"] == \
            metrics["val/recall_per_class"]
        runs[resident] = (events, metrics, ckpt)
    # the same seeds, the same windows: the first forward reads the same ids
    (ev_r, m_r, ckpt), (ev_h, m_h, _) = runs["true"], runs["false"]
    first = lambda ev: [e["trainer/loss"] for e in ev if e["event"] == "train"][0]
    assert first(ev_r) == first(ev_h)
    # accuracy is the support-weighted mean of the per-class recall; the support is what the
    # splits' shared generator drew after the train epoch's 16 windows
    import finetune as FT
    from dna_amd.compose import compose
    cfg = compose(os.path.join(ROOT, "configs"), "config", common)
    twin = FT._pool_splits(cfg.dataset, FT._char_tokenizer(256), 256, seed=cfg.train.seed)
    twin["train"].rows(16)
    for split, name in (("dev", "val"), ("test", "test")):
        targets = twin[split].rows(16)[3].tolist()
        support = [targets.count(c) for c in range(2)]
        assert m_r[f"{name}/accuracy"] == pytest.approx(
            sum(r * s for r, s in zip(m_r[f"{name}/recall_per_class"], support)) / 16, abs=1e-12)
    # last.ckpt reloads into the classifier
    events, _ = _run(monkeypatch, str(tmp_path / "ck_again"), *common, "dataset.resident=true",
                     f"train.pretrained_model_path={os.path.join(ckpt, 'last.ckpt')}",
                     "train.max_steps=1")
    assert events[0]["event"] == "load_backbone" and events[0]["loaded"] == "classifier"
    saved = torch.load(os.path.join(ckpt, "last.ckpt"), map_location="cpu", weights_only=False)
    assert len(saved["state_dict"]) > 0


def test_chromatin_profile_resident_then_item_by_item(monkeypatch, tmp_path):
    gold, fa = GF.chromatin_folder(tmp_path)
    common = ["experiment=hyena/chromatin_profile_hyena", f"dataset.data_path={tmp_path}",
              f"dataset.ref_genome_path={fa}", "dataset.batch_size=4", "dataset.eval_batch_size=8",
              "dataset.train_len=9"]
    runs = {}
    for resident in ("true", "false"):
        ckpt = str(tmp_path / f"ck_{resident}")
        events, metrics = _run(monkeypatch, ckpt, *common, f"dataset.resident={resident}")
        kinds = [e["event"] for e in events]
        assert kinds[0] == "start" and kinds.count("train") == 3 and kinds[-1] == "eval"
        assert events[0] == {"event": "start", "train": 9, "dev": 9, "test": 9, "num_labels": 7,
                             "batch_size": 4}
        assert all(math.isfinite(e["trainer/loss"]) for e in events if e["event"] == "train")
        for k in ("val/loss", "test/loss", "val/roc", "test/roc"):
            assert math.isfinite(metrics[k]), k
        assert "val/recall_per_class" not in metrics  # task.metrics does not name it
        assert os.path.exists(os.path.join(ckpt, "last.ckpt"))
        runs[resident] = (events, metrics)
    first = lambda ev: [e["trainer/loss"] for e in ev if e["event"] == "train"][0]
    assert first(runs["true"][0]) == first(runs["false"][0])  # the same ids on both paths
    events, _ = _run(monkeypatch, str(tmp_path / "ck_again"), *common, "dataset.resident=true",
                     f"train.pretrained_model_path={tmp_path / 'ck_true' / 'last.ckpt'}",
                     "train.max_steps=1")
    assert events[0]["event"] == "load_backbone" and events[0]["loaded"] == "classifier"
