#!/usr/bin/env python
"""Golden fixture for the regression / multi-label fine-tuning tasks, produced by running the
REFERENCE code.

Run from the repo root:  python tests/golden/make_regression_golden.py
Imports the reference's src/tasks/metrics.py by path and its src/dataloaders/datasets/deepstarr.py
and deepsea.py as modules (read-only, never copied), with stand-ins for the packages this image
lacks: those of WANTED below (torchmetrics, genomic_benchmarks, torchvision, polars, pyfaidx,
Lightning, Hydra, ...) that no real finder locates become empty modules whose attributes are
empty classes. Writes tests/golden/regression_tasks.npz:

  mse_*        outs, y fp32 [37, 2] -> customMSE, pearsonr_dev, pearsonr_hk, pearsonr_mean (the
               three metrics as scipy returns them on the whole batch)
  bce_*        logits fp32, y 0/1 [16, 919] -> deepsea_loss
  deepstarr_*  a tiny Sequences_Train.fa / Sequences_activity_Train.txt (sequences as strings,
               the table's two target columns and one more column) and what
               DeepSTARRDataset.__getitem__ returns for every item: ids, targets
  deepsea_*    a tiny train.csv.gz (sequences, labels uint8 [n, 919]) and what
               DeepSEADataset.__getitem__ returns: ids, targets
The datasets are given this project's CharacterTokenizer (dna_amd/tokenizer.py, itself checked
against the reference's by char_golden.npz): the reference's own does not construct under the
installed transformers. max_length 12, left padding, no eos, no augmentation.
"""
import gzip
import importlib.abc
import importlib.machinery
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = os.environ.get("DNA_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
MAX_LENGTH = 12


class _StandInClass(type):
    def __getattr__(cls, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _StandInClass(k, (), {})

    def __call__(cls, *a, **k):
        if len(a) == 1 and callable(a[0]) and not k:  # used as a decorator
            return a[0]
        return super().__call__()


class _StandInModule(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _StandInClass(k, (), {})


# what the reference's modules import (directly or through src/dataloaders/__init__.py); those
# that are not installed are stood in for
WANTED = ("torchmetrics", "genomic_benchmarks", "torchvision", "polars", "pyfaidx", "liftover",
          "pytorch_lightning", "hydra", "omegaconf", "torchtext", "torchaudio")


class _AbsentPackages(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Last on sys.meta_path: asked only for what nothing else found."""
    stood_in = set()

    def find_spec(self, name, path, target=None):
        top = name.split(".")[0]
        if top in WANTED:
            self.stood_in.add(top)
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _StandInModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, m):
        pass


def _by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    from dna_amd.tokenizer import CharacterTokenizer
    sys.meta_path.append(_AbsentPackages())
    metrics = _by_path("ref_metrics", "src/tasks/metrics.py")
    import src.dataloaders.datasets.deepsea as ref_deepsea
    import src.dataloaders.datasets.deepstarr as ref_deepstarr

    rng = np.random.default_rng(2222)
    out = {}
    y = rng.standard_normal((37, 2)).astype(np.float32)
    outs = (0.6 * y + 0.8 * rng.standard_normal((37, 2)) + 0.3).astype(np.float32)
    ot, yt = torch.tensor(outs), torch.tensor(y)
    out["mse_outs"], out["mse_y"] = outs, y
    out["mse_customMSE"] = np.float64(metrics.customMSE(ot, yt).double().item())
    for name in ("pearsonr_dev", "pearsonr_hk", "pearsonr_mean"):
        out["mse_" + name] = np.float64(getattr(metrics, name)(ot, yt))
    logits = (2.0 * rng.standard_normal((16, 919))).astype(np.float32)
    labels = (rng.random((16, 919)) < 0.4).astype(np.float32)
    out["bce_logits"], out["bce_y"] = logits, labels
    out["bce_deepsea_loss"] = np.float64(
        metrics.deepsea_loss(torch.tensor(logits), torch.tensor(labels)).double().item())

    tok = CharacterTokenizer(["A", "C", "G", "T", "N"], MAX_LENGTH + 2, padding_side="left")
    kw = dict(max_length=MAX_LENGTH, tokenizer=tok, use_padding=True, add_eos=False, rc_aug=False)
    base = np.array(list("ACGTN"))
    lengths = [5, 12, 20, 1, 13]
    seqs = ["".join(base[rng.integers(0, 5, n)]) for n in lengths]
    table = rng.standard_normal((len(seqs), 3)).astype(np.float32)  # dev, another column, hk
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "Sequences_Train.fa"), "w") as f:
            for i, s in enumerate(seqs):
                f.write(f">seq{i}\n{s}\n")
        with open(os.path.join(tmp, "Sequences_activity_Train.txt"), "w") as f:
            f.write("Dev_log2_enrichment\tother\tHk_log2_enrichment\n")
            for r in table:
                f.write("\t".join(repr(float(v)) for v in r) + "\n")
        ds = ref_deepstarr.DeepSTARRDataset("train", dest_path=tmp, **kw)
        items = [ds[i] for i in range(len(ds))]
        out["deepstarr_seqs"] = np.array(seqs)
        out["deepstarr_table"] = table
        out["deepstarr_ids"] = np.stack([i[0].numpy() for i in items]).astype(np.int64)
        out["deepstarr_targets"] = np.stack([i[1].numpy().reshape(-1) for i in items])

        sea_seqs = ["".join(base[rng.integers(0, 4, n)]) for n in (12, 30, 7, 12)]
        sea_labels = (rng.random((len(sea_seqs), 919)) < 0.1).astype(np.uint8)
        with gzip.open(os.path.join(tmp, "train.csv.gz"), "wt") as f:
            for s, row in zip(sea_seqs, sea_labels):
                f.write(s + "," + ",".join(str(int(v)) for v in row) + "\n")
        ds = ref_deepsea.DeepSEADataset("train", dest_path=tmp, **kw)
        items = [ds[i] for i in range(len(ds))]
        out["deepsea_seqs"] = np.array(sea_seqs)
        out["deepsea_labels"] = sea_labels
        out["deepsea_ids"] = np.stack([i[0].numpy() for i in items]).astype(np.int64)
        out["deepsea_targets"] = np.stack([i[1].numpy().reshape(-1) for i in items]).astype(np.float32)
    out["max_length"] = np.array(MAX_LENGTH)
    path = os.path.join(HERE, "regression_tasks.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes); stand-ins: "
          f"{sorted(_AbsentPackages.stood_in)}")


if __name__ == "__main__":
    main()
