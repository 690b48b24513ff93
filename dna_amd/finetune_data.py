"""Labelled-sequence data for fine-tuning: GUE-layout folders (the DNABERT-2 benchmark's
`train.csv` / `dev.csv` / `test.csv`, each row `sequence,label`), tokenised with the C++ BPE
tokenizer as [CLS] ... [SEP], truncated to max_length, padded per batch."""
import csv
import os

import torch

from .tokenizer import DNABertTokenizer

SPLITS = ("train", "dev", "test")


def _is_int(s):
    try:
        int(s)
        return True
    except ValueError:
        return False


def read_csv(path):
    """-> (sequences, int labels); a first row whose label is not an integer is a header."""
    seqs, labels = [], []
    with open(path, newline="") as f:
        for i, row in enumerate(csv.reader(f)):
            if len(row) < 2:
                continue
            if i == 0 and not _is_int(row[1].strip()):
                continue
            seqs.append(row[0].strip())
            labels.append(int(row[1]))
    return seqs, labels


class SequenceClassificationCSV(torch.utils.data.Dataset):
    """One split of a GUE-layout folder. Items are (ids int64 [n <= max_length], label); the whole
    split is tokenised once at construction (GUE splits are a few thousand short sequences)."""

    def __init__(self, data_dir, split="train", max_length=128, tokenizer=None):
        if split not in SPLITS:
            raise ValueError(f"split {split!r}: one of {SPLITS}")
        self.path = os.path.join(data_dir, f"{split}.csv")
        if not os.path.exists(self.path):
            raise FileNotFoundError(f"{self.path}: a GUE folder holds train.csv, dev.csv, test.csv")
        self.max_length = int(max_length)
        self.tokenizer = tokenizer or DNABertTokenizer()
        seqs, labels = read_csv(self.path)
        self.labels = torch.tensor(labels, dtype=torch.int64)
        self.ids = [torch.tensor(self.tokenizer(s, max_length=self.max_length, truncation=True)
                                 ["input_ids"], dtype=torch.int64) for s in seqs]
        self.num_labels = int(self.labels.max()) + 1 if labels else 0

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        return self.ids[i], self.labels[i]

    @property
    def pad_token_id(self):
        return self.tokenizer.pad_token_id

    def collate(self, items):
        return collate_padded(items, self.pad_token_id)


def collate_padded(items, pad_token_id=3, multiple=64):
    """[(ids, label)] -> (ids [b, W] int64, labels [b]): W = the batch maximum rounded up to
    `multiple` (the bf16 attention kernel's tile), [PAD] fill."""
    width = max(int(ids.numel()) for ids, _ in items)
    width = (width + multiple - 1) // multiple * multiple
    out = torch.full((len(items), width), pad_token_id, dtype=torch.int64)
    for r, (ids, _) in enumerate(items):
        out[r, : ids.numel()] = ids
    return out, torch.stack([torch.as_tensor(l) for _, l in items])
