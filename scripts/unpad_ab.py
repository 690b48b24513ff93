#!/usr/bin/env python
"""Padded against packed fine-tuning step (GPU): what `finetune.py dataset.unpad=true` buys.

    python scripts/unpad_ab.py [--out results.json] [--rounds 7] [--steps 3] [--batches 32,128]
                               [--data-dir /data/GUE/prom/prom_300_all]

One process, DNABERT-2-117M in bf16, one ClsTrainer. For every batch size and length
distribution the same sequences run as
  arm A  the padded step: ids [b, S], S the batch maximum rounded up to 64 (collate_padded);
  arm B  the packed step: the same ids with their PackedIndex, T = sum(len) rows.
Rounds of `--steps` optimizer steps per arm alternate A, B, A, B, ... after a warm-up of both;
HIP events around each round; the table reports the median and the minimum step time per arm,
B/A of the medians, and the row ratio sum(len) / (b * S) that B/A should track. Before timing,
the eval-mode logits of both arms on the batch are compared (they must agree to bf16 accuracy).

Length distributions are synthetic, drawn once from a fixed seed: uniform 15-25, 55-75, 90-110
and 64-512 tokens, and all exactly 128 (nothing to save: the cost of the plainer attention
kernel). --data-dir adds the first sequences of a GUE folder's train split, tokenised.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
PAD = 3
MODEL_CFG = dict(vocab_size=4096, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                 intermediate_size=3072, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0,
                 layer_norm_eps=1e-12, pad_token_id=0, type_vocab_size=2, num_labels=2)
DISTRIBUTIONS = (("uniform 15-25", 15, 25), ("uniform 55-75", 55, 75), ("uniform 90-110", 90, 110),
                 ("uniform 64-512", 64, 512), ("all 128", 128, 128))


def batch_of(lengths, gen):
    """-> (ids padded to a multiple of 64, ids at the batch maximum, labels), host tensors."""
    from dna_amd.finetune_data import collate_padded
    items = []
    for n in lengths:
        ids = torch.randint(5, 4096, (int(n),), generator=gen)
        ids[0] = 1
        items.append((ids, torch.randint(0, 2, (), generator=gen)))
    padded, labels = collate_padded(items, PAD)
    tight, _ = collate_padded(items, PAD, multiple=1)
    return padded, tight, labels


def cases(batches, data_dir=None):
    gen = torch.Generator().manual_seed(20240)
    for b in batches:
        for name, lo, hi in DISTRIBUTIONS:
            lengths = torch.randint(lo, hi + 1, (b,), generator=gen).tolist()
            yield b, name, lengths, batch_of(lengths, gen)
        if data_dir:
            from dna_amd.finetune_data import SequenceClassificationCSV
            ds = SequenceClassificationCSV(data_dir, "train", max_length=512)
            lengths = [int(ds[i][0].numel()) for i in range(min(b, len(ds)))]
            if len(lengths) == b:
                yield b, os.path.basename(os.path.normpath(data_dir)), lengths, batch_of(lengths, gen)


def row_ratio(lengths, padded):
    return sum(lengths) / float(padded.numel())


def measure(tr, lengths, padded, tight, labels, rounds, steps, warmup=3):
    from dna_amd.bert_layers import PackedIndex
    packed = PackedIndex.build(tight, PAD).to(DEV)
    a_ids, b_ids, y = padded.to(DEV), tight.to(DEV), labels.to(DEV)
    arms = {"A": lambda: tr.step(a_ids, y), "B": lambda: tr.step(b_ids, y, packed=packed)}
    la = tr.evaluate(a_ids)[0]
    lb = tr.evaluate(b_ids, packed=packed)[0]
    diff = (la - lb).abs().max().item()
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():  # interleaved
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(steps):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) / steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"S_padded": int(padded.shape[1]), "rows_padded": int(padded.numel()),
            "rows_packed": int(sum(lengths)), "row_ratio": round(row_ratio(lengths, padded), 3),
            "A_ms_median": round(med["A"], 3), "A_ms_min": round(min(times["A"]), 3),
            "B_ms_median": round(med["B"], 3), "B_ms_min": round(min(times["B"]), 3),
            "B_over_A": round(med["B"] / med["A"], 3), "eval_logits_max_diff": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--data-dir", default=None)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("unpad_ab.py measures on the GPU; none found")
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.trainer import ClsTrainer
    torch.manual_seed(0)
    tr = ClsTrainer(BertForSequenceClassification(MODEL_CFG, precision="bf16"), DEV, lr=1e-5, seed=1)
    res = []
    for b, name, lengths, (padded, tight, labels) in cases(batches, a.data_dir):
        row = dict({"batch": b, "lengths": name},
                   **measure(tr, lengths, padded, tight, labels, a.rounds, a.steps))
        res.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
