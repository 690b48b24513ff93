#!/usr/bin/env python
"""Generate the sequence-classification parity fixtures by running the REFERENCE code on the CPU.

Run from the repo root:  python tests/golden/make_cls_golden.py
Needs the reference checkout (DNA_REFERENCE, imported by path, never copied) and `transformers`.
Writes only data files next to this script:

  cls_tiny.npz            reference BertForSequenceClassification / BertModel
                          (src/models/DNABERT2/bert_layers.py:881-1009, :531-644), hash-initialised
                          (oracle/hashinit.py), eval mode, 2 layers, d = 128, 2 heads, ff = 256, on
                          one 5 x 72 batch (neither a tile multiple; one full row, rows padded at 40
                          and at 7 tokens, [CLS] = 1 in column 0), for three heads:
                            c3  3 labels, single_label_classification (int64 labels)
                            c1  1 label,  regression
                            c4  4 labels, multi_label_classification (float labels)
                          per head: labels, fp32 logits and loss, the logits under CPU bf16
                          autocast, and the gradients of the embedding / pooler / classifier
                          parameters; once: ids, BertModel's sequence_output and pooled_output.
  cls_tiny_grad_<head>_l<i>.npz   the gradients of encoder layer i's parameters for that head
                          (full arrays; one file per layer keeps every file under 1 MiB).

The generator is the only place that imports the reference; tests read the fixtures alone.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shims, REF, PAD, VOCAB; puts the repo root on sys.path)

from oracle.hashinit import hash_tensor  # noqa: E402

LAYERS, D, HEADS, FF = 2, 128, 2, 256
B, S = 5, 72
HEADS_CFG = {"c3": (3, "single_label_classification"), "c1": (1, "regression"),
             "c4": (4, "multi_label_classification")}


def _config(num_labels, problem_type):
    import transformers
    d = mg._model_cfg(LAYERS, D, HEADS, FF)
    d.pop("hyena_framework")
    d.update(num_labels=num_labels, problem_type=problem_type, classifier_dropout=None)
    return transformers.BertConfig.from_dict(d)


def _ref_model(num_labels, problem_type):
    from src.models.DNABERT2 import bert_layers as bl
    m = bl.BertForSequenceClassification(_config(num_labels, problem_type))
    sd = {k: torch.from_numpy(hash_tensor(k, tuple(v.shape))) for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    return m.eval()


def _batch(rng):
    ids = rng.integers(5, mg.VOCAB, size=(B, S))
    ids[:, 0] = 1  # [CLS]
    ids[:, -1] = 2  # [SEP]
    for r, n in {2: 40, 4: 7}.items():
        ids[r, n:] = mg.PAD
        ids[r, n - 1] = 2
    return ids


def _labels(tag, rng):
    if tag == "c3":
        return rng.integers(0, 3, size=(B,)).astype(np.int64)
    if tag == "c1":
        return rng.standard_normal((B,)).astype(np.float32)
    return (rng.random((B, 4)) < 0.4).astype(np.float32)


def main():
    mg._install_shims()
    sys.path.insert(0, mg.REF)
    torch.set_num_threads(8)
    rng = np.random.default_rng(4242)
    ids = _batch(rng)
    tids = torch.as_tensor(ids)
    amask = (tids != mg.PAD).long()
    res = dict(input_ids=ids.astype(np.int16),
               config=np.bytes_(json.dumps([LAYERS, D, HEADS, FF])))
    for tag, (C, problem) in HEADS_CFG.items():
        labels = _labels(tag, rng)
        tl = torch.as_tensor(labels)
        m = _ref_model(C, problem)
        out = m(input_ids=tids, attention_mask=amask, labels=tl, return_dict=True)
        out.loss.backward()
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
            out16 = _ref_model(C, problem)(input_ids=tids, attention_mask=amask, return_dict=True)
        res[f"{tag}/labels"] = labels
        res[f"{tag}/logits"] = out.logits.detach().numpy()
        res[f"{tag}/loss"] = np.float64(out.loss.item())
        res[f"{tag}/logits_bf16"] = out16.logits.detach().float().numpy()
        per_layer = {i: {} for i in range(LAYERS)}
        for n, p in m.named_parameters():
            g = p.grad.detach().numpy()
            if n.startswith("bert.encoder.layer."):
                per_layer[int(n.split(".")[3])]["grad/" + n] = g
            else:
                res[f"{tag}/grad/{n}"] = g
        for i, d in per_layer.items():
            np.savez_compressed(os.path.join(HERE, f"cls_tiny_grad_{tag}_l{i}.npz"), **d)
        if tag == "c3":
            with torch.no_grad():
                seq, pooled = m.bert(tids, attention_mask=amask)
            res["sequence_output"] = seq.numpy()
            res["pooled_output"] = pooled.numpy()
        print(f"cls_tiny {tag}: loss {out.loss.item():.6f}, bf16 logit deviation "
              f"{np.abs(res[f'{tag}/logits_bf16'] - res[f'{tag}/logits']).max():.3e}")
    np.savez_compressed(os.path.join(HERE, "cls_tiny.npz"), **res)


if __name__ == "__main__":
    main()
