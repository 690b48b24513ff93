#!/usr/bin/env python
"""Classification-head measurements (GPU): the fused head (DF.ClsHead, csrc/cls_head.hip) against
the torch composition it replaces, and one fine-tuning step of the 117M model.

    python scripts/cls_head_ab.py [--out results.json] [--reps 50] [--no-step]

Head A/B: forward (with loss) + backward at (B, H, C) = (32, 768, 2) and (512, 768, 9), x = the
[CLS] rows of a [B*S, H] activation (S = 128). The torch arm is index_select -> fp32 F.linear ->
tanh -> dropout -> F.linear -> cross_entropy and its autograd. HIP events around each repetition,
the two arms interleaved, median after warm-up; kernel launches per repetition counted with
torch.profiler in a repetition of their own. Step: ClsTrainer at b = 32, S = 128, bf16, the
DNABERT-2-117M shape: HIP-event step time and the per-family OpTimer breakdown (a separate run
of steps, since the timer's events add host work).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dna_amd import functional as DF  # noqa: E402

DEV = "cuda"
MODEL_CFG = dict(vocab_size=4096, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                 intermediate_size=3072, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0,
                 layer_norm_eps=1e-12, pad_token_id=0, type_vocab_size=2, num_labels=2)


def _arms(B, H, C, S=128, p=0.1):
    g = torch.Generator().manual_seed(B + C)
    act = torch.randn(B * S, H, generator=g).to(DEV).requires_grad_(True)
    prm = [(torch.randn(*s, generator=g) * 0.03).to(DEV).requires_grad_(True)
           for s in ((H, H), (H,), (C, H), (C,))]
    labels = torch.randint(0, C, (B,), generator=g).to(DEV)
    rows = torch.arange(B, device=DEV) * S
    rng = DF.DropoutRNG(1)

    def clear():
        act.grad = None
        for q in prm:
            q.grad = None

    def fused():
        clear()
        _, loss, _ = DF.cls_head(act.view(B, S, H)[:, 0], *prm, p=p, rng=rng, labels=labels,
                                 problem_type="single_label_classification")
        loss.backward()

    def composed():
        clear()
        x = act.index_select(0, rows)
        a = F.dropout(torch.tanh(F.linear(x, prm[0], prm[1])), p, True)
        F.cross_entropy(F.linear(a, prm[2], prm[3]), labels).backward()

    return fused, composed


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def head_ab(reps, warmup=10):
    out = []
    for B, H, C in ((32, 768, 2), (512, 768, 9)):
        arms = dict(zip(("fused", "composed"), _arms(B, H, C)))
        for _ in range(warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():  # interleaved
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3)
        row = {"B": B, "H": H, "C": C, "reps": reps}
        for k in arms:
            row[f"{k}_us_median"] = round(statistics.median(times[k]), 2)
            row[f"{k}_us_min"] = round(min(times[k]), 2)
            row[f"{k}_launches"] = _launches(arms[k])
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def finetune_step(steps=20, warmup=5, b=32, S=128):
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.trainer import ClsTrainer
    torch.manual_seed(0)
    tr = ClsTrainer(BertForSequenceClassification(MODEL_CFG, precision="bf16"), DEV, seed=1)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(5, 4096, (b, S), generator=g)
    ids[:, 0] = 1
    ids[::4, 100:] = 3
    ids, labels = ids.to(DEV), torch.randint(0, 2, (b,), generator=g).to(DEV)
    for _ in range(warmup):
        tr.step(ids, labels)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.step(ids, labels)
        e.record()
        e.synchronize()
        ts.append(a.elapsed_time(e))
    with DF.OpTimer() as timer:
        for _ in range(5):
            tr.step(ids, labels)
        torch.cuda.synchronize()
    fam = {k: {"launches_per_step": n / 5, "ms_per_step": round(n * ms / 5, 4)}
           for k, (n, ms, _, _) in sorted(timer.summary().items())}
    row = {"b": b, "S": S, "precision": "bf16", "step_ms_median": round(statistics.median(ts), 3),
           "step_ms_min": round(min(ts), 3), "families": fam,
           "families_ms_sum": round(sum(v["ms_per_step"] for v in fam.values()), 3)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cls_head_ab.py measures on the GPU; none found")
    res = {"head": head_ab(a.reps)}
    if not a.no_step:
        res["finetune_step"] = finetune_step()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
