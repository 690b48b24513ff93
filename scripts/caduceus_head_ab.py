#!/usr/bin/env python
"""Caduceus masked-LM training step (GPU): CaduceusForMaskedLM.mlm_loss (the fused head of
csrc/lm_head.hip; RC-equivariant for rcps) against forward(input_ids, labels) (dense logits, for
rcps two projections and a flipped copy of half the hidden state, fp32 cast, torch's cross entropy).

    python scripts/caduceus_head_ab.py [--out results.json] [--steps 20] [--warmup 5]

Two shapes, bf16 autocast, ModuleTrainer steps (forward, backward, clip + AdamW):
  experiment  configs/experiment/caduceus/bert_hg38_caduceus.yaml: rcps, d_model 256, 4 layers,
              B = 128, L = 1024
  config_e    BASELINE config E: rcps off, d_model 256, 8 layers, B = 1, L = 131072
HIP events around each step, the two arms interleaved, median after warm-up. Then a few steps of
the fused arm under functional.OpTimer: the head's own launches (lm_head[_rc]_fwd / _bwd).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dna_amd import functional as DF  # noqa: E402

DEV = "cuda"
SHAPES = {"experiment": dict(rcps=True, n_layer=4, B=128, L=1024, residual_in_fp32=False),
          "config_e": dict(rcps=False, n_layer=8, B=1, L=131072)}


def _arms(rcps, n_layer, B, L, residual_in_fp32=True):
    from dna_amd.caduceus import CaduceusForMaskedLM
    from dna_amd.hyena_lm import BlmIndex
    from dna_amd.tokenizer import CharacterTokenizer
    from dna_amd.trainer import ModuleTrainer
    g = torch.Generator(device=DEV).manual_seed(1)
    ids = torch.randint(7, 11, (B, L), device=DEV, generator=g)
    masked = torch.rand(B, L, device=DEV, generator=g) < 0.15
    inp = torch.where(masked, torch.full_like(ids, 3), ids)
    labels = torch.where(masked, ids, torch.full_like(ids, -100))
    index = BlmIndex.build(masked.cpu(), ids.cpu(), 16).to(DEV)
    kw = dict(d_model=256, n_layer=n_layer, vocab_size=12,
              residual_in_fp32=residual_in_fp32)
    if rcps:
        kw.update(rcps=True, complement_map=CharacterTokenizer(["A", "C", "G", "T", "N"],
                                                               L + 2).complement_map())
    losses = {"fused": lambda m, b: m.mlm_loss(inp, masked, index)[0],
              "dense": lambda m, b: m(inp, labels=labels)[0]}
    arms = {}
    for name, fn in losses.items():
        torch.manual_seed(0)
        tr = ModuleTrainer(CaduceusForMaskedLM(**kw), DEV, fn, lr=1e-3, weight_decay=0.1,
                           max_grad_norm=1.0)
        arms[name] = (lambda tr=tr: tr.step(None))
    return arms


def step_ab(name, steps, warmup):
    arms = _arms(**SHAPES[name])
    first = {k: float(fn()) for k, fn in arms.items()}
    for _ in range(warmup - 1):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(steps):
        for k, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    row = dict(shape=name, **SHAPES[name], dtype="bf16", steps=steps, warmup=warmup,
               loss_fused=first["fused"], loss_dense=first["dense"])
    for k, ts in times.items():
        row[f"{k}_ms_median"] = round(statistics.median(ts), 3)
        row[f"{k}_ms_min"] = round(min(ts), 3)
    row["fused_over_dense"] = round(row["fused_ms_median"] / row["dense_ms_median"], 4)
    with DF.OpTimer() as t:
        for _ in range(5):
            arms["fused"]()
        torch.cuda.synchronize()
    row["head_ms"] = {k: round(ms, 4) for k, (n, ms, _, _) in t.summary().items()
                      if k.startswith("lm_head")}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("caduceus_head_ab.py measures on the GPU; none found")
    res = {name: step_ab(name, a.steps, a.warmup) for name in a.shapes}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
