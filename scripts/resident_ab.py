#!/usr/bin/env python
"""A/B of the fine-tuning loop's two batch paths on a synthetic Nucleotide-Transformer-shaped task:
item-by-item (tokenise each string on the host, stack, copy) against a device-resident split
whose batches one HIP kernel builds (dna_amd.resident).

    python scripts/resident_ab.py [--rounds 5] [--steps 128] [--out resident_ab.json]

The script writes its own data (4,096 train and 1,024 test sequences of 500 bp, seeded) into a
temporary folder and, for denoise_cnn (experiment denoise/nt_denoise), dna_embedding
(hyena/nt_hyena) and caduceus_cls (caduceus/nt_caduceus) at batch 128, reports per path

  build   host time per batch for building the batch alone (item-by-item: tokenise + collate;
          resident: the launch, unsynchronised -- what the Python thread spends; `build_sync`
          is the same with a device synchronise, i.e. until the batch exists)
  step    wall time per training step over `--steps` steps ending in a synchronise, batch
          building and the host-to-device copies included, as finetune._fit runs them
  eval    wall time of one evaluation pass over the test split (finetune.evaluate)

after a warm-up of every shape, as the median over `--rounds` rounds that alternate the two
paths, with the min-max spread. The last column says whether the resident path wins by more
than the larger of the two spreads: the rule for dataset.resident in the NT experiments.
Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, LENGTH, N_TRAIN, N_TEST = 128, 500, 4096, 1024
MODELS = {"denoise_cnn": "denoise/nt_denoise", "dna_embedding": "hyena/nt_hyena",
          "caduceus_cls": "caduceus/nt_caduceus"}


def write_folder(root, name="synthetic"):
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, name))
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for split, n in (("train", N_TRAIN), ("test", N_TEST)):
        with open(os.path.join(root, name, f"{name}_{split}.fasta"), "w") as f:
            for i in range(n):
                seq = letters[rng.integers(0, 4, LENGTH)].tobytes().decode()
                f.write(f">{split}_{i}|{i % 2}\n{seq}\n")
    return name


def sync_time(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


def summary(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs),
            "max_ms": 1e3 * max(xs)}


def measure(model_name, experiment, root, task, rounds, steps, device):
    import finetune as FT
    from dna_amd.compose import compose
    from dna_amd.resident import ResidentSplit
    from dna_amd.trainer import SeqClsTrainer
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  [f"experiment={experiment}", f"dataset.dest_path={root}",
                   f"dataset.dataset_name={task}", f"dataset.max_length={LENGTH}",
                   "dataset.d_output=2", f"dataset.train_len={N_TRAIN}", "dataset.metric=mcc",
                   f"dataset.batch_size={BATCH}"])
    FT._nt_defaults(cfg)
    torch.manual_seed(0)
    tok = FT._char_tokenizer(LENGTH, cfg.dataset.get("padding_side", "left"))
    host = FT._pool_splits(cfg.dataset, tok, LENGTH)
    model = FT._pool_model(cfg, 2, tok)
    opt = cfg.optimizer.to_container()
    trainer = SeqClsTrainer(model, device, lr=float(opt["lr"]), weight_decay=float(opt["weight_decay"]),
                            scheduler=FT._scheduler(cfg), scheduler_name=FT._scheduler_name(cfg),
                            seed=0, autocast=torch.bfloat16)
    dev = {k: ResidentSplit.from_dataset(v, device) for k, v in (("train", host["train"]),
                                                                 ("test", host["test"]))}
    order = torch.randperm(N_TRAIN, generator=torch.Generator().manual_seed(0))
    dev["train"].set_epoch(order)
    order = order.tolist()
    starts = [(k * BATCH) % N_TRAIN for k in range(steps)]
    train = host["train"]

    def build_item():
        for i in starts:
            train.collate([train[j] for j in order[i:i + BATCH]])

    def build_resident():
        for i in starts:
            dev["train"].batch(i, i + BATCH)

    def steps_item():
        for i in starts:
            ids, labels = train.collate([train[j] for j in order[i:i + BATCH]])
            trainer.step(ids.to(device, non_blocking=True), labels.to(device, non_blocking=True))

    def steps_resident():
        for i in starts:
            trainer.step(*dev["train"].batch(i, i + BATCH))

    def eval_pass(split):
        return lambda: FT.evaluate(trainer, split, BATCH, device, 2)

    # the two paths must feed the model the same batches
    a = train.collate([train[j] for j in order[:BATCH]])
    b = dev["train"].batch(0, BATCH)
    assert all(torch.equal(x, y.cpu()) for x, y in zip(a, b)), "the two paths differ"
    # warm-up: every shape both paths use, the short last eval batch included
    for fn in (steps_item, steps_resident, eval_pass(host["test"]), eval_pass(dev["test"])):
        fn()
    torch.cuda.synchronize(device)
    res = {k: [] for k in ("build_item", "build_resident", "build_sync_resident", "step_item",
                           "step_resident", "eval_item", "eval_resident")}
    for _ in range(rounds):  # alternate the paths inside every round
        t0 = time.perf_counter()
        build_item()
        res["build_item"].append((time.perf_counter() - t0) / steps)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        build_resident()
        res["build_resident"].append((time.perf_counter() - t0) / steps)
        res["build_sync_resident"].append(sync_time(build_resident, device) / steps)
        res["step_item"].append(sync_time(steps_item, device) / steps)
        res["step_resident"].append(sync_time(steps_resident, device) / steps)
        res["eval_item"].append(sync_time(eval_pass(host["test"]), device))
        res["eval_resident"].append(sync_time(eval_pass(dev["test"]), device))
    out = {k: summary(v) for k, v in res.items()}
    for what in ("step", "eval"):
        it, rs = out[f"{what}_item"], out[f"{what}_resident"]
        spread = max(it["max_ms"] - it["min_ms"], rs["max_ms"] - rs["min_ms"])
        out[f"{what}_resident_wins"] = bool(it["median_ms"] - rs["median_ms"] > spread)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=128, help="training steps per timed window")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resident_ab.py measures on a GPU; none is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    result = {"batch": BATCH, "length": LENGTH, "train": N_TRAIN, "test": N_TEST,
              "rounds": a.rounds, "steps": a.steps, "device": torch.cuda.get_device_name(device),
              "models": {}}
    with tempfile.TemporaryDirectory() as root:
        task = write_folder(root)
        for name in a.models.split(","):
            result["models"][name] = measure(name, MODELS[name], root, task, a.rounds, a.steps, device)
    fmt = lambda s: f"{s['median_ms']:.2f} ({s['min_ms']:.2f}-{s['max_ms']:.2f})"
    print("| model | quantity | item-by-item ms | resident ms | resident wins by more than the spread |")
    print("|---|---|---|---|---|")
    for name, r in result["models"].items():
        print(f"| {name} | build per batch (host) | {fmt(r['build_item'])} | {fmt(r['build_resident'])}"
              f"; synchronised {fmt(r['build_sync_resident'])} | |")
        print(f"| {name} | training step | {fmt(r['step_item'])} | {fmt(r['step_resident'])} | "
              f"{'yes' if r['step_resident_wins'] else 'no'} |")
        print(f"| {name} | evaluation pass ({N_TEST} sequences) | {fmt(r['eval_item'])} | "
              f"{fmt(r['eval_resident'])} | {'yes' if r['eval_resident_wins'] else 'no'} |")
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
