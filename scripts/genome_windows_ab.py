#!/usr/bin/env python
"""A/B of the fine-tuning loop's two batch paths for the datasets that cut windows out of whole
genomes: item by item (slice the chromosome, tokenise the string on the host, stack, copy)
against a device-resident genome whose batches one HIP kernel builds (resident.ResidentWindows).

    python scripts/genome_windows_ab.py [--rounds 5] [--steps 16] [--out genome_windows_ab.json]

The script writes its own data (seeded) into a temporary folder -- two species with chromosomes
of 200,000 bp, and a three-record genome of 1,000,000 bp each with 4,000 + 1,000 coordinate rows
of 919 labels -- and measures hyena/species_hyena and caduceus/species_caduceus at windows of
1,024 and 32,768 bases (batch 8) and hyena/chromatin_profile_hyena at batch 1,000 x 1,024:

  step    wall time per training step over `--steps` steps ending in a synchronise, batch
          building included as finetune._fit runs it (resident: the pass's set_epoch -- the
          host's draws and one upload -- is inside the timed window)
  eval    wall time of one finetune.evaluate pass over the validation split

after a warm-up of every shape, as the median over `--rounds` rounds that alternate the two
paths, with the min-max spread. "wins" says whether the resident path is faster by more than the
larger of the two spreads: the rule for dataset.resident in the three experiments. Also printed:
the bytes each resident split holds on the device. Needs a GPU; there is no CPU fallback.
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

SPECIES = ["mouse", "hippo"]
CHROM_BP, GENOME_BP, ROWS_TRAIN, ROWS_EVAL, LABELS = 200_000, 1_000_000, 4000, 1000, 919
CASES = [  # (name, experiment, window, batch, eval batch)
    ("species_hyena L=1024", "hyena/species_hyena", 1024, 8, 16),
    ("species_hyena L=32768", "hyena/species_hyena", 32768, 8, 16),
    ("species_caduceus L=1024", "caduceus/species_caduceus", 1024, 8, 16),
    ("species_caduceus L=32768", "caduceus/species_caduceus", 32768, 8, 16),
    ("chromatin_profile_hyena 1000 x 1024", "hyena/chromatin_profile_hyena", 1024, 1000, 1000),
]


def _fasta(path, records, rng):
    letters = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
    with open(path, "w") as f:
        for name, n in records:
            seq = letters[rng.choice(9, n, p=[.22, .22, .22, .22, .025, .025, .025, .025, .02])]
            f.write(f">{name}\n")
            f.write(b"\n".join(seq[i:i + 80].tobytes() for i in range(0, n, 80)).decode() + "\n")


def write_data(root):
    from dna_amd.finetune_data import SPECIES_SPLITS
    rng = np.random.default_rng(0)
    for spec in SPECIES:
        os.makedirs(os.path.join(root, "species", spec))
        for split in ("train", "valid", "test"):
            for chrom in SPECIES_SPLITS[spec][split]:
                _fasta(os.path.join(root, "species", spec, f"chr{chrom}.fna"),
                       [(f"chr{chrom}", CHROM_BP)], rng)
    os.makedirs(os.path.join(root, "chromatin"))
    _fasta(os.path.join(root, "chromatin", "genome.fa"),
           [(f"chr{i + 1}", GENOME_BP) for i in range(3)], rng)
    header = ",".join(["Chr_No", "Start", "End"] + [f"y_{i}" for i in range(LABELS)])
    for split, n in (("train", ROWS_TRAIN), ("val", ROWS_EVAL), ("test", ROWS_EVAL)):
        starts = rng.integers(0, GENOME_BP - 1000, n)
        starts[:4] = (0, 3, GENOME_BP - 1000, GENOME_BP - 1003)  # windows off both ends
        labels = rng.integers(0, 2, (n, LABELS))
        with open(os.path.join(root, "chromatin", f"{split}_hg38_coords_targets.csv"), "w") as f:
            f.write(header + "\n")
            for i in range(n):
                f.write(f"{i % 3},{starts[i]},{starts[i] + 1000},"
                        + ",".join(map(str, labels[i].tolist())) + "\n")


def sync_time(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


def summary(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs),
            "max_ms": 1e3 * max(xs)}


def measure(experiment, window, batch, eval_batch, root, rounds, steps, device):
    import finetune as FT
    from dna_amd.compose import compose
    from dna_amd.resident import ResidentWindows
    from dna_amd.trainer import SeqClsTrainer
    over = [f"experiment={experiment}", f"dataset.max_length={window}",
            f"dataset.batch_size={batch}"]
    if "species" in experiment:
        over += [f"dataset.species_dir={os.path.join(root, 'species')}",
                 f"dataset.species=[{','.join(SPECIES)}]", f"dataset.total_size={steps * batch}"]
    else:
        over += [f"dataset.data_path={os.path.join(root, 'chromatin')}",
                 f"dataset.ref_genome_path={os.path.join(root, 'chromatin', 'genome.fa')}"]
    if "hyena" in experiment:
        over.append(f"model.layer.l_max={window + 2}")
    cfg = compose(os.path.join(ROOT, "configs"), "config", over)
    FT._genome_defaults(cfg)
    torch.manual_seed(0)
    tok = FT._char_tokenizer(window)
    host = FT._pool_splits(cfg.dataset, tok, window, seed=0)
    species = "species" in experiment
    # species: a twin set of splits on a generator of its own, seeded alike
    twin = FT._pool_splits(cfg.dataset, tok, window, seed=0) if species else host
    if species:  # a short validation pass: 4 eval batches
        for s in (host, twin):
            s["dev"].total_size = 4 * eval_batch
    num_labels = host["train"].num_labels
    model = FT._pool_model(cfg, num_labels, tok)
    opt = cfg.optimizer.to_container()
    trainer = SeqClsTrainer(model, device, lr=float(opt["lr"]),
                            weight_decay=float(opt["weight_decay"]), scheduler=FT._scheduler(cfg),
                            scheduler_name=FT._scheduler_name(cfg), seed=0, autocast=torch.bfloat16)
    dev = {k: ResidentWindows.from_dataset(twin[k], device) for k in ("train", "dev")}
    train, n = host["train"], steps * batch
    order = list(range(n)) if species else torch.randint(
        len(train), (n,), generator=torch.Generator().manual_seed(0)).tolist()

    def steps_item():
        for i in range(0, n, batch):
            ids, labels = train.collate([train[j] for j in order[i:i + batch]])
            trainer.step(ids.to(device, non_blocking=True), labels.to(device, non_blocking=True))

    def steps_resident():
        dev["train"].set_epoch(order)
        for i in range(0, n, batch):
            trainer.step(*dev["train"].batch(i, i + batch))

    def eval_pass(split):
        return lambda: FT.evaluate(trainer, split, eval_batch, device, num_labels,
                                   model.problem_type)

    # the two paths must feed the model the same batches (same seeds: twin generators)
    a = train.collate([train[j] for j in order[:batch]])
    dev["train"].set_epoch(order[:batch])
    b = dev["train"].batch(0, batch)
    assert all(torch.equal(x, y.cpu()) for x, y in zip(a, b)), "the two paths differ"
    for fn in (steps_item, steps_resident, eval_pass(host["dev"]), eval_pass(dev["dev"])):
        fn()
    torch.cuda.synchronize(device)
    res = {k: [] for k in ("step_item", "step_resident", "eval_item", "eval_resident")}
    for _ in range(rounds):  # alternate the paths inside every round
        res["step_item"].append(sync_time(steps_item, device) / steps)
        res["step_resident"].append(sync_time(steps_resident, device) / steps)
        res["eval_item"].append(sync_time(eval_pass(host["dev"]), device))
        res["eval_resident"].append(sync_time(eval_pass(dev["dev"]), device))
    out = {k: summary(v) for k, v in res.items()}
    for what in ("step", "eval"):
        it, rs = out[f"{what}_item"], out[f"{what}_resident"]
        spread = max(it["max_ms"] - it["min_ms"], rs["max_ms"] - rs["min_ms"])
        out[f"{what}_resident_wins"] = bool(it["median_ms"] - rs["median_ms"] > spread)
    out["eval_rows"] = len(host["dev"])
    out["device_bytes"] = {k: v.device_bytes() for k, v in dev.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=16, help="training steps per timed window")
    ap.add_argument("--cases", default=None, help="comma-separated indices into CASES")
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("genome_windows_ab.py measures on a GPU; none is visible")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    cases = CASES if a.cases is None else [CASES[int(i)] for i in a.cases.split(",")]
    result = {"rounds": a.rounds, "steps": a.steps, "chromosome_bp": CHROM_BP,
              "genome_bp": GENOME_BP, "device": torch.cuda.get_device_name(device), "cases": {}}
    with tempfile.TemporaryDirectory() as root:
        write_data(root)
        for name, experiment, window, batch, eval_batch in cases:
            result["cases"][name] = measure(experiment, window, batch, eval_batch, root, a.rounds,
                                            a.steps, device)
            print(f"# {name}: done", flush=True)
    fmt = lambda s: f"{s['median_ms']:.2f} ({s['min_ms']:.2f}-{s['max_ms']:.2f})"
    print("| case | quantity | item-by-item ms | resident ms | resident wins by more than the spread |")
    print("|---|---|---|---|---|")
    for name, r in result["cases"].items():
        print(f"| {name} | training step | {fmt(r['step_item'])} | {fmt(r['step_resident'])} | "
              f"{'yes' if r['step_resident_wins'] else 'no'} |")
        print(f"| {name} | evaluation pass ({r['eval_rows']} rows) | {fmt(r['eval_item'])} | "
              f"{fmt(r['eval_resident'])} | {'yes' if r['eval_resident_wins'] else 'no'} |")
    for name, r in result["cases"].items():
        print(f"# {name}: device bytes per split {r['device_bytes']}")
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
