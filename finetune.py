#!/usr/bin/env python
"""Fine-tune DNABERT-2 for sequence classification on a GUE-layout folder (single GPU).

    python finetune.py dataset.data_dir=/data/GUE/prom/prom_300_all \\
        train.pretrained_model_path=checkpoints/last.ckpt trainer.max_epochs=3
    python finetune.py --dry-run                       # compose + build, no GPU
    python finetune.py dataset.unpad=true ...          # packed batches: no work on [PAD] rows
    python finetune.py experiment=hyena/genomic_benchmark_hyena dataset.dest_path=/data/gb
    python finetune.py experiment=caduceus/genomic_benchmark_caduceus dataset.dest_path=/data/gb

`key=value` overrides are composed by dna_amd.compose over configs/ with the experiment
dnabert2/dnabert2_gue_finetune (another one: experiment=...). The run trains with ClsTrainer
(HIP encoder + fused classification head, AdamW, linear warmup), evaluates dev and test after every
epoch (loss, accuracy, MCC, macro F1 over the pooled predictions of the split), prints one JSON
line per event, and writes the best (train.monitor / train.mode, default val/mcc max) and last
checkpoints in train.py's Lightning layout. train.pretrained_model_path takes an MLM checkpoint
written by train.py (the MLM head is dropped, pooler and classifier start from their
initialisation) or a fine-tuning checkpoint.

model._name_ picks the path: dnabert2_cls as above; dna_embedding (HyenaDNA backbone +
SequenceDecoder), caduceus_cls (CaduceusForSequenceClassification) and denoise_cnn (the gated
dilated-CNN backbone + SequenceDecoder, experiment=denoise/*, dataset.use_tokenizer=false) read a Genomic Benchmarks
folder (dataset.dest_path / dataset.dataset_name, character tokens at a fixed length), train with
SeqClsTrainer on the fused pooling head, and share the epoch loop, metrics, events and
checkpoints. The benchmarks have no validation split: val and test are both the test folder.
dataset._name_ deepstarr (task regression, loss customMSE: two targets, reports loss and
pearsonr_dev / pearsonr_hk / pearsonr_mean) and deepsea (task multilabel_classification, loss
deepsea_loss: 919 labels on the wide pooling head, reports loss, roc and roc_labels_skipped) read
their own train / val / test files:

    python finetune.py experiment=hyena/deepstarr_hyena dataset.dest_path=/data/deepstarr
    python finetune.py experiment=hyena/deepsea_hyena dataset.dest_path=/data/deepsea
    python finetune.py experiment=caduceus/deepstarr_caduceus dataset.dest_path=/data/deepstarr

dataset._name_ nucleotide_transformer reads one task of the Nucleotide Transformer benchmark
(<dest_path>/<dataset_name>/*train*.fasta and *test*.fasta, labels in the headers; val and test
are both the test file); length, labels, schedule length and the monitored metric come from the
task table (finetune_data.NT_TASKS) unless given, with the cosine_warmup_timm schedule:

    python finetune.py experiment=hyena/nt_hyena dataset.dest_path=/data/nt dataset.dataset_name=H3

dataset._name_ species (a random window of a random chromosome of a random species, classified
by species; dataset.species_dir holds <species>/chr<name>.fna) and chromatin_profile (919
chromatin features of a window centred on a coordinate of hg19 / hg38; dataset.data_path holds the
coordinates tables, dataset.ref_genome_path the genome) cut their windows out of whole genomes:

    python finetune.py experiment=hyena/species_hyena dataset.species_dir=/data/species
    python finetune.py experiment=hyena/chromatin_profile_hyena dataset.data_path=/data/chromatin \\
        dataset.ref_genome_path=/data/hg38/hg38.ml.fa

dataset.resident=true (the pooling models; every dataset above) keeps the splits on the device and
builds each batch there with one HIP kernel (dna_amd.resident), bit-identical to the item-by-item
path for the same seeds.

train.pretrained_model_path there takes an LM / masked-LM checkpoint of train.py (backbone
loaded, head fresh; dna_embedding honours train.pretrained_model_state_hook.freeze_backbone: the
backbone then gets no update and no weight decay) or one of this script's checkpoints.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from dna_amd.compose import compose  # noqa: E402

EXPERIMENT = "dnabert2/dnabert2_gue_finetune"


def _model_config(cfg, num_labels=None):
    mc = cfg.model.config.to_container()
    if mc.get("num_labels") is None:
        mc["num_labels"] = int(num_labels) if num_labels else 2
    return mc


FT_SCHEDULERS = ("linear_warmup", "cosine_warmup_timm")


def _scheduler_name(cfg):
    if "scheduler" not in cfg or cfg.scheduler is None:
        return "linear_warmup"
    return cfg.scheduler._name_


def _scheduler(cfg):
    """-> the scheduler's keyword arguments (its class: _scheduler_name). cosine_warmup_timm with
    t_initial, warmup_t or lr_min null takes them as the reference's Nucleotide Transformer
    experiments compute them: t_initial = ceil(dataset.train_len / dataset.batch_size) *
    trainer.max_epochs, warmup_t = 1 % of t_initial, lr_min = 0.1 * optimizer.lr."""
    if "scheduler" not in cfg or cfg.scheduler is None:
        return None
    if cfg.scheduler._name_ not in FT_SCHEDULERS:
        raise NotImplementedError(f"scheduler {cfg.scheduler._name_!r} (one of {FT_SCHEDULERS})")
    sched = {k: v for k, v in cfg.scheduler.to_container().items() if k != "_name_"}
    if cfg.scheduler._name_ == "cosine_warmup_timm":
        if sched.get("t_initial") is None or sched.get("warmup_t") is None:
            train_len = cfg.dataset.get("train_len")
            if train_len is None:
                raise ValueError("scheduler.t_initial / warmup_t are null: dataset.train_len (the "
                                 "number of training sequences) is needed to compute them")
            steps = -(-int(train_len) // int(cfg.dataset.get("batch_size", 32)))
            run = steps * int(cfg.trainer.get("max_epochs", 1))
            if sched.get("t_initial") is None:
                sched["t_initial"] = run
            if sched.get("warmup_t") is None:
                sched["warmup_t"] = run * 0.01
        if sched.get("lr_min") is None:
            sched["lr_min"] = 0.1 * float(cfg.optimizer.get("lr", 6e-4))
    return sched


def _nt_defaults(cfg):
    """dataset._name_ nucleotide_transformer: max_length, d_output, train_len and metric left
    null come from finetune_data.NT_TASKS by dataset.dataset_name (explicit values win), and a
    null train.monitor follows the task's metric as val/<metric>, mode max. Idempotent."""
    ds = cfg.get("dataset")
    if ds is None or ds.get("_name_") != "nucleotide_transformer":
        return
    from dna_amd.finetune_data import NT_TASKS
    keys = {"max_length": "max_length", "d_output": "classes", "train_len": "train_len",
            "metric": "metric"}
    if any(ds.get(k) is None for k in keys):
        task = NT_TASKS.get(ds.get("dataset_name"))
        if task is None:
            raise ValueError(f"dataset.dataset_name={ds.get('dataset_name')!r}: not one of the "
                             f"Nucleotide Transformer tasks {sorted(NT_TASKS)}; set "
                             "dataset.max_length, d_output, train_len and metric yourself")
        for k, src in keys.items():
            if ds.get(k) is None:
                ds[k] = task[src]
    if cfg.train.get("monitor") is None:
        cfg.train["monitor"] = f"val/{ds.metric}"
    if cfg.train.get("mode") is None:
        cfg.train["mode"] = "max"


def _metric(problem_type, num_labels, per_class=()):
    """The evaluator of a problem type: (accumulator, whether it reads the logits -- or the
    head's argmax). Single-label: accuracy, mcc, f1_macro (+ the *_per_class lists that
    task.metrics names); regression: pearsonr_dev, pearsonr_hk (the DeepSTARR targets' names)
    and pearsonr_mean; multi-label: roc, roc_labels_skipped."""
    from dna_amd.tasks import ConfusionMatrix, MultilabelAUROC, PearsonR
    if problem_type == "regression":
        names = ("dev", "hk") if num_labels == 2 else tuple(str(i) for i in range(num_labels))
        return PearsonR(names), True
    if problem_type == "multi_label_classification":
        return MultilabelAUROC(num_labels), True
    return ConfusionMatrix(num_labels, per_class), False


@torch.no_grad()
def evaluate(trainer, ds, batch_size, device, num_labels,
             problem_type="single_label_classification", unpad=False, per_class=()):
    """-> {"loss", ...the problem type's metrics (_metric)} of one split; the metric's state
    stays on the device until the split is done. unpad: packed batches (dataset.unpad). A
    resident.ResidentSplit builds its batches on the device, in the split's own order; a
    resident.ResidentWindows starts a pass of its own (a species split draws its windows then)."""
    from dna_amd.resident import RESIDENT, ResidentWindows
    metric, on_logits = _metric(problem_type, num_labels, per_class)
    total = torch.zeros((), device=device, dtype=torch.float64)
    resident = isinstance(ds, RESIDENT)
    if isinstance(ds, ResidentWindows):
        ds.set_epoch()
    for i in range(0, len(ds), batch_size):
        if resident:
            (ids, labels), packed = ds.batch(i, i + batch_size)[:2], None
        else:
            items = [ds[j] for j in range(i, min(i + batch_size, len(ds)))]
            if unpad:
                ids, labels, packed = ds.collate(items, unpad=True)
                packed = packed.to(device)
            else:
                (ids, labels), packed = ds.collate(items), None
            ids, labels = ids.to(device), labels.to(device)
        logits, loss, pred = (trainer.evaluate(ids, labels, packed=packed) if unpad
                              else trainer.evaluate(ids, labels))
        total += loss.double() * ids.shape[0]
        metric.update(logits if on_logits else pred, labels)
    out = metric.compute()
    out["loss"] = (total / max(len(ds), 1)).item()
    return out


POOL_MODELS = ("dna_embedding", "caduceus_cls", "denoise_cnn")


def _char_tokenizer(max_length, padding_side="left"):
    from dna_amd.tokenizer import CharacterTokenizer
    return CharacterTokenizer(["A", "C", "G", "T", "N"], int(max_length) + 2,
                              padding_side=padding_side)


def _pool_task(cfg, num_labels):
    """-> (problem_type, loss_scale) from task._name_ and task.loss (tasks.pool_loss)."""
    from dna_amd.tasks import pool_loss
    task = cfg.get("task")
    task = task.to_container() if task is not None else {}
    loss = task.get("loss")
    if isinstance(loss, dict):
        loss = loss.get("_name_")
    return pool_loss(task.get("_name_", "sequence_classification"), loss, num_labels)


def _pool_model(cfg, num_labels, tokenizer):
    """The model of a pooling-head experiment from cfg.model (+ cfg.decoder for dna_embedding);
    its head's problem type and loss scale from cfg.task."""
    problem, scale = _pool_task(cfg, num_labels)
    mc = {k: v for k, v in cfg.model.to_container().items() if k != "_name_"}
    if cfg.model._name_ == "dna_embedding":
        from dna_amd.decoders import SequenceClassifier
        from dna_amd.hyena_lm import DNAEmbeddingModel
        dec = cfg.get("decoder")
        dec = dec.to_container() if dec is not None else {}
        if dec.get("_name_", "sequence") != "sequence":
            raise NotImplementedError(f"decoder {dec.get('_name_')!r} (sequence only)")
        return SequenceClassifier(DNAEmbeddingModel(**mc), num_labels, mode=dec.get("mode", "pool"),
                                  use_lengths=dec.get("use_lengths", False), problem_type=problem,
                                  loss_scale=scale)
    if cfg.model._name_ == "denoise_cnn":
        from dna_amd.decoders import SequenceClassifier
        from dna_amd.denoise import CNNModel
        dec = cfg.get("decoder")
        dec = dec.to_container() if dec is not None else {}
        if dec.get("_name_", "sequence") != "sequence":
            raise NotImplementedError(f"decoder {dec.get('_name_')!r} (sequence only)")
        return SequenceClassifier(CNNModel(**mc), num_labels, mode=dec.get("mode", "pool"),
                                  use_lengths=dec.get("use_lengths", False), problem_type=problem,
                                  loss_scale=scale)
    from dna_amd.caduceus import CaduceusForSequenceClassification
    head = {k: mc.pop(k) for k in ("pooling_strategy", "conjoin_train", "conjoin_eval") if k in mc}
    config = mc.pop("config")
    if mc:
        raise TypeError(f"caduceus_cls: unknown model keys {sorted(mc)}")
    if config.get("rcps") and config.get("complement_map") is None:
        config["complement_map"] = tokenizer.complement_map()
    return CaduceusForSequenceClassification(num_labels=num_labels, problem_type=problem,
                                             loss_scale=scale, **head, **config)


def load_pretrained(model, state_dict, freeze_backbone=False):
    """train.pretrained_model_path for the pooling-head models -> what was loaded, for the log.
    A "model." prefix (train.py's and finetune.py's checkpoint layout) is stripped first. A
    dna_embedding classifier takes an LM checkpoint through hyena_lm.load_backbone (backbone
    loaded, heads fresh, freeze_backbone honoured) or one of finetune.py's own checkpoints (keys
    model.* and decoder.0.*: everything loaded, strictly). A Caduceus classifier loads whatever
    keys match: the masked-LM backbone, or a fine-tuning checkpoint with its score."""
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.trainer import strip_model_prefix
    sd = strip_model_prefix(state_dict)
    from dna_amd.denoise import CNNModel
    if isinstance(model, SequenceClassifier) and isinstance(model.model, CNNModel):
        # denoise_cnn: one of this script's checkpoints (keys model.* and decoder.0.*: everything,
        # strictly) or a same-key backbone state dict (the reference's, or train.py's masked-LM
        # checkpoint; its decoder.* and out_linear.* keys are dropped and the head stays fresh),
        # also strictly
        if freeze_backbone:
            raise NotImplementedError("freeze_backbone is built for dna_embedding only")
        if any(k.startswith("model.") for k in sd):
            model.load_state_dict(sd)
            return {"loaded": "classifier"}
        model.model.load_state_dict({k: v for k, v in sd.items()
                                     if not k.startswith(("decoder.", "out_linear."))})
        return {"loaded": "backbone", "kept_fresh": ["decoder.0.output_transform"]}
    if isinstance(model, SequenceClassifier):
        if any(k.startswith("decoder.0.") for k in sd):
            model.load_state_dict(sd)
            return {"loaded": "classifier"}
        from dna_amd.hyena_lm import load_backbone
        return {"kept_fresh": load_backbone(model.model, sd, freeze_backbone=freeze_backbone)}
    if freeze_backbone:
        raise NotImplementedError("freeze_backbone is built for dna_embedding only")
    missing, unexpected = model.load_state_dict(sd, strict=False)
    return {"missing": list(missing), "unexpected": len(unexpected)}


POOL_DATASETS = ("genomic_benchmark", "deepstarr", "deepsea", "nucleotide_transformer",
                 "species", "chromatin_profile")
GENOME_DATASETS = ("species", "chromatin_profile")  # windows cut out of whole genomes


def _genome_defaults(cfg):
    """dataset._name_ species: d_output is the number of species, and a null train_len (the
    cosine schedule's length) is the train split's size, total_size * ((max_length_test + 2) //
    max_length). chromatin_profile: a null d_output is the number of y_* columns of the train
    table when dataset.data_path is there to read, DeepSEA's 919 otherwise. Idempotent."""
    ds = cfg.get("dataset")
    if ds is None or ds.get("_name_") not in GENOME_DATASETS:
        return
    from dna_amd import finetune_data as FD
    if ds._name_ == "species":
        if ds.get("task", "species_classification") == "next_token_pred":
            raise NotImplementedError("dataset.task=next_token_pred is not built; "
                                      "species_classification only")
        ds["d_output"] = len(ds.species)
        if ds.get("train_len") is None:
            ds["train_len"] = FD.species_split_sizes(
                ds.total_size, int(ds.max_length), ds.get("max_length_val"),
                ds.get("max_length_test"))["train"][0]
    elif ds.get("d_output") is None:
        path = os.path.join(str(ds.get("data_path")),
                            f"train_{ds.get('ref_genome_version')}_coords_targets.csv")
        if ds.get("data_path") and os.path.exists(path):
            with open(path) as f:
                ds["d_output"] = sum(c.strip()[:2] == "y_" for c in f.readline().split(","))
        else:
            ds["d_output"] = FD.DEEPSEA_LABELS


def _pool_splits(ds, tok, max_length, seed=None):
    """dataset._name_ -> {"train", "dev", "test": dataset}. Genomic Benchmarks have no validation
    split (dev is the test folder); DeepSTARR and DeepSEA have their own train / val / test
    files; the Nucleotide Transformer benchmark has no validation split either. species and
    chromatin_profile cut windows out of genomes; seed: of the generator the species splits draw
    their windows from."""
    from dna_amd import finetune_data as FD
    # dataset.use_tokenizer=false (the one-hot models): ids A C G T N = 0..4 (finetune_data.remap_ids)
    kw = dict(max_length=max_length, tokenizer=tok, use_padding=ds.get("use_padding", True),
              add_eos=ds.get("add_eos", False), id_remap=not ds.get("use_tokenizer", True))
    rc = ds.get("rc_aug", False)
    name = ds.get("_name_", "genomic_benchmark")
    if name == "genomic_benchmark":
        train_ds = FD.GenomicBenchmarkFolder(ds.dest_path, ds.dataset_name, "train", rc_aug=rc, **kw)
        test_ds = FD.GenomicBenchmarkFolder(ds.dest_path, ds.dataset_name, "val",
                                            classes=train_ds.classes, **kw)
        return {"train": train_ds, "dev": test_ds, "test": test_ds}
    if name == "nucleotide_transformer":
        make = lambda split, **k: FD.NucleotideTransformerFasta(
            ds.dest_path, ds.dataset_name, split, d_output=ds.get("d_output"), **kw, **k)
        test_ds = make("val")
        return {"train": make("train", rc_aug=rc), "dev": test_ds, "test": test_ds}
    if name == "species":
        import random
        # one generator for the three splits, as the reference's share the global one
        rng = random.Random(seed)
        sizes = FD.species_split_sizes(ds.total_size, max_length, ds.get("max_length_val"),
                                       ds.get("max_length_test"))
        weights = lambda w: w.to_container() if hasattr(w, "to_container") else w
        make = lambda split: FD.SpeciesWindows(
            list(ds.species), ds.species_dir, split, sizes[split][1], sizes[split][0],
            tokenizer=tok, add_eos=ds.get("add_eos", True), rng=rng,
            species_weights=weights(ds.get("species_weights", "uniform")),
            chromosome_weights=weights(ds.get("chromosome_weights", "uniform")),
            task=ds.get("task", "species_classification"),
            remove_tail_ends=ds.get("remove_tail_ends", False),
            cutoff_train=ds.get("cutoff_train", 0.1), cutoff_test=ds.get("cutoff_test", 0.2),
            id_remap=kw["id_remap"])
        return {"train": make("train"), "dev": make("valid"), "test": make("test")}
    if name == "chromatin_profile":
        from dna_amd.genome import GenomeStore
        genome = GenomeStore.from_fasta(ds.ref_genome_path)  # read once, shared by the splits
        make = lambda split: FD.ChromatinProfile(
            ds.data_path, ds.ref_genome_path, ds.ref_genome_version, split, max_length,
            tokenizer=tok, id_remap=kw["id_remap"], genome=genome)
        return {"train": make("train"), "dev": make("val"), "test": make("test")}
    if name == "deepstarr":
        make = lambda split, **k: FD.DeepSTARRFolder(ds.dest_path, split, **kw, **k)
    else:
        make = lambda split, **k: FD.DeepSEACsv(ds.dest_path, split,
                                                max_rows=ds.get("max_rows", 40000), **kw, **k)
    return {"train": make("train", rc_aug=rc), "dev": make("val"), "test": make("test")}


def finetune_pool(cfg, dry_run=False, out=sys.stdout):
    """The dna_embedding / caduceus_cls path: a Genomic Benchmarks folder, the DeepSTARR files or
    the DeepSEA tables (dataset._name_), the head and its loss from cfg.task, SeqClsTrainer."""
    import train as T

    if T.n_devices(cfg.trainer) != 1:
        raise NotImplementedError("finetune.py: single-GPU fine-tuning only (trainer.devices=1)")
    seed = cfg.train.get("seed")
    if seed is not None:
        torch.manual_seed(int(seed))
    precision = T._precision(cfg.trainer.get("precision", "bf16"))
    ds = cfg.dataset
    if ds.get("_name_", "genomic_benchmark") not in POOL_DATASETS:
        raise ValueError(f"dataset._name_={ds.get('_name_')!r}: one of {POOL_DATASETS}")
    _nt_defaults(cfg)
    _genome_defaults(cfg)
    sched = _scheduler(cfg)
    opt = cfg.optimizer.to_container()
    resident = bool(ds.get("resident", False))
    genome = ds.get("_name_") in GENOME_DATASETS
    if resident and not ds.get("use_padding", True):
        raise ValueError("dataset.resident=true with dataset.use_padding=false: ragged items have "
                         "no fixed length, a resident split builds rectangles only")
    max_length = int(ds.get("max_length", 200))
    if ds.get("unpad", False):
        raise ValueError(f"dataset.unpad=true: model._name_={cfg.model._name_!r} has no packed "
                         "path (fixed-length character tokens); dnabert2_cls only")
    tok = _char_tokenizer(max_length, ds.get("padding_side", "left"))
    if dry_run:
        model = _pool_model(cfg, int(ds.get("d_output") or 2), tok)
        print(json.dumps({"dry_run": True, "model": cfg.model._name_,
                          "model_params": sum(p.numel() for p in model.parameters()),
                          "num_labels": model.num_labels, "problem_type": model.problem_type,
                          "loss_scale": model.loss_scale, "dataset": ds.get("_name_"),
                          "dest_path": ds.get("dest_path"),
                          "dataset_name": ds.get("dataset_name"), "max_length": max_length,
                          "d_output": ds.get("d_output"),
                          "resident": resident, "scheduler_name": _scheduler_name(cfg),
                          "monitor": cfg.train.monitor, "mode": cfg.train.mode,
                          "scheduler": sched, "optimizer": opt}), file=out)
        return None
    if ds.get("_name_") == "species" and not ds.get("species_dir"):
        raise ValueError("dataset.species_dir=<folder of <species>/chr*.fna> is required")
    if ds.get("_name_") == "chromatin_profile" and not (ds.get("data_path")
                                                        and ds.get("ref_genome_path")):
        raise ValueError("dataset.data_path=<folder of the coordinates tables> and "
                         "dataset.ref_genome_path=<the genome's FASTA> are required")
    if not genome and not ds.get("dest_path"):
        raise ValueError("dataset.dest_path=<folder holding the dataset's files> is required "
                         "(genomic_benchmark: <dataset_name>/train and /test)")
    splits = _pool_splits(ds, tok, max_length, seed=seed)
    num_labels = int(splits["train"].num_labels if genome
                     else ds.get("d_output") or splits["train"].num_labels)
    model = _pool_model(cfg, num_labels, tok)
    pre = cfg.train.get("pretrained_model_path")
    if pre:
        ck = torch.load(pre, map_location="cpu", weights_only=True)
        hook = (cfg.train.get("pretrained_model_state_hook") or {})
        info = load_pretrained(model, ck.get("state_dict", ck),
                               freeze_backbone=bool(hook.get("freeze_backbone", False)))
        print(json.dumps(dict({"event": "load_backbone", "path": pre}, **info)), file=out,
              flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    from dna_amd.trainer import SeqClsTrainer
    trainer = SeqClsTrainer(model, device, lr=float(opt.get("lr", 6e-4)),
                            weight_decay=float(opt.get("weight_decay", 0.1)),
                            betas=tuple(opt.get("betas", (0.9, 0.999))),
                            eps=float(opt.get("eps", 1e-8)),
                            max_grad_norm=cfg.trainer.get("gradient_clip_val", 1.0),
                            scheduler=sched, scheduler_name=_scheduler_name(cfg), seed=seed,
                            autocast=torch.bfloat16 if precision == "bf16" else None)
    if resident:
        # each split once (dev and test may be one dataset): bytes, offsets and targets go to the
        # device here, and _fit / evaluate take their batches from there
        from dna_amd.resident import ResidentSplit, ResidentWindows
        cls = ResidentWindows if genome else ResidentSplit
        made = {}
        for name, split in list(splits.items()):
            if id(split) not in made:
                made[id(split)] = cls.from_dataset(split, device)
            splits[name] = made[id(split)]
    return _fit(cfg, trainer, model, splits, device, out)


def finetune(cfg, dry_run=False, out=sys.stdout):
    import train as T
    from dna_amd.bert_layers import BertForSequenceClassification
    from dna_amd.finetune_data import SequenceClassificationCSV
    from dna_amd.trainer import ClsTrainer, load_backbone

    if cfg.model._name_ in POOL_MODELS:
        return finetune_pool(cfg, dry_run=dry_run, out=out)
    if cfg.model._name_ != "dnabert2_cls":
        raise ValueError(f"model._name_={cfg.model._name_!r}: finetune.py runs dnabert2_cls, "
                         + ", ".join(POOL_MODELS))
    if T.n_devices(cfg.trainer) != 1:
        raise NotImplementedError("finetune.py: single-GPU fine-tuning only (trainer.devices=1)")
    seed = cfg.train.get("seed")
    if seed is not None:
        torch.manual_seed(int(seed))
    problem = cfg.model.config.get("problem_type") or "single_label_classification"
    if problem != "single_label_classification":
        raise NotImplementedError(
            f"model.config.problem_type={problem!r}: finetune.py reads integer labels and reports "
            "accuracy / MCC / F1 from the argmax, i.e. single_label_classification; regression "
            "and multi-label heads train through ClsTrainer directly")
    if cfg.dataset.get("resident", False):
        raise ValueError("dataset.resident=true: dnabert2_cls reads BPE tokens of a GUE CSV, "
                         "padded per batch or packed (dataset.unpad); a resident split holds one "
                         "byte per character token at a fixed length, for the pooling models "
                         + ", ".join(POOL_MODELS))
    precision = T._precision(cfg.trainer.get("precision", "bf16"))
    sched = _scheduler(cfg)
    opt = cfg.optimizer.to_container()
    data_dir = cfg.dataset.get("data_dir")
    if dry_run:
        model = BertForSequenceClassification(_model_config(cfg), precision=precision)
        info = {"dry_run": True, "model": cfg.model._name_,
                "model_params": sum(p.numel() for p in model.parameters()),
                "num_labels": model.num_labels, "data_dir": data_dir,
                "monitor": cfg.train.monitor, "mode": cfg.train.mode,
                "scheduler": sched, "optimizer": opt}
        if cfg.dataset.get("unpad") is not None:  # dataset.unpad=true|false was given
            info["unpad"] = bool(cfg.dataset.get("unpad"))
        print(json.dumps(info), file=out)
        return None
    if not data_dir:
        raise ValueError("dataset.data_dir=<folder with train.csv, dev.csv, test.csv> is required")

    max_length = int(cfg.dataset.get("max_length", 128))
    splits = {s: SequenceClassificationCSV(data_dir, s, max_length) for s in ("train", "dev", "test")}
    train_ds = splits["train"]
    model = BertForSequenceClassification(_model_config(cfg, train_ds.num_labels),
                                          precision=precision)
    pre = cfg.train.get("pretrained_model_path")
    if pre:
        missing, unexpected = load_backbone(model, pre)
        print(json.dumps({"event": "load_backbone", "path": pre, "missing": missing,
                          "unexpected": len(unexpected)}), file=out, flush=True)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    trainer = ClsTrainer(model, device, lr=float(opt.get("lr", 3e-5)),
                         weight_decay=float(opt.get("weight_decay", 0.01)),
                         betas=tuple(opt.get("betas", (0.9, 0.999))), eps=float(opt.get("eps", 1e-8)),
                         max_grad_norm=cfg.trainer.get("gradient_clip_val", 1.0), scheduler=sched,
                         scheduler_name=_scheduler_name(cfg), seed=seed)
    return _fit(cfg, trainer, model, splits, device, out)


def _fit(cfg, trainer, model, splits, device, out):
    """The epoch loop shared by every model: train, evaluate dev and test after each epoch, JSON
    events, best and last checkpoints. -> the last epoch's metrics."""
    import train as T
    train_ds = splits["train"]
    ck = (cfg.get("callbacks", {}) or {}).get("model_checkpoint")
    ck = ck.to_container() if ck is not None else {}
    dirpath = ck.get("dirpath", "checkpoints/")
    best = T.BestCheckpoint(dirpath, ck.get("monitor", cfg.train.monitor),
                            ck.get("mode", cfg.train.mode), ck.get("filename"),
                            ck.get("save_top_k", 1))
    bs = int(cfg.dataset.get("batch_size", 32))
    ebs = int(cfg.dataset.get("eval_batch_size", bs))
    log_every = int(cfg.trainer.get("log_every_n_steps", 10))
    max_steps = cfg.train.get("max_steps")
    unpad = bool(cfg.dataset.get("unpad", False))  # packed batches: no kernel runs on [PAD] rows
    from dna_amd.resident import RESIDENT
    resident = isinstance(train_ds, RESIDENT)
    # the *_per_class lists are reported only where task.metrics asks for them
    per_class = [m for m in ((cfg.get("task") or {}).get("metrics") or [])
                 if str(m).endswith("_per_class")]
    gen = torch.Generator().manual_seed(int(cfg.train.get("seed") or 0))
    print(json.dumps({"event": "start", "train": len(train_ds), "dev": len(splits["dev"]),
                      "test": len(splits["test"]), "num_labels": model.num_labels,
                      "batch_size": bs}), file=out, flush=True)
    metrics = {}
    for epoch in range(int(cfg.trainer.get("max_epochs", 1))):
        order = (torch.randperm(len(train_ds), generator=gen) if cfg.dataset.get("shuffle", True)
                 else torch.arange(len(train_ds)))
        if resident:
            train_ds.set_epoch(order)  # one upload; the rc_aug flags are drawn here, in order
        order = order.tolist()
        for i in range(0, len(order), bs):
            if resident:
                loss = trainer.step(*train_ds.batch(i, i + bs)[:2])
            elif unpad:
                items = [train_ds[j] for j in order[i:i + bs]]
                ids, labels, packed = train_ds.collate(items, unpad=True)
                loss = trainer.step(ids.to(device, non_blocking=True),
                                    labels.to(device, non_blocking=True),
                                    packed=packed.to(device, non_blocking=True))
            else:
                items = [train_ds[j] for j in order[i:i + bs]]
                ids, labels = train_ds.collate(items)
                loss = trainer.step(ids.to(device, non_blocking=True),
                                    labels.to(device, non_blocking=True))
            if trainer.global_step % log_every == 0:
                print(json.dumps({"event": "train", "epoch": epoch, "step": trainer.global_step,
                                  "trainer/loss": loss.item(), "lr": trainer.opt.param_groups[0]["lr"]}),
                      file=out, flush=True)
            if max_steps and trainer.global_step >= int(max_steps):
                break
        metrics = {}
        for name, split in (("val", "dev"), ("test", "test")):
            for k, v in evaluate(trainer, splits[split], ebs, device, model.num_labels,
                                 getattr(model, "problem_type", None)
                                 or "single_label_classification", unpad=unpad,
                                 per_class=per_class).items():
                metrics[f"{name}/{k}"] = v
        print(json.dumps(dict({"event": "eval", "epoch": epoch, "step": trainer.global_step},
                              **metrics)), file=out, flush=True)
        value = metrics.get(best.monitor)
        if best.enabled and value is not None and best.improves(value):
            best.score = value
            T.save_checkpoint(best.path, trainer, epoch + 1, metrics=metrics, best=best)
        if ck.get("save_last", True):
            T.save_checkpoint(os.path.join(dirpath, "last.ckpt"), trainer, epoch + 1,
                              metrics=metrics, best=best if best.enabled else None)
        if max_steps and trainer.global_step >= int(max_steps):
            break
    return metrics


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config-dir", default=os.environ.get("DNA_CONFIG_DIR",
                                                           os.path.join(ROOT, "configs")))
    ap.add_argument("--config-name", default="config")
    ap.add_argument("--dry-run", action="store_true", help="compose + build, no training")
    ap.add_argument("--print-config", action="store_true")
    ap.add_argument("overrides", nargs="*")
    a = ap.parse_args(argv)
    overrides = list(a.overrides)
    if not any(o.startswith("experiment=") for o in overrides):
        overrides.insert(0, "experiment=" + EXPERIMENT)
    cfg = compose(a.config_dir, a.config_name, overrides)
    _nt_defaults(cfg)
    _genome_defaults(cfg)
    if a.print_config or a.dry_run:
        print(json.dumps(cfg.to_container(skip_errors=True), indent=1, default=str))
    return finetune(cfg, dry_run=a.dry_run)


if __name__ == "__main__":
    main()
