"""The Nucleotide Transformer benchmark on the host: the FASTA loader, the task table, the three
experiments' --dry-run, the cosine schedule of the fine-tuning trainers, dataset.resident's
refusals. No GPU."""
import io
import json
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXPERIMENTS = ["hyena/nt_hyena", "caduceus/nt_caduceus", "denoise/nt_denoise"]


def _write(path, records, width=None):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for key, seq in records:
            f.write(f">{key}\n")
            if width:
                for i in range(0, len(seq), width):
                    f.write(seq[i:i + width] + "\n")
            else:
                f.write(seq + "\n")


RECORDS = [("seq_0|0", "ACGTACGTACGTAC"), ("seq_1|1", "TTTTGGGGCCCCAAAANN"), ("chr2:5-9 label 1 ", "ACG"),
           ("seq_3|0", "GGGGGGGGGGGGGGGGGGGGGGGGG")]


def _folder(tmp_path, name="toy"):
    d = tmp_path / name
    _write(str(d / f"{name}_train.fasta"), RECORDS, width=5)  # wrapped lines
    _write(str(d / f"{name}_test.fasta"), RECORDS[:2])
    return d


# ------------------------------------------------------------------------------------ loader
def test_loader_reads_wrapped_records_and_header_labels(tmp_path):
    from dna_amd.finetune_data import NucleotideTransformerFasta
    _folder(tmp_path)
    ds = NucleotideTransformerFasta(tmp_path, "toy", "train", 12, d_output=2)
    assert len(ds) == 4 and ds.all_seqs == [s for _, s in RECORDS]
    assert ds.all_labels == [0, 1, 1, 0] and ds.num_labels == 2
    ids, label = ds[2]
    assert ids.tolist() == [4] * 9 + [7, 8, 9] and label.dtype == torch.int64 and int(label) == 1
    assert [(s, int(t)) for s, t in ds.pairs()] == [(s, l) for (_, s), l in
                                                    zip(RECORDS, [0, 1, 1, 0])]
    # tokenisation goes through _CharItems like the other loaders: eos, mask, the one-hot ids
    ds = NucleotideTransformerFasta(tmp_path, "toy", "train", 6, add_eos=True, return_mask=True,
                                    use_tokenizer=False)
    ids, _, mask = ds[2]
    assert ids.tolist() == [4, 4, 0, 1, 2, 4] and mask.tolist() == [False, False, True, True, True, True]


def test_val_reads_the_test_file(tmp_path):
    from dna_amd.finetune_data import NucleotideTransformerFasta
    _folder(tmp_path)
    val = NucleotideTransformerFasta(tmp_path, "toy", "val", 12)
    test = NucleotideTransformerFasta(tmp_path, "toy", "test", 12)
    assert val.path == test.path and val.path.endswith("toy_test.fasta") and len(val) == 2


def test_loader_errors(tmp_path):
    from dna_amd.finetune_data import NucleotideTransformerFasta as NT
    with pytest.raises(FileNotFoundError, match=r"not downloaded here.*<dest_path>/toy/\*train\*\.fasta"):
        NT(tmp_path, "toy", "train", 12)
    d = _folder(tmp_path)
    with pytest.raises(ValueError, match="label 1, but d_output is 1"):
        NT(tmp_path, "toy", "train", 12, d_output=1)
    _write(str(d / "other_train.fasta"), RECORDS)
    with pytest.raises(ValueError, match="exactly one"):
        NT(tmp_path, "toy", "train", 12)
    os.remove(d / "other_train.fasta")
    os.remove(d / "toy_test.fasta")
    with pytest.raises(FileNotFoundError, match="no \\*.fasta file named after the split 'test'"):
        NT(tmp_path, "toy", "val", 12)
    _write(str(d / "toy_test.fasta"), RECORDS + RECORDS[:1])
    with pytest.raises(ValueError, match="duplicate header 'seq_0\\|0'"):
        NT(tmp_path, "toy", "test", 12)


def test_split_is_matched_in_the_file_name_only(tmp_path):
    """A parent folder named like a split must not make every file match (the reference tests the
    whole path)."""
    from dna_amd.finetune_data import NucleotideTransformerFasta
    root = tmp_path / "train_data"
    _folder(root)
    assert NucleotideTransformerFasta(root, "toy", "test", 12).path.endswith("toy_test.fasta")
    assert NucleotideTransformerFasta(root, "toy", "train", 12).path.endswith("toy_train.fasta")


# ------------------------------------------------------------------------------------ task table
def test_task_table_is_the_golden_one():
    from dna_amd.finetune_data import NT_TASKS
    with open(os.path.join(ROOT, "tests", "golden", "nt_tasks.json")) as f:
        golden = json.load(f)
    assert len(golden) == 18 and NT_TASKS == golden


# ------------------------------------------------------------------------------------ dry run
def _dry_run(*overrides):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--dry-run", *overrides],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("experiment", EXPERIMENTS)
def test_dry_run_takes_the_task_from_the_table(experiment):
    from dna_amd.finetune_data import NT_TASKS
    info = _dry_run(f"experiment={experiment}", "dataset.dataset_name=H3")
    assert info["dry_run"] and info["dataset"] == "nucleotide_transformer"
    assert (info["num_labels"], info["max_length"], info["monitor"], info["mode"]) == \
        (2, 500, "val/mcc", "max")
    assert info["problem_type"] == "single_label_classification"  # task masked_multiclass
    # dataset.resident is echoed as the experiment sets it (on where the step gains)
    assert info["resident"] is (experiment != "caduceus/nt_caduceus")
    assert info["scheduler_name"] == "cosine_warmup_timm"
    run = math.ceil(NT_TASKS["H3"]["train_len"] / 128) * 20
    assert info["scheduler"]["t_initial"] == run == 2120
    assert info["scheduler"]["warmup_t"] == pytest.approx(0.01 * run)
    assert info["scheduler"]["lr_min"] == pytest.approx(0.1 * 1e-3)
    assert info["optimizer"]["lr"] == 1e-3 and info["optimizer"]["weight_decay"] == 0.1


@pytest.mark.parametrize("task,labels,length,monitor", [
    ("promoter_tata", 2, 300, "val/f1_macro"), ("enhancer_types", 3, 200, "val/mcc"),
    ("splice_sites_donor", 2, 600, "val/f1_macro")])
def test_dry_run_per_task(task, labels, length, monitor):
    """In process (one interpreter start less per case): what --dry-run prints last."""
    import finetune as FT
    from dna_amd.compose import compose
    from dna_amd.finetune_data import NT_TASKS
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  ["experiment=hyena/nt_hyena", f"dataset.dataset_name={task}",
                   "dataset.resident=true"])
    out = io.StringIO()
    FT.finetune(cfg, dry_run=True, out=out)
    info = json.loads(out.getvalue())
    assert (info["num_labels"], info["max_length"], info["monitor"]) == (labels, length, monitor)
    assert info["resident"] is True
    run = math.ceil(NT_TASKS[task]["train_len"] / 128) * 20
    assert info["scheduler"]["t_initial"] == run
    assert info["scheduler"]["warmup_t"] == pytest.approx(0.01 * run)
    assert info["scheduler"]["lr_min"] == pytest.approx(1e-4)


def test_explicit_values_win_over_the_table():
    import finetune as FT
    from dna_amd.compose import compose
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  ["experiment=denoise/nt_denoise", "dataset.dataset_name=H3",
                   "dataset.max_length=40", "dataset.train_len=64", "dataset.batch_size=16",
                   "trainer.max_epochs=1", "scheduler.lr_min=5e-4", "train.monitor=val/accuracy"])
    out = io.StringIO()
    FT.finetune(cfg, dry_run=True, out=out)
    info = json.loads(out.getvalue())
    assert info["max_length"] == 40 and info["monitor"] == "val/accuracy"
    assert info["scheduler"]["t_initial"] == 4 and info["scheduler"]["lr_min"] == 5e-4
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  ["experiment=denoise/nt_denoise", "dataset.dataset_name=no_such_task"])
    with pytest.raises(ValueError, match="no_such_task"):
        FT.finetune(cfg, dry_run=True, out=io.StringIO())


# ------------------------------------------------------------------------------------ schedule
class _Opt:
    def __init__(self, lrs):
        self.param_groups = [{"lr": lr} for lr in lrs]


def test_cosine_schedule_through_the_trainers_constructor_path():
    from dna_amd.optim import LinearLRSchedulerWarmup, TimmCosineLRScheduler
    from dna_amd.trainer import _ClsSteps
    kw = dict(t_in_epochs=False, t_initial=2120, warmup_t=21.2, warmup_lr_init=1e-6, lr_min=1e-4)
    a, b = _Opt([1e-3, 2e-4]), _Opt([1e-3, 2e-4])
    got, want = _ClsSteps._make_sched(a, kw, "cosine_warmup_timm"), TimmCosineLRScheduler(b, **kw)
    assert isinstance(got, TimmCosineLRScheduler)
    peak = 0.0
    for _ in range(2200):
        assert [g["lr"] for g in a.param_groups] == [g["lr"] for g in b.param_groups]
        peak = max(peak, a.param_groups[0]["lr"])
        got.step()
        want.step()
    assert peak <= 1e-3 and a.param_groups[0]["lr"] == 1e-4  # never over the base lr; the floor
    assert isinstance(_ClsSteps._make_sched(_Opt([1e-3]), kw), LinearLRSchedulerWarmup)
    assert _ClsSteps._make_sched(_Opt([1e-3]), None, "cosine_warmup_timm") is None
    with pytest.raises(NotImplementedError, match="cycle"):  # the same refusals
        _ClsSteps._make_sched(_Opt([1e-3]), dict(kw, cycle_limit=2), "cosine_warmup_timm")


def test_linear_warmup_experiments_compose_as_before():
    import finetune as FT
    from dna_amd.compose import compose
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  ["experiment=hyena/genomic_benchmark_hyena"])
    assert FT._scheduler_name(cfg) == "linear_warmup"
    assert FT._scheduler(cfg) == {"t_in_epochs": False, "t_initial": 15630, "warmup_t": 156,
                                  "warmup_lr_init": 1e-6, "lr_min": 6e-5}
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  ["experiment=hyena/genomic_benchmark_hyena", "scheduler._name_=plateau"])
    with pytest.raises(NotImplementedError, match="plateau"):
        FT._scheduler(cfg)


# ------------------------------------------------------------------------------------ resident
def test_resident_is_refused_where_it_cannot_work():
    import finetune as FT
    from dna_amd.compose import compose
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  ["experiment=dnabert2/dnabert2_gue_finetune", "dataset.resident=true"])
    with pytest.raises(ValueError, match="BPE"):
        FT.finetune(cfg, dry_run=True, out=io.StringIO())
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  ["experiment=hyena/nt_hyena", "dataset.resident=true",
                   "dataset.use_padding=false"])
    with pytest.raises(ValueError, match="ragged"):
        FT.finetune(cfg, dry_run=True, out=io.StringIO())


@pytest.mark.parametrize("experiment", ["hyena/genomic_benchmark_hyena", "hyena/deepstarr_hyena",
                                        "hyena/deepsea_hyena", "hyena/nt_hyena"])
def test_resident_is_accepted_for_every_pooling_dataset(experiment):
    import finetune as FT
    from dna_amd.compose import compose
    for flag in ("true", "false"):
        cfg = compose(os.path.join(ROOT, "configs"), "config",
                      [f"experiment={experiment}", f"dataset.resident={flag}"])
        out = io.StringIO()
        FT.finetune(cfg, dry_run=True, out=out)
        assert json.loads(out.getvalue())["resident"] is (flag == "true")


def test_unknown_dataset_name_still_raises():
    import finetune as FT
    from dna_amd.compose import compose
    cfg = compose(os.path.join(ROOT, "configs"), "config",
                  ["experiment=hyena/nt_hyena", "dataset._name_=nucleotide_transformers"])
    with pytest.raises(ValueError, match="one of"):
        FT.finetune(cfg, dry_run=True, out=io.StringIO())


def test_resident_split_refuses_ragged_items_without_a_device(tmp_path):
    from dna_amd.finetune_data import NucleotideTransformerFasta
    from dna_amd.resident import ResidentSplit, complement_table
    _folder(tmp_path)
    ds = NucleotideTransformerFasta(tmp_path, "toy", "train", 12, use_padding=False)
    with pytest.raises(ValueError, match="ragged"):
        ResidentSplit.from_dataset(ds, "cuda")
    from dna_amd.finetune_data import string_reverse_complement
    text = "".join(chr(i) for i in range(256))
    assert bytes(complement_table()[::-1]) == string_reverse_complement(text).encode("latin-1")


def test_new_symbol_is_declared_exported_and_counted():
    from dna_amd import _native as N
    L = N.lib()
    assert "dna_char_batch" in N.declared_symbols() and "dna_char_batch" in N._SIGS
    assert hasattr(L, "dna_char_batch")
    assert L.dna_abi_version() == 1 and L.dna_abi_revision() >= 7
    import ctypes
    P = ctypes.c_void_p(4096)
    ok = dict(bases=P, n_bases=10, offsets=P, n_seqs=2, idx=P, rc=None, lut=P, comp=P, B=2, L=5,
              pad_left=1, pad_id=4, eos_id=-1, ids=P, mask=None, stream=None)
    for bad in (dict(bases=None), dict(offsets=None), dict(idx=None), dict(lut=None),
                dict(comp=None), dict(ids=None), dict(n_seqs=0), dict(n_bases=-1), dict(B=-1),
                dict(L=0), dict(pad_id=-1), dict(idx=ctypes.c_void_p(4100))):
        assert L.dna_char_batch(*dict(ok, **bad).values()) == 1, bad
        assert b"dna_char_batch" in L.dna_last_error(), bad
    assert L.dna_char_batch(*dict(ok, B=0).values()) == 0  # an empty batch launches nothing
