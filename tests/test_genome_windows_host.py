"""The whole-genome fine-tuning datasets on the host: finetune_data.SpeciesWindows and
ChromatinProfile against the reference's own outputs (tests/golden/species_golden.json,
chromatin_golden.json; make_species_golden.py / make_chromatin_golden.py), SPECIES_SPLITS against
the reference's table, the genome store, the error cases, the per-class metrics, the new symbol,
and the dry runs of the three experiments."""
import ctypes
import io
import json
import os
import random
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import genome_fixtures as GF  # noqa: E402


@pytest.fixture(scope="module")
def species(tmp_path_factory):
    root = tmp_path_factory.mktemp("species")
    return GF.species_folder(root), str(root)


@pytest.fixture(scope="module")
def chromatin(tmp_path_factory):
    root = tmp_path_factory.mktemp("chromatin")
    gold, fa = GF.chromatin_folder(root)
    return gold, str(root), fa


def _species_ds(gold, root, case, **kw):
    from dna_amd.finetune_data import SpeciesWindows
    args = dict(add_eos=case["add_eos"], remove_tail_ends=case["remove_tail_ends"],
                cutoff_train=gold["cutoff_train"], cutoff_test=gold["cutoff_test"],
                rng=random.Random(case["seed"]))
    args.update(kw)
    return SpeciesWindows(gold["species"], root, case["split"], gold["max_length"],
                          gold["total_size"], **args)


# ------------------------------------------------------------------------------------ species
def test_species_splits_equal_the_reference_table():
    from dna_amd.finetune_data import SPECIES_SPLITS
    assert SPECIES_SPLITS == GF.load("species_splits.json")


@pytest.mark.parametrize("case", range(5))
def test_species_windows_equal_the_reference(species, case):
    gold, root = species
    case = gold["cases"][case]
    ds = _species_ds(gold, root, case)
    assert len(ds) == gold["total_size"] and ds.num_labels == 2
    items = [ds[i] for i in range(len(ds))]
    ids = torch.stack([x for x, _ in items])
    assert ids.dtype == torch.int64 and ids.tolist() == case["ids"]
    assert [int(t) for _, t in items] == case["targets"]
    assert ids.shape[1] == gold["max_length"] - (0 if case["add_eos"] else 1) == ds.row_length
    # the reference's quirk is in the fixture: partly and wholly N-padded rows
    assert 0 in case["bases_read"] and any(0 < n < gold["max_length"] for n in case["bases_read"])
    # rows(k): the same draws as k accesses, as (src, n, left) into the split's own store
    ds2 = _species_ds(gold, root, case)
    src, n, left, tgt = ds2.rows(len(ds2))
    assert n.tolist() == case["bases_read"] and tgt.tolist() == case["targets"]
    assert (left + n == gold["max_length"]).all()
    assert int(src.min()) >= 0 and int((src + n).max()) <= ds2.store.n_bases
    assert ds2.rng.random() == ds.rng.random()  # both consumed three draws per item


def test_species_one_hot_ids_and_weights(species):
    gold, root = species
    from dna_amd.finetune_data import remap_ids
    case = gold["cases"][2]
    ds = _species_ds(gold, root, case, use_tokenizer=False)
    got = torch.stack([ds[i][0] for i in range(8)])
    assert torch.equal(got, remap_ids(torch.tensor(case["ids"][:8])))
    lut, fill, eos, tail = ds.window_spec()
    assert (fill, eos, tail) == (4, -1, -1) and lut[ord("A")] == 0 and lut[ord("N")] == 4
    by_bp = _species_ds(gold, root, case, species_weights="weighted_by_bp",
                        chromosome_weights="weighted_by_bp")
    assert sum(by_bp.species_weights) == pytest.approx(1.0)
    lens = [by_bp.store.length(f"mouse/chr{c}") for c in by_bp.chromosomes["mouse"]]
    assert by_bp.chromosome_weights["mouse"] == [x / sum(lens) for x in lens]
    only = _species_ds(gold, root, case, species_weights=[0, 1])
    assert {int(only[i][1]) for i in range(16)} == {1}
    with pytest.raises(ValueError, match="species_weights"):
        _species_ds(gold, root, case, species_weights=[1])
    with pytest.raises(ValueError, match="chromosome_weights"):
        _species_ds(gold, root, case, chromosome_weights={"mouse": [1], "hippo": "uniform"})


def test_species_split_sizes_follow_the_reference():
    from dna_amd.finetune_data import species_split_sizes
    assert species_split_sizes(1000, 1024) == {"train": (1000, 1024), "valid": (1000, 1024),
                                               "test": (1000, 1024)}
    assert species_split_sizes(10, 256, 512, 1024) == {"train": (40, 256), "valid": (20, 512),
                                                       "test": (10, 1024)}


def test_species_errors(species):
    gold, root = species
    case = gold["cases"][0]
    with pytest.raises(NotImplementedError, match="next_token_pred"):
        _species_ds(gold, root, case, task="next_token_pred")
    # a chromosome shorter than max_length: randint(0, len - max_length) raises, as the
    # reference's does
    from dna_amd.finetune_data import SpeciesWindows
    short = SpeciesWindows(gold["species"], root, "train", 500, 4, rng=random.Random(0))
    with pytest.raises(ValueError):
        short[0]
    with pytest.raises(ValueError, match="zebra"):
        SpeciesWindows(["zebra"], root, "train", 64, 4)
    with pytest.raises(FileNotFoundError):
        SpeciesWindows(["human"], root, "train", 64, 4)


# ------------------------------------------------------------------------------------ genome
def test_genome_store_reads_plain_and_gz_alike(tmp_path):
    from dna_amd.genome import GenomeStore
    gold, fa = GF.chromatin_folder(tmp_path)
    _, gz = GF.chromatin_folder(tmp_path, gz=True)
    before = sorted(os.listdir(tmp_path))
    a, b = GenomeStore.from_fasta(fa), GenomeStore.from_fasta(gz)
    assert sorted(os.listdir(tmp_path)) == before  # a .gz is read in memory: nothing is written
    assert a.names == b.names == ["chr1", "chr2", "chr3"]
    assert [a.length(k) for k in a.names] == [1300, 1777, 2500]
    assert all(a.record(k) == b.record(k) for k in a.names)
    assert a.offsets.tolist() == [0, 1300, 3077, 5577] and a.n_bases == 5577
    assert a.bases.dtype == torch.uint8 and a.bases.numel() == 5578
    assert bytes(a.bases[1300:1310].tolist()) == a.record("chr2")[:10]
    sub = a.subset(["chr3", "chr1"])
    assert sub.names == ["chr3", "chr1"] and sub.offset("chr1") == 2500
    up = GenomeStore.from_fasta(fa, upper=True)
    assert up.record("chr1") == a.record("chr1").upper() != a.record("chr1")
    assert a.to("cpu").bases is not None and a.to("cpu").names == a.names


# ------------------------------------------------------------------------------------ chromatin
@pytest.mark.parametrize("max_length", [512, 1000, 1024, 1100])
def test_chromatin_profile_equals_the_reference(chromatin, max_length):
    from dna_amd.finetune_data import ChromatinProfile
    gold, root, fa = chromatin
    want = gold["cases"][str(max_length)]
    ds = ChromatinProfile(root, fa, gold["version"], gold["split"], max_length)
    assert len(ds) == 9 and ds.num_labels == 7 and ds.row_length == max_length + 1
    for i in range(len(ds)):
        ids, y = ds[i]
        assert ids.dtype == torch.int64 and ids.tolist() == want["ids"][i], i
        assert y.dtype == torch.float32 and y.tolist() == [float(v) for v in want["targets"][i]]
        name, start, n, left, right = ds._windows[i]
        w = want["windows"][i]
        assert (left, right) == (len(w) - len(w.lstrip(".")), len(w) - len(w.rstrip("."))), i
        assert ds.store.record(name)[start:start + n].decode() == w.strip("."), i
    src, n, left, right = ds.rows()
    assert (left + n + right == max_length).all()
    kinds = {(bool(l), bool(r)) for l, r in zip(left.tolist(), right.tolist())}
    if max_length > 1000:
        assert {(True, False), (False, True), (False, False)} <= kinds
    lut, fill, eos, tail = ds.window_spec()
    assert fill == 6 and lut[ord("a")] == lut[ord("A")] == 7 and lut[ord(".")] == 6
    assert (eos, tail) == ((-1, 1) if max_length > 1000 else (1, -1))


def test_chromatin_one_hot_ids_and_shared_genome(chromatin):
    from dna_amd.finetune_data import ChromatinProfile, remap_ids
    from dna_amd.genome import GenomeStore
    gold, root, fa = chromatin
    genome = GenomeStore.from_fasta(fa)
    ds = ChromatinProfile(root, None, "hg38", "val", 1024, use_tokenizer=False, genome=genome)
    want = remap_ids(torch.tensor(gold["cases"]["1024"]["ids"]))
    assert torch.equal(torch.stack([ds[i][0] for i in range(len(ds))]), want)
    assert ds.store.names == ["chr1", "chr2", "chr3"]
    assert ds.window_spec()[1:] == (4, -1, 4)


def test_chromatin_errors(chromatin, tmp_path):
    from dna_amd.finetune_data import ChromatinProfile
    gold, root, fa = chromatin
    with pytest.raises(ValueError, match="(?i)liftover"):  # the tables are hg38's
        ChromatinProfile(root, fa, "hg19", "train", 1024)
    with pytest.raises(ValueError, match="(?i)liftover"):
        ChromatinProfile(None, fa, "hg19", "train", 1024, coords_target_path=os.path.join(
            root, "train_hg38_coords_targets.csv"))
    with pytest.raises(ValueError, match="even"):
        ChromatinProfile(root, fa, "hg38", "train", 1023)
    with pytest.raises(ValueError, match="hg19"):
        ChromatinProfile(root, fa, "hg37", "train", 1024)
    with pytest.raises(FileNotFoundError):
        ChromatinProfile(str(tmp_path), fa, "hg38", "train", 1024)


# ------------------------------------------------------------------------------------ metrics
def test_per_class_lists_come_only_when_asked():
    from dna_amd.tasks import ConfusionMatrix
    target = torch.tensor([0, 0, 0, 1, 1, 2])
    pred = torch.tensor([0, 0, 1, 1, 1, 1])
    plain = ConfusionMatrix(4)
    plain.update(pred, target)
    assert sorted(plain.compute()) == ["accuracy", "f1_macro", "mcc"]
    m = ConfusionMatrix(4, per_class=["recall_per_class", "accuracy_per_class",
                                      "precision_per_class", "accuracy"])
    m.update(pred, target)
    out = m.compute()
    assert out["recall_per_class"] == out["accuracy_per_class"] == [2 / 3, 1.0, 0.0, 0.0]
    assert out["precision_per_class"] == [1.0, 0.5, 0.0, 0.0]  # empty classes report 0
    support = [3, 2, 1, 0]
    assert out["accuracy"] == pytest.approx(
        sum(r * s for r, s in zip(out["recall_per_class"], support)) / 6)
    assert {k: out[k] for k in plain.compute()} == plain.compute()


# ------------------------------------------------------------------------------------ ABI
def test_genome_windows_symbol_is_declared_exported_and_counted():
    from dna_amd import _native as N
    L = N.lib()
    assert "dna_genome_windows" in N.declared_symbols() and "dna_genome_windows" in N._SIGS
    assert hasattr(L, "dna_genome_windows")
    assert L.dna_abi_version() == 1 and L.dna_abi_revision() >= 8
    P = ctypes.c_void_p(4096)
    ok = dict(bases=P, n_bases=10, src=P, n=P, left=P, lut=P, B=2, L=5, fill_id=4, eos_id=-1,
              ids=P, stream=None)
    for bad in (dict(bases=None), dict(src=None), dict(n=None), dict(left=None), dict(lut=None),
                dict(ids=None), dict(n_bases=-1), dict(B=-1), dict(L=0), dict(fill_id=-1),
                dict(src=ctypes.c_void_p(4100)), dict(n=ctypes.c_void_p(4098))):
        assert L.dna_genome_windows(*dict(ok, **bad).values()) == 1, bad
        assert b"dna_genome_windows" in L.dna_last_error(), bad
    assert L.dna_genome_windows(*dict(ok, B=0).values()) == 0  # an empty batch launches nothing


# ------------------------------------------------------------------------------------ dry runs
def _dry(*overrides):
    import finetune as FT
    from dna_amd.compose import compose
    cfg = compose(os.path.join(ROOT, "configs"), "config", list(overrides))
    out = io.StringIO()
    FT.finetune(cfg, dry_run=True, out=out)
    return json.loads(out.getvalue())


@pytest.mark.parametrize("experiment,model", [("hyena/species_hyena", "dna_embedding"),
                                              ("caduceus/species_caduceus", "caduceus_cls")])
def test_species_experiments_compose(experiment, model):
    info = _dry(f"experiment={experiment}")
    assert info["model"] == model and info["dataset"] == "species"
    assert info["num_labels"] == info["d_output"] == 2 and info["max_length"] == 1024
    assert info["problem_type"] == "single_label_classification"
    assert info["monitor"] == "val/accuracy" and info["scheduler_name"] == "cosine_warmup_timm"
    # 1,000 windows an epoch at batch 8 for 100 epochs, 1 % warmup, floor 0.1 lr
    assert info["scheduler"]["t_initial"] == 12500
    assert info["scheduler"]["warmup_t"] == pytest.approx(125.0)
    assert info["scheduler"]["lr_min"] == pytest.approx(0.1 * info["optimizer"]["lr"])
    three = _dry(f"experiment={experiment}", "dataset.species=[human,mouse,pig]",
                 "dataset.max_length=256", "dataset.max_length_test=1024", "dataset.total_size=10")
    assert three["num_labels"] == 3 and three["scheduler"]["t_initial"] == 5 * 100
    with pytest.raises(NotImplementedError, match="next_token_pred"):
        _dry(f"experiment={experiment}", "dataset.task=next_token_pred")


def test_chromatin_experiment_composes(chromatin):
    info = _dry("experiment=hyena/chromatin_profile_hyena")
    assert info["model"] == "dna_embedding" and info["dataset"] == "chromatin_profile"
    assert info["num_labels"] == info["d_output"] == 919 and info["max_length"] == 1024
    assert info["problem_type"] == "multi_label_classification" and info["loss_scale"] == 1.0
    assert info["monitor"] == "val/roc" and info["mode"] == "max"
    assert info["scheduler"]["t_initial"] == 2200 * 100 and info["optimizer"]["lr"] == 6e-4
    _, root, fa = chromatin  # with the tables at hand, d_output is their number of y_ columns
    seven = _dry("experiment=hyena/chromatin_profile_hyena", f"dataset.data_path={root}",
                 f"dataset.ref_genome_path={fa}")
    assert seven["num_labels"] == seven["d_output"] == 7
    for flag in ("true", "false"):
        assert _dry("experiment=hyena/chromatin_profile_hyena",
                    f"dataset.resident={flag}")["resident"] is (flag == "true")
