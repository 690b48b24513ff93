"""CPU: the host side of fine-tuning the pooling-head classifiers -- the Genomic Benchmarks folder
dataset, finetune.py's dry runs of the two new experiments, the options that are not built, and
the no-CPU-fallback error of the head."""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEQS = {"train": {"positive": ["ACGTACGTAC", "TTGCA"], "negative": ["GGGGCCCCAAAATTTTACGT", "N"]},
        "test": {"negative": ["CATG"], "positive": ["AACC", "GT"]}}


def _write(tmp_path, name="toy"):
    for split, classes in SEQS.items():
        for cls, seqs in classes.items():
            d = tmp_path / name / split / cls
            d.mkdir(parents=True)
            for i, s in enumerate(seqs):
                (d / f"{i}.txt").write_text(s)
    return str(tmp_path)


def test_genomic_benchmark_folder(tmp_path):
    from dna_amd.finetune_data import GenomicBenchmarkFolder, string_reverse_complement
    from dna_amd.tokenizer import CharacterTokenizer
    dest = _write(tmp_path)
    tok = CharacterTokenizer(["A", "C", "G", "T", "N"], 14)
    ds = GenomicBenchmarkFolder(dest, "toy", "train", max_length=12, tokenizer=tok)
    # classes by sorted folder name, whatever order they were created in
    assert ds.classes == ["negative", "positive"] and ds.num_labels == 2 and len(ds) == 4
    assert ds.all_labels == [0, 0, 1, 1]
    rows = [ds[i] for i in range(4)]
    for (ids, label), seq in zip(rows, SEQS["train"]["negative"] + SEQS["train"]["positive"]):
        raw = tok.encode_raw(seq)[:12]  # truncated to max_length
        assert ids.dtype == torch.int64 and ids.shape == (12,)
        assert ids[12 - len(raw):].tolist() == raw  # left padding
        assert bool((ids[: 12 - len(raw)] == tok.pad_token_id).all())
    assert len(SEQS["train"]["negative"][0]) > 12  # truncation was exercised
    ids, labels = ds.collate(rows)
    assert ids.shape == (4, 12) and labels.tolist() == [0, 0, 1, 1]
    # val reads the test folder
    val = GenomicBenchmarkFolder(dest, "toy", "val", max_length=12, tokenizer=tok)
    test = GenomicBenchmarkFolder(dest, "toy", "test", max_length=12, tokenizer=tok)
    assert val.all_seqs == test.all_seqs == ["CATG", "AACC", "GT"] and val.all_labels == [0, 1, 1]
    # mask and eos
    dm = GenomicBenchmarkFolder(dest, "toy", "test", max_length=8, tokenizer=tok, return_mask=True,
                                add_eos=True)
    ids, label, mask = dm[0]
    assert ids.tolist() == [4, 4, 4] + tok.encode_raw("CATG") + [tok.sep_token_id]
    assert mask.tolist() == [False] * 3 + [True] * 5 and mask.dtype == torch.bool
    ids, labels, masks = dm.collate([dm[0], dm[2]])
    assert ids.shape == masks.shape == (2, 8) and masks.sum(-1).tolist() == [5, 3]
    # rc_aug with a seeded generator: the draws of random.Random(0) decide which items flip
    aug = GenomicBenchmarkFolder(dest, "toy", "train", max_length=12, tokenizer=tok, rc_aug=True,
                                 rng=random.Random(0))
    draws = random.Random(0)
    flipped = 0
    for i in (2, 3, 2, 3, 2, 3):
        seq = ds.all_seqs[i]
        want = string_reverse_complement(seq) if draws.random() < 0.5 else seq
        flipped += want != seq
        raw = tok.encode_raw(want)
        assert aug[i][0][12 - len(raw):].tolist() == raw
    assert 0 < flipped < 6
    assert string_reverse_complement("AACGTNx") == "xNACGTT"
    # nothing is downloaded: a missing folder says where the files belong
    with pytest.raises(FileNotFoundError, match=r"not downloaded.*<dest_path>/nope/train"):
        GenomicBenchmarkFolder(dest, "nope", "train", max_length=12)


def test_split_with_other_class_folders_is_refused(tmp_path):
    from dna_amd.finetune_data import GenomicBenchmarkFolder
    dest = _write(tmp_path)
    train = GenomicBenchmarkFolder(dest, "toy", "train", max_length=12)
    GenomicBenchmarkFolder(dest, "toy", "val", max_length=12, classes=train.classes)
    (tmp_path / "toy" / "test" / "negative" / "0.txt").unlink()
    (tmp_path / "toy" / "test" / "negative").rmdir()
    with pytest.raises(ValueError, match="differ"):
        GenomicBenchmarkFolder(dest, "toy", "val", max_length=12, classes=train.classes)


def test_load_pretrained_takes_lm_and_finetuning_checkpoints():
    """finetune.py's own checkpoints (train.py's "model." prefix in front of model.* and
    decoder.0.*) load back whole; an LM checkpoint goes through load_backbone."""
    sys.path.insert(0, ROOT)
    from finetune import load_pretrained
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.hyena_lm import BertLMHeadModel, DNAEmbeddingModel
    layer = {"_name_": "hyena", "emb_dim": 5, "filter_order": 16, "short_filter_order": 3,
             "l_max": 66, "modulate": True, "w": 10, "lr_pos_emb": 0.0}
    kw = dict(d_model=32, n_layer=1, d_inner=64, vocab_size=12, pad_vocab_size_multiple=8,
              layer=layer)
    torch.manual_seed(1)
    src = SequenceClassifier(DNAEmbeddingModel(**kw), 3)
    with torch.no_grad():
        for q in src.parameters():
            q.add_(torch.randn_like(q) * 0.05)
    ckpt = {"model." + k: v.clone() for k, v in src.state_dict().items()}
    assert "model.model.backbone.ln_f.weight" in ckpt
    assert "model.decoder.0.output_transform.weight" in ckpt
    dst = SequenceClassifier(DNAEmbeddingModel(**kw), 3)
    assert load_pretrained(dst, ckpt) == {"loaded": "classifier"}
    for (n, a), (_, b) in zip(sorted(dst.state_dict().items()), sorted(src.state_dict().items())):
        assert torch.equal(a, b), n
    lm = BertLMHeadModel(**kw)
    dst2 = SequenceClassifier(DNAEmbeddingModel(**kw), 3)
    fresh = dst2.decoder[0].output_transform.weight.detach().clone()
    info = load_pretrained(dst2, {"model." + k: v for k, v in lm.state_dict().items()},
                           freeze_backbone=True)
    assert info == {"kept_fresh": ["lm_head.weight"]}
    assert torch.equal(dst2.model.backbone.ln_f.weight, lm.backbone.ln_f.weight)
    assert torch.equal(dst2.decoder[0].output_transform.weight, fresh)
    assert not any(q.requires_grad for q in dst2.model.parameters())
    assert all(q.requires_grad for q in dst2.decoder.parameters())


def _dry_run(*overrides):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "finetune.py"), "--dry-run", *overrides],
                       capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("experiment,name,params", [
    ("hyena/genomic_benchmark_hyena", "dna_embedding", (400_000, 500_000)),
    ("caduceus/genomic_benchmark_caduceus", "caduceus_cls", (1_900_000, 2_000_000))])
def test_finetune_dry_run_of_the_pooling_experiments(experiment, name, params):
    out, last = _dry_run("experiment=" + experiment, "dataset.d_output=3")
    assert last["dry_run"] is True and last["model"] == name and last["num_labels"] == 3
    assert params[0] < last["model_params"] < params[1]
    assert last["scheduler"]["warmup_lr_init"] == 1e-6 and last["optimizer"]["_name_"] == "adamw"
    cfg = json.loads(out[: out.rindex('{"dry_run"')])
    assert cfg["scheduler"]["_name_"] == "linear_warmup"
    assert cfg["dataset"]["_name_"] == "genomic_benchmark" and cfg["dataset"]["max_length"] == 200


def test_default_dry_run_is_unchanged():
    _, last = _dry_run("model.config.num_hidden_layers=1")
    assert sorted(last) == sorted(["dry_run", "model", "model_params", "num_labels", "data_dir",
                                   "monitor", "mode", "scheduler", "optimizer"])
    assert last["model"] == "dnabert2_cls" and last["num_labels"] == 2
    assert last["monitor"] == "val/mcc" and last["scheduler"]["warmup_t"] == 50


def test_unsupported_options_say_so():
    from dna_amd.caduceus import CaduceusForSequenceClassification
    from dna_amd.decoders import SequenceDecoder
    d = SequenceDecoder(16, 2, l_output=0, mode="pool")
    assert sorted(d.state_dict()) == ["output_transform.bias", "output_transform.weight"]
    for kw, word in ((dict(mode="sum"), "sum"), (dict(mode="ragged"), "ragged"),
                     (dict(l_output=4), "l_output"), (dict(l_output=None), "l_output"),
                     (dict(d_output=None), "d_output")):
        args = dict(d_model=16, d_output=2, l_output=0, mode="pool")
        args.update(kw)
        with pytest.raises(NotImplementedError, match=word):
            SequenceDecoder(**args)
    with pytest.raises(NotImplementedError, match="max"):
        CaduceusForSequenceClassification(pooling_strategy="max", d_model=16, n_layer=1,
                                          vocab_size=12)
    with pytest.raises(NotImplementedError):
        CaduceusForSequenceClassification(pooling_strategy="median", d_model=16, n_layer=1,
                                          vocab_size=12)


def test_decoder_windows():
    from dna_amd.decoders import SequenceDecoder
    x = torch.zeros(3, 10, 16)
    mask = torch.tensor([[1] * 10, [1] * 4 + [0] * 6, [0] * 10])
    win = lambda **kw: SequenceDecoder(16, 2, l_output=0, **kw)
    lst = lambda t: None if t is None else t.tolist()
    assert win(mode="pool").window(x) == (None, None)
    s, c = win(mode="pool").window(x, mask=mask)
    assert s is None and c.dtype == torch.int32 and c.tolist() == [10, 4, 0]
    s, c = win(mode="pool", use_lengths=True).window(x, lengths=[3, 10, 1])
    assert s is None and c.tolist() == [3, 10, 1]
    assert [lst(t) for t in win(mode="first").window(x)] == [None, [1, 1, 1]]
    assert [lst(t) for t in win(mode="last").window(x)] == [[9, 9, 9], [1, 1, 1]]
    assert [lst(t) for t in win(mode="last", use_lengths=True).window(x, lengths=[3, 10, 1])] == \
        [[2, 9, 0], [1, 1, 1]]
    with pytest.raises(ValueError, match="lengths"):
        win(mode="pool", use_lengths=True).window(x)


def test_pool_head_has_no_cpu_fallback():
    from dna_amd import functional as DF
    from dna_amd.decoders import SequenceDecoder
    x, w = torch.zeros(2, 6, 8), torch.zeros(3, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        DF.pool_head(x, w)
    with pytest.raises(RuntimeError, match="GPU only"):
        DF.PoolHead.apply(x, None, w, None, None, None, False, False, False, None, 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        SequenceDecoder(8, 3, l_output=0, mode="pool")(x)
