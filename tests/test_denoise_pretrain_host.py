"""Host side of denoise_cnn masked-LM pretraining from train.py, no GPU: the constructor against
the state-dict keys recorded from the reference (tests/golden/denoise_pretrain.npz), --dry-run of
the new experiment, the `stdmlm_onehot` objective against bert_mask in the one-hot id space,
finetune.load_pretrained on a checkpoint that carries out_linear.*, and the new C-ABI entries."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

CONFIGS = os.path.join(ROOT, "configs")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _maker():
    spec = importlib.util.spec_from_file_location(
        "make_denoise_pretrain_golden", os.path.join(GOLDEN, "make_denoise_pretrain_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = _maker()
Z = np.load(os.path.join(GOLDEN, "denoise_pretrain.npz"))


# ---------------------------------------------------------------------------------- constructor
@pytest.mark.parametrize("tag", ["P", "Q"])
def test_pretrain_configuration_has_the_reference_state_dict(tag):
    from dna_amd.denoise import CNNModel
    m = CNNModel(**MK.model_kwargs(MK.CONFIGS[tag]))
    ref = [(k, tuple(s)) for k, s in json.loads(Z[f"{tag}/keys"].tobytes().decode())]
    ours = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert sorted(ours) == sorted(ref)
    V, D = 5, MK.CONFIGS[tag]["D"]
    assert ("out_linear.weight", (V, D)) in ours and ("out_linear.bias", (V,)) in ours
    assert m.pretrain and m.lm_head is m.out_linear
    assert not any(k.startswith("lm_head") for k, _ in ours)  # the property adds no key
    assert ("final_conv.0.weight" in dict(ours)) == MK.CONFIGS[tag]["final_conv"]
    m.load_state_dict(MK.denoise_state(ref), strict=True)


def test_the_other_combinations_still_raise():
    from dna_amd.denoise import CNNModel
    kw = MK.model_kwargs(MK.CONFIGS["P"])
    with pytest.raises(NotImplementedError, match="pretrain"):
        CNNModel(**dict(kw, for_representation=True))
    with pytest.raises(NotImplementedError, match="for_representation=False"):
        CNNModel(**dict(kw, pretrain=False))
    # a fine-tuning model has no lm_head and no mlm_loss
    ft = CNNModel(**dict(kw, pretrain=False, for_representation=True))
    assert not hasattr(ft, "lm_head") and "out_linear.weight" not in ft.state_dict()
    with pytest.raises(RuntimeError, match="pretrain=True"):
        ft.mlm_loss(None, None, None)


def test_forward_wants_the_tuple_and_the_gpu():
    from dna_amd.denoise import CNNModel
    m = CNNModel(**MK.model_kwargs(MK.CONFIGS["P"]))
    ids = torch.zeros(1, 16, dtype=torch.int64)
    with pytest.raises(TypeError, match=r"\(input_ids, mask\)"):
        m(ids)
    with pytest.raises(RuntimeError, match="GPU"):
        m((ids, torch.zeros(1, 16, dtype=torch.bool)))


def test_masked_lm_head_refuses_bias_with_a_complement_map():
    from dna_amd import functional as DF
    with pytest.raises(ValueError, match="no bias"):
        DF.masked_lm_head(torch.zeros(4, 16), torch.zeros(5, 8), torch.zeros(4, dtype=torch.int64),
                          complement_map=torch.arange(5), bias=torch.zeros(5))
    with pytest.raises(RuntimeError, match="GPU only"):
        DF.masked_lm_head(torch.zeros(4, 8), torch.zeros(5, 8), torch.zeros(4, dtype=torch.int64),
                          bias=torch.zeros(5))


# ------------------------------------------------------------------------------------- dry run
@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    from dna_amd.synthetic import write_hg38
    root = tmp_path_factory.mktemp("denoise_data")
    write_hg38(str(root), n_chroms=2, chrom_len=60_000, max_length=256)
    return str(root)


EXP = ["experiment=denoise/bert_hg38_denoise", "dataset.max_length=256", "dataset.batch_size=4",
       "trainer.devices=1", "dataset.num_workers=0", "wandb=null"]


def test_dry_run_bert_hg38_denoise(data_root):
    """The command line, in a process of its own: exit status 0 and the dry run's JSON line."""
    import train
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--dry-run"] + EXP,
                       capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, DATA_PATH=data_root))
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["dry_run"] and res["model"] == "denoise_cnn" and res["task"] == "bert_cross_entropy"
    assert res["scheduler_name"] == "cosine_warmup_timm" and res["param_groups"] == 1
    assert res["optimizer"]["lr"] == 1e-3 and res["optimizer"]["weight_decay"] == 0.0
    assert res["train_windows"] > 0 and res["model_params"] > 1_600_000
    assert train.MODEL_REGISTRY["denoise_cnn"] == "dna_amd.denoise.CNNModel"
    assert train.TRAINER_REGISTRY["denoise_cnn"] == "dna_amd.trainer.BlmTrainer"
    assert train.on_module_trainer("denoise_cnn")


def test_experiment_composes_with_the_fine_tuning_shapes():
    from dna_amd.compose import compose
    cfg = compose(CONFIGS, "config", ["experiment=denoise/bert_hg38_denoise"])
    m = cfg.model.to_container()
    assert m["_name_"] == "denoise_cnn" and m["pretrain"] is True and m["for_representation"] is False
    assert (m["kernel_size"], m["dilation"], m["num_conv1d"], m["d_inner"]) == (9, 4, 5, 2)
    assert m["forget"] is True and m["use_comp"] is True and m["args"]["hidden_dim"] == 128
    d = cfg.dataset
    assert (d._name_, d.tokenizer_name, d.use_tokenizer, d.objective) == \
        ("bert_hg38", "char", False, "stdmlm_onehot")
    assert d.add_eos is True and d.max_length == 1024 and d.batch_size == 128
    assert cfg.scheduler._name_ == "cosine_warmup_timm" and str(cfg.trainer.precision) == "bf16"
    # everything but the two switches is the fine-tuning experiments' model block
    for exp in ("genomic_benchmark_denoise", "deepstarr_denoise", "deepsea_denoise"):
        ft = compose(CONFIGS, "config", [f"experiment=denoise/{exp}"]).model.to_container()
        skip = ("pretrain", "for_representation", "length", "out_dim")  # no parameter shapes
        a, b = ({k: v for k, v in x.items() if k not in skip} for x in (ft, m))
        a["args"], b["args"] = (dict(x["args"], dropout=None) for x in (a, b))
        assert a == b, exp


# --------------------------------------------------------------------------------- the objective
def _n_fasta(root):
    """One chromosome with runs of N, its index and a one-window-per-row BED."""
    rng = np.random.default_rng(5)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1200)].copy()
    for s, n in ((0, 9), (100, 17), (395, 10), (700, 40)):
        seq[s:s + n] = ord("N")
    fa, bed = os.path.join(root, "n.fa"), os.path.join(root, "n.bed")
    with open(fa, "wb") as f:
        f.write(b">chr1\n")
        off = f.tell()
        for i in range(0, 1200, 60):
            f.write(seq[i:i + 60].tobytes() + b"\n")
    with open(fa + ".fai", "w") as f:
        f.write(f"chr1\t1200\t{off}\t60\t61\n")
    with open(bed, "w") as f:
        for s in range(0, 1200, 200):
            f.write(f"chr1\t{s}\t{s + 200}\ttrain\n")
    return fa, bed, seq


def _dataset(root, **kw):
    from dna_amd.hg38 import BertHG38Dataset
    from dna_amd.tokenizer import CharacterTokenizer
    fa, bed, seq = _n_fasta(root)
    tok = CharacterTokenizer(characters=["A", "C", "G", "T", "N"], model_max_length=202)
    return BertHG38Dataset("train", bed, fa, max_length=200, tokenizer=tok, tokenizer_name="char",
                           add_eos=True, **kw), seq


def test_stdmlm_onehot_is_bert_mask_in_the_one_hot_id_space(tmp_path):
    from dna_amd.hg38 import bert_mask
    ds, seq = _dataset(str(tmp_path), use_tokenizer=False, objective="stdmlm_onehot")
    code = {ord(c): i for i, c in enumerate("ACGTN")}
    n_masked = n_random = n_N = 0
    for i in range(len(ds)):
        torch.manual_seed(100 + i)
        (ids, mask, labels), target = ds[i]
        # the remapped ids: the window's bases (truncated to max_length with the end-of-sequence
        # token, as the tokenizer does), then that token's position as 4
        want = torch.tensor([code[b] for b in seq[200 * i:200 * i + 199]] + [4])
        assert torch.equal(target, want)
        torch.manual_seed(100 + i)
        e_ids, e_mask, e_labels = bert_mask(want.clone(), 4, 4, 4, special_token_ids=[])
        assert torch.equal(ids, e_ids) and torch.equal(mask, e_mask) and torch.equal(labels, e_labels)
        assert int(ids.min()) >= 0 and int(ids.max()) <= 4
        assert bool(((labels[mask] >= 0) & (labels[mask] <= 3)).all())
        assert bool((labels[~mask] == -100).all())
        assert torch.equal(labels[mask], target[mask])
        assert not bool(mask[target == 4].any()) and not bool(mask[-1])  # no N, no eos
        assert torch.equal(ids[~mask], target[~mask])
        shown = ids[mask]
        assert bool((shown[shown != target[mask]] <= 4).all())
        n_masked += int(mask.sum())
        n_random += int(((shown != 4) & (shown != target[mask])).sum())
        n_N += int((target == 4).sum())
    assert n_masked > 100 and n_random > 0 and n_N > 70  # 6 x 200 positions at 15 %
    # objective stdmlm with use_tokenizer false stays what it was: the tokenizer's ids
    old, _ = _dataset(str(tmp_path), use_tokenizer=False, objective="stdmlm")
    torch.manual_seed(100)
    (ids, mask, labels), target = old[0]
    tok = old.tokenizer
    torch.manual_seed(100)
    e = bert_mask(target.clone(), tok.mask_token_id, tok.pad_token_id, tok.vocab_size,
                  special_token_ids=tok.all_special_ids)
    assert torch.equal(ids, e[0]) and torch.equal(mask, e[1]) and int(ids.max()) > 4


def test_stdmlm_onehot_needs_the_remapped_ids(tmp_path):
    from dna_amd.hg38 import BertHG38
    with pytest.raises(ValueError, match="use_tokenizer"):
        _dataset(str(tmp_path), use_tokenizer=True, objective="stdmlm_onehot")
    with pytest.raises(ValueError, match="use_tokenizer"):
        BertHG38(tokenizer_name="char", objective="stdmlm_onehot")
    BertHG38(tokenizer_name="char", objective="stdmlm_onehot", use_tokenizer=False)


# ---------------------------------------------------------------------------------- fine-tuning
def test_load_pretrained_takes_a_masked_lm_checkpoint():
    import finetune
    from dna_amd.decoders import SequenceClassifier
    from dna_amd.denoise import CNNModel
    c = MK.CONFIGS["P"]
    torch.manual_seed(3)
    pre = CNNModel(**MK.model_kwargs(c))
    ck = {"model." + k: v.clone() for k, v in pre.state_dict().items()}  # train.py's layout
    assert "model.out_linear.weight" in ck and "model.out_linear.bias" in ck
    kw = dict(MK.model_kwargs(c), pretrain=False, for_representation=True)
    clf = SequenceClassifier(CNNModel(**kw), 2, mode="pool")
    info = finetune.load_pretrained(clf, ck)
    assert info == {"loaded": "backbone", "kept_fresh": ["decoder.0.output_transform"]}
    got = clf.model.state_dict()
    assert sorted(got) == sorted(k for k in pre.state_dict() if not k.startswith("out_linear."))
    assert all(torch.equal(v, pre.state_dict()[k]) for k, v in got.items())
    with pytest.raises(RuntimeError, match="gates.1"):  # the rest still loads strictly
        finetune.load_pretrained(clf, {k: v for k, v in ck.items() if "gates.1" not in k})


# ------------------------------------------------------------------------------------------ ABI
def test_biased_head_and_relu_abi_entries():
    """The new symbols are exported and declared; bad arguments return DNA_ERR_INVALID and set
    dna_last_error before anything touches a GPU (host buffers stand in for device memory)."""
    from dna_amd import _native as N
    L = N.lib()
    for sym in ("dna_lm_head_bias_fwd", "dna_lm_head_bias_bwd", "dna_lm_head_bias_bwd_workspace"):
        assert hasattr(L, sym) and sym in N.declared_symbols(), sym
    assert L.dna_abi_version() == 1 and L.dna_abi_revision() >= 6
    assert (N.ACT_NONE, N.ACT_GELU, N.ACT_SIGMOID, N.ACT_RELU) == (0, 1, 2, 3)
    with open(N.HEADER) as f:
        assert "DNA_ACT_RELU = 3" in f.read()
    # the bias partials: one [V] block per chunk of rows on top of dW's
    # (chunks of whole 256-row blocks, at most 256 of them: 70,000 rows -> 137 chunks of 512)
    for T, chunks in ((300, 2), (257, 2), (256, 1), (70_000, 137)):
        assert L.dna_lm_head_bias_bwd_workspace(T, 128, 5) == \
            L.dna_lm_head_bwd_workspace(T, 128, 5) + chunks * 5 * 4, T
    assert L.dna_lm_head_bias_bwd_workspace(0, 128, 5) == 0
    buf = (ctypes.c_char * ((1 << 16) + 16))()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def fwd(V=5, D=8, stride=8, h=p, lab=p, ws=p, nws=1 << 16, hdt=N.F32):
        return L.dna_lm_head_bias_fwd(h, stride, hdt, p, N.F32, p, lab, 4, D, V, 0.0, p, p, p, p,
                                      ws, nws, None)

    def bwd(V=5, D=8, stride=8, coef=p, T=4, ws=p, nws=1 << 16, dh=p, dw=p, db=p):
        return L.dna_lm_head_bias_bwd(coef, p, 8, N.F32, p, N.F32, p, p, None, 0.0, T, D, V, dh,
                                      stride, dw, db, 0, ws, nws, None)

    for call, word in ((lambda: fwd(V=0), "vocabulary"), (lambda: fwd(V=65), "vocabulary"),
                       (lambda: fwd(stride=7), "stride"), (lambda: fwd(h=None), "null"),
                       (lambda: fwd(lab=None), "null"), (lambda: fwd(D=0), "width"),
                       (lambda: fwd(hdt=N.F16), "fp32 or bf16"),
                       (lambda: fwd(ws=None), "workspace"), (lambda: fwd(nws=8), "workspace"),
                       (lambda: bwd(V=65), "vocabulary"), (lambda: bwd(stride=7), "stride"),
                       (lambda: bwd(coef=None), "null"), (lambda: bwd(T=0), "rows"),
                       # (the workspace is checked after dh's launch: no dh here)
                       (lambda: bwd(ws=None, dh=None), "workspace"),
                       # dW's partials alone (5 * 8 floats) do not hold dbias's
                       (lambda: bwd(nws=5 * 8 * 4, dh=None), "workspace"),
                       (lambda: bwd(dw=None), "dbias")):
        assert call() == 1, word  # DNA_ERR_INVALID
        assert "dna_lm_head_bias_" in N.last_error() and word in N.last_error(), \
            (word, N.last_error())
    # the one-hot layer refuses an unknown activation, and dna_dconv_fwd still refuses ReLU
    assert L.dna_onehot_conv_fwd(p, p, p, 1, 8, 64, 5, 9, 0, 4, p, None) == 1
    assert "act 4" in N.last_error()
    assert L.dna_onehot_conv_bwd(p, p, p, p, 1, 8, 64, 5, 9, 0, 4, p, p, 0, p, 1 << 16, None) == 1
    assert "act 4" in N.last_error()
    assert L.dna_dconv_fwd(p, N.F32, p, p, 1, 8, 64, 3, 1, 0, N.ACT_RELU, None, None, p, None, None,
                           None) == 1
    assert "act 3" in N.last_error()
