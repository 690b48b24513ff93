"""Host side of HyenaDNA (blm) pretraining from train.py, no GPU: the cosine schedule's closed-form
points, the optimizer grouping rule and the grouped flat layout, --dry-run of the two new
experiments (and of the reference's own, when its configs are present), the new C-ABI entries."""
import ctypes
import io
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.test_train_cli import REF_CONFIGS  # the reference's configs/ tree, when it is mounted

CONFIGS = os.path.join(ROOT, "configs")


class _Opt:
    def __init__(self, lrs):
        self.param_groups = [dict(lr=lr, initial_lr=lr) for lr in lrs]


# ------------------------------------------------------------------------------------ schedule
def test_cosine_schedule_closed_form_points():
    from dna_amd.optim import TimmCosineLRScheduler
    base, lr_min, w0, wt, T = 6e-4, 6e-5, 1e-6, 10, 200
    opt = _Opt([base])
    s = TimmCosineLRScheduler(opt, t_initial=T, warmup_t=wt, warmup_lr_init=w0, lr_min=lr_min)
    assert s.get_last_lr() == [w0]                                      # t = 0
    seen = {0: w0}
    for t in range(1, T + 5):
        s.step()
        seen[t] = opt.param_groups[0]["lr"]
    assert seen[5] == pytest.approx(w0 + 5 * (base - w0) / wt, rel=1e-12)  # inside the warmup
    cos = lambda t: lr_min + 0.5 * (base - lr_min) * (1 + math.cos(math.pi * t / T))
    assert seen[wt] == pytest.approx(cos(wt), rel=1e-12)                # t = warmup_t
    assert seen[T // 2] == pytest.approx(lr_min + 0.5 * (base - lr_min), rel=1e-12)  # the midpoint
    assert seen[T - 1] == pytest.approx(cos(T - 1), rel=1e-12)
    assert seen[T] == lr_min and seen[T + 4] == lr_min                  # t >= t_initial
    assert all(seen[t + 1] <= seen[t] for t in range(wt, T + 3))        # monotone after warmup


def test_cosine_schedule_groups_scale_from_their_own_base_and_round_trip():
    from dna_amd.optim import TimmCosineLRScheduler
    kw = dict(t_initial=100, warmup_t=4, warmup_lr_init=1e-6, lr_min=1e-5)
    opt = _Opt([6e-4, 1e-3])
    s = TimmCosineLRScheduler(opt, **kw)
    for _ in range(2):
        s.step()
    assert s.get_last_lr() == pytest.approx([1e-6 + 2 * (6e-4 - 1e-6) / 4,
                                             1e-6 + 2 * (1e-3 - 1e-6) / 4], rel=1e-12)
    for _ in range(48):
        s.step()
    assert s.get_last_lr() == pytest.approx([1e-5 + 0.5 * (6e-4 - 1e-5), 1e-5 + 0.5 * (1e-3 - 1e-5)],
                                            rel=1e-12)
    sd = s.state_dict()
    assert sd["_last_epoch"] == 50 and sd["base_values"] == [6e-4, 1e-3]
    opt2 = _Opt([6e-4, 1e-3])
    s2 = TimmCosineLRScheduler(opt2, **kw)
    s2.load_state_dict(sd)
    assert s2.get_last_lr() == s.get_last_lr()
    s.step()
    s2.step()
    assert s2.get_last_lr() == s.get_last_lr()
    with pytest.raises(NotImplementedError):
        TimmCosineLRScheduler(_Opt([1e-3]), t_initial=10, cycle_limit=2)


# ------------------------------------------------------------------------------------ grouping
def _tiny_blm(wd=0.0, lr=3e-4, **kw):
    from dna_amd.hyena_lm import BertLMHeadModel
    layer = {"_name_": "hyena", "emb_dim": 5, "filter_order": 16, "short_filter_order": 3,
             "l_max": 64, "modulate": True, "w": 10, "lr": lr, "wd": wd, "lr_pos_emb": 0.0,
             "bidirectional": True}
    return BertLMHeadModel(d_model=64, n_layer=2, d_inner=256, vocab_size=12,
                           pad_vocab_size_multiple=8, embed_dropout=0.0, residual_in_fp32=True,
                           layer=layer, **kw)


def test_grouping_rule_on_a_cpu_built_model():
    """Parameters without `_optim` are group 0; the implicit filter's linears carry
    {"lr", "weight_decay": 0.0} and form one more group per distinct dict; torch indices run over
    the normal parameters first, then each group, in registration order."""
    from dna_amd.flat import ALIGN, FlatParams
    from dna_amd.optim import ParamGroups
    m = _tiny_blm()
    pg = ParamGroups(m)
    names = {id(p): n for n, p in m.named_parameters()}
    tagged = {n for n, p in m.named_parameters() if hasattr(p, "_optim")}
    assert tagged and all("filter_fn" in n for n in tagged)
    assert any("implicit_filter" in n for n in tagged)
    assert len(pg) == 1 + len({frozenset(p._optim.items()) for p in m.parameters()
                               if hasattr(p, "_optim")})
    for p in m.parameters():
        assert (pg(p) == 0) == (names[id(p)] not in tagged)
        if pg(p):
            assert pg.overrides[pg(p)] == {k: v for k, v in p._optim.items() if v is not None}
    filt = next(p for n, p in m.named_parameters() if "implicit_filter" in n)
    assert pg.overrides[pg(filt)] == {"lr": 3e-4, "weight_decay": 0.0}
    assert "backbone.embeddings.word_embeddings.weight" not in tagged  # tied weight: decayed
    # registration order inside every group
    reg = [id(p) for p in m.parameters()]
    for gi in range(len(pg)):
        idx = [reg.index(id(p)) for p in pg.members(gi)]
        assert idx == sorted(idx) and idx
    assert sum(len(pg.members(gi)) for gi in range(len(pg))) == len(reg)
    # the grouped flat layout: every group one contiguous ALIGN-aligned extent, in group order
    flat = FlatParams(m, "cpu", shadow_dtype=None, group_of=pg)
    ext = flat.group_extents
    assert sorted(ext) == list(range(len(pg))) and ext[0][0] == 0
    assert ext[len(pg) - 1][1] == flat.numel
    for gi in range(len(pg)):
        s, e = ext[gi]
        assert s % ALIGN == 0 and e % ALIGN == 0 and s < e
        if gi:
            assert ext[gi - 1][1] == s
        for p in pg.members(gi):
            o, n, _ = flat.slice_of(p)
            assert s <= o and o + n <= e


def test_flat_layout_without_the_opt_in_is_unchanged():
    from dna_amd.flat import ALIGN, FlatParams
    m = _tiny_blm()
    flat = FlatParams(m, "cpu", shadow_dtype=None)
    assert flat.group_extents is None
    assert [id(p) for p in flat.params] == [id(p) for p in list(m.parameters())[::-1]]
    off = 0
    for p, (o, n, shape) in zip(flat.params, flat.slices):
        assert (o, n, shape) == (off, p.numel(), tuple(p.shape))
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    assert flat.numel == off


# ------------------------------------------------------------------------------------ dry runs
@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    from dna_amd.synthetic import write_hg38
    root = tmp_path_factory.mktemp("blm_data")
    write_hg38(str(root), n_chroms=2, chrom_len=60_000, max_length=256)
    z = np.load(os.path.join(ROOT, "tests", "golden", "corpus_golden.npz"))
    d = root / "dnabert2"
    d.mkdir()
    for split in ("train", "dev"):
        (d / f"{split}.txt").write_text("\n".join(str(s) for s in z["lines"]) + "\n")
    return str(root)


def _dry(config_dir, overrides, data_root, monkeypatch):
    import train
    from dna_amd.compose import compose
    monkeypatch.setenv("DATA_PATH", data_root)
    cfg = compose(config_dir, "config", overrides + ["trainer.devices=1", "dataset.num_workers=0",
                                                     "wandb=null",
                                                     "trainer.resume_from_checkpoint=null"])
    buf = io.StringIO()
    train.train(cfg, dry_run=True, out=buf)
    return cfg, json.loads(buf.getvalue())


HG38 = ["experiment=hyena/bert_hg38_hyena", "dataset.max_length=256", "dataset.batch_size=4"]


def test_dry_run_bert_hg38_hyena(data_root, monkeypatch):
    cfg, res = _dry(CONFIGS, HG38, data_root, monkeypatch)
    assert res["model"] == "blm" and res["task"] == "bert_cross_entropy"
    assert res["scheduler_name"] == "cosine_warmup_timm"
    assert res["scheduler"]["warmup_lr_init"] == 1e-6 and res["scheduler"]["lr_min"] == 6e-5
    assert res["param_groups"] == 2
    assert res["train_windows"] > 0 and res["model_params"] > 1_000_000
    assert cfg.model.layer.l_max == 256 and cfg.optimizer.weight_decay == 0.1
    assert cfg.dataset.tokenizer_name == "char"


def test_dry_run_hyena_dnabert2_pretrain(data_root, monkeypatch):
    cfg, res = _dry(CONFIGS, ["experiment=hyena/hyena_dnabert2_pretrain",
                              f"dataset.text_file={data_root}/dnabert2"], data_root, monkeypatch)
    assert res["model"] == "blm" and res["scheduler_name"] == "cosine_warmup_timm"
    assert res["scheduler"]["t_initial"] == 500000 and res["scheduler"]["warmup_t"] == 30000
    assert res["param_groups"] == 2 and res["train_windows"] > 0
    assert cfg.model.vocab_size == 4096 and cfg.model.n_layer == 8 and cfg.dataset.max_length == 128


def test_scheduler_group_file_composes(data_root, monkeypatch):
    from dna_amd.compose import compose
    cfg = compose(CONFIGS, "config", ["experiment=dnabert2/dnabert2_hg38_pretrain",
                                      "scheduler=cosine_warmup_timm"])
    assert cfg.train.interval == "step"


def test_unknown_scheduler_and_model_raise(data_root, monkeypatch):
    with pytest.raises(NotImplementedError, match="plateau"):
        _dry(CONFIGS, HG38 + ["scheduler._name_=plateau"], data_root, monkeypatch)
    # the cosine schedule belongs to the blm trainer; dnabert2 keeps linear_warmup only
    with pytest.raises(NotImplementedError, match="cosine_warmup_timm"):
        _dry(CONFIGS, ["experiment=dnabert2/dnabert2_hg38_pretrain",
                       "model.config.num_hidden_layers=1", "dataset.batch_size=4",
                       "scheduler._name_=cosine_warmup_timm"], data_root, monkeypatch)
    with pytest.raises(KeyError, match="not in train.py's registry"):
        _dry(CONFIGS, HG38 + ["model._name_=lm"], data_root, monkeypatch)
    # keys LMBackbone refuses keep raising
    with pytest.raises(NotImplementedError, match="fused_mlp"):
        _dry(CONFIGS, HG38 + ["model.fused_mlp=true"], data_root, monkeypatch)


@pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="reference configs not mounted")
def test_reference_blm_config_composes_and_dry_runs(data_root, monkeypatch):
    """The reference's own experiment=hg38/bert_hg38_hyena (+ its defaults tree) composes through
    dna_amd.compose and builds the same run: blm from cfg.model's keys, cosine_warmup_timm, the
    filter group. Its precision 16 runs as bf16 here (a warning)."""
    with pytest.warns(UserWarning, match="bf16"):
        cfg, res = _dry(REF_CONFIGS, ["experiment=hg38/bert_hg38_hyena", "dataset.max_length=256",
                                      "dataset.batch_size=4"], data_root, monkeypatch)
    assert cfg.hydra_choices["scheduler"] == ["cosine_warmup_timm"]
    assert res["model"] == "blm" and res["scheduler_name"] == "cosine_warmup_timm"
    assert res["param_groups"] == 2 and res["task"] == "bert_cross_entropy"
    assert cfg.model.d_inner == 1024 and cfg.model.layer.l_max == 256
    assert res["scheduler"]["lr_min"] == pytest.approx(6e-5)


# ----------------------------------------------------------------------------------------- ABI
def test_lm_head_abi_entries():
    """The new symbols are exported; the additions are counted by dna_abi_revision (the version
    stays 1: every earlier entry point is as it was). Bad arguments return DNA_ERR_INVALID and set
    dna_last_error before anything touches a GPU (host buffers stand in for device memory)."""
    from dna_amd import _native as N
    L = N.lib()
    for sym in ("dna_lm_head_fwd", "dna_lm_head_bwd", "dna_lm_head_fwd_workspace",
                "dna_lm_head_bwd_workspace", "dna_abi_revision"):
        assert hasattr(L, sym) and sym in N.declared_symbols(), sym
    assert L.dna_abi_version() == 1 and L.dna_abi_revision() >= 1
    assert L.dna_lm_head_fwd_workspace(0) == 0 and L.dna_lm_head_fwd_workspace(64) == 16
    assert L.dna_lm_head_fwd_workspace(65) == 32
    assert L.dna_lm_head_bwd_workspace(300, 256, 16) == 2 * 16 * 256 * 4
    assert L.dna_lm_head_bwd_workspace(0, 256, 16) == 0
    buf = (ctypes.c_char * (1 << 16))()
    p = ctypes.addressof(buf)

    def fwd(V=16, D=8, stride=8, h=p, lab=p, ws=p, nws=1 << 16, hdt=N.F32):
        return L.dna_lm_head_fwd(h, stride, hdt, p, N.F32, lab, 4, D, V, 0.0, p, p, p, p, ws, nws,
                                 None)

    def bwd(V=16, D=8, stride=8, coef=p, T=4):
        return L.dna_lm_head_bwd(coef, p, 8, N.F32, p, N.F32, p, p, None, 0.0, T, D, V, p, stride, p,
                                 0, p, 1 << 16, None)

    for call, word in ((lambda: fwd(V=0), "vocabulary"), (lambda: fwd(V=65), "vocabulary"),
                       (lambda: fwd(stride=7), "stride"), (lambda: fwd(h=None), "null"),
                       (lambda: fwd(lab=None), "null"), (lambda: fwd(D=0), "width"),
                       (lambda: fwd(hdt=N.F16), "fp32 or bf16"),
                       (lambda: fwd(ws=None), "workspace"), (lambda: fwd(nws=8), "workspace"),
                       (lambda: bwd(V=0), "vocabulary"), (lambda: bwd(V=65), "vocabulary"),
                       (lambda: bwd(stride=7), "stride"), (lambda: bwd(coef=None), "null"),
                       (lambda: bwd(T=0), "rows")):
        assert call() == 1, word  # DNA_ERR_INVALID
        assert word in N.last_error(), (word, N.last_error())


def test_masked_lm_head_has_no_cpu_fallback():
    from dna_amd import functional as DF
    with pytest.raises(RuntimeError, match="GPU only"):
        DF.masked_lm_head(torch.zeros(4, 8), torch.zeros(5, 8), torch.zeros(4, dtype=torch.int64))
    m = _tiny_blm()
    from dna_amd.hyena_lm import BlmIndex
    mask = torch.zeros(2, 64, dtype=torch.bool)
    mask[:, ::7] = True
    target = torch.randint(7, 11, (2, 64))
    idx = BlmIndex.build(mask, target, 16)
    assert idx.labels.shape == (128,) and int((idx.labels >= 0).sum()) == int(mask.sum())
    assert torch.equal(idx.labels[idx.flat_masked], idx.target)
    assert (idx.labels[~mask.reshape(-1)] == -100).all()
    with pytest.raises(ValueError, match="targets must lie in"):
        BlmIndex.build(mask, target + 10, 16)
    assert callable(m.mlm_loss)
